"""The fit and the fitted warp under the conditions of tests/test_gpu_concurrency.py: two streams of the library in flight at once (section A:
the scratch block one call frees on a stream is handed to a call on another while the first is still queued), and eight host threads inside
libzignal_hip.so at once, each on its own stream (section B). The harness (Op, handover, rotation, run_threads, Case) is that module's,
unchanged; this one adds ops and cases, after tests/test_gpu_concurrency_features.py.

  fit_matches_<kind>_<scalar>     transform_fit.hip launch_fit: the ScratchBlock that holds the gathered from / to points (capacity 65536 for
                                  similarity and projective: 2 MiB in f64) -> zg_transform_fit_matches_host
  fit_matches_warp_lanczos        the same block, then geom.hip's warp_fitted with the Lanczos table every thread and stream shares
                                  (device_lanczos_lut's per-device table behind its mutex) -> the host fit and zg_warp with its m32
Every expected value is computed serially before any concurrent work starts; every comparison is of bytes."""
import numpy as np
import pytest

torch = pytest.importorskip("torch")
import zignal_amd as zg  # noqa: E402
from zignal_amd import _lib as L  # noqa: E402
from zignal_amd import transform as TF  # noqa: E402
from tests import transform_cases as K  # noqa: E402
from tests.test_gpu_concurrency import Op, _op_case, handover, rotation, run_threads  # noqa: E402

pytestmark = pytest.mark.gpu
KP, MATCH = zg.KEYPOINT_DTYPE, zg.MATCH_DTYPE
NAMES = {TF.SIMILARITY: "similarity", TF.AFFINE: "affine", TF.PROJECTIVE: "projective"}
ROWS, COLS = 97, 131


def _bytes(a):
    return np.ascontiguousarray(a).view(np.uint8).reshape(-1)


def _lists(kind, n, seed):
    """Keypoints and a match list of n entries whose points follow a map of the kind, another for every seed."""
    rng = np.random.default_rng(6100 + 17 * seed + kind)
    nq, nt = n + 9, n + 21
    q, t = np.zeros(nq, KP), np.zeros(nt, KP)
    q["x"], q["y"] = rng.uniform(0, COLS, nq).astype(np.float32), rng.uniform(0, ROWS, nq).astype(np.float32)
    t["x"], t["y"] = rng.uniform(0, COLS, nt).astype(np.float32), rng.uniform(0, ROWS, nt).astype(np.float32)
    m = np.zeros(n, MATCH)
    m["query_idx"], m["train_idx"] = rng.permutation(nq)[:n], rng.permutation(nt)[:n]
    f = np.stack([q["x"][m["query_idx"]], q["y"][m["query_idx"]]], 1).astype(np.float64)
    if kind == TF.PROJECTIVE:
        mapped = K._apply_h(np.array([[0.97, 0.04, 2.0], [-0.03, 1.02, -1.5], [1e-4, -1e-4, 1.0]]) + rng.uniform(-0.01, 0.01, (3, 3)) * [[1, 1, 50], [1, 1, 50], [0, 0, 0]], f)
    else:
        a = np.deg2rad(rng.uniform(-8, 8))
        mapped = f @ (rng.uniform(0.95, 1.05) * np.array([[np.cos(a), -np.sin(a)], [np.sin(a), np.cos(a)]])).T + rng.uniform(-4, 4, 2)
    mapped = mapped + rng.normal(0, 0.3, mapped.shape)
    t["x"][m["train_idx"]], t["y"][m["train_idx"]] = mapped[:, 0].astype(np.float32), mapped[:, 1].astype(np.float32)
    return [_bytes(q).copy(), _bytes(t).copy(), _bytes(m).copy(), np.array([n - 2], np.int32)]  # the count word: two entries fewer than the list holds


def _host_record(kind, scalar, h):
    r = TF.fit_matches_host(kind, scalar, h[0], h[1], h[2], count=int(h[3][0]))
    assert r["status"] == L.FIT_OK, r
    return r


def _fit_op(kind, scalar, n, capacity):
    """capacity: what the call is told the list may hold (the scratch block is sized by it); the tensor holds n entries and the count says n - 2."""
    def call(ins, outs):
        TF.fit_matches_into(kind, scalar, ins[0], ins[1], ins[2], outs[0], count=ins[3], capacity=capacity)

    def alloc(ins):
        return [torch.zeros(128, dtype=torch.uint8, device="cuda")]

    def make(seed):
        h = _lists(kind, n, seed)
        pad = np.zeros(capacity * MATCH.itemsize, np.uint8)
        pad[:h[2].size] = h[2]
        return [h[0], h[1], pad, h[3]]
    return Op(f"fit_matches_{NAMES[kind]}_{'f32' if scalar == L.SCALAR_F32 else 'f64'}", make, call,
              lambda h: [np.frombuffer(_host_record(kind, scalar, h).tobytes(), np.uint8)], alloc)


class _M32:
    def __init__(self, r):
        self.kind, self.m = int(r["kind"]), np.array(r["m32"])

    def coefficients(self):
        return self.m if self.kind == TF.PROJECTIVE else self.m[:6]


def _warp_op(kind, n, capacity):
    """fit from matches, then warp_fitted with Lanczos of a frame that rides along as an input. want() needs the device for zg_warp with the
    host fit's matrix: it runs serially, before the concurrent part."""
    def make(seed):
        h = _lists(kind, n, seed)
        pad = np.zeros(capacity * MATCH.itemsize, np.uint8)
        pad[:h[2].size] = h[2]
        frame = np.random.default_rng(6900 + seed).integers(0, 256, (ROWS, COLS, 4), dtype=np.uint8)
        return [h[0], h[1], pad, h[3], frame]

    def call(ins, outs):
        TF.fit_matches_into(kind, L.SCALAR_F64, ins[0], ins[1], ins[2], outs[0], count=ins[3], capacity=capacity)
        TF.warp_fitted(zg.Image(ins[4]), outs[0], zg.Image(outs[1]), zg.Interpolation.lanczos)

    def alloc(ins):
        return [torch.zeros(128, dtype=torch.uint8, device="cuda"), torch.zeros((ROWS, COLS, 4), dtype=torch.uint8, device="cuda")]

    def want(h):
        r = _host_record(kind, L.SCALAR_F64, h)
        src = zg.Image(torch.from_numpy(h[4]).cuda())
        out = src.warp(_M32(r), (ROWS, COLS), zg.Interpolation.lanczos).to_numpy()
        torch.cuda.synchronize()
        return [np.frombuffer(r.tobytes(), np.uint8), out]
    return Op(f"fit_matches_warp_lanczos_{NAMES[kind]}", make, call, want, alloc)


def transform_ops(small=False):
    n = 70 if small else 300
    big = 4096 if small else L.FIT_MAX_POINTS  # f64 at 65536: a 2 MiB block
    ops = [_fit_op(TF.SIMILARITY, L.SCALAR_F64, n, big), _fit_op(TF.PROJECTIVE, L.SCALAR_F64, n, big), _fit_op(TF.AFFINE, L.SCALAR_F32, n, L.FIT_MAX_POINTS_AFFINE),
           _warp_op(TF.SIMILARITY, n, big), _warp_op(TF.PROJECTIVE, n, big)]
    return {op.name: op for op in ops}


A_NAMES = ("fit_matches_similarity_f64", "fit_matches_projective_f64", "fit_matches_affine_f32", "fit_matches_warp_lanczos_similarity",
           "fit_matches_warp_lanczos_projective")


@pytest.mark.parametrize("name", A_NAMES)
def test_a_block_freed_on_one_stream_is_handed_to_another(name):
    handover(transform_ops()[name])


def test_a_block_goes_round_three_streams_twice():
    rotation(transform_ops()["fit_matches_warp_lanczos_similarity"])


def test_b_eight_threads_each_on_its_own_stream(oracle):
    ops = transform_ops(small=True)
    cases = [_op_case(ops[name], 40 + i, "small") for i, name in enumerate(A_NAMES)]
    big = transform_ops()
    cases += [_op_case(big[name], 50 + i, "large") for i, name in enumerate(A_NAMES[:2])]
    run_threads(oracle, cases, threads=8, passes=3)
