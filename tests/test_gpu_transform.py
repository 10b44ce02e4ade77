"""Geometry fitting on the device (include/zignal_hip_transform.h) against the library's _host forms, which run the same header
(zignal_amd/csrc/zg_transform_fit.h) on the CPU and are themselves pinned to tests/transform_ref.py bit for bit
(tests/test_transform_fit_host.py): every comparison here is of the 128 bytes of a record, or of the bytes of a frame.

  sizes        N around every seam of the workgroup's executor: the minimum, 63-65 (a wave), the chunk of the ordered sums - 1, + 0, + 1,
               two chunks and three; affine also at 85, 86 (Matrix.gemm's threshold in the reference) and 4096 (the bound: U fills LDS)
  families     every point set of tests/transform_cases.py: reflections, duplicated, all-equal and collinear points, f32 inputs scaled to
               1e-20 (products under the normal range: a flushed subnormal or an approximate division or square root shows here) and 1e+15
  counts       a count word above the capacity, a count of 0, a capacity above the bound under a count word; points past the count are NaN
  matches      a match list and two keypoint arrays, both directions; an index outside its array
  project, invert, warp_fitted against their host forms and zg_warp with the downloaded m32; a failed record leaves a poisoned dst untouched
  chain        ORB twice, match with cross-check, fit, warp: captured in a graph and replayed on a changed second frame"""
import numpy as np
import pytest

torch = pytest.importorskip("torch")
import zignal_amd as zg  # noqa: E402
from zignal_amd import _lib as L  # noqa: E402
from zignal_amd import transform as TF  # noqa: E402
from tests import transform_cases as K  # noqa: E402

pytestmark = pytest.mark.gpu
KINDS = (TF.SIMILARITY, TF.AFFINE, TF.PROJECTIVE)
KIND_NAMES = {TF.SIMILARITY: "similarity", TF.AFFINE: "affine", TF.PROJECTIVE: "projective"}
SCALARS = (L.SCALAR_F32, L.SCALAR_F64)
KP, MATCH = zg.KEYPOINT_DTYPE, zg.MATCH_DTYPE


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def device_fit(kind, f, t, count=None, capacity=None):
    rec = torch.full((128,), 0xAB, dtype=torch.uint8, device="cuda")
    cnt = None if count is None else dev(np.array([count], np.uint32).view(np.int32))
    TF.fit_points_into(kind, dev(f), dev(t), rec, count=cnt, capacity=capacity)
    return rec.cpu().numpy()


def host_fit(kind, f, t, count=None):
    return np.frombuffer(TF.fit_points_host(kind, f, t, count=count).tobytes(), np.uint8)


def same_record(got, want, what):
    if not np.array_equal(got, want):
        g, w = got.view(TF.FIT_DTYPE)[0], want.view(TF.FIT_DTYPE)[0]
        raise AssertionError(f"{what}: device {g} host {w}")


def sizes(kind):
    lo, chunk = K.MIN_POINTS[kind], TF.chunk()
    out = [lo, lo + 1, 63, 64, 65, chunk - 1, chunk, chunk + 1, 2 * chunk + 3, 3 * chunk]
    if kind == TF.AFFINE:
        out += [85, 86, 4096]
    return out


@pytest.mark.parametrize("scalar", SCALARS)
@pytest.mark.parametrize("kind", KINDS)
def test_sizes_around_every_seam(kind, scalar):
    assert TF.chunk() >= 66
    for n in sizes(kind):
        f, t = K.cloud(kind, scalar, n)
        want = host_fit(kind, f, t)
        if n > K.MIN_POINTS[kind]:  # at four points the f32 8 x 8 system of pixel coordinates falls under SMatrix.solve's tolerance
            assert want.view(TF.FIT_DTYPE)[0]["status"] == L.FIT_OK, (KIND_NAMES[kind], n)
        same_record(device_fit(kind, f, t), want, f"{KIND_NAMES[kind]} scalar {scalar} n {n}")


def hook_child():
    """Run in a child process started with ZIGNAL_HIP_FIT_VARIANT set: the sizes and a share of the families, device against host."""
    for kind in KINDS:
        for scalar in SCALARS:
            test_sizes_around_every_seam(kind, scalar)
            for name, f, t in K.fit_cases(kind, scalar)[::5]:
                same_record(device_fit(kind, f, t), host_fit(kind, f, t), f"{KIND_NAMES[kind]} scalar {scalar} {name} n {len(f)}")


@pytest.mark.parametrize("variant", (1, 2, 3))
def test_the_forms_behind_the_tuning_hook_give_the_same_bits(variant):
    """ZIGNAL_HIP_FIT_VARIANT (read once per process, so a child): the 9 x 9 SVD on one lane, the SVD's dot products unstaged, both."""
    import os
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    out = subprocess.run([sys.executable, "-c", "from tests.test_gpu_transform import hook_child; hook_child(); print('ok')"], capture_output=True, text=True,
                         timeout=300, cwd=root, env=dict(os.environ, ZIGNAL_HIP_FIT_VARIANT=str(variant)))
    assert out.returncode == 0 and out.stdout.strip().endswith("ok"), out.stdout[-2000:] + out.stderr[-3000:]


@pytest.mark.parametrize("scalar", SCALARS)
@pytest.mark.parametrize("kind", KINDS)
def test_every_family_of_point_sets(kind, scalar):
    statuses = set()
    for name, f, t in K.fit_cases(kind, scalar):
        want = host_fit(kind, f, t)
        statuses.add(int(want.view(TF.FIT_DTYPE)[0]["status"]))
        same_record(device_fit(kind, f, t), want, f"{KIND_NAMES[kind]} scalar {scalar} {name} n {len(f)}")
    assert {L.FIT_OK, L.FIT_RANK_DEFICIENT} <= statuses
    if (kind, scalar) == (TF.PROJECTIVE, L.SCALAR_F32):  # coordinates at 1e+15 in f32: the 9 x 9 SVD passes 300 iterations
        assert L.FIT_NOT_CONVERGED in statuses


@pytest.mark.parametrize("kind", KINDS)
def test_count_word_and_bounds(kind):
    lo, hi = K.MIN_POINTS[kind], (L.FIT_MAX_POINTS_AFFINE if kind == TF.AFFINE else L.FIT_MAX_POINTS)
    for scalar in SCALARS:
        f, t = K.cloud(kind, scalar, 40, seed=1)
        # a count above the capacity is the capacity; below it, the points past it are never read (they are NaN here)
        same_record(device_fit(kind, f, t, count=1000), host_fit(kind, f, t), "count above capacity")
        same_record(device_fit(kind, f, t, count=2 ** 32 - 1), host_fit(kind, f, t), "count 2^32 - 1")
        fn, tn = f.copy(), t.copy()
        fn[17:], tn[17:] = np.nan, np.nan
        got = device_fit(kind, fn, tn, count=17)
        same_record(got, host_fit(kind, f[:17], t[:17]), "count below capacity")
        assert got.view(TF.FIT_DTYPE)[0]["status"] == L.FIT_OK and got.view(TF.FIT_DTYPE)[0]["n_points"] == 17
        # too few, none, too many: ZG_FIT_BAD_COUNT and the identity
        for count in (0, lo - 1):
            got = device_fit(kind, f, t, count=count)
            same_record(got, host_fit(kind, f, t, count=count), f"count {count}")
            r = got.view(TF.FIT_DTYPE)[0]
            assert r["status"] == L.FIT_BAD_COUNT and r["n_points"] == count and r["kind"] == kind
            ident = [1, 0, 0, 1, 0, 0, 0, 0, 0] if kind != TF.PROJECTIVE else [1, 0, 0, 0, 1, 0, 0, 0, 1]
            assert r["m64"].tolist() == ident and r["m32"].tolist() == ident
        big = np.zeros((hi + 1, 2), f.dtype)
        big[:40] = f
        got = device_fit(kind, big, big)
        same_record(got, host_fit(kind, big, big), "one point past the bound")
        assert got.view(TF.FIT_DTYPE)[0]["status"] == L.FIT_BAD_COUNT
        same_record(device_fit(kind, big, big[::-1].copy(), count=40), host_fit(kind, big, big[::-1].copy(), count=40), "capacity past the bound, count under it")


def _keypoints(rng, n):
    k = np.zeros(n, KP)
    k["x"], k["y"] = rng.uniform(0, 640, n).astype(np.float32), rng.uniform(0, 480, n).astype(np.float32)
    k["size"], k["angle"], k["octave"], k["class_id"] = 31.0, rng.uniform(0, 360, n).astype(np.float32), rng.integers(0, 8, n), -1
    return k


def _match_setup(kind, n, seed):
    rng = np.random.default_rng(4100 + seed)
    nq, nt = n + 13, n + 40
    q = _keypoints(rng, nq)
    t = _keypoints(rng, nt)
    m = np.zeros(n, MATCH)
    m["query_idx"], m["train_idx"] = rng.permutation(nq)[:n], rng.permutation(nt)[:n]
    m["distance"] = rng.integers(0, 64, n).astype(np.float32)
    f = np.stack([q["x"][m["query_idx"]], q["y"][m["query_idx"]]], 1).astype(np.float64)
    mapped = K._mapped(rng, kind, f) + rng.normal(0, 0.3, f.shape)
    t["x"][m["train_idx"]], t["y"][m["train_idx"]] = mapped[:, 0].astype(np.float32), mapped[:, 1].astype(np.float32)
    return q, t, m


def device_fit_matches(kind, scalar, q, t, m, count=None, train_to_query=False):
    rec = torch.full((128,), 0xCD, dtype=torch.uint8, device="cuda")
    cnt = None if count is None else dev(np.array([count], np.uint32).view(np.int32))
    TF.fit_matches_into(kind, scalar, dev(q.view(np.uint8).reshape(-1)), dev(t.view(np.uint8).reshape(-1)), dev(m.view(np.uint8).reshape(-1)), rec, count=cnt,
                        train_to_query=train_to_query)
    return rec.cpu().numpy()


@pytest.mark.parametrize("kind", KINDS)
def test_fit_from_matches(kind):
    chunk = TF.chunk()
    for scalar in SCALARS:
        for n in (K.MIN_POINTS[kind], 65, chunk + 1, 2 * chunk + 3):
            q, t, m = _match_setup(kind, n, n)
            for back in (False, True):
                want = np.frombuffer(TF.fit_matches_host(kind, scalar, q, t, m, train_to_query=back).tobytes(), np.uint8)
                same_record(device_fit_matches(kind, scalar, q, t, m, train_to_query=back), want, f"{KIND_NAMES[kind]} matches n {n} back {back}")
                # the same points as two raw arrays in the scalar type
                dt = K.DTYPES[scalar]
                f = np.stack([q["x"][m["query_idx"]], q["y"][m["query_idx"]]], 1).astype(dt)
                o = np.stack([t["x"][m["train_idx"]], t["y"][m["train_idx"]]], 1).astype(dt)
                same_record(want, host_fit(kind, o, f) if back else host_fit(kind, f, o), "matches against raw points")
            if n > 10:  # the count word zg_match_descriptors writes: fewer than the list holds, and more
                want = np.frombuffer(TF.fit_matches_host(kind, scalar, q, t, m, count=n - 3).tobytes(), np.uint8)
                same_record(device_fit_matches(kind, scalar, q, t, m, count=n - 3), want, "count below capacity")
                same_record(device_fit_matches(kind, scalar, q, t, m, count=n + 9), np.frombuffer(TF.fit_matches_host(kind, scalar, q, t, m).tobytes(), np.uint8),
                            "count above capacity")
        # an index outside its keypoint array, query side and train side: ZG_FIT_BAD_INPUT, the identity, and no read past the arrays
        q, t, m = _match_setup(kind, 70, 5)
        for field, limit in (("query_idx", len(q)), ("train_idx", len(t))):
            for bad in (limit, 2 ** 32 - 1):
                mb = m.copy()
                mb[field][41] = bad
                got = device_fit_matches(kind, scalar, q, t, mb)
                same_record(got, np.frombuffer(TF.fit_matches_host(kind, scalar, q, t, mb).tobytes(), np.uint8), f"{field} = {bad}")
                r = got.view(TF.FIT_DTYPE)[0]
                assert r["status"] == L.FIT_BAD_INPUT and r["n_points"] == 70 and r["m32"][0] == 1.0
                # past the count the bad entry is not looked at
                assert device_fit_matches(kind, scalar, q, t, mb, count=41).view(TF.FIT_DTYPE)[0]["status"] == L.FIT_OK


def _status_records():
    """One record per status, from fits that end that way."""
    out = {}
    for kind in KINDS:
        for scalar in SCALARS:
            for name, f, t in K.fit_cases(kind, scalar):
                r = TF.fit_points_host(kind, f, t)
                out.setdefault((int(r["status"]), kind), (r, scalar))
    return out


def test_project_points_and_invert():
    rng = np.random.default_rng(9)
    for (status, kind), (r, scalar) in sorted(_status_records().items()):
        rec = TF.upload_record(r)
        for s in SCALARS:
            pts = rng.uniform(-100, 700, size=(1000, 2)).astype(K.DTYPES[s])
            pts[0] = 0
            got = TF.project_points(rec, dev(pts)).cpu().numpy()
            want = TF.project_points(r, pts)
            assert got.tobytes() == want.tobytes(), (status, kind, s)
            inv = TF.invert(rec, s).cpu().numpy()
            same_record(inv, np.frombuffer(TF.invert(r, s).tobytes(), np.uint8), f"invert status {status} kind {kind} scalar {s}")
            ri = inv.view(TF.FIT_DTYPE)[0]
            if status != L.FIT_OK:
                assert ri["status"] == status
            elif kind != TF.PROJECTIVE:
                assert ri["status"] == L.FIT_BAD_INPUT
    # a matrix with no inverse: SMatrix.inv's null
    r = np.zeros(1, TF.FIT_DTYPE)[0]
    r["kind"], r["m64"], r["m32"] = TF.PROJECTIVE, [1, 2, 3, 2, 4, 6, 0, 0, 1], [1, 2, 3, 2, 4, 6, 0, 0, 1]
    for s in SCALARS:
        inv = TF.invert(TF.upload_record(r), s).cpu().numpy()
        same_record(inv, np.frombuffer(TF.invert(r, s).tobytes(), np.uint8), "singular")
        assert inv.view(TF.FIT_DTYPE)[0]["status"] == L.FIT_RANK_DEFICIENT and inv.view(TF.FIT_DTYPE)[0]["m64"].tolist() == [1, 0, 0, 0, 1, 0, 0, 0, 1]
    # in place
    f, t = K.cloud(TF.PROJECTIVE, L.SCALAR_F64, 12)
    r = TF.fit_points_host(TF.PROJECTIVE, f, t)
    rec = TF.upload_record(r)
    TF.invert(rec, L.SCALAR_F64, out=rec)
    same_record(rec.cpu().numpy(), np.frombuffer(TF.invert(r, L.SCALAR_F64).tobytes(), np.uint8), "invert in place")


class _Coefficients:
    def __init__(self, kind, m32):
        self.kind, self.m = kind, m32

    def coefficients(self):
        return self.m if self.kind == TF.PROJECTIVE else self.m[:6]


def _warp_record(kind, rows, cols):
    """A fit whose map keeps most of a rows x cols frame inside the source."""
    rng = np.random.default_rng(300 + kind)
    f = rng.uniform(0, 1, size=(24, 2)) * (cols, rows)
    if kind == TF.PROJECTIVE:
        h = np.array([[0.96, 0.05, 3.0], [-0.04, 1.03, -2.0], [1e-4, -2e-4, 1.0]])
        t = K._apply_h(h, f)
    else:
        a = np.deg2rad(7.0)
        m = 1.05 * np.array([[np.cos(a), -np.sin(a)], [np.sin(a), np.cos(a)]]) + (0 if kind == TF.SIMILARITY else np.array([[0.0, 0.08], [0.0, 0.0]]))
        t = f @ m.T + (4.0, -6.0)
    r = TF.fit_points_host(kind, f, t + rng.normal(0, 0.2, t.shape), scalar=np.float64)
    assert r["status"] == L.FIT_OK
    return r


@pytest.mark.parametrize("pixel", ("rgba_u8", "f32"))
def test_warp_fitted_equals_warp_with_the_downloaded_matrix(pixel):
    rows, cols = 97, 131
    rng = np.random.default_rng(12)
    frame = rng.integers(0, 256, (rows, cols, 4), dtype=np.uint8) if pixel == "rgba_u8" else rng.random((rows, cols), np.float32)
    src = zg.Image(dev(frame))
    for kind in KINDS:
        r = _warp_record(kind, rows, cols)
        rec = TF.upload_record(r)
        for method in (zg.Interpolation.nearest, zg.Interpolation.bilinear, zg.Interpolation.lanczos):
            for shape in ((rows, cols), (61, 200)):
                want = src.warp(_Coefficients(kind, np.array(r["m32"])), shape, method).to_numpy()
                got = TF.warp_fitted(src, rec, shape, method).to_numpy()
                assert got.tobytes() == want.tobytes(), (pixel, KIND_NAMES[kind], method, shape)
                assert not np.array_equal(got, np.zeros_like(got))
        # a record that is not ZG_FIT_OK leaves a poisoned destination untouched, whatever its matrix says
        for status in (L.FIT_NOT_CONVERGED, L.FIT_RANK_DEFICIENT, L.FIT_BAD_COUNT, L.FIT_BAD_INPUT):
            failed = r.copy()
            failed["status"] = status
            poison = np.full_like(frame, 0x5A) if pixel == "rgba_u8" else np.full_like(frame, -7.5)
            out = zg.Image(dev(poison))
            TF.warp_fitted(src, TF.upload_record(failed), out, zg.Interpolation.bilinear)
            assert out.to_numpy().tobytes() == poison.tobytes(), status


# ---- the chain: two frames in, aligned frame out -------------------------------------------------------------------------------------

CAP = 500


class Chain:
    """ORB on both frames, match with cross-check, fit from the matches, warp the second frame onto the first one's grid: nothing but
    enqueues on the current stream."""

    def __init__(self, rows, cols, kind=TF.SIMILARITY, scalar=L.SCALAR_F64):
        z = lambda n, dt=torch.uint8: torch.zeros(n, dtype=dt, device="cuda")  # noqa: E731
        self.kind, self.scalar = kind, scalar
        self.a, self.b, self.out = z((rows, cols)), z((rows, cols)), z((rows, cols))
        self.kps = [z(CAP * KP.itemsize), z(CAP * KP.itemsize)]
        self.des = [z(CAP * 32), z(CAP * 32)]
        self.counts = [z(1, torch.int32), z(1, torch.int32)]
        self.matches, self.n_matches = z(CAP * MATCH.itemsize), z(1, torch.int32)
        self.record = z(128)
        self.orb, self.matcher = zg.Orb(), zg.BruteForceMatcher(cross_check=True)

    def features(self):
        for img, k, d, c in zip((self.a, self.b), self.kps, self.des, self.counts):
            self.orb.detect_and_compute_into(zg.Image(img), k, d, c, CAP)
        self.matcher.match_into(self.des[0], self.des[1], self.matches, self.n_matches, CAP, query_count=self.counts[0], train_count=self.counts[1])

    def run(self):
        """Query = frame a, train = frame b; the fit maps a's coordinates onto b's, which is what warp needs to resample b onto a's grid."""
        self.features()
        TF.fit_matches_into(self.kind, self.scalar, self.kps[0], self.kps[1], self.matches, self.record, count=self.n_matches, capacity=CAP)
        TF.warp_fitted(zg.Image(self.b), self.record, zg.Image(self.out), zg.Interpolation.bilinear)

    def run_with_host_fit(self):
        """The same with the fit on the host: download the lists, zg_transform_fit_matches_host, zg_warp with its m32."""
        self.features()
        torch.cuda.synchronize()
        n = int(self.n_matches.item())
        r = TF.fit_matches_host(self.kind, self.scalar, self.kps[0].cpu().numpy(), self.kps[1].cpu().numpy(), self.matches.cpu().numpy(), count=n)
        out = zg.Image(torch.zeros_like(self.out))
        if r["status"] == L.FIT_OK:
            zg.Image(self.b).warp(_Coefficients(self.kind, np.array(r["m32"])), out, zg.Interpolation.bilinear)
        return r, out.to_numpy()


def chain_frames(oracle, rows, cols, seed):
    """A synthetic frame with corners at several scales, and two similarity-warped copies of it."""
    from tests import fast_ref as F
    base = F.photo_like(oracle.synth_u8(1200 + seed, (rows, cols)))
    src = zg.Image(dev(base))
    copies = []
    for deg, scale, shift in ((2.0, 1.02, (5.0, -3.0)), (-3.0, 0.98, (-4.0, 9.0))):
        a = np.deg2rad(deg)
        m = scale * np.array([[np.cos(a), -np.sin(a)], [np.sin(a), np.cos(a)]])
        centre = np.array([cols / 2, rows / 2])
        bias = centre - m @ centre + shift
        copies.append(src.warp(zg.SimilarityTransform(m, bias), (rows, cols), zg.Interpolation.bilinear).to_numpy())
    return base, copies


def test_chain_captured_in_a_graph_and_replayed_on_a_changed_second_frame(oracle):
    rows, cols = 256, 320
    base, copies = chain_frames(oracle, rows, cols, 0)
    chain = Chain(rows, cols)
    chain.a.copy_(torch.from_numpy(base))
    chain.b.copy_(torch.from_numpy(copies[0]))
    chain.run()  # the process's first calls: tables and scratch enter the caches
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        chain.run()
    outs = []
    for k in (0, 1, 0):
        chain.b.copy_(torch.from_numpy(copies[k]))
        chain.out.fill_(0x77)
        chain.record.fill_(0xEE)
        torch.cuda.synchronize()
        graph.replay()
        torch.cuda.synchronize()
        got_record, got = chain.record.cpu().numpy(), chain.out.cpu().numpy()
        want_record, want = chain.run_with_host_fit()
        same_record(got_record, np.frombuffer(want_record.tobytes(), np.uint8), f"chain, second frame {k}")
        # two points determine a similarity; from three on the fit is a least-squares one and every stage of find has work to do
        assert want_record["status"] == L.FIT_OK and want_record["n_points"] >= 3, want_record
        assert got.tobytes() == want.tobytes(), k
        outs.append(got)
    assert not np.array_equal(outs[0], outs[1]) and np.array_equal(outs[0], outs[2])
    del graph
    torch.cuda.synchronize()
    assert zg.lib().zg_release_graph_scratch() == 0
