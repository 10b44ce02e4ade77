"""zg_flood_fill on the device against tests/flood_ref.py, byte for byte and count for count: every shared case (tests/flood_cases.py)
in every pixel type, mode and connectivity, strided views, device seeds, the host form, a captured chain replayed on changed frames,
two streams at once, and the edge detectors that share the union-find helpers and the scratch cache, before and after."""
import functools

import numpy as np
import pytest

import zignal_amd as zg
from tests import flood_cases as K
from tests import flood_ref as R

try:
    import torch
except Exception:  # pragma: no cover
    torch = None

T = zg.flood_fill_tile()  # a host constant of the library: no GPU needed to read it
CASES = K.cases(T)
INDEX = {c.name: i for i, c in enumerate(CASES)}
SMALL = 4096  # pixels


@functools.lru_cache(maxsize=None)
def want(index, pixel, mode, conn):
    """The restatement's (filled image, count) of one case: computed once, shared by the tests below, never written."""
    case = CASES[index]
    out, n = R.flood_fill_fast(K.image_of(case, pixel), *case.seed, K.fill_of(case, pixel), K.threshold_of(case, pixel), conn, mode)
    out.setflags(write=False)
    return out, n


def same_bytes(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def new_count():
    return torch.full((1,), -1, dtype=torch.int32, device="cuda")


# ---- every case ------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("index", range(len(CASES)), ids=[c.name for c in CASES])
def test_flood_fill_equals_the_reference(index):
    case = CASES[index]
    for pixel in K.pixels_of(case):
        host = K.image_of(case, pixel)
        fill, thr = K.fill_of(case, pixel), K.threshold_of(case, pixel)
        for mode in K.MODES:
            for conn in K.CONNECTIVITIES:
                dev = torch.from_numpy(host).cuda()
                count = new_count()
                img = zg.Image(dev)
                assert img.flood_fill(*case.seed, fill, thr, conn, mode, count=count) is img
                out, n = want(index, pixel, mode, conn)
                assert same_bytes(dev.cpu().numpy(), out), (pixel, mode, conn)
                assert int(count.item()) == n, (pixel, mode, conn)


@pytest.mark.gpu
def test_options_object_and_no_count():
    index = INDEX["checkerboard"]
    case = CASES[index]
    dev = torch.from_numpy(K.image_of(case, "rgb_u8")).cuda()
    zg.Image(dev).flood_fill(*case.seed, K.fill_of(case, "rgb_u8"), options=zg.FloodFillOptions(0.0, 8, "neighbor"))
    assert same_bytes(dev.cpu().numpy(), want(index, "rgb_u8", "neighbor", 8)[0])
    dev = torch.from_numpy(K.image_of(case, "u8")).cuda()
    zg.Image(dev).flood_fill(*case.seed, K.fill_of(case, "u8"))  # the defaults: threshold 0, four, seed
    assert same_bytes(dev.cpu().numpy(), want(index, "u8", "seed", 4)[0])


# ---- views -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("name", [f"shape_{T + 1}x{T + 1}", "comb", "threshold_inf", "ramp_across", "shape_1xN", "shape_Nx1"])
def test_views_of_a_wider_tensor_leave_their_surroundings_alone(name):
    """The surroundings hold the seed's own value: a kernel that looked or wrote past the view's columns or rows would join or fill them."""
    index = INDEX[name]
    case = CASES[index]
    for k, pixel in enumerate(K.PIXELS):
        inner = K.image_of(case, pixel)
        rows, cols = inner.shape[:2]
        top, left = 2, 1 + k % 4  # the first pixel's address takes every alignment
        wide = np.empty((rows + 5, cols + left + 3) + inner.shape[2:], inner.dtype)
        wide[...] = inner[case.seed]
        wide[top:top + rows, left:left + cols] = inner
        fill, thr = K.fill_of(case, pixel), K.threshold_of(case, pixel)
        for mode in K.MODES:
            dev = torch.from_numpy(wide).cuda()
            count = new_count()
            zg.Image(dev[top:top + rows, left:left + cols]).flood_fill(*case.seed, fill, thr, 8, mode, count=count)
            out, n = want(index, pixel, mode, 8)
            expect = wide.copy()
            expect[top:top + rows, left:left + cols] = out
            assert same_bytes(dev.cpu().numpy(), expect), (pixel, mode)
            assert int(count.item()) == n, (pixel, mode)


# ---- a seed on the device ----------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_a_device_seed_in_range_and_out_of_range():
    index = INDEX[f"shape_{T + 1}x{2 * T + 1}"]
    case = CASES[index]
    for pixel in K.PIXELS:
        host = K.image_of(case, pixel)
        rows, cols = host.shape[:2]
        fill, thr = K.fill_of(case, pixel), K.threshold_of(case, pixel)
        dev = torch.from_numpy(host).cuda()
        count = new_count()
        seed = torch.tensor(case.seed, dtype=torch.int32, device="cuda")
        zg.Image(dev).flood_fill(rows - 1, cols - 1, fill, thr, 8, "neighbor", seed=seed, count=count)  # the host's seed is ignored
        out, n = want(index, pixel, "neighbor", 8)
        assert same_bytes(dev.cpu().numpy(), out) and int(count.item()) == n, pixel
        for outside in ((rows, 0), (0, cols), (rows, cols), (-1, 0), (0, -1), (1 << 30, 1 << 30)):  # -1 is 2^32 - 1 as a u32
            dev = torch.from_numpy(host).cuda()
            count = new_count()
            seed = torch.tensor(outside, dtype=torch.int32, device="cuda")
            for mode in K.MODES:
                zg.Image(dev).flood_fill(0, 0, fill, thr, 8, mode, seed=seed, count=count)
                assert same_bytes(dev.cpu().numpy(), host) and int(count.item()) == 0, (pixel, outside, mode)


# ---- host pointers -----------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("index", [i for i, c in enumerate(CASES) if (c.image if c.plane is None else c.plane).size < SMALL],
                         ids=[c.name for c in CASES if (c.image if c.plane is None else c.plane).size < SMALL])
def test_the_host_form_on_the_small_cases(index):
    case = CASES[index]
    for pixel in K.pixels_of(case):
        fill, thr = K.fill_of(case, pixel), K.threshold_of(case, pixel)
        for mode in K.MODES:
            for conn in K.CONNECTIVITIES:
                host = K.image_of(case, pixel)
                out, n = want(index, pixel, mode, conn)
                assert zg.Image(host).flood_fill(*case.seed, fill, thr, conn, mode) == n, (pixel, mode, conn)
                assert same_bytes(host, out), (pixel, mode, conn)


@pytest.mark.gpu
def test_the_host_form_on_a_view_keeps_the_bytes_between_cols_and_stride():
    index = INDEX["ramp_across"]
    case = CASES[index]
    for pixel in K.PIXELS:
        inner = K.image_of(case, pixel)
        rows, cols = inner.shape[:2]
        wide = np.empty((rows, cols + 5) + inner.shape[2:], inner.dtype)
        wide[...] = inner[case.seed]
        wide[:, 2:2 + cols] = inner
        expect = wide.copy()
        out, n = want(index, pixel, "neighbor", 4)
        expect[:, 2:2 + cols] = out
        assert zg.Image(wide[:, 2:2 + cols]).flood_fill(*case.seed, K.fill_of(case, pixel), K.threshold_of(case, pixel), 4, "neighbor") == n
        assert same_bytes(wide, expect), pixel


# ---- a captured chain --------------------------------------------------------------------------------------------------------------
ROWS, COLS = 2 * T + 22, 3 * T + 9


def photo(seed):
    """Patches of grey levels eight pixels wide with a little noise: edges for the detectors, regions for the threshold."""
    rng = np.random.default_rng(seed)
    coarse = rng.integers(20, 236, ((ROWS + 7) // 8, (COLS + 7) // 8))
    frame = np.kron(coarse, np.ones((8, 8), np.int64))[:ROWS, :COLS] + rng.integers(-6, 7, (ROWS, COLS))
    return np.clip(frame, 0, 255).astype(np.uint8)


class Chain:
    """threshold -> flood_fill with a device seed and a count, on the current stream."""

    def __init__(self):
        self.src = torch.zeros((ROWS, COLS), dtype=torch.uint8, device="cuda")
        self.binary = torch.zeros_like(self.src)
        self.seed = torch.zeros(2, dtype=torch.int32, device="cuda")
        self.count = new_count()

    def load(self, frame_seed, seed):
        self.src.copy_(torch.from_numpy(photo(frame_seed)))
        self.seed.copy_(torch.tensor(seed, dtype=torch.int32))
        self.binary.fill_(7)
        self.count.fill_(-1)
        self.at = seed

    def enqueue(self):
        zg.Image(self.src).threshold_adaptive_mean(3, 2.0, out=self.binary)
        zg.Image(self.binary).flood_fill(0, 0, 128, 0.0, 8, "seed", seed=self.seed, count=self.count)

    def check(self, name):
        binary = zg.Image(self.src).threshold_adaptive_mean(3, 2.0).to_numpy()  # the same op on its own: what the fill saw
        assert set(np.unique(binary)) == {0, 255}, name
        out, n = R.flood_fill_fast(binary, *self.at, 128, 0.0, 8, "seed")
        assert n > 1 and same_bytes(self.binary.cpu().numpy(), out), name
        assert int(self.count.item()) == n, name


@pytest.mark.gpu
def test_threshold_then_flood_fill_replays_from_a_graph_on_changed_frames_and_seeds():
    chain = Chain()
    side = torch.cuda.Stream()
    chain.load(1, (5, 5))
    torch.cuda.synchronize()
    with torch.cuda.stream(side):
        chain.enqueue()  # warm-up outside the capture
    side.synchronize()
    chain.check("eager")
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        chain.enqueue()
    for frame_seed, seed in ((2, (T, T - 1)), (3, (ROWS - 1, COLS - 1))):
        chain.load(frame_seed, seed)
        torch.cuda.synchronize()
        graph.replay()
        torch.cuda.synchronize()
        chain.check(f"replay on frame {frame_seed}")
    del graph
    torch.cuda.synchronize()
    assert zg.lib().zg_release_graph_scratch() == 0


# ---- two streams -------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_two_streams_fill_two_images_at_once():
    index = INDEX[f"shape_{2 * T + 1}x{2 * T + 1}"]
    case = CASES[index]
    pixels = ("u8", "rgba_f32")
    hosts = [K.image_of(case, p) for p in pixels]
    devs = [torch.from_numpy(h).cuda() for h in hosts]
    counts = [torch.zeros(4, dtype=torch.int32, device="cuda") for _ in pixels]
    streams = [torch.cuda.Stream(), torch.cuda.Stream()]
    rounds = [((0, 0), 201), (case.seed, 202), ((2 * T, 2 * T), 203), ((T, T), 204)]
    torch.cuda.synchronize()
    for k, (seed, value) in enumerate(rounds):  # both streams stay busy: each call is enqueued behind the other stream's, none is waited for
        for dev, count, pixel, s in zip(devs, counts, pixels, streams):
            with torch.cuda.stream(s):
                zg.Image(dev).flood_fill(*seed, K._typed(value, pixel, case.channel).tolist(), K.threshold_of(case, pixel), 8, "neighbor", count=count[k:])
    torch.cuda.synchronize()
    for dev, count, pixel, host in zip(devs, counts, pixels, hosts):
        expect, ns = host, []
        for seed, value in rounds:
            expect, n = R.flood_fill_fast(expect, *seed, K._typed(value, pixel, case.channel).tolist(), K.threshold_of(case, pixel), 8, "neighbor")
            ns.append(n)
        assert same_bytes(dev.cpu().numpy(), expect), pixel
        assert count.cpu().tolist() == ns, pixel


# ---- the detectors that share the union-find and the scratch cache ----------------------------------------------------------------------
@pytest.mark.gpu
def test_canny_and_shen_castan_are_unchanged_by_flood_fills_in_between():
    frame = torch.from_numpy(photo(9)).cuda()

    def detect():
        canny = zg.Image(frame).canny(1.0, 30, 90).to_numpy()
        shen = zg.Image(frame).shen_castan().to_numpy()
        assert 100 < np.count_nonzero(canny) < canny.size and 100 < np.count_nonzero(shen) < shen.size
        return canny, shen

    before = detect()
    for name in ("spiral", f"shape_{T - 1}x{2 * T + 1}", "comb"):
        index = INDEX[name]
        case = CASES[index]
        for pixel in ("u8", "rgb_f32"):
            dev = torch.from_numpy(K.image_of(case, pixel)).cuda()
            zg.Image(dev).flood_fill(*case.seed, K.fill_of(case, pixel), K.threshold_of(case, pixel), 8, "seed")
            assert same_bytes(dev.cpu().numpy(), want(index, pixel, "seed", 8)[0]), (name, pixel)
    edges = torch.from_numpy(before[0]).cuda()  # an edge map already on the device is what the fill is for
    zg.Image(edges).flood_fill(0, 0, 64, 0.0, 4, "seed")
    assert same_bytes(edges.cpu().numpy(), R.flood_fill_fast(before[0], 0, 0, 64, 0.0, 4, "seed")[0])
    after = detect()
    assert same_bytes(before[0], after[0]) and same_bytes(before[1], after[1])
