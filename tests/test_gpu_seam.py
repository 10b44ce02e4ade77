"""The zg_seam_* entry points on the device against tests/seam_ref.py, byte for byte: the energy map, the seam and the removal on every
shared case (tests/seam_cases.py), the whole iteration in four pixel types and both axes, the staged loop against the fused call, views
of wider tensors at every start alignment, the host forms, a captured carve replayed on changed frames, two streams at once, and the
detectors that share the scratch cache and the Sobel kernels, before and after."""
import functools

import numpy as np
import pytest

import zignal_amd as zg
from oracle import pyoracle as oracle  # the checker's sobel: read, never the thing under test
from tests import seam_cases as K
from tests import seam_ref as R

try:
    import torch
except Exception:  # pragma: no cover
    torch = None

B, S = zg.seam_band_rows(), zg.seam_strip_cols()  # host constants of the library: no GPU needed to read them
CASES = K.edge_cases(B, S)
INDEX = {c.name: i for i, c in enumerate(CASES)}
LARGEST = (3 * B + 1, 2 * S + 3)
SMALL_SHAPES = ((1, 9), (7, 2), (2, 2), (B + 1, S + 1), (5, 2 * S + 3))
CARVE_PIXELS = ("u8", "rgb_u8", "rgba_u8", "rgba_f32")


@functools.lru_cache(maxsize=None)
def want_energy(index):
    e = R.compute_energy_fast(CASES[index].edges)
    e.setflags(write=False)
    return e


@functools.lru_cache(maxsize=None)
def want_seam(index):
    s = R.compute_seam_fast(want_energy(index))
    s.setflags(write=False)
    return s


@functools.lru_cache(maxsize=None)
def want_carve(shape, pixel, n, seed=1):
    """The restatement's (carved frame, seams) of one frame: computed once, shared, never written."""
    out, seams = R.carve(K.frame(seed, *shape, pixel), n, oracle.sobel)
    out.setflags(write=False)
    seams.setflags(write=False)
    return out, seams


def same_bytes(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def words(t):
    """A device word buffer as numpy uint32."""
    return t.cpu().numpy().view(np.uint32)


def device_words(a):
    return torch.from_numpy(np.array(a, np.uint32).view(np.int32)).cuda()


def new_words(count):
    return torch.full((count,), -7, dtype=torch.int32, device="cuda")


# ---- the three stages on every case ---------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("index", range(len(CASES)), ids=[c.name for c in CASES])
def test_energy_and_seam_equal_the_reference(index):
    case = CASES[index]
    rows, cols = case.edges.shape
    edges = torch.from_numpy(case.edges).cuda()
    energy = zg.seam_energy(edges)
    assert tuple(energy.shape) == (rows, cols)
    assert np.array_equal(words(energy), want_energy(index))
    seam = zg.seam_find(energy, rows, cols)
    assert np.array_equal(words(seam), want_seam(index))
    if case.seam is not None:
        assert np.array_equal(words(seam), case.seam)
    # the seam of a map that did not come from the energy kernel: the case's bytes themselves, as sums
    raw = case.edges.astype(np.uint32) * np.uint32(0x01000193)  # large words: the compare is unsigned
    assert np.array_equal(words(zg.seam_find(device_words(raw), rows, cols)), R.compute_seam_fast(raw))
    assert same_bytes(edges.cpu().numpy(), case.edges)


@pytest.mark.gpu
@pytest.mark.parametrize("pixel", K.PIXELS)
def test_removal_moves_pixels_in_all_six_types(pixel):
    rng = np.random.default_rng(8)
    for name in ("shape_1xN", "shape_Nx2", "shape_2x2", "shape_Nx1", f"shape_{B + 1}x{S + 1}", "diagonal_valley", "right_border", "left_border"):
        index = INDEX[name]
        rows, cols = CASES[index].edges.shape
        host = K.pixels_like(index, rows, cols, pixel)
        seams = [np.asarray(want_seam(index)), rng.integers(0, cols, rows).astype(np.uint32)]
        past = seams[1].copy()
        past[::3] = (cols, cols + 1, 0xFFFFFFFF)[index % 3]  # removes nothing from the row and drops its last pixel
        seams.append(past)
        for seam in seams:
            src = torch.from_numpy(host).cuda()
            out = zg.Image(src).seam_remove(device_words(seam))
            assert same_bytes(out.to_numpy(), R.remove_seam(host, seam)), (name, pixel)
            assert same_bytes(src.cpu().numpy(), host)


# ---- the iteration --------------------------------------------------------------------------------------------------------------------
def carve_on_device(host, n, axis="vertical"):
    src = torch.from_numpy(host).cuda()
    along = host.shape[1] if axis == "horizontal" else host.shape[0]
    seams = new_words(n * along)
    out = zg.Image(src).seam_carve(n, axis=axis, seams=seams)
    assert same_bytes(src.cpu().numpy(), host)  # src comes back unchanged
    return out.to_numpy(), words(seams).reshape(n, along)


@pytest.mark.gpu
@pytest.mark.parametrize("pixel", CARVE_PIXELS)
@pytest.mark.parametrize("shape", SMALL_SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_carve_equals_the_reference_on_the_small_shapes(shape, pixel):
    host = K.frame(1, *shape, pixel)
    for n in sorted({1, 2, shape[1] - 1}):
        if not 1 <= n < shape[1]:
            continue
        got, seams = carve_on_device(host, n)
        out, ref_seams = want_carve(shape, pixel, n)
        assert same_bytes(got, out), n
        assert np.array_equal(seams, ref_seams), n


@pytest.mark.gpu
@pytest.mark.parametrize("pixel", CARVE_PIXELS)
def test_carve_of_eight_seams_on_the_largest_shape(pixel):
    got, seams = carve_on_device(K.frame(1, *LARGEST, pixel), 8)
    out, ref_seams = want_carve(LARGEST, pixel, 8)
    assert same_bytes(got, out) and np.array_equal(seams, ref_seams)


@pytest.mark.gpu
@pytest.mark.parametrize("pixel", ("rgba_u8", "f32"))
def test_the_staged_loop_equals_the_fused_call(pixel):
    shape, n = (2 * B + 1, S + 1), 5
    host = K.frame(2, *shape, pixel)
    fused, fused_seams = carve_on_device(host, n)
    cur = zg.Image(torch.from_numpy(host).cuda())
    for k in range(n):
        edges = cur.sobel()
        energy = zg.seam_energy(edges)
        seam = zg.seam_find(energy, cur.rows, cur.cols)
        assert np.array_equal(words(seam), fused_seams[k]), k
        cur = cur.seam_remove(seam)
    assert same_bytes(cur.to_numpy(), fused)
    out, ref_seams = want_carve(shape, pixel, n, 2)
    assert same_bytes(fused, out) and np.array_equal(fused_seams, ref_seams)


@pytest.mark.gpu
@pytest.mark.parametrize("pixel", ("u8", "rgb_u8", "rgba_f32"))
def test_horizontal_is_vertical_on_the_transposed_frame(pixel):
    for shape, n in (((S + 1, B + 1), 3), ((40, 33), 2), ((2, 5), 1), ((9, 1), 8)):
        host = K.frame(3, *shape, pixel)
        got, seams = carve_on_device(host, n, "horizontal")
        turned, turned_seams = carve_on_device(R.transpose(host), n)
        assert same_bytes(got, R.transpose(turned)) and np.array_equal(seams, turned_seams), shape
        out, ref_seams = R.carve_horizontal(host, n, oracle.sobel)
        assert same_bytes(got, out) and np.array_equal(seams, ref_seams), shape
        assert got.shape[:2] == (shape[0] - n, shape[1])


# ---- the walk behind the tuning hook ------------------------------------------------------------------------------------------------------
def hook_child():
    """Run in a child process started with ZIGNAL_HIP_SEAM_PLAIN_WALK=1: every case's seam, and the iteration on the largest shape."""
    for index in range(len(CASES)):
        test_energy_and_seam_equal_the_reference(index)
    for pixel in ("u8", "rgba_u8"):
        test_carve_of_eight_seams_on_the_largest_shape(pixel)
    test_horizontal_is_vertical_on_the_transposed_frame("rgb_u8")


@pytest.mark.gpu
def test_the_plain_walk_behind_the_tuning_hook_gives_the_same_bits():
    """ZIGNAL_HIP_SEAM_PLAIN_WALK=1 (read once per process, so a child): one lane walks the sums in global memory."""
    import os
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    out = subprocess.run([sys.executable, "-c", "from tests.test_gpu_seam import hook_child; hook_child(); print('ok')"], capture_output=True, text=True,
                         timeout=300, cwd=root, env=dict(os.environ, ZIGNAL_HIP_SEAM_PLAIN_WALK="1"))
    assert out.returncode == 0 and out.stdout.strip().endswith("ok"), out.stdout[-2000:] + out.stderr[-3000:]


# ---- views ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("axis", ("vertical", "horizontal"))
def test_views_of_wider_tensors_leave_their_surroundings_alone(axis):
    shape, n = (B + 2, 70), 3
    for k, pixel in enumerate(K.PIXELS):
        host = K.frame(4 + k, *shape, pixel)
        want_out, want_seams = (R.carve if axis == "vertical" else R.carve_horizontal)(host, n, oracle.sobel)
        out_rows, out_cols = want_out.shape[:2]
        for left in range(1, 5):  # the first pixel's address takes every alignment
            top = 1 + left % 2
            wide_src = K.pixels_like(20 + left, shape[0] + 4, shape[1] + left + 3, pixel)
            wide_src[top:top + shape[0], left:left + shape[1]] = host
            wide_dst = K.pixels_like(30 + left, out_rows + 3, out_cols + left + 2, pixel)
            src, dst = torch.from_numpy(wide_src).cuda(), torch.from_numpy(wide_dst).cuda()
            along = shape[1] if axis == "horizontal" else shape[0]
            seams = new_words(n * along + 2)
            view = dst[1:1 + out_rows, left:left + out_cols]
            got = zg.Image(src[top:top + shape[0], left:left + shape[1]]).seam_carve(n, axis=axis, out=view, seams=seams[1:])
            assert got.data.data_ptr() == view.data_ptr()
            expect = wide_dst.copy()
            expect[1:1 + out_rows, left:left + out_cols] = want_out
            assert same_bytes(dst.cpu().numpy(), expect), (pixel, left)
            assert same_bytes(src.cpu().numpy(), wide_src), (pixel, left)
            s = words(seams)
            assert s[0] == s[-1] == np.uint32(-7 & 0xFFFFFFFF) and np.array_equal(s[1:-1].reshape(n, along), want_seams), (pixel, left)


@pytest.mark.gpu
def test_the_stages_take_views_too():
    index = INDEX[f"shape_{B + 1}x{S + 1}"]
    edges = CASES[index].edges
    rows, cols = edges.shape
    wide = torch.from_numpy(np.pad(edges, ((2, 1), (3, 2)), constant_values=0)).cuda()  # zeros around: cheap sums a stray read would take
    assert np.array_equal(words(zg.seam_energy(wide[2:2 + rows, 3:3 + cols])), want_energy(index))
    for pixel in K.PIXELS:
        host = K.pixels_like(1, rows, cols, pixel)
        frame = K.pixels_like(2, rows + 2, cols + 4, pixel)
        dst = torch.from_numpy(frame).cuda()
        src = torch.from_numpy(np.pad(host, ((1, 1), (2, 1)) + ((0, 0),) * (host.ndim - 2))).cuda()
        zg.Image(src[1:1 + rows, 2:2 + cols]).seam_remove(device_words(want_seam(index)), out=dst[1:1 + rows, 3:3 + cols - 1])
        expect = frame.copy()
        expect[1:1 + rows, 3:3 + cols - 1] = R.remove_seam(host, want_seam(index))
        assert same_bytes(dst.cpu().numpy(), expect), pixel


# ---- the host forms ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_the_host_forms():
    for name in ("shape_2x2", "shape_1xN", f"shape_{B + 1}x{S + 1}", "diagonal_valley", "tie_left_eq_right_at_2"):
        index = INDEX[name]
        edges = CASES[index].edges
        energy = zg.seam_energy(edges)
        assert isinstance(energy, np.ndarray) and energy.dtype == np.uint32 and np.array_equal(energy, want_energy(index))
        seam = zg.seam_find(energy, *edges.shape)
        assert seam.dtype == np.uint32 and np.array_equal(seam, want_seam(index))
        for pixel in ("rgb_u8", "f32"):
            host = K.pixels_like(3, *edges.shape, pixel)
            assert same_bytes(zg.Image(host).seam_remove(seam).to_numpy(), R.remove_seam(host, seam))
    for pixel in ("rgba_u8", "rgb_f32"):
        shape, n = (B + 1, 50), 4
        host = K.frame(5, *shape, pixel)
        keep = host.copy()
        for axis, ref, along in (("vertical", R.carve, shape[0]), ("horizontal", R.carve_horizontal, shape[1])):
            seams = np.zeros(n * along, np.uint32)
            got = zg.Image(host).seam_carve(n, axis=axis, seams=seams).to_numpy()
            out, ref_seams = ref(host, n, oracle.sobel)
            assert same_bytes(got, out) and np.array_equal(seams.reshape(n, along), ref_seams), (pixel, axis)
        assert same_bytes(host, keep)
    # a destination view on the host keeps the bytes between cols and stride
    host = K.frame(6, 9, 12, "rgba_u8")
    wide = K.pixels_like(7, 9, 16, "rgba_u8")
    expect = wide.copy()
    expect[:, :10] = R.carve(host, 2, oracle.sobel)[0]
    zg.Image(host).seam_carve(2, out=wide[:, :10])
    assert same_bytes(wide, expect)


# ---- graph capture and replay --------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_a_captured_carve_replays_on_changed_frames_with_eager_calls_in_between():
    shape, n, pixel = (B + 3, S + 5), 3, "rgba_u8"
    src = torch.from_numpy(K.frame(10, *shape, pixel)).cuda()
    dst = torch.zeros((shape[0], shape[1] - n, 4), dtype=torch.uint8, device="cuda")
    seams = new_words(n * shape[0])
    side = torch.cuda.Stream()

    def check(seed, label):
        out, ref_seams = want_carve(shape, pixel, n, seed)
        assert same_bytes(dst.cpu().numpy(), out), label
        assert np.array_equal(words(seams).reshape(n, shape[0]), ref_seams), label

    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):  # the process's first carve of this size may be the captured one
        zg.Image(src).seam_carve(n, out=dst, seams=seams)
    for seed in (11, 12):
        src.copy_(torch.from_numpy(K.frame(seed, *shape, pixel)))
        dst.zero_()
        seams.fill_(-7)
        torch.cuda.synchronize()
        graph.replay()
        torch.cuda.synchronize()
        check(seed, f"replay on frame {seed}")
        # an eager call of the same size takes its scratch from the same cache: the graph's must not be handed out
        got, got_seams = carve_on_device(K.frame(10, *shape, pixel), n)
        out, ref_seams = want_carve(shape, pixel, n, 10)
        assert same_bytes(got, out) and np.array_equal(got_seams, ref_seams)
    del graph
    torch.cuda.synchronize()
    assert zg.lib().zg_release_graph_scratch() == 0


# ---- two streams ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_two_streams_carve_two_frames_at_once():
    jobs = [((2 * B + 1, S + 1), "rgba_u8", 4, 21), ((B + 1, 2 * S + 3), "u8", 4, 22)]
    streams = [torch.cuda.Stream(), torch.cuda.Stream()]
    srcs = [torch.from_numpy(K.frame(seed, *shape, pixel)).cuda() for shape, pixel, _, seed in jobs]
    seams = [new_words(n * shape[0]) for shape, _, n, _ in jobs]
    torch.cuda.synchronize()
    outs = [[], []]
    for _ in range(3):  # both streams stay busy: each call is enqueued behind the other stream's, none is waited for
        for k, ((shape, pixel, n, seed), s) in enumerate(zip(jobs, streams)):
            with torch.cuda.stream(s):
                outs[k].append(zg.Image(srcs[k]).seam_carve(n, seams=seams[k]))
    torch.cuda.synchronize()
    for k, (shape, pixel, n, seed) in enumerate(jobs):
        out, ref_seams = want_carve(shape, pixel, n, seed)
        for got in outs[k]:
            assert same_bytes(got.to_numpy(), out), pixel
        assert np.array_equal(words(seams[k]).reshape(n, shape[0]), ref_seams), pixel


# ---- the operations that share the scratch cache and the Sobel kernels --------------------------------------------------------------------
@pytest.mark.gpu
def test_sobel_canny_and_flood_fill_are_unchanged_by_carves_in_between():
    from tests import flood_cases as FK
    from tests import flood_ref as FR
    host = K.frame(31, 3 * B + 1, 2 * S + 3, "rgba_u8")
    frame = torch.from_numpy(host).cuda()
    fcase = FK.cases(zg.flood_fill_tile())[0]
    fimg = FK.image_of(fcase, "u8")
    fill, thr = FK.fill_of(fcase, "u8"), FK.threshold_of(fcase, "u8")

    def others():
        sobel = zg.Image(frame).sobel().to_numpy()
        canny = zg.Image(frame).canny(1.0, 30, 90).to_numpy()
        dev = torch.from_numpy(fimg).cuda()
        zg.Image(dev).flood_fill(*fcase.seed, fill, thr, 8, "seed")
        return sobel, canny, dev.cpu().numpy()

    before = others()
    assert same_bytes(before[0], oracle.sobel(host)) and same_bytes(before[1], oracle.canny(host, 1.0, 30, 90))
    assert same_bytes(before[2], FR.flood_fill_fast(fimg, *fcase.seed, fill, thr, 8, "seed")[0])
    for pixel, n in (("rgba_u8", 6), ("f32", 2)):
        got, seams = carve_on_device(K.frame(1, *LARGEST, pixel), n)
        ref = R.carve(K.frame(1, *LARGEST, pixel), n, oracle.sobel)
        assert same_bytes(got, ref[0]) and np.array_equal(seams, ref[1])
    after = others()
    for a, b in zip(before, after):
        assert same_bytes(a, b)
