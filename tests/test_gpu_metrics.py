"""Image.psnr / ssim / mean_pixel_error and zg_sum_f64_sequential on the device against tests/metrics_ref.py, bit for bit: the sum on
every kind of input at sizes around the chunk, the three metrics on all six pixel types, views with two strides, the SSIM map, a caller's
window, the host forms, a captured blur -> ssim chain replayed on changed frames, and how many terms the sum adds serially."""
import functools
import math

import numpy as np
import pytest

import zignal_amd as zg
from zignal_amd import metrics as M
from tests import metrics_ref as R

try:
    import torch
except Exception:  # pragma: no cover
    torch = None

CHUNK = zg.sum_f64_chunk()  # a host constant of the library: no GPU needed to read it
LAYOUTS = {"u8": (np.uint8, 1), "f32": (np.float32, 1), "rgb_u8": (np.uint8, 3), "rgba_u8": (np.uint8, 4), "rgb_f32": (np.float32, 3),
           "rgba_f32": (np.float32, 4)}
N_LARGE = (1 << 20) + 37


def record(t):
    return M._record(t)


def new_result(device="cuda"):
    return torch.full((4,), -1.0, dtype=torch.float64, device=device)


# ---- the sequential sum ---------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def sum_input(name, n):
    """(values, non-negative?) — built once, never written."""
    if name in R.DOMAIN_SUM_INPUTS:
        return R.domain_sum_input(name, n, CHUNK), False
    rng = np.random.default_rng(len(name) * 1000 + n % 997)
    non_negative = True
    if name == "uniform":
        v = rng.random(n)
    elif name == "squared_f32_differences":  # a tie in about every second chunk
        d = rng.random(n, np.float32).astype(np.float64) - rng.random(n, np.float32).astype(np.float64)
        v = d * d
    elif name == "mixed_signs":
        v, non_negative = rng.standard_normal(n), False
    elif name == "all_negative":
        v, non_negative = -rng.random(n), False
    elif name == "all_zero":
        v = np.zeros(n)
    elif name == "zeros_then_values":
        v = np.concatenate((np.zeros(n // 2), rng.random(n - n // 2)))
    elif name == "tiny_and_huge":
        v = rng.random(n)
        v[: n // 3] = 1e-300
        v[n // 3: n // 3 + 5] = 1e300
    elif name == "binade_edge":  # 1024, then the sum alternates between 1025 and 1024
        v, non_negative = np.tile([1.0, -1.0], n // 2 + 1)[:n].copy(), False
        if n:
            v[0] = 1024.0
    else:
        raise KeyError(name)
    v.setflags(write=False)
    return v, non_negative


ORDINARY_SUM_INPUTS = ("uniform", "squared_f32_differences", "mixed_signs", "all_negative", "all_zero", "zeros_then_values", "tiny_and_huge", "binade_edge")
# infinities, NaN, overflow, subnormal sums, chunks of ties, sums around 2^53, -0.0 terms (tests/metrics_ref.py: domain_sum_input; the numpy
# model runs the same kinds in tests/test_metrics_oracle.py). Several of them are added serially from the first special term on, so they run
# at R.DOMAIN_SUM_N terms and at the sizes around a chunk, not at N_LARGE.
SUM_INPUTS = ORDINARY_SUM_INPUTS + R.DOMAIN_SUM_INPUTS


def check_sum(name, n):
    values, non_negative = sum_input(name, n)
    with np.errstate(all="ignore"):
        want = R.sequential_sum(values)
    dev = torch.from_numpy(values.copy()).cuda()
    for chunk_log2 in (0, 6):
        got = zg.sum_f64_sequential(dev, chunk_log2)
        # bit for bit, every NaN one class (x86 and gfx950 differ in the NaN they make and pass on)
        assert R.same_bits_nan_class(float(got["sum"]), want), (name, n, chunk_log2, float(got["sum"]).hex(), want.hex())
        assert R.same_bits_nan_class(float(got["value"]), want) and int(got["count"]) == n
        serial = int(got["serial_terms"])
        assert 0 <= serial <= n
        if name == "all_zero":
            assert serial <= (CHUNK if chunk_log2 == 0 else 64)
        # a condition on the algorithm, not a timing: the first chunk and one or two per binade crossed; the CPU model stays below n / 25
        if chunk_log2 == 0 and non_negative and n >= 1 << 20:
            assert serial <= n // 8, (name, serial)


@pytest.mark.gpu
@pytest.mark.parametrize("name", ORDINARY_SUM_INPUTS)
def test_the_sequential_sum_has_the_loops_bits(name):
    check_sum(name, N_LARGE)


@pytest.mark.gpu
@pytest.mark.parametrize("name", R.DOMAIN_SUM_INPUTS)
def test_the_sequential_sum_on_infinities_nan_subnormals_ties_and_2_to_the_53(name):
    check_sum(name, R.DOMAIN_SUM_N)


@pytest.mark.gpu
@pytest.mark.parametrize("n", [0, 1, CHUNK - 1, CHUNK, CHUNK + 1])
def test_the_sequential_sum_at_sizes_around_a_chunk(n):
    for name in SUM_INPUTS:
        check_sum(name, n)


@pytest.mark.gpu
def test_the_sequential_sum_fills_a_result_tensor_without_synchronising():
    values, _ = sum_input("uniform", 5000)
    dev = torch.from_numpy(values.copy()).cuda()
    res = new_result()
    assert zg.sum_f64_sequential(dev, 0, result=res) is res
    torch.cuda.synchronize()
    assert R.bits(float(record(res)["sum"])) == R.bits(R.sequential_sum(values))
    with pytest.raises(ValueError):
        zg.sum_f64_sequential(dev.float())
    with pytest.raises(zg.InvalidArgument):
        zg.sum_f64_sequential(dev, 3)


# ---- images -------------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def pair(layout, rows, cols, seed=0):
    """Two images of a layout: b is a disturbed a (most components equal or close), both read-only."""
    dtype, ch = LAYOUTS[layout]
    rng = np.random.default_rng(seed * 100 + rows + cols + ch)
    shape = (rows, cols) if ch == 1 else (rows, cols, ch)
    if dtype == np.uint8:
        a = rng.integers(0, 256, shape).astype(np.uint8)
        b = np.clip(a.astype(np.int32) + rng.integers(-9, 10, shape) * (rng.random(shape) < 0.6), 0, 255).astype(np.uint8)
    else:
        a = rng.random(shape, np.float32)
        b = (a + (rng.random(shape, np.float32) - np.float32(0.5)) * np.float32(0.1) * (rng.random(shape) < 0.6)).astype(np.float32)
    a.setflags(write=False)
    b.setflags(write=False)
    return a, b


def dev_image(a):
    return zg.Image(torch.from_numpy(np.array(a)).cuda())


def dev_view(a, top, left, extra_rows, extra_cols, seed):
    """`a` as a view of a larger device frame whose other pixels are garbage (NaN for floats)."""
    rng = np.random.default_rng(seed)
    shape = (a.shape[0] + top + extra_rows, a.shape[1] + left + extra_cols) + a.shape[2:]
    frame = rng.integers(0, 256, shape).astype(np.uint8) if a.dtype == np.uint8 else np.full(shape, np.nan, np.float32)
    frame[top:top + a.shape[0], left:left + a.shape[1]] = a
    t = torch.from_numpy(frame).cuda()
    return zg.Image(t[top:top + a.shape[0], left:left + a.shape[1]])


def check_difference_metrics(a, b, ia, ib):
    mx = R.component_max(a)
    terms_sq, terms_abs = R.difference_terms(a, b, True), R.difference_terms(a, b, False)
    res = new_result()
    assert ia.psnr(ib, result=res) is res
    r = record(res)
    want_sum = R.left_to_right(terms_sq)
    assert R.bits(float(r["sum"])) == R.bits(want_sum) and int(r["count"]) == terms_sq.size
    assert R.bits(float(r["value"])) == R.bits(R.mse(a, b))
    if a.dtype == np.uint8:
        assert int(r["serial_terms"]) == 0
    got = ia.psnr(ib)
    assert R.bits(got) == R.bits(zg.psnr_from_mse(R.mse(a, b), mx))
    want = R.psnr(a, b)
    assert got == want or abs(got - want) <= 1e-12 * abs(want)  # log10 is not pinned at the last ulp
    ia.mean_pixel_error(ib, result=res)
    r = record(res)
    assert R.bits(float(r["sum"])) == R.bits(R.left_to_right(terms_abs)) and int(r["count"]) == terms_abs.size
    assert R.bits(float(r["value"])) == R.bits(R.mean_pixel_error(a, b))
    assert R.bits(ia.mean_pixel_error(ib)) == R.bits(R.mean_pixel_error(a, b))


@pytest.mark.gpu
@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("rows,cols", [(37, 53), (1021, 1031)])
def test_psnr_and_mean_pixel_error_equal_the_reference(layout, rows, cols):
    a, b = pair(layout, rows, cols)
    check_difference_metrics(a, b, dev_image(a), dev_image(b))


@pytest.mark.gpu
@pytest.mark.parametrize("layout", LAYOUTS)
def test_psnr_and_mean_pixel_error_on_views_with_two_strides(layout):
    a, b = pair(layout, 67, 131)
    check_difference_metrics(a, b, dev_view(a, 3, 5, 2, 7, 1), dev_view(b, 0, 1, 4, 13, 2))
    check_difference_metrics(a, b, dev_image(a), dev_view(b, 1, 0, 0, 3, 3))


@pytest.mark.gpu
@pytest.mark.parametrize("layout", LAYOUTS)
def test_identical_images_and_a_single_differing_pixel(layout):
    a, _ = pair(layout, 129, 257)
    ia = dev_image(a)
    res = new_result()
    assert ia.psnr(dev_image(a)) == math.inf and ia.mean_pixel_error(dev_image(a)) == 0.0
    if a.dtype != np.uint8:  # chunks of zeros are skipped whatever the sum: identical images add nothing serially
        ia.psnr(dev_image(a), result=res)
        assert int(record(res)["serial_terms"]) == 0 and float(record(res)["sum"]) == 0.0
    b = a.copy()
    b[77, 200] = 0 if a.dtype == np.uint8 else np.float32(0.0)
    if np.array_equal(a, b):
        b[77, 200] = 1
    check_difference_metrics(a, b, ia, dev_image(b))
    b = a.copy()
    b[-1, -1] = 255 - a[-1, -1] if a.dtype == np.uint8 else np.float32(1.0) - a[-1, -1]  # the last term of all
    check_difference_metrics(a, b, ia, dev_image(b))


@pytest.mark.gpu
def test_the_host_forms_return_the_references_values():
    for layout in LAYOUTS:
        a, b = pair(layout, 37, 53)
        got = zg.Image(a).psnr(zg.Image(b))
        assert R.bits(got) == R.bits(zg.psnr_from_mse(R.mse(a, b), R.component_max(a)))
        assert R.bits(zg.Image(a).mean_pixel_error(zg.Image(b))) == R.bits(R.mean_pixel_error(a, b))
        frame = np.zeros((40, 60) + a.shape[2:], a.dtype)
        frame[2:39, 4:57] = b
        assert R.bits(zg.Image(a).mean_pixel_error(zg.Image(frame[2:39, 4:57]))) == R.bits(R.mean_pixel_error(a, b))
        window = zg.ssim_window()
        m = np.full((27, 43), -1.0)
        assert R.bits(zg.Image(a).ssim(zg.Image(b), map=m)) == R.bits(R.ssim(a, b, window))
        assert np.array_equal(m.view(np.uint64), R.ssim_map(a, b, window).view(np.uint64))


# ---- ssim ------------------------------------------------------------------------------------------------------------------------------------
def check_ssim(a, b, ia, ib, window=None):
    """window None: the library's own table (held to the reference's construction in tests/test_metrics_oracle.py)."""
    w = zg.ssim_window() if window is None else window
    want_map = R.ssim_map(a, b, w)
    ssim_map = torch.full(want_map.shape, -7.0, dtype=torch.float64, device="cuda")
    res = new_result()
    assert ia.ssim(ib, map=ssim_map, result=res, window=window) is res
    r = record(res)
    got_map = ssim_map.cpu().numpy()
    same = got_map.view(np.uint64) == want_map.view(np.uint64)
    assert same.all(), (np.argwhere(~same)[:4], got_map[~same][:4], want_map[~same][:4])
    assert R.bits(float(r["sum"])) == R.bits(R.left_to_right(want_map)) and int(r["count"]) == want_map.size
    assert R.bits(float(r["value"])) == R.bits(R.ssim(a, b, w))
    assert R.bits(ia.ssim(ib, window=window)) == R.bits(R.ssim(a, b, w))  # the map in scratch


@pytest.mark.gpu
@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("rows,cols", [(11, 11), (12, 75), (139, 523)])
def test_ssim_equals_the_reference(layout, rows, cols):
    a, b = pair(layout, rows, cols)
    check_ssim(a, b, dev_image(a), dev_image(b))


@pytest.mark.gpu
@pytest.mark.parametrize("layout", LAYOUTS)
def test_ssim_on_views_and_with_a_callers_window(layout):
    a, b = pair(layout, 43, 91)
    check_ssim(a, b, dev_view(a, 3, 5, 2, 7, 4), dev_view(b, 0, 1, 4, 13, 5))
    check_ssim(a, b, dev_image(a), dev_image(b), R.ssim_window().reshape(11, 11))  # the correctly rounded exponentials, as a Zig host would pass its own
    flat = np.full(121, 1.0 / 121.0)
    check_ssim(a, b, dev_image(a), dev_view(b, 1, 1, 1, 1, 6), flat)


@pytest.mark.gpu
def test_ssim_of_the_references_luminance_test_and_of_equal_images():
    a = np.zeros((12, 12, 3), np.uint8)  # "ssim rgb scales with luminance" (metrics.zig:274-293)
    r, c = np.indices((12, 12))
    a[(r + c) % 2 == 0] = (255, 0, 0)
    a[(r + c) % 2 == 1] = (0, 255, 0)
    b = np.zeros_like(a)
    got = dev_image(a).ssim(dev_image(b))
    assert got < 0.99 and R.bits(got) == R.bits(R.ssim(a, b, zg.ssim_window()))
    z = np.zeros((64, 80), np.float32)
    assert dev_image(z).ssim(dev_image(z)) == 1.0
    with pytest.raises(zg.InvalidArgument):
        dev_image(z[:10]).ssim(dev_image(z[:10]))
    with pytest.raises(zg.DimensionMismatch):
        dev_image(z).ssim(dev_image(z[:, :70]))


# ---- a captured chain --------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_blur_then_ssim_replays_from_a_graph_on_changed_frames():
    rows, cols = 75, 139
    src = torch.zeros((rows, cols, 4), dtype=torch.uint8, device="cuda")
    blurred = torch.zeros_like(src)
    res, mpe = new_result(), new_result()
    side = torch.cuda.Stream()

    def enqueue():
        zg.Image(src).gaussian_blur(1.2, zg.Image(blurred))
        zg.Image(src).ssim(zg.Image(blurred), result=res)
        zg.Image(src).mean_pixel_error(zg.Image(blurred), result=mpe)

    def check(what):
        a, b = src.cpu().numpy(), blurred.cpu().numpy()
        assert R.bits(float(record(res)["value"])) == R.bits(R.ssim(a, b, zg.ssim_window())), what
        assert R.bits(float(record(mpe)["value"])) == R.bits(R.mean_pixel_error(a, b)), what

    def load(seed):
        src.copy_(torch.from_numpy(np.array(pair("rgba_u8", rows, cols, seed)[0])))

    load(1)
    torch.cuda.synchronize()
    with torch.cuda.stream(side):
        enqueue()  # warm-up outside the capture
    side.synchronize()
    check("eager")
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        enqueue()
    for seed in (2, 3):
        load(seed)
        res.fill_(-1.0)
        torch.cuda.synchronize()
        graph.replay()
        torch.cuda.synchronize()
        check(f"replay on frame {seed}")
    del graph
    torch.cuda.synchronize()
    assert zg.lib().zg_release_graph_scratch() == 0
