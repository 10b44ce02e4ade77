"""Image metrics without a GPU: the two CPU restatements of tests/metrics_ref.py against each other, the reference's own tests and
hand-computed cases through them, the chunked sequential sum's model against the plain loop, the host arithmetic of the zg_psnr / zg_ssim
entry points (exp, log10, the SSIM window), their argument checks, and the module's boundary (header, bindings, Zig file)."""
import ctypes
import math
import os
import re

import mpmath
import numpy as np
import pytest

import zignal_amd as zg
from zignal_amd import _lib as L
from tests import metrics_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LAYOUTS = [(np.uint8, 1), (np.float32, 1), (np.uint8, 3), (np.uint8, 4), (np.float32, 3), (np.float32, 4)]  # ZG_PIXEL_* order


def image(rng, dtype, ch, rows, cols):
    shape = (rows, cols) if ch == 1 else (rows, cols, ch)
    return rng.integers(0, 256, shape).astype(np.uint8) if dtype == np.uint8 else rng.random(shape, np.float32)


def constant(dtype, ch, rows, cols, value):
    shape = (rows, cols) if ch == 1 else (rows, cols, ch)
    return np.full(shape, value, dtype)


# ---- the two restatements ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype,ch", LAYOUTS)
def test_the_two_restatements_agree(dtype, ch):
    rng = np.random.default_rng(7 + ch)
    a, b = image(rng, dtype, ch, 13, 17), image(rng, dtype, ch, 13, 17)
    assert R.bits(R.mse(a, b)) == R.bits(R.mse_loops(a, b))
    assert R.bits(R.mean_pixel_error(a, b)) == R.bits(R.mean_pixel_error_loops(a, b))
    assert R.bits(R.ssim(a, b)) == R.bits(R.ssim_loops(a, b))
    va, vb = np.ascontiguousarray(a[1:, 2:]), np.ascontiguousarray(b[1:, 2:])  # another shape: 12 x 15
    assert R.bits(R.ssim(va, vb)) == R.bits(R.ssim_loops(va, vb))


def test_the_references_own_tests():
    # "meanPixelError RGB example" (metrics.zig:251-272)
    a, b = np.array([[[255, 0, 0]]], np.uint8), np.zeros((1, 1, 3), np.uint8)
    assert abs(R.mean_pixel_error(a, b) - 1.0 / 3.0) <= 1e-9 and abs(R.mean_pixel_error_loops(a, b) - 1.0 / 3.0) <= 1e-9
    # "ssim rgb scales with luminance" (:274-293)
    a = np.zeros((12, 12, 3), np.uint8)
    r, c = np.indices((12, 12))
    a[(r + c) % 2 == 0] = (255, 0, 0)
    a[(r + c) % 2 == 1] = (0, 255, 0)
    b = np.zeros_like(a)
    assert R.ssim(a, b) < 0.99 and R.ssim_loops(a, b) < 0.99


@pytest.mark.parametrize("dtype,ch", LAYOUTS)
def test_hand_computed_cases(dtype, ch):
    top = 255 if dtype == np.uint8 else 1.0
    # 1 x 1: one pixel at the maximum against zero: every field differs by the maximum
    a, b = constant(dtype, ch, 1, 1, top), constant(dtype, ch, 1, 1, 0)
    assert R.mse(a, b) == float(top) * float(top) and R.mean_pixel_error(a, b) == 1.0
    assert R.psnr(a, b) == 20.0 * math.log10(float(top)) - 10.0 * math.log10(float(top) ** 2)  # 0 dB up to log10's rounding
    assert abs(R.psnr(a, b)) < 1e-12
    assert R.psnr(a, a) == math.inf and R.mean_pixel_error(a, a) == 0.0
    # 11 x 11 (one window). Equal images: 2 mu mu = mu mu + mu mu and 2 sigma = sigma + sigma exactly, so the quotient is 1 wherever the
    # variance did not round below zero; it cannot on a black image
    z = constant(dtype, ch, 11, 11, 0)
    assert R.ssim(z, z) == 1.0 and R.ssim_loops(z, z) == 1.0
    # half the maximum against black: mse = h^2, error = h / max; ssim = c1 c2 / ((mu^2 + c1)(sigma + c2)) with mu the window's mean
    half = 128 if dtype == np.uint8 else 0.5
    h = constant(dtype, ch, 11, 11, half)
    assert R.mse(h, z) == float(half) ** 2 and R.mean_pixel_error(h, z) == float(half) / float(top)
    scalar = float(R.pixel_scalar(h)[0, 0])
    if dtype == np.uint8 and ch > 1:
        assert abs(scalar - 128.0) < 1e-10  # the luma weights add up to 1
    else:
        assert scalar == float(half)
    c1, c2 = (0.01 * top) ** 2, (0.03 * top) ** 2
    want = c1 * c2 / ((scalar ** 2 + c1) * c2)  # a constant image has no variance
    assert abs(R.ssim(h, z) - want) <= 1e-9 * want


def test_rgb_f32_takes_the_mean_branch():
    p = np.array([[[0.25, 0.5, 1.0]]], np.float32)  # meta.isRgb is false for f32 fields (src/meta.zig:146-171)
    assert R.pixel_scalar(p)[0, 0] == (0.25 + 0.5 + 1.0) / 3.0
    q = np.array([[[10, 20, 30, 99]]], np.uint8)    # alpha is not part of the luma
    assert R.pixel_scalar(q)[0, 0] == (0.2126 * (10 / 255.0) + 0.7152 * (20 / 255.0) + 0.0722 * (30 / 255.0)) * 255.0


# ---- the chunked sequential sum: the model against the loop -------------------------------------------------------------------------------
@pytest.mark.parametrize("seed", [1, 2])
def test_the_chunk_model_has_the_loops_bits(seed):
    assert zg.sum_f64_chunk() == 4096  # the model below is run at the library's default chunk
    for name, values, non_negative in R.sum_inputs(seed):
        want = R.bits(R.sequential_sum(values))
        assert R.bits(R.left_to_right(values)) == want, name
        for chunk in (4096, 1024):
            got, serial = R.chunked_sum(values, chunk)
            assert R.bits(got) == want, (name, chunk)
            if non_negative and values.size >= 1 << 20:
                assert serial <= values.size // 25, (name, chunk, serial)  # the first chunk and one or two per binade crossed


def test_the_chunk_model_on_edge_inputs():
    n = 20000
    rng = np.random.default_rng(3)
    edge = np.concatenate(([1024.0], np.tile([1.0, -1.0], n // 2)))  # the sum alternates between 1025 and 1024: a binade's edge
    huge = np.concatenate((np.full(100, 1e-300), np.full(10, 1e300), np.full(100, 1e-300), rng.random(n)))
    zeros_then = np.concatenate((np.zeros(n), rng.random(n)))
    for name, values in (("edge", edge), ("huge", huge), ("zeros_then_values", zeros_then), ("zeros", np.zeros(n)), ("one", np.array([0.1])),
                         ("none", np.zeros(0)), ("negative_zeros", np.full(300, -0.0))):
        want = R.bits(R.sequential_sum(values))
        for chunk in (4096, 64):
            got, serial = R.chunked_sum(values, chunk)
            assert R.bits(got) == want, (name, chunk)
            if name in ("zeros", "negative_zeros", "none"):
                assert serial == 0


def test_the_chunk_model_on_infinities_nan_subnormals_ties_and_2_to_the_53():
    """The kinds tests/test_gpu_metrics.py adds to its SUM_INPUTS, through the model at the library's chunk and at 64: the sum is compared
    with NaN as a class (the loop's NaN and the model's may differ in sign or payload)."""
    n = R.DOMAIN_SUM_N
    for name in R.DOMAIN_SUM_INPUTS:
        values = R.domain_sum_input(name, n)
        assert values.size == n and not values.flags.writeable
        with np.errstate(all="ignore"):
            want = R.sequential_sum(values)
            assert R.same_bits_nan_class(R.left_to_right(values), want), name
            for chunk in (4096, 64):
                got, serial = R.chunked_sum(values, chunk)
                assert R.same_bits_nan_class(got, want), (name, chunk, got, want)
                assert 0 <= serial <= n
                if name == "every_term_a_tie" and chunk == 4096:
                    assert serial <= n // 4, serial  # records carry the parity: most chunks of ties are applied, not added
    # each kind is what its name says
    tiny = 2.0 ** -1022
    with np.errstate(all="ignore"):
        s = {name: R.sequential_sum(R.domain_sum_input(name, n)) for name in R.DOMAIN_SUM_INPUTS}
    assert s["inf_in_the_middle"] == math.inf and math.isnan(s["nan_in_the_middle"]) and math.isnan(s["inf_then_minus_inf"])
    assert s["finite_overflow"] == math.inf and np.isfinite(R.domain_sum_input("finite_overflow", n)).all()
    assert 0 < s["subnormal_sum"] < tiny and R.domain_sum_input("subnormal_into_normal", n).max() < tiny < s["subnormal_into_normal"]
    ties = R.domain_sum_input("every_term_a_tie", n)
    assert 2.0 ** 52 < s["every_term_a_tie"] < 2.0 ** 53 and np.all(ties[1:] % 1.0 == 0.5)
    assert s["reaches_2^53_in_a_chunk"] == 2.0 ** 53 and R.sequential_sum(R.domain_sum_input("reaches_2^53_in_a_chunk", 1000)) == 2.0 ** 53 - 1.0
    assert R.sequential_sum(R.domain_sum_input("chunk_ends_at_2^53-1", 4096)) == 2.0 ** 53 - 1.0 and s["chunk_ends_at_2^53-1"] == 2.0 ** 53
    zeros = R.domain_sum_input("negative_zeros", n)
    assert 0.25 < np.count_nonzero(np.signbit(zeros)) / n < 0.35 and s["negative_zeros"] > 0
    alt = R.domain_sum_input("alternating_positive_sum", n)
    assert np.all(alt[0::2] > 0) and np.all(alt[1::2] <= 0) and s["alternating_positive_sum"] > 0
    for name in R.DOMAIN_SUM_INPUTS:  # defined at every size
        assert [R.domain_sum_input(name, k).size for k in (0, 1, 2)] == [0, 1, 2]


# ---- host arithmetic -----------------------------------------------------------------------------------------------------------------------
def _ulps_from_exact(got: float, exact) -> float:
    return float(abs(mpmath.mpf(got) - exact) / mpmath.mpf(float(np.spacing(abs(float(exact))))))


def test_exp_f64_on_every_argument_of_the_window():
    """musl's exp, which Zig ports, documents an error below 1 ulp, not correct rounding: the restatement is held to that bound against the
    exact value, and to the correctly rounded value wherever musl's own rounding allows (19 of the 20 arguments; exp(-10 / 4.5) is off by
    one unit at 0.518 ulp from the exact value)."""
    mpmath.mp.prec = 300
    lib = zg.lib()
    args = sorted({-(x * x + y * y) / (2.0 * 1.5 * 1.5) for x in range(6) for y in range(6)})
    assert len(args) == 20
    correctly_rounded = 0
    for a in args:
        exact = mpmath.exp(mpmath.mpf(a))
        got = lib.zg_exp_f64_host(a)
        assert _ulps_from_exact(got, exact) < 1.0, a
        correctly_rounded += got == float(exact)
    assert correctly_rounded >= 19
    assert lib.zg_exp_f64_host(0.0) == 1.0 and lib.zg_exp_f64_host(-math.inf) == 0.0 and lib.zg_exp_f64_host(math.inf) == math.inf
    assert math.isnan(lib.zg_exp_f64_host(math.nan)) and lib.zg_exp_f64_host(-800.0) == 0.0 and lib.zg_exp_f64_host(800.0) == math.inf


def test_the_window_is_built_as_the_reference_builds_it():
    lib = zg.lib()
    w = zg.ssim_window()
    assert w.shape == (11, 11) and w.dtype == np.float64
    g = np.array([[lib.zg_exp_f64_host(-(float(dx - 5) ** 2 + float(dy - 5) ** 2) / (2.0 * 1.5 * 1.5)) for dx in range(11)] for dy in range(11)])
    want = g / R.sequential_sum(g)  # :247: one division each by the left-to-right sum
    assert np.array_equal(w.view(np.uint64), want.view(np.uint64))
    ref = R.ssim_window().reshape(11, 11)  # the correctly rounded exponentials: a last-place matter
    assert np.max(np.abs(w - ref) / ref) < 4 * np.finfo(np.float64).eps
    assert np.array_equal(w, w.T) and np.array_equal(w, w[::-1, ::-1]) and w[5, 5] == w.max()
    assert lib.zg_ssim_window_host(None) == L.ERR_INVALID_ARGUMENT


def test_log10_f64_on_a_sweep():
    """musl's log10: below 1 ulp of the exact value (its documented bound) over mse-like and max-like arguments; exact at powers of ten that
    the algorithm reaches exactly."""
    mpmath.mp.prec = 300
    lib = zg.lib()
    rng = np.random.default_rng(5)
    xs = np.concatenate((np.exp(rng.uniform(-40, 40, 6000)), rng.uniform(0, 65025, 3000), rng.uniform(0.5, 2.0, 3000), [255.0, 65025.0, 10.0, 100.0, 1e-5, 5e-324]))
    worst = 0.0
    for x in xs.tolist():
        exact = mpmath.log10(mpmath.mpf(x))
        got = lib.zg_log10_f64_host(x)
        if exact == 0:
            assert got == 0.0
            continue
        worst = max(worst, _ulps_from_exact(got, exact))
    print(f"log10_f64: worst error {worst:.4f} ulp over {xs.size} arguments")
    assert worst < 1.0
    assert lib.zg_log10_f64_host(1.0) == 0.0 and lib.zg_log10_f64_host(0.0) == -math.inf and lib.zg_log10_f64_host(math.inf) == math.inf
    assert math.isnan(lib.zg_log10_f64_host(-1.0)) and math.isnan(lib.zg_log10_f64_host(math.nan))


def test_psnr_from_mse():
    lib = zg.lib()
    assert zg.psnr_from_mse(0.0, 255.0) == math.inf and zg.psnr_from_mse(-0.0, 1.0) == math.inf
    for mse, mx in ((1.0, 255.0), (0.25, 1.0), (123.456, 255.0), (1e-9, 1.0)):
        want = 20.0 * lib.zg_log10_f64_host(mx) - 10.0 * lib.zg_log10_f64_host(mse)  # :53, as written
        assert R.bits(zg.psnr_from_mse(mse, mx)) == R.bits(want)
        assert abs(zg.psnr_from_mse(mse, mx) - R.psnr_from_mse(mse, mx)) <= 1e-12 * max(1.0, abs(want))
    assert math.isnan(zg.psnr_from_mse(math.nan, 1.0))


# ---- argument errors, answered without a device --------------------------------------------------------------------------------------------
def _has_device():
    return zg.lib().zg_device_count() > 0


def test_the_metrics_decide_their_status_before_anything_is_enqueued():
    lib = zg.lib()
    pa, pb = np.zeros((12, 16), np.uint8), np.zeros((12, 16), np.uint8)
    a, b = L.ZgImage(pa.ctypes.data, 16, 12, 16, L.PIXEL_U8), L.ZgImage(pb.ctypes.data, 16, 12, 16, L.PIXEL_U8)
    res = L.ZgMetricResult(1.0, 2, 3.0, 4)
    value = ctypes.c_double(7.0)
    device = {n: (lambda x, y, n=n: getattr(lib, f"zg_{n}")(x, y, None, ctypes.byref(res), None)) for n in ("psnr", "mean_pixel_error", "ssim")}
    host = {n: (lambda x, y, n=n: getattr(lib, f"zg_{n}_host")(x, y, None, ctypes.byref(value), ctypes.byref(res))) for n in ("psnr", "mean_pixel_error", "ssim")}
    for calls in (device, host):
        for name, call in calls.items():
            assert call(None, ctypes.byref(b)) == L.ERR_INVALID_ARGUMENT and call(ctypes.byref(a), None) == L.ERR_INVALID_ARGUMENT
            other = L.ZgImage(pb.ctypes.data, 16, 12, 16, L.PIXEL_F32)
            assert call(ctypes.byref(a), ctypes.byref(other)) == L.ERR_INVALID_ARGUMENT, name  # two pixel types
            for rows, cols in ((12, 15), (11, 16)):
                assert call(ctypes.byref(a), ctypes.byref(L.ZgImage(pb.ctypes.data, 16, rows, cols, L.PIXEL_U8))) == L.ERR_DIMENSION_MISMATCH, name
            bad = L.ZgImage(pa.ctypes.data, 8, 12, 16, L.PIXEL_U8)  # stride below cols
            assert call(ctypes.byref(bad), ctypes.byref(b)) == L.ERR_INVALID_ARGUMENT
        for rows, cols in ((10, 16), (12, 10), (1, 1)):  # error.ImageTooSmall
            sa, sb = L.ZgImage(pa.ctypes.data, 16, rows, cols, L.PIXEL_U8), L.ZgImage(pb.ctypes.data, 16, rows, cols, L.PIXEL_U8)
            assert calls["ssim"](ctypes.byref(sa), ctypes.byref(sb)) == L.ERR_INVALID_ARGUMENT
            assert b"ImageTooSmall" in lib.zg_last_error()
        # a mismatch is reported before the size, as in the reference (:57-62)
        sa, sb = L.ZgImage(pa.ctypes.data, 16, 5, 5, L.PIXEL_U8), L.ZgImage(pb.ctypes.data, 16, 5, 6, L.PIXEL_U8)
        assert calls["ssim"](ctypes.byref(sa), ctypes.byref(sb)) == L.ERR_DIMENSION_MISMATCH
        # nearly 2^60 u8 components of up to 255^2 could pass 2^53; nothing is touched
        side = (1 << 30) - 1
        ha, hb = L.ZgImage(pa.ctypes.data, side, side, side, L.PIXEL_U8), L.ZgImage(pb.ctypes.data, side, side, side, L.PIXEL_U8)
        assert calls["psnr"](ctypes.byref(ha), ctypes.byref(hb)) == L.ERR_UNSUPPORTED
        assert calls["mean_pixel_error"](ctypes.byref(ha), ctypes.byref(hb)) == L.ERR_UNSUPPORTED
    for name in device:
        assert getattr(lib, f"zg_{name}")(ctypes.byref(a), ctypes.byref(b), None, None, None) == L.ERR_INVALID_ARGUMENT  # null result
        assert getattr(lib, f"zg_{name}_host")(ctypes.byref(a), ctypes.byref(b), None, None, None) == L.ERR_INVALID_ARGUMENT  # null value
    values = np.zeros(128)
    assert lib.zg_sum_f64_sequential(values.ctypes.data, 128, 0, None, None) == L.ERR_INVALID_ARGUMENT
    assert lib.zg_sum_f64_sequential(None, 128, 0, ctypes.byref(res), None) == L.ERR_INVALID_ARGUMENT
    for log2 in (1, 5, 17, 40):
        assert lib.zg_sum_f64_sequential(values.ctypes.data, 128, log2, ctypes.byref(res), None) == L.ERR_INVALID_ARGUMENT, log2
    assert lib.zg_sum_f64_sequential(values.ctypes.data, 1 << 40, 0, ctypes.byref(res), None) == L.ERR_UNSUPPORTED
    assert (res.sum, res.count, res.value, res.serial_terms, value.value) == (1.0, 2, 3.0, 4, 7.0)
    with pytest.raises(zg.DimensionMismatch):
        zg.Image(pa).psnr(zg.Image(pb[:, :15]))
    with pytest.raises(zg.InvalidArgument):
        zg.Image(pa[:10]).ssim(zg.Image(pb[:10]))
    with pytest.raises(ValueError):
        zg.Image(pa).ssim(zg.Image(pb), map=np.zeros((3, 3)))
    with pytest.raises(ValueError):
        zg.Image(pa).ssim(zg.Image(pb), window=np.zeros(120))
    with pytest.raises(ValueError):
        zg.Image(pa).psnr(zg.Image(pb), result=np.zeros(4))
    if not _has_device():  # the argument errors first, then the missing device
        for calls in (device, host):
            for call in calls.values():
                assert call(ctypes.byref(a), ctypes.byref(b)) == L.ERR_HIP
        assert lib.zg_sum_f64_sequential(values.ctypes.data, 128, 0, ctypes.byref(res), None) == L.ERR_HIP
        with pytest.raises(zg.ZignalError):
            zg.Image(pa).mean_pixel_error(zg.Image(pb))


def test_the_structs_mirror_the_header():
    assert ctypes.sizeof(L.ZgMetricResult) == 32 and R.bits(1.0) == 0x3FF0000000000000
    assert [getattr(L.ZgMetricResult, n).offset for n in ("sum", "count", "value", "serial_terms")] == [0, 8, 16, 24]
    assert ctypes.sizeof(L.ZgMetricOptions) == 16 and [getattr(L.ZgMetricOptions, n).offset for n in ("ssim_window", "ssim_map")] == [0, 8]
    assert zg.METRIC_RESULT_DTYPE.itemsize == 32 and zg.METRIC_RESULT_DTYPE.names == ("sum", "count", "value", "serial_terms")
    chunk = zg.sum_f64_chunk()
    assert chunk & (chunk - 1) == 0 and 64 <= chunk <= 1 << 16


# ---- the module's boundary -----------------------------------------------------------------------------------------------------------
def _metrics_header():
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "zignal_hip_metrics.h")).read(), flags=re.S)
    protos = re.findall(r"ZG_API\s+[\w\s\*]+?\b(zg_\w+)\s*\(([^;]*?)\)\s*;", text, flags=re.S)
    return {name: ([] if args.strip() == "void" else args.split(",")) for name, args in protos}


def test_metrics_header_bindings_and_zig_file_declare_the_same_symbols():
    protos = _metrics_header()
    assert sorted(protos) == sorted(L.METRICS_EXPORTED_SYMBOLS) and len(protos) == 12
    raw = ctypes.CDLL(L.LIB_PATH)
    for name, args in protos.items():
        assert hasattr(raw, name), f"{name} declared in include/zignal_hip_metrics.h but not exported"
        assert len(L._METRICS_SIGNATURES[name]) == len(args), name
        assert getattr(zg.lib(), name).argtypes is not None or not args
    others = (set(L.EXPORTED_SYMBOLS) | set(L.ORB_EXPORTED_SYMBOLS) | set(L.MATCH_EXPORTED_SYMBOLS) | set(L.HOUGH_EXPORTED_SYMBOLS)
              | set(L.FLOOD_EXPORTED_SYMBOLS))
    assert not set(L.METRICS_EXPORTED_SYMBOLS) & others
    shim = open(os.path.join(ROOT, "zig", "zignal_hip_metrics.zig")).read()
    externs = dict(re.findall(r"pub extern fn (zg_\w+)\(([^)]*)\)", shim))
    assert set(externs) == set(protos)
    for name, args in externs.items():
        assert len([a for a in args.split(",") if a.strip()]) == len(protos[name]), name
    main = open(os.path.join(ROOT, "include", "zignal_hip.h")).read()
    assert main.index('#include "zignal_hip_flood.h"') < main.index('#include "zignal_hip_metrics.h"')
    assert os.path.isfile(os.path.join(ROOT, "zignal_amd", "csrc", "metrics.hip"))
    source = open(os.path.join(ROOT, "zignal_amd", "csrc", "metrics.hip")).read()
    assert '#include "zg_scan.h"' in source and "ScratchBlock" in source and "hipMalloc" not in source and "hipMemcpy" not in source
