"""Flood fill without a GPU: the two CPU restatements of Image(T).floodFill (tests/flood_ref.py) against each other on every shared
case and against scipy's labelling, the reference's own four test scenarios, zg_flood_fill_bound_host against a brute-force table and
against square-root probes, the argument checks of the zg_flood_fill* entry points, and the module's boundary (header, bindings, Zig file)."""
import ctypes
import math
import os
import re

import numpy as np
import pytest
from scipy import ndimage

import zignal_amd as zg
from zignal_amd import _lib as L
from tests import flood_cases as K
from tests import flood_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
T = zg.flood_fill_tile()
CASES = K.cases(T)
LITERAL_ALL_TYPES_BELOW = 4096  # pixels: the literal loop is Python; larger frames take two pixel types each, in rotation


def same_bytes(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def literal_pixels(index, case):
    px = K.pixels_of(case)
    if len(px) == 1 or case.plane.size < LITERAL_ALL_TYPES_BELOW:
        return px
    return (px[index % 6], px[(index + 3) % 6])


def test_the_tile_side_is_a_host_constant():
    assert T == zg.lib().zg_flood_fill_tile() and T >= 8 and T & (T - 1) == 0


@pytest.mark.parametrize("index", range(len(CASES)), ids=[c.name for c in CASES])
def test_the_two_restatements_agree(index):
    case = CASES[index]
    for pixel in literal_pixels(index, case):
        img, fill, thr = K.image_of(case, pixel), K.fill_of(case, pixel), K.threshold_of(case, pixel)
        for mode in K.MODES:
            for conn in K.CONNECTIVITIES:
                a, na = R.flood_fill_literal(img, *case.seed, fill, thr, conn, mode)
                b, nb = R.flood_fill_fast(img, *case.seed, fill, thr, conn, mode)
                assert same_bytes(a, b) and na == nb >= 1, (pixel, mode, conn)
                assert same_bytes(img, K.image_of(case, pixel))  # neither wrote its input


def test_the_large_cases_cover_all_six_pixel_types_between_them():
    seen = set()
    for index, case in enumerate(CASES):
        if case.pixel is None and case.plane.size >= LITERAL_ALL_TYPES_BELOW:
            seen |= set(literal_pixels(index, case))
    assert seen == set(K.PIXELS)


@pytest.mark.parametrize("index", range(len(CASES)), ids=[c.name for c in CASES])
def test_seed_mode_is_scipys_component_of_the_pass_mask(index):
    case = CASES[index]
    four = ndimage.generate_binary_structure(2, 1)
    eight = ndimage.generate_binary_structure(2, 2)
    for pixel in K.pixels_of(case):
        img, fill, thr = K.image_of(case, pixel), K.fill_of(case, pixel), K.threshold_of(case, pixel)
        ok = R.pass_mask(img, *case.seed, thr)  # the seed is forced in
        assert ok[case.seed]
        for conn, structure in ((4, four), (8, eight)):
            labels, _ = ndimage.label(ok, structure)
            want = labels == labels[case.seed]
            assert np.array_equal(R.filled_mask(img, *case.seed, thr, conn, "seed"), want), (pixel, conn)
            if img.size < LITERAL_ALL_TYPES_BELOW:
                out, n = R.flood_fill_literal(img, *case.seed, fill, thr, conn, "seed")
                expect = img.copy()
                expect[want] = fill
                assert same_bytes(out, expect) and n == int(want.sum()), (pixel, conn)


def test_the_cases_are_what_their_names_say():
    by_name = {c.name: c for c in CASES}
    sides = (T - 1, T, T + 1, 2 * T + 1)
    for rows in sides:
        for cols in sides:
            assert by_name[f"shape_{rows}x{cols}"].plane.shape == (rows, cols)
    assert by_name["shape_1xN"].plane.shape == (1, 2 * T + 1) and by_name["shape_Nx1"].plane.shape == (2 * T + 1, 1)
    assert max(max(c.plane.shape) for c in CASES if c.plane is not None) <= 4 * T

    def count(name, conn, mode, pixel="u8"):
        c = by_name[name]
        return int(R.filled_mask(K.image_of(c, pixel), *c.seed, K.threshold_of(c, pixel), conn, mode).sum())

    spiral = by_name["spiral"]
    assert min(spiral.plane.shape) >= 3 * T and count("spiral", 4, "seed") == int((spiral.plane == K.FLOOR).sum()) > T * T
    assert count("spiral_from_the_centre", 4, "neighbor") == count("spiral", 4, "seed")
    comb = by_name["comb"].plane
    assert count("comb", 4, "seed") == int((comb == K.FLOOR).sum()) and comb.shape[0] > T and comb.shape[1] > 2 * T
    for corner in ("tl", "tr", "bl", "br"):
        c = by_name[f"four_edges_seed_{corner}"]
        mask = R.filled_mask(c.plane, *c.seed, 0.0, 4, "seed")
        assert mask[0, :].all() and mask[-1, :].all() and mask[:, 0].all() and mask[:, -1].all() and not mask.all()
    assert {by_name[f"tile_corner_seed_{d}"].seed for d in ("nw", "ne", "sw", "se")} == {(T - 1, T - 1), (T - 1, T), (T, T - 1), (T, T)}
    board = by_name["checkerboard"].plane
    for mode in K.MODES:
        assert count("checkerboard", 4, mode) == 1 and count("checkerboard", 8, mode) == int((board == board[1, 1]).sum()) == board.size // 2
    for name in ("corner_link_main", "corner_link_anti"):
        for mode in K.MODES:
            for pixel in K.PIXELS:
                assert count(name, 4, mode, pixel) == 16 and count(name, 8, mode, pixel) == 32
    for name in ("ramp_across", "ramp_down"):
        assert count(name, 4, "neighbor") == by_name[name].plane.size and count(name, 4, "seed") == 3 * 3
    for name, t in (("zero", 0.0), ("minus_zero", -0.0), ("minus_one", -1.0), ("nan", math.nan), ("inf", math.inf)):
        c = by_name[f"threshold_{name}"]
        assert repr(float(c.threshold)) == repr(float(t))
    for pixel in K.PIXELS:
        assert count("threshold_minus_one", 8, "neighbor", pixel) == 1 == count("threshold_nan", 8, "seed", pixel)
        assert count("threshold_inf", 4, "seed", pixel) == by_name["threshold_inf"].plane.size
        assert count("threshold_zero", 8, "seed", pixel) == count("threshold_minus_zero", 8, "seed", pixel) > 1
    c = by_name["fill_equals_seed"]
    for pixel in K.PIXELS:
        img = K.image_of(c, pixel)
        assert np.array_equal(np.asarray(K.fill_of(c, pixel), img.dtype), img[c.seed])
        out, n = R.flood_fill_fast(img, *c.seed, K.fill_of(c, pixel), K.threshold_of(c, pixel), 4, "seed")
        assert n > 1
    c = by_name["region_already_holds_fill"]
    for pixel in K.PIXELS:
        img = K.image_of(c, pixel)
        mask = R.filled_mask(img, *c.seed, K.threshold_of(c, pixel), 8, "seed")
        holds = (img.reshape(img.shape[0], img.shape[1], -1) == np.asarray(K.fill_of(c, pixel), img.dtype).reshape(1, 1, -1)).all(axis=2)
        assert (mask & holds).any() and (mask & ~holds).any()
    # the thresholds at sqrt(s): one more pixel joins at the threshold than just below it
    for pixel, names in (("rgb_u8", ("sqrt3", "sqrt50", "sqrt51")), ("rgba_u8", ("sqrt25", "sqrt49")), ("rgb_f32", ("step0", "step1", "step2")),
                         ("rgba_f32", ("step0", "step1", "step2"))):
        for name in names:
            at, below = by_name[f"{pixel}_{name}"], by_name[f"{pixel}_{name}_below"]
            assert below.threshold == math.nextafter(at.threshold, 0.0)
            n_at = int(R.filled_mask(at.image, *at.seed, at.threshold, 4, "seed").sum())
            n_below = int(R.filled_mask(below.image, *below.seed, below.threshold, 4, "seed").sum())
            assert n_at > n_below, (pixel, name)
    a = by_name["rgba_u8_sqrt25"].image
    assert (a[..., :3] == a[0, 0, :3]).all() and len(np.unique(a[..., 3])) > 3  # alpha is the only field that differs
    f = by_name["f32_nan_seed"]
    assert np.isnan(f.image[f.seed]) and np.isinf(f.image).any()
    for mode in K.MODES:
        assert int(R.filled_mask(f.image, *f.seed, math.inf, 8, mode).sum()) == 1
    g = by_name["f32_inf_seed_inf_threshold"]  # |inf - x| = inf <= inf for a finite or -inf x; inf - inf is NaN and joins nothing
    seed_mask, neighbor_mask = (R.filled_mask(g.image, *g.seed, math.inf, 4, mode) for mode in K.MODES)
    other_inf = g.image == np.inf
    other_inf[g.seed] = False
    assert other_inf.any() and not (seed_mask & other_inf).any() and (seed_mask & (g.image == -np.inf)).any()
    assert (neighbor_mask & other_inf).any()  # reached through a finite pixel in between


# ---- the reference's own tests (src/image/tests/flood_fill.zig), through the restatements -----------------------------------------
@pytest.mark.parametrize("fill", [R.flood_fill_literal, R.flood_fill_fast])
def test_the_references_four_scenarios(fill):
    img = np.zeros((5, 5), np.uint8)
    for r, c in ((0, 1), (1, 2), (2, 0), (2, 1), (2, 2), (2, 3), (2, 4), (3, 2), (4, 2)):
        img[r, c] = 5
    out4, n4 = fill(img, 2, 2, 9, 0.0, 4)
    assert (out4[0, 1], out4[1, 2], out4[2, 2]) == (5, 9, 9) and n4 == 8
    out8, n8 = fill(img, 2, 2, 9, 0.0, 8)
    assert (out8[0, 1], out8[1, 2], out8[2, 2]) == (9, 9, 9) and n8 == 9
    ramp = np.arange(5, dtype=np.uint8).reshape(1, 5)
    assert fill(ramp, 0, 0, 9, 1.0, 4, "seed")[0].tolist() == [[9, 9, 2, 3, 4]]
    assert fill(ramp, 0, 0, 9, 1.0, 4, "neighbor")[0].tolist() == [[9, 9, 9, 9, 9]]
    rgb = np.array([[[100, 100, 100], [100, 100, 103], [100, 100, 107]]], np.uint8)
    red = (255, 0, 0)
    assert fill(rgb, 0, 0, red, 4.0)[0].tolist() == [[[255, 0, 0], [255, 0, 0], [100, 100, 107]]]
    assert fill(rgb, 0, 0, red, 8.0)[0].tolist() == [[[255, 0, 0]] * 3]
    with pytest.raises(R.OutOfBounds):
        fill(np.zeros((3, 3), np.uint8), 3, 3, 9, 1.0)


# ---- the constant of the device compare --------------------------------------------------------------------------------------------
MAX_SUM_SQ = 4 * 255 * 255


def threshold_set():
    """Every boundary value sqrt(s) of the byte sums of squares, its two f64 neighbours, random values and the special ones."""
    s = np.arange(0, MAX_SUM_SQ + 1, 63, dtype=np.float64)  # a sample of the sums, the perfect squares among them added below
    s = np.unique(np.concatenate([s, np.arange(0, 2 * 255 + 1, dtype=np.float64) ** 2, [1, 2, 3, 50, 51, MAX_SUM_SQ - 1, MAX_SUM_SQ]]))
    roots = np.sqrt(s)
    rng = np.random.default_rng(3)
    t = np.concatenate([roots, np.nextafter(roots, -np.inf), np.nextafter(roots, np.inf), rng.random(500) * 520, rng.random(100) * 4,
                        [0.0, -0.0, 1e-200, 1e200, math.inf, 5e-324, 254.99999999999997, 255.0, 255.00000000000003, 509.99999999999994, 510.0,
                         510.00000000000006, 1e6]])
    return t[t >= 0]


def test_flood_fill_bound_of_byte_structs_equals_the_brute_force_table():
    sums = np.arange(0, MAX_SUM_SQ + 1, dtype=np.float64)
    roots = np.sqrt(sums)
    thresholds = threshold_set()
    assert len(thresholds) > 12000
    for pixel in (L.PIXEL_RGB_U8, L.PIXEL_RGBA_U8):
        for t in thresholds.tolist():
            joins = int((roots <= t).sum())  # the table: how many sums s have sqrt(f64(s)) <= t
            b = zg.flood_fill_bound(pixel, t)
            assert b == float(int(b)) and -1 <= b <= MAX_SUM_SQ
            assert int(np.searchsorted(sums, b, side="right")) == joins, (pixel, t)  # the sums ascend: how many have s <= bound


def test_flood_fill_bound_of_u8_is_the_largest_difference_that_joins():
    diffs = np.arange(256, dtype=np.float64)
    for t in np.concatenate([diffs, np.nextafter(diffs, -np.inf), np.nextafter(diffs, np.inf), [0.5, 254.5, 1e200, math.inf, 5e-324]]).tolist():
        want = int((diffs <= t).sum()) - 1
        assert zg.flood_fill_bound(L.PIXEL_U8, t) == want, t


def test_flood_fill_bound_special_values():
    for pixel in range(6):
        for t in (-1.0, -5e-324, -math.inf, math.nan):
            assert zg.flood_fill_bound(pixel, t) == -1.0, (pixel, t)
        for t in (0.0, -0.0):
            b = zg.flood_fill_bound(pixel, t)
            assert b == 0.0 and math.copysign(1.0, b) == 1.0
    assert zg.flood_fill_bound(L.PIXEL_U8, math.inf) == 255 and zg.flood_fill_bound(L.PIXEL_RGBA_U8, math.inf) == MAX_SUM_SQ
    for pixel in (L.PIXEL_F32, L.PIXEL_RGB_F32, L.PIXEL_RGBA_F32):
        assert zg.flood_fill_bound(pixel, math.inf) == math.inf
    for t in (0.5, 1e-200, 1e200, 3.0000000000000004):
        assert zg.flood_fill_bound(L.PIXEL_F32, t) == t  # a scalar distance takes no square root
    with pytest.raises(zg.InvalidArgument):
        zg.flood_fill_bound(6, 1.0)
    assert zg.lib().zg_flood_fill_bound_host(0, 1.0, None) == L.ERR_INVALID_ARGUMENT


def test_flood_fill_bound_of_float_structs_is_the_largest_f64_whose_root_is_within_the_threshold():
    rng = np.random.default_rng(11)
    ts = np.concatenate([rng.random(300), rng.random(300) * 1e3, 10.0 ** rng.uniform(-300, 300, 400), np.sqrt(rng.random(200)),
                         [1.0, 2.0, math.sqrt(2.0), math.sqrt(3.0), 1e-200, 1e200, 1.3407807929942596e154, 1.3407807929942597e154, 1.7e308, 5e-324,
                          1.5e-162, 2.2250738585072014e-308]]).tolist()
    for pixel in (L.PIXEL_RGB_F32, L.PIXEL_RGBA_F32):
        for t in ts:
            s = zg.flood_fill_bound(pixel, t)
            assert s >= 0.0 and math.sqrt(s) <= t, (pixel, t, s)
            if s == 1.7976931348623157e308:  # the largest finite f64: everything finite joins
                assert math.sqrt(s) <= t
            else:
                assert math.sqrt(math.nextafter(s, math.inf)) > t, (pixel, t, s)
    # where t * t overflows or underflows the bisection still lands on the boundary
    assert zg.flood_fill_bound(L.PIXEL_RGBA_F32, 1e200) == 1.7976931348623157e308
    assert zg.flood_fill_bound(L.PIXEL_RGBA_F32, 1e-200) == 0.0  # the root of the smallest denormal is 2.2e-162: only a zero sum joins
    assert zg.flood_fill_bound(L.PIXEL_RGBA_F32, 2.3e-162) == 5e-324


# ---- the error convention, decided on the host: right without a GPU ----------------------------------------------------------------
def _has_device():
    return zg.lib().zg_device_count() > 0


def test_flood_fill_decides_its_status_before_anything_is_enqueued():
    lib = zg.lib()
    pixels = np.zeros((6, 8), np.uint8)
    img = L.ZgImage(pixels.ctypes.data, 8, 6, 8, L.PIXEL_U8)
    fill = (ctypes.c_uint8 * 16)(9)
    count = ctypes.c_uint32(77)

    def device(image, row, col, value, opt):
        return lib.zg_flood_fill(image, row, col, None, value, opt, None, None)

    def host(image, row, col, value, opt):
        return lib.zg_flood_fill_host(image, row, col, value, opt, ctypes.byref(count))

    for call in (device, host):
        ok = L.ZgFloodFillOptions(1.0, 4, 0)
        assert call(None, 0, 0, fill, ctypes.byref(ok)) == L.ERR_INVALID_ARGUMENT
        assert call(ctypes.byref(img), 0, 0, None, ctypes.byref(ok)) == L.ERR_INVALID_ARGUMENT
        for conn in (0, 1, 5, 6, 16, -4):
            assert call(ctypes.byref(img), 0, 0, fill, ctypes.byref(L.ZgFloodFillOptions(1.0, conn, 0))) == L.ERR_INVALID_ARGUMENT, conn
        for mode in (-1, 2, 8):
            assert call(ctypes.byref(img), 0, 0, fill, ctypes.byref(L.ZgFloodFillOptions(1.0, 8, mode))) == L.ERR_INVALID_ARGUMENT, mode
        for row, col in ((6, 0), (0, 8), (6, 8), (0xFFFFFFFF, 0), (0, 0xFFFFFFFF)):  # error.OutOfBounds
            assert call(ctypes.byref(img), row, col, fill, ctypes.byref(ok)) == L.ERR_INVALID_ARGUMENT, (row, col)
            assert call(ctypes.byref(img), row, col, fill, None) == L.ERR_INVALID_ARGUMENT
        assert b"OutOfBounds" in lib.zg_last_error()
        empty = L.ZgImage(None, 0, 0, 0, L.PIXEL_U8)
        assert call(ctypes.byref(empty), 0, 0, fill, None) == L.ERR_INVALID_ARGUMENT  # every seed is outside an empty image
        bad = L.ZgImage(pixels.ctypes.data, 4, 6, 8, L.PIXEL_U8)  # stride below cols
        assert call(ctypes.byref(bad), 0, 0, fill, None) == L.ERR_INVALID_ARGUMENT
        huge = L.ZgImage(pixels.ctypes.data, 1 << 16, 1 << 15, 1 << 16, L.PIXEL_U8)  # 2^31 pixels; nothing is touched
        assert call(ctypes.byref(huge), 0, 0, fill, None) == L.ERR_UNSUPPORTED
    assert count.value == 77 and not pixels.any()
    with pytest.raises(zg.InvalidArgument):
        zg.Image(pixels).flood_fill(6, 0, 9)
    with pytest.raises(zg.InvalidArgument):
        zg.Image(pixels).flood_fill(0, 0, 9, connectivity=6)
    with pytest.raises(zg.InvalidArgument):
        zg.Image(pixels).flood_fill(0, 0, 9, mode="parent")
    with pytest.raises(zg.InvalidArgument):
        zg.Image(pixels).flood_fill(-1, 0, 9)
    with pytest.raises(ValueError):
        zg.Image(pixels).flood_fill(0, 0, 9, count=np.zeros(1, np.uint32))
    if not _has_device():  # the argument errors first, then the missing device
        for call in (device, host):
            assert call(ctypes.byref(img), 0, 0, fill, None) == L.ERR_HIP
        with pytest.raises(zg.ZignalError):
            zg.Image(pixels).flood_fill(0, 0, 9)
        assert count.value == 77 and not pixels.any()


def test_the_options_mirror_the_struct():
    o = zg.FloodFillOptions()
    assert (o.threshold, o.connectivity, o.mode) == (0.0, 4, "seed")  # FloodFillOptions.default
    c = zg.FloodFillOptions(2.5, 8, "neighbor")._c()
    assert (c.threshold, c.connectivity, c.mode) == (2.5, 8, L.FLOOD_MODE_NEIGHBOR)
    assert ctypes.sizeof(L.ZgFloodFillOptions) == 16
    assert [getattr(L.ZgFloodFillOptions, n).offset for n in ("threshold", "connectivity", "mode")] == [0, 8, 12]


# ---- the module's boundary -----------------------------------------------------------------------------------------------------------
def _flood_header():
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "zignal_hip_flood.h")).read(), flags=re.S)
    protos = re.findall(r"ZG_API\s+[\w\s\*]+?\b(zg_\w+)\s*\(([^;]*?)\)\s*;", text, flags=re.S)
    return {name: ([] if args.strip() == "void" else args.split(",")) for name, args in protos}


def test_flood_header_bindings_and_zig_file_declare_the_same_symbols():
    protos = _flood_header()
    assert sorted(protos) == sorted(L.FLOOD_EXPORTED_SYMBOLS) == sorted(["zg_flood_fill", "zg_flood_fill_host", "zg_flood_fill_bound_host",
                                                                         "zg_flood_fill_tile"])
    raw = ctypes.CDLL(L.LIB_PATH)
    for name, args in protos.items():
        assert hasattr(raw, name), f"{name} declared in include/zignal_hip_flood.h but not exported"
        assert len(L._FLOOD_SIGNATURES[name]) == len(args), name
        assert getattr(zg.lib(), name).argtypes is not None or not args
    others = set(L.EXPORTED_SYMBOLS) | set(L.ORB_EXPORTED_SYMBOLS) | set(L.MATCH_EXPORTED_SYMBOLS) | set(L.HOUGH_EXPORTED_SYMBOLS)
    assert not set(L.FLOOD_EXPORTED_SYMBOLS) & others
    shim = open(os.path.join(ROOT, "zig", "zignal_hip_flood.zig")).read()
    externs = dict(re.findall(r"pub extern fn (zg_\w+)\(([^)]*)\)", shim))
    assert set(externs) == set(protos)
    for name, args in externs.items():
        assert len([a for a in args.split(",") if a.strip()]) == len(protos[name]), name
    main = open(os.path.join(ROOT, "include", "zignal_hip.h")).read()
    assert main.index('#include "zignal_hip_hough.h"') < main.index('#include "zignal_hip_flood.h"')
    makefile = open(os.path.join(ROOT, "zignal_amd", "csrc", "Makefile")).read()
    # both object rules depend on every header of include/ and of csrc/
    assert "$(wildcard ../../include/*.h)" in makefile and "$(wildcard *.h)" in makefile and makefile.count("$(HEADERS)") == 2
    assert os.path.isfile(os.path.join(ROOT, "include", "zignal_hip_flood.h")) and os.path.isfile(os.path.join(ROOT, "zignal_amd", "csrc", "zg_unionfind.h"))
