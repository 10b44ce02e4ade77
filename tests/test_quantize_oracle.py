"""CPU checks of the quantisation module (include/zignal_hip_quantize.h): the two restatements of error diffusion in tests/quantize_ref.py
agree with each other, the library's host functions (median cut from a histogram, the lookup table, the fixed palettes) equal the
restatement byte for byte, argument errors are answered without a device, and the module's symbols are declared, exported and bound."""
import ctypes
import os
import re

import numpy as np
import pytest

from tests import quantize_ref as R
import zignal_amd as zg
from zignal_amd import _lib as L

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

TWO_GREYS = np.array([[64, 64, 64], [192, 192, 192]], np.uint8)  # every error is up to 64 either way: the updates clamp at both ends


def noise(seed, rows, cols, ch=3):
    shape = (rows, cols) if ch == 1 else (rows, cols, ch)
    return np.random.default_rng(seed).integers(0, 256, shape, dtype=np.uint8)


def random_palette(seed, n):
    return np.random.default_rng(1000 + seed).integers(0, 256, (n, 3), dtype=np.uint8)


# (name, image, palette): every image is uniform u8 noise, which with these palettes clamps at both ends and truncates negative products
DIFFUSION_CASES = [
    ("two greys 37x53", noise(1, 37, 53), TWO_GREYS),
    ("two greys 3x3", noise(2, 3, 3), TWO_GREYS),
    ("two greys 2x40", noise(3, 2, 40), TWO_GREYS),
    ("two greys 40x2", noise(4, 40, 2), TWO_GREYS),
    ("two greys 40x3", noise(5, 40, 3), TWO_GREYS),
    ("vga16 31x29", noise(6, 31, 29), R.fixed_palette(R.FIXED_VGA16)),
    ("six random 24x24", noise(7, 24, 24), random_palette(7, 6)),
]


@pytest.mark.parametrize("mode", [R.FLOYD_STEINBERG, R.ATKINSON], ids=["floyd_steinberg", "atkinson"])
@pytest.mark.parametrize("case", DIFFUSION_CASES, ids=[c[0] for c in DIFFUSION_CASES])
def test_the_two_restatements_of_error_diffusion_agree(case, mode):
    _, img, palette = case
    lut = R.palette_lut(palette)
    stats = R.DiffusionStats()
    literal = R.dither_literal(img, palette, lut, mode, stats)
    print(f"clamped at 0: {stats.clamped_low}, at 255: {stats.clamped_high}, truncated: {stats.truncated}")
    # a case that never clamps does not test the order of the updates
    assert stats.clamped_low > 0 and stats.clamped_high > 0 and stats.truncated > 0
    assert np.array_equal(literal, R.dither_gather(img, palette, lut, mode))


@pytest.mark.parametrize("mode", [R.FLOYD_STEINBERG, R.ATKINSON], ids=["floyd_steinberg", "atkinson"])
@pytest.mark.parametrize("shape", [(1, 1), (1, 2), (1, 3), (2, 1), (3, 1), (1, 9), (9, 1), (2, 2), (2, 3), (3, 2)])
def test_the_two_restatements_agree_on_the_smallest_shapes(shape, mode):
    img = noise(shape[0] * 16 + shape[1], *shape)
    lut = R.palette_lut(TWO_GREYS)
    assert np.array_equal(R.dither_literal(img, TWO_GREYS, lut, mode), R.dither_gather(img, TWO_GREYS, lut, mode))


def test_the_order_of_the_updates_matters():
    """The same errors applied in another order give other pixels: what the gather order is there for."""
    img, lut = noise(1, 37, 53), R.palette_lut(TWO_GREYS)
    saved = R.FS_GATHER
    try:
        R.FS_GATHER = tuple(reversed(saved))
        other = R.dither_gather(img, TWO_GREYS, lut, R.FLOYD_STEINBERG)
    finally:
        R.FS_GATHER = saved
    assert not np.array_equal(other, R.dither_gather(img, TWO_GREYS, lut, R.FLOYD_STEINBERG))


# ---- the library's host functions ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 2, 15, 16, 17, 256])
def test_host_lookup_table_equals_the_restatement(n):
    palette = random_palette(n, n)
    assert np.array_equal(zg.palette_lut(palette), R.palette_lut(palette))


def test_host_lookup_table_ties_go_to_the_lowest_index():
    palette = np.array([[10, 20, 30], [200, 100, 50], [10, 20, 30], [200, 100, 50]], np.uint8)
    lut = zg.palette_lut(palette)
    assert np.array_equal(lut, R.palette_lut(palette)) and set(np.unique(lut)) == {0, 1}


@pytest.mark.parametrize("mode", [R.FIXED_6X7X6, R.FIXED_VGA16, R.FIXED_WEB216])
def test_fixed_palettes_equal_the_restatement(mode):
    got = zg.build_palette(mode)
    assert np.array_equal(got, R.fixed_palette(mode)) and len(got) == (252, 16, 216)[mode]


def test_fixed_palette_known_answers():
    p = zg.build_palette(zg.PaletteMode.fixed_6x7x6)
    # quantize.zig:415-429: entry (r, g, b) of the 6 x 7 x 6 grid at r * 42 + g * 6 + b
    assert tuple(p[0]) == (0, 0, 0) and tuple(p[251]) == (255, 255, 255) and tuple(p[1 * 42 + 1 * 6 + 1]) == (51, 43, 51)
    assert tuple(zg.build_palette(zg.PaletteMode.fixed_vga16)[7]) == (192, 192, 192)  # quantize.zig:464, Silver
    assert tuple(zg.build_palette(zg.PaletteMode.fixed_web216)[215]) == (255, 255, 255)


def many_equal_keys(seed):
    """Few distinct values per channel: every sort meets long runs of equal keys, which is where an unstable sort shows."""
    rng = np.random.default_rng(seed)
    levels = np.array([0, 8, 64, 72, 200, 248], np.uint8)
    return levels[rng.integers(0, len(levels), (48, 48, 3))]


MEDIAN_CUT_CASES = [("noise 64x64", noise(11, 64, 64), 256), ("noise 64x64, 2 colours", noise(11, 64, 64), 2), ("noise 64x64, 17", noise(12, 64, 64), 17),
                    ("equal keys, 16", many_equal_keys(13), 16), ("equal keys, 256", many_equal_keys(14), 256),
                    ("two colours, 256", TWO_GREYS[np.random.default_rng(15).integers(0, 2, (9, 9))], 256),
                    ("grey noise", noise(16, 40, 40, 1), 32), ("rgba noise", noise(17, 40, 40, 4), 64)]


@pytest.mark.parametrize("case", MEDIAN_CUT_CASES, ids=[c[0] for c in MEDIAN_CUT_CASES])
def test_host_median_cut_equals_the_restatement(case):
    _, img, max_colors = case
    counts, first = R.histogram(img)
    want = R.median_cut_from_histogram(counts, first, max_colors)
    got = zg.median_cut_from_histogram(counts, first, max_colors)
    assert got.shape == want.shape and np.array_equal(got, want)
    assert 1 <= len(got) <= max_colors


def test_median_cut_depends_on_the_order_the_cells_were_touched():
    """The same populations with `first` reversed: the heap sort is unstable, so the colour list's order reaches the palette."""
    img = many_equal_keys(13)
    counts, first = R.histogram(img)
    counts_r, first_r = R.histogram(img[::-1, ::-1])
    assert np.array_equal(counts, counts_r) and not np.array_equal(first, first_r)
    for c, f in ((counts, first), (counts_r, first_r)):
        assert np.array_equal(zg.median_cut_from_histogram(c, f, 16), R.median_cut_from_histogram(c, f, 16))


def test_median_cut_single_colour_and_capacity():
    img = np.full((5, 7, 3), 77, np.uint8)
    counts, first = R.histogram(img)
    got = zg.median_cut_from_histogram(counts, first, 256)
    assert got.tolist() == [[R.expand5(77 >> 3)] * 3]  # the early return (quantize.zig:245-252): the cell's colour, not the pixel's
    counts, first = R.histogram(noise(18, 32, 32))
    assert len(zg.median_cut_from_histogram(counts, first, 256, capacity=5)) == 5
    assert np.array_equal(zg.median_cut_from_histogram(counts, first, 256, capacity=5), R.median_cut_from_histogram(counts, first, 256, 5))


def test_median_cut_no_palette_colors():
    counts, first = np.zeros(R.CELLS, np.uint32), np.full(R.CELLS, R.UNTOUCHED, np.uint32)
    with pytest.raises(zg.InvalidArgument, match="NoPaletteColors"):
        zg.median_cut_from_histogram(counts, first, 256)
    counts, first = R.histogram(noise(19, 8, 8))
    with pytest.raises(zg.InvalidArgument, match="NoPaletteColors"):
        zg.median_cut_from_histogram(counts, first, 0)
    with pytest.raises(R.NoPaletteColors):
        R.median_cut_from_histogram(counts, first, 0)


def test_reference_unit_test_known_answers():
    """Answers the reference's own unit tests state for these functions, on the restatement and on the library's host functions."""
    # sixel.zig:490-513 "palette mode - fixed 6x7x6 color mapping": pure red, green and blue map to themselves in the 6x7x6 palette
    p = zg.build_palette(zg.PaletteMode.fixed_6x7x6)
    lut = zg.palette_lut(p)
    for rgb in ((255, 0, 0), (0, 255, 0), (0, 0, 255), (0, 0, 0), (255, 255, 255)):
        assert tuple(p[R.lookup(lut, np.array(rgb, np.uint8))]) == rgb
    # gif.zig:1572-1602 "encode - caller-supplied palette, exact round-trip": four pixels of a four-colour palette come back exactly,
    # which asks of mapImageToPalette that a palette colour maps to its own index
    palette = np.array([[0, 0, 0], [255, 0, 0], [0, 255, 0], [0, 0, 255]], np.uint8)
    img = palette[np.array([[0, 1], [2, 3]])]
    assert R.map_to_palette(img, palette, False).tolist() == [[0, 1], [2, 3]]
    assert R.lookup(zg.palette_lut(palette), img).tolist() == [[0, 1], [2, 3]]
    # gif.zig:1604-1626 "encode - auto median-cut on 16x16 gradient": max_colors 16 gives a palette of 2 to 16 entries
    grad = np.zeros((16, 16, 3), np.uint8)
    grad[:, :, 0] = (np.arange(16) * 16)[None, :]
    grad[:, :, 1] = (np.arange(16) * 16)[:, None]
    grad[:, :, 2] = 128
    got = zg.median_cut_from_histogram(*R.histogram(grad), 16)
    assert 2 <= len(got) <= 16 and np.array_equal(got, R.median_cut(grad, 16))


# ---- argument errors, answered before any device call ------------------------------------------------------------------------------
def _img(rows, cols, pixel, data=0x1000, stride=None):
    return L.ZgImage(data, cols if stride is None else stride, rows, cols, pixel)


def test_argument_errors_without_a_gpu():
    lib = zg.lib()
    p, t = ctypes.c_void_p(0x2000), ctypes.c_void_p(0x3000)
    rgb, f32, grey = _img(4, 4, L.PIXEL_RGB_U8), _img(4, 4, L.PIXEL_RGB_F32), _img(4, 4, L.PIXEL_U8)
    assert lib.zg_color_histogram(ctypes.byref(f32), p, t, None) == L.ERR_UNSUPPORTED
    assert lib.zg_color_histogram(ctypes.byref(rgb), None, t, None) == L.ERR_INVALID_ARGUMENT
    assert lib.zg_color_histogram(ctypes.byref(_img(65536, 65536, L.PIXEL_U8)), p, t, None) == L.ERR_UNSUPPORTED  # 2^32 pixels
    assert lib.zg_palette_lut(p, 0, t, None) == L.ERR_INVALID_ARGUMENT
    assert lib.zg_palette_lut(p, 257, t, None) == L.ERR_INVALID_ARGUMENT
    host = (ctypes.c_uint8 * 768)()
    table = (ctypes.c_uint8 * 32768)()
    assert lib.zg_palette_lut_host(host, 0, table) == L.ERR_INVALID_ARGUMENT
    assert lib.zg_palette_lut_host(host, 257, table) == L.ERR_INVALID_ARGUMENT
    assert lib.zg_dither(ctypes.byref(grey), p, 2, t, L.DITHER_ORDERED, None) == L.ERR_UNSUPPORTED       # Rgb(u8) only
    assert lib.zg_dither(ctypes.byref(rgb), p, 2, t, 5, None) == L.ERR_INVALID_ARGUMENT                  # mode
    assert lib.zg_dither(ctypes.byref(rgb), p, 0, t, L.DITHER_ORDERED, None) == L.ERR_INVALID_ARGUMENT   # n
    assert lib.zg_dither(ctypes.byref(rgb), p, 2, None, L.DITHER_ORDERED, None) == L.ERR_INVALID_ARGUMENT
    assert lib.zg_dither_frames(ctypes.byref(rgb), 3, 10, p, 2, t, L.DITHER_ORDERED, None) == L.ERR_INVALID_ARGUMENT  # frames overlap
    idx = _img(4, 4, L.PIXEL_U8, data=0x4000)
    assert lib.zg_palette_map(ctypes.byref(rgb), ctypes.byref(_img(4, 5, L.PIXEL_U8, data=0x4000)), p, 2, 0, -1, None) == L.ERR_DIMENSION_MISMATCH
    assert lib.zg_palette_map(ctypes.byref(rgb), ctypes.byref(rgb), p, 2, 0, -1, None) == L.ERR_INVALID_ARGUMENT      # the index plane is u8
    assert lib.zg_palette_map(ctypes.byref(f32), ctypes.byref(idx), p, 2, 0, -1, None) == L.ERR_UNSUPPORTED
    assert lib.zg_palette_map(ctypes.byref(rgb), ctypes.byref(idx), p, 1, 0, 0, None) == L.ERR_INVALID_ARGUMENT       # nothing left to look up
    assert lib.zg_palette_map(ctypes.byref(rgb), ctypes.byref(idx), p, 2, 0, 256, None) == L.ERR_INVALID_ARGUMENT
    n = ctypes.c_uint32()
    assert lib.zg_build_palette(None, 7, 256, host, ctypes.byref(n)) == L.ERR_INVALID_ARGUMENT
    assert lib.zg_median_cut(ctypes.byref(f32), 256, 256, host, ctypes.byref(n)) == L.ERR_UNSUPPORTED


def test_dither_geometry_and_ordinals():
    band, phase, per_launch = zg.dither_geometry()
    assert band == 64 and phase >= 128 and per_launch % band == 0 and per_launch <= 1024
    assert (zg.DitherMode.none, zg.DitherMode.floyd_steinberg, zg.DitherMode.atkinson, zg.DitherMode.ordered, zg.DitherMode.auto) == (0, 1, 2, 3, 4)  # dither.zig:18-30
    assert (zg.PaletteMode.fixed_6x7x6, zg.PaletteMode.fixed_vga16, zg.PaletteMode.fixed_web216, zg.PaletteMode.adaptive) == (0, 1, 2, 3)       # quantize.zig:476-488


# ---- the module's boundary, as tests/test_abi.py keeps it for the main header ---------------------------------------------------------
def _header_protos():
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "zignal_hip_quantize.h")).read(), flags=re.S)
    return re.findall(r"ZG_API\s+[\w\s\*]+?\b(zg_\w+)\s*\(([^;]*?)\)\s*;", text, flags=re.S)


def test_every_declared_symbol_is_exported_and_bound():
    protos = _header_protos()
    assert len(protos) == 10
    raw = ctypes.CDLL(L.LIB_PATH)
    for name, args in protos:
        assert hasattr(raw, name), f"{name} declared in include/zignal_hip_quantize.h but not exported"
        args = args.strip()
        n = 0 if args in ("", "void") else len(args.split(","))
        assert len(L._QUANTIZE_SIGNATURES[name]) == n, name
    assert sorted(L.QUANTIZE_EXPORTED_SYMBOLS) == sorted(name for name, _ in protos)


def test_zig_shim_declares_the_module():
    shim = open(os.path.join(ROOT, "zig", "zignal_hip_quantize.zig")).read()
    assert set(re.findall(r"pub extern fn (zg_\w+)\(", shim)) == {name for name, _ in _header_protos()}


def test_main_header_includes_the_module():
    main = open(os.path.join(ROOT, "include", "zignal_hip.h")).read()
    assert main.index('#include "zignal_hip_metrics.h"') < main.index('#include "zignal_hip_quantize.h"')


# ---- the cases of tests/test_gpu_quantize.py: the device is held to the gather form, the gather form here to the literal one ---------
def _gpu_cases():
    from tests import test_gpu_quantize as G
    cases = [(f"{r}x{c}", r, c, 7, "two greys") for r, c in G.SHAPES]
    cases += [(name, G.BAND + 7, G.PHASE + 13, 8, name) for name in G.PALETTES]
    return G, cases


@pytest.mark.parametrize("mode", [R.FLOYD_STEINBERG, R.ATKINSON], ids=["floyd_steinberg", "atkinson"])
def test_the_two_restatements_agree_on_every_case_of_the_gpu_tests(mode):
    G, cases = _gpu_cases()
    for name, rows, cols, seed, palette in cases:
        stats = R.DiffusionStats()
        literal = R.dither_literal(G.noise(seed, rows, cols), G.PALETTES[palette], G.lut_of(palette), mode, stats)
        print(f"{name}: clamped at 0: {stats.clamped_low}, at 255: {stats.clamped_high}, truncated: {stats.truncated}")
        assert literal.tobytes() == G.want(rows, cols, seed, palette, mode).tobytes(), name
        if rows * cols >= 500:  # a frame of a few pixels has too few updates to meet all three
            assert stats.clamped_low > 0 and stats.clamped_high > 0 and stats.truncated > 0, name
