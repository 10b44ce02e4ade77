"""Seam carving without a GPU: the two CPU restatements of the reference's seam_carve example (tests/seam_ref.py) against each other on
every shared case, the cases against what their names promise (a tie case must tell the reference's rule from a neighbouring one), the
argument checks of the zg_seam_* entry points, and the module's boundary (header, bindings, Zig file)."""
import ctypes
import os
import re

import numpy as np
import pytest

import zignal_amd as zg
from zignal_amd import _lib as L
from tests import seam_cases as K
from tests import seam_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
B, S = zg.seam_band_rows(), zg.seam_strip_cols()
CASES = K.edge_cases(B, S)
BY_NAME = {c.name: c for c in CASES}


def test_the_tile_is_a_pair_of_host_constants():
    assert B == zg.lib().zg_seam_band_rows() >= 2 and S == zg.lib().zg_seam_strip_cols() >= 8
    assert max(max(c.edges.shape) for c in CASES) <= 2 * S + 3 and 3 * B + 1 <= 512 and 2 * S + 3 <= 512  # a few hundred pixels a side


@pytest.mark.parametrize("index", range(len(CASES)), ids=[c.name for c in CASES])
def test_the_two_restatements_agree(index):
    case = CASES[index]
    before = case.edges.copy()
    energy = R.compute_energy_literal(case.edges)
    assert energy.dtype == np.uint32 and np.array_equal(energy, R.compute_energy_fast(case.edges))
    seam = R.compute_seam_literal(energy)
    assert seam.dtype == np.uint32 and np.array_equal(seam, R.compute_seam_fast(energy))
    assert np.array_equal(case.edges, before)
    if case.seam is not None:
        assert np.array_equal(seam, case.seam)
    # a seam is connected and inside the frame
    assert (seam < case.edges.shape[1]).all() and (np.abs(np.diff(seam.astype(np.int64))) <= 1).all()
    # column `cols` reading column cols - 1 is the centre once more: it never lowers a minimum, so it equals leaving the column out
    assert np.array_equal(seam, R.compute_seam_literal(energy, cols_rule="skip"))


def test_the_shapes_sit_on_both_sides_of_the_tile():
    for rows in (B - 1, B, B + 1, 2 * B + 1, 3 * B + 1):
        for cols in (S - 1, S, S + 1, 2 * S + 3):
            assert BY_NAME[f"shape_{rows}x{cols}"].edges.shape == (rows, cols)
    assert BY_NAME["shape_1xN"].edges.shape[0] == 1 and BY_NAME["shape_Nx2"].edges.shape[1] == 2 and BY_NAME["shape_2x2"].edges.shape == (2, 2)


def test_every_tie_case_tells_the_rule_from_a_wrong_one():
    ties = [c for c in CASES if c.tie is not None]
    assert {c.tie for c in ties} == {"leftmost", "rightmost", "last"} and len(ties) >= 10
    for c in ties:
        energy = R.compute_energy_literal(c.edges)
        right = R.compute_seam_literal(energy)
        wrong = R.compute_seam_literal(energy, bottom="last") if c.tie == "last" else R.compute_seam_literal(energy, back=c.tie)
        assert not np.array_equal(right, wrong), c.name
    # the three patterns are what their names say, in the row above the seam's end
    for m in (2, S - 1, S):
        for name, rel in (("left_eq_centre", lambda l, c, r: l == c < r), ("centre_eq_right", lambda l, c, r: c == r < l),
                          ("left_eq_right", lambda l, c, r: l == r < c)):
            e = R.compute_energy_literal(BY_NAME[f"tie_{name}_at_{m}"].edges)
            assert rel(*(int(v) for v in e[0, m - 1: m + 2])) and int(np.argmin(e[1])) == m and (e[1] == e[1].min()).sum() == 1
    e = R.compute_energy_literal(BY_NAME["tie_bottom_row"].edges)
    assert (e[-1] == e[-1].min()).sum() == 2
    flat = R.compute_energy_literal(BY_NAME["flat"].edges)
    assert all(len(set(row.tolist())) == 1 for row in flat)  # every comparison a tie


def test_the_border_and_valley_cases_are_what_their_names_say():
    right = BY_NAME["right_border"]
    energy = R.compute_energy_literal(right.edges)
    cols = right.edges.shape[1]
    assert (R.compute_seam_literal(energy) == cols - 1).all()
    # the rule for column `cols` matters: a walker that has none reads the packed map past the row's end, the next row's first sum
    lost = R.compute_seam_literal(energy, cols_rule="packed")
    assert not np.array_equal(lost, right.seam) and (lost >= cols).any()
    left = BY_NAME["left_border"]
    assert (R.compute_seam_literal(R.compute_energy_literal(left.edges)) == 0).all()
    v = K.valley_columns(B, S).astype(np.int64)
    assert np.array_equal(BY_NAME["diagonal_valley"].seam, v) and (np.abs(np.diff(v)) == 1).all()
    step = np.diff(v)
    assert {int(step[r - 1]) for r in (1 + B, 1 + 2 * B)} == {1, -1}  # bands start at rows 1 + k B: a border is crossed in each direction
    crossings = [int(step[r]) for r in range(len(step)) if {int(v[r]), int(v[r + 1])} == {S - 1, S}]
    assert sorted(crossings) == [-1, 1]  # and so is the strip border
    big = R.compute_energy_literal(BY_NAME["all_255"].edges)
    assert int(big.max()) == 255 * (3 * B + 1)


def test_remove_seam_drops_one_pixel_a_row():
    img = K.pixels_like(5, 4, 6, "rgb_u8")
    out = R.remove_seam(img, [0, 5, 2, 9])  # an entry past the row drops the last pixel
    assert np.array_equal(out[0], img[0, 1:]) and np.array_equal(out[1], img[1, :5]) and np.array_equal(out[3], img[3, :5])
    assert np.array_equal(out[2], np.concatenate([img[2, :2], img[2, 3:]]))


def test_the_iteration_agrees_in_both_forms(oracle):
    for pixel, shape in (("rgba_u8", (9, 13)), ("u8", (B + 1, 7)), ("f32", (5, 5))):
        img = K.frame(3, *shape, pixel)
        a, sa = R.carve(img, 3, oracle.sobel, literal=True)
        b, sb = R.carve(img, 3, oracle.sobel)
        assert a.tobytes() == b.tobytes() and np.array_equal(sa, sb) and a.shape[1] == shape[1] - 3
    h, sh = R.carve_horizontal(K.frame(3, 9, 13, "rgba_u8"), 2, oracle.sobel)
    assert h.shape == (7, 13, 4) and sh.shape == (2, 13)


# ---- the error convention, decided on the host: right without a GPU ----------------------------------------------------------------
def _has_device():
    return zg.lib().zg_device_count() > 0


def _img(a, pixel, rows=None, cols=None, stride=None):
    rows = a.shape[0] if rows is None else rows
    cols = a.shape[1] if cols is None else cols
    return L.ZgImage(a.ctypes.data, cols if stride is None else stride, rows, cols, pixel)


def test_the_seam_entry_points_decide_their_status_before_anything_is_enqueued():
    lib = zg.lib()
    src = np.zeros((6, 8, 4), np.uint8)
    dst = np.full((6, 8, 4), 7, np.uint8)
    edges = np.zeros((6, 8), np.uint8)
    words = np.full(6 * 8, 5, np.uint32)
    seam = np.zeros(6, np.uint32)
    wp, sp = ctypes.c_void_p(words.ctypes.data), ctypes.c_void_p(seam.ctypes.data)
    s8, e8 = _img(src, L.PIXEL_RGBA_U8), _img(edges, L.PIXEL_U8)
    huge = L.ZgImage(src.ctypes.data, 1 << 16, 1 << 15, 1 << 16, L.PIXEL_U8)  # 2^31 pixels; nothing is touched

    def carve(device, a, b, n, axis=0, source=None, out=None):
        return lib.zg_seam_carve(a, b, n, axis, source, out, None) if device else lib.zg_seam_carve_host(a, b, n, axis, source, out)

    for device in (True, False):
        d7, d6 = _img(dst, L.PIXEL_RGBA_U8, cols=7, stride=8), _img(dst, L.PIXEL_RGBA_U8, cols=6, stride=8)
        assert carve(device, None, ctypes.byref(d7), 1) == L.ERR_INVALID_ARGUMENT
        assert carve(device, ctypes.byref(s8), None, 1) == L.ERR_INVALID_ARGUMENT
        for n in (0, 8, 9, 0xFFFFFFFF):
            assert carve(device, ctypes.byref(s8), ctypes.byref(d7), n) == L.ERR_INVALID_ARGUMENT, n
        for axis in (-1, 2):
            assert carve(device, ctypes.byref(s8), ctypes.byref(d7), 1, axis) == L.ERR_INVALID_ARGUMENT
        assert carve(device, ctypes.byref(s8), ctypes.byref(d7), 1, 0, ctypes.byref(e8)) == L.ERR_UNSUPPORTED  # the reserved argument
        assert b"energy_source" in lib.zg_last_error()
        assert carve(device, ctypes.byref(s8), ctypes.byref(d6), 1) == L.ERR_DIMENSION_MISMATCH
        assert carve(device, ctypes.byref(s8), ctypes.byref(d7), 1, 1) == L.ERR_DIMENSION_MISMATCH  # horizontal: 5 x 8
        other = _img(dst, L.PIXEL_RGBA_F32, cols=1, stride=2)
        assert carve(device, ctypes.byref(s8), ctypes.byref(other), 7) == L.ERR_INVALID_ARGUMENT  # another pixel type
        shared = _img(src, L.PIXEL_RGBA_U8, cols=7, stride=8)
        assert carve(device, ctypes.byref(s8), ctypes.byref(shared), 1) == L.ERR_INVALID_ARGUMENT  # not disjoint
        empty = L.ZgImage(None, 0, 0, 8, L.PIXEL_RGBA_U8)
        assert carve(device, ctypes.byref(empty), ctypes.byref(L.ZgImage(None, 0, 0, 7, L.PIXEL_RGBA_U8)), 1) == L.ERR_INVALID_ARGUMENT
        hd = L.ZgImage(dst.ctypes.data, 1 << 16, 1 << 15, (1 << 16) - 1, L.PIXEL_U8)
        assert carve(device, ctypes.byref(huge), ctypes.byref(hd), 1) == L.ERR_UNSUPPORTED

        energy = (lambda e, w: lib.zg_seam_energy(e, w, None)) if device else lib.zg_seam_energy_host
        assert energy(None, wp) == L.ERR_INVALID_ARGUMENT and energy(ctypes.byref(e8), None) == L.ERR_INVALID_ARGUMENT
        assert energy(ctypes.byref(s8), wp) == L.ERR_INVALID_ARGUMENT  # not an Image(u8)
        assert energy(ctypes.byref(huge), wp) == L.ERR_UNSUPPORTED
        find = (lambda e, r, c, s: lib.zg_seam_find(e, r, c, s, None)) if device else lib.zg_seam_find_host
        assert find(None, 6, 8, sp) == L.ERR_INVALID_ARGUMENT and find(wp, 6, 8, None) == L.ERR_INVALID_ARGUMENT
        assert find(wp, 0, 8, sp) == L.ERR_INVALID_ARGUMENT and find(wp, 6, 0, sp) == L.ERR_INVALID_ARGUMENT
        assert find(wp, 1 << 15, 1 << 16, sp) == L.ERR_UNSUPPORTED
        remove = (lambda a, s, b: lib.zg_seam_remove(a, s, b, None)) if device else lib.zg_seam_remove_host
        assert remove(None, sp, ctypes.byref(d7)) == L.ERR_INVALID_ARGUMENT and remove(ctypes.byref(s8), None, ctypes.byref(d7)) == L.ERR_INVALID_ARGUMENT
        assert remove(ctypes.byref(s8), sp, None) == L.ERR_INVALID_ARGUMENT
        assert remove(ctypes.byref(s8), sp, ctypes.byref(d6)) == L.ERR_DIMENSION_MISMATCH
        assert remove(ctypes.byref(s8), sp, ctypes.byref(shared)) == L.ERR_INVALID_ARGUMENT
        assert remove(ctypes.byref(s8), sp, ctypes.byref(_img(dst, L.PIXEL_RGB_U8, cols=7, stride=8))) == L.ERR_INVALID_ARGUMENT
        if not _has_device():  # the argument errors first, then the missing device
            assert carve(device, ctypes.byref(s8), ctypes.byref(d7), 1) == L.ERR_HIP
            assert energy(ctypes.byref(e8), wp) == L.ERR_HIP and find(wp, 6, 8, sp) == L.ERR_HIP
            assert remove(ctypes.byref(s8), sp, ctypes.byref(d7)) == L.ERR_HIP
    assert not src.any() and (dst == 7).all() and (words == 5).all() and not seam.any()


def test_the_python_mirror_checks_what_the_library_cannot():
    img = zg.Image(np.zeros((6, 8), np.uint8))
    with pytest.raises(zg.InvalidArgument):
        img.seam_carve(1, axis="diagonal")
    with pytest.raises(zg.InvalidArgument):
        img.seam_carve(0)
    with pytest.raises(zg.InvalidArgument):
        img.seam_carve(8)
    with pytest.raises(zg.InvalidArgument):
        img.seam_carve(-1)
    with pytest.raises(ValueError):
        img.seam_carve(1, seams=np.zeros(5, np.uint32))  # n * rows words
    with pytest.raises(ValueError):
        img.seam_remove(np.zeros(6, np.float64))
    with pytest.raises(zg.DimensionMismatch):
        img.seam_remove(np.zeros(6, np.uint32), out=np.zeros((6, 8), np.uint8))
    with pytest.raises(zg.InvalidArgument):
        zg.seam_find(np.zeros(4, np.uint32), 0, 4)
    if not _has_device():
        with pytest.raises(zg.ZignalError):
            img.seam_carve(1)
        with pytest.raises(zg.ZignalError):
            zg.seam_energy(np.zeros((6, 8), np.uint8))


# ---- the module's boundary -----------------------------------------------------------------------------------------------------------
def _seam_header():
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "zignal_hip_seam.h")).read(), flags=re.S)
    protos = re.findall(r"ZG_API\s+[\w\s\*]+?\b(zg_\w+)\s*\(([^;]*?)\)\s*;", text, flags=re.S)
    return {name: ([] if args.strip() == "void" else args.split(",")) for name, args in protos}


def test_seam_header_bindings_and_zig_file_declare_the_same_symbols():
    protos = _seam_header()
    assert sorted(protos) == sorted(L.SEAM_EXPORTED_SYMBOLS) == sorted(
        ["zg_seam_band_rows", "zg_seam_strip_cols", "zg_seam_energy", "zg_seam_find", "zg_seam_remove", "zg_seam_carve", "zg_seam_energy_host",
         "zg_seam_find_host", "zg_seam_remove_host", "zg_seam_carve_host"])
    raw = ctypes.CDLL(L.LIB_PATH)
    for name, args in protos.items():
        assert hasattr(raw, name), f"{name} declared in include/zignal_hip_seam.h but not exported"
        assert len(L._SEAM_SIGNATURES[name]) == len(args), name
        assert getattr(zg.lib(), name).argtypes is not None or not args
    assert not set(L.SEAM_EXPORTED_SYMBOLS) & (set(L.EXPORTED_SYMBOLS) | set(L.FLOOD_EXPORTED_SYMBOLS) | set(L.TRANSFORM_EXPORTED_SYMBOLS))
    shim = open(os.path.join(ROOT, "zig", "zignal_hip_seam.zig")).read()
    externs = dict(re.findall(r"pub extern fn (zg_\w+)\(([^)]*)\)", shim))
    assert set(externs) == set(protos)
    for name, args in externs.items():
        assert len([a for a in args.split(",") if a.strip()]) == len(protos[name]), name
    main = open(os.path.join(ROOT, "include", "zignal_hip.h")).read()
    assert main.index('#include "zignal_hip_transform.h"') < main.index('#include "zignal_hip_seam.h"')
    header = open(os.path.join(ROOT, "include", "zignal_hip_seam.h")).read()
    assert "#define ZG_SEAM_VERTICAL 0" in header and "#define ZG_SEAM_HORIZONTAL 1" in header
    assert (L.SEAM_VERTICAL, L.SEAM_HORIZONTAL) == (0, 1)
