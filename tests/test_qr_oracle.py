"""tests/qr_ref.py, the restatement of the reference's QR detector (src/qrcode/detector.zig:57-641), held to what a detector has to do:
on clean renders of planted module matrices (tests/qr_cases.py) it returns the planted matrix, the planted corners and, for versions
7 and 10, the planted version; rotated and mirrored renders still give the matrix under one of decoder.orientedModule's eight
orientations. The reference's own tests need its encoder and its decoder, which are outside this project; these properties are what
stands behind the restatement the device is compared with. Every case asserts that no cast of the restatement was undefined.
Also here: the new entry points are exported with the documented signatures (no GPU needed)."""
import os
import re

import numpy as np
import pytest

from tests import qr_cases as K
from tests import qr_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PX = 4


@pytest.mark.parametrize("version", (1, 2, 7, 10))
def test_clean_axis_aligned_renders_give_the_planted_matrix(version):
    mat = K.matrix(version)
    dim = mat.shape[0]
    h = K.shift(9, 6)
    s = K.side(version, PX)
    frame = K.render(mat, PX, s + 15, s + 21, h)
    res = R.detect(K.binarize(frame))
    assert R.UNDEFINED_CASTS[0] == 0
    assert res["triple"] is not None and res["estimate"] == version and res["versions"][0] == version
    first = res["grids"][0]
    assert first["version"] == version and np.array_equal(first["modules"], mat)
    planted = K.planted_corners(dim, PX, h)
    assert np.abs(first["corners"].reshape(4, 2) - planted).max() <= PX / 2
    assert first["version_hint"] == (version if version >= 7 else -1)
    if version >= 2:
        assert res["fourths"][0][2] and first["fourth_index"] == 0  # the alignment pattern was found and used first
        ax, ay = K.apply(h, (K.QUIET + dim - 6.5) * PX, (K.QUIET + dim - 6.5) * PX)
        assert abs(res["fourths"][0][0] - ax) <= PX / 2 and abs(res["fourths"][0][1] - ay) <= PX / 2
    else:
        assert [f[2] for f in res["fourths"]] == [False]
    tl, tr, bl = res["triple"]
    for got, (mx, my) in zip((tl, tr, bl), ((3.5, 3.5), (dim - 3.5, 3.5), (3.5, dim - 3.5))):
        x, y = K.apply(h, (K.QUIET + mx) * PX, (K.QUIET + my) * PX)
        assert abs(got[0] - x) <= PX / 2 and abs(got[1] - y) <= PX / 2 and abs(got[2] - PX) <= 0.5


@pytest.mark.parametrize("kind", ("rot90", "rot180", "rot37", "mirror"))
def test_rotated_and_mirrored_renders_give_the_matrix_in_one_of_eight_orientations(kind):
    version = 3
    mat = K.matrix(version)
    s = K.side(version, PX)
    n = int(s * 1.5) | 1
    centre = K.shift(n / 2 - s / 2, n / 2 - s / 2)
    h = K.rotation({"rot90": 90, "rot180": 180, "rot37": 37, "mirror": 0}[kind], n / 2, n / 2) @ centre
    frame = K.render(mat, PX, n, n, h, mirror=kind == "mirror")
    res = R.detect(K.binarize(frame))
    assert R.UNDEFINED_CASTS[0] == 0
    assert len(res["grids"]) >= 1
    grids = [g["modules"] for g in res["grids"] if g["version"] == version]
    assert any(np.array_equal(R.oriented(g, o), mat) for g in grids for o in range(8))
    if kind == "mirror":  # only a mirrored orientation can match
        assert not any(np.array_equal(R.oriented(g, o), mat) for g in grids for o in range(4))


def test_the_version_codewords_are_a_code_of_distance_eight():
    words = [R.version_codeword(v) for v in range(7, 41)]
    assert words[0] == 0x07C94  # version 7's, the one value every description of the symbology quotes
    assert min(bin(a ^ b).count("1") for i, a in enumerate(words) for b in words[:i]) == 8
    assert all(w >> 12 == v for v, w in zip(range(7, 41), words))


def test_frames_below_21_pixels_are_empty():
    assert R.detect(np.zeros((20, 40), np.uint8))["merged_count"] == 0 and R.detect(np.zeros((40, 20), np.uint8))["grids"] == []


def test_the_merge_keeps_what_the_buffer_held_behind_the_filtered_list():
    """:102-109 compacts in place: with fewer than three confirmed entries the list stays as long as it was, its head overwritten."""
    buf = []
    for p in ((10, 10), (100, 10), (10, 100), (100, 100)):
        R.add_candidate(buf, (R.F(p[0]), R.F(p[1]), R.F(3)))
    R.add_candidate(buf, (R.F(101), R.F(100), R.F(3)))
    assert len(buf) == 4 and [float(f[3]) for f in buf] == [1, 1, 1, 2] and float(buf[3][0]) == 100.5


# ---- the entry points ------------------------------------------------------------------------------------------------------------------
def _declared():
    text = open(os.path.join(ROOT, "include", "zignal_hip_qr.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    out = {}
    for m in re.finditer(r"ZG_API\s+[\w\s\*]+?\b(zg_\w+)\s*\(([^)]*)\)\s*;", text):
        params = m.group(2).strip()
        out[m.group(1)] = 0 if params in ("", "void") else params.count(",") + 1
    return out


def test_the_new_symbols_load_with_the_documented_signatures():
    from zignal_amd import _lib as L
    import ctypes as C
    declared = _declared()
    assert set(declared) == set(L.QR_EXPORTED_SYMBOLS) == {"zg_qr_sizeof_detection", "zg_qr_sizeof_grid", "zg_qr_scratch_bytes", "zg_qr_detect", "zg_qr_detect_host",
                                                            "zg_canvas_cmds_from_qr"}
    lib = L.lib()
    for name, n in declared.items():
        assert len(L._QR_SIGNATURES[name]) == n, name
        assert getattr(lib, name).argtypes == L._QR_SIGNATURES[name]
    assert lib.zg_qr_sizeof_detection() == C.sizeof(L.ZgQrDetection) == R.DETECTION_DTYPE.itemsize
    assert lib.zg_qr_sizeof_grid() == C.sizeof(L.ZgQrGrid) == R.GRID_DTYPE.itemsize
    assert '#include "zignal_hip_qr.h"' in open(os.path.join(ROOT, "include", "zignal_hip.h")).read()
    zig = open(os.path.join(ROOT, "zig", "zignal_hip_qr.zig")).read()
    assert set(re.findall(r"extern fn (zg_\w+)", zig)) == set(declared)
    import zignal_amd as zg
    assert zg.QrDetector and zg.QrGrid and zg.qr.DETECTION_DTYPE == R.DETECTION_DTYPE and zg.qr.GRID_DTYPE == R.GRID_DTYPE
