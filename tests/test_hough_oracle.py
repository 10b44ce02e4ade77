"""The Hough transform without a GPU: zg_hough_tables_host against the restated init for every size, the restated f64 cos / sin
against mpmath, the table entries a one-ulp change of them could move, the two CPU restatements of compute (tests/hough_ref.py)
against each other, the known answers of the reference's own test, the argument checks of the zg_hough_* entry points, and the
module's boundary (header, bindings, Zig file)."""
import ctypes
import math
import os
import re
from collections import Counter

import numpy as np
import pytest

import zignal_amd as zg
from zignal_amd import _lib as L
from tests import hough_cases as K
from tests import hough_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIZES = range(2, 2049)


def quarter_points(size: int):
    """The entries whose exact value, +-32768, is an integer: t = even_size / 4 and 3 even_size / 4 when even_size % 4 == 0."""
    e = R.even_size(size)
    return {e // 4, 3 * e // 4} if e % 4 == 0 else set()


def test_tables_host_equals_the_restated_init_for_every_size():
    for size in SIZES:
        cos_t, sin_t = zg.HoughTransform.tables(size)
        want_c, want_s = R.tables(size)
        assert np.array_equal(cos_t, want_c) and np.array_equal(sin_t, want_s), size


def test_restated_cos_and_sin_are_within_one_ulp_of_mpmath_at_every_table_angle():
    libmp = pytest.importorskip("mpmath").libmp  # the functions under mpmath.cos / sin, without a context object per value
    angles = sorted({R.theta(t, size) for size in SIZES for t in range(size)})
    worst = 0.0
    for x in angles:
        want_c, want_s = libmp.mpf_cos_sin(libmp.from_float(x), 80)
        for got, want in ((R.cos64(x), want_c), (R.sin64(x), want_s)):
            err = abs(libmp.to_float(libmp.mpf_sub(libmp.from_float(got), want, 30)))  # the subtraction is of 53 and 80 bits: exact enough at 30
            ulp = math.ulp(got) if got != 0.0 else math.ulp(libmp.to_float(want))
            assert err <= ulp, (x, got)
            worst = max(worst, err / ulp)
    print(f"{len(angles)} angles, worst error {worst:.3f} ulp")


def test_no_entry_but_a_quarter_point_can_be_moved_by_one_ulp():
    """Moving the cosine or the sine to a neighbouring f64 changes trunc(65536 * v / sqrt 2) only where the exact entry is an integer,
    +-32768 at the quarter points: everywhere else the host's libm, Zig's and the restatement agree whatever their last bit. Not
    every quarter point is sensitive (at size 220, t = 165 the rounding of theta itself moves the quotient off the integer), so the
    assertion is the inclusion, which is the half exactness rests on; sizes 63, 126, 130, 250 have no quarter point at all."""
    seen = Counter()
    for size in SIZES:
        sensitive = set()
        for t in range(size):
            x = R.theta(t, size)
            for v in (R.cos64(x), R.sin64(x)):
                if len({R.table_entry(u) for u in (math.nextafter(v, -math.inf), v, math.nextafter(v, math.inf))}) > 1:
                    sensitive.add(t)
        assert sensitive <= quarter_points(size), size
        e = R.even_size(size)
        seen["first"] += e // 4 in sensitive
        seen["third"] += 3 * e // 4 in sensitive and e % 4 == 0
    print(dict(seen))
    assert seen["first"] > 0 and seen["third"] > 0  # the probe does find the entries it is meant to find
    for size in (63, 126, 130, 250):
        assert quarter_points(size) == set()


def test_quarter_point_entries_of_size_64_are_pinned():
    """theta = fl(pi) / 4 for a power-of-two even_size: a correctly rounded cosine and sine give 32768 and 32767."""
    for tables in (R.tables(64), zg.HoughTransform.tables(64)):
        cos_t, sin_t = tables
        assert (int(cos_t[16]), int(sin_t[16])) == (32768, 32767)
    for size in (4, 8, 256, 1024, 2048):
        cos_t, sin_t = zg.HoughTransform.tables(size)
        assert (int(cos_t[size // 4]), int(sin_t[size // 4])) == (32768, 32767), size


def random_edges(seed, rows, cols, density):
    rng = np.random.default_rng(seed)
    return np.where(rng.random((rows, cols)) < density, rng.choice(np.array([1, 128, 255], np.uint8), (rows, cols)), 0).astype(np.uint8)


@pytest.mark.parametrize("size,rows,cols,box", [(2, 2, 2, (0, 0, 2, 2)), (3, 5, 4, (1, 1, 4, 4)), (5, 5, 5, (0, 0, 5, 5)), (16, 20, 12, (3, 2, 19, 18)),
                                                (31, 31, 31, (0, 0, 31, 31)), (8, 4, 4, (9, 9, 17, 17))])
def test_the_two_restatements_of_compute_agree(size, rows, cols, box):
    edges = random_edges(size, rows, cols, 0.4)
    a = np.full((size, size), 7, np.uint32)
    b = a.copy()
    ca, cb = Counter(), Counter()
    R.compute(edges, box, a, size, ca)
    R.compute_fast(edges, box, b, size, cb)
    assert np.array_equal(a, b) and ca == cb
    if R.area_of(edges, box) is None:
        assert ca["no_area"] == 1 and (a == 7).all()
    else:
        assert int(a.sum()) - 7 * size * size == ca["vote"] > 0


def test_no_vote_of_a_pixel_inside_the_box_falls_outside_the_accumulator():
    """The rr range check (:112, :133) cannot fail: |rho| <= (size - 1) * 65535, so rho / 131072 lies within (size - 1) / 2 of 0 and
    rr = floor(rho / 131072 + even_size / 2) within [0, size - 1]. Its two counters stay 0 for the corners and full boxes below, and
    no test of the device code can make them count."""
    for size in (2, 3, 4, 5, 63, 64, 97, 300):
        edges = np.zeros((size, size), np.uint8)
        edges[[0, 0, -1, -1], [0, -1, 0, -1]] = 255
        if size <= 64:
            edges[:] = 1
        c = Counter()
        R.compute_fast(edges, (0, 0, size, size), np.zeros((size, size), np.uint32), size, c)
        assert c["vote"] == int(np.count_nonzero(edges)) * size and c["rr_above"] == 0 and c["rr_below"] == 0, size


def horizontal_line_accumulator():
    edges = np.zeros((64, 64), np.uint8)
    edges[32, :] = 255
    return R.compute(edges, (0, 0, 64, 64), np.zeros((64, 64), np.uint32), 64)


def test_known_answers_of_the_reference_test():
    """hough.zig:259-279: 64 x 64 edges with row 32 set. 64 pixels x 64 columns all land inside: the sum is 4096."""
    acc = horizontal_line_accumulator()
    assert int(acc.sum()) == 4096
    n, lines = R.find_lines(acc, 64, 30, 10.0, 5.0)
    assert len(lines) == 1
    assert lines[0]["angle"] == np.float32(1.40625) and lines[0]["radius"] == np.float32(0.70710677) and lines[0]["score"] == 64
    assert abs(float(lines[0]["angle"])) <= 2.0  # what the reference's test asks


def test_known_answer_of_the_pure_tie_order_case():
    c = Counter()
    n, lines = R.find_lines(np.zeros((9, 9), np.uint32), 9, 0, 10.0, 5.0, c)
    assert (n, len(lines)) == (49, 14)
    assert c["sort_ties"] == 48 and c["plateau_candidates"] == 49 and c["suppressed_near"] > 0
    assert lines[0]["angle"] == np.float32(-67.5) and lines[0]["radius"] == np.float32(-4.2426405)


def test_clip_line_branches_that_find_lines_cannot_reach():
    """createLine's segments are never parallel to an axis in f32 at an interior column (angle = -90 is column 0; at 0 and 90 degrees
    the cosine and sine of fl(pi / 2) and fl(pi) are 4e-8 and 9e-8, not 0), so the p == 0 branches are exercised here directly."""
    f = np.float32
    c = Counter()
    p1, p2 = [f(2), f(-3)], [f(2), f(20)]
    R.clip_line(f(0), f(0), f(9), f(9), p1, p2, c)
    assert c["clip_parallel_inside"] == 2 and (p1, p2) == ([f(2), f(0)], [f(2), f(9)])
    p1, p2 = [f(-2), f(-3)], [f(-2), f(20)]
    R.clip_line(f(0), f(0), f(9), f(9), p1, p2, c)
    assert c["clip_parallel_outside"] == 1 and (p1, p2) == ([f(-2), f(-3)], [f(-2), f(20)])
    p1, p2 = [f(-5), f(20)], [f(20), f(30)]
    R.clip_line(f(0), f(0), f(9), f(9), p1, p2, c)
    assert c["clip_leaves_before_entering"] + c["clip_enters_after_leaving"] == 1 and p1 == [f(-5), f(20)]
    assert c["clip_empty"] == 0


def limits():
    return int(zg.lib().zg_hough_lds_max_size()), int(zg.lib().zg_hough_pixel_chunk())


def test_the_shared_find_lines_cases_reach_the_branches_they_are_there_for():
    """What tests/test_gpu_hough.py relies on. Never counted, by any input: the rr range check (above), clip_empty (clip_line's
    docstring) and the two p == 0 branches of clipLine (the test above)."""
    want = {name: K.want_lines(name, *limits()) for name in K.find_cases(*limits())}
    total = sum((c for _, _, c in want.values()), Counter())
    print(dict(total))
    for branch in ("suppressed_near", "suppressed_wrapped", "sort_ties", "plateau_candidates", "clipped", "clip_enter_moves", "clip_enter_stays",
                   "clip_leave_moves", "clip_leave_stays", "clip_enters_after_leaving", "clip_leaves_before_entering", "too_small"):
        assert total[branch] > 0, branch
    for branch in ("clip_empty", "clip_parallel_inside", "clip_parallel_outside"):
        assert total[branch] == 0, branch
    assert want["wrap"][2]["suppressed_wrapped"] == 1 and len(want["wrap"][1]) == 3 and len(want["wrap_off"][1]) == 4
    assert (want["ties9_default"][0], len(want["ties9_default"][1])) == (49, 14)
    for name in ("ties9_nan_angle", "ties9_nan_radius", "ties9_negative", "ties9_zero"):  # strict < with NaN, negative or 0: nothing is suppressed
        assert len(want[name][1]) == 49, name
    assert len(want["ties9_inf"][1]) == 1
    assert want["plateau"][0] == 9 and want["plateau_threshold_above_all"][0] == 0
    assert want["size3"][0] == 1 and want["size2"][0] == 0
    assert max(n for n, _, _ in want.values()) > 256  # more candidates than one workgroup of the sort holds
    assert want["acc_lines97_box_inside"][0] == 3  # the three drawn lines
    # the 256-cell trips of the device's column and row loops: candidates on both sides of every trip's end, few enough for the reference's loops
    for name, n_marks in (("trips259", 1), ("trips515", 2)):
        size, acc, thr, _, _ = K.find_cases(*limits())[name]
        n, lines, counters = want[name]
        cand = R.candidate_mask(acc, size, thr)
        marks, last = K.trip_marks(size), size - 2
        assert len(marks) == n_marks and last == marks[-1] + 1, name
        assert n == int(cand.sum()) and 24 <= n < 300 and len(lines) > n // 2 and counters["sort_ties"] >= 4, (name, n, len(lines))  # two pairs, a plateau
        assert cand[last - 1, last - 1], name  # the last interior row and column
        for m in marks:
            in_row = [c for c in range(m - 1, m + 3) if c <= last]
            assert all(cand[K.TRIP_ROW - 1, c - 1] for c in in_row) and {m, m + 1} <= set(in_row), (name, m)
            assert cand[m - 1].any() and cand[m].any(), (name, m)  # rows m and m + 1
        rows_with = np.nonzero(cand.any(axis=1))[0] + 1
        assert (np.diff(rows_with) > 1).any() and rows_with[0] == 1, name  # empty rows between candidate rows


def test_the_shared_compute_cases_cover_what_they_name():
    lds_max, chunk = limits()
    cases = K.compute_cases(lds_max, chunk)
    assert cases["above_lds"][2] == lds_max + 1
    for name, (edges, box, size, start) in cases.items():
        assert box[2] - box[0] == size and box[3] - box[1] == size, name
        area = R.area_of(edges, box)
        assert (area is None) == name.startswith("box_misses"), name
        if area is not None:
            want = K.want_accumulator(name, lds_max, chunk)
            first = np.zeros((size, size), np.uint32) if start is None else start
            votes = int((want.astype(np.int64) - first.astype(np.int64)).sum())
            assert votes == size * int(np.count_nonzero(edges[area[1]:area[3], area[0]:area[2]])), name
    assert {int(np.count_nonzero(cases[f"edges{n}"][0])) for n in (chunk - 1, chunk, chunk + 1, 2 * chunk + 1)} == {chunk - 1, chunk, chunk + 1, 2 * chunk + 1}
    assert set(np.unique(cases["random97"][0])) == {0, 1, 128, 255}
    assert cases["lines97_box_past_right"][1][2] > cases["lines97_box_past_right"][0].shape[1]
    assert cases["box_past_bottom"][1][3] > cases["box_past_bottom"][0].shape[0]


# ---- the error convention, decided on the host: right without a GPU ----------------------------------------------------------------
def test_create_rejects_sizes_below_two_and_above_the_bound():
    lib = zg.lib()
    h = ctypes.c_void_p()
    t = (ctypes.c_int32 * 4)()
    for size in (0, 1):
        assert lib.zg_hough_create(size, ctypes.byref(h)) == L.ERR_INVALID_ARGUMENT
        assert lib.zg_hough_tables_host(size, t, t) == L.ERR_INVALID_ARGUMENT
        with pytest.raises(zg.InvalidArgument):
            zg.HoughTransform(size)
    assert L.HOUGH_MAX_SIZE == 32768
    for size in (L.HOUGH_MAX_SIZE + 1, 0xFFFFFFFF):
        assert lib.zg_hough_create(size, ctypes.byref(h)) == L.ERR_UNSUPPORTED
        assert lib.zg_hough_tables_host(size, t, t) == L.ERR_UNSUPPORTED
    assert h.value is None


def test_the_size_bound_is_where_the_i32_expressions_stop_fitting():
    """|rho| <= (size - 1) * (|cos| + |sin|) and (rho >> 1) + (offset << 1), with the real tables of the largest size and its corners."""
    size = L.HOUGH_MAX_SIZE
    e = R.even_size(size)
    t = np.arange(0, size, 257, dtype=np.float64)  # a sample of the columns, the quarter point among them
    t = np.unique(np.concatenate([t, [0, e // 4, e // 2, 3 * e // 4, size - 1]]))
    c = np.trunc(65536.0 * np.cos(t * R.PI64 / e) / R.SQRT2_64).astype(np.int64)
    s = np.trunc(65536.0 * np.sin(t * R.PI64 / e) / R.SQRT2_64).astype(np.int64)
    assert int((np.abs(c) + np.abs(s)).max()) <= 65536
    rho = (size - 1) * (np.abs(c) + np.abs(s))
    assert int(rho.max()) <= R.I32_MAX and int((rho >> 1).max()) + (R.offset_of(size) << 1) <= R.I32_MAX
    assert (size + 1 - 1) * 65536 > R.I32_MAX  # the bound of the header's derivation fails one size later


def test_compute_and_find_lines_decide_their_status_before_anything_is_enqueued():
    lib = zg.lib()
    h = ctypes.c_void_p()
    assert lib.zg_hough_create(8, ctypes.byref(h)) == L.OK and lib.zg_hough_size(h) == 8
    try:
        pixels = np.zeros((16, 16), np.uint8)
        acc = np.zeros((8, 8), np.uint32)
        img = L.ZgImage(pixels.ctypes.data, 16, 16, 16, L.PIXEL_U8)
        for box in ((0, 0, 7, 8), (0, 0, 8, 9), (1, 1, 8, 8), (4, 4, 2, 2), (0, 0, 16, 16)):
            for fn, extra in ((lib.zg_hough_compute, (None,)), (lib.zg_hough_compute_host, ())):
                assert fn(h, ctypes.byref(img), *box, acc.ctypes.data, 8, *extra) == L.ERR_DIMENSION_MISMATCH, box
        f32img = L.ZgImage(pixels.ctypes.data, 4, 16, 4, L.PIXEL_F32)
        assert lib.zg_hough_compute_host(h, ctypes.byref(f32img), 0, 0, 8, 8, acc.ctypes.data, 8) == L.ERR_UNSUPPORTED
        assert lib.zg_hough_compute_host(h, ctypes.byref(img), 0, 0, 8, 8, acc.ctypes.data, 7) == L.ERR_INVALID_ARGUMENT
        assert lib.zg_hough_compute_host(h, ctypes.byref(img), 0, 0, 8, 8, None, 8) == L.ERR_INVALID_ARGUMENT
        counts = (ctypes.c_uint32 * 2)()
        assert lib.zg_hough_find_lines_host(h, acc.ctypes.data, 8, 0, 10.0, 5.0, L.HOUGH_MAX_CANDIDATES + 1, None, 0, counts) == L.ERR_UNSUPPORTED
        assert lib.zg_hough_find_lines_host(h, acc.ctypes.data, 8, 0, 10.0, 5.0, 16, None, 4, counts) == L.ERR_INVALID_ARGUMENT
        assert lib.zg_hough_find_lines_host(h, acc.ctypes.data, 7, 0, 10.0, 5.0, 16, None, 0, counts) == L.ERR_INVALID_ARGUMENT
        assert lib.zg_hough_find_lines_host(h, acc.ctypes.data, 8, 0, 10.0, 5.0, 16, None, 0, None) == L.ERR_INVALID_ARGUMENT
        with pytest.raises(zg.DimensionMismatch):
            zg.HoughTransform(8).compute(pixels, (0, 0, 9, 8))
    finally:
        assert lib.zg_hough_destroy(h) == L.OK
    assert lib.zg_hough_destroy(None) == L.OK


# ---- the module's boundary -----------------------------------------------------------------------------------------------------------
def _hough_header():
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "zignal_hip_hough.h")).read(), flags=re.S)
    protos = re.findall(r"ZG_API\s+[\w\s\*]+?\b(zg_\w+)\s*\(([^;]*?)\)\s*;", text, flags=re.S)
    return {name: ([] if args.strip() == "void" else args.split(",")) for name, args in protos}


def test_hough_header_bindings_and_zig_file_declare_the_same_symbols():
    protos = _hough_header()
    assert sorted(protos) == sorted(L.HOUGH_EXPORTED_SYMBOLS) and len(protos) == 11
    raw = ctypes.CDLL(L.LIB_PATH)
    for name, args in protos.items():
        assert hasattr(raw, name), f"{name} declared in include/zignal_hip_hough.h but not exported"
        assert len(L._HOUGH_SIGNATURES[name]) == len(args), name
    assert not set(L.HOUGH_EXPORTED_SYMBOLS) & (set(L.EXPORTED_SYMBOLS) | set(L.ORB_EXPORTED_SYMBOLS) | set(L.MATCH_EXPORTED_SYMBOLS))
    shim = open(os.path.join(ROOT, "zig", "zignal_hip_hough.zig")).read()
    externs = dict(re.findall(r"pub extern fn (zg_\w+)\(([^)]*)\)", shim))
    assert set(externs) == set(protos)
    for name, args in externs.items():
        assert len([a for a in args.split(",") if a.strip()]) == len(protos[name]), name
    main = open(os.path.join(ROOT, "include", "zignal_hip.h")).read()
    assert main.index('#include "zignal_hip_match.h"') < main.index('#include "zignal_hip_hough.h"')
    assert zg.HOUGH_LINE_DTYPE.itemsize == 28 == ctypes.sizeof(L.ZgHoughLine)
    assert [zg.HOUGH_LINE_DTYPE.fields[n][1] for n in ("angle", "radius", "score", "p1", "p2")] == [0, 4, 8, 12, 20]
    assert zg.HoughLine._fields == ("angle", "radius", "score", "p1", "p2")
    makefile = open(os.path.join(ROOT, "zignal_amd", "csrc", "Makefile")).read()  # both object rules depend on every header of include/
    assert "$(wildcard ../../include/*.h)" in makefile and makefile.count("$(HEADERS)") == 2
    assert os.path.isfile(os.path.join(ROOT, "include", "zignal_hip_hough.h"))
    header = open(os.path.join(ROOT, "include", "zignal_hip_hough.h")).read()
    assert f"#define ZG_HOUGH_MAX_SIZE {L.HOUGH_MAX_SIZE}u" in header and f"#define ZG_HOUGH_MAX_CANDIDATES {L.HOUGH_MAX_CANDIDATES}u" in header
    assert L.HOUGH_MAX_CANDIDATES >= 65536


def test_the_lds_limit_and_the_pixel_chunk_are_host_constants():
    lib = zg.lib()
    assert 128 <= lib.zg_hough_lds_max_size() < L.HOUGH_MAX_SIZE
    assert lib.zg_hough_pixel_chunk() >= 256
