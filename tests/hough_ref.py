"""HoughTransform (reference src/image/hough.zig) restated on the CPU, for the tests of zg_hough_*.

init, compute, findLines, getLineProperties, createLine and clipLine as they are written there: i32 arithmetic carried in Python
integers and checked against the i32 range at every step, f32 arithmetic in numpy float32 scalars one operation at a time, @sin / @cos
of an f32 from the oracle library's zo_sinf / zo_cosf (as tests/orb_ref.py takes them) and @cos / @sin of an f64 restated below from
musl's __cos / __sin / __rem_pio2, which Zig's compiler-rt ports. compute_fast is a second, vectorised compute for large sparse inputs.

Every function that has branches counts them in the `counters` dictionary it is given; the tests assert the counters they rely on."""
import ctypes as C
import functools
import struct
from collections import Counter

import numpy as np

from oracle import pyoracle as oracle
from zignal_amd import HOUGH_LINE_DTYPE

f32 = np.float32
I32_MIN, I32_MAX = -(1 << 31), (1 << 31) - 1


def i32(v: int) -> int:
    """An i32 result: Zig traps on overflow, so a value out of range is a mistake of the test's input."""
    assert I32_MIN <= v <= I32_MAX, f"i32 overflow: {v}"
    return v


def sinf(x) -> np.float32:
    return f32(oracle.lib().zo_sinf(C.c_float(x)))


def cosf(x) -> np.float32:
    return f32(oracle.lib().zo_cosf(C.c_float(x)))


# ---- @cos / @sin of an f64 -----------------------------------------------------------------------------------------------------
def _high_word(x: float) -> int:
    return struct.unpack("<Q", struct.pack("<d", x))[0] >> 32


def _k_sin(x: float, y: float, iy: int) -> float:
    S1, S2, S3 = -1.66666666666666324348e-01, 8.33333333332248946124e-03, -1.98412698298579493134e-04
    S4, S5, S6 = 2.75573137070700676789e-06, -2.50507602534068634195e-08, 1.58969099521155010221e-10
    z = x * x
    w = z * z
    r = S2 + z * (S3 + z * S4) + z * w * (S5 + z * S6)
    v = z * x
    if iy == 0:
        return x + v * (S1 + z * r)
    return x - ((z * (0.5 * y - v * r) - y) - v * S1)


def _k_cos(x: float, y: float) -> float:
    C1, C2, C3 = 4.16666666666666019037e-02, -1.38888888888741095749e-03, 2.48015872894767294178e-05
    C4, C5, C6 = -2.75573143513906633035e-07, 2.08757232129817482790e-09, -1.13596475577881948265e-11
    z = x * x
    w = z * z
    r = z * (C1 + z * (C2 + z * C3)) + w * w * (C4 + z * (C5 + z * C6))
    hz = 0.5 * z
    w = 1.0 - hz
    return w + (((1.0 - w) - hz) + (z * r - x * y))


def _rem_pio2(x: float):
    """The medium path of __rem_pio2 (|x| < 2^20 pi/2); the special cases below 9 pi/4 do the same steps."""
    toint, pio4, invpio2 = 1.5 / 2.220446049250313e-16, float.fromhex("0x1.921fb54442d18p-1"), 6.36619772367581382433e-01
    pio2_1, pio2_1t = 1.57079632673412561417e+00, 6.07710050650619224932e-11
    pio2_2, pio2_2t = 6.07710050630396597660e-11, 2.02226624879595063154e-21
    pio2_3, pio2_3t = 2.02226624871116645580e-21, 8.47842766036889956997e-32
    ix = _high_word(x) & 0x7FFFFFFF
    fn = x * invpio2 + toint - toint
    n = int(fn)
    r, w = x - fn * pio2_1, fn * pio2_1t
    if r - w < -pio4:
        n, fn = n - 1, fn - 1.0
        r, w = x - fn * pio2_1, fn * pio2_1t
    elif r - w > pio4:
        n, fn = n + 1, fn + 1.0
        r, w = x - fn * pio2_1, fn * pio2_1t
    y0 = r - w
    ey, ex = _high_word(y0) >> 20 & 0x7FF, ix >> 20
    if ex - ey > 16:
        t = r
        w = fn * pio2_2
        r = t - w
        w = fn * pio2_2t - ((t - r) - w)
        y0 = r - w
        ey = _high_word(y0) >> 20 & 0x7FF
        if ex - ey > 49:
            t = r
            w = fn * pio2_3
            r = t - w
            w = fn * pio2_3t - ((t - r) - w)
            y0 = r - w
    return n, y0, (r - y0) - w


@functools.lru_cache(maxsize=None)
def cos64(x: float) -> float:
    ix = _high_word(x) & 0x7FFFFFFF
    if ix <= 0x3FE921FB:
        return 1.0 if ix < 0x3E46A09E else _k_cos(x, 0.0)
    n, y0, y1 = _rem_pio2(x)
    return (_k_cos(y0, y1), -_k_sin(y0, y1, 1), -_k_cos(y0, y1), _k_sin(y0, y1, 1))[n & 3]


@functools.lru_cache(maxsize=None)
def sin64(x: float) -> float:
    ix = _high_word(x) & 0x7FFFFFFF
    if ix <= 0x3FE921FB:
        return x if ix < 0x3E500000 else _k_sin(x, 0.0, 0)
    n, y0, y1 = _rem_pio2(x)
    return (_k_sin(y0, y1, 1), _k_cos(y0, y1), -_k_sin(y0, y1, 1), -_k_cos(y0, y1))[n & 3]


PI64, SQRT2_64 = 3.141592653589793, 1.4142135623730951


def even_size(size: int) -> int:
    return size if size % 2 == 0 else size - 1


def theta(t: int, size: int) -> float:
    return float(t) * PI64 / float(even_size(size))  # :53


def table_entry(value: float) -> int:
    return int(65536.0 * value / SQRT2_64)  # @trunc: int() truncates towards zero


@functools.lru_cache(maxsize=None)
def tables(size: int):
    """init (:38-66): (cos_table, sin_table) as read-only int32 arrays."""
    assert size > 1
    c = np.array([table_entry(cos64(theta(t, size))) for t in range(size)], np.int32)
    s = np.array([table_entry(sin64(theta(t, size))) for t in range(size)], np.int32)
    c.setflags(write=False)
    s.setflags(write=False)
    return c, s


def offset_of(size: int) -> int:
    return i32(int(round(65536.0 * float(even_size(size)) / 4.0)))  # :84, exact


def area_of(edges, box):
    """box.intersect(edges.getRectangle()) (:79): (l, t, r, b) or None."""
    l, t, r, b = box
    rows, cols = edges.shape
    ar, ab = min(r, cols), min(b, rows)
    return None if l >= ar or t >= ab else (l, t, ar, ab)


# ---- compute -------------------------------------------------------------------------------------------------------------------
def compute(edges, box, acc, size, counters=None):
    """compute (:75-139), a loop for a loop (the four-fold unrolling computes what the remainder loop computes). Adds to acc."""
    counters = Counter() if counters is None else counters
    l, t, r, b = box
    assert r - l == size and b - t == size and acc.shape == (size, size)
    area = area_of(edges, box)
    if area is None:
        counters["no_area"] += 1
        return acc
    cos_t, sin_t = (x.tolist() for x in tables(size))
    size_minus_one, offset = size - 1, offset_of(size)
    off2 = i32(offset << 1)
    for row in range(area[1], area[3]):
        y_val = i32(2 * (row - t) - size_minus_one)
        y_cache = [i32(y_val * sin_t[k]) for k in range(size)]
        for col in range(area[0], area[2]):
            if edges[row, col] == 0:
                continue
            x_val = i32(2 * (col - l) - size_minus_one)
            for k in range(size):
                rho = i32(i32(x_val * cos_t[k]) + y_cache[k])
                rr = i32((rho >> 1) + off2) >> 16
                if 0 <= rr < size:
                    acc[rr, k] += 1
                    counters["vote"] += 1
                elif rr < 0:
                    counters["rr_below"] += 1
                else:
                    counters["rr_above"] += 1
    return acc


def compute_fast(edges, box, acc, size, counters=None):
    """The same accumulator from the list of non-zero pixels, all theta columns at once in int64 with the i32 range asserted."""
    counters = Counter() if counters is None else counters
    l, t, r, b = box
    assert r - l == size and b - t == size and acc.shape == (size, size)
    area = area_of(edges, box)
    if area is None:
        counters["no_area"] += 1
        return acc
    cos_t, sin_t = (x.astype(np.int64) for x in tables(size))
    rows, cols = np.nonzero(edges[area[1]:area[3], area[0]:area[2]])
    off2 = offset_of(size) << 1
    cols_idx = np.arange(size)
    for i0 in range(0, len(rows), 4096):
        y = 2 * rows[i0:i0 + 4096].astype(np.int64) - (size - 1)  # the area starts at the box's corner
        x = 2 * cols[i0:i0 + 4096].astype(np.int64) - (size - 1)
        rho = x[:, None] * cos_t[None, :] + y[:, None] * sin_t[None, :]
        s = (rho >> 1) + off2
        assert rho.min(initial=0) >= I32_MIN and rho.max(initial=0) <= I32_MAX and s.max(initial=0) <= I32_MAX and s.min(initial=0) >= I32_MIN
        rr = s >> 16
        ok = (rr >= 0) & (rr < size)
        counters["vote"] += int(ok.sum())
        counters["rr_below"] += int((rr < 0).sum())
        counters["rr_above"] += int((rr >= size).sum())
        np.add.at(acc, (rr[ok], np.broadcast_to(cols_idx, rr.shape)[ok]), 1)
    return acc


# ---- findLines -----------------------------------------------------------------------------------------------------------------
def line_properties(size, theta_idx, rho_idx):
    """getLineProperties (:207-212)."""
    center_val = f32(size - 1) / f32(2.0)
    angle = f32(180.0) * (f32(theta_idx) - center_val) / f32(even_size(size))
    radius = (f32(rho_idx) - center_val) * np.sqrt(f32(2.0))
    return f32(angle), f32(radius)


def clip_line(l, t, r, b, p1, p2, counters):
    """clipLine (:232-257) on [x, y] lists of f32, in place. `empty` (t0 > t1 at the end) cannot be counted by any input: an entering
    ratio above t1 and a leaving one below t0 have returned before, so t0 <= t1 holds after every step."""
    t0, t1 = f32(0.0), f32(1.0)
    dx, dy = f32(p2[0] - p1[0]), f32(p2[1] - p1[1])
    p = [f32(-dx), dx, f32(-dy), dy]
    q = [f32(p1[0] - l), f32(r - p1[0]), f32(p1[1] - t), f32(b - p1[1])]
    for i in range(4):
        if p[i] == 0:
            if q[i] < 0:
                counters["clip_parallel_outside"] += 1
                return
            counters["clip_parallel_inside"] += 1
        else:
            ratio = f32(q[i] / p[i])
            if p[i] < 0:
                if ratio > t1:
                    counters["clip_enters_after_leaving"] += 1
                    return
                if ratio > t0:
                    t0 = ratio
                    counters["clip_enter_moves"] += 1
                else:
                    counters["clip_enter_stays"] += 1
            else:
                if ratio < t0:
                    counters["clip_leaves_before_entering"] += 1
                    return
                if ratio < t1:
                    t1 = ratio
                    counters["clip_leave_moves"] += 1
                else:
                    counters["clip_leave_stays"] += 1
    if t0 > t1:
        counters["clip_empty"] += 1
        return
    counters["clipped"] += 1
    ox, oy = p1[0], p1[1]
    p1[0], p1[1] = f32(ox + f32(t0 * dx)), f32(oy + f32(t0 * dy))
    p2[0], p2[1] = f32(ox + f32(t1 * dx)), f32(oy + f32(t1 * dy))


def create_line(size, angle, radius, score, counters):
    """createLine (:214-229): (angle, radius, score, p1, p2)."""
    center = f32(size - 1) / f32(2.0)
    theta_rad = f32(f32(f32(angle + f32(90.0)) * f32(np.pi)) / f32(180.0))
    cos_t, sin_t = cosf(theta_rad), sinf(theta_rad)
    pcx, pcy = f32(radius * cos_t), f32(radius * sin_t)
    dir_x, dir_y = f32(-sin_t), cos_t
    huge = f32(size) * f32(2.0)
    p1 = [f32(f32(center + pcx) + f32(dir_x * huge)), f32(f32(center + pcy) + f32(dir_y * huge))]
    p2 = [f32(f32(center + pcx) - f32(dir_x * huge)), f32(f32(center + pcy) - f32(dir_y * huge))]
    clip_line(f32(0), f32(0), f32(size), f32(size), p1, p2, counters)
    return angle, radius, score, p1, p2


def candidate_mask(acc, size, threshold):
    """:158-170 for every interior cell at once: [r - 1, c - 1] says whether cell (r, c) is a candidate (size >= 3)."""
    a = acc.astype(np.int64)
    # the 3 x 3 maximum around every interior cell, the cell itself included: no neighbour is strictly greater when it equals the cell
    nb = np.max([a[1 + dr:size - 1 + dr, 1 + dc:size - 1 + dc] for dr in (-1, 0, 1) for dc in (-1, 0, 1)], axis=0)
    inner = a[1:-1, 1:-1]
    return (inner >= threshold) & (nb == inner)


def find_lines(acc, size, threshold, angle_nms_thresh, radius_nms_thresh, counters=None):
    """findLines (:142-204) of a size x size accumulator: (number of candidates, HOUGH_LINE_DTYPE array)."""
    counters = Counter() if counters is None else counters
    assert acc.shape == (size, size)
    out = []
    if size < 3:
        counters["too_small"] += 1
        return 0, np.zeros(0, HOUGH_LINE_DTYPE)
    a = acc.astype(np.int64)
    inner = a[1:-1, 1:-1]
    is_cand = candidate_mask(acc, size, threshold)
    rows, cols = np.nonzero(is_cand)  # row-major order
    counters["plateau_candidates"] += int((is_cand & (
        np.sum([a[1 + dr:size - 1 + dr, 1 + dc:size - 1 + dc] == inner for dr in (-1, 0, 1) for dc in (-1, 0, 1)], axis=0) > 1)).sum())
    cands = []
    for r, c in zip((rows + 1).tolist(), (cols + 1).tolist()):
        angle, radius = line_properties(size, c, r)
        cands.append((angle, radius, int(acc[r, c]), r, c))
    cands.sort(key=lambda x: -x[2])  # std.mem.sort is stable; so is this
    counters["sort_ties"] += sum(1 for x, y in zip(cands, cands[1:]) if x[2] == y[2])
    a_thr, r_thr = f32(angle_nms_thresh), f32(radius_nms_thresh)
    kept = []
    for cand in cands:
        too_close = False
        for ex in kept:
            da = np.abs(f32(ex[0] - cand[0]))
            dr = np.abs(f32(ex[1] - cand[1]))
            if da < a_thr and dr < r_thr:
                counters["suppressed_near"] += 1
                too_close = True
                break
            if f32(f32(180.0) - da) < a_thr and np.abs(f32(ex[1] + cand[1])) < r_thr:
                counters["suppressed_wrapped"] += 1
                too_close = True
                break
        if not too_close:
            kept.append(cand)
    for angle, radius, score, _, _ in kept:
        out.append(create_line(size, angle, radius, score, counters))
    lines = np.zeros(len(out), HOUGH_LINE_DTYPE)
    for i, (angle, radius, score, p1, p2) in enumerate(out):
        lines[i] = (angle, radius, score, p1, p2)
    return len(cands), lines
