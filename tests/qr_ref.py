"""The QR detector of the reference (src/qrcode/detector.zig:57-641, and decoder.readVersion, decoder.zig:147-162) restated in Python:
what the device (zignal_amd/csrc/qr.hip) is held to, byte for byte. Every f32 step is one numpy.float32 operation in the reference's
order, every f64 step a Python float. `detect(binary)` is detectAndDecode (:86-156) on a binary map (a pixel is dark iff its byte is 0)
without the decoder: every trial that passed sampleTimingLines, timingOk and sampleGrid is recorded, in the order of the loops, and
every intermediate result comes back. `pack` lays a result out as the device's records (include/zignal_hip_qr.h).

Three steps that the reference's text does not pin, restated as its compiler emits them:
  * ProjectiveTransform.project is SMatrix.dot, a gemm whose 3 x 1 product is ((m0 x + m1 y) + m2 1) per row for every vector length
    a target can choose (SMatrix.zig:527-560);
  * @round in estimateVersion (:404) rounds ties away from zero;
  * a float cast to an integer outside its range (or NaN) has no defined result: `_cast` counts them in UNDEFINED_CASTS, and every
    test asserts that the counter stays 0."""
import math

import numpy as np

F = np.float32
UNDEFINED_CASTS = [0]

MAX_FINDERS, MAX_VERSIONS, MAX_FOURTHS = 64, 8, 5
SCAN_TOL, CROSS_TOL, DIAG_TOL = F(0.5), F(0.7), F(0.8)

FOURTH_DTYPE = np.dtype([("x", "<f4"), ("y", "<f4"), ("is_alignment", "<u4")])
DETECTION_DTYPE = np.dtype([("finders", "<f4", (MAX_FINDERS, 4)), ("finder_count", "<u4"), ("merged_count", "<u4"), ("triple_found", "<u4"),
                            ("triple", "<f4", (3, 4)), ("version_estimate", "<u4"), ("version_count", "<u4"), ("versions", "u1", (MAX_VERSIONS,)),
                            ("fourth_count", "<u4"), ("fourths", FOURTH_DTYPE, (MAX_FOURTHS,)), ("grids_total", "<u4"), ("grids_written", "<u4"),
                            ("modules_written", "<u4")])
GRID_DTYPE = np.dtype([("version", "<u4"), ("dim", "<u4"), ("fourth_index", "<u4"), ("modules_offset", "<u4"), ("version_hint", "<i4"),
                       ("corners", "<f4", (8,)), ("reserved", "<u4"), ("transform", "<f8", (9,))])
assert DETECTION_DTYPE.itemsize == 1176 and GRID_DTYPE.itemsize == 128


def _cast(v, hi=1 << 63):
    """@intFromFloat: truncation toward zero; outside [0, hi) or NaN it is undefined, counted, and 0 here."""
    v = float(v)
    if not math.isfinite(v) or v <= -1.0 or v >= hi:
        UNDEFINED_CASTS[0] += 1
        return 0
    return int(v)


# ---- checkRatio, traceRuns, crossCheck, confirmCandidate (:210-307) ----------------------------------------------------------------
def check_ratio(runs, tolerance):
    total = 0
    for r in runs:
        if r == 0:
            return False
        total += r
    if total < 7:
        return False
    unit = F(total) / F(7)
    for run, expected in zip(runs, (1, 1, 3, 1, 1)):
        eu = F(expected) * unit
        if abs(F(run) - eu) > eu * tolerance:
            return False
    return True


def trace_runs(dark, r, c, dr, dc, limit=None):
    rows, cols = dark.shape
    runs = [0, 0, 0]
    state = 0
    while 0 <= r < rows and 0 <= c < cols:
        if bool(dark[r, c]) != (state != 1):
            if state == 2:
                break
            state += 1
            continue
        runs[state] += 1
        if limit is not None:
            if state == 2:
                return runs
            if runs[state] > limit:
                return None
        r += dr
        c += dc
    if runs[1] == 0 or runs[2] == 0:
        return None
    return runs


def cross_center(base, forward, total):
    return F(base + 1 + forward) - F(total) / F(2)


def cross_check(dark, row, col, dr, dc, tolerance):
    back = trace_runs(dark, row, col, -dr, -dc)
    if back is None:
        return None
    fwd = trace_runs(dark, row + dr, col + dc, dr, dc)
    if fwd is None:
        return None
    runs = (back[2], back[1], back[0] + fwd[0], fwd[1], fwd[2])
    if not check_ratio(runs, tolerance):
        return None
    return sum(runs), fwd[0] + fwd[1] + fwd[2]


def confirm_candidate(dark, row, col):
    """(x, y, module_size) or None."""
    if col >= dark.shape[1] or not dark[row, col]:
        return None
    v = cross_check(dark, row, col, 1, 0, CROSS_TOL)
    if v is None:
        return None
    center_row = cross_center(row, v[1], v[0])
    crow = _cast(center_row)
    if not dark[crow, col]:
        return None
    h = cross_check(dark, crow, col, 0, 1, CROSS_TOL)
    if h is None:
        return None
    center_col = cross_center(col, h[1], h[0])
    ccol = _cast(center_col)
    if not dark[crow, ccol]:
        return None
    if cross_check(dark, crow, ccol, 1, 1, DIAG_TOL) is None:
        return None
    return center_col, center_row, F(v[0] + h[0]) / F(14)


def row_hits(dark, row):
    """findFinderPatterns' inner loop on one row (:183-206): the confirmed patterns in column order. The windows are tested together:
    the same single f32 operations on arrays."""
    line = dark[row]
    cols = line.shape[0]
    change = np.flatnonzero(line[1:] != line[:-1]) + 1
    starts = np.concatenate(([0], change))
    ends = np.concatenate((change, [cols]))
    lengths = ends - starts
    k = np.arange(4, len(lengths))
    k = k[line[starts[k]]]  # the windows that end with a dark run
    if len(k) == 0:
        return []
    w = np.stack([lengths[k - 4 + i] for i in range(5)])  # all > 0: a run has a pixel
    total = w.sum(axis=0)
    unit = total.astype(F) / F(7)
    ok = total >= 7
    for i, expected in enumerate((1, 1, 3, 1, 1)):
        eu = F(expected) * unit
        ok &= ~(np.abs(w[i].astype(F) - eu) > eu * SCAN_TOL)
    out = []
    for j in np.flatnonzero(ok):
        r = [int(x) for x in w[:, j]]
        assert check_ratio(r, SCAN_TOL)
        mid_start = int(ends[k[j]]) - r[4] - r[3] - r[2]
        p = confirm_candidate(dark, row, mid_start + r[2] // 2)
        if p is not None:
            out.append(p)
    return out


def add_candidate(buf, pattern):
    """addCandidate (:309-326); buf entries are [x, y, module_size, hits]."""
    px, py, pms = pattern
    for e in buf:
        near = F(2) * e[2]
        if abs(e[0] - px) < near and abs(e[1] - py) < near:
            w = e[3]
            s = F(1) / (w + F(1))
            e[0] = (e[0] * w + px) * s
            e[1] = (e[1] * w + py) * s
            e[2] = (e[2] * w + pms) / (w + F(1))
            e[3] = e[3] + F(1)
            return
    if len(buf) < MAX_FINDERS:
        buf.append([px, py, pms, F(1)])


# ---- pickFinderTriple, estimateVersion (:342-406) ----------------------------------------------------------------------------------
def _dist(a, b):
    dx, dy = a[0] - b[0], a[1] - b[1]
    return np.sqrt(dx * dx + dy * dy)


def triple_score(a, b, c):
    """One (a, b, c) of the loops: None where the reference continues, else (score, (corner, top right, bottom left))."""
    ms_max = max(a[2], max(b[2], c[2]))
    ms_min = min(a[2], min(b[2], c[2]))
    if ms_max > F(1.6) * ms_min:
        return None
    ms = (a[2] + b[2] + c[2]) / F(3)
    ab, ac, bc = _dist(a, b), _dist(a, c), _dist(b, c)
    corner, m1, m2 = c, a, b
    if bc >= ab and bc >= ac:
        corner, m1, m2 = a, b, c
    elif ac >= ab and ac >= bc:
        corner, m1, m2 = b, a, c
    v1 = (m1[0] - corner[0], m1[1] - corner[1])
    v2 = (m2[0] - corner[0], m2[1] - corner[1])
    len1 = np.sqrt(v1[0] * v1[0] + v1[1] * v1[1])
    len2 = np.sqrt(v2[0] * v2[0] + v2[1] * v2[1])
    if min(len1, len2) < F(10) * ms:
        return None
    imbalance = abs(len1 - len2) / max(len1, len2)
    if imbalance > F(0.35):
        return None
    cos = (v1[0] * v2[0] + v1[1] * v2[1]) / (len1 * len2)
    if abs(cos) > F(0.35):
        return None
    triple = (corner, m1, m2) if v1[0] * v2[1] - v1[1] * v2[0] > 0 else (corner, m2, m1)
    return (ms_max - ms_min) / ms + imbalance + abs(cos), triple


def pick_finder_triple(finders):
    best_score, best = np.finfo(F).max, None
    n = len(finders)
    ms = np.array([f[2] for f in finders], F)
    for i in range(n):
        for j in range(i + 1, n):
            for k in range(j + 1, n):
                hi, lo = max(ms[i], ms[j], ms[k]), min(ms[i], ms[j], ms[k])
                if hi > F(1.6) * lo:  # the loop's first test, before the distances
                    continue
                r = triple_score(finders[i], finders[j], finders[k])
                if r is not None and r[0] < best_score:
                    best_score, best = r
    return best


def module_size(triple):
    return (triple[0][2] + triple[1][2] + triple[2][2]) / F(3)


def estimate_version(triple):
    tl, tr, bl = triple
    side = (_dist(tl, tr) + _dist(tl, bl)) / F(2)
    dim_est = side / module_size(triple) + F(7)
    q = (dim_est - F(17)) / F(4)
    version = F(math.floor(abs(float(q)) + 0.5)) * (F(-1) if q < 0 else F(1))  # @round: ties away from zero (exact: |q| is an f32)
    version = min(max(version, F(1)), F(40))
    return _cast(version, 256)


# ---- fourthCandidates (:442-562) ---------------------------------------------------------------------------------------------------
def near_module(length, expected):
    return abs(F(length) - expected) <= expected * F(0.6)


def alignment_axis(dark, row, col, dr, dc, ms, limit):
    back = trace_runs(dark, row, col, -dr, -dc, limit)
    if back is None or not near_module(back[1], ms):
        return None
    fwd = trace_runs(dark, row + dr, col + dc, dr, dc, limit)
    if fwd is None:
        return None
    if not near_module(back[0] + fwd[0], ms) or not near_module(fwd[1], ms):
        return None
    base = F(col if dc != 0 else row)
    center = base + (F(fwd[0]) - F(back[0])) / F(2) + F(1)
    return center, back[0] + fwd[0]


def check_alignment(dark, row, col, ms):
    rows, cols = dark.shape
    limit = _cast(ms * F(1.6) + F(1))
    h = alignment_axis(dark, row, col, 0, 1, ms, limit)
    if h is None:
        return None
    ccol = _cast(h[0])
    if ccol >= cols or not dark[row, ccol]:
        return None
    v = alignment_axis(dark, row, ccol, 1, 0, ms, limit)
    if v is None:
        return None
    local_ms = F(h[1] + v[1]) / F(2)
    for d0, d1 in ((1, 1), (1, -1), (-1, 1), (-1, -1)):
        for scale, want in ((1, False), (2, True)):
            pr = v[0] + F(d0) * F(scale) * local_ms
            pc = h[0] + F(d1) * F(scale) * local_ms
            if not (pc >= 0 and pc < F(cols) and pr >= 0 and pr < F(rows)):
                return None
            if bool(dark[_cast(pr), _cast(pc)]) != want:
                return None
    return h[0], v[0]


def insert_nearest(found, cand, ms):
    """insertNearest (:492-507); entries are (x, y, d2)."""
    for i, e in enumerate(found):
        if abs(e[0] - cand[0]) < ms and abs(e[1] - cand[1]) < ms:
            if cand[2] < e[2]:
                found[i] = cand
            return
    at = len(found)
    while at > 0 and cand[2] < found[at - 1][2]:
        at -= 1
    if at >= 4:
        return
    found.insert(at, cand)
    del found[4:]


def fourth_candidates(dark, triple, dim):
    """[(x, y, is_alignment)]"""
    rows, cols = dark.shape
    tl, tr, bl = triple
    out = []
    if dim >= 25:
        span, steps = F(dim - 7), F(dim - 10)
        inv = F(1) / span
        pm = (((tr[0] - tl[0]) + (bl[0] - tl[0])) * inv, ((tr[1] - tl[1]) + (bl[1] - tl[1])) * inv)
        pred = (tl[0] + pm[0] * steps, tl[1] + pm[1] * steps)
        ms = module_size(triple)
        radius = ms * max(F(5), F(0.2) * steps)
        step = np.trunc(max(F(1), ms / F(2)))
        found = []
        y = pred[1] - radius
        while y <= pred[1] + radius:
            if not y < 0:
                py = _cast(y)
                if py >= rows:
                    break
                x = pred[0] - radius
                while x <= pred[0] + radius:
                    if not x < 0:
                        px = _cast(x)
                        if px >= cols:
                            break
                        if dark[py, px]:
                            c = check_alignment(dark, py, px, ms)
                            if c is not None:
                                dx, dy = c[0] - pred[0], c[1] - pred[1]
                                insert_nearest(found, (c[0], c[1], dx * dx + dy * dy), ms)
                    x = x + step
            y = y + step
        out = [(e[0], e[1], True) for e in found]
    out.append(((tr[0] + bl[0]) - tl[0], (tr[1] + bl[1]) - tl[1], False))
    return out


# ---- ProjectiveTransform(f64).init with four points (transforms.zig:242-268, Point.zig:200-253, SMatrix.zig:729-766) -----------------
def _collinear3(s, b, c):
    swap = b[0] > c[0] or (b[0] == c[0] and b[1] > c[1])
    p1, p2 = (c, b) if swap else (b, c)
    u = s[0] * (p1[1] - p2[1]) + p1[0] * (p2[1] - s[1]) + p2[0] * (s[1] - p1[1])
    return u == 0


def all_collinear(points):
    i = 1
    while i < len(points) and points[i] == points[0]:
        i += 1
    if i == len(points):
        return True
    return all(_collinear3(points[0], points[i], p) for p in points[i + 1:])


def solve(a):
    """SMatrix.solve on the augmented n x (n + 1) system `a` (a list of lists of Python floats, changed in place): x, or None."""
    n = len(a)
    max_entry = 0.0
    for r in range(n):
        for c in range(n):
            max_entry = max(max_entry, abs(a[r][c]))
    if max_entry == 0:
        return None
    tolerance = max_entry * 2.220446049250313e-16 * 100
    for c in range(n):
        pivot = c
        for r in range(c + 1, n):
            if abs(a[r][c]) > abs(a[pivot][c]):
                pivot = r
        if abs(a[pivot][c]) < tolerance:
            return None
        a[c], a[pivot] = a[pivot], a[c]
        for r in range(n):
            if r == c:
                continue
            factor = a[r][c] / a[c][c]
            if factor == 0:
                continue
            for idx in range(c, n + 1):
                a[r][idx] -= factor * a[c][idx]
    return [a[i][n] / a[i][i] for i in range(n)]


def projective4(frm, to):
    """The 3 x 3 matrix as nine floats, row-major, or None."""
    frm = [(float(x), float(y)) for x, y in frm]
    to = [(float(x), float(y)) for x, y in to]
    if all_collinear(frm) or all_collinear(to):
        return None
    a = []
    for (fx, fy), (tx, ty) in zip(frm, to):
        a.append([fx, fy, 1.0, 0.0, 0.0, 0.0, -tx * fx, -tx * fy, tx])
        a.append([0.0, 0.0, 0.0, fx, fy, 1.0, -ty * fx, -ty * fy, ty])
    h = solve(a)
    return None if h is None else h + [1.0]


def build_transform(triple, dim, fourth):
    d = float(dim)
    module = d - 6.5 if fourth[2] else d - 3.5
    frm = [(3.5, 3.5), (d - 3.5, 3.5), (3.5, d - 3.5), (module, module)]
    to = [(triple[0][0], triple[0][1]), (triple[1][0], triple[1][1]), (triple[2][0], triple[2][1]), (fourth[0], fourth[1])]
    return projective4(frm, to)


def project(m, x, y):
    px = (m[0] * x + m[1] * y) + m[2] * 1.0
    py = (m[3] * x + m[4] * y) + m[5] * 1.0
    w = (m[6] * x + m[7] * y) + m[8] * 1.0
    if w != 0:
        s = 1.0 / w
        px, py = px * s, py * s
    return px, py


# ---- sampling (:567-641) -----------------------------------------------------------------------------------------------------------
_OFFSETS = ((0.0, 0.0), (0.25, 0.0), (-0.25, 0.0), (0.0, 0.25), (0.0, -0.25))


def sample_module(dark, m, row, col):
    rows, cols = dark.shape
    votes = 0
    for k, (ox, oy) in enumerate(_OFFSETS):
        if votes >= 3 or votes + (5 - k) < 3:
            break
        px, py = project(m, float(col) + 0.5 + ox, float(row) + 0.5 + oy)
        if not (px >= 0 and px < cols and py >= 0 and py < rows):  # Rectangle.contains: half-open, NaN outside
            if k == 0:
                return None
            continue
        if dark[_cast(py), _cast(px)]:
            votes += 1
    return 1 if votes >= 3 else 0


def sample_timing_lines(dark, m, dim, grid):
    for line in (6, dim - 7):
        for i in range(8, dim - 8):
            for r, c in ((line, i), (i, line)):
                v = sample_module(dark, m, r, c)
                if v is None:
                    return False
                grid[r, c] = v
    return True


def timing_ok(grid, dim):
    row_best = col_best = 0
    for line in (6, dim - 7):
        row_match = col_match = 0
        for i in range(8, dim - 8):
            expected = 1 if i % 2 == 0 else 0
            row_match += grid[line, i] == expected
            col_match += grid[i, line] == expected
        row_best, col_best = max(row_best, row_match), max(col_best, col_match)
    needed = (dim - 16) * 3 // 4
    return row_best >= needed and col_best >= needed


def sample_grid(dark, m, dim, grid):
    for r in range(dim):
        for c in range(dim):
            v = sample_module(dark, m, r, c)
            if v is None:
                return False
            grid[r, c] = v
    return True


def symbol_corners(m, dim):
    d = float(dim)
    out = []
    for x, y in ((0.0, 0.0), (d, 0.0), (0.0, d), (d, d)):
        px, py = project(m, x, y)
        out += [F(px), F(py)]
    return np.array(out, F)


# ---- decoder.readVersion (decoder.zig:118-162), tables.bchRemainder (tables.zig:226-261) -------------------------------------------
def bch_remainder(data, generator, total_bits, data_bits):
    gen_degree = total_bits - data_bits
    rem = data << gen_degree
    bit = total_bits
    while bit > gen_degree:
        bit -= 1
        if rem >> bit & 1:
            rem ^= generator << (bit - gen_degree)
    return rem


def version_codeword(version):
    return version << 12 | bch_remainder(version, 0x1f25, 18, 6)


def oriented_module(grid, dim, orientation, row, col):
    r, c = (col, row) if orientation & 4 else (row, col)
    o = orientation & 3
    if o == 0:
        return grid[r, c]
    if o == 1:
        return grid[dim - 1 - c, r]
    if o == 2:
        return grid[dim - 1 - r, dim - 1 - c]
    return grid[c, dim - 1 - r]


def oriented(grid, orientation):
    dim = grid.shape[0]
    return np.array([[oriented_module(grid, dim, orientation, r, c) for c in range(dim)] for r in range(dim)], np.uint8)


def read_version(grid, dim):
    best_distance, best_index = 4, None
    for orientation in range(8):
        codeword = 0
        for i in range(6):
            for j in range(3):
                codeword |= int(oriented_module(grid, dim, orientation, dim - 11 + j, i)) << (3 * i + j)
        for index in range(34):
            distance = bin(codeword ^ version_codeword(index + 7)).count("1")
            if distance < best_distance:
                best_distance, best_index = distance, index
    return None if best_index is None else best_index + 7


# ---- detectAndDecode (:86-156) -----------------------------------------------------------------------------------------------------
def _append(candidates, version):
    if version not in candidates and len(candidates) < MAX_VERSIONS:
        candidates.append(version)


def detect(binary):
    """Every intermediate result of detectAndDecode on a binary map (rows x cols uint8). `consumed` tells whether the residue-1 and
    residue-2 row passes were merged."""
    binary = np.asarray(binary, np.uint8)
    rows, cols = binary.shape
    res = dict(finders=[], merged_count=0, finder_count=0, triple=None, estimate=0, versions=[], fourths=[], grids=[], consumed=False)
    if rows < 21 or cols < 21:  # :58
        return res
    dark = binary == 0
    buf = []
    step = 3 if rows > 300 else 1
    for row in range(0, rows, step):
        for p in row_hits(dark, row):
            add_candidate(buf, p)
    if len(buf) < 3 and step > 1:
        res["consumed"] = True
        for start in (1, 2):
            for row in range(start, rows, step):
                for p in row_hits(dark, row):
                    add_candidate(buf, p)
    res["merged_count"] = res["finder_count"] = len(buf)
    res["finders"] = buf
    if len(buf) < 3:
        return res
    confirmed = 0
    for f in list(buf):  # in place, as the reference compacts (:102-109): the tail of the buffer keeps what it held
        if f[3] >= 2:
            buf[confirmed] = list(f)
            confirmed += 1
    finders = buf[:confirmed] if confirmed >= 3 else buf
    res["finder_count"] = len(finders)
    triple = pick_finder_triple(finders)
    if triple is None:
        return res
    res["triple"] = [list(t) for t in triple]
    candidates = []
    estimate = estimate_version(triple)
    res["estimate"] = estimate
    _append(candidates, estimate)
    if estimate > 1:
        _append(candidates, estimate - 1)
    if estimate < 40:
        _append(candidates, estimate + 1)
    fourths = fourth_candidates(dark, triple, 17 + 4 * min(estimate + 1, 40))
    res["fourths"] = fourths
    res["versions"] = candidates
    i = 0
    while i < len(candidates):
        version = candidates[i]
        dim = 17 + 4 * version
        grid = np.zeros((dim, dim), np.uint8)
        for fi, fourth in enumerate(fourths):
            if fourth[2] and version < 2:
                continue
            m = build_transform(triple, dim, fourth)
            if m is None:
                continue
            if not sample_timing_lines(dark, m, dim, grid):
                continue
            if not timing_ok(grid, dim):
                continue
            if not sample_grid(dark, m, dim, grid):
                continue
            hint = None
            if version >= 7:
                hint = read_version(grid, dim)
                if hint is not None:
                    _append(candidates, hint)
            res["grids"].append(dict(version=version, dim=dim, fourth_index=fi, version_hint=-1 if hint is None else hint,
                                     corners=symbol_corners(m, dim), transform=np.array(m, np.float64), modules=grid.copy()))
        i += 1
    return res


def pack(res, grid_capacity=1 << 30, module_capacity=1 << 30):
    """(detection record, grid records, module bytes) as the device writes them under the two capacities: only whole grids, stopping at
    the first that does not fit either."""
    det = np.zeros((), DETECTION_DTYPE)
    for i, f in enumerate(res["finders"]):
        det["finders"][i] = f
    det["finder_count"], det["merged_count"] = res["finder_count"], res["merged_count"]
    if res["triple"] is not None:
        det["triple_found"] = 1
        det["triple"][:] = np.array(res["triple"], F)
        det["version_estimate"] = res["estimate"]
        det["version_count"] = len(res["versions"])
        det["versions"][:len(res["versions"])] = res["versions"]
        det["fourth_count"] = len(res["fourths"])
        for i, (x, y, al) in enumerate(res["fourths"]):
            det["fourths"][i] = (x, y, 1 if al else 0)
    det["grids_total"] = len(res["grids"])
    grids, modules, offset = [], [], 0
    for g in res["grids"]:
        n = g["dim"] * g["dim"]
        if len(grids) >= grid_capacity or offset + n > module_capacity:
            break
        rec = np.zeros((), GRID_DTYPE)
        rec["version"], rec["dim"], rec["fourth_index"], rec["modules_offset"], rec["version_hint"] = g["version"], g["dim"], g["fourth_index"], offset, g["version_hint"]
        rec["corners"], rec["transform"] = g["corners"], g["transform"]
        grids.append(rec)
        modules.append(g["modules"].reshape(-1))
        offset += n
    det["grids_written"], det["modules_written"] = len(grids), offset
    grids = np.array(grids, GRID_DTYPE) if grids else np.zeros(0, GRID_DTYPE)
    modules = np.concatenate(modules) if modules else np.zeros(0, np.uint8)
    return det, grids, modules


# ---- the fixtures of tests/test_qr_geom_host.py (tests/golden/qr_geom.json, qr_geom_records.bin, qr_geom_ratio.bin) -----------------
def _h64(v):
    return "%016x" % int(np.float64(v).view(np.uint64))


def _h32(v):
    return "%08x" % int(F(v).view(np.uint32))


def ratio_bits():
    """checkRatio on every window with runs in 0 .. 12, at the three tolerances: a bit per window (run 0 the slowest index), packed."""
    r = np.arange(13)
    w = np.stack(np.meshgrid(r, r, r, r, r, indexing="ij")).reshape(5, -1)
    total = w.sum(axis=0)
    unit = total.astype(F) / F(7)
    out = []
    for tol in (SCAN_TOL, CROSS_TOL, DIAG_TOL):
        ok = (w > 0).all(axis=0) & (total >= 7)
        for i, expected in enumerate((1, 1, 3, 1, 1)):
            eu = F(expected) * unit
            ok &= ~(np.abs(w[i].astype(F) - eu) > eu * tol)
        out.append(np.packbits(ok, bitorder="little"))
    return np.concatenate(out)


def geom_records(seed=20):
    """Lines for tests/c/qr_geom.cpp, each a kind letter and hexadecimal words: see that file."""
    rng = np.random.default_rng(seed)
    lines = []

    def quad(frm, to):
        m = projective4(frm, to)
        words = [_h64(v) for p in frm for v in p] + [_h64(v) for p in to for v in p]
        words.append("1" if m is not None else "0")
        mm = m if m is not None else [0.0] * 9
        words += [_h64(v) for v in mm]
        for x, y in ((0.0, 0.0), (float(rng.integers(0, 60)) + 0.75, float(rng.integers(0, 60)) + 0.5)):
            px, py = project(mm, x, y) if m is not None else (0.0, 0.0)
            words += [_h64(x), _h64(y), _h64(px), _h64(py)]
        lines.append("Q " + " ".join(words))
        return m

    solved = 0
    for _ in range(200):
        dim = 17 + 4 * int(rng.integers(1, 41))
        d = float(dim)
        module = d - 6.5 if rng.integers(0, 2) else d - 3.5
        frm = [(3.5, 3.5), (d - 3.5, 3.5), (3.5, d - 3.5), (module, module)]
        base = rng.uniform(20, 400, 2)
        ax, ay = rng.uniform(-1, 1, 2), rng.uniform(-1, 1, 2)
        scale = rng.uniform(2, 9)
        to = []
        for fx, fy in frm:
            w = 1 + rng.uniform(-0.002, 0.002) * fx + rng.uniform(-0.002, 0.002) * fy
            to.append((float(F(base[0] + scale * (ax[0] * fx + ay[0] * fy) / w)), float(F(base[1] + scale * (ax[1] * fx + ay[1] * fy) / w))))
        solved += quad(frm, to) is not None
    assert solved > 170
    square = [(3.5, 3.5), (17.5, 3.5), (3.5, 17.5), (14.5, 14.5)]
    assert quad(square, [(1.0, 1.0), (2.0, 2.0), (3.0, 3.0), (5.0, 5.0)]) is None and all_collinear([(1.0, 1.0), (2.0, 2.0), (3.0, 3.0), (5.0, 5.0)])
    assert quad([(0.0, 0.0), (1.0, 0.0), (2.0, 0.0), (3.0, 0.0)], square) is None
    degenerate = [(0.0, 0.0), (1.0, 0.0), (2.0, 0.0), (0.0, 1.0)]  # three on a line: not collinear as a set, but the system has a zero pivot
    assert not all_collinear(degenerate) and quad(degenerate, square) is None
    assert quad(square, [(0.0, 0.0)] * 4) is None
    # triple scores on a lattice: equal sides and right angles, so equal scores
    lattice = [[F(20 + 30 * int(rng.integers(0, 6))), F(20 + 30 * int(rng.integers(0, 6))), F(3), F(2)] for _ in range(12)]
    loose = [[F(rng.uniform(0, 300)), F(rng.uniform(0, 300)), F(rng.uniform(2.5, 4.5)), F(1)] for _ in range(12)]
    scores = []
    for fs in (lattice, loose):
        for i in range(len(fs)):
            for j in range(i + 1, len(fs)):
                for k in range(j + 1, len(fs)):
                    a, b, c = fs[i], fs[j], fs[k]
                    r = triple_score(a, b, c)
                    words = [_h32(v) for f in (a, b, c) for v in f]
                    if r is None:
                        lines.append("S " + " ".join(words + ["0", _h32(0), "0", "0", "0"]))
                    else:
                        order = [[id(x) for x in (a, b, c)].index(id(t)) for t in r[1]]
                        scores.append(_h32(r[0]))
                        lines.append("S " + " ".join(words + ["1", _h32(r[0])] + [str(o) for o in order]))
                        lines.append("V " + " ".join([_h32(v) for t in r[1] for v in t] + [str(estimate_version(r[1]))]))
    assert len(scores) > len(set(scores)) > 10  # ties, and more than a few values
    for v in range(7, 41):
        lines.append("B %x %x" % (v, version_codeword(v)))
    for length in range(0, 20):
        for expected in (F(1), F(2.5), F(3.3333333), F(7.1)):
            lines.append("N %x %s %d" % (length, _h32(expected), near_module(length, expected)))
    for base, fwd, total in ((0, 3, 7), (10, 11, 21), (1000, 37, 70), (5, 10, 23)):
        lines.append("C %x %x %x %s" % (base, fwd, total, _h32(cross_center(base, fwd, total))))
    for version in (1, 2, 7, 12, 40):
        dim = 17 + 4 * version
        for trial in range(6 if version < 40 else 2):
            grid = rng.integers(0, 2, (dim, dim)).astype(np.uint8)
            if trial % 2 == 0:
                for i in range(8, dim - 8):
                    grid[6, i] = grid[i, 6] = 1 if i % 2 == 0 else 0
            if version >= 7 and trial < 4:
                word = version_codeword(version) ^ (0b101 << trial if trial else 0)  # up to two bit errors
                for i in range(6):
                    for j in range(3):
                        grid[dim - 11 + j, i] = word >> (3 * i + j) & 1
                grid = oriented(grid, trial)
            hint = read_version(grid, dim) if version >= 7 else None
            lines.append("G %x %s %d %d" % (dim, "".join(str(int(v)) for v in grid.reshape(-1)), timing_ok(grid, dim), -1 if hint is None else hint))
    return lines
