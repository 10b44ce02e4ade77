"""Tracer (reference src/features/Tracer.zig) restated line by line in numpy float32: trace (:46-80), neighbors (:88-105), followPath
(:109-173), simplifyPath (:176-201), douglasPeucker (:204-236), and Point.normalize / dot / distanceToSegment
(src/geometry/Point.zig:117-138, :177-195). The reference records no expected output for Tracer, so the device (tests/test_gpu_tracer.py)
and the shared header (tests/test_tracer_step_host.py) are held to this file, and tests/test_tracer_oracle.py holds this file to what
follows from the reference's code. Every f32 operation is one numpy float32 operation, in the reference's order.

`python -m tests.tracer_ref` rewrites the fixtures under tests/golden/ (tracer_step.json, tracer_step_dist.bin, tracer_cpp_paths.bin)."""
from __future__ import annotations

import json
import os
from collections import deque

import numpy as np

f32 = np.float32
OFFSETS = ((-1, -1), (-1, 0), (-1, 1), (0, -1), (0, 1), (1, -1), (1, 0), (1, 1))  # (row, col), :90-94


def _neighbor_dir(k):  # :96-101
    dx, dy = f32(OFFSETS[k][1]), f32(OFFSETS[k][0])
    ln = np.sqrt(dx * dx + dy * dy)
    return dx / ln, dy / ln


DIRS = tuple(_neighbor_dir(k) for k in range(8))


def prev_dir(prev_k):
    """p_curr.sub(p_prev).normalize() (:128-130) when the last step was neighbour prev_k: a point is (x = col, y = row)."""
    x, y = f32(OFFSETS[prev_k][1]), f32(OFFSETS[prev_k][0])
    n = np.sqrt(x * x + y * y)  # norm = @sqrt(dot(self, self))
    if n == 0:
        return x, y
    s = f32(1.0) / n
    return x * s, y * s


def score(prev_k, k):
    ux, uy = prev_dir(prev_k)
    vx, vy = DIRS[k]
    return ux * vx + uy * vy  # @reduce(.Add, a * b)


SCORE = [[score(pk, k) for k in range(8)] for pk in range(8)]


def choose(prev_k, mask):
    """The neighbour the loop at :134-161 ends with, -1 for none. prev_k -1: no history."""
    best, best_score = -1, f32(-2.0)
    for k in range(8):
        if not (mask >> k) & 1:
            continue
        if prev_k < 0:
            return k
        s = SCORE[prev_k][k]
        if s > best_score:
            best_score, best = s, k
    return best


CHOICE = [[choose(pk, m) for m in range(256)] for pk in range(-1, 8)]  # [prev_k + 1][mask]


def follow_path(op: bytearray, rows: int, cols: int, r: int, c: int, events=None):
    """followPath. op[r * cols + c] is 1 iff the pixel is an edge and not visited; visiting clears it. Returns the pixel indices.
    events: a set that receives every (prev_k, mask) pair a decision was made on."""
    path = [r * cols + c]
    op[r * cols + c] = 0
    prev_k = -1
    while True:
        mask = 0
        for k, (dr, dc) in enumerate(OFFSETS):
            rr, cc = r + dr, c + dc
            if 0 <= rr < rows and 0 <= cc < cols and op[rr * cols + cc]:
                mask |= 1 << k
        if events is not None:
            events.add((prev_k, mask))
        k = CHOICE[prev_k + 1][mask]
        if k < 0:
            return path
        r, c = r + OFFSETS[k][0], c + OFFSETS[k][1]
        path.append(r * cols + c)
        op[r * cols + c] = 0
        prev_k = k


def trace_raw(edges: np.ndarray, events=None):
    """Every raw path of trace's scan (:58-77), dropped ones included, as lists of pixel indices in the order they start."""
    edges = np.asarray(edges)
    rows, cols = edges.shape
    op = bytearray((edges > 0).astype(np.uint8).tobytes())
    paths, p = [], op.find(1)
    while p >= 0:
        paths.append(follow_path(op, rows, cols, p // cols, p % cols, events))
        p = op.find(1, p + 1)
    return paths


def points_of(path, cols: int) -> np.ndarray:
    idx = np.asarray(path, np.int64)
    return np.stack([(idx % cols).astype(np.float32), (idx // cols).astype(np.float32)], axis=1)


def distance_to_segment(p, a, b):
    """Point.distanceToSegment for p of shape (..., 2) and two points a, b; returns (distance, which of the four returns)."""
    p = np.asarray(p, np.float32).reshape(-1, 2)
    a, b = np.asarray(a, np.float32), np.asarray(b, np.float32)
    abx, aby = b[0] - a[0], b[1] - a[1]
    apx, apy = p[:, 0] - a[0], p[:, 1] - a[1]
    ab_len_sq = abx * abx + aby * aby
    ap_norm = np.sqrt(apx * apx + apy * apy)
    if ab_len_sq == 0:
        return ap_norm, np.zeros(len(p), np.int32)
    t = (apx * abx + apy * aby) / ab_len_sq
    bx, by = p[:, 0] - b[0], p[:, 1] - b[1]
    pb_norm = np.sqrt(bx * bx + by * by)
    ex, ey = apx - abx * t, apy - aby * t
    perp = np.sqrt(ex * ex + ey * ey)
    which = np.where(t <= 0, 1, np.where(t >= 1, 2, 3)).astype(np.int32)
    return np.where(which == 1, ap_norm, np.where(which == 2, pb_norm, perp)).astype(np.float32), which


def _split(points, start, end, eps):
    """One range of douglasPeucker (:212-234): the index to keep, or -1."""
    if end <= start + 1:
        return -1
    d, _ = distance_to_segment(points[start + 1:end], points[start], points[end])
    i = int(np.argmax(d))  # the first of the largest: d > max_dist is strict
    if not d[i] > 0:  # max_dist starts at 0
        return -1
    return start + 1 + i if d[i] > f32(eps) else -1


def douglas_peucker_stack(points, eps):
    keep = np.zeros(len(points), bool)
    keep[0] = keep[-1] = True
    stack = [(0, len(points) - 1)]
    while stack:
        start, end = stack.pop()
        i = _split(points, start, end, eps)
        if i >= 0:
            keep[i] = True
            stack.append((start, i))
            stack.append((i, end))
    return keep


def douglas_peucker_levels(points, eps):
    keep = np.zeros(len(points), bool)
    keep[0] = keep[-1] = True
    level = [(0, len(points) - 1)]
    while level:
        nxt = []
        for start, end in level:
            i = _split(points, start, end, eps)
            if i >= 0:
                keep[i] = True
                nxt += [(start, i), (i, end)]
        level = nxt
    return keep


def simplify_path(points: np.ndarray, eps) -> np.ndarray:
    if len(points) < 3:
        return points.copy()
    return points[douglas_peucker_stack(points, eps)]


def finish(raw_paths, cols, min_path_length=5, simplification_epsilon=1.0):
    """trace's lines 64-74 over the raw paths."""
    out = []
    for path in raw_paths:
        if len(path) >= min_path_length:
            pts = points_of(path, cols)
            out.append(simplify_path(pts, simplification_epsilon) if f32(simplification_epsilon) > 0 else pts)
    return out


def trace(edges, min_path_length=5, simplification_epsilon=1.0):
    edges = np.asarray(edges)
    return finish(trace_raw(edges), edges.shape[1], min_path_length, simplification_epsilon)


def components(edges):
    """The 8-connected components of edges > 0, as boolean masks."""
    edges = np.asarray(edges) > 0
    rows, cols = edges.shape
    seen = np.zeros_like(edges)
    out = []
    for r0, c0 in zip(*np.nonzero(edges)):
        if seen[r0, c0]:
            continue
        mask = np.zeros_like(edges)
        seen[r0, c0] = mask[r0, c0] = True
        todo = deque([(int(r0), int(c0))])
        while todo:
            r, c = todo.popleft()
            for dr, dc in OFFSETS:
                rr, cc = r + dr, c + dc
                if 0 <= rr < rows and 0 <= cc < cols and edges[rr, cc] and not seen[rr, cc]:
                    seen[rr, cc] = mask[rr, cc] = True
                    todo.append((rr, cc))
        out.append(mask)
    return out


def trace_raw_by_components(edges):
    paths = []
    for mask in components(edges):
        paths += trace_raw(mask)
    return sorted(paths, key=lambda p: p[0])


def pack(paths):
    """(counts[0..1], path_offsets, points) as the device writes them with room for everything."""
    offsets = np.zeros(len(paths) + 1, np.uint32)
    offsets[1:] = np.cumsum([len(p) for p in paths])
    points = np.concatenate(paths).astype(np.float32) if paths else np.zeros((0, 2), np.float32)
    return np.array([len(paths), len(points)], np.uint32), offsets, points.reshape(-1, 2)


# ---- fixtures ---------------------------------------------------------------------------------------------------------------

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def dist_cases():
    """Integer triples (p, a, b) that reach all four returns: small coordinates (ties, zero segments, projections on both sides) and
    frame-sized ones."""
    rng = np.random.default_rng(20)
    small = rng.integers(-3, 9, size=(2500, 6))
    big = rng.integers(0, 4096, size=(1200, 6))
    zero = rng.integers(0, 300, size=(200, 6))
    zero[:, 4:6] = zero[:, 2:4]  # a == b
    line = rng.integers(0, 60, size=(196, 6))
    line[:, 1] = line[:, 3] = line[:, 5] = 7  # collinear: distance 0 inside, the end distances outside
    return np.concatenate([small, big, zero, line]).astype(np.int32)


def cpp_frame():
    """The 48 x 64 map tests/cpp/test_tracer.cpp traces: a ring, a T junction, a diagonal, a short speck (dropped) and a zigzag."""
    e = np.zeros((48, 64), np.uint8)
    yy, xx = np.mgrid[0:48, 0:64]
    d = np.hypot(yy - 16, xx - 16)
    e[(d > 9.5) & (d < 10.5)] = 255
    e[30, 5:40] = 255
    e[30:46, 22] = 255
    for i in range(20):
        e[3 + i, 40 + i] = 255
    e[44, 60:63] = 255
    for i in range(24):
        e[36 + (i % 6 if (i // 6) % 2 == 0 else 5 - i % 6), 36 + i] = 255
    return e


def write_fixtures():
    step = {"offsets": [list(o) for o in OFFSETS],
            "score_bits": [["%08x" % int(np.float32(s).view(np.uint32)) for s in row] for row in SCORE],
            "choice": CHOICE}
    with open(os.path.join(GOLDEN, "tracer_step.json"), "w") as f:
        json.dump(step, f, separators=(",", ":"))
        f.write("\n")
    cases = dist_cases()
    rec = np.zeros((len(cases), 8), np.uint32)
    rec[:, :6] = cases.view(np.uint32)
    for i, c in enumerate(cases):
        d, which = distance_to_segment(c[0:2], c[2:4], c[4:6])
        rec[i, 6], rec[i, 7] = d.view(np.uint32)[0], which[0]
    rec.astype("<u4").tofile(os.path.join(GOLDEN, "tracer_step_dist.bin"))
    e = cpp_frame()
    counts, offsets, points = pack(trace(e))
    with open(os.path.join(GOLDEN, "tracer_cpp_paths.bin"), "wb") as f:  # rows cols | map | counts[2] | offsets | points
        f.write(np.array(e.shape, "<u4").tobytes() + e.tobytes() + counts.astype("<u4").tobytes() + offsets.astype("<u4").tobytes()
                + points.astype("<f4").tobytes())


if __name__ == "__main__":
    write_fixtures()
