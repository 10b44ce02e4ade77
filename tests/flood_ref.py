"""Image(T).floodFill restated twice, in this project's own words, for the tests of zg_flood_fill.

flood_fill_literal   the reference's loop as it stands: a stack, `visited` set before the push, fill_value written at the pop, the
                     neighbour offsets in its order, pixelDistance in f64 with a real square root.
flood_fill_fast      the filled set as a graph problem: numpy predicates give one plane of links per direction, a breadth-first search
                     from the seed over those links (scipy.sparse.csgraph) gives the component.

Images are numpy arrays, (rows, cols) or (rows, cols, channels), uint8 or float32; fill_value a scalar or a sequence of channels.
Both return (filled image, number of filled pixels) and leave their input alone."""
import math

import numpy as np
from scipy.sparse import coo_matrix
from scipy.sparse.csgraph import breadth_first_order

# (d_row, d_col) in the reference's order: the first four are 4-connectivity
OFFSETS = ((-1, 0), (1, 0), (0, -1), (0, 1), (-1, -1), (-1, 1), (1, -1), (1, 1))


class OutOfBounds(Exception):
    """error.OutOfBounds: the seed is outside the image."""


def _check(img, connectivity, mode):
    assert connectivity in (4, 8) and mode in ("seed", "neighbor")
    assert img.dtype in (np.uint8, np.float32) and img.ndim in (2, 3)


def pixel_distance(a, b):
    """pixelDistance of two pixels given as tuples of Python floats (f64): |a - b| for one channel, otherwise the square root of the
    sum of squares accumulated from 0.0 in field order."""
    if len(a) == 1:
        return abs(a[0] - b[0])
    sum_sq = 0.0
    for x, y in zip(a, b):
        diff = x - y
        sum_sq += diff * diff
    return math.sqrt(sum_sq)


def flood_fill_literal(img, row, col, fill_value, threshold=0.0, connectivity=4, mode="seed"):
    _check(img, connectivity, mode)
    rows, cols = img.shape[:2]
    if row >= rows or col >= cols:
        raise OutOfBounds((row, col))
    threshold = float(threshold)
    # every pixel as a tuple of f64: the loop only ever compares original values, so the copy read here is never written
    orig = [[tuple(px) for px in line] for line in img.astype(np.float64).reshape(rows, cols, -1).tolist()]
    out = img.copy()
    seed_val = orig[row][col]
    visited = [False] * (rows * cols)
    stack = [(row, col)]
    visited[row * cols + col] = True
    filled = 0
    while stack:
        r, c = stack.pop()
        out[r, c] = fill_value
        filled += 1
        compare = seed_val if mode == "seed" else orig[r][c]
        for dr, dc in OFFSETS[:connectivity]:
            nr, nc = r + dr, c + dc
            if nr < 0 or nr >= rows or nc < 0 or nc >= cols:
                continue
            idx = nr * cols + nc
            if not visited[idx]:
                if pixel_distance(orig[nr][nc], compare) <= threshold:  # False for a NaN on either side
                    visited[idx] = True
                    stack.append((nr, nc))
    return out, filled


def _distance_planes(a, b):
    """pixelDistance of two equally shaped (rows, cols, channels) f64 arrays, pixel by pixel."""
    with np.errstate(all="ignore"):
        if a.shape[2] == 1:
            return np.abs(a[..., 0] - b[..., 0])
        sum_sq = np.zeros(a.shape[:2], np.float64)
        for k in range(a.shape[2]):
            diff = a[..., k] - b[..., k]
            sum_sq = sum_sq + diff * diff
        return np.sqrt(sum_sq)


def pass_mask(img, row, col, threshold):
    """seed mode: the pixels within the threshold of the seed's value, the seed itself always."""
    rows, cols = img.shape[:2]
    px = img.astype(np.float64).reshape(rows, cols, -1)
    with np.errstate(all="ignore"):
        ok = _distance_planes(px, np.broadcast_to(px[row, col], px.shape)) <= float(threshold)
    ok[row, col] = True
    return ok


def link_planes(img, row, col, threshold, connectivity, mode):
    """{(d_row, d_col): bool plane} for the directions E, S, SE, SW: plane[r, c] says that (r, c) and (r + d_row, c + d_col) are linked.
    Each plane has the shape of the pixels that have that neighbour."""
    rows, cols = img.shape[:2]
    px = img.astype(np.float64).reshape(rows, cols, -1)
    dirs = ((0, 1), (1, 0)) + (((1, 1), (1, -1)) if connectivity == 8 else ())
    ok = pass_mask(img, row, col, threshold) if mode == "seed" else None
    planes = {}
    for dr, dc in dirs:
        if dc >= 0:
            here, there = (slice(0, rows - dr), slice(0, cols - dc)), (slice(dr, rows), slice(dc, cols))
        else:
            here, there = (slice(0, rows - dr), slice(1, cols)), (slice(dr, rows), slice(0, cols - 1))
        if mode == "seed":
            planes[(dr, dc)] = ok[here] & ok[there]
        else:
            with np.errstate(all="ignore"):
                planes[(dr, dc)] = _distance_planes(px[here], px[there]) <= float(threshold)
    return planes


def filled_mask(img, row, col, threshold=0.0, connectivity=4, mode="seed"):
    _check(img, connectivity, mode)
    rows, cols = img.shape[:2]
    if row >= rows or col >= cols:
        raise OutOfBounds((row, col))
    index = np.arange(rows * cols, dtype=np.int64).reshape(rows, cols)
    src, dst = [], []
    for (dr, dc), plane in link_planes(img, row, col, threshold, connectivity, mode).items():
        if dc >= 0:
            a, b = index[0:rows - dr, 0:cols - dc], index[dr:rows, dc:cols]
        else:
            a, b = index[0:rows - dr, 1:cols], index[dr:rows, 0:cols - 1]
        src.append(a[plane])
        dst.append(b[plane])
    src, dst = np.concatenate(src), np.concatenate(dst)
    graph = coo_matrix((np.ones(len(src), np.int8), (src, dst)), shape=(rows * cols, rows * cols)).tocsr()
    reached = breadth_first_order(graph, row * cols + col, directed=False, return_predecessors=False)
    mask = np.zeros(rows * cols, bool)
    mask[reached] = True
    return mask.reshape(rows, cols)


def flood_fill_fast(img, row, col, fill_value, threshold=0.0, connectivity=4, mode="seed"):
    mask = filled_mask(img, row, col, threshold, connectivity, mode)
    out = img.copy()
    out[mask] = fill_value
    return out, int(mask.sum())
