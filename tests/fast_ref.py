"""Two independent CPU restatements of Fast.detect (reference src/features/Fast.zig:38-254), the checker of zg.Fast.

detect_literal walks the reference's loops one by one (slow: images up to about 96 x 96); detect_fast is vectorised numpy and
handles a 4096^2 frame in seconds. Both return KEYPOINT_DTYPE arrays (KeyPoint.zig:9-28) in the reference's order.
"""
import numpy as np

from zignal_amd import KEYPOINT_DTYPE

# (dx, dy), clockwise from 12 o'clock (Fast.zig:30-35)
CIRCLE = ((0, -3), (1, -3), (2, -2), (3, -1), (3, 0), (3, 1), (2, 2), (1, 3),
          (0, 3), (-1, 3), (-2, 2), (-3, 1), (-3, 0), (-3, -1), (-2, -2), (-1, -3))
GRID = 20  # suppressNonMaximal's grid_size (:172)


def _keypoints(rows, cols, scores) -> np.ndarray:
    out = np.zeros(len(rows), KEYPOINT_DTYPE)
    out["x"] = np.asarray(cols, np.float32)
    out["y"] = np.asarray(rows, np.float32)
    out["size"] = 7.0
    out["angle"] = -1.0
    out["response"] = np.asarray(scores, np.float32)
    out["octave"] = 0
    out["class_id"] = -1
    return out


def _check(img, threshold, min_contiguous):
    img = np.asarray(img)
    assert img.dtype == np.uint8 and img.ndim == 2, "Fast.detect takes Image(u8)"
    assert img.shape[0] > 7 and img.shape[1] > 7  # :39
    assert 0 <= threshold <= 255 and 0 <= min_contiguous <= 255  # u8 fields (:16-24)
    return img


# ---- loop for loop ----------------------------------------------------------------------------------------------------
def _is_corner_literal(img, r, c, t, mc):
    center = int(img[r, c])
    bright, dark = min(center + t, 255), max(center - t, 0)  # +| and -| on u8 (:76-79)
    nb = nd = 0
    for i in (0, 4, 8, 12):  # quick rejection (:81-102)
        dx, dy = CIRCLE[i]
        p = int(img[r + dy, c + dx])
        if p > bright:
            nb += 1
        elif p < dark:
            nd += 1
    if nb < 3 and nd < 3:
        return False
    run_b = run_d = best_b = best_d = 0
    for k in range(32):  # twice round the circle (:104-132)
        dx, dy = CIRCLE[k % 16]
        p = int(img[r + dy, c + dx])
        if p > bright:
            run_b, run_d = run_b + 1, 0
            best_b = max(best_b, run_b)
        elif p < dark:
            run_d, run_b = run_d + 1, 0
            best_d = max(best_d, run_d)
        else:
            run_b = run_d = 0
    return best_b >= mc or best_d >= mc


def _score_literal(img, r, c, t):
    center = int(img[r, c])
    s = 0
    for dx, dy in CIRCLE:  # :135-152
        d = abs(int(img[r + dy, c + dx]) - center)
        if d > t:
            s += d
    return s


def detect_literal(img, threshold=20, min_contiguous=9, nonmax_suppression=True) -> np.ndarray:
    img = _check(img, threshold, min_contiguous)
    rows, cols = img.shape
    kps = []  # (row, col, score) in raster order (:45-65)
    for r in range(3, rows - 3):
        for c in range(3, cols - 3):
            if _is_corner_literal(img, r, c, threshold, min_contiguous):
                kps.append((r, c, _score_literal(img, r, c, threshold)))
    if not nonmax_suppression or not kps:
        return _keypoints([k[0] for k in kps], [k[1] for k in kps], [k[2] for k in kps])
    # suppressNonMaximal (:155-254)
    min_r = min(k[0] for k in kps)
    min_c = min(k[1] for k in kps)
    grid_rows = (max(k[0] for k in kps) - min_r) // GRID + 1
    grid_cols = (max(k[1] for k in kps) - min_c) // GRID + 1
    grid = [[] for _ in range(grid_rows * grid_cols)]
    for k in kps:
        grid[(k[0] - min_r) // GRID * grid_cols + (k[1] - min_c) // GRID].append(k)
    kept = []
    for gr in range(grid_rows):
        for gc in range(grid_cols):
            cell = grid[gr * grid_cols + gc]
            cell.sort(key=lambda k: -k[2])  # stable, descending response (KeyPoint.compareResponse)
            for k in cell:
                is_max = True
                for rr in range(max(gr - 1, 0), min(gr + 2, grid_rows)):
                    for cc in range(max(gc - 1, 0), min(gc + 2, grid_cols)):
                        for o in grid[rr * grid_cols + cc]:
                            if o[0] == k[0] and o[1] == k[1]:
                                continue
                            if (o[0] - k[0]) ** 2 + (o[1] - k[1]) ** 2 < 25 and o[2] > k[2]:
                                is_max = False
                                break
                        if not is_max:
                            break
                    if not is_max:
                        break
                if is_max:
                    kept.append(k)
    return _keypoints([k[0] for k in kept], [k[1] for k in kept], [k[2] for k in kept])


# ---- vectorised -------------------------------------------------------------------------------------------------------
def _longest_runs(mask16: np.ndarray) -> np.ndarray:
    """The reference's arc length per pixel: 32 for a full circle, else the longest circular run of set bits."""
    x = mask16.astype(np.uint32)
    x = x | (x << np.uint32(16))
    run = np.zeros(mask16.shape, np.int32)
    y = x.copy()
    for k in range(1, 16):  # after k - 1 ANDs, bit i of y is set iff bits i .. i + k - 1 of x are
        run = np.where((y & np.uint32(0xFFFF)) != 0, k, run)
        y &= x >> np.uint32(k)
    return np.where(mask16 == 0xFFFF, 32, run)


def score_map(img, threshold=20, min_contiguous=9) -> np.ndarray:
    """int32 (rows - 6) x (cols - 6): the score of every corner among the candidates, 0 elsewhere."""
    img = _check(img, threshold, min_contiguous)
    rows, cols = img.shape
    h, w = rows - 6, cols - 6
    center = img[3:3 + h, 3:3 + w].astype(np.int32)
    bright, dark = np.minimum(center + threshold, 255), np.maximum(center - threshold, 0)
    bm = np.zeros((h, w), np.uint32)
    dm = np.zeros((h, w), np.uint32)
    score = np.zeros((h, w), np.int32)
    for i, (dx, dy) in enumerate(CIRCLE):
        p = img[3 + dy:3 + dy + h, 3 + dx:3 + dx + w].astype(np.int32)
        bm |= (p > bright).astype(np.uint32) << np.uint32(i)
        dm |= (p < dark).astype(np.uint32) << np.uint32(i)
        d = np.abs(p - center)
        score += np.where(d > threshold, d, 0)
    quad = np.uint32(0x1111)

    def popcount4(m):
        m = m & quad
        return ((m & 1) + ((m >> 4) & 1) + ((m >> 8) & 1) + ((m >> 12) & 1)).astype(np.int32)

    quick = (popcount4(bm) >= 3) | (popcount4(dm) >= 3)
    arc = np.maximum(_longest_runs(bm), _longest_runs(dm)) >= min_contiguous
    return np.where(quick & arc, score, 0)


def detect_fast(img, threshold=20, min_contiguous=9, nonmax_suppression=True) -> np.ndarray:
    s = score_map(img, threshold, min_contiguous)
    h, w = s.shape
    if not nonmax_suppression:
        ys, xs = np.nonzero(s)  # raster order
        return _keypoints(ys + 3, xs + 3, s[ys, xs])
    ys, xs = np.nonzero(s)
    if len(ys) == 0:
        return _keypoints([], [], [])
    # kept iff no other corner at dx^2 + dy^2 < 25 scores strictly higher
    pad = np.zeros((h + 8, w + 8), np.int32)
    pad[4:4 + h, 4:4 + w] = s
    most = np.zeros((h, w), np.int32)
    for dy in range(-4, 5):
        for dx in range(-4, 5):
            if (dx or dy) and dx * dx + dy * dy < 25:
                np.maximum(most, pad[4 + dy:4 + dy + h, 4 + dx:4 + dx + w], out=most)
    keep = (s > 0) & (most <= s)
    ky, kx = np.nonzero(keep)
    ksc = s[ky, kx]
    # order: grid cells anchored at the smallest row / col of ALL corners, row-major; by descending score, ties in raster order
    cell = ((ky - ys.min()) // GRID).astype(np.int64) * (w // GRID + 2) + (kx - xs.min()) // GRID
    raster = ky.astype(np.int64) * w + kx
    order = np.lexsort((raster, -ksc, cell))
    return _keypoints(ky[order] + 3, kx[order] + 3, ksc[order])


def photo_like(noise: np.ndarray) -> np.ndarray:
    """The field-plus-noise frame of tests/test_next_rows.py:test_detectors_at_frame_sizes: shapes with hard edges, a little
    sensor noise (`noise` is a synth_u8 plane of the frame's shape)."""
    rows, cols = noise.shape
    yy, xx = np.mgrid[0:rows, 0:cols]
    field = ((np.sin(yy / 37.0) * np.cos(xx / 53.0) + (((xx // 160) + (yy // 120)) % 2)) * 70 + 90).astype(np.float32)
    return (field + noise.astype(np.float32) * 0.08).clip(0, 255).astype(np.uint8)
