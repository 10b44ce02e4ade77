"""The edge maps tests/test_gpu_tracer.py traces, and what each is there for. Everything is deterministic; the restatement's answer for a
frame is computed once (want_raw) and shared."""
import functools

import numpy as np

from tests import tracer_ref as R

ON = 255


def _blank(rows, cols):
    return np.zeros((rows, cols), np.uint8)


# ---- every step decision ----------------------------------------------------------------------------------------------------------
CELL, CELLS_PER_ROW = 8, 46  # 7 x 7 pixels of pattern and a blank row and column; 46 x 46 cells make the 368 x 368 frame


def _ring_route(to):
    """Pixels of the cell's outer ring from (0, 0) to `to`, along column 0 and row 6 for targets on them, else along row 0 and column 6."""
    r, c = to
    if c == 0 or r == 6:
        return [(i, 0) for i in range(0, (r if c == 0 else 6) + 1)] + ([(6, j) for j in range(1, c + 1)] if c else [])
    return [(0, j) for j in range(0, (c if r == 0 else 6) + 1)] + ([(i, 6) for i in range(1, r + 1)] if r else [])


def step_cell(prev_k, mask):
    """A 7 x 7 pattern on which the walk reaches the centre X = (3, 3) by a step in direction prev_k with exactly `mask` open around it:
    the start (0, 0) is the pattern's raster-first pixel, the route follows the outer ring to P3 = X - 3 d, then runs straight through
    P2 and P to X (at every pixel on the way straight on scores highest). mask must not hold the neighbour opposite to prev_k: that is
    P, visited. prev_k -1: X = (0, 1) is the start itself and mask holds E, SW, S, SE only (anything else would have started the path)."""
    cell = np.zeros((7, 7), np.uint8)
    if prev_k < 0:
        x = (0, 1)
    else:
        x = (3, 3)
        dr, dc = R.OFFSETS[prev_k]
        for p in _ring_route((3 - 3 * dr, 3 - 3 * dc)) + [(3 - 2 * dr, 3 - 2 * dc), (3 - dr, 3 - dc)]:
            cell[p] = ON
    cell[x] = ON
    for k, (dr, dc) in enumerate(R.OFFSETS):
        if (mask >> k) & 1:
            cell[x[0] + dr, x[1] + dc] = ON
    return cell


def step_pairs():
    """Every (prev_k, mask) the reference can meet: with history, every mask without the neighbour it came from; without, E SW S SE."""
    pairs = [(-1, m) for m in range(256) if not m & 0b00001111]
    pairs += [(pk, m) for pk in range(8) for m in range(256) if not (m >> (7 - pk)) & 1]  # neighbour 7 - k is the opposite of k
    return pairs


@functools.lru_cache(maxsize=None)
def step_frame():
    pairs = step_pairs()
    assert len(pairs) == 16 + 8 * 128 <= CELLS_PER_ROW ** 2
    frame = _blank(CELL * CELLS_PER_ROW, CELL * CELLS_PER_ROW)
    for i, (pk, m) in enumerate(pairs):
        r0, c0 = CELL * (i // CELLS_PER_ROW), CELL * (i % CELLS_PER_ROW)
        frame[r0:r0 + 7, c0:c0 + 7] = step_cell(pk, m)
    frame.flags.writeable = False
    return frame


# ---- shapes -----------------------------------------------------------------------------------------------------------------------
def diagonal(rows, cols, anti=False, first_col=None):
    """(i, first_col + i), or for anti (i, first_col - i), as far as it stays inside."""
    e = _blank(rows, cols)
    if first_col is None:
        first_col = cols - 1 if anti else 0
    for i in range(rows):
        c = first_col - i if anti else first_col + i
        if 0 <= c < cols:
            e[i, c] = ON
    return e


def ring(rows, cols, cy=64, cx=64, radius=23.0):
    yy, xx = np.mgrid[0:rows, 0:cols]
    d = np.hypot(yy - cy, xx - cx)
    return (((d > radius - 0.5) & (d < radius + 0.5)) * ON).astype(np.uint8)


def spiral(rows, cols, gap=3):
    """A rectangular spiral from the top-left corner inwards with gap - 1 blank pixels between its turns."""
    e = _blank(rows, cols)
    r = c = 0
    dr, dc = 0, 1
    top, left, bottom, right = 0, 0, rows - 1, cols - 1
    e[r, c] = ON
    while True:
        moved = 0
        while {(0, 1): c < right, (1, 0): r < bottom, (0, -1): c > left, (-1, 0): r > top}[(dr, dc)]:  # only the bound ahead
            r, c, moved = r + dr, c + dc, moved + 1
            e[r, c] = ON
        if moved < gap:
            return e
        if (dr, dc) == (0, 1):
            top += gap
        elif (dr, dc) == (1, 0):
            right -= gap
        elif (dr, dc) == (0, -1):
            bottom -= gap
        else:
            left += gap
        dr, dc = dc, -dr


def serpentine(rows, cols):
    """Every second row full, joined at alternating ends: one component, one path, about rows * cols / 2 points."""
    e = _blank(rows, cols)
    e[0::2] = ON
    for i, r in enumerate(range(1, rows - 1, 2)):
        e[r, cols - 1 if i % 2 == 0 else 0] = ON
    return e


def junctions():
    e = _blank(48, 70)
    e[5, 3:30] = ON; e[5:20, 16] = ON                  # T
    e[8:30, 45] = ON; e[19, 34:57] = ON                # X (a cross)
    for i in range(12):                                # Y
        e[24 + i, 10 + i] = ON; e[24 + i, 34 - i] = ON
    e[36:47, 22] = ON
    e[40:42, 30:66] = ON                               # a line two pixels thick
    for i in range(20):
        e[2 + i, 60 - i // 2] = ON; e[2 + i, 61 - i // 2] = ON  # and a slanted one
    return e


def noise(density, seed, shape=(200, 300)):
    return ((np.random.default_rng(1000 * seed + int(density * 100)).random(shape) < density) * ON).astype(np.uint8)


def photo(rows=384, cols=512, seed=3):
    """A photo-like Rgb-free grey frame: a smooth gradient, discs, boxes and a slanted band under mild noise: Canny finds long closed
    contours, junctions where shapes overlap, and specks."""
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:rows, 0:cols].astype(np.float64)
    img = 60 + 50 * np.sin(xx / 90.0) * np.cos(yy / 70.0) + 0.1 * xx
    for _ in range(9):
        cy, cx, rad = rng.uniform(0, rows), rng.uniform(0, cols), rng.uniform(12, 70)
        img[np.hypot(yy - cy, xx - cx) < rad] += rng.uniform(-70, 90)
    for _ in range(6):
        r0, c0 = int(rng.uniform(0, rows - 40)), int(rng.uniform(0, cols - 60))
        img[r0:r0 + int(rng.uniform(15, 120)), c0:c0 + int(rng.uniform(15, 160))] += rng.uniform(-60, 80)
    img[np.abs(yy - 0.6 * xx - 40) < 9] += 45
    img += rng.normal(0, 2.0, img.shape)
    return np.clip(np.rint(img), 0, 255).astype(np.uint8)


FRAMES = {
    "empty": lambda: _blank(9, 13),
    "one_pixel": lambda: np.pad(np.full((1, 1), ON, np.uint8), 4),
    "full_row": lambda: np.pad(np.full((1, 21), ON, np.uint8), ((3, 3), (0, 0))),
    "full_column": lambda: np.pad(np.full((21, 1), ON, np.uint8), ((0, 0), (3, 3))),
    "1x1": lambda: np.full((1, 1), ON, np.uint8),
    "1x1_blank": lambda: _blank(1, 1),
    "1x70": lambda: np.full((1, 70), ON, np.uint8),
    "70x1": lambda: np.full((70, 1), ON, np.uint8),
    "all_16x16": lambda: np.full((16, 16), ON, np.uint8),
    "all_70x70": lambda: np.full((70, 70), ON, np.uint8),
    "steps": step_frame,
    "junctions": junctions,
    "diag_130": lambda: diagonal(130, 130),
    "anti_130": lambda: diagonal(130, 130, True, 127),  # (63, 64) -> (64, 63): across the tile corner
    "ring_130": lambda: ring(130, 130),
    "spiral_130": lambda: spiral(130, 130),
    "diag_65x200": lambda: diagonal(65, 200) | diagonal(65, 200, False, 64),  # through the corners at (64, 64) and (64, 128)
    "anti_65x200": lambda: diagonal(65, 200, True, 127) | diagonal(65, 200, True, 191),  # (63, 64) -> (64, 63), (63, 128) -> (64, 127)
    "ring_65x200": lambda: ring(65, 200, 32, 64, 23.0) | ring(65, 200, 64, 128, 30.0),
    "spiral_65x200": lambda: spiral(65, 200),
    "serpentine_260": lambda: serpentine(260, 260),
    "serpentine_260_t": lambda: np.ascontiguousarray(serpentine(260, 260).T),
}
for _d in (0.05, 0.3, 0.45, 0.6):
    for _s in (0, 1, 2):
        FRAMES["noise_%g_%d" % (_d, _s)] = functools.partial(noise, _d, _s)


@functools.lru_cache(maxsize=None)
def frame(name):
    e = np.ascontiguousarray(FRAMES[name]())
    e.flags.writeable = False
    return e


@functools.lru_cache(maxsize=None)
def want_raw(name):
    """The restatement's raw paths of a named frame, computed once."""
    return tuple(tuple(p) for p in R.trace_raw(frame(name)))


def want(name, min_path_length=5, eps=1.0):
    return R.finish(want_raw(name), frame(name).shape[1], min_path_length, eps)
