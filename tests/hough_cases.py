"""The inputs the Hough tests share, each with its expected result from tests/hough_ref.py computed once and left unchanged:
tests/test_hough_oracle.py asserts, without a GPU, that they reach the branches they are there for; tests/test_gpu_hough.py runs the
device code on them."""
import functools
from collections import Counter

import numpy as np

from tests import hough_ref as R


def random_edges(seed, rows, cols, density):
    rng = np.random.default_rng(seed)
    values = rng.choice(np.array([1, 128, 255], np.uint8), (rows, cols))  # the three edge values: every non-zero byte votes once
    return np.where(rng.random((rows, cols)) < density, values, 0).astype(np.uint8)


def draw_line(edges, p, q, value=255):
    n = int(max(abs(q[0] - p[0]), abs(q[1] - p[1]))) + 1
    rows = np.round(np.linspace(p[0], q[0], n)).astype(int)
    cols = np.round(np.linspace(p[1], q[1], n)).astype(int)
    ok = (rows >= 0) & (rows < edges.shape[0]) & (cols >= 0) & (cols < edges.shape[1])
    edges[rows[ok], cols[ok]] = value


def exactly(seed, size, count):
    """A size x size edge map with exactly `count` non-zero bytes."""
    rng = np.random.default_rng(seed)
    edges = np.zeros(size * size, np.uint8)
    edges[rng.choice(size * size, count, replace=False)] = 255
    return edges.reshape(size, size)


@functools.lru_cache(maxsize=None)
def compute_cases(lds_max_size: int, pixel_chunk: int):
    """name -> (edges, box, size, start): `start` is what the accumulator holds before the call (None: zeros)."""
    cases = {}
    for size in (2, 3, 4, 5, 63, 64, 97):  # 5, 63, 97 are odd: the last column is theta = pi
        cases[f"random{size}"] = (random_edges(size, size, size, 0.2 if size > 5 else 0.7), (0, 0, size, size), size, None)
    big = lds_max_size + 1
    sparse = random_edges(7, big, big, 300.0 / (big * big))
    draw_line(sparse, (100, 50), (big - 300, big - 20))
    cases["above_lds"] = (sparse, (0, 0, big, big), big, None)
    cases["dense64"] = (np.ones((64, 64), np.uint8), (0, 0, 64, 64), 64, None)
    lines = random_edges(11, 120, 110, 0.02)
    for p, q in (((35, 25), (100, 105)), ((60, 0), (62, 109)), ((0, 70), (119, 64))):
        draw_line(lines, p, q)
    cases["lines97_box_past_right"] = (lines, (20, 30, 117, 127), 97, None)  # the 120 x 110 image ends at column 110 and row 120
    inside = random_edges(12, 130, 125, 0.02)
    for p, q in (((35, 25), (120, 115)), ((60, 20), (62, 116)), ((30, 70), (126, 64))):
        draw_line(inside, p, q)
    cases["lines97_box_inside"] = (inside, (20, 30, 117, 127), 97, None)
    cases["box_past_bottom"] = (random_edges(13, 40, 80, 0.1), (5, 20, 69, 84), 64, None)
    cases["box_past_corner"] = (random_edges(14, 40, 50, 0.1), (10, 20, 74, 84), 64, None)
    cases["box_misses_right"] = (random_edges(15, 40, 50, 0.5), (50, 0, 114, 64), 64, np.full((64, 64), 3, np.uint32))
    cases["box_misses_below"] = (random_edges(15, 40, 50, 0.5), (0, 40, 64, 104), 64, np.full((64, 64), 3, np.uint32))
    rng = np.random.default_rng(16)
    cases["starts_non_zero"] = (random_edges(17, 64, 64, 0.05), (0, 0, 64, 64), 64, rng.integers(0, 1 << 32, (64, 64), dtype=np.uint32))
    for count in (pixel_chunk - 1, pixel_chunk, pixel_chunk + 1, 2 * pixel_chunk + 1, 8 * pixel_chunk + 1):
        cases[f"edges{count}"] = (exactly(count, 97, count), (0, 0, 97, 97), 97, None)
    for c in cases.values():
        c[0].setflags(write=False)
        if c[3] is not None:
            c[3].setflags(write=False)
    return cases


@functools.lru_cache(maxsize=None)
def want_accumulator(name: str, lds_max_size: int, pixel_chunk: int):
    edges, box, size, start = compute_cases(lds_max_size, pixel_chunk)[name]
    acc = np.zeros((size, size), np.uint32) if start is None else start.copy()
    with np.errstate(over="ignore"):
        R.compute_fast(edges, box, acc, size)  # u32 counters wrap like the device's when `start` is near 2^32; no case gets there
    acc.setflags(write=False)
    return acc


def hand_made():
    """name -> (size, accumulator)."""
    out = {}
    out["ties9"] = (9, np.zeros((9, 9), np.uint32))
    plateau = np.zeros((12, 12), np.uint32)
    plateau[3:5, 3:6] = 9       # six equal cells: none has a strictly greater neighbour, all are candidates
    plateau[8, 8:10] = 9
    plateau[7, 8] = 10          # strictly greater: (8, 8) and (8, 9) are no candidates, (7, 8) is
    plateau[10, 2] = 5
    plateau[1, 10] = 9          # first interior row, last interior column
    plateau[0, 5] = 20          # a border cell is no candidate but hides its interior neighbours
    plateau[1, 4:7] = 6
    out["plateau"] = (12, plateau)
    wrap = np.zeros((33, 33), np.uint32)
    wrap[20, 1], wrap[12, 31] = 50, 40      # angles -84.375 and 84.375, radii 5.66 and -5.66: the same line met from both ends
    wrap[25, 1], wrap[25, 31] = 30, 20      # radii of equal sign: two lines
    out["wrap"] = (33, wrap)
    angles = np.zeros((33, 33), np.uint32)
    for i, (r, c) in enumerate(((16, 16), (1, 16), (31, 16), (16, 1), (16, 31), (1, 1), (31, 31), (1, 31), (31, 1), (8, 8), (24, 8), (8, 24), (24, 24),
                                (4, 16), (28, 16), (16, 4), (16, 28), (2, 9), (30, 23), (5, 30), (29, 2))):
        angles[r, c] = 100 - i
    out["angles33"] = (33, angles)
    even = np.zeros((34, 34), np.uint32)
    for i, (r, c) in enumerate(((17, 17), (16, 16), (1, 17), (32, 16), (17, 1), (16, 32), (1, 1), (32, 32), (1, 32), (32, 1), (9, 25), (25, 9))):
        even[r, c] = 60 - i
    out["angles34"] = (34, even)
    out["size3"] = (3, np.array([[0, 0, 0], [0, 4, 0], [0, 0, 0]], np.uint32))
    out["size2"] = (2, np.ones((2, 2), np.uint32))
    out["trips259"] = (259, trip_boundaries(259))  # 257 interior cells a side: two trips, the second with one live thread
    out["trips515"] = (515, trip_boundaries(515))  # 513: three trips
    return out


TRIP_ROW = 100  # the row of trip_boundaries' plateaus


def trip_marks(size):
    """The rows and columns m that are the last cell of a 256-cell trip (interior cell m is index m - 1): m + 1 opens the next trip."""
    return [m for m in (256, 512) if m < size - 2]


def trip_boundaries(size):
    """Zeros and a few dozen peaks for findLines' device loops, which walk the interior columns of a row and the interior rows 256 cells
    a trip and carry a sum from trip to trip: candidates on both sides of every trip's end in a row and in the rows, empty rows
    between candidate rows, one in the last interior row and column. Scores are distinct (the order is forced) but for two far-apart
    pairs and the plateaus of TRIP_ROW, whose cells are neighbours and so must be equal to be candidates: the stable sort's path."""
    acc = np.zeros((size, size), np.uint32)
    last = size - 2
    score = [3000]

    def peak(r, c, value=None):
        assert not acc[r - 1:r + 2, c - 1:c + 2].any(), (r, c)  # no neighbour: a lower peak next to a higher one is no candidate
        acc[r, c] = score[0] if value is None else value
        score[0] -= 5

    for m in trip_marks(size):
        acc[TRIP_ROW, m - 1:m + 3] = 5000 + m  # columns m - 1 .. m + 2; the last plateau ends on the border column, which is no candidate
        peak(m, 40)           # the last row of a trip ...
        peak(m, m - 2)
        peak(m + 1, 90)       # ... and the first of the next
        peak(m + 1, m + 1)    # size 259 and 515: the last interior row and column
    assert acc[last, last] != 0
    for r in (1, 37, 129, 254, 300, 400, 510):
        if r < last:
            for c in (2, 64 + r % 7, 131, 254, 300, 509, last):
                if c <= last:
                    peak(r, c)
    peak(30, 20, 4000)
    peak(200, 240, 4000)  # equal scores far apart: row-major order decides
    peak(60, 200, 4100)
    peak(60, 10, 4100)
    return acc


NAN, INF = float("nan"), float("inf")


@functools.lru_cache(maxsize=None)
def find_cases(lds_max_size: int, pixel_chunk: int):
    """name -> (size, accumulator, threshold, angle_nms_thresh, radius_nms_thresh)."""
    cases = {}
    hm = hand_made()
    for name, (a, r) in (("default", (10.0, 5.0)), ("nan_angle", (NAN, 5.0)), ("nan_radius", (10.0, NAN)), ("negative", (-1.0, -1.0)),
                         ("inf", (INF, INF)), ("zero", (0.0, 0.0)), ("wide", (180.0, 1.5))):
        cases[f"ties9_{name}"] = (9, hm["ties9"][1], 0, a, r)
    cases["plateau"] = (12, hm["plateau"][1], 5, 10.0, 1.0)
    cases["plateau_threshold_above_all"] = (12, hm["plateau"][1], 21, 10.0, 1.0)
    cases["wrap"] = (33, hm["wrap"][1], 10, 15.0, 3.0)
    cases["wrap_off"] = (33, hm["wrap"][1], 10, 11.25, 3.0)  # 180 - da = 11.25 is not < 11.25
    cases["angles33"] = (33, hm["angles33"][1], 1, 1.0, 1.0)
    cases["angles34"] = (34, hm["angles34"][1], 1, 1.0, 1.0)
    cases["size3"] = (3, hm["size3"][1], 1, 10.0, 5.0)
    cases["size2"] = (2, hm["size2"][1], 0, 10.0, 5.0)
    cases["trips259"] = (259, hm["trips259"][1], 1, 1.0, 1.0)  # a low threshold and narrow suppression: most candidates become lines
    cases["trips515"] = (515, hm["trips515"][1], 1, 1.0, 1.0)
    for name, thr in (("random63", None), ("random64", None), ("random97", None), ("dense64", None), ("lines97_box_inside", None),
                      ("lines97_box_past_right", None), ("starts_non_zero", 1 << 31)):
        acc = want_accumulator(name, lds_max_size, pixel_chunk)
        cases[f"acc_{name}"] = (acc.shape[0], acc, max(1, int(acc.max()) // 2) if thr is None else thr, 5.0, 5.0)
    edges = np.zeros((64, 64), np.uint8)
    edges[32, :] = 255
    row = R.compute_fast(edges, (0, 0, 64, 64), np.zeros((64, 64), np.uint32), 64)
    cases["row32"] = (64, row, 30, 10.0, 5.0)
    cases["row32_high"] = (64, row, 24, 2.0, 2.0)
    for c in cases.values():
        c[1].setflags(write=False)
    return cases


@functools.lru_cache(maxsize=None)
def want_lines(name: str, lds_max_size: int, pixel_chunk: int):
    """(number of candidates, lines, counters) of the reference."""
    size, acc, thr, a, r = find_cases(lds_max_size, pixel_chunk)[name]
    counters = Counter()
    n, lines = R.find_lines(acc, size, thr, a, r, counters)
    lines.setflags(write=False)
    return n, lines, counters
