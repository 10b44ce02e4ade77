"""The shared cases of the seam-carving tests, built from the energy kernel's tile: B = zg_seam_band_rows() rows a launch,
S = zg_seam_strip_cols() columns a wave. Edge maps (u8) for the energy / seam / removal stages, and frames for the whole iteration."""
from collections import namedtuple

import numpy as np

EdgeCase = namedtuple("EdgeCase", "name edges seam tie")  # seam: the expected seam when the case forces one; tie: the wrong rule it must expose
PIXELS = ("u8", "f32", "rgb_u8", "rgba_u8", "rgb_f32", "rgba_f32")


def _noise(seed, shape, low=0, high=256):
    return np.random.default_rng(seed).integers(low, high, shape, dtype=np.uint8)


def valley_columns(B, S):
    """One column a row: right across the strip border S and a band border, then left across another band border and the strip border."""
    rows = 3 * B + 1
    turn = rows // 2
    start = S - B // 2 - 4
    return np.asarray([start + r if r <= turn else start + 2 * turn - r for r in range(rows)])


def edge_cases(B, S):
    cases = []

    def add(name, edges, seam=None, tie=None):
        cases.append(EdgeCase(name, np.ascontiguousarray(edges, np.uint8), None if seam is None else np.asarray(seam, np.uint32), tie))

    n = 2 * S + 3
    add("shape_1xN", _noise(1, (1, n)))
    add("shape_Nx2", _noise(2, (3 * B + 1, 2)))
    add("shape_Nx1", _noise(3, (B + 1, 1)))
    add("shape_2x2", _noise(4, (2, 2)))
    seed = 10
    for rows in (B - 1, B, B + 1, 2 * B + 1, 3 * B + 1):
        for cols in (S - 1, S, S + 1, 2 * S + 3):
            # few distinct values: equal sums, and so ties, are common
            add(f"shape_{rows}x{cols}", _noise(seed, (rows, cols), 0, 4 if seed % 2 else 256))
            seed += 1
    rows, cols = 2 * B + 1, S + 1
    add("flat", np.full((B + 1, S + 1), 7), seam=np.zeros(B + 1))
    right = np.full((rows, cols), 255)
    right[:, -1] = 1
    right[: rows // 2, 0] = 0  # cheap sums at the start of the rows: what a walker without the rule for column `cols` would read
    add("right_border", right, seam=np.full(rows, cols - 1))
    left = np.full((rows, cols), 255)
    left[:, 0] = 0
    add("left_border", left, seam=np.zeros(rows))
    v = valley_columns(B, S)
    valley = np.full((len(v), 2 * S + 3), 255)
    valley[np.arange(len(v)), v] = 0
    add("diagonal_valley", valley, seam=v)
    add("all_255", np.full((3 * B + 1, S + 1), 255), seam=np.zeros(3 * B + 1))
    # ties among the three sums above the seam: a unique minimum in the bottom row at column m, the pattern above it
    for m in (2, S - 1, S):
        width = m + 3
        for name, (l, c, r), tie, want in (("left_eq_centre", (1, 1, 5), "leftmost", m), ("centre_eq_right", (5, 1, 1), "rightmost", m),
                                           ("left_eq_right", (1, 5, 1), "rightmost", m - 1)):
            e = np.full((2, width), 9)
            e[0, m - 1: m + 2] = (l, c, r)
            e[1, m] = 0
            add(f"tie_{name}_at_{m}", e, seam=(want, m), tie=tie)
    two = np.full((B + 2, S + 2), 3)
    two[-1, 5] = two[-1, S] = 0  # two minima in the bottom row
    add("tie_bottom_row", two, tie="last")
    return cases


def frame(seed, rows, cols, pixel):
    """A frame with structure (a few soft blobs) and noise on top, of one of the six pixel types."""
    rng = np.random.default_rng(seed)
    ch = {"u8": 1, "f32": 1, "rgb_u8": 3, "rgba_u8": 4, "rgb_f32": 3, "rgba_f32": 4}[pixel]
    yy, xx = np.mgrid[0:rows, 0:cols]
    plane = np.zeros((rows, cols, ch))
    for _ in range(4):
        cy, cx, rad = rng.uniform(0, rows), rng.uniform(0, cols), rng.uniform(2, 2 + max(rows, cols) / 3)
        plane += (((yy - cy) ** 2 + (xx - cx) ** 2) < rad * rad)[..., None] * rng.uniform(20, 120, ch)
    plane += rng.uniform(0, 24, (rows, cols, ch))
    plane = np.clip(plane, 0, 255)
    if pixel.endswith("u8"):
        out = plane.astype(np.uint8)
    elif pixel == "f32":
        out = plane.astype(np.float32)  # a scalar float frame is its own grey plane
    else:
        out = (plane / 255.0).astype(np.float32)
    return np.ascontiguousarray(out[..., 0] if ch == 1 else out)


def pixels_like(seed, rows, cols, pixel):
    """Arbitrary pixels of a type, for the removal (which only moves them)."""
    rng = np.random.default_rng(seed)
    ch = {"u8": 1, "f32": 1, "rgb_u8": 3, "rgba_u8": 4, "rgb_f32": 3, "rgba_f32": 4}[pixel]
    shape = (rows, cols) if ch == 1 else (rows, cols, ch)
    if pixel.endswith("u8"):
        return rng.integers(0, 256, shape, dtype=np.uint8)
    return rng.standard_normal(shape).astype(np.float32)
