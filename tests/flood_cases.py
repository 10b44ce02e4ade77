"""Named flood-fill cases shared by tests/test_flood_oracle.py (CPU) and tests/test_gpu_flood.py, built from the tile side T of the
device code (zg_flood_fill_tile()), so that shapes, seeds and links fall on both sides of a tile edge without the tests hard-coding it.

A generic case is a (rows, cols) plane of small integers, a seed, a threshold in the plane's units and a fill value; image_of() turns it
into any of the six pixel types: the plane goes into one channel (`channel` modulo the channel count; 3 is alpha for Rgba), the other
channels hold constants, and float types halve everything (values, threshold, fill), which is exact in binary, so a case links the
same pixels in every type. A typed case carries its image as it is and names the one pixel type it is about.

Every case is run with both modes and both connectivities; the expected bytes always come from tests/flood_ref.py."""
import math
from typing import NamedTuple, Optional, Tuple

import numpy as np

PIXELS = ("u8", "f32", "rgb_u8", "rgba_u8", "rgb_f32", "rgba_f32")  # in the order of ZG_PIXEL_*
CHANNELS = {"u8": 1, "f32": 1, "rgb_u8": 3, "rgba_u8": 4, "rgb_f32": 3, "rgba_f32": 4}
MODES = ("seed", "neighbor")
CONNECTIVITIES = (4, 8)
BASE = (10, 60, 30, 77)  # the channels the plane does not occupy
WALL, FLOOR = 200, 50


class Case(NamedTuple):
    name: str
    plane: Optional[np.ndarray]        # generic: (rows, cols) uint8
    seed: Tuple[int, int]
    threshold: float
    fill: Optional[int]                # generic: the plane-unit fill value; None: the seed's own value
    channel: int = 0
    image: Optional[np.ndarray] = None  # typed: the image itself
    pixel: Optional[str] = None        # typed: its pixel type
    fill_value: object = None          # typed: the fill value as given to the call


def is_float(pixel):
    return pixel.endswith("f32")


def dtype_of(pixel):
    return np.float32 if is_float(pixel) else np.uint8


def pixels_of(case):
    return PIXELS if case.pixel is None else (case.pixel,)


def _typed(values, pixel, channel):
    """A plane (or one value) of plane units as pixels of `pixel`."""
    values = np.asarray(values)
    scale = 0.5 if is_float(pixel) else 1
    ch = CHANNELS[pixel]
    if ch == 1:
        return (values * scale).astype(dtype_of(pixel))
    out = np.empty(values.shape + (ch,), dtype_of(pixel))
    for k in range(ch):
        out[..., k] = (values if k == channel % ch else BASE[k]) * scale
    return out


def image_of(case, pixel):
    if case.image is not None:
        assert pixel == case.pixel
        return case.image.copy()
    return np.ascontiguousarray(_typed(case.plane, pixel, case.channel))


def threshold_of(case, pixel):
    return case.threshold * (0.5 if is_float(pixel) and case.image is None else 1)


def fill_of(case, pixel):
    if case.image is not None:
        return case.fill_value
    v = case.plane[case.seed] if case.fill is None else case.fill
    out = _typed(v, pixel, case.channel)
    return out.item() if out.ndim == 0 else tuple(out.tolist())


# ---- planes ---------------------------------------------------------------------------------------------------------------------
def blobs(seed, rows, cols):
    """Patches of 100 / 101 / 103 a few pixels wide with a tenth of the pixels redrawn: with threshold 1, 100 and 101 link and 103
    stands apart, components are many, of every size, and cross tile edges."""
    rng = np.random.default_rng(seed)
    coarse = rng.integers(0, 3, ((rows + 2) // 3, (cols + 2) // 3))
    idx = np.kron(coarse, np.ones((3, 3), np.int64))[:rows, :cols]
    redraw = rng.random((rows, cols)) < 0.1
    idx = np.where(redraw, rng.integers(0, 3, (rows, cols)), idx)
    return np.array([100, 101, 103], np.uint8)[idx]


def first_of(plane, value, near):
    """The pixel holding `value` nearest to `near` (a seed that sits in a region of the wanted kind)."""
    rr, cc = np.nonzero(plane == value)
    k = int(np.argmin((rr - near[0]) ** 2 + (cc - near[1]) ** 2))
    return int(rr[k]), int(cc[k])


def spiral(n):
    """A one-pixel corridor of FLOOR between one-pixel walls, from (0, 0) inwards: about n * n / 2 pixels in one chain."""
    g = np.full((n, n), WALL, np.uint8)
    t, l, b, r = 0, 0, n - 1, n - 1
    while t <= b and l <= r:
        g[t, max(l - 2, 0):r + 1] = FLOOR
        g[t:b + 1, r] = FLOOR
        g[b, l:r + 1] = FLOOR
        g[t + 2:b + 1, l] = FLOOR
        t, l, b, r = t + 2, l + 2, b - 2, r - 2
    return g


def comb(rows, cols):
    g = np.full((rows, cols), WALL, np.uint8)
    g[0, :] = FLOOR
    g[:, ::2] = FLOOR  # a tooth in every other column, down to the last row
    return g


def frame(n):
    """A ring along the four image edges and a cross through the centre."""
    g = np.full((n, n), WALL, np.uint8)
    g[0, :] = g[-1, :] = g[:, 0] = g[:, -1] = FLOOR
    g[n // 2, :] = g[:, n // 2] = FLOOR
    return g


def checkerboard(rows, cols):
    rr, cc = np.indices((rows, cols))
    return np.where((rr + cc) % 2 == 0, FLOOR, WALL).astype(np.uint8)


def corner_link(T, main_diagonal):
    """Two 4 x 4 squares in diagonally opposite tiles of a 2T x 2T frame that touch only across the shared tile corner."""
    g = np.full((2 * T, 2 * T), WALL, np.uint8)
    if main_diagonal:
        g[T - 4:T, T - 4:T] = FLOOR
        g[T:T + 4, T:T + 4] = FLOOR
        return g, (T - 2, T - 2)
    g[T - 4:T, T:T + 4] = FLOOR
    g[T:T + 4, T - 4:T] = FLOOR
    return g, (T - 2, T + 1)


# ---- typed cases ------------------------------------------------------------------------------------------------------------------
def _sqrt_cases(pixel):
    """Struct-of-u8 pixels at known squared distances from the seed, with thresholds exactly sqrt(s) and the f64 just below it."""
    ch = CHANNELS[pixel]
    base = np.array(BASE[:ch], np.int64)
    if pixel == "rgba_u8":  # alpha is the only field that differs
        offsets = [(0, 0, 0, 5), (0, 0, 0, 7), (0, 0, 0, 1), (0, 0, 0, 8), (0, 0, 0, 0), (0, 0, 0, 5), (0, 0, 0, 6), (0, 0, 0, 4)]
        thresholds = {"sqrt25": 5.0, "sqrt49": 7.0}
    else:
        offsets = [(1, 1, 1), (1, 2, 2), (2, 3, 6), (1, 1, 0), (3, 4, 5), (0, 0, 0), (1, 1, 1), (5, 5, 1)]
        thresholds = {"sqrt3": math.sqrt(3.0), "sqrt50": math.sqrt(50.0), "sqrt51": math.sqrt(51.0)}
    img = np.empty((3, 9, ch), np.uint8)
    img[:] = base + np.array((0, 0, 0, 100) if pixel == "rgba_u8" else (9, 9, 9))  # far away
    img[1, 4] = base
    for k, off in enumerate(offsets):  # a row through the seed: every pixel links to the seed's side only through the ones before it
        col = 4 + (k // 2 + 1) * (1 if k % 2 == 0 else -1)
        img[1, col] = base + np.array(off)
    img[0, :] = img[1, :][::-1]
    fill = tuple(int(v) for v in (base + 100))
    out = []
    for name, t in thresholds.items():
        out.append(Case(f"{pixel}_{name}", None, (1, 4), t, None, image=img, pixel=pixel, fill_value=fill))
        out.append(Case(f"{pixel}_{name}_below", None, (1, 4), math.nextafter(t, 0.0), None, image=img, pixel=pixel, fill_value=fill))
    return out


def _f32_special_cases():
    nan, inf = np.float32("nan"), np.float32("inf")
    img = np.array([[1.0, 1.5, nan, 1.0, inf, inf, 2.0],
                    [1.0, -inf, 1.0, 1.25, 3.0e38, -3.0e38, 2.0],
                    [nan, 1.0, 1.0, inf, 1.0, -inf, -inf]], np.float32)
    out = []
    for name, seed, t in (("finite_seed", (0, 0), 0.5), ("finite_seed_inf_threshold", (0, 0), math.inf), ("nan_seed", (0, 2), math.inf),
                          ("nan_seed_zero", (2, 0), 0.0), ("inf_seed", (0, 4), 0.0), ("inf_seed_inf_threshold", (0, 4), math.inf),
                          ("huge_difference", (1, 4), 3.0e38)):
        out.append(Case(f"f32_{name}", None, seed, t, None, image=img, pixel="f32", fill_value=-7.5))
    return out


def _float_struct_cases(pixel):
    """A threshold at a boundary of S(t): the f64 square root of one pixel's f64 sum of squares, and the f64 below it."""
    ch = CHANNELS[pixel]
    base = np.array((0.25, 0.5, 0.75, 1.0)[:ch], np.float32)
    steps = [np.array((1e-3, 2e-3, 5e-4, 7e-4)[:ch], np.float32), np.array((0.2, 0.1, 0.15, 0.05)[:ch], np.float32),
             np.array((0.1, 0.2, 0.3, 0.4)[:ch], np.float32)]  # ascending in length: each is reached through the shorter ones
    img = np.empty((2, 7, ch), np.float32)
    img[:] = base + np.float32(10)
    img[0, 3] = base
    for k, step in enumerate(steps):
        img[0, 3 + k + 1] = img[0, 3 + k] + step  # neighbor mode walks to the right step by step
        img[0, 3 - k - 1] = base + step           # seed mode sees each step from the seed
    img[1, :] = img[0, ::-1]
    out = []
    for k in range(len(steps)):
        a, b = img[0, 3].astype(np.float64), img[0, 3 - k - 1].astype(np.float64)
        sum_sq = 0.0
        for x, y in zip(a.tolist(), b.tolist()):
            sum_sq += (y - x) * (y - x)
        t = math.sqrt(sum_sq)
        out.append(Case(f"{pixel}_step{k}", None, (0, 3), t, None, image=img, pixel=pixel, fill_value=(-1.0,) * ch))
        out.append(Case(f"{pixel}_step{k}_below", None, (0, 3), math.nextafter(t, 0.0), None, image=img, pixel=pixel, fill_value=(-1.0,) * ch))
    out.append(Case(f"{pixel}_inf_threshold", None, (0, 3), math.inf, None, image=img, pixel=pixel, fill_value=(-1.0,) * ch))
    return out


# ---- the list ---------------------------------------------------------------------------------------------------------------------
def cases(T):
    """Every case, in a fixed order, for tile side T."""
    out = []
    sides = (T - 1, T, T + 1, 2 * T + 1)
    k = 0
    for rows in sides:
        for cols in sides:
            p = blobs(1000 + k, rows, cols)
            out.append(Case(f"shape_{rows}x{cols}", p, first_of(p, 100, (rows // 2, cols // 2)), 1.0, 9, channel=k))
            k += 1
    out.append(Case("shape_1x1", np.array([[100]], np.uint8), (0, 0), 1.0, 9))
    line = blobs(7, 1, 2 * T + 1)
    out.append(Case("shape_1xN", line, first_of(line, 100, (0, T)), 1.0, 9, channel=1))
    out.append(Case("shape_Nx1", np.ascontiguousarray(line.T), first_of(line.T, 100, (T, 0)), 1.0, 9, channel=2))
    out.append(Case("spiral", spiral(3 * T + 1), (0, 0), 0.0, 9, channel=3))
    out.append(Case("spiral_from_the_centre", spiral(3 * T + 1), first_of(spiral(3 * T + 1), FLOOR, (3 * T // 2, 3 * T // 2)), 0.0, 9))
    out.append(Case("comb", comb(T + 5, 2 * T + 3), (T + 4, 2 * T + 2), 0.0, 9, channel=1))
    n = 2 * T + 1
    for name, seed in (("tl", (0, 0)), ("tr", (0, n - 1)), ("bl", (n - 1, 0)), ("br", (n - 1, n - 1))):
        out.append(Case(f"four_edges_seed_{name}", frame(n), seed, 0.0, 9, channel=2))
    p = blobs(77, 2 * T, 2 * T)
    p[T - 2:T + 2, T - 2:T + 2] = 100  # the four pixels round the tile corner share a region
    for name, seed in (("nw", (T - 1, T - 1)), ("ne", (T - 1, T)), ("sw", (T, T - 1)), ("se", (T, T))):
        out.append(Case(f"tile_corner_seed_{name}", p, seed, 1.0, 9, channel=3))
    out.append(Case("checkerboard", checkerboard(T + 2, T + 3), (1, 1), 0.0, 9))
    for name, main in (("corner_link_main", True), ("corner_link_anti", False)):
        g, seed = corner_link(T, main)
        out.append(Case(name, g, seed, 0.0, 9, channel=1))
    ramp = np.broadcast_to(np.arange(T + 10, dtype=np.uint8), (3, T + 10)).copy()
    out.append(Case("ramp_across", ramp, (1, 40), 1.0, 250, channel=2))
    out.append(Case("ramp_down", np.ascontiguousarray(ramp.T), (40, 1), 1.0, 250, channel=3))
    p = blobs(5, T + 1, T + 1)
    seed = first_of(p, 100, (T // 2, T // 2))
    for name, t in (("zero", 0.0), ("minus_zero", -0.0), ("minus_one", -1.0), ("nan", math.nan), ("inf", math.inf)):
        out.append(Case(f"threshold_{name}", p, seed, t, 9, channel=1))
    out.append(Case("fill_equals_seed", p, seed, 1.0, None, channel=2))
    out.append(Case("region_already_holds_fill", p, seed, 1.0, 101, channel=3))
    for pixel in ("rgb_u8", "rgba_u8"):
        out += _sqrt_cases(pixel)
    out += _f32_special_cases()
    for pixel in ("rgb_f32", "rgba_f32"):
        out += _float_struct_cases(pixel)
    assert len({c.name for c in out}) == len(out)
    return out
