"""f32 test frames outside [0, 1): negative values, exponents up to 126, subnormals, both zeros, infinities and NaN. tests/util.py: synth
yields non-negative multiples of 2^-24 below 1 only; the frames here are what tests/test_gpu_f32_domain.py runs the f32 routes on, and
tests/test_domain_frames.py holds each of them to its name without a GPU.

frame(name, kind, rows, cols) is deterministic (the generator is seeded from its four arguments) and returns a read-only array."""
import functools
import zlib

import numpy as np

CHANNELS = {"f32": 1, "rgb_f32": 3, "rgba_f32": 4}
NAMES = ("signed", "tiny", "huge", "huge_sat", "negzero", "nonfinite", "nonfinite_corner")
NEG_ZERO, POS_INF, NEG_INF, QNAN = 0x80000000, 0x7F800000, 0xFF800000, 0x7FC00000
# The order in which nonfinite places them at nonfinite_sites(). The two NaN sit on the last row and the last column, where a 17-tap blur
# spreads each over 9 x 17 pixels and not 17 x 17 (47 x 67 keeps below 10 % NaN that way); infinities whose 17 x 17 neighbourhoods meet (the
# corner and the first interior point, the centre and the second) have the same sign, so that they make no NaN between them.
SPECIALS = (POS_INF, NEG_INF, QNAN, QNAN, POS_INF, NEG_INF)
PATCH = 4  # negzero's patch of 1.5 is PATCH x PATCH pixels


def _rng(name, kind, rows, cols):
    return np.random.default_rng(zlib.crc32(f"{name}/{kind}/{rows}x{cols}".encode()))


def _sign_exponent_mantissa(rng, shape, lo, hi):
    """Random sign, unbiased exponent in lo..hi, random mantissa: the bit patterns."""
    sign = rng.integers(0, 2, shape, dtype=np.uint32) << np.uint32(31)
    exponent = rng.integers(lo + 127, hi + 128, shape, dtype=np.uint32) << np.uint32(23)
    return sign | exponent | rng.integers(0, 1 << 23, shape, dtype=np.uint32)


def nonfinite_sites(rows, cols):
    """(row, col) of the six specials of `nonfinite`, in the order of SPECIALS: the top-left corner, the centre, the last row, the last
    column and two interior points."""
    return ((0, 0), (rows // 2, cols // 2), (rows - 1, cols // 3), (rows // 3, cols - 1), (rows // 4, cols // 4), (3 * rows // 4, 2 * cols // 3))


def corner_sites(rows, cols):
    """(row, col) of the three specials of `nonfinite_corner` (+inf, -inf, NaN), inside the bottom-right 3 x 3 pixels."""
    return ((rows - 3, cols - 2), (rows - 2, cols - 3), (rows - 1, cols - 1))


def _background(rng, shape):
    return ((rng.random(shape, np.float32) - np.float32(0.5)) * np.float32(4)).view(np.uint32)


@functools.lru_cache(maxsize=None)
def frame(name, kind, rows, cols):
    ch = CHANNELS[kind]
    shape = (rows, cols, ch)
    rng = _rng(name, kind, rows, cols)
    if name == "signed":
        bits = _sign_exponent_mantissa(rng, shape, -40, 40)
    elif name == "tiny":  # below 2^25: biased exponents 0..3, so subnormals and the smallest normals
        bits = rng.integers(0, 1 << 25, shape, dtype=np.uint32) | (rng.integers(0, 2, shape, dtype=np.uint32) << np.uint32(31))
        flat = bits.reshape(-1)
        flat[::19] = 0
        flat[::17] = NEG_ZERO  # a multiple of both is -0.0
    elif name == "huge":
        bits = _sign_exponent_mantissa(rng, shape, 107, 126)
    elif name == "huge_sat":  # what an integral image of a few thousand pixels still holds in f32
        bits = _sign_exponent_mantissa(rng, shape, 90, 109)
    elif name == "negzero":
        bits = np.full(shape, NEG_ZERO, np.uint32)
        bits[::3, ::5] = 0
        r0, c0 = rows // 2, cols // 2 + 1  # off the +0.0 grid's corner on purpose: the patch covers some of each zero
        bits[r0:r0 + PATCH, c0:c0 + PATCH] = np.float32(1.5).view(np.uint32)
    elif name == "nonfinite":
        bits = _background(rng, shape)
        for i, ((r, c), special) in enumerate(zip(nonfinite_sites(rows, cols), SPECIALS)):
            bits[r, c, i % ch] = special
    elif name == "nonfinite_corner":
        bits = _background(rng, shape)
        for i, ((r, c), special) in enumerate(zip(corner_sites(rows, cols), SPECIALS)):
            bits[r, c, i % ch] = special
    else:
        raise KeyError(name)
    out = np.ascontiguousarray(bits).view(np.float32).reshape((rows, cols) if ch == 1 else shape)
    out.flags.writeable = False
    return out


# ---- classes of f32 values, by bit pattern (numpy's own predicates treat -0.0 == 0.0) ----------------------------------------------------
def u32(a):
    return np.ascontiguousarray(a).view(np.uint32)


def is_nan(a):
    return (u32(a) & np.uint32(0x7FFFFFFF)) > np.uint32(0x7F800000)


def is_inf(a):
    return (u32(a) & np.uint32(0x7FFFFFFF)) == np.uint32(0x7F800000)


def is_subnormal(a):
    m = u32(a) & np.uint32(0x7FFFFFFF)
    return (m != 0) & (m < np.uint32(0x00800000))


def is_neg_zero(a):
    return u32(a) == np.uint32(NEG_ZERO)


def is_pos_zero(a):
    return u32(a) == np.uint32(0)
