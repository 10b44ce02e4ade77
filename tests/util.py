"""Shared helpers for the GPU parity tests."""
import numpy as np

SHAPES = {"u8": (), "f32": (), "rgb_u8": (3,), "rgba_u8": (4,), "rgb_f32": (3,), "rgba_f32": (4,)}
IS_FLOAT = {"u8": False, "f32": True, "rgb_u8": False, "rgba_u8": False, "rgb_f32": True, "rgba_f32": True}
ALL_TYPES = tuple(SHAPES)


def synth(oracle, kind: str, seed: int, rows: int, cols: int) -> np.ndarray:
    shape = (rows, cols) + SHAPES[kind]
    return oracle.synth_f32(seed, shape) if IS_FLOAT[kind] else oracle.synth_u8(seed, shape)


def assert_bits_equal(got: np.ndarray, want: np.ndarray, what: str = ""):
    assert got.shape == want.shape and got.dtype == want.dtype, f"{what}: {got.shape}/{got.dtype} vs {want.shape}/{want.dtype}"
    g, w = np.ascontiguousarray(got), np.ascontiguousarray(want)
    if g.dtype == np.float32:
        g, w = g.view(np.uint32), w.view(np.uint32)
    if not np.array_equal(g, w):
        bad = np.argwhere(g != w)
        first = tuple(bad[0])
        raise AssertionError(f"{what}: {len(bad)} of {g.size} elements differ; first at {first}: "
                             f"got {got[first]!r} want {want[first]!r}")


def assert_bits_equal_nan_class(got: np.ndarray, want: np.ndarray, what: str = ""):
    """assert_bits_equal with NaN as one class: for f32 the NaN positions must be the same set and every other element bit-equal (the sign
    of a zero and of an infinity count); a NaN's payload and sign do not (x86 and gfx950 propagate payloads differently and the reference
    promises neither). Anything that is not f32 goes through assert_bits_equal."""
    if got.dtype != np.float32 or want.dtype != np.float32:
        return assert_bits_equal(got, want, what)
    assert got.shape == want.shape, f"{what}: {got.shape} vs {want.shape}"
    g, w = np.ascontiguousarray(got).view(np.uint32).copy(), np.ascontiguousarray(want).view(np.uint32).copy()
    for bits in (g, w):  # every NaN becomes the one quiet NaN; no other pattern maps to it
        bits[(bits & np.uint32(0x7FFFFFFF)) > np.uint32(0x7F800000)] = np.uint32(0x7FC00000)
    if not np.array_equal(g, w):
        bad = np.argwhere(g != w)
        first = tuple(bad[0])
        raise AssertionError(f"{what}: {len(bad)} of {g.size} elements differ (NaN as a class); first at {first}: "
                             f"got {got[first]!r} ({int(np.ascontiguousarray(got).view(np.uint32)[first]):#010x}) "
                             f"want {want[first]!r} ({int(np.ascontiguousarray(want).view(np.uint32)[first]):#010x})")


def ulp_diff(a: np.ndarray, b: np.ndarray) -> np.ndarray:
    ai = a.view(np.int32).astype(np.int64)
    bi = b.view(np.int32).astype(np.int64)
    ai = np.where(ai < 0, np.int64(-2147483648) - ai, ai)
    bi = np.where(bi < 0, np.int64(-2147483648) - bi, bi)
    return np.abs(ai - bi)
