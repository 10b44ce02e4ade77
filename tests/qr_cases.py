"""Symbol-like frames for the QR detector tests, built without any table of the standard: a dim x dim module matrix with the three finder
patterns and their separators, the two timing lines, for version >= 2 one alignment pattern centred at (dim - 7, dim - 7), for version >= 7
both version-information blocks from the BCH formula, and seeded random modules everywhere else; rendered at a chosen module size with a
4-module quiet zone through a chosen homography onto a grey frame (dark 30, light 200), optionally with a linear lighting gradient, seeded
+-20 noise and a horizontal mirror. The detector never decodes, so the data region needs no meaning.

CASES are the frames of tests/test_gpu_qr.py; `want(name)` is the restatement's result on the case's binary map, computed once."""
import functools
import math

import numpy as np

from tests import qr_ref as R

DARK, LIGHT, QUIET = 30, 200, 4


def matrix(version, seed=0):
    """The module matrix (1 = dark) of a symbol-like pattern of this version."""
    dim = 17 + 4 * version
    rng = np.random.default_rng(1000 * version + seed)
    m = rng.integers(0, 2, (dim, dim)).astype(np.uint8)
    finder = np.ones((7, 7), np.uint8)
    finder[1:6, 1:6] = 0
    finder[2:5, 2:5] = 1
    for r, c in ((0, 0), (0, dim - 7), (dim - 7, 0)):
        m[max(r - 1, 0):r + 8, max(c - 1, 0):c + 8] = 0  # the separator
        m[r:r + 7, c:c + 7] = finder
    for i in range(8, dim - 8):
        m[6, i] = m[i, 6] = 1 if i % 2 == 0 else 0
    if version >= 2:
        a = dim - 7
        m[a - 2:a + 3, a - 2:a + 3] = 1
        m[a - 1:a + 2, a - 1:a + 2] = 0
        m[a, a] = 1
    if version >= 7:
        word = R.version_codeword(version)
        for i in range(6):
            for j in range(3):
                bit = word >> (3 * i + j) & 1
                m[dim - 11 + j, i] = bit  # what decoder.readVersion reads (decoder.zig:143)
                m[i, dim - 11 + j] = bit  # the transposed copy
    return m


def shift(tx, ty):
    return np.array([[1, 0, tx], [0, 1, ty], [0, 0, 1]], np.float64)


def rotation(degrees, cx, cy):
    """Rotation about (cx, cy), frame coordinates (x right, y down)."""
    a = math.radians(degrees)
    c, s = math.cos(a), math.sin(a)
    return shift(cx, cy) @ np.array([[c, -s, 0], [s, c, 0], [0, 0, 1]], np.float64) @ shift(-cx, -cy)


def apply(h, x, y):
    w = h[2, 0] * x + h[2, 1] * y + h[2, 2]
    return (h[0, 0] * x + h[0, 1] * y + h[0, 2]) / w, (h[1, 0] * x + h[1, 1] * y + h[1, 2]) / w


def render(mat, px, rows, cols, h=None, mirror=False, gradient=0.0, noise=0, seed=0):
    """The matrix at px pixels a module with its quiet zone, its top-left quiet corner at symbol coordinates (0, 0), mapped into the
    frame by h (symbol pixels -> frame pixels; None: the identity). Nearest module at every pixel centre."""
    dim = mat.shape[0]
    h = np.eye(3) if h is None else h
    inv = np.linalg.inv(h)
    ys, xs = np.mgrid[0:rows, 0:cols]
    u, v = apply(inv, xs + 0.5, ys + 0.5)
    mc = np.floor(u / px).astype(np.int64) - QUIET
    mr = np.floor(v / px).astype(np.int64) - QUIET
    if mirror:
        mc = dim - 1 - mc
    inside = (mc >= 0) & (mc < dim) & (mr >= 0) & (mr < dim)
    dark = np.zeros((rows, cols), bool)
    dark[inside] = mat[mr[inside], mc[inside]] == 1
    frame = np.where(dark, float(DARK), float(LIGHT))
    if gradient:
        frame = frame + gradient * (xs / cols - 0.5) * 2
    if noise:
        frame = frame + np.random.default_rng(seed).integers(-noise, noise + 1, (rows, cols))
    return np.clip(np.rint(frame), 0, 255).astype(np.uint8)


def planted_corners(dim, px, h=None, mirror=False):
    """The frame positions of the module-space corners (0, 0), (dim, 0), (0, dim), (dim, dim), as symbolCorners orders them."""
    h = np.eye(3) if h is None else h
    out = []
    for mx, my in ((0, 0), (dim, 0), (0, dim), (dim, dim)):
        if mirror:
            mx = dim - mx
        out.append(apply(h, (mx + QUIET) * px, (my + QUIET) * px))
    return np.array(out, np.float64)


def binarize(frame):
    """A fixed global threshold: the map for binarize mode 2 (a pixel is dark iff its byte is 0)."""
    return np.where(frame > 115, 255, 0).astype(np.uint8)


def side(version, px):
    return (17 + 4 * version + 2 * QUIET) * px


# ---- the frames of tests/test_gpu_qr.py ---------------------------------------------------------------------------------------------
def _axis(version, px=3, rows=None, cols=None, tx=7, ty=5, **kw):
    s = side(version, px)
    return render(matrix(version), px, rows or s + 2 * ty + 1, cols or s + 2 * tx + 4, shift(tx, ty), **kw)


def _rotated(version, degrees, px=3, pad=1.5, **kw):
    s = side(version, px)
    n = int(s * pad) | 1
    return render(matrix(version), px, n, n + 6, rotation(degrees, n / 2 + 3, n / 2) @ shift(n / 2 + 3 - s / 2, n / 2 - s / 2), **kw)


def _perspective(version, px=4):
    s = side(version, px)
    quad = np.array([[s * 0.15, s * 0.10], [s * 1.05, s * 0.04], [s * 0.06, s * 1.03], [s * 1.12, s * 1.10]])
    m = R.projective4([(0, 0), (s, 0), (0, s), (s, s)], [tuple(q) for q in quad])
    return render(matrix(version), px, int(s * 1.22), int(s * 1.25), np.array(m).reshape(3, 3))


def _finder_box(version, px, which, tx, ty):
    """(row0, col0) of the finder pattern `which` (0 TL, 1 TR, 2 BL) in an _axis frame."""
    dim = 17 + 4 * version
    mr, mc = ((0, 0), (0, dim - 7), (dim - 7, 0))[which]
    return ty + (QUIET + mr) * px, tx + (QUIET + mc) * px


def _tall(damaged, px=6, tx=40, ty=52):
    """320 rows, so rows are scanned by residue mod 3 (:89). Damaged: on the rows = 0 mod 3 that cross the core of the top-right finder,
    its left two modules are painted light. No row of the first pass sees that finder's 1:1:3:1:1 any more; the column through its centre,
    the diagonal and (its centre row being 1 mod 3) the row through its centre are untouched, so the later passes confirm it."""
    frame = _axis(2, px, 320, 300, tx, ty)
    if damaged:
        r0, c0 = _finder_box(2, px, 1, tx, ty)
        core = np.arange(r0 + 2 * px, r0 + 5 * px)
        assert (r0 + 3 * px + px // 2) % 3 != 0
        frame[core[core % 3 == 0], c0:c0 + 2 * px] = LIGHT
    return frame


def _tiled(n_rows=8, n_cols=10, px=3, pitch=10):
    """80 bare finder patterns on a lattice, `pitch` modules apart: the 64-entry buffer fills, later hits merge or are dropped, and equal
    sides and right angles make ties in the triple score."""
    finder = np.ones((7, 7), np.uint8)
    finder[1:6, 1:6] = 0
    finder[2:5, 2:5] = 1
    frame = np.full((n_rows * pitch * px + 9, n_cols * pitch * px + 5), LIGHT, np.uint8)
    block = np.kron(finder, np.ones((px, px), np.uint8))
    for i in range(n_rows):
        for j in range(n_cols):
            r, c = 6 + i * pitch * px, 4 + j * pitch * px
            frame[r:r + 7 * px, c:c + 7 * px] = np.where(block == 1, DARK, LIGHT)
    return frame


def _cut(version=2, px=4):
    """Rotated by 45 degrees, so the bottom-right corner of the symbol points down, and cropped just above the centre of the corner
    module: the three finders, the alignment pattern and the timing lines are inside, one module centre is not, and sampleGrid fails."""
    full = _rotated(version, 45, px, pad=1.6)
    s = side(version, px)
    n = full.shape[0]
    h = rotation(45, n / 2 + 3, n / 2) @ shift(n / 2 + 3 - s / 2, n / 2 - s / 2)
    dim = 17 + 4 * version
    _, y = apply(h, (QUIET + dim - 0.5) * px, (QUIET + dim - 0.5) * px)
    return full[:int(y) - 1]


CASES = {
    "v1_axis": lambda: _axis(1),
    "v2_axis": lambda: _axis(2),
    "v7_axis": lambda: _axis(7),
    "v10_axis": lambda: _axis(10),
    "v4_rot37": lambda: _rotated(4, 37),
    "v3_perspective": lambda: _perspective(3),
    "v2_mirrored": lambda: _axis(2, 4, mirror=True),
    "v5_gradient_noise": lambda: _axis(5, 4, gradient=40.0, noise=20, seed=5),
    "frame_96": lambda: _axis(1, 3, 96, 96, 4, 5),
    "frame_21": lambda: _axis(1, 1, 21, 21, -4, -4),
    "frame_20x40": lambda: _axis(1, 1, 20, 40, 0, 0),
    "tall_damaged": lambda: _tall(True),
    "tall_undamaged": lambda: _tall(False),
    "tiled_finders": _tiled,
    "cut_corner": _cut,
    "uncut_corner": lambda: _rotated(2, 45, 4, pad=1.6),
    "all_light": lambda: np.full((64, 70), LIGHT, np.uint8),
    "all_dark": lambda: np.full((64, 70), DARK, np.uint8),
}


@functools.lru_cache(maxsize=None)
def frame(name):
    f = CASES[name]()
    f.setflags(write=False)
    return f


@functools.lru_cache(maxsize=None)
def binary(name):
    b = binarize(frame(name))
    b.setflags(write=False)
    return b


@functools.lru_cache(maxsize=None)
def want(name):
    """The restatement on the case's binary map; shared, not to be changed."""
    return R.detect(binary(name))
