"""The point sets the transform-fitting tests share (tests/test_transform_fit_host.py, tests/test_gpu_transform.py): for every kind and
scalar type at least 300 pairs (from, to) of numpy arrays of shape (n, 2) in that scalar type, built from a fixed seed."""
from __future__ import annotations

import functools

import numpy as np

SIMILARITY, AFFINE, PROJECTIVE = 0, 1, 2
MIN_POINTS = {SIMILARITY: 2, AFFINE: 3, PROJECTIVE: 4}
DTYPES = {0: np.float32, 1: np.float64}


def _similarity_map(rng, reflect=False):
    angle, scale = rng.uniform(-np.pi, np.pi), rng.uniform(0.3, 3.0)
    c, s = np.cos(angle) * scale, np.sin(angle) * scale
    m = np.array([[c, -s], [s, c]])
    if reflect:
        m = m @ np.array([[1.0, 0.0], [0.0, -1.0]])
    return m, rng.uniform(-50, 50, size=2)


def _affine_map(rng):
    return rng.uniform(-2, 2, size=(2, 2)) + np.eye(2), rng.uniform(-50, 50, size=2)


def _homography(rng):
    h = np.eye(3) + rng.uniform(-0.2, 0.2, size=(3, 3))
    h[2, :2] = rng.uniform(-1e-3, 1e-3, size=2)
    h[:2, 2] = rng.uniform(-30, 30, size=2)
    return h


def _apply_h(h, pts):
    q = np.concatenate([pts, np.ones((len(pts), 1))], axis=1) @ h.T
    return q[:, :2] / q[:, 2:3]


def _mapped(rng, kind, pts, reflect=False):
    if kind == PROJECTIVE:
        return _apply_h(_homography(rng), pts)
    m, b = _similarity_map(rng, reflect) if (kind == SIMILARITY or reflect) else _affine_map(rng)
    return pts @ m.T + b


@functools.lru_cache(maxsize=None)
def fit_cases(kind: int, scalar: int):
    """[(name, from, to)]."""
    rng = np.random.default_rng(1000 + 10 * kind + scalar)
    dt = DTYPES[scalar]
    lo = MIN_POINTS[kind]
    out = []

    def add(name, f, t):
        out.append((name, np.ascontiguousarray(f, dt), np.ascontiguousarray(t, dt)))

    for i in range(110):  # random well-conditioned fits: unrelated point clouds
        n = int(rng.integers(lo, lo + 20))
        add("random", rng.uniform(0, 640, size=(n, 2)), rng.uniform(0, 480, size=(n, 2)))
    for i in range(70):  # exact maps of the kind, then the same plus noise
        n = int(rng.integers(lo, lo + 16))
        f = rng.uniform(0, 640, size=(n, 2))
        t = _mapped(rng, kind, f)
        add("exact", f, t)
        if i % 2:
            add("noisy", f, t + rng.normal(0, 0.5, size=t.shape))
    for i in range(30):  # reflections: det(cov) < 0
        n = int(rng.integers(lo, lo + 12))
        f = rng.uniform(-100, 100, size=(n, 2))
        add("reflection", f, _mapped(rng, kind, f, reflect=True))
    for i in range(12):  # duplicated points
        n = int(rng.integers(lo, lo + 10))
        f = rng.uniform(0, 100, size=(n, 2))
        f[1:1 + n // 2] = f[0]
        add("duplicated", f, _mapped(rng, kind, f))
    for i in range(10):  # all-equal points on one side or both
        n = int(rng.integers(lo, lo + 6))
        same = np.tile(rng.uniform(0, 100, size=(1, 2)), (n, 1))
        other = rng.uniform(0, 100, size=(n, 2))
        add("all_equal", same, other if i % 3 else same)
        if i % 2:
            add("all_equal_to", other, same)
    for i in range(24):  # collinear sets: exactly (integers on a line) and nearly
        n = int(rng.integers(lo, lo + 8))
        k = rng.permutation(np.arange(-n, n))[:n].astype(np.float64)
        line = np.stack([3.0 + 2.0 * k, 7.0 - 5.0 * k], axis=1)
        other = rng.uniform(0, 100, size=(n, 2))
        which = i % 4
        if which == 0:
            add("collinear_from", line, other)
        elif which == 1:
            add("collinear_to", other, line)
        elif which == 2:
            add("collinear_both", line, line[::-1])
        else:
            add("nearly_collinear", line + rng.normal(0, 1e-7, size=line.shape), other)
    for i in range(30):  # N at the minimum; every third in small coordinates, where the f32 8 x 8 system clears SMatrix.solve's tolerance
        f = rng.uniform(0, 640 if i % 3 else 4, size=(lo, 2))
        add("minimum", f, _mapped(rng, kind, f) if i % 2 else rng.uniform(0, 480, size=(lo, 2)))
    for i in range(20):  # tiny and huge coordinates: f32 products fall under the normal range, resp. lose every fraction
        n = int(rng.integers(lo, lo + 10))
        f = rng.uniform(1, 640, size=(n, 2))
        t = _mapped(rng, kind, f) + rng.normal(0, 0.5, size=(n, 2))
        add("scale_1e-20", f * 1e-20, t * 1e-20)
        add("scale_1e+15", f * 1e15, t * 1e15)
        if i % 4 == 0:
            add("scale_mixed", f * 1e-20, t * 1e15)
    if kind == AFFINE:  # either side of Matrix.gemm's 512 multiply-adds
        for n in (85, 86, 85, 86):
            f = rng.uniform(0, 640, size=(n, 2))
            add("gemm_threshold_%d" % n, f, _mapped(rng, kind, f) + rng.normal(0, 0.5, size=(n, 2)))
    assert len(out) >= 300, len(out)
    return out


def cloud(kind: int, scalar: int, n: int, seed: int = 0):
    """n points and their image under a map of the kind plus half a pixel of noise: the device-versus-host sizes."""
    rng = np.random.default_rng(77 + 1000 * kind + 10 * scalar + seed)
    f = rng.uniform(0, 640, size=(n, 2))
    t = _mapped(rng, kind, f) + rng.normal(0, 0.5, size=(n, 2))
    dt = DTYPES[scalar]
    return np.ascontiguousarray(f, dt), np.ascontiguousarray(t, dt)
