"""Inputs the feature-distribution-matching tests share: the covariance families of the solve tests (host program and device kernels) and
the frames of the end-to-end tests. Everything is generated from fixed seeds; only exact_statistics calls the library (host arithmetic)."""
from __future__ import annotations

import numpy as np


def _sym(c):
    c = np.asarray(c, np.float64)
    return (c + c.T) / 2.0


def _rotation(rng):
    q, r = np.linalg.qr(rng.normal(size=(3, 3)))
    return q * np.sign(np.diag(r))


def covariance_matrices(seed: int = 20):
    """(family, 3 x 3 symmetric f64) over: random SPD, rank-deficient, zero, diagonal, nearly equal singular values."""
    rng = np.random.default_rng(seed)
    out = []
    for _ in range(120):
        a = rng.normal(size=(3, 3)) * rng.uniform(0.01, 0.3)
        out.append(("spd", _sym(a @ a.T)))
    for _ in range(30):
        a = rng.normal(size=(3, 2)) * 0.2
        out.append(("rank2", _sym(a @ a.T)))
    for _ in range(30):
        v = rng.normal(size=(3, 1)) * 0.2
        out.append(("rank1", _sym(v @ v.T)))
    for k in range(3):  # one channel only, and two equal channels
        d = np.zeros((3, 3))
        d[k, k] = 0.04
        out.append(("rank1", d))
        e = np.full((3, 3), 0.0)
        i, j = [x for x in range(3) if x != k]
        e[i, i] = e[j, j] = e[i, j] = e[j, i] = 0.02
        out.append(("rank1", e))
    out.append(("rank1", np.full((3, 3), 0.03)))  # a grey frame's covariance
    out.append(("zero", np.zeros((3, 3))))
    for _ in range(30):
        out.append(("diagonal", np.diag(rng.uniform(0.0, 0.25, size=3))))
    out.append(("diagonal", np.diag([0.1, 0.1, 0.1])))
    out.append(("diagonal", np.diag([0.1, 0.0, 0.2])))
    out.append(("diagonal", np.diag([1e-11, 1e-9, 1e-3])))  # both sides of the 1e-10 guard
    for k in range(3, 17):
        for _ in range(4):
            q = _rotation(rng)
            s = rng.uniform(0.01, 0.2)
            d = np.diag([s, s * (1.0 + 10.0 ** -k), s * (1.0 + 2.0 * 10.0 ** -k)])
            out.append(("near_equal", _sym(q @ d @ q.T)))
    return out


def solve_cases(seed: int = 21):
    """(pixel, target_is_gray, tmean[3], tcov 3x3, smean[3], scov 3x3): every matrix above as a source against a rotating choice of targets,
    on the colour route, and a share of them on the two scalar routes (where only mean[0] and cov[0][0] count)."""
    rng = np.random.default_rng(seed)
    mats = covariance_matrices()
    cases = []
    for i, (_, scov) in enumerate(mats):
        _, tcov = mats[(i * 7 + 3) % len(mats)]
        tmean, smean = rng.uniform(0.0, 1.0, size=3), rng.uniform(0.0, 1.0, size=3)
        cases.append((2, 0, tmean, tcov, smean, scov))
        if i % 5 == 0:
            cases.append((0, 1, tmean, tcov, smean, scov))
            cases.append((3, 1, tmean, tcov, smean, scov))
    return cases


def correlated_rgb(rng, rows, cols, mix=None, base=(110, 120, 100), spread=38.0):
    """A random frame whose channels are correlated: three noise planes through a mixing matrix, around a base colour."""
    if mix is None:
        mix = rng.uniform(-1.0, 1.0, size=(3, 3))
    z = rng.normal(size=(rows, cols, 3))
    v = z @ mix.T * spread + np.asarray(base, np.float64)
    return np.clip(np.rint(v), 0, 255).astype(np.uint8)


def moments_for(cov, n=1000, s=128000):
    """Integer moments (n, sum[3], prod[6]) whose covariance (n Sxy - Sx Sy) / (65025 n (n - 1)) is about `cov`: every channel sum is s."""
    prod = []
    for i in range(3):
        for j in range(i, 3):
            prod.append(max(0, int(round(s * s / n + float(cov[i][j]) * 65025.0 * (n - 1)))))
    return n, [s, s, s], prod


def end_to_end_cases(seed: int = 3):
    """(name, source, target) frames of the end-to-end tests: colour to colour, u8 to u8, a colour source against a grey colour target, a
    constant source (the 1e-10 guard's scale = 1 and W = 0 sides), source equal to target, 1 x 1 frames."""
    rng = np.random.default_rng(seed)
    rgb_a = correlated_rgb(rng, 64, 64)
    rgb_b = correlated_rgb(rng, 40, 56, base=(90, 140, 70), spread=30.0)
    rgba_a = np.dstack([correlated_rgb(rng, 37, 53), rng.integers(0, 256, size=(37, 53, 1), dtype=np.uint8)])
    rgba_b = np.dstack([correlated_rgb(rng, 21, 30, base=(150, 100, 120)), rng.integers(0, 256, size=(21, 30, 1), dtype=np.uint8)])
    u8_a = np.clip(np.rint(rng.normal(120.0, 30.0, size=(64, 64))), 0, 255).astype(np.uint8)
    u8_b = np.clip(np.rint(rng.normal(90.0, 45.0, size=(37, 53))), 0, 255).astype(np.uint8)
    gray_plane = np.clip(np.rint(rng.normal(140.0, 35.0, size=(30, 44))), 0, 255).astype(np.uint8)
    gray_rgb = np.repeat(gray_plane[..., None], 3, axis=2)
    gray_rgba = np.dstack([gray_rgb, rng.integers(0, 256, size=(30, 44, 1), dtype=np.uint8)])
    const_rgb = np.empty((16, 20, 3), np.uint8)
    const_rgb[...] = (40, 90, 200)
    return [
        ("rgb_to_rgb", rgb_a, rgb_b),
        ("rgba_to_rgba", rgba_a, rgba_b),
        ("u8_to_u8", u8_a, u8_b),
        ("rgb_gray_target", rgb_a, gray_rgb),
        ("rgba_gray_target", rgba_a, gray_rgba),
        ("constant_rgb_source", const_rgb, rgb_b),
        ("constant_u8_source", np.full((9, 31), 77, np.uint8), u8_b),
        ("rgb_source_is_target", rgb_b, rgb_b),
        ("u8_source_is_target", u8_b, u8_b),
        ("rgb_1x1", rgb_a[:1, :1].copy(), rgb_b[:1, :1].copy()),
        ("u8_1x1", u8_a[:1, :1].copy(), u8_b[:1, :1].copy()),
        ("rgb_1x1_source", rgb_a[2:3, 5:6].copy(), rgb_b),
    ]


def exact_statistics(img, luminance: bool = False):
    """(mean[3], cov[3][3]) from the frame's integer moments as the device derives them: zg_fdm_stats_from_moments_host, host arithmetic of
    the library, no GPU. luminance: those of the byte (u8) or of the luminance byte, three times over."""
    from tests import fdm_ref as R
    from zignal_amd import _lib as L
    from zignal_amd import fdm
    m = R.moments(img)
    rec = L.ZgFdmMoments()
    rec.n = m["n"]
    for i in range(3):
        rec.sum[i] = m["sum"][i]
    for i in range(6):
        rec.prod[i] = m["prod"][i]
    rec.lum_sum, rec.lum_sq, rec.not_gray = m["lum_sum"], m["lum_sq"], m["not_gray"]
    mean, cov = fdm.stats_from_moments(rec, luminance or img.ndim == 2)
    return list(mean), cov.tolist()


def match_with_exact_statistics(src, tgt, return_pre: bool = False):
    """tests/fdm_ref.py's match with the statistics above in place of Welford's: what the device is expected to compute."""
    from tests import fdm_ref as R
    gray = R.is_gray(tgt)
    target = R.make_target(*exact_statistics(tgt), gray)
    return R.apply(src, R.make_transform(src.ndim == 2, target, *exact_statistics(src, gray)), return_pre)
