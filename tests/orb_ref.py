"""Two independent CPU restatements of Orb.detectAndCompute / Orb.compute (reference src/features/orb.zig:119-276, 336-517), the
checker of zg.Orb.

detect_and_compute_literal walks the reference's loops keypoint by keypoint and tap by tap (slow: small images);
detect_and_compute_fast holds arrays across the keypoints and loops over the 961 taps and 256 pairs, which keeps every sum's order,
and handles a 4096^2 frame. Both stand on oracle.pyramid, fast_ref.detect_fast and the oracle's zo_powf / zo_sinf / zo_cosf /
zo_atan2f / zo_expf, do every f32 step as np.float32, and return (keypoints, descriptors, counters): KEYPOINT_DTYPE and
BINARY_DESCRIPTOR_DTYPE arrays in the reference's order and the coverage counters of COUNTERS.
"""
import ctypes as C
import hashlib

import numpy as np

from oracle import pyoracle as oracle
from tests import fast_ref as F
from zignal_amd import BINARY_DESCRIPTOR_DTYPE, KEYPOINT_DTYPE

f32 = np.float32
PATCH, HALF = 31, 15  # DEFAULT_PATCH_SIZE (:15)
DEG = f32(180.0 / np.pi)  # radiansToDegrees: ang * f32(180 / pi)
RAD = f32(np.pi / 180.0)  # degreesToRadians: ang * f32(pi / 180)
COUNTERS = ("sorted_levels", "unsorted_levels", "ties_at_cut", "margin_dropped", "bounds_checked", "oob_bits", "m00_small")

# The 256 sampling pairs of the ORB descriptor (Rublee et al. 2011): x1, y1, x2, y2 per pair, 8 pairs a line.
PAIRS = np.array([
      8,  -3,   9,   5,   4,   2,   7, -12, -11,   9,  -8,   2,   7, -12,  12, -13,   2, -13,   2,  12,   1,  -7,   1,   6,  -2, -10,  -2,  -4, -13, -13, -11,  -8,
    -13,  -3, -12,  -9,  10,   4,  11,   9, -13,  -8,  -8,  -9, -11,   7,  -9,  12,   7,   7,  12,   6,  -4,  -5,  -3,   0, -13,   2, -12,  -3,  -9,   0,  -7,   5,
     12,  -6,  12,  -1,  -3,   6,  -2,  12,  -6, -13,  -4,  -8,  11, -13,  12,  -8,   4,   7,   5,   1,   5,  -3,  10,  -3,   3,  -7,   6,  12,  -8,  -7,  -6,  -2,
     -2,  11,  -1, -10, -13,  12,  -8,  10,  -7,   3,  -5,  -3,  -4,   2,  -3,   7, -10, -12,  -6,  11,   5, -12,   6,  -7,   5,  -6,   7,  -1,   1,   0,   4,  -5,
      9,  11,  11, -13,   4,   7,   4,  12,   2,  -1,   4,   4,  -4, -12,  -2,   7,  -8,  -5,  -7, -10,   4,  11,   9,  12,   0,  -8,   1, -13, -13,  -2,  -8,   2,
     -3,  -2,  -2,   3,  -6,   9,  -4,  -9,   8,  12,  10,   7,   0,   9,   1,   3,   7,  -5,  11, -10, -13,  -6, -11,   0,  10,   7,  12,   1,  -6,  -3,  -6,  12,
     10,  -9,  12,  -4, -13,   8,  -8, -12, -13,   0,  -8,  -4,   3,   3,   7,   8,   5,   7,  10,  -7,  -1,   7,   1, -12,   3, -10,   5,   6,   2,  -4,   3, -10,
    -13,   0, -13,   5, -13,  -7, -12,  12, -13,   3, -11,   8,  -7,  12,  -4,   7,   6, -10,  12,   8,  -9,  -1,  -7,  -6,  -2,  -5,   0,  12, -12,   5,  -7,   5,
      3, -10,   8, -13,  -7,  -7,  -4,   5,  -3,  -2,  -1,  -7,   2,   9,   5, -11, -11, -13,  -5, -13,  -1,   6,   0,  -1,   5,  -3,   5,   2,  -4, -13,  -4,  12,
     -9,  -6,  -9,   6, -12, -10,  -8,  -4,  10,   2,  12,  -3,   7,  12,  12,  12,  -7, -13,  -6,   5,  -4,   9,  -3,   4,   7,  -1,  12,   2,  -7,   6,  -5,   1,
    -13,  11, -12,   5,  -3,   7,  -2,  -6,   7,  -8,  12,  -7, -13,  -7, -11, -12,   1,  -3,  12,  12,   2,  -6,   3,   0,  -4,   3,  -2, -13,  -1, -13,   1,   9,
      7,   1,   8,  -6,   1,  -1,   3,  12,   9,   1,  12,   6,  -1,  -9,  -1,   3, -13, -13, -10,   5,   7,   7,  10,  12,  12,  -5,  12,   9,   6,   3,   7,  11,
      5, -13,   6,  10,   2, -12,   2,   3,   3,   8,   4,  -6,   2,   6,  12, -13,   9, -12,  10,   3,  -8,   4,  -7,   9, -11,  12,  -4,  -6,   1,  12,   2,  -8,
      6,  -9,   7,  -4,   2,   3,   3,  -2,   6,   3,  11,   0,   3,  -3,   8,  -8,   7,   8,   9,   3, -11,  -5,  -6,  -4, -10,  11,  -5,  10,  -5,  -8,  -3,  12,
    -10,   5,  -9,   0,   8,  -1,  12,  -6,   4,  -6,   6, -11, -10,  12,  -8,   7,   4,  -2,   6,   7,  -2,   0,  -2,  12,  -5,  -8,  -5,   2,   7,  -6,  10,  12,
     -9, -13,  -8,  -8,  -5, -13,  -5,  -2,   8,  -8,   9, -13,  -9, -11,  -9,   0,   1,  -8,   1,  -2,   7,  -4,   9,   1,  -2,   1,  -1,  -4,  11,  -6,  12, -11,
    -12,  -9,  -6,   4,   3,   7,   7,  12,   5,   5,  10,   8,   0,  -4,   2,   8,  -9,  12,  -5, -13,   0,   7,   2,  12,  -1,   2,   1,   7,   5,  11,   7,  -9,
      3,   5,   6,  -8, -13,  -4,  -8,   9,  -5,   9,  -3,  -3,  -4,  -7,  -3, -12,   6,   5,   8,   0,  -7,   6,  -6,  12, -13,   6,  -5,  -2,   1, -10,   3,  10,
      4,   1,   8,  -4,  -2,  -2,   2, -13,   2, -12,  12,  12,  -2, -13,   0,  -6,   4,   1,   9,   3,  -6, -10,  -3,  -5,  -3, -13,  -1,   1,   7,   5,  12, -11,
      4,  -2,   5,  -7, -13,   9,  -9,  -5,   7,   1,   8,   6,   7,  -8,   7,   6,  -7,  -4,  -7,   1,  -8,  11,  -7,  -8, -13,   6, -12,  -8,   2,   4,   3,   9,
     10,  -5,  12,   3,  -6,  -5,  -6,   7,   8,  -3,   9,  -8,   2, -12,   2,   8, -11,  -2, -10,   3, -12, -13,  -7,  -9, -11,   0, -10,  -5,   5,  -3,  11,   8,
     -2, -13,  -1,  12,  -1,  -8,   0,   9, -13, -11, -12,  -5, -10,  -2, -10,  11,  -3,   9,  -2, -13,   2,  -3,   3,   2,  -9, -13,  -4,   0,  -4,   6,  -3, -10,
     -4,  12,  -2,  -7,  -6, -11,  -4,   9,   6,  -3,   6,  11, -13,  11,  -5,   5,  11,  11,  12,   6,   7,  -5,  12,  -2,  -1,  12,   0,   7,  -4,  -8,  -3,  -2,
     -7,   1,  -6,   7, -13, -12,  -8, -13,  -7,  -2,  -6,  -8,  -8,   5,  -6,  -9,  -5,  -1,  -4,   5, -13,   7,  -8,  10,   1,   5,   5, -13,   1,   0,  10, -13,
      9,  12,  10,  -1,   5,  -8,  10,  -9,  -1,  11,   1, -13,  -9,  -3,  -6,   2,  -1, -10,   1,  12, -13,   1,  -8, -10,   8, -11,  10,  -6,   2, -13,   3,  -6,
      7, -13,  12,  -9, -10, -10,  -5,  -7, -10,  -8,  -8, -13,   4,  -6,   8,   5,   3,  12,   8, -13,  -4,   2,  -3,  -3,   5, -13,  10, -12,   4, -13,   5,  -1,
     -9,   9,  -4,   3,   0,   3,   3,  -9, -12,   1,  -6,   1,   3,   2,   4,  -8, -10, -10, -10,   9,   8, -13,  12,  12,  -8, -12,  -6,  -5,   2,   2,   3,   7,
     10,   6,  11,  -8,   6,   8,   8, -12,  -7,  10,  -6,   5,  -3,  -9,  -3,   9,  -1, -13,  -1,   5,  -3,  -7,  -3,   4,  -8,  -2,  -8,   3,   4,   2,  12,  12,
      2,  -5,   3,  11,   6,  -9,  11, -13,   3,  -1,   7,  12,  11,  -1,  12,   4,  -3,   0,  -3,   6,   4, -11,   4,  12,   2,  -4,   2,   1, -10,  -6,  -8,   1,
    -13,   7, -11,   1, -13,  12, -11, -13,   6,   0,  11, -13,   0,  -1,   1,   4, -13,   3,  -9,  -2,  -9,   8,  -6,  -3, -13,  -6,  -8,  -2,   5,  -9,   8,  10,
      2,   7,   3,  -9,  -1,  -6,  -1,  -1,   9,   5,  11,  -2,  11,  -3,  12,  -8,   3,   0,   3,   5,  -1,   4,   0,  10,   3,  -6,   4,   5, -13,   0, -10,   5,
      5,   8,  12,  11,   8,   9,   9,  -6,   7,  -4,   8, -12, -10,   4, -10,   9,   7,   3,  12,   4,   9,  -7,  10,  -2,   7,   0,  12,  -2,  -1,  -6,   0, -11,
], np.int8).reshape(256, 4)
PAIRS_SHA256 = "2164181aea6ff9ac426ca512d5130d15e1f6e3cd47b1cbdd568bbe1e55d49023"


def pairs_sha256() -> str:
    return hashlib.sha256(PAIRS.tobytes()).hexdigest()


def _lib():
    l = oracle.lib()
    l.zo_atan2f.restype = C.c_float
    l.zo_atan2f.argtypes = [C.c_float, C.c_float]
    return l


def powf(x, y) -> np.float32:
    return f32(_lib().zo_powf(C.c_float(x), C.c_float(y)))


def atan2f(y, x) -> np.float32:
    return f32(_lib().zo_atan2f(C.c_float(y), C.c_float(x)))


def sinf(x) -> np.float32:
    return f32(_lib().zo_sinf(C.c_float(x)))


def cosf(x) -> np.float32:
    return f32(_lib().zo_cosf(C.c_float(x)))


def expf(x) -> np.float32:
    return f32(_lib().zo_expf(C.c_float(x)))


def round_away(v):
    """@round: halves away from zero (exact in f64 for the magnitudes here)."""
    v = np.asarray(v, np.float64)
    return np.sign(v) * np.floor(np.abs(v) + 0.5)


_weights = None


def orientation_weights() -> np.ndarray:
    """orientation_weights (:340-357): exp(-d^2 / (225 / 2)) inside d^2 <= 225, 0 outside; 961 floats."""
    global _weights
    if _weights is None:
        w = np.zeros(PATCH * PATCH, f32)
        radius_sq = f32(HALF * HALF)
        denom = radius_sq / f32(2.0)
        for v in range(PATCH):
            for u in range(PATCH):
                dist_sq = f32((u - HALF) ** 2 + (v - HALF) ** 2)
                if dist_sq <= radius_sq:
                    w[v * PATCH + u] = expf(-dist_sq / denom)
        _weights = w
    return _weights.copy()


class Params:
    """Orb's fields and defaults (:87-109)."""

    def __init__(self, n_features=500, scale_factor=1.2, n_levels=8, edge_threshold=15, first_level=0, fast_threshold=20, harris=False,
                 weights=None):
        self.n_features, self.scale_factor, self.n_levels = int(n_features), f32(scale_factor), int(n_levels)
        self.edge_threshold, self.first_level, self.fast_threshold, self.harris = int(edge_threshold), int(first_level), int(fast_threshold), bool(harris)
        self.weights = orientation_weights() if weights is None else np.asarray(weights, f32).reshape(-1)

    def kwargs(self):
        """The arguments of zg.Orb for the same detector."""
        return dict(n_features=self.n_features, scale_factor=float(self.scale_factor), n_levels=self.n_levels, edge_threshold=self.edge_threshold,
                    first_level=self.first_level, fast_threshold=self.fast_threshold, score_type="harris_score" if self.harris else "fast_score")


def features_per_level(p: Params):
    """computeFeaturesPerLevel (:279-334), left to right in f32."""
    nl, nf = p.n_levels, p.n_features
    if nl == 1 or p.scale_factor <= f32(1.0):
        base, rem = (nf // nl, nf % nl) if nl else (0, 0)
        return [base + (1 if l < rem else 0) for l in range(nl)]
    factor = f32(1.0) / p.scale_factor
    factor_to_n = powf(factor, f32(nl))
    out, assigned = [], 0
    for level in range(nl):
        remaining = nf - assigned if assigned < nf else 0
        if level == nl - 1 or remaining == 0:
            out.append(remaining)
            assigned += remaining
            continue
        level_factor = powf(factor, f32(level))
        desired = f32(f32(f32(f32(nf) * f32(f32(1.0) - factor)) / f32(f32(1.0) - factor_to_n)) * level_factor)
        clamped = min(int(round_away(desired)), remaining)
        base_min = max(10, nf // (nl * 3))
        min_features = min(remaining, base_min)
        out.append(min_features if clamped < min_features else clamped)
        assigned += out[-1]
    return out


def adaptive_threshold(p: Params, level: int) -> int:
    """computeAdaptiveThreshold (:511-517)."""
    level_scale = powf(p.scale_factor, f32(level))
    attenuation = f32(1.0) / level_scale
    v = f32(f32(p.fast_threshold) * attenuation)
    v = min(max(v, f32(5.0)), f32(255.0))
    return int(round_away(v))


def _pyramid(img, p: Params):
    levels = oracle.pyramid(np.ascontiguousarray(img), p.n_levels, float(p.scale_factor), 1.6)
    assert len(levels) == p.n_levels, "the pyramid stops before n_levels: the reference indexes past its end"
    return levels


def _margin(p: Params, scale):
    return max(f32(3.0), f32(f32(p.edge_threshold) / scale))


# ---- loop for loop --------------------------------------------------------------------------------------------------
def _harris_literal(img, x, y):
    rows, cols = img.shape
    ixx = iyy = ixy = f32(0)
    for dy in range(7):
        yy = y + dy - 3
        if yy <= 0 or yy >= rows - 1:
            continue
        for dx in range(7):
            xx = x + dx - 3
            if xx <= 0 or xx >= cols - 1:
                continue
            a = lambda r, c: int(img[r, c])  # noqa: E731
            gx = a(yy - 1, xx + 1) - a(yy - 1, xx - 1) + 2 * (a(yy, xx + 1) - a(yy, xx - 1)) + a(yy + 1, xx + 1) - a(yy + 1, xx - 1)
            gy = a(yy + 1, xx - 1) - a(yy - 1, xx - 1) + 2 * (a(yy + 1, xx) - a(yy - 1, xx)) + a(yy + 1, xx + 1) - a(yy - 1, xx + 1)
            fx, fy = f32(gx) / f32(8.0), f32(gy) / f32(8.0)
            ixx = f32(ixx + f32(fx * fx))
            iyy = f32(iyy + f32(fy * fy))
            ixy = f32(ixy + f32(fx * fy))
    det = f32(f32(ixx * iyy) - f32(ixy * ixy))
    trace = f32(ixx + iyy)
    return f32(det - f32(f32(f32(0.04) * trace) * trace))


def _orientation_literal(img, x, y, w, counters):
    rows, cols = img.shape
    safe = HALF <= x < cols - HALF and HALF <= y < rows - HALF
    if not safe:
        counters["bounds_checked"] += 1
    m00 = m10 = m01 = f32(0)
    for v in range(PATCH):
        dy = v - HALF
        py = y + dy
        if not safe and (py < 0 or py >= rows):
            continue
        for u in range(PATCH):
            dx = u - HALF
            px = x + dx
            if not safe and (px < 0 or px >= cols):
                continue
            intensity = f32(f32(img[py, px]) * w[v * PATCH + u])
            m00 = f32(m00 + intensity)
            m10 = f32(m10 + f32(intensity * f32(dx)))
            m01 = f32(m01 + f32(intensity * f32(dy)))
    if m00 < f32(0.001):
        counters["m00_small"] += 1
        return f32(0)
    return f32(atan2f(f32(m01 / m00), f32(m10 / m00)) * DEG)


def _descriptor_literal(img, kx, ky, angle, counters):
    rows, cols = img.shape
    rad = f32(angle * RAD)
    c, s = cosf(rad), sinf(rad)
    bits = np.zeros(32, np.uint8)
    for i in range(256):
        x1, y1, x2, y2 = (f32(v) for v in PAIRS[i])
        rx1, ry1 = f32(f32(c * x1) - f32(s * y1)), f32(f32(s * x1) + f32(c * y1))
        rx2, ry2 = f32(f32(c * x2) - f32(s * y2)), f32(f32(s * x2) + f32(c * y2))
        pts = []
        for ry, rx in ((ry1, rx1), (ry2, rx2)):
            r, cc = int(round_away(f32(ky + ry))), int(round_away(f32(kx + rx)))
            if r < 0 or cc < 0 or r >= rows or cc >= cols:
                break
            pts.append(int(img[r, cc]))
        if len(pts) < 2:
            counters["oob_bits"] += 1
            continue
        if pts[0] < pts[1]:
            bits[i // 8] |= 1 << (i % 8)
    return bits


def compute_literal(img, keypoints, p: Params = None, counters=None, levels=None):
    """Orb.compute (:133-144, 224-247)."""
    p = p or Params()
    counters = counters if counters is not None else dict.fromkeys(COUNTERS, 0)
    levels = levels or _pyramid(img, p)
    out = np.zeros(len(keypoints), BINARY_DESCRIPTOR_DTYPE)
    for i, kp in enumerate(keypoints):
        level = min(max(0, int(kp["octave"])), p.n_levels - 1)
        scale = powf(p.scale_factor, f32(level))
        out["bits"][i] = _descriptor_literal(levels[level], f32(kp["x"] / scale), f32(kp["y"] / scale), f32(kp["angle"]), counters)
    return out


def detect_and_compute_literal(img, p: Params = None):
    p = p or Params()
    counters = dict.fromkeys(COUNTERS, 0)
    levels = _pyramid(img, p)
    shares = features_per_level(p)
    kept = []
    for level in range(p.n_levels):
        if level < p.first_level or shares[level] == 0:
            continue
        lim = levels[level]
        corners = F.detect_fast(lim, adaptive_threshold(p, level), 9, True)
        if p.harris:
            for k in corners:
                k["response"] = _harris_literal(lim, int(k["x"]), int(k["y"]))
        chosen = list(range(len(corners)))
        if len(corners) > shares[level]:
            counters["sorted_levels"] += 1
            chosen = sorted(chosen, key=lambda i: -float(corners["response"][i]))  # stable (std.mem.sort)
            if corners["response"][chosen[shares[level] - 1]] == corners["response"][chosen[shares[level]]]:
                counters["ties_at_cut"] += 1
            chosen = chosen[: shares[level]]
        else:
            counters["unsorted_levels"] += 1
        scale = powf(p.scale_factor, f32(level))
        margin = _margin(p, scale)
        rows, cols = lim.shape
        for i in chosen:
            kp = corners[i].copy()
            if kp["x"] < margin or kp["x"] >= f32(cols) - margin or kp["y"] < margin or kp["y"] >= f32(rows) - margin:
                counters["margin_dropped"] += 1
                continue
            kp["angle"] = _orientation_literal(lim, int(kp["x"]), int(kp["y"]), p.weights, counters)
            kp["octave"] = level
            kp["x"] = f32(kp["x"] * scale)
            kp["y"] = f32(kp["y"] * scale)
            kp["size"] = f32(kp["size"] * scale)
            kept.append(kp)
    kps = np.array(kept, KEYPOINT_DTYPE) if kept else np.zeros(0, KEYPOINT_DTYPE)
    return kps, compute_literal(img, kps, p, counters, levels), counters


# ---- arrays across the keypoints ----------------------------------------------------------------------------------------
def _harris_fast(img, xs, ys):
    rows, cols = img.shape
    im = img.astype(np.int32)
    ixx = np.zeros(len(xs), f32)
    iyy = np.zeros(len(xs), f32)
    ixy = np.zeros(len(xs), f32)
    for dy in range(7):
        yy = ys + (dy - 3)
        oky = (yy > 0) & (yy < rows - 1)
        yc = np.clip(yy, 1, rows - 2)
        for dx in range(7):
            xx = xs + (dx - 3)
            ok = oky & (xx > 0) & (xx < cols - 1)
            xc = np.clip(xx, 1, cols - 2)
            gx = im[yc - 1, xc + 1] - im[yc - 1, xc - 1] + 2 * (im[yc, xc + 1] - im[yc, xc - 1]) + im[yc + 1, xc + 1] - im[yc + 1, xc - 1]
            gy = im[yc + 1, xc - 1] - im[yc - 1, xc - 1] + 2 * (im[yc + 1, xc] - im[yc - 1, xc]) + im[yc + 1, xc + 1] - im[yc - 1, xc + 1]
            fx, fy = gx.astype(f32) / f32(8.0), gy.astype(f32) / f32(8.0)
            ixx = np.where(ok, ixx + fx * fx, ixx)
            iyy = np.where(ok, iyy + fy * fy, iyy)
            ixy = np.where(ok, ixy + fx * fy, ixy)
    det = ixx * iyy - ixy * ixy
    trace = ixx + iyy
    return (det - (f32(0.04) * trace) * trace).astype(f32)


def _orientation_fast(img, xs, ys, w, counters):
    rows, cols = img.shape
    n = len(xs)
    safe = (xs >= HALF) & (xs < cols - HALF) & (ys >= HALF) & (ys < rows - HALF)
    counters["bounds_checked"] += int((~safe).sum())
    m00 = np.zeros(n, f32)
    m10 = np.zeros(n, f32)
    m01 = np.zeros(n, f32)
    for v in range(PATCH):
        dy = v - HALF
        py = ys + dy
        oky = (py >= 0) & (py < rows)
        pyc = np.clip(py, 0, rows - 1)
        for u in range(PATCH):
            dx = u - HALF
            px = xs + dx
            ok = oky & (px >= 0) & (px < cols)
            intensity = img[pyc, np.clip(px, 0, cols - 1)].astype(f32) * w[v * PATCH + u]
            m00 = np.where(ok, m00 + intensity, m00)
            m10 = np.where(ok, m10 + intensity * f32(dx), m10)
            m01 = np.where(ok, m01 + intensity * f32(dy), m01)
    small = m00 < f32(0.001)
    counters["m00_small"] += int(small.sum())
    angles = np.zeros(n, f32)
    with np.errstate(divide="ignore", invalid="ignore"):
        qy, qx = m01 / m00, m10 / m00
    for i in np.nonzero(~small)[0]:
        angles[i] = f32(atan2f(qy[i], qx[i]) * DEG)
    return angles


def _descriptors_fast(img, kx, ky, angles, counters):
    rows, cols = img.shape
    n = len(kx)
    rad = (angles * RAD).astype(f32)
    c = np.array([cosf(r) for r in rad], f32)
    s = np.array([sinf(r) for r in rad], f32)
    bits = np.zeros((n, 32), np.uint8)
    for i in range(256):
        x1, y1, x2, y2 = (f32(v) for v in PAIRS[i])
        vals, ok = [], np.ones(n, bool)
        for x, y in ((x1, y1), (x2, y2)):
            rx = c * x - s * y
            ry = s * x + c * y
            r = round_away(ky + ry).astype(np.int64)
            cc = round_away(kx + rx).astype(np.int64)
            ok &= (r >= 0) & (cc >= 0) & (r < rows) & (cc < cols)
            vals.append(img[np.clip(r, 0, rows - 1), np.clip(cc, 0, cols - 1)])
        counters["oob_bits"] += int((~ok).sum())
        bits[:, i // 8] |= ((ok & (vals[0] < vals[1])).astype(np.uint8) << np.uint8(i % 8))
    return bits


def compute_fast(img, keypoints, p: Params = None, counters=None, levels=None):
    """Orb.compute (:133-144, 224-247)."""
    p = p or Params()
    counters = counters if counters is not None else dict.fromkeys(COUNTERS, 0)
    levels = levels or _pyramid(img, p)
    out = np.zeros(len(keypoints), BINARY_DESCRIPTOR_DTYPE)
    lv = np.minimum(np.maximum(0, keypoints["octave"].astype(np.int64)), p.n_levels - 1)
    for level in np.unique(lv):
        idx = np.nonzero(lv == level)[0]
        scale = powf(p.scale_factor, f32(level))
        k = keypoints[idx]
        out["bits"][idx] = _descriptors_fast(levels[level], (k["x"] / scale).astype(f32), (k["y"] / scale).astype(f32), k["angle"].astype(f32), counters)
    return out


def detect_and_compute_fast(img, p: Params = None):
    p = p or Params()
    counters = dict.fromkeys(COUNTERS, 0)
    levels = _pyramid(img, p)
    shares = features_per_level(p)
    parts = []
    for level in range(p.n_levels):
        if level < p.first_level or shares[level] == 0:
            continue
        lim = levels[level]
        rows, cols = lim.shape
        corners = F.detect_fast(lim, adaptive_threshold(p, level), 9, True)
        xs, ys = corners["x"].astype(np.int64), corners["y"].astype(np.int64)
        if p.harris and len(corners):
            corners["response"] = _harris_fast(lim, xs, ys)
        nd = shares[level]
        if len(corners) > nd:
            counters["sorted_levels"] += 1
            order = np.argsort(-corners["response"], kind="stable")
            counters["ties_at_cut"] += int(corners["response"][order[nd - 1]] == corners["response"][order[nd]])
            corners = corners[order[:nd]]
        else:
            counters["unsorted_levels"] += 1
        scale = powf(p.scale_factor, f32(level))
        margin = _margin(p, scale)
        drop = (corners["x"] < margin) | (corners["x"] >= f32(cols) - margin) | (corners["y"] < margin) | (corners["y"] >= f32(rows) - margin)
        counters["margin_dropped"] += int(drop.sum())
        k = corners[~drop].copy()
        k["angle"] = _orientation_fast(lim, k["x"].astype(np.int64), k["y"].astype(np.int64), p.weights, counters)
        k["octave"] = level
        k["x"] = k["x"] * scale
        k["y"] = k["y"] * scale
        k["size"] = k["size"] * scale
        parts.append(k)
    kps = np.concatenate(parts) if parts else np.zeros(0, KEYPOINT_DTYPE)
    return kps, compute_fast(img, kps, p, counters, levels), counters
