"""A restatement of FeatureDistributionMatching (reference src/fdm.zig) written for this project's tests: CovarianceStats' Welford
recurrence (src/stats.zig:261-320), the Golub-Reinsch SVD kernel as SMatrix(f64, 3, 3).svd(.skinny_u, no V) runs it
(src/matrix/svd.zig:149-495), the two Matrix.dot products, the bias and the three apply routes. Scalars are Python floats (IEEE f64, one
rounding per operation, no fused multiply-add); the per-pixel maps are numpy elementwise f64 with the operation order written out.

Images are numpy uint8 arrays: (rows, cols) for u8, (rows, cols, 3) for Rgb(u8), (rows, cols, 4) for Rgba(u8)."""
from __future__ import annotations

import math

import numpy as np

ROUTE_COLOR, ROUTE_SCALAR, ROUTE_GRAY_TARGET = range(3)
EPS = 2.220446049250313e-16
TOL = 2.2250738585072014e-308 / EPS


class NotConverged(Exception):
    pass


def luminance(img: np.ndarray) -> np.ndarray:
    """convertColor(u8, pixel) of a colour image: BT.709 in 16.16 fixed point (src/color.zig:1031-1041); alpha takes no part."""
    c = img.astype(np.int64)
    y = (13933 * c[..., 0] + 46871 * c[..., 1] + 4732 * c[..., 2] + 32768) >> 16
    return np.clip(y, 0, 255).astype(np.uint8)


def welford(samples):
    """CovarianceStats(3, f64) over an iterable of (a, b, c): (count, mean[3], m2[3][3])."""
    count = 0
    mean = [0.0, 0.0, 0.0]
    m2 = [[0.0] * 3 for _ in range(3)]
    for sample in samples:
        count += 1
        n = float(count)
        delta = [0.0, 0.0, 0.0]
        for i in range(3):
            delta[i] = sample[i] - mean[i]
            mean[i] += delta[i] / n
        for i in range(3):
            for j in range(i, 3):
                term = delta[i] * (sample[j] - mean[j])
                m2[i][j] += term
                if i != j:
                    m2[j][i] += term
    return count, mean, m2


def covariance(count, m2):
    """covarianceMatrix / varianceVector (stats.zig:289-320): zeros for count <= 1."""
    if count <= 1:
        return [[0.0] * 3 for _ in range(3)]
    n_1 = float(count - 1)
    return [[m2[min(i, j)][max(i, j)] / n_1 for j in range(3)] for i in range(3)]


def image_stats(img: np.ndarray, as_luminance: bool = False):
    """(mean[3], cov[3][3]) as setTarget / update accumulate them: v = byte / 255.0, a scalar three times over."""
    if img.ndim == 2 or as_luminance:
        plane = img if img.ndim == 2 else luminance(img)
        vals = (plane.reshape(-1).astype(np.float64) / 255.0).tolist()
        count, mean, m2 = welford((v, v, v) for v in vals)
    else:
        rgb = (img[..., :3].reshape(-1, 3).astype(np.float64) / 255.0).tolist()
        count, mean, m2 = welford(rgb)
    if count == 0:
        mean = [0.0, 0.0, 0.0]
    return mean, covariance(count, m2)


def is_gray(img: np.ndarray) -> bool:
    if img.ndim == 2:
        return True
    return not bool(np.any((img[..., 0] != img[..., 1]) | (img[..., 1] != img[..., 2])))


def svd3(a):
    """(u[3][3], q[3], converged) of a 3 x 3 matrix given as rows."""
    n = 3
    u = [[float(a[i][j]) for j in range(3)] for i in range(3)]
    q = [0.0, 0.0, 0.0]
    e = [0.0, 0.0, 0.0]
    eps = EPS
    retval = 0
    g = 0.0
    x = 0.0
    l = 0
    for i in range(n):
        e[i] = g
        s = 0.0
        l = i + 1
        for j in range(i, n):
            s += u[j][i] * u[j][i]
        if s < TOL:
            g = 0.0
        else:
            f = u[i][i]
            g = math.sqrt(s) if f < 0 else -math.sqrt(s)
            h = f * g - s
            u[i][i] = f - g
            for j in range(l, n):
                s = 0.0
                for k in range(i, n):
                    s += u[k][i] * u[k][j]
                f = s / h
                for k in range(i, n):
                    u[k][j] += f * u[k][i]
        q[i] = g
        s = 0.0
        for j in range(l, n):
            s += u[i][j] * u[i][j]
        if s < TOL:
            g = 0.0
        else:
            f = u[i][i + 1]
            g = math.sqrt(s) if f < 0 else -math.sqrt(s)
            h = f * g - s
            u[i][i + 1] = f - g
            for j in range(l, n):
                e[j] = u[i][j] / h
            for j in range(l, n):
                s = 0.0
                for k in range(l, n):
                    s += u[j][k] * u[i][k]
                for k in range(l, n):
                    u[j][k] += s * e[k]
        y = abs(q[i]) + abs(e[i])
        x = y if (y > x or x != x) else x
    for i in range(n - 1, -1, -1):
        l = i + 1
        g = q[i]
        for j in range(l, n):
            u[i][j] = 0.0
        if g != 0:
            h = u[i][i] * g
            for j in range(l, n):
                s = 0.0
                for k in range(l, n):
                    s += u[k][i] * u[k][j]
                f = s / h
                for k in range(i, n):
                    u[k][j] += f * u[k][i]
            for j in range(i, n):
                u[j][i] /= g
        else:
            for j in range(i, n):
                u[j][i] = 0.0
        u[i][i] += 1.0
    eps *= x
    for k in range(n - 1, -1, -1):
        it = 0
        state = "split"
        z = 0.0
        while state != "done":
            if state == "split":
                state = "converge"
                l = k
                while True:
                    if abs(e[l]) <= eps:
                        break
                    if l == 0:
                        break
                    if abs(q[l - 1]) <= eps:
                        state = "cancel"
                        break
                    l -= 1
            elif state == "cancel":
                c = 0.0
                s = 1.0
                l1 = l - 1
                state = "converge"
                for i in range(l, k + 1):
                    f = s * e[i]
                    e[i] *= c
                    if abs(f) <= eps:
                        break
                    g = q[i]
                    h = math.sqrt(f * f + g * g)
                    q[i] = h
                    c = g / h
                    s = -f / h
                    for j in range(n):
                        y = u[j][l1]
                        z = u[j][i]
                        u[j][l1] = y * c + z * s
                        u[j][i] = -y * s + z * c
            elif state == "converge":
                z = q[k]
                if l == k:
                    state = "check"
                    continue
                it += 1
                if it > 300:
                    retval = k
                    state = "done"
                    continue
                x = q[l]
                y = q[k - 1]
                g = e[k - 1]
                h = e[k]
                f = ((y - z) * (y + z) + (g - h) * (g + h)) / (2.0 * h * y)
                g = math.sqrt(f * f + 1.0)
                f = ((x - z) * (x + z) + h * (y / ((f - g) if f < 0 else (f + g)) - h)) / x
                c = 1.0
                s = 1.0
                for i in range(l + 1, k + 1):
                    g = e[i]
                    y = q[i]
                    h = s * g
                    g *= c
                    z = math.sqrt(f * f + h * h)
                    e[i - 1] = z
                    c = f / z
                    s = h / z
                    f = x * c + g * s
                    g = -x * s + g * c
                    h = y * s
                    y *= c
                    z = math.sqrt(f * f + h * h)
                    q[i - 1] = z
                    if z != 0:
                        c = f / z
                        s = h / z
                    f = c * g + s * y
                    x = -s * g + c * y
                    for j in range(n):
                        y = u[j][i - 1]
                        z = u[j][i]
                        u[j][i - 1] = y * c + z * s
                        u[j][i] = -y * s + z * c
                e[l] = 0.0
                e[k] = f
                q[k] = x
                state = "split"
            elif state == "check":
                if z < 0:
                    q[k] = -z
                state = "done"
    for i in range(n):
        max_idx, max_val = i, q[i]
        for j in range(i + 1, n):
            if q[j] > max_val:
                max_idx, max_val = j, q[j]
        if max_idx != i:
            q[i], q[max_idx] = q[max_idx], q[i]
            for row in range(n):
                u[row][i], u[row][max_idx] = u[row][max_idx], u[row][i]
    return u, q, retval


def dot3(a, b):
    """Matrix.dot on 3 x 3: the scalar gemm loop (Matrix.zig:806-817) onto a zeroed result."""
    out = [[0.0] * 3 for _ in range(3)]
    for i in range(3):
        for j in range(3):
            acc = 0.0
            for k in range(3):
                acc += a[i][k] * b[k][j]
            out[i][j] += 1.0 * acc
    return out


def make_target(mean, cov, gray: bool):
    """setTarget from the statistics: a dict with mean, u, s, is_gray."""
    if gray:
        return {"mean": list(mean), "u": [[0.0] * 3 for _ in range(3)], "s": [cov[0][0], 0.0, 0.0], "is_gray": True}
    u, s, conv = svd3(cov)
    if conv != 0:
        raise NotConverged(conv)
    return {"mean": list(mean), "u": u, "s": s, "is_gray": False}


def make_transform(is_u8: bool, target, mean, cov):
    """update between the statistics and the pixel loop: a dict with route, w, bias, scale, offset."""
    route = ROUTE_SCALAR if is_u8 else (ROUTE_GRAY_TARGET if target["is_gray"] else ROUTE_COLOR)
    x = {"route": route, "w": [[0.0] * 3 for _ in range(3)], "bias": [0.0] * 3, "scale": 1.0, "offset": 0.0}
    if route != ROUTE_COLOR:
        var = cov[0][0]
        x["scale"] = math.sqrt(target["s"][0] / var) if var > 1e-10 else 1.0
        x["offset"] = target["mean"][0] - mean[0] * x["scale"]
        return x
    us, ss, conv = svd3(cov)
    if conv != 0:
        raise NotConverged(conv)
    x["source_s"] = ss
    sigma = [[0.0] * 3 for _ in range(3)]
    for i in range(3):
        if ss[i] > 1e-10:
            sigma[i][i] = math.sqrt(target["s"][i] / ss[i])
    ut_t = [[target["u"][j][i] for j in range(3)] for i in range(3)]
    w = dot3(dot3(us, sigma), ut_t)
    x["w"] = w
    for j in range(3):
        total = 0.0
        for k in range(3):
            total += mean[k] * w[k][j]
        x["bias"][j] = target["mean"][j] - total
    return x


def _round_unit(res: np.ndarray):
    """(bytes, 255 * clamp(res, 0, 1)): @round is half away from zero; on [0, 255] that is trunc plus a compare, exactly."""
    c = np.where(res != res, 1.0, np.where(res < 0.0, 0.0, np.where(res > 1.0, 1.0, res)))
    p = 255.0 * c
    t = np.trunc(p)
    return (t + ((p - t) >= 0.5)).astype(np.uint8), p


def apply(img: np.ndarray, x, return_pre: bool = False):
    """The pixel loops of update (fdm.zig:184-198, :257-271) on a copy of img. return_pre: also every 255 * clamp(...) before @round."""
    out = img.copy()
    if x["route"] == ROUTE_COLOR:
        r, g, b = (img[..., k].astype(np.float64) / 255.0 for k in range(3))
        w, bias = x["w"], x["bias"]
        pres = []
        for j in range(3):
            res = ((r * w[0][j] + g * w[1][j]) + b * w[2][j]) + bias[j]
            out[..., j], p = _round_unit(res)
            pres.append(p)
        pre = np.stack(pres, -1)
    else:
        plane = img if img.ndim == 2 else luminance(img)
        val = plane.astype(np.float64) / 255.0
        byte, pre = _round_unit(val * x["scale"] + x["offset"])
        if img.ndim == 2:
            out[...] = byte
        else:
            out[..., 0] = out[..., 1] = out[..., 2] = byte
            if img.shape[2] == 4:
                out[..., 3] = 0  # the struct literal of fdm.zig:196 leaves `a` at its field default, 0 (src/color.zig:405)
    return (out, pre) if return_pre else out


def prepare_target(target_img: np.ndarray):
    gray = is_gray(target_img)
    mean, cov = image_stats(target_img)
    return make_target(mean, cov, gray)


def source_transform(src: np.ndarray, target):
    mean, cov = image_stats(src, as_luminance=(src.ndim == 3 and target["is_gray"]))
    return make_transform(src.ndim == 2, target, mean, cov)


def match(src: np.ndarray, target_img: np.ndarray, return_pre: bool = False):
    """FeatureDistributionMatching(T).match on copies: the matched source."""
    target = prepare_target(target_img)
    return apply(src, source_transform(src, target), return_pre)


# ---- the same from exact integer moments, as the device derives its statistics --------------------------------------------------------

def moments(img: np.ndarray):
    """The integer moments of a frame: n, sum[3], prod[6] (rr rg rb gg gb bb), lum_sum, lum_sq, not_gray, as Python ints."""
    if img.ndim == 2:
        v = img.reshape(-1).astype(np.uint64)
        return {"n": int(v.size), "sum": [0, 0, 0], "prod": [0] * 6, "lum_sum": int(v.sum()), "lum_sq": int((v * v).sum()), "not_gray": 0}
    c = img[..., :3].reshape(-1, 3).astype(np.uint64)
    y = luminance(img).reshape(-1).astype(np.uint64)
    prod = [int((c[:, i] * c[:, j]).sum()) for i in range(3) for j in range(i, 3)]
    return {"n": int(c.shape[0]), "sum": [int(c[:, k].sum()) for k in range(3)], "prod": prod, "lum_sum": int(y.sum()), "lum_sq": int((y * y).sum()),
            "not_gray": 0 if is_gray(img) else 1}


def exact_cov(n, sx, sy, sxy):
    from fractions import Fraction
    return Fraction(0) if n <= 1 else Fraction(n * sxy - sx * sy, 65025 * n * (n - 1))


def exact_mean(n, sx):
    from fractions import Fraction
    return Fraction(0) if n == 0 else Fraction(sx, 255 * n)
