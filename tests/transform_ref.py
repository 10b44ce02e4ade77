"""A restatement of SimilarityTransform.find, AffineTransform.find and ProjectiveTransform.find (reference src/geometry/transforms.zig:47-112,
:155-191, :242-290) written for this project's tests, line by line, with what they stand on: the Golub-Reinsch SVD kernel for m x n
(src/matrix/svd.zig:149-495), SMatrix.gemm (src/matrix/SMatrix.zig:472-566), SMatrix.solve (:729-766), SMatrix.inv (:685-726), Matrix.pinv
(src/matrix/Matrix.zig:447-509), Point.orientation and areAllCollinear (src/geometry/Point.zig:200-253).

Scalars are Python floats for f64 (IEEE f64, one rounding per operation, no fused multiply-add) and numpy.float32 for f32 (every operation
on two float32 scalars is computed and rounded in f32). `T` below is that constructor: float or numpy.float32. Every constant goes through
T, so no operation is ever carried out in a wider type.

Matrices are lists of rows. Matrix.gemm's scalar loop is used for every size: the reference leaves it at 512 multiply-adds, which
AffineTransform.find's q.dot(pinv) reaches at 86 points; from there the reference's value depends on its build's vector width (DESIGN.md,
section 8) and this restatement, like the library, keeps the scalar chain."""
from __future__ import annotations

import math

import numpy as np

F32, F64 = np.float32, float
SIMILARITY, AFFINE, PROJECTIVE = 0, 1, 2
OK, NOT_CONVERGED, RANK_DEFICIENT, BAD_COUNT, BAD_INPUT = range(5)
NO_U, SKINNY_U, FULL_U = range(3)
MIN_POINTS = {SIMILARITY: 2, AFFINE: 3, PROJECTIVE: 4}
MAX_POINTS = {SIMILARITY: 65536, AFFINE: 4096, PROJECTIVE: 65536}


class NotConverged(Exception):
    pass


class RankDeficient(Exception):
    pass


def eps_of(T):
    return T(2.0 ** -23) if T is F32 else T(2.0 ** -52)


def tiny_of(T):
    return T(2.0 ** -126) if T is F32 else T(2.0 ** -1022)


def _sqrt(T, v):
    return np.sqrt(v) if T is F32 else math.sqrt(v)


def _max(a, b):
    """@max: the other operand when one is NaN."""
    return b if (b > a or a != a) else a


def zeros(T, rows, cols):
    return [[T(0) for _ in range(cols)] for _ in range(rows)]


def identity(T, n):
    m = zeros(T, n, n)
    for i in range(n):
        m[i][i] = T(1)
    return m


def svd(T, a, with_v: bool, mode: int):
    """svd.kernel: (u, q, v, converged) of an m x n matrix, m >= n. u is m x m for FULL_U, m x n for SKINNY_U."""
    m, n = len(a), len(a[0])
    ucols = m if mode == FULL_U else n
    u = zeros(T, m, ucols)
    v = zeros(T, n, n)
    q = [T(0)] * n
    e = [T(0)] * n
    eps = eps_of(T)
    tol = tiny_of(T) / eps
    retval = 0
    zero, one, two = T(0), T(1), T(2)
    for i in range(m):
        for j in range(n):
            u[i][j] = T(a[i][j])
    g = zero
    x = zero
    l = 0
    for i in range(n):
        e[i] = g
        s = zero
        l = i + 1
        for j in range(i, m):
            s += u[j][i] * u[j][i]
        if s < tol:
            g = zero
        else:
            f = u[i][i]
            g = _sqrt(T, s) if f < zero else -_sqrt(T, s)
            h = f * g - s
            u[i][i] = f - g
            for j in range(l, n):
                s = zero
                for k in range(i, m):
                    s += u[k][i] * u[k][j]
                f = s / h
                for k in range(i, m):
                    u[k][j] += f * u[k][i]
        q[i] = g
        s = zero
        for j in range(l, n):
            s += u[i][j] * u[i][j]
        if s < tol:
            g = zero
        else:
            f = u[i][i + 1]
            g = _sqrt(T, s) if f < zero else -_sqrt(T, s)
            h = f * g - s
            u[i][i + 1] = f - g
            for j in range(l, n):
                e[j] = u[i][j] / h
            for j in range(l, m):
                s = zero
                for k in range(l, n):
                    s += u[j][k] * u[i][k]
                for k in range(l, n):
                    u[j][k] += s * e[k]
        y = abs(q[i]) + abs(e[i])
        x = _max(x, y)
    if with_v:
        for i in range(n - 1, -1, -1):
            if g != zero:
                h = u[i][i + 1] * g
                for j in range(l, n):
                    v[j][i] = u[i][j] / h
                for j in range(l, n):
                    s = zero
                    for k in range(l, n):
                        s += u[i][k] * v[k][j]
                    for k in range(l, n):
                        v[k][j] += s * v[k][i]
            for j in range(l, n):
                v[i][j] = zero
                v[j][i] = zero
            v[i][i] = one
            g = e[i]
            l = i
    if mode != NO_U:
        for i in range(n, m):
            for j in range(n, ucols):
                u[i][j] = zero
            if i < ucols:
                u[i][i] = one
        for i in range(n - 1, -1, -1):
            l = i + 1
            g = q[i]
            for j in range(l, ucols):
                u[i][j] = zero
            if g != zero:
                h = u[i][i] * g
                for j in range(l, ucols):
                    s = zero
                    for k in range(l, m):
                        s += u[k][i] * u[k][j]
                    f = s / h
                    for k in range(i, m):
                        u[k][j] += f * u[k][i]
                for j in range(i, m):
                    u[j][i] /= g
            else:
                for j in range(i, m):
                    u[j][i] = zero
            u[i][i] += one
    eps = eps * x
    for k in range(n - 1, -1, -1):
        it = 0
        state = "split"
        z = zero
        while state != "done":
            if state == "split":
                state = "converge"
                l = k
                while True:
                    if abs(e[l]) <= eps:
                        break
                    if l == 0:  # e[0] is 0: reached only where eps is NaN, where the reference would index q[-1]
                        break
                    if abs(q[l - 1]) <= eps:
                        state = "cancel"
                        break
                    l -= 1
            elif state == "cancel":
                c = zero
                s = one
                l1 = l - 1
                state = "converge"
                for i in range(l, k + 1):
                    f = s * e[i]
                    e[i] *= c
                    if abs(f) <= eps:
                        break
                    g = q[i]
                    h = _sqrt(T, f * f + g * g)
                    q[i] = h
                    c = g / h
                    s = -f / h
                    if mode != NO_U:
                        for j in range(m):
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
                f = ((y - z) * (y + z) + (g - h) * (g + h)) / (two * h * y)
                g = _sqrt(T, f * f + one)
                f = ((x - z) * (x + z) + h * (y / ((f - g) if f < zero else (f + g)) - h)) / x
                c = one
                s = one
                for i in range(l + 1, k + 1):
                    g = e[i]
                    y = q[i]
                    h = s * g
                    g *= c
                    z = _sqrt(T, f * f + h * h)
                    e[i - 1] = z
                    c = f / z
                    s = h / z
                    f = x * c + g * s
                    g = -x * s + g * c
                    h = y * s
                    y *= c
                    if with_v:
                        for j in range(n):
                            x = v[j][i - 1]
                            z = v[j][i]
                            v[j][i - 1] = x * c + z * s
                            v[j][i] = -x * s + z * c
                    z = _sqrt(T, f * f + h * h)
                    q[i - 1] = z
                    if z != zero:
                        c = f / z
                        s = h / z
                    f = c * g + s * y
                    x = -s * g + c * y
                    if mode != NO_U:
                        for j in range(m):
                            y = u[j][i - 1]
                            z = u[j][i]
                            u[j][i - 1] = y * c + z * s
                            u[j][i] = -y * s + z * c
                e[l] = zero
                e[k] = f
                q[k] = x
                state = "split"
            elif state == "check":
                if z < zero:
                    q[k] = -z
                    if with_v:
                        for j in range(n):
                            v[j][k] = -v[j][k]
                state = "done"
    for i in range(n):
        max_idx, max_val = i, q[i]
        for j in range(i + 1, n):
            if q[j] > max_val:
                max_idx, max_val = j, q[j]
        if max_idx != i:
            q[i], q[max_idx] = q[max_idx], q[i]
            if mode != NO_U:
                for row in range(m):
                    u[row][i], u[row][max_idx] = u[row][max_idx], u[row][i]
            if with_v:
                for row in range(n):
                    v[row][i], v[row][max_idx] = v[row][max_idx], v[row][i]
    return u, q, v, retval


def gemm(T, a, b, trans_b: bool = False):
    """gemm(false, other, trans_b, 1.0, 0.0, null), the scalar loop: a zeroed result, an accumulator from 0 in k order, result += 1.0 * acc."""
    rows, inner = len(a), len(a[0])
    cols = len(b) if trans_b else len(b[0])
    out = zeros(T, rows, cols)
    for i in range(rows):
        for j in range(cols):
            acc = T(0)
            for k in range(inner):
                acc += a[i][k] * (b[j][k] if trans_b else b[k][j])
            out[i][j] += T(1) * acc
    return out


def det2(a):
    return a[0][0] * a[1][1] - a[0][1] * a[1][0]


def transpose(a):
    return [[a[r][c] for r in range(len(a))] for c in range(len(a[0]))]


def solve(T, a_in, b_in):
    """SMatrix.solve with one column: the solution as a list, or None."""
    n = len(a_in)
    a = [[T(a_in[r][c]) for c in range(n)] + [T(b_in[r])] for r in range(n)]
    max_entry = T(0)
    for r in range(n):
        for c in range(n):
            max_entry = _max(max_entry, abs(a[r][c]))
    if max_entry == T(0):
        return None
    tolerance = max_entry * eps_of(T) * T(100)
    for c in range(n):
        pivot = c
        for r in range(c + 1, n):
            if abs(a[r][c]) > abs(a[pivot][c]):
                pivot = r
        if abs(a[pivot][c]) < tolerance:
            return None
        a[c], a[pivot] = a[pivot], a[c]
        for r in range(n):
            if r == c:
                continue
            factor = a[r][c] / a[c][c]
            if factor == T(0):
                continue
            for idx in range(c, n + 1):
                a[r][idx] -= factor * a[c][idx]
    return [a[i][n] / a[i][i] for i in range(n)]


def inv3(T, s):
    """SMatrix.inv, rows == 3: rows, or None."""
    c00 = s[1][1] * s[2][2] - s[1][2] * s[2][1]
    c01 = s[0][2] * s[2][1] - s[0][1] * s[2][2]
    c02 = s[0][1] * s[1][2] - s[0][2] * s[1][1]
    d = s[0][0] * c00 + s[1][0] * c01 + s[2][0] * c02
    if d == T(0):
        return None
    return [[c00 / d, c01 / d, c02 / d],
            [(s[1][2] * s[2][0] - s[1][0] * s[2][2]) / d, (s[0][0] * s[2][2] - s[0][2] * s[2][0]) / d, (s[0][2] * s[1][0] - s[0][0] * s[1][2]) / d],
            [(s[1][0] * s[2][1] - s[1][1] * s[2][0]) / d, (s[0][1] * s[2][0] - s[0][0] * s[2][1]) / d, (s[0][0] * s[1][1] - s[0][1] * s[1][0]) / d]]


def collinear3(T, a, b, c):
    swap = (b[0] > c[0]) or (b[0] == c[0] and b[1] > c[1])
    p1, p2 = (c, b) if swap else (b, c)
    u = a[0] * (p1[1] - p2[1]) + p1[0] * (p2[1] - a[1]) + p2[0] * (a[1] - p1[1])
    return u == T(0)


def all_collinear(T, pts):
    if len(pts) < 3:
        return True
    p1 = pts[0]
    i = 1
    while i < len(pts):
        if not (pts[i][0] == p1[0] and pts[i][1] == p1[1]):
            break
        i += 1
    if i == len(pts):
        return True
    p2 = pts[i]
    for p in pts[i + 1:]:
        if not collinear3(T, p1, p2, p):
            return False
    return True


def _points(T, pts):
    return [(T(p[0]), T(p[1])) for p in pts]


def find_similarity(T, from_points, to_points):
    """(matrix 2 x 2, bias[2]); raises NotConverged / RankDeficient."""
    fp, tp = _points(T, from_points), _points(T, to_points)
    assert len(fp) >= 2 and len(fp) == len(tp)
    num_points = T(len(fp))
    mfx = mfy = mtx = mty = T(0)
    for i in range(len(fp)):
        mfx = mfx + fp[i][0]
        mfy = mfy + fp[i][1]
        mtx = mtx + tp[i][0]
        mty = mty + tp[i][1]
    inv_n = T(1) / num_points
    mfx, mfy, mtx, mty = mfx * inv_n, mfy * inv_n, mtx * inv_n, mty * inv_n
    sigma_from = T(0)
    cov = zeros(T, 2, 2)
    for i in range(len(fp)):
        fx, fy = fp[i][0] - mfx, fp[i][1] - mfy
        tx, ty = tp[i][0] - mtx, tp[i][1] - mty
        sigma_from += fx * fx + fy * fy
        prod = gemm(T, [[tx], [ty]], [[fx, fy]])
        cov = [[cov[r][c] + prod[r][c] for c in range(2)] for r in range(2)]
    sigma_from /= num_points
    cov = [[inv_n * cov[r][c] for c in range(2)] for r in range(2)]
    det_cov = det2(cov)
    u, s_values, v, converged = svd(T, cov, True, SKINNY_U)
    if converged != 0:
        raise NotConverged(converged)
    tol = s_values[0] * eps_of(T) * T(2)
    effective_rank = sum(1 for i in range(2) if s_values[i] > tol)
    if effective_rank == 0:
        raise RankDeficient()
    d = [[s_values[0], T(0)], [T(0), s_values[1]]]
    det_u, det_v = det2(u), det2(v)
    s = identity(T, 2)
    if det_cov < T(0) or (det_cov == T(0) and det_u * det_v < T(0)):
        if d[1][1] < d[0][0]:
            s[1][1] = T(-1)
        else:
            s[0][0] = T(-1)
    r = gemm(T, u, gemm(T, s, transpose(v)))
    c = T(1)
    if sigma_from != T(0):
        ds = gemm(T, d, s)
        trace = T(0)
        for i in range(2):
            trace += ds[i][i]
        c = T(1) / sigma_from * trace
    rm = gemm(T, r, [[mfx], [mfy]])
    matrix = [[c * r[i][j] for j in range(2)] for i in range(2)]
    bias = [mtx + (-c) * rm[0][0], mty + (-c) * rm[1][0]]
    return matrix, bias


def find_affine(T, from_points, to_points):
    fp, tp = _points(T, from_points), _points(T, to_points)
    assert len(fp) >= 3 and len(fp) == len(tp)
    n = len(fp)
    p_t = [[fp[i][0], fp[i][1], T(1)] for i in range(n)]  # p.transpose(): pinv of a wide matrix runs pinvTall on the transpose
    q = [[tp[i][0] for i in range(n)], [tp[i][1] for i in range(n)]]
    u, s, v, converged = svd(T, p_t, True, SKINNY_U)
    if converged != 0:
        raise NotConverged(converged)
    sigma_max = s[0]
    if sigma_max == T(0):
        raise RankDeficient()  # the zero matrix with effective_rank 0
    tol = sigma_max * T(max(n, 3)) * eps_of(T)
    v_sigma = [row[:] for row in v]
    effective_rank = 0
    for i in range(3):
        sigma = s[i]
        inv_sigma = T(1) / sigma if sigma > tol else T(0)
        if sigma > tol:
            effective_rank += 1
        for r in range(3):
            v_sigma[r][i] *= inv_sigma
    if effective_rank < 3:
        raise RankDeficient()
    pinv = transpose(gemm(T, v_sigma, u, trans_b=True))  # n x 3
    m = gemm(T, q, pinv)
    return [[m[0][0], m[0][1]], [m[1][0], m[1][1]]], [m[0][2], m[1][2]]


def find_projective(T, from_points, to_points):
    """The 3 x 3 matrix as rows."""
    fp, tp = _points(T, from_points), _points(T, to_points)
    assert len(fp) >= 4 and len(fp) == len(tp)
    if all_collinear(T, fp) or all_collinear(T, tp):
        raise RankDeficient()
    zero, one = T(0), T(1)
    if len(fp) == 4:
        a, b = [], []
        for f, t in zip(fp, tp):
            a.append([f[0], f[1], one, zero, zero, zero, -t[0] * f[0], -t[0] * f[1]])
            a.append([zero, zero, zero, f[0], f[1], one, -t[1] * f[0], -t[1] * f[1]])
            b.append(t[0])
            b.append(t[1])
        h = solve(T, a, b)
        if h is None:
            raise RankDeficient()
        return [[h[0], h[1], h[2]], [h[3], h[4], h[5]], [h[6], h[7], one]]
    accum = zeros(T, 9, 9)
    b = zeros(T, 2, 9)
    for i in range(len(fp)):
        f = [fp[i][0], fp[i][1], one]
        tx, ty = tp[i][0], tp[i][1]
        neg_tx_f = [(-tx) * v for v in f]
        ty_f = [ty * v for v in f]
        b[0][0:3] = ty_f
        b[1][0:3] = f
        b[0][3:6] = neg_tx_f
        b[1][6:9] = neg_tx_f
        prod = gemm(T, transpose(b), b)
        accum = [[accum[r][c] + prod[r][c] for c in range(9)] for r in range(9)]
    u, _, _, converged = svd(T, accum, False, FULL_U)
    if converged != 0:
        raise NotConverged(converged)
    col = [u[r][8] for r in range(9)]
    return [col[0:3], col[3:6], col[6:9]]


def project(T, kind, m, point):
    """project for a flat m laid out as zg_warp takes it."""
    px, py = T(point[0]), T(point[1])
    if kind == PROJECTIVE:
        d = gemm(T, [list(m[0:3]), list(m[3:6]), list(m[6:9])], [[px], [py], [T(1)]])
        x, y, w = d[0][0], d[1][0], d[2][0]
        if w != T(0):
            inv = T(1) / w
            x, y = inv * x, inv * y
        return x, y
    d = gemm(T, [list(m[0:2]), list(m[2:4])], [[px], [py]])
    return d[0][0] + m[4], d[1][0] + m[5]


def identity_flat(T, kind):
    m = [T(0)] * 9
    m[0] = T(1)
    if kind == PROJECTIVE:
        m[4] = m[8] = T(1)
    else:
        m[3] = T(1)
    return m


def fit(T, kind, from_points, to_points):
    """(status, m[9] as T) the way the library's record reports a fit: the identity on any failure."""
    n = len(from_points)
    if n < MIN_POINTS[kind] or n > MAX_POINTS[kind]:
        return BAD_COUNT, identity_flat(T, kind)
    try:
        if kind == PROJECTIVE:
            rows = find_projective(T, from_points, to_points)
            return OK, [rows[r][c] for r in range(3) for c in range(3)]
        matrix, bias = (find_similarity if kind == SIMILARITY else find_affine)(T, from_points, to_points)
        return OK, [matrix[0][0], matrix[0][1], matrix[1][0], matrix[1][1], bias[0], bias[1], T(0), T(0), T(0)]
    except NotConverged:
        return NOT_CONVERGED, identity_flat(T, kind)
    except RankDeficient:
        return RANK_DEFICIENT, identity_flat(T, kind)
