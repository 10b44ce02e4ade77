// zg_transform_fit.h — SimilarityTransform.find, AffineTransform.find and ProjectiveTransform.find (reference src/geometry/transforms.zig:47-112,
// :155-191, :242-290) with everything under them, written once for the host and the device: the Golub-Reinsch SVD kernel for m x n, m >= n
// (src/matrix/svd.zig:149-495), SMatrix.gemm on small matrices (SMatrix.zig:472-566), the 8 x 8 Gauss-Jordan solve (:729-766), Matrix.pinv
// (Matrix.zig:447-509), Point.orientation and areAllCollinear (Point.zig:200-253), project for the three kinds, SMatrix.inv of 3 x 3
// (SMatrix.zig:685-726). It includes nothing of HIP or of the library; a host build defines __host__ and __device__ away.
// Only + - * /, sqrt and fabs on T = float or double, each rounded as written: NO FMA MAY BE FORMED, so every build of this header, the
// host's too, uses -ffp-contract=off (the pragma below says the same to clang).
//
// The text is written against an executor X, so that one text serves one thread and one workgroup:
//   x.rows(r0, r1, f)          f(k) for k in [r0, r1): operations that are independent from one k to the next
//   x.chains<K>(r0, r1, t, o)  o[c] = (((0 + t(r0, c)) + t(r0 + 1, c)) + ...) for c < K: K sequential sums in index order
//   x.first(r0, r1, p)         the lowest k in [r0, r1) with p(k), or r1
//   x.solo(f)                  f() once: everything that is one dependent chain anyway
// Serial (below) runs them as plain loops. A workgroup's executor (transform_fit.hip) deals rows to lanes, lets all lanes compute the terms
// of a sum into LDS and one lane per sum add them in order, and runs solo on one lane between two barriers; every lane walks the same text
// with the same values, so control flow is uniform. Arrays indexed by run-time values (every work array of the SVD) are the caller's:
// LDS on the device, where a lane's own array would be scratch memory.
#pragma once
#include <math.h>
#include <stdint.h>

#if defined(__clang__)
#pragma clang fp contract(off)
#endif

namespace zg_tf {

enum { KIND_SIMILARITY = 0, KIND_AFFINE = 1, KIND_PROJECTIVE = 2 }; // zg_transform_kind
enum { FIT_OK = 0, FIT_NOT_CONVERGED = 1, FIT_RANK_DEFICIENT = 2, FIT_BAD_COUNT = 3, FIT_BAD_INPUT = 4 }; // ZG_FIT_*
enum { SVD_NO_U = 0, SVD_SKINNY_U = 1, SVD_FULL_U = 2 };                                                // svd.zig's Mode
enum { MAX_POINTS = 65536, MAX_POINTS_AFFINE = 4096, MAX_CHAINS = 45 };

template <typename T> struct Num;
template <> struct Num<float> {
    __host__ __device__ static inline float eps() { return 1.1920928955078125e-07f; }   // floatEps(f32) = 2^-23
    __host__ __device__ static inline float tiny() { return 1.1754943508222875e-38f; }  // floatMin(f32) = 2^-126
    __host__ __device__ static inline float sqrt_(float v) { return sqrtf(v); }
    __host__ __device__ static inline float abs_(float v) { return fabsf(v); }
};
template <> struct Num<double> {
    __host__ __device__ static inline double eps() { return 2.220446049250313e-16; }    // floatEps(f64) = 2^-52
    __host__ __device__ static inline double tiny() { return 2.2250738585072014e-308; } // floatMin(f64) = 2^-1022
    __host__ __device__ static inline double sqrt_(double v) { return sqrt(v); }
    __host__ __device__ static inline double abs_(double v) { return fabs(v); }
};
// @max(a, b): the other operand when one is NaN
template <typename T> __host__ __device__ inline T max_(T a, T b) { return (b > a || a != a) ? b : a; }

__host__ __device__ inline int min_points(int kind) { return kind == KIND_SIMILARITY ? 2 : (kind == KIND_AFFINE ? 3 : 4); }
__host__ __device__ inline int max_points(int kind) { return kind == KIND_AFFINE ? (int)MAX_POINTS_AFFINE : (int)MAX_POINTS; }

struct Serial {
    template <typename F> __host__ __device__ inline void rows(int r0, int r1, F f) {
        for (int k = r0; k < r1; ++k) f(k);
    }
    template <int K, typename T, typename F> __host__ __device__ inline void chains(int r0, int r1, F term, T *out) {
        for (int c = 0; c < K; ++c) {
            T s = (T)0;
            for (int k = r0; k < r1; ++k) s += term(k, c);
            out[c] = s;
        }
    }
    template <typename P> __host__ __device__ inline int first(int r0, int r1, P pred) {
        for (int k = r0; k < r1; ++k)
            if (pred(k)) return k;
        return r1;
    }
    template <typename F> __host__ __device__ inline void solo(F f) { f(); }
};

// s = 0; s += t(k) for k in [r0, r1): one sum through the executor; `slot` is one T of the caller's work memory
template <typename T, typename X, typename F> __host__ __device__ inline T chain(X &x, int r0, int r1, F term, T *slot) {
    x.template chains<1>(r0, r1, [=](int k, int) { return term(k); }, slot);
    return *slot;
}

// ---- svd.kernel ------------------------------------------------------------------------------------------------------------------------

// a (m x n, row-major, or null when the caller has put it into u already), u (m x ucols, ucols = m for .full_u, n otherwise), v (n x n, read
// and written only with with_v), q and e (n), slot (one T). mode is .skinny_u or .full_u (.no_u has no caller here). Returns the
// reference's `converged`: 0, or the k whose QR iteration passed 300 steps. Line numbers are svd.zig's. Sums over the m rows go through
// x.chains, sums over the n columns are short and every thread adds them itself, in the same order.
template <typename T, typename X>
__host__ __device__ inline int svd(X &x, const T *a, T *u, int m, int n, int mode, T *v, T *q, T *e, bool with_v, T *slot) {
    typedef Num<T> N_;
    const int ucols = mode == SVD_FULL_U ? m : n;
    const int max_iterations = 300;
    T eps = N_::eps();
    const T tol = N_::tiny() / eps; // :180
    int l = 0, retval = 0;
    T c = (T)0, f = (T)0, g = (T)0, h = (T)0, s = (T)0, x_ = (T)0, y = (T)0, z = (T)0;
#define ZG_U(r, cc) u[(r) * ucols + (cc)]
#define ZG_V(r, cc) v[(r) * n + (cc)]
    if (a) { // :194-198
        x.rows(0, m, [=](int i) {
            for (int j = 0; j < n; ++j) ZG_U(i, j) = a[i * n + j];
        });
    }
    x.solo([=]() {
        for (int i = 0; i < n; ++i) q[i] = e[i] = (T)0;
    });
    // Householder's reduction to bidiagonal form (:201-264)
    g = (T)0;
    x_ = (T)0;
    for (int i = 0; i < n; ++i) {
        const T g_in = g;
        x.solo([=]() { e[i] = g_in; });
        l = i + 1;
        s = chain<T>(x, i, m, [=](int j) { return ZG_U(j, i) * ZG_U(j, i); }, slot);
        if (s < tol) {
            g = (T)0;
        } else {
            f = ZG_U(i, i);
            g = f < (T)0 ? N_::sqrt_(s) : -N_::sqrt_(s); // :216
            h = f * g - s;
            {
                const T d = f - g;
                x.solo([=]() { ZG_U(i, i) = d; });
            }
            for (int j = l; j < n; ++j) {
                s = chain<T>(x, i, m, [=](int k) { return ZG_U(k, i) * ZG_U(k, j); }, slot);
                f = s / h;
                const T ff = f;
                x.rows(i, m, [=](int k) { ZG_U(k, j) += ff * ZG_U(k, i); });
            }
        }
        {
            const T gq = g;
            x.solo([=]() { q[i] = gq; });
        }
        // deliberate: in a workgroup every lane adds this short sum, and the scalars of the QR sweep below, for itself from LDS; handing them
        // round through solo() would cost two barriers each
        s = (T)0;
        for (int j = l; j < n; ++j) s += ZG_U(i, j) * ZG_U(i, j);
        if (s < tol) {
            g = (T)0;
        } else {
            f = ZG_U(i, i + 1);
            g = f < (T)0 ? N_::sqrt_(s) : -N_::sqrt_(s); // :244
            h = f * g - s;
            const T d = f - g, hh = h;
            const int ll = l;
            x.solo([=]() {
                ZG_U(i, i + 1) = d;
                for (int j = ll; j < n; ++j) e[j] = ZG_U(i, j) / hh;
            });
            x.rows(l, m, [=](int j) {
                T sj = (T)0;
                for (int k = ll; k < n; ++k) sj += ZG_U(j, k) * ZG_U(i, k);
                for (int k = ll; k < n; ++k) ZG_U(j, k) += sj * e[k];
            });
        }
        y = N_::abs_(q[i]) + N_::abs_(e[i]);
        x_ = max_(x_, y); // :263
    }
    // accumulation of right-hand transformations (:267-293): n x n, one dependent chain
    if (with_v) {
        const T g_in = g;
        const int l_in = l;
        x.solo([=]() {
            T gg = g_in, hh, ss;
            int ll = l_in;
            for (int i = n - 1; i >= 0; --i) {
                if (gg != (T)0) {
                    hh = ZG_U(i, i + 1) * gg;
                    for (int j = ll; j < n; ++j) ZG_V(j, i) = ZG_U(i, j) / hh;
                    for (int j = ll; j < n; ++j) {
                        ss = (T)0;
                        for (int k = ll; k < n; ++k) ss += ZG_U(i, k) * ZG_V(k, j);
                        for (int k = ll; k < n; ++k) ZG_V(k, j) += ss * ZG_V(k, i);
                    }
                }
                for (int j = ll; j < n; ++j) {
                    ZG_V(i, j) = (T)0;
                    ZG_V(j, i) = (T)0;
                }
                ZG_V(i, i) = (T)1;
                gg = e[i];
                ll = i;
            }
        });
        g = e[0];
        l = 0;
    }
    // accumulation of left-hand transformations (:296-338)
    x.rows(n, m, [=](int i) {
        for (int j = n; j < ucols; ++j) ZG_U(i, j) = (T)0;
        if (i < ucols) ZG_U(i, i) = (T)1;
    });
    for (int i = n - 1; i >= 0; --i) {
        l = i + 1;
        g = q[i];
        {
            const int ll = l;
            x.solo([=]() {
                for (int j = ll; j < ucols; ++j) ZG_U(i, j) = (T)0;
            });
        }
        if (g != (T)0) {
            h = ZG_U(i, i) * g;
            for (int j = l; j < ucols; ++j) {
                s = chain<T>(x, l, m, [=](int k) { return ZG_U(k, i) * ZG_U(k, j); }, slot);
                f = s / h;
                const T ff = f;
                x.rows(i, m, [=](int k) { ZG_U(k, j) += ff * ZG_U(k, i); });
            }
            const T gg = g;
            x.rows(i, m, [=](int j) { ZG_U(j, i) /= gg; });
        } else {
            x.rows(i, m, [=](int j) { ZG_U(j, i) = (T)0; });
        }
        x.solo([=]() { ZG_U(i, i) += (T)1; });
    }
    // diagonalization of the bidiagonal form (:341-468)
    eps *= x_;
    for (int k = n - 1; k >= 0; --k) {
        int iter = 0;
        enum { TEST_SPLITTING, CANCELLATION, TEST_CONVERGENCE, CONVERGENCE_CHECK, DONE } state = TEST_SPLITTING;
        z = (T)0;
        while (state != DONE) {
            switch (state) {
            case TEST_SPLITTING: {
                state = TEST_CONVERGENCE;
                for (l = k; l >= 0; --l) {
                    if (N_::abs_(e[l]) <= eps) break; // e[0] is 0, so l = 0 ends here for every finite input ...
                    if (l == 0) break;                // ... and here where e[0] compares false (a NaN eps): the reference would index q[-1]
                    if (N_::abs_(q[l - 1]) <= eps) {
                        state = CANCELLATION;
                        break;
                    }
                }
                break;
            }
            case CANCELLATION: {
                c = (T)0;
                s = (T)1;
                const int l1 = l - 1;
                state = TEST_CONVERGENCE;
                for (int i = l; i <= k; ++i) {
                    f = s * e[i];
                    {
                        const T ec = e[i] * c;
                        x.solo([=]() { e[i] = ec; });
                    }
                    if (N_::abs_(f) <= eps) break;
                    g = q[i];
                    h = N_::sqrt_(f * f + g * g);
                    {
                        const T hq = h;
                        x.solo([=]() { q[i] = hq; });
                    }
                    c = g / h;
                    s = -f / h;
                    const T cc = c, ss = s;
                    x.rows(0, m, [=](int j) {
                        const T yy = ZG_U(j, l1), zz = ZG_U(j, i);
                        ZG_U(j, l1) = yy * cc + zz * ss;
                        ZG_U(j, i) = -yy * ss + zz * cc;
                    });
                }
                break;
            }
            case TEST_CONVERGENCE: {
                z = q[k];
                if (l == k) {
                    state = CONVERGENCE_CHECK;
                    break;
                }
                iter += 1;
                if (iter > max_iterations) {
                    retval = k;
                    state = DONE;
                    break;
                }
                // shift from the bottom 2 x 2 minor (:401-407)
                x_ = q[l];
                y = q[k - 1];
                g = e[k - 1];
                h = e[k];
                f = ((y - z) * (y + z) + (g - h) * (g + h)) / ((T)2 * h * y);
                g = N_::sqrt_(f * f + (T)1);
                f = ((x_ - z) * (x_ + z) + h * (y / (f < (T)0 ? (f - g) : (f + g)) - h)) / x_;
                // next QR transformation (:410-452)
                c = (T)1;
                s = (T)1;
                for (int i = l + 1; i <= k; ++i) {
                    g = e[i];
                    y = q[i];
                    h = s * g;
                    g *= c;
                    z = N_::sqrt_(f * f + h * h);
                    {
                        const T ze = z;
                        x.solo([=]() { e[i - 1] = ze; });
                    }
                    c = f / z;
                    s = h / z;
                    f = x_ * c + g * s;
                    g = -x_ * s + g * c;
                    h = y * s;
                    y *= c;
                    if (with_v) {
                        const T cc = c, ss = s;
                        x.rows(0, n, [=](int j) {
                            const T xx = ZG_V(j, i - 1), zz = ZG_V(j, i);
                            ZG_V(j, i - 1) = xx * cc + zz * ss;
                            ZG_V(j, i) = -xx * ss + zz * cc;
                        });
                    }
                    z = N_::sqrt_(f * f + h * h);
                    {
                        const T zq = z;
                        x.solo([=]() { q[i - 1] = zq; });
                    }
                    if (z != (T)0) {
                        c = f / z;
                        s = h / z;
                    }
                    f = c * g + s * y;
                    x_ = -s * g + c * y;
                    const T cc = c, ss = s;
                    x.rows(0, m, [=](int j) {
                        const T yy = ZG_U(j, i - 1), zz = ZG_U(j, i);
                        ZG_U(j, i - 1) = yy * cc + zz * ss;
                        ZG_U(j, i) = -yy * ss + zz * cc;
                    });
                }
                {
                    const T fe = f, xq = x_;
                    const int ll = l;
                    x.solo([=]() {
                        e[ll] = (T)0;
                        e[k] = fe;
                        q[k] = xq;
                    });
                }
                state = TEST_SPLITTING;
                break;
            }
            case CONVERGENCE_CHECK: {
                if (z < (T)0) {
                    const T zn = -z;
                    x.solo([=]() { q[k] = zn; });
                    if (with_v) x.rows(0, n, [=](int j) { ZG_V(j, k) = -ZG_V(j, k); });
                }
                state = DONE;
                break;
            }
            default: state = DONE; break;
            }
        }
    }
    // descending order, the columns of U and V with the values (:470-493)
    for (int i = 0; i < n; ++i) {
        int max_idx = i;
        T max_val = q[i];
        for (int j = i + 1; j < n; ++j) {
            if (q[j] > max_val) {
                max_idx = j;
                max_val = q[j];
            }
        }
        if (max_idx != i) {
            x.solo([=]() {
                const T t = q[i];
                q[i] = q[max_idx];
                q[max_idx] = t;
            });
            x.rows(0, m, [=](int row) {
                const T w = ZG_U(row, i);
                ZG_U(row, i) = ZG_U(row, max_idx);
                ZG_U(row, max_idx) = w;
            });
            if (with_v) {
                x.rows(0, n, [=](int row) {
                    const T w = ZG_V(row, i);
                    ZG_V(row, i) = ZG_V(row, max_idx);
                    ZG_V(row, max_idx) = w;
                });
            }
        }
    }
#undef ZG_U
#undef ZG_V
    return retval;
}

// ---- small matrices ------------------------------------------------------------------------------------------------------------------

// SMatrix.gemm(false, other, false, 1.0, 0.0, null) of (AR x AC)(AC x BC), AC <= 3: a zeroed result, an accumulator from 0 in k order,
// result += 1.0 * accumulator. Where the reference build's vector length is at most AC its leading chunk adds p0 + p1 first and then
// 0 + that: the two differ from (0 + p0) + p1 only in the sign of a zero, which the accumulator's own 0 + ... absorbs.
template <int AR, int AC, int BC, typename T> __host__ __device__ inline void gemm_small(const T *a, const T *b, T *out) {
    for (int i = 0; i < AR; ++i) {
        for (int j = 0; j < BC; ++j) {
            T acc = (T)0;
            for (int k = 0; k < AC; ++k) acc += a[i * AC + k] * b[k * BC + j];
            T r = (T)0;
            r += (T)1 * acc;
            out[i * BC + j] = r;
        }
    }
}
template <typename T> __host__ __device__ inline T det2(const T *a) { return a[0] * a[3] - a[1] * a[2]; } // SMatrix.det, rows == 2

// SMatrix.solve of 8 x 8 with one column (SMatrix.zig:729-766): a is the augmented [A | b], 8 rows of 9; false is the reference's null
template <typename T> __host__ __device__ inline bool solve8(T *a, T *xs) {
    typedef Num<T> N_;
    T max_entry = (T)0;
    for (int r = 0; r < 8; ++r)
        for (int c = 0; c < 8; ++c) max_entry = max_(max_entry, N_::abs_(a[r * 9 + c]));
    if (max_entry == (T)0) return false;
    const T tolerance = max_entry * N_::eps() * (T)100;
    for (int c = 0; c < 8; ++c) {
        int pivot = c;
        for (int r = c + 1; r < 8; ++r)
            if (N_::abs_(a[r * 9 + c]) > N_::abs_(a[pivot * 9 + c])) pivot = r;
        if (N_::abs_(a[pivot * 9 + c]) < tolerance) return false;
        if (pivot != c) {
            for (int k = 0; k < 9; ++k) {
                const T t = a[c * 9 + k];
                a[c * 9 + k] = a[pivot * 9 + k];
                a[pivot * 9 + k] = t;
            }
        }
        for (int r = 0; r < 8; ++r) {
            if (r == c) continue;
            const T factor = a[r * 9 + c] / a[c * 9 + c];
            if (factor == (T)0) continue;
            for (int k = c; k < 9; ++k) a[r * 9 + k] -= factor * a[c * 9 + k];
        }
    }
    for (int i = 0; i < 8; ++i) xs[i] = a[i * 9 + 8] / a[i * 9 + i];
    return true;
}

// SMatrix.inv, rows == 3 (SMatrix.zig:702-719); false is the reference's null
template <typename T> __host__ __device__ inline bool inv3(const T *a, T *o) {
    const T c00 = a[4] * a[8] - a[5] * a[7];
    const T c01 = a[2] * a[7] - a[1] * a[8];
    const T c02 = a[1] * a[5] - a[2] * a[4];
    const T d = a[0] * c00 + a[3] * c01 + a[6] * c02;
    if (d == (T)0) return false;
    o[0] = c00 / d;
    o[1] = c01 / d;
    o[2] = c02 / d;
    o[3] = (a[5] * a[6] - a[3] * a[8]) / d;
    o[4] = (a[0] * a[8] - a[2] * a[6]) / d;
    o[5] = (a[2] * a[3] - a[0] * a[5]) / d;
    o[6] = (a[3] * a[7] - a[4] * a[6]) / d;
    o[7] = (a[1] * a[6] - a[0] * a[7]) / d;
    o[8] = (a[0] * a[4] - a[1] * a[3]) / d;
    return true;
}

// project (transforms.zig:39-42, :147-150, :224-231) with m laid out as the record's: matrix.dot(src) is gemm_small's chain
template <typename T> __host__ __device__ inline void project(int kind, const T *m, T px, T py, T &ox, T &oy) {
    T acc, X, Y;
    if (kind == KIND_PROJECTIVE) {
        T W;
        acc = (T)0; acc += m[0] * px; acc += m[1] * py; acc += m[2] * (T)1; X = (T)0; X += (T)1 * acc;
        acc = (T)0; acc += m[3] * px; acc += m[4] * py; acc += m[5] * (T)1; Y = (T)0; Y += (T)1 * acc;
        acc = (T)0; acc += m[6] * px; acc += m[7] * py; acc += m[8] * (T)1; W = (T)0; W += (T)1 * acc;
        if (W != (T)0) {
            const T inv = (T)1 / W;
            X = inv * X;
            Y = inv * Y;
        }
        ox = X;
        oy = Y;
        return;
    }
    acc = (T)0; acc += m[0] * px; acc += m[1] * py; X = (T)0; X += (T)1 * acc;
    acc = (T)0; acc += m[2] * px; acc += m[3] * py; Y = (T)0; Y += (T)1 * acc;
    ox = X + m[4];
    oy = Y + m[5];
}

// Point.orientation(self, b, c) == .collinear (Point.zig:200-210)
template <typename T> __host__ __device__ inline bool collinear3(T ax, T ay, T bx, T by, T cx, T cy) {
    const bool swap = (bx > cx) || (bx == cx && by > cy);
    const T p1x = swap ? cx : bx, p1y = swap ? cy : by, p2x = swap ? bx : cx, p2y = swap ? by : cy;
    const T u = ax * (p1y - p2y) + p1x * (p2y - ay) + p2x * (ay - p1y);
    return u == (T)0;
}

// ---- the fits --------------------------------------------------------------------------------------------------------------------------

// Everything a fit indexes at run time, and what its threads hand one another: LDS on the device.
template <typename T> struct Work {
    T sums[MAX_CHAINS]; // what x.chains leaves
    T slot;             // chain()'s
    T mat[81];          // cov (4), the augmented 8 x 9 system (72), accum (81)
    T u[81], v[9], q[9], e[9];
    T m[9];             // the result
    int status, converged, flag;
};

template <typename T> __host__ __device__ inline void set_identity(int kind, T *m) {
    for (int i = 0; i < 9; ++i) m[i] = (T)0;
    m[0] = (T)1;
    if (kind == KIND_PROJECTIVE) {
        m[4] = (T)1;
        m[8] = (T)1;
    } else {
        m[3] = (T)1;
    }
}

// SimilarityTransform(T).find (transforms.zig:47-112). from, to: n points of (x, y). The result goes to w->m, w->status, w->converged.
template <typename T, typename X> __host__ __device__ inline void find_similarity(X &x, const T *from, const T *to, int n, Work<T> *w) {
    typedef Num<T> N_;
    // mean_from = mean_from.add(from_points[i]) from the origin: four sums of the coordinates themselves (:55-58)
    x.template chains<4>(0, n, [=](int k, int c) { return c < 2 ? from[2 * k + c] : to[2 * k + c - 2]; }, w->sums);
    const T num_points = (T)n;
    const T inv_n = (T)1 / num_points;
    const T mfx = w->sums[0] * inv_n, mfy = w->sums[1] * inv_n, mtx = w->sums[2] * inv_n, mty = w->sums[3] * inv_n; // :59-60
    // sigma_from += from.normSquared(); cov = cov.add(to_mat.dot(from_mat)): the dot's inner dimension is 1, an accumulator 0 + to * from, a
    // result 0 + 1.0 * accumulator (:62-71)
    x.template chains<5>(0, n, [=](int k, int c) {
        const T fx = from[2 * k] - mfx, fy = from[2 * k + 1] - mfy;
        if (c == 0) return fx * fx + fy * fy;
        const T tx = to[2 * k] - mtx, ty = to[2 * k + 1] - mty;
        T acc = (T)0;
        acc += (c <= 2 ? tx : ty) * ((c & 1) ? fx : fy);
        T r = (T)0;
        r += (T)1 * acc;
        return r;
    }, w->sums);
    x.solo([=]() {
        set_identity(KIND_SIMILARITY, w->m);
        w->status = FIT_OK;
        T sigma_from = w->sums[0];
        T *cov = w->mat;
        sigma_from /= num_points;
        for (int i = 0; i < 4; ++i) cov[i] = inv_n * w->sums[1 + i]; // cov.scale(1.0 / num_points)
        const T det_cov = det2(cov);
        Serial one;
        w->converged = svd<T>(one, cov, w->u, 2, 2, SVD_SKINNY_U, w->v, w->q, w->e, true, &w->slot);
        if (w->converged != 0) {
            w->status = FIT_NOT_CONVERGED;
            return;
        }
        const T tol = w->q[0] * N_::eps() * (T)2; // :80
        int effective_rank = 0;
        for (int i = 0; i < 2; ++i)
            if (w->q[i] > tol) effective_rank += 1;
        if (effective_rank == 0) {
            w->status = FIT_RANK_DEFICIENT;
            return;
        }
        T d[4] = {w->q[0], (T)0, (T)0, w->q[1]};
        const T det_u = det2(w->u), det_v = det2(w->v);
        T s[4] = {(T)1, (T)0, (T)0, (T)1};
        if (det_cov < (T)0 || (det_cov == (T)0 && det_u * det_v < (T)0)) {
            if (d[3] < d[0]) s[3] = (T)-1;
            else s[0] = (T)-1;
        }
        T vt[4] = {w->v[0], w->v[2], w->v[1], w->v[3]}, svt[4], r[4], ds[4], rm[2];
        gemm_small<2, 2, 2>(s, vt, svt);
        gemm_small<2, 2, 2>(w->u, svt, r); // :103
        T c = (T)1;
        if (sigma_from != (T)0) {
            gemm_small<2, 2, 2>(d, s, ds);
            T trace = (T)0;
            trace += ds[0];
            trace += ds[3];
            c = (T)1 / sigma_from * trace; // :106
        }
        T m_from[2] = {mfx, mfy};
        gemm_small<2, 2, 1>(r, m_from, rm);
        for (int i = 0; i < 4; ++i) w->m[i] = c * r[i];  // r.scale(c)
        w->m[4] = mtx + (-c) * rm[0];                    // m_to.add(r.dot(m_from).scale(-c))
        w->m[5] = mty + (-c) * rm[1];
    });
}

// Point.areAllCollinear (Point.zig:232-253), n >= 3
template <typename T, typename X> __host__ __device__ inline bool all_collinear(X &x, const T *p, int n) {
    const T p1x = p[0], p1y = p[1];
    const int i = x.first(1, n, [=](int k) { return !(p[2 * k] == p1x && p[2 * k + 1] == p1y); });
    if (i == n) return true;
    const T p2x = p[2 * i], p2y = p[2 * i + 1];
    return x.first(i + 1, n, [=](int k) { return !collinear3(p1x, p1y, p2x, p2y, p[2 * k], p[2 * k + 1]); }) == n;
}

// entry (row, col) of the 2 x 9 matrix b of :272-280: row 0 = [ty f | -tx f | 0], row 1 = [f | 0 | -tx f], f = (fx, fy, 1); scale is
// value * item
template <typename T> __host__ __device__ inline T b_entry(int row, int col, T fx, T fy, T tx, T ty) {
    const int part = col / 3, at = col - part * 3;
    const T f = at == 0 ? fx : (at == 1 ? fy : (T)1);
    if (row == 0) return part == 0 ? ty * f : (part == 1 ? (-tx) * f : (T)0);
    return part == 0 ? f : (part == 1 ? (T)0 : (-tx) * f);
}

// ProjectiveTransform(T).find (transforms.zig:242-290)
// svd_through_x: the 9 x 9 SVD through the executor instead of inside solo: the same operations; the device kernels' choice, where it measured faster
template <typename T, typename X>
__host__ __device__ inline void find_projective(X &x, const T *from, const T *to, int n, Work<T> *w, bool svd_through_x = false) {
    x.solo([=]() {
        set_identity(KIND_PROJECTIVE, w->m);
        w->status = FIT_OK;
        w->converged = 0;
    });
    const bool degenerate = all_collinear(x, from, n) || all_collinear(x, to, n); // the second only when the first is false, on every thread alike
    if (degenerate) {
        x.solo([=]() { w->status = FIT_RANK_DEFICIENT; });
        return;
    }
    if (n == 4) { // :248-269
        x.solo([=]() {
            T *a = w->mat;
            for (int i = 0; i < 4; ++i) {
                const T fx = from[2 * i], fy = from[2 * i + 1], tx = to[2 * i], ty = to[2 * i + 1];
                T *r0 = a + (2 * i) * 9, *r1 = a + (2 * i + 1) * 9;
                r0[0] = fx; r0[1] = fy; r0[2] = (T)1; r0[3] = (T)0; r0[4] = (T)0; r0[5] = (T)0; r0[6] = -tx * fx; r0[7] = -tx * fy; r0[8] = tx;
                r1[0] = (T)0; r1[1] = (T)0; r1[2] = (T)0; r1[3] = fx; r1[4] = fy; r1[5] = (T)1; r1[6] = -ty * fx; r1[7] = -ty * fy; r1[8] = ty;
            }
            if (!solve8(a, w->q)) {
                w->status = FIT_RANK_DEFICIENT;
                return;
            }
            for (int i = 0; i < 8; ++i) w->m[i] = w->q[i];
            w->m[8] = (T)1;
        });
        return;
    }
    // accum = accum.add(b.transpose().dot(b)) (:281): entry (r, c) of the product is 0 + 1.0 * ((0 + b0r b0c) + b1r b1c), and equal to entry
    // (c, r) bit for bit, so the 45 entries with r <= c are summed and mirrored. Chain t is entry (r, c) in row-major order of the upper
    // triangle.
    x.template chains<45>(0, n, [=](int k, int t) {
        int r = 0, rest = t;
        while (rest >= 9 - r) {
            rest -= 9 - r;
            ++r;
        }
        const int c = r + rest;
        const T fx = from[2 * k], fy = from[2 * k + 1], tx = to[2 * k], ty = to[2 * k + 1];
        T acc = (T)0;
        acc += b_entry(0, r, fx, fy, tx, ty) * b_entry(0, c, fx, fy, tx, ty);
        acc += b_entry(1, r, fx, fy, tx, ty) * b_entry(1, c, fx, fy, tx, ty);
        T v = (T)0;
        v += (T)1 * acc;
        return v;
    }, w->sums);
    x.solo([=]() {
        int t = 0;
        for (int r = 0; r < 9; ++r)
            for (int c = r; c < 9; ++c, ++t) w->mat[r * 9 + c] = w->mat[c * 9 + r] = w->sums[t];
    });
    if (svd_through_x) {
        const int converged = svd<T>(x, (const T *)w->mat, w->u, 9, 9, SVD_FULL_U, w->v, w->q, w->e, false, &w->slot);
        x.solo([=]() { w->converged = converged; });
    } else {
        x.solo([=]() {
            Serial one;
            w->converged = svd<T>(one, (const T *)w->mat, w->u, 9, 9, SVD_FULL_U, w->v, w->q, w->e, false, &w->slot); // :283
        });
    }
    x.solo([=]() {
        if (w->converged != 0) {
            w->status = FIT_NOT_CONVERGED;
            return;
        }
        for (int i = 0; i < 9; ++i) w->m[i] = w->u[i * 9 + 8]; // u.col(8).reshape(3, 3)
    });
}

// AffineTransform(T).find (transforms.zig:155-191). big: room for n x 3 values (LDS on the device): the transpose of p, then U of its SVD,
// then the transpose of pinv, row by row in place.
template <typename T, typename X> __host__ __device__ inline void find_affine(X &x, const T *from, const T *to, int n, T *big, Work<T> *w) {
    typedef Num<T> N_;
    x.solo([=]() {
        set_identity(KIND_AFFINE, w->m);
        w->status = FIT_OK;
    });
    x.rows(0, n, [=](int k) { // p.transpose(): row k is (x, y, 1)
        big[3 * k] = from[2 * k];
        big[3 * k + 1] = from[2 * k + 1];
        big[3 * k + 2] = (T)1;
    });
    // Matrix.pinv of 3 x n with n >= 3: the transpose's pinvTall (Matrix.zig:454-460, :463-509)
    const int converged = svd<T>(x, (const T *)nullptr, big, n, 3, SVD_SKINNY_U, w->v, w->q, w->e, true, &w->slot);
    if (converged != 0) {
        x.solo([=]() {
            w->converged = converged;
            w->status = FIT_NOT_CONVERGED;
        });
        return;
    }
    const T sigma_max = w->q[0];
    int effective_rank = 0;
    if (sigma_max != (T)0) {
        const T tol = sigma_max * (T)(n > 3 ? n : 3) * N_::eps(); // :486
        for (int i = 0; i < 3; ++i)
            if (w->q[i] > tol) effective_rank += 1;
        x.solo([=]() { // v_sigma: the columns of V times 1 / sigma, or 0 (:495-502), into mat
            for (int i = 0; i < 3; ++i) {
                const T sigma = w->q[i];
                const T inv_sigma = sigma > tol ? (T)1 / sigma : (T)0;
                for (int r = 0; r < 3; ++r) w->mat[r * 3 + i] = w->v[r * 3 + i] * inv_sigma;
            }
        });
    }
    x.solo([=]() { w->converged = 0; });
    if (effective_rank < 3) { // :174
        x.solo([=]() { w->status = FIT_RANK_DEFICIENT; });
        return;
    }
    // v_sigma.dotTranspose(u), 3 x n, transposed (:508, :460): entry (k, i) = 0 + 1.0 * (((0 + vs[i][0] u[k][0]) + vs[i][1] u[k][1]) + vs[i][2] u[k][2])
    x.rows(0, n, [=](int k) {
        const T u0 = big[3 * k], u1 = big[3 * k + 1], u2 = big[3 * k + 2];
        for (int i = 0; i < 3; ++i) {
            T acc = (T)0;
            acc += w->mat[i * 3] * u0;
            acc += w->mat[i * 3 + 1] * u1;
            acc += w->mat[i * 3 + 2] * u2;
            T r = (T)0;
            r += (T)1 * acc;
            big[3 * k + i] = r;
        }
    });
    // m = q.dot(pinv), 2 x 3 over n terms each (:179): the scalar chain for every n (the departure at n >= 86: DESIGN.md, section 8)
    x.template chains<6>(0, n, [=](int k, int c) { return to[2 * k + c / 3] * big[3 * k + c % 3]; }, w->sums);
    x.solo([=]() {
        T m[6];
        for (int i = 0; i < 6; ++i) {
            T r = (T)0;
            r += (T)1 * w->sums[i];
            m[i] = r;
        }
        w->m[0] = m[0]; w->m[1] = m[1]; w->m[2] = m[3]; w->m[3] = m[4]; // subMatrix(0, 0, 2, 2)
        w->m[4] = m[2]; w->m[5] = m[5];                                  // col(2)
    });
}

// ---- the record ------------------------------------------------------------------------------------------------------------------------

struct Record { // zg_transform_fit, field for field
    int32_t kind, status;
    uint32_t n_points, svd_converged;
    double m64[9];
    float m32[9];
    uint32_t reserved;
};

// .as(f32) of an f64 result (@floatCast), or an f32 result widened
template <typename T> __host__ __device__ inline void to_record(int kind, int status, uint32_t n, int converged, const T *m, Record *r) {
    r->kind = kind;
    r->status = status;
    r->n_points = n;
    r->svd_converged = (uint32_t)converged;
    for (int i = 0; i < 9; ++i) {
        r->m32[i] = (float)m[i];
        r->m64[i] = sizeof(T) == 4 ? (double)(float)m[i] : (double)m[i];
    }
    r->reserved = 0;
}
// a record that reports `status` and the identity
__host__ __device__ inline void failed_record(int kind, int status, uint32_t n, Record *r) {
    double m[9];
    set_identity(kind, m);
    to_record(kind, status, n, 0, m, r);
}

// find for `kind` on n points, n within the kind's bounds; big is read and written by affine alone
template <typename T, typename X> __host__ __device__ inline void find(X &x, int kind, const T *from, const T *to, int n, T *big, Work<T> *w) {
    x.solo([=]() { w->converged = 0; });
    if (kind == KIND_SIMILARITY) find_similarity(x, from, to, n, w);
    else if (kind == KIND_AFFINE) find_affine(x, from, to, n, big, w);
    else find_projective(x, from, to, n, w);
}

// ProjectiveTransform.inv of a record in T (m32 for f32, m64 for f64)
template <typename T> __host__ __device__ inline void invert_record(const Record *in, Record *out) {
    if (in->status != FIT_OK) {
        *out = *in;
        return;
    }
    if (in->kind != KIND_PROJECTIVE) {
        failed_record(in->kind, FIT_BAD_INPUT, in->n_points, out);
        return;
    }
    T a[9], o[9];
    for (int i = 0; i < 9; ++i) a[i] = sizeof(T) == 4 ? (T)in->m32[i] : (T)in->m64[i];
    if (!inv3(a, o)) {
        failed_record(KIND_PROJECTIVE, FIT_RANK_DEFICIENT, in->n_points, out);
        return;
    }
    to_record(KIND_PROJECTIVE, FIT_OK, in->n_points, (int)in->svd_converged, o, out);
}

// project of one point with a record's matrix in T
template <typename T> __host__ __device__ inline void project_record(const Record *r, T px, T py, T &ox, T &oy) {
    T m[9];
    for (int i = 0; i < 9; ++i) m[i] = sizeof(T) == 4 ? (T)r->m32[i] : (T)r->m64[i];
    project(r->kind, m, px, py, ox, oy);
}

} // namespace zg_tf
