// zg_fdm_solve.h — everything of FeatureDistributionMatching (reference src/fdm.zig) between the pixel statistics and the per-pixel map,
// written once for the host and the device: moments to mean and covariance, the Golub-Reinsch SVD of a 3 x 3 f64 matrix as
// SMatrix(f64, 3, 3).svd(.{ .with_v = false, .mode = .skinny_u }) runs it (src/matrix/svd.zig:149-495), and the rest of setTarget and
// update (fdm.zig:92-121, :174-254). It includes nothing of HIP or of the library; a host build defines __host__ and __device__ away.
// Only + - * /, sqrt and fabs on f64, each rounded as written: NO FMA MAY BE FORMED, so every build of this header, the host's too, uses
// -ffp-contract=off (the pragma below says the same to clang).
#pragma once
#include <math.h>
#include <stdint.h>

#if defined(__clang__)
#pragma clang fp contract(off)
#endif

namespace zg_fdm {

enum { ROUTE_COLOR = 0, ROUTE_SCALAR = 1, ROUTE_GRAY_TARGET = 2 };
enum { PIXEL_U8 = 0, PIXEL_RGB_U8 = 2, PIXEL_RGBA_U8 = 3 }; // zg_pixel's ordinals

// ---- (a) exact moments to f64 statistics ---------------------------------------------------------------------------------------------

struct U128 {
    uint64_t hi, lo;
};

__host__ __device__ inline U128 mul_64x64(uint64_t a, uint64_t b) {
    const uint64_t a0 = a & 0xffffffffu, a1 = a >> 32, b0 = b & 0xffffffffu, b1 = b >> 32;
    const uint64_t p00 = a0 * b0, p01 = a0 * b1, p10 = a1 * b0, p11 = a1 * b1;
    const uint64_t mid = (p00 >> 32) + (p01 & 0xffffffffu) + (p10 & 0xffffffffu); // below 3 * 2^32
    U128 r;
    r.lo = (p00 & 0xffffffffu) | (mid << 32);
    r.hi = p11 + (p01 >> 32) + (p10 >> 32) + (mid >> 32);
    return r;
}
__host__ __device__ inline bool less_128(U128 a, U128 b) { return a.hi < b.hi || (a.hi == b.hi && a.lo < b.lo); }
__host__ __device__ inline U128 sub_128(U128 a, U128 b) { // a >= b
    U128 r;
    r.lo = a.lo - b.lo;
    r.hi = a.hi - b.hi - (a.lo < b.lo ? 1u : 0u);
    return r;
}
// the nearest f64 (ties to even) of a 128-bit integer: the top 64 bits with everything below them folded into the lowest one (eleven
// places under the rounding position), converted once, scaled by an exact power of two
__host__ __device__ inline double to_f64_128(U128 v) {
    if (v.hi == 0) return (double)v.lo;
    int shift = 64;
    while (!(v.hi >> 63)) { // the top bit of v lands on bit 63 of m
        v.hi = (v.hi << 1) | (v.lo >> 63);
        v.lo <<= 1;
        --shift;
    }
    const uint64_t m = v.hi | (v.lo != 0 ? 1u : 0u);
    double r = (double)m;
    for (int i = 0; i < shift; ++i) r *= 2.0;
    return r;
}

// (n * sxy - sx * sy) / (65025 * n * (n - 1)): the sample covariance of two byte channels over 255, numerator and denominator exact, each
// rounded once, one division. 0 for n <= 1 (stats.zig:290, :303). n < 2^32, so every product stays below 2^81.
__host__ __device__ inline double cov_from_moments(uint64_t n, uint64_t sx, uint64_t sy, uint64_t sxy) {
    if (n <= 1) return 0.0;
    const U128 a = mul_64x64(n, sxy), b = mul_64x64(sx, sy);
    const bool neg = less_128(a, b);
    const double num = to_f64_128(neg ? sub_128(b, a) : sub_128(a, b));
    const double den = to_f64_128(mul_64x64(n * (n - 1), 65025u));
    const double q = num / den;
    return neg ? -q : q;
}
__host__ __device__ inline double mean_from_moments(uint64_t n, uint64_t sx) { // sx / (255 n), both exact in f64; 0 for no samples (stats.zig:284)
    return n == 0 ? 0.0 : (double)sx / (double)(255u * n);
}
// mean[3] and the symmetric cov[9] from the sums of r, g, b and of rr, rg, rb, gg, gb, bb
__host__ __device__ inline void stats_from_moments(uint64_t n, const uint64_t sum[3], const uint64_t prod[6], double mean[3], double cov[9]) {
    int t = 0;
    for (int i = 0; i < 3; ++i) {
        mean[i] = mean_from_moments(n, sum[i]);
        for (int j = i; j < 3; ++j, ++t) cov[i * 3 + j] = cov[j * 3 + i] = cov_from_moments(n, sum[i], sum[j], prod[t]);
    }
}
// the same for one channel present three times (fdm.zig:77, :152, :161): every mean and every entry of cov is the one value
__host__ __device__ inline void stats_from_scalar_moments(uint64_t n, uint64_t s, uint64_t ss, double mean[3], double cov[9]) {
    const double m = mean_from_moments(n, s), v = cov_from_moments(n, s, s, ss);
    for (int i = 0; i < 3; ++i) mean[i] = m;
    for (int i = 0; i < 9; ++i) cov[i] = v;
}

// ---- (b) svd.kernel for a 3 x 3 f64 matrix, .skinny_u, no V --------------------------------------------------------------------------

// u (row-major) receives U, q the singular values in descending order; e is the kernel's work vector. Returns the reference's
// `converged`: 0, or the index k of the singular value whose QR iteration passed 300 steps. Line numbers are svd.zig's. The arrays are
// indexed by values known only at run time (l, k), so a device caller hands in memory it chose (LDS) and no array lives on the stack.
__host__ __device__ inline int svd3(const double a[9], double u[9], double q[3], double e[3]) {
    const int N = 3;
    const int max_iterations = 300;
    double eps = 2.220446049250313e-16;                      // floatEps(f64)
    const double tol = 2.2250738585072014e-308 / eps;        // floatMin(f64) / eps (:180)
    int l = 0, retval = 0;
    double c, f, g, h, s, x, y, z;
    for (int i = 0; i < 9; ++i) u[i] = a[i];
    for (int i = 0; i < N; ++i) q[i] = e[i] = 0.0;
#define ZG_U(r, cc) u[(r) * 3 + (cc)]
    // Householder's reduction to bidiagonal form (:201-264)
    g = 0.0;
    x = 0.0;
    for (int i = 0; i < N; ++i) {
        e[i] = g;
        s = 0.0;
        l = i + 1;
        for (int j = i; j < N; ++j) s += ZG_U(j, i) * ZG_U(j, i);
        if (s < tol) {
            g = 0.0;
        } else {
            f = ZG_U(i, i);
            g = f < 0.0 ? sqrt(s) : -sqrt(s); // :216
            h = f * g - s;
            ZG_U(i, i) = f - g;
            for (int j = l; j < N; ++j) {
                s = 0.0;
                for (int k = i; k < N; ++k) s += ZG_U(k, i) * ZG_U(k, j);
                f = s / h;
                for (int k = i; k < N; ++k) ZG_U(k, j) += f * ZG_U(k, i);
            }
        }
        q[i] = g;
        s = 0.0;
        for (int j = l; j < N; ++j) s += ZG_U(i, j) * ZG_U(i, j);
        if (s < tol) { // always for i = 2: the sum is empty
            g = 0.0;
        } else {
            f = ZG_U(i, i + 1);
            g = f < 0.0 ? sqrt(s) : -sqrt(s); // :244
            h = f * g - s;
            ZG_U(i, i + 1) = f - g;
            for (int j = l; j < N; ++j) e[j] = ZG_U(i, j) / h;
            for (int j = l; j < N; ++j) {
                s = 0.0;
                for (int k = l; k < N; ++k) s += ZG_U(j, k) * ZG_U(i, k);
                for (int k = l; k < N; ++k) ZG_U(j, k) += s * e[k];
            }
        }
        y = fabs(q[i]) + fabs(e[i]);
        x = (y > x || x != x) ? y : x; // @max(x, y): the other operand when one is NaN
    }
    // accumulation of left-hand transformations (:307-338); u is 3 x 3, so the loops of :297-305 are empty
    for (int i = N - 1; i >= 0; --i) {
        l = i + 1;
        g = q[i];
        for (int j = l; j < N; ++j) ZG_U(i, j) = 0.0;
        if (g != 0.0) {
            h = ZG_U(i, i) * g;
            for (int j = l; j < N; ++j) {
                s = 0.0;
                for (int k = l; k < N; ++k) s += ZG_U(k, i) * ZG_U(k, j);
                f = s / h;
                for (int k = i; k < N; ++k) ZG_U(k, j) += f * ZG_U(k, i);
            }
            for (int j = i; j < N; ++j) ZG_U(j, i) /= g;
        } else {
            for (int j = i; j < N; ++j) ZG_U(j, i) = 0.0;
        }
        ZG_U(i, i) += 1.0;
    }
    // diagonalization of the bidiagonal form (:341-468)
    eps *= x;
    for (int k = N - 1; k >= 0; --k) {
        int iter = 0;
        enum { TEST_SPLITTING, CANCELLATION, TEST_CONVERGENCE, CONVERGENCE_CHECK, DONE } state = TEST_SPLITTING;
        z = 0.0;
        while (state != DONE) {
            switch (state) {
            case TEST_SPLITTING: {
                state = TEST_CONVERGENCE;
                for (l = k; l >= 0; --l) {
                    if (fabs(e[l]) <= eps) break; // e[0] is 0, so l = 0 ends here for every finite input ...
                    if (l == 0) break;            // ... and here where e[0] compares false (a NaN eps): the reference would index q[-1]
                    if (fabs(q[l - 1]) <= eps) {
                        state = CANCELLATION;
                        break;
                    }
                }
                if (l < 0) l = 0;
                break;
            }
            case CANCELLATION: {
                c = 0.0;
                s = 1.0;
                const int l1 = l - 1;
                state = TEST_CONVERGENCE;
                for (int i = l; i <= k; ++i) {
                    f = s * e[i];
                    e[i] *= c;
                    if (fabs(f) <= eps) break;
                    g = q[i];
                    h = sqrt(f * f + g * g);
                    q[i] = h;
                    c = g / h;
                    s = -f / h;
                    for (int j = 0; j < N; ++j) {
                        y = ZG_U(j, l1);
                        z = ZG_U(j, i);
                        ZG_U(j, l1) = y * c + z * s;
                        ZG_U(j, i) = -y * s + z * c;
                    }
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
                x = q[l];
                y = q[k - 1];
                g = e[k - 1];
                h = e[k];
                f = ((y - z) * (y + z) + (g - h) * (g + h)) / (2.0 * h * y);
                g = sqrt(f * f + 1.0);
                f = ((x - z) * (x + z) + h * (y / (f < 0.0 ? (f - g) : (f + g)) - h)) / x;
                // next QR transformation (:410-452)
                c = 1.0;
                s = 1.0;
                for (int i = l + 1; i <= k; ++i) {
                    g = e[i];
                    y = q[i];
                    h = s * g;
                    g *= c;
                    z = sqrt(f * f + h * h);
                    e[i - 1] = z;
                    c = f / z;
                    s = h / z;
                    f = x * c + g * s;
                    g = -x * s + g * c;
                    h = y * s;
                    y *= c;
                    z = sqrt(f * f + h * h);
                    q[i - 1] = z;
                    if (z != 0.0) {
                        c = f / z;
                        s = h / z;
                    }
                    f = c * g + s * y;
                    x = -s * g + c * y;
                    for (int j = 0; j < N; ++j) {
                        y = ZG_U(j, i - 1);
                        z = ZG_U(j, i);
                        ZG_U(j, i - 1) = y * c + z * s;
                        ZG_U(j, i) = -y * s + z * c;
                    }
                }
                e[l] = 0.0;
                e[k] = f;
                q[k] = x;
                state = TEST_SPLITTING;
                break;
            }
            case CONVERGENCE_CHECK: {
                if (z < 0.0) q[k] = -z;
                state = DONE;
                break;
            }
            default: state = DONE; break;
            }
        }
    }
    // descending order, U's columns with the values (:470-493)
    for (int i = 0; i < N; ++i) {
        int max_idx = i;
        double max_val = q[i];
        for (int j = i + 1; j < N; ++j) {
            if (q[j] > max_val) {
                max_idx = j;
                max_val = q[j];
            }
        }
        if (max_idx != i) {
            const double t = q[i];
            q[i] = q[max_idx];
            q[max_idx] = t;
            for (int row = 0; row < N; ++row) {
                const double w = ZG_U(row, i);
                ZG_U(row, i) = ZG_U(row, max_idx);
                ZG_U(row, max_idx) = w;
            }
        }
    }
#undef ZG_U
    return retval;
}

// ---- (c) setTarget and update between the statistics and the pixels ------------------------------------------------------------------

// Matrix.dot of two 3 x 3 matrices: gemm(false, other, false, 1.0, 0.0, null) on 27 operations takes the scalar loop (Matrix.zig:806-817):
// a zeroed result, an accumulator from 0 in k order, result += 1.0 * accumulator.
__host__ __device__ inline void dot3(const double a[9], const double b[9], double out[9]) {
    for (int i = 0; i < 3; ++i) {
        for (int j = 0; j < 3; ++j) {
            double acc = 0.0;
            for (int k = 0; k < 3; ++k) acc += a[i * 3 + k] * b[k * 3 + j];
            double r = 0.0;
            r += 1.0 * acc;
            out[i * 3 + j] = r;
        }
    }
}

struct Target { // what setTarget keeps (fdm.zig:29-32)
    double mean[3];
    double u[9]; // zeros for a grey target, whose U the reference leaves empty
    double s[3];
    int is_gray;
    int status; // 0, or the SVD's k: error.NotConverged (fdm.zig:113-115)
};
struct Transform { // what update applies to every pixel
    int route;
    int status; // 0, or why the frame stays as it is: the target's status, or the source SVD's k (fdm.zig:210-212)
    double w[9];
    double bias[3];
    double scale, offset;
};
struct Scratch { // the matrices update allocates, and the SVD's work vector
    double us[9], ss[3], e[3], sigma[9], ut_t[9], w_temp[9];
};

// setTarget from the statistics (fdm.zig:92-121). is_gray: the frame is u8, or no pixel had r != g or g != b.
__host__ __device__ inline void target_from_stats(const double mean[3], const double cov[9], int is_gray, Target *t, Scratch *k) {
    for (int i = 0; i < 3; ++i) t->mean[i] = mean[i];
    t->is_gray = is_gray ? 1 : 0;
    t->status = 0;
    if (is_gray) {
        t->s[0] = cov[0];
        t->s[1] = 0.0;
        t->s[2] = 0.0;
        for (int i = 0; i < 9; ++i) t->u[i] = 0.0;
    } else {
        t->status = svd3(cov, t->u, t->s, k->e);
    }
}

// update from the source's statistics (fdm.zig:174-254). For the two scalar routes (a u8 frame, or a grey target) mean[0] and cov[0] are
// those of the byte, resp. of the luminance byte convertColor(u8, pixel).
__host__ __device__ inline void transform_from_stats(int pixel, const Target *t, const double mean[3], const double cov[9], Transform *x, Scratch *k) {
    x->route = pixel == PIXEL_U8 ? ROUTE_SCALAR : (t->is_gray ? ROUTE_GRAY_TARGET : ROUTE_COLOR);
    x->status = t->status;
    for (int i = 0; i < 9; ++i) x->w[i] = 0.0;
    for (int i = 0; i < 3; ++i) x->bias[i] = 0.0;
    x->scale = 1.0;
    x->offset = 0.0;
    if (x->status != 0) return;
    if (x->route != ROUTE_COLOR) {
        const double source_var = cov[0];
        x->scale = source_var > 1e-10 ? sqrt(t->s[0] / source_var) : 1.0; // :181
        x->offset = t->mean[0] - mean[0] * x->scale;                       // :182
        return;
    }
    double *us = k->us, *ss = k->ss, *sigma = k->sigma, *ut_t = k->ut_t, *w_temp = k->w_temp;
    x->status = svd3(cov, us, ss, k->e);
    if (x->status != 0) return;
    for (int i = 0; i < 9; ++i) sigma[i] = 0.0;
    for (int i = 0; i < 3; ++i) {
        if (ss[i] > 1e-10) sigma[i * 3 + i] = sqrt(t->s[i] / ss[i]); // :222-224
    }
    for (int i = 0; i < 3; ++i) {
        for (int j = 0; j < 3; ++j) ut_t[i * 3 + j] = t->u[j * 3 + i];
    }
    dot3(us, sigma, w_temp); // :234
    dot3(w_temp, ut_t, x->w); // :238
    for (int j = 0; j < 3; ++j) { // :247-254
        double sum = 0.0;
        for (int k = 0; k < 3; ++k) sum += mean[k] * x->w[k * 3 + j];
        x->bias[j] = t->mean[j] - sum;
    }
}

// ---- the per-pixel tail, shared so that a table built on the host and the device kernel round alike -----------------------------------

// @round(255.0 * clamp(v, 0, 1)) as a byte (fdm.zig:187-188, :268-270). std.math.clamp is @max(0, @min(v, 1)) and returns the other operand
// for a NaN: 1. 255 * c is in [0, 255], where trunc and a compare give round-half-away-from-zero exactly.
__host__ __device__ inline uint8_t unit_to_byte(double v) {
    const double c = v != v ? 1.0 : (v < 0.0 ? 0.0 : (v > 1.0 ? 1.0 : v));
    const double p = 255.0 * c;
    const int t = (int)p;
    return (uint8_t)(t + ((p - (double)t) >= 0.5 ? 1 : 0));
}
__host__ __device__ inline uint8_t scalar_map(uint8_t byte, double scale, double offset) {
    const double val = (double)byte / 255.0;
    return unit_to_byte(val * scale + offset);
}

} // namespace zg_fdm
