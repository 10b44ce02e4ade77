// zg_qr_geom.h — the arithmetic of the QR detector (reference src/qrcode/detector.zig:210-641, decoder.readVersion) that has to match
// the reference bit for bit, with no device code in it: qr.hip includes it for the kernels, tests/c/qr_geom.cpp for plain g++ under
// ASan/UBSan. Built with -ffp-contract=off; f32 and f64 sqrt and / are correctly rounded on both sides. Every f32 step is one
// operation in the reference's order. Integers are u32: a frame has fewer than 2^31 pixels, so every run length and sum fits.
#pragma once
#include <math.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define ZG_QR_HD __host__ __device__ inline
#else
#define ZG_QR_HD inline
#endif

namespace zg {
namespace qr {

struct Finder { float x, y, ms, hits; }; // centre (x = column, y = row), module size, merged hits

constexpr float SCAN_TOL = 0.5f, CROSS_TOL = 0.7f, DIAG_TOL = 0.8f;

// checkRatio (:210-223)
ZG_QR_HD bool check_ratio(const uint32_t runs[5], float tolerance) {
    uint32_t total = 0;
    for (int i = 0; i < 5; ++i) {
        if (runs[i] == 0) return false;
        total += runs[i];
    }
    if (total < 7) return false;
    const float unit = (float)total / 7.0f;
    for (int i = 0; i < 5; ++i) {
        const float expected = i == 2 ? 3.0f : 1.0f;
        const float width = (float)runs[i];
        const float eu = expected * unit;
        if (fabsf(width - eu) > eu * tolerance) return false;
    }
    return true;
}

// Cross.center (:265-268)
ZG_QR_HD float cross_center(uint32_t base, uint32_t forward, uint32_t total) { return (float)(base + 1u + forward) - (float)total / 2.0f; }

ZG_QR_HD float dist(const Finder &a, const Finder &b) {
    const float dx = a.x - b.x, dy = a.y - b.y;
    return sqrtf(dx * dx + dy * dy);
}

ZG_QR_HD const Finder &pick(int i, const Finder &a, const Finder &b, const Finder &c) { return i == 0 ? a : (i == 1 ? b : c); }

// One (a, b, c) of pickFinderTriple's loops (:348-389): false where the reference `continue`s; else the score and which of the three
// is the corner (top left), the top right and the bottom left.
ZG_QR_HD bool triple_score(const Finder &a, const Finder &b, const Finder &c, float *score, int order[3]) {
    const float ms_max = fmaxf(a.ms, fmaxf(b.ms, c.ms));
    const float ms_min = fminf(a.ms, fminf(b.ms, c.ms));
    if (ms_max > 1.6f * ms_min) return false;
    const float ms = (a.ms + b.ms + c.ms) / 3.0f;
    const float ab = dist(a, b), ac = dist(a, c), bc = dist(b, c);
    int ic = 2, i1 = 0, i2 = 1;
    if (bc >= ab && bc >= ac) {
        ic = 0; i1 = 1; i2 = 2;
    } else if (ac >= ab && ac >= bc) {
        ic = 1; i1 = 0; i2 = 2;
    }
    const Finder &fc = pick(ic, a, b, c), &f1 = pick(i1, a, b, c), &f2 = pick(i2, a, b, c);
    const float v1x = f1.x - fc.x, v1y = f1.y - fc.y;
    const float v2x = f2.x - fc.x, v2y = f2.y - fc.y;
    const float len1 = sqrtf(v1x * v1x + v1y * v1y), len2 = sqrtf(v2x * v2x + v2y * v2y);
    if (fminf(len1, len2) < 10.0f * ms) return false;
    const float imbalance = fabsf(len1 - len2) / fmaxf(len1, len2);
    if (imbalance > 0.35f) return false;
    const float cosv = (v1x * v2x + v1y * v2y) / (len1 * len2);
    if (fabsf(cosv) > 0.35f) return false;
    const bool pos = v1x * v2y - v1y * v2x > 0.0f;
    order[0] = ic;
    order[1] = pos ? i1 : i2;
    order[2] = pos ? i2 : i1;
    *score = (ms_max - ms_min) / ms + imbalance + fabsf(cosv);
    return true;
}

ZG_QR_HD float triple_module_size(const Finder &tl, const Finder &tr, const Finder &bl) { return (tl.ms + tr.ms + bl.ms) / 3.0f; }

// estimateVersion (:400-406). @round is roundf (ties away from zero). The value is finite: module sizes are at least 1.
ZG_QR_HD uint32_t estimate_version(const Finder &tl, const Finder &tr, const Finder &bl) {
    const float side = (dist(tl, tr) + dist(tl, bl)) / 2.0f;
    const float dim_est = side / triple_module_size(tl, tr, bl) + 7.0f;
    float version = roundf((dim_est - 17.0f) / 4.0f);
    version = version < 1.0f ? 1.0f : (version > 40.0f ? 40.0f : version);
    return (uint32_t)version;
}

// nearModule (:510-512)
ZG_QR_HD bool near_module(uint32_t len, float expected) { return fabsf((float)len - expected) <= expected * 0.6f; }

// Point.orientation(...) == .collinear (Point.zig:200-214), with its sorted operands
ZG_QR_HD bool collinear3(const double s[2], const double b[2], const double c[2]) {
    const bool swap = b[0] > c[0] || (b[0] == c[0] && b[1] > c[1]);
    const double *p1 = swap ? c : b, *p2 = swap ? b : c;
    const double u = s[0] * (p1[1] - p2[1]) + p1[0] * (p2[1] - s[1]) + p2[0] * (s[1] - p1[1]);
    return u == 0.0;
}

// Point.areAllCollinear (Point.zig:232-253) of four points
ZG_QR_HD bool all_collinear4(const double p[4][2]) {
    int i = 1;
    while (i < 4 && p[i][0] == p[0][0] && p[i][1] == p[0][1]) ++i;
    if (i == 4) return true;
    for (int k = i + 1; k < 4; ++k)
        if (!collinear3(p[0], p[i], p[k])) return false;
    return true;
}

// SMatrix(f64, 8, 8).solve of one column (SMatrix.zig:729-766): a is the augmented [A | b]; false is the reference's null.
ZG_QR_HD bool solve8(double a[8][9], double x[8]) {
    double max_entry = 0.0;
    for (int r = 0; r < 8; ++r)
        for (int c = 0; c < 8; ++c) max_entry = fmax(max_entry, fabs(a[r][c]));
    if (max_entry == 0.0) return false;
    const double tolerance = max_entry * 2.220446049250313e-16 * 100.0;
    for (int c = 0; c < 8; ++c) {
        int pivot = c;
        for (int r = c + 1; r < 8; ++r)
            if (fabs(a[r][c]) > fabs(a[pivot][c])) pivot = r;
        if (fabs(a[pivot][c]) < tolerance) return false;
        if (pivot != c)
            for (int k = 0; k < 9; ++k) {
                const double t = a[c][k];
                a[c][k] = a[pivot][k];
                a[pivot][k] = t;
            }
        for (int r = 0; r < 8; ++r) {
            if (r == c) continue;
            const double factor = a[r][c] / a[c][c];
            if (factor == 0.0) continue;
            for (int k = c; k < 9; ++k) a[r][k] -= factor * a[c][k];
        }
    }
    for (int i = 0; i < 8; ++i) x[i] = a[i][8] / a[i][i];
    return true;
}

// ProjectiveTransform(f64).init with four correspondences (transforms.zig:242-268): m is the 3 x 3 matrix, row-major; a is the
// caller's room for the augmented system (LDS on the device, where a lane's own array would be scratch memory).
ZG_QR_HD bool projective4(const double from[4][2], const double to[4][2], double a[8][9], double m[9]) {
    if (all_collinear4(from) || all_collinear4(to)) return false;
    for (int i = 0; i < 4; ++i) {
        const double fx = from[i][0], fy = from[i][1], tx = to[i][0], ty = to[i][1];
        double *r0 = a[2 * i], *r1 = a[2 * i + 1];
        r0[0] = fx; r0[1] = fy; r0[2] = 1.0; r0[3] = 0.0; r0[4] = 0.0; r0[5] = 0.0; r0[6] = -tx * fx; r0[7] = -tx * fy; r0[8] = tx;
        r1[0] = 0.0; r1[1] = 0.0; r1[2] = 0.0; r1[3] = fx; r1[4] = fy; r1[5] = 1.0; r1[6] = -ty * fx; r1[7] = -ty * fy; r1[8] = ty;
    }
    if (!solve8(a, m)) return false;
    m[8] = 1.0;
    return true;
}

// buildTransform (:417-435): the three finder centres and a fourth correspondence. pts (two sets of four points) and a are the caller's
// room, as in projective4.
ZG_QR_HD bool build_transform(const Finder &tl, const Finder &tr, const Finder &bl, float fx, float fy, bool is_alignment, uint32_t dim, double pts[2][4][2],
                              double a[8][9], double m[9]) {
    const double d = (double)dim;
    const double module = is_alignment ? d - 6.5 : d - 3.5;
    double(*from)[2] = pts[0], (*to)[2] = pts[1];
    from[0][0] = 3.5; from[0][1] = 3.5;
    from[1][0] = d - 3.5; from[1][1] = 3.5;
    from[2][0] = 3.5; from[2][1] = d - 3.5;
    from[3][0] = module; from[3][1] = module;
    to[0][0] = (double)tl.x; to[0][1] = (double)tl.y;
    to[1][0] = (double)tr.x; to[1][1] = (double)tr.y;
    to[2][0] = (double)bl.x; to[2][1] = (double)bl.y;
    to[3][0] = (double)fx; to[3][1] = (double)fy;
    return projective4(from, to, a, m);
}

// ProjectiveTransform.project (transforms.zig:224-231): the product's rows are ((m0 x + m1 y) + m2 1), then a scale by 1 / w
ZG_QR_HD void project(const double m[9], double x, double y, double *ox, double *oy) {
    double px = (m[0] * x + m[1] * y) + m[2] * 1.0;
    double py = (m[3] * x + m[4] * y) + m[5] * 1.0;
    const double w = (m[6] * x + m[7] * y) + m[8] * 1.0;
    if (w != 0.0) {
        const double s = 1.0 / w;
        px = px * s;
        py = py * s;
    }
    *ox = px;
    *oy = py;
}

// timingOk (:624-641)
ZG_QR_HD bool timing_ok(const uint8_t *modules, uint32_t dim) {
    const uint32_t lines[2] = {6u, dim - 7u};
    uint32_t row_best = 0, col_best = 0;
    for (int l = 0; l < 2; ++l) {
        const uint32_t line = lines[l];
        uint32_t row_match = 0, col_match = 0;
        for (uint32_t i = 8; i < dim - 8u; ++i) {
            const uint8_t expected = i % 2u == 0u ? 1 : 0;
            if (modules[line * dim + i] == expected) ++row_match;
            if (modules[i * dim + line] == expected) ++col_match;
        }
        row_best = row_match > row_best ? row_match : row_best;
        col_best = col_match > col_best ? col_match : col_best;
    }
    const uint32_t needed = (dim - 16u) * 3u / 4u;
    return row_best >= needed && col_best >= needed;
}

// tables.bchRemainder (tables.zig:226-235)
ZG_QR_HD uint32_t bch_remainder(uint32_t data, uint32_t generator, uint32_t total_bits, uint32_t data_bits) {
    const uint32_t gen_degree = total_bits - data_bits;
    uint32_t rem = data << gen_degree;
    uint32_t bit = total_bits;
    while (bit > gen_degree) {
        --bit;
        if ((rem >> bit) & 1u) rem ^= generator << (bit - gen_degree);
    }
    return rem;
}

// the version information codeword of version v in 7 .. 40 (tables.zig:254-261)
ZG_QR_HD uint32_t version_codeword(uint32_t v) { return v << 12 | bch_remainder(v, 0x1f25u, 18u, 6u); }

// decoder.orientedModule (decoder.zig:118-128)
ZG_QR_HD uint8_t oriented_module(const uint8_t *modules, uint32_t dim, uint32_t orientation, uint32_t row, uint32_t col) {
    uint32_t r = row, c = col;
    if (orientation & 4u) {
        r = col;
        c = row;
    }
    switch (orientation & 3u) {
    case 0: return modules[r * dim + c];
    case 1: return modules[(dim - 1u - c) * dim + r];
    case 2: return modules[(dim - 1u - r) * dim + (dim - 1u - c)];
    default: return modules[c * dim + (dim - 1u - r)];
    }
}

// decoder.readVersion (decoder.zig:147-162): the version, or -1. Ties go to the first orientation and the first codeword.
ZG_QR_HD int read_version(const uint8_t *modules, uint32_t dim) {
    uint32_t best_distance = 4;
    int best_index = -1;
    for (uint32_t orientation = 0; orientation < 8; ++orientation) {
        uint32_t codeword = 0;
        for (uint32_t i = 0; i < 6; ++i)
            for (uint32_t j = 0; j < 3; ++j) codeword |= (uint32_t)oriented_module(modules, dim, orientation, dim - 11u + j, i) << (3u * i + j);
        for (uint32_t index = 0; index < 34; ++index) {
            uint32_t x = codeword ^ version_codeword(index + 7u), distance = 0;
            while (x) {
                x &= x - 1u;
                ++distance;
            }
            if (distance < best_distance) {
                best_distance = distance;
                best_index = (int)index;
            }
        }
    }
    return best_index < 0 ? -1 : best_index + 7;
}

} // namespace qr
} // namespace zg
