// orb.hip — Orb.detect / compute / detectAndCompute (reference src/features/orb.zig:119-276, 336-517) on the device, bit for bit.
//
// One call enqueues, with no host synchronisation and no copy back:
//   zg_pyramid_build        the levels the call uses, into scratch
//   fast_detect_compact     FAST (adaptive threshold, NMS, arc 9) on every level with a share of the budget: the reference's list per
//                           level as 8-byte entries (pixel index, integer score), sized for every candidate of the level
//   k_orb_harris            [harris_score] the list's scores replaced by computeHarrisResponse (:460-508) in its order-preserving form
//   k_orb_hist x <= 8       a level with more corners than its share: radix select, a byte per launch, of the n_desired smallest of the
//                           unique 64-bit keys (~response key) << 32 | list index — descending response, ties in list order, which is
//                           what the reference's stable sort of the list keeps (:186-190). Every workgroup re-derives the digits
//                           chosen so far from the earlier launches' histograms; bytes that are the same for every entry are skipped
//   k_orb_gather            the survivors (key <= the selected one), in any order
//   k_orb_orient            a lane per selected corner: its rank among the survivors (a level within its share keeps list order,
//                           :185), the border filter (:194-205), the intensity centroid (:398-426) summed in raster order by that
//                           one lane, coordinates scaled to the source (:209-214)
//   k_orb_compact           the levels' survivors of the border filter in ascending level order into the caller's array, the count
//   k_orb_describe          a wave per keypoint: rotated BRIEF (:429-457), lane l tests pairs l, 64 + l, 128 + l, 192 + l, and four
//                           ballots are the descriptor's four little-endian words
// Scratch, worst case, with S = sum over the levels of 1 / scale^2 (3.2 at the defaults): S - 1 bytes per source pixel of level images,
// 8 S of FAST list, FAST's own 2 S of score map and about S / 100 of cell counts: 35 bytes per source pixel at the defaults.
#include "zg_internal.h"
#include "zg_devmath.h"
#include "zg_hostmath.h"
#include "zg_scan.h"

#include <algorithm>
#include <cmath>
#include <vector>

#pragma clang fp contract(off)

namespace zg {
namespace {

constexpr int ORB_MAX_LEVELS = 32;
constexpr int PATCH = 31, HALF = 15; // DEFAULT_PATCH_SIZE (:15)
constexpr float PYRAMID_SIGMA = 1.6f; // :125

// The 256 sampling pairs of the ORB descriptor (Rublee et al. 2011), x1, y1, x2, y2 per pair, 8 pairs a line.
__constant__ int8_t ORB_PAIRS[256 * 4] = {
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
};

struct OrbJob { // a level that detects
    const uint8_t *img;
    uint64_t stride;
    uint32_t *pos, *key; // FAST's list of the level: pixel index row * cols + col, response key
    int32_t rows, cols;
    float scale, margin;
    uint32_t nd;         // the level's share (n_desired)
    uint32_t sel_off;    // its first slot in sel / tmp, min(nd, candidates) of them
    uint32_t cand;       // list capacity = number of candidates
    int32_t octave;
};
struct OrbArgs {
    OrbJob job[ORB_MAX_LEVELS];
    int32_t n;
    int32_t harris;
    uint32_t *counts;    // [n] list lengths
    uint32_t *hist;      // [n][8][256], zeroed before the call
    uint32_t *sel_n;     // [n], zeroed
    uint64_t *sel;
    zg_keypoint *tmp;
    const float *weights; // the caller's table, or null
    zg_keypoint *out;
    uint32_t capacity;
    uint32_t *count;
};
struct OrbPyramid {
    const uint8_t *img[ORB_MAX_LEVELS];
    uint64_t stride[ORB_MAX_LEVELS];
    int32_t rows[ORB_MAX_LEVELS], cols[ORB_MAX_LEVELS];
    float scale[ORB_MAX_LEVELS];
    int32_t n_levels;
};

// f32 <-> u32 with the same order (no NaN reaches it: the responses are sums and products of finite values)
__device__ inline uint32_t order_key(float f) {
    const uint32_t u = __float_as_uint(f == 0.0f ? 0.0f : f);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ inline float key_response(uint32_t k, int harris) {
    if (!harris) return (float)k;
    return __uint_as_float((k & 0x80000000u) ? (k ^ 0x80000000u) : ~k);
}

// ---- Harris --------------------------------------------------------------------------------------------------------
__device__ inline float harris_response(const OrbJob &J, int x, int y) { // :460-508
    float ixx = 0.0f, iyy = 0.0f, ixy = 0.0f;
    for (int dy = 0; dy < 7; ++dy) {
        const int yy = y + dy - 3;
        if (yy <= 0 || yy >= J.rows - 1) continue;
        const uint8_t *r0 = J.img + (size_t)(yy - 1) * J.stride, *r1 = r0 + J.stride, *r2 = r1 + J.stride;
        for (int dx = 0; dx < 7; ++dx) {
            const int xx = x + dx - 3;
            if (xx <= 0 || xx >= J.cols - 1) continue;
            const int gx = (int)r0[xx + 1] - (int)r0[xx - 1] + 2 * ((int)r1[xx + 1] - (int)r1[xx - 1]) + (int)r2[xx + 1] - (int)r2[xx - 1];
            const int gy = (int)r2[xx - 1] - (int)r0[xx - 1] + 2 * ((int)r2[xx] - (int)r0[xx]) + (int)r2[xx + 1] - (int)r0[xx + 1];
            const float fx = (float)gx / 8.0f, fy = (float)gy / 8.0f;
            ixx += fx * fx;
            iyy += fy * fy;
            ixy += fx * fy;
        }
    }
    const float det = ixx * iyy - ixy * ixy;
    const float trace = ixx + iyy;
    return det - 0.04f * trace * trace;
}

__global__ __launch_bounds__(256) void k_orb_harris(OrbArgs a) {
    const OrbJob &J = a.job[blockIdx.y];
    const uint32_t n = min(a.counts[blockIdx.y], J.cand);
    for (uint32_t i = blockIdx.x * 256u + threadIdx.x; i < n; i += gridDim.x * 256u) {
        const uint32_t p = J.pos[i];
        J.key[i] = order_key(harris_response(J, (int)(p % (uint32_t)J.cols), (int)(p / (uint32_t)J.cols)));
    }
}

// ---- selection -----------------------------------------------------------------------------------------------------
// Byte `pass` (0 = the highest) of every key of the level when it is known without looking: FAST scores are below 2^16, list
// indices below the candidate count. -1: it has to be counted.
__device__ __host__ inline int fixed_digit(int harris, uint32_t cand, int pass) {
    if (!harris && pass < 2) return 0xFF;
    if (pass == 4 && cand <= (1u << 24)) return 0;
    if (pass == 5 && cand <= (1u << 16)) return 0;
    if (pass == 6 && cand <= (1u << 8)) return 0;
    return -1;
}
__device__ inline uint64_t select_key(const OrbJob &J, uint32_t i) { return ((uint64_t)(~J.key[i]) << 32) | i; }

// The digits chosen by passes 0 .. upto - 1 (as a prefix) and how many of the entries under that prefix are still wanted; every
// thread of the workgroup calls it, wave 0 works it out: lane l holds bins 4l .. 4l + 3 of a pass's histogram.
__device__ inline void select_state(const OrbArgs &a, int j, int upto, uint64_t *s_prefix, uint32_t *s_k) {
    if (threadIdx.x < 64) {
        const OrbJob &J = a.job[j];
        const int lane = (int)threadIdx.x;
        uint64_t prefix = 0;
        uint32_t k = J.nd;
        for (int q = 0; q < upto; ++q) {
            uint32_t d;
            const int fd = fixed_digit(a.harris, J.cand, q);
            if (fd >= 0) {
                d = (uint32_t)fd;
            } else {
                const uint32_t *h = a.hist + ((size_t)j * 8 + q) * 256 + 4 * lane;
                const uint32_t v0 = h[0], v1 = h[1], v2 = h[2], v3 = h[3];
                const uint32_t sum = v0 + v1 + v2 + v3, incl = wave_inclusive_sum(sum);
                const uint64_t reach = __ballot(incl >= k);
                const int first = reach ? __ffsll((long long)reach) - 1 : 63; // reach != 0: the entries under the prefix are at least k
                uint32_t kk = k - __shfl(incl - sum, first);
                const uint32_t w0 = __shfl(v0, first), w1 = __shfl(v1, first), w2 = __shfl(v2, first);
                d = 4u * (uint32_t)first;
                if (kk > w0) {
                    kk -= w0; ++d;
                    if (kk > w1) {
                        kk -= w1; ++d;
                        if (kk > w2) { kk -= w2; ++d; }
                    }
                }
                k = kk;
            }
            prefix = (prefix << 8) | d;
        }
        if (lane == 0) { *s_prefix = prefix; *s_k = k; }
    }
    __syncthreads();
}

__global__ __launch_bounds__(256) void k_orb_hist(OrbArgs a, int pass) {
    const int j = (int)blockIdx.y;
    const OrbJob &J = a.job[j];
    const uint32_t n = min(a.counts[j], J.cand);
    if (n <= J.nd || fixed_digit(a.harris, J.cand, pass) >= 0) return; // uniform
    __shared__ uint32_t h[256];
    __shared__ uint64_t s_prefix;
    __shared__ uint32_t s_k;
    h[threadIdx.x] = 0;
    select_state(a, j, pass, &s_prefix, &s_k);
    const uint64_t prefix = s_prefix;
    const int shift = 8 * (7 - pass);
    for (uint32_t i = blockIdx.x * 256u + threadIdx.x; i < n; i += gridDim.x * 256u) {
        const uint64_t k = select_key(J, i);
        if (pass == 0 || (k >> (shift + 8)) == prefix) atomicAdd(&h[(uint32_t)(k >> shift) & 255u], 1u);
    }
    __syncthreads();
    if (h[threadIdx.x]) atomicAdd(&a.hist[((size_t)j * 8 + pass) * 256 + threadIdx.x], h[threadIdx.x]);
}

__global__ __launch_bounds__(256) void k_orb_gather(OrbArgs a) {
    const int j = (int)blockIdx.y;
    const OrbJob &J = a.job[j];
    const uint32_t n = min(a.counts[j], J.cand);
    if (n <= J.nd) return;
    __shared__ uint64_t s_prefix;
    __shared__ uint32_t s_k;
    select_state(a, j, 8, &s_prefix, &s_k);
    const uint64_t cut = s_prefix; // exactly nd keys are <= cut
    for (uint32_t i = blockIdx.x * 256u + threadIdx.x; i < n; i += gridDim.x * 256u) {
        const uint64_t k = select_key(J, i);
        if (k <= cut) {
            const uint32_t slot = atomicAdd(&a.sel_n[j], 1u);
            if (slot < J.nd) a.sel[J.sel_off + slot] = k;
        }
    }
}

// ---- rank, border filter, orientation ----------------------------------------------------------------------------------
__global__ __launch_bounds__(64) void k_orb_orient(OrbArgs a) {
    const int j = (int)blockIdx.y;
    const OrbJob &J = a.job[j];
    const uint32_t n = min(a.counts[j], J.cand);
    const uint32_t m = min(n, J.nd);
    if (blockIdx.x * 64u >= m) return; // uniform
    __shared__ float w[PATCH * PATCH];
    for (int t = (int)threadIdx.x; t < PATCH * PATCH; t += 64) {
        if (a.weights) {
            w[t] = a.weights[t];
        } else { // orientation_weights (:340-357)
            const int dy = t / PATCH - HALF, dx = t % PATCH - HALF;
            const float dist_sq = (float)(dx * dx + dy * dy);
            w[t] = dist_sq <= 225.0f ? dev_expf(-dist_sq / 112.5f) : 0.0f;
        }
    }
    __syncthreads();
    const uint32_t i = blockIdx.x * 64u + threadIdx.x;
    if (i >= m) return;
    uint32_t idx = i, rank = i;
    if (n > J.nd) {
        const uint64_t *sel = a.sel + J.sel_off;
        const uint64_t mine = sel[i];
        rank = 0;
        for (uint32_t q = 0; q < m; ++q) rank += sel[q] < mine;
        idx = min((uint32_t)mine, n - 1); // the low word is a list index: always below n
    }
    const uint32_t p = J.pos[idx];
    const int x = (int)(p % (uint32_t)J.cols), y = (int)(p / (uint32_t)J.cols);
    const float xf = (float)x, yf = (float)y;
    zg_keypoint kp;
    kp.x = xf * J.scale;
    kp.y = yf * J.scale;
    kp.size = 7.0f * J.scale;
    kp.angle = 0.0f;
    kp.response = key_response(J.key[idx], a.harris);
    kp.octave = J.octave;
    kp.class_id = -1;
    if (xf < J.margin || xf >= (float)J.cols - J.margin || yf < J.margin || yf >= (float)J.rows - J.margin) {
        kp.octave = -1; // dropped (:201-205)
    } else {
        float m00 = 0.0f, m10 = 0.0f, m01 = 0.0f; // :359-395: raster order, one adder each; a zero weight adds nothing
        for (int v = 0; v < PATCH; ++v) {
            const int dy = v - HALF, py = y + dy;
            if (py < 0 || py >= J.rows) continue;
            const uint8_t *row = J.img + (size_t)py * J.stride;
            for (int u = 0; u < PATCH; ++u) {
                const int dx = u - HALF, px = x + dx;
                const float wt = w[v * PATCH + u];
                if (px < 0 || px >= J.cols || wt == 0.0f) continue;
                const float intensity = (float)row[px] * wt;
                m00 += intensity;
                m10 += intensity * (float)dx;
                m01 += intensity * (float)dy;
            }
        }
        if (!(m00 < 0.001f)) kp.angle = dev_atan2f(m01 / m00, m10 / m00) * 57.29577951308232f; // radiansToDegrees
    }
    a.tmp[J.sel_off + rank] = kp;
}

// ---- the levels' lists, one after the other ------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_orb_compact(OrbArgs a) {
    const int tid = (int)threadIdx.x;
    uint32_t base = 0;
    for (int j = 0; j < a.n; ++j) {
        const OrbJob &J = a.job[j];
        const uint32_t m = min(min(a.counts[j], J.cand), J.nd);
        for (uint32_t i0 = 0; i0 < m; i0 += 256) {
            const uint32_t i = i0 + (uint32_t)tid;
            zg_keypoint kp;
            kp.octave = -1;
            if (i < m) kp = a.tmp[J.sel_off + i];
            const bool keep = kp.octave >= 0;
            uint32_t total;
            const uint32_t before = block_exclusive_count(keep, &total);
            if (keep && base + before < a.capacity) a.out[base + before] = kp;
            base += total;
        }
    }
    if (tid == 0) *a.count = base;
}

// ---- descriptors -----------------------------------------------------------------------------------------------------
__device__ inline bool sample(const OrbPyramid &P, int level, float fy, float fx, int *value) { // atOrNull(@round(y), @round(x))
    const float r = roundf(fy), c = roundf(fx);
    if (!(r >= 0.0f && c >= 0.0f && r < (float)P.rows[level] && c < (float)P.cols[level])) return false;
    *value = P.img[level][(size_t)(int)r * P.stride[level] + (size_t)(int)c];
    return true;
}

__global__ __launch_bounds__(256) void k_orb_describe(OrbPyramid P, const zg_keypoint *kps, const uint32_t *count, uint32_t limit,
                                                      zg_binary_descriptor *out) {
    const uint32_t n = count ? min(*count, limit) : limit;
    const int lane = (int)threadIdx.x & 63;
    for (uint32_t i = blockIdx.x * 4u + (threadIdx.x >> 6); i < n; i += gridDim.x * 4u) { // uniform per wave
        const zg_keypoint kp = kps[i];
        const int level = min(max(0, kp.octave), P.n_levels - 1); // :228
        const float scale = P.scale[level];
        const float kx = kp.x / scale, ky = kp.y / scale;
        const float rad = kp.angle * 0.017453292519943295f; // degreesToRadians
        const float c = dev_cosf(rad), s = dev_sinf(rad);
        uint64_t word[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const int8_t *pr = ORB_PAIRS + 4 * (64 * k + lane);
            const float x1 = (float)pr[0], y1 = (float)pr[1], x2 = (float)pr[2], y2 = (float)pr[3];
            const float rx1 = c * x1 - s * y1, ry1 = s * x1 + c * y1;
            const float rx2 = c * x2 - s * y2, ry2 = s * x2 + c * y2;
            int p1 = 0, p2 = 0;
            const bool ok = sample(P, level, ky + ry1, kx + rx1, &p1) && sample(P, level, ky + ry2, kx + rx2, &p2);
            word[k] = __ballot(ok && p1 < p2);
        }
        if (lane < 32) {
            const uint64_t wd = lane < 8 ? word[0] : lane < 16 ? word[1] : lane < 24 ? word[2] : word[3];
            out[i].bits[lane] = (uint8_t)(wd >> (8 * (lane & 7)));
        }
    }
}

int check_params(const zg_orb_params *p) {
    ZG_REQUIRE(p != nullptr, ZG_ERR_INVALID_ARGUMENT, "orb: null params");
    ZG_REQUIRE(p->n_levels >= 1 && p->n_levels <= 255, ZG_ERR_INVALID_ARGUMENT, "orb: n_levels %u is not in 1 .. 255 (orb.zig:94)", p->n_levels);
    ZG_REQUIRE(p->scale_factor > 1.0f, ZG_ERR_INVALID_ARGUMENT, "orb: scale_factor %g must be above 1 (pyramid.zig:38)", (double)p->scale_factor);
    ZG_REQUIRE(p->edge_threshold <= 255, ZG_ERR_INVALID_ARGUMENT, "orb: edge_threshold %u does not fit the reference's u8 (orb.zig:97)", p->edge_threshold);
    ZG_REQUIRE(p->first_level <= 255, ZG_ERR_INVALID_ARGUMENT, "orb: first_level %u does not fit the reference's u8 (orb.zig:100)", p->first_level);
    ZG_REQUIRE(p->fast_threshold <= 255, ZG_ERR_INVALID_ARGUMENT, "orb: fast_threshold %u does not fit the reference's u8 (orb.zig:106)", p->fast_threshold);
    ZG_REQUIRE(p->wta_k == 2, ZG_ERR_INVALID_ARGUMENT, "orb: wta_k %u: the reference's descriptor compares pairs (wta_k = 2, orb.zig:103)", p->wta_k);
    ZG_REQUIRE(p->score_type == ZG_ORB_HARRIS_SCORE || p->score_type == ZG_ORB_FAST_SCORE, ZG_ERR_INVALID_ARGUMENT, "orb: score_type %d", p->score_type);
    return ZG_OK;
}

// computeFeaturesPerLevel (:279-334); scale_factor > 1 here, so the even split is the n_levels == 1 branch alone
void features_per_level(const zg_orb_params *p, uint32_t *out) {
    const uint32_t nl = p->n_levels, nf = p->n_features;
    if (nl == 1) {
        out[0] = nf;
        return;
    }
    const float factor = 1.0f / p->scale_factor;
    const float factor_to_n = hostmath::pow_f32(factor, (float)nl);
    uint32_t assigned = 0;
    const float nf_f = (float)nf;
    for (uint32_t level = 0; level < nl; ++level) {
        const uint32_t remaining = assigned < nf ? nf - assigned : 0;
        if (level == nl - 1 || remaining == 0) {
            out[level] = remaining;
            assigned += remaining;
            continue;
        }
        const float level_factor = hostmath::pow_f32(factor, (float)level);
        const float desired = nf_f * (1.0f - factor) / (1.0f - factor_to_n) * level_factor;
        const double rounded = std::round((double)desired); // @round: halves away from zero
        const uint32_t clamped = rounded >= (double)remaining ? remaining : (uint32_t)rounded;
        const uint32_t base_min = std::max<uint32_t>(10u, nf / (nl * 3u));
        const uint32_t min_features = std::min(remaining, base_min);
        out[level] = clamped < min_features ? min_features : clamped;
        assigned += out[level];
    }
}

uint32_t adaptive_threshold(const zg_orb_params *p, uint32_t level) { // :511-517
    const float level_scale = hostmath::pow_f32(p->scale_factor, (float)level);
    const float attenuation = 1.0f / level_scale;
    float v = (float)p->fast_threshold * attenuation;
    v = v < 5.0f ? 5.0f : (v > 255.0f ? 255.0f : v);
    return (uint32_t)std::round(v);
}

// What a call works on: the pyramid's shapes, every level's share and threshold.
struct Plan {
    uint32_t n_levels = 0;
    uint32_t rows[ORB_MAX_LEVELS], cols[ORB_MAX_LEVELS];
    float scale[ORB_MAX_LEVELS], sigma[ORB_MAX_LEVELS];
    uint32_t nd[ORB_MAX_LEVELS], threshold[ORB_MAX_LEVELS];
};
int make_plan(const zg_image *src, const zg_orb_params *p, bool device_pointer, Plan *plan) {
    int rc;
    if ((rc = check_params(p)) || (rc = check_image(src, "src", device_pointer))) return rc;
    ZG_REQUIRE(src->pixel == ZG_PIXEL_U8, ZG_ERR_UNSUPPORTED, "orb: src is not Image(u8) (Orb takes Image(u8) only)");
    ZG_REQUIRE(src->rows > 7 && src->cols > 7, ZG_ERR_INVALID_ARGUMENT, "orb: src is %ux%u; Fast.detect needs rows > 7 and cols > 7 (Fast.zig:39)",
               src->rows, src->cols);
    ZG_REQUIRE((uint64_t)src->rows * src->cols < (1ull << 32), ZG_ERR_UNSUPPORTED, "orb: %ux%u has 2^32 pixels or more", src->rows, src->cols);
    plan->n_levels = p->n_levels;
    for (uint32_t l = 0; l < p->n_levels; ++l) {
        const float scale = hostmath::pow_f32(p->scale_factor, (float)l);
        uint32_t r = src->rows, c = src->cols;
        float sigma = 0.0f;
        if (l > 0) {
            if ((rc = zg_pyramid_level(src->rows, src->cols, scale, PYRAMID_SIGMA, &r, &c, &sigma))) return rc;
            ZG_REQUIRE(r >= 8 && c >= 8, ZG_ERR_INVALID_ARGUMENT,
                       "orb: level %u of a %ux%u image is %ux%u, below 8 x 8: the pyramid stops before n_levels = %u (pyramid.zig:64-66, orb.zig:159)", l,
                       src->rows, src->cols, r, c, p->n_levels);
        }
        ZG_REQUIRE(l < (uint32_t)ORB_MAX_LEVELS, ZG_ERR_UNSUPPORTED, "orb: more than %d pyramid levels", ORB_MAX_LEVELS);
        plan->rows[l] = r;
        plan->cols[l] = c;
        plan->scale[l] = scale;
        plan->sigma[l] = sigma;
        plan->threshold[l] = adaptive_threshold(p, l);
    }
    features_per_level(p, plan->nd);
    return ZG_OK;
}

// The pyramid's levels first .. n_levels - 1 (level 0 is the source) at base, packed; fills P and builds them on s.
size_t pyramid_bytes(const Plan &plan, uint32_t first) {
    size_t b = 0;
    for (uint32_t l = std::max(first, 1u); l < plan.n_levels; ++l) b += align256((size_t)plan.rows[l] * plan.cols[l]);
    return b;
}
int build_pyramid(const zg_image *src, const Plan &plan, uint32_t first, char *base, OrbPyramid *P, hipStream_t s) {
    std::vector<zg_image> levels;
    std::vector<float> sigmas;
    P->n_levels = (int32_t)plan.n_levels;
    for (uint32_t l = 0; l < plan.n_levels; ++l) {
        P->rows[l] = (int32_t)plan.rows[l];
        P->cols[l] = (int32_t)plan.cols[l];
        P->scale[l] = plan.scale[l];
        if (l == 0) {
            P->img[0] = (const uint8_t *)src->data;
            P->stride[0] = src->stride;
        } else if (l < first) { // never read: no keypoint of this call lies on it
            P->img[l] = nullptr;
            P->stride[l] = 0;
        } else {
            P->img[l] = (const uint8_t *)base;
            P->stride[l] = plan.cols[l];
            levels.push_back(zg_image{base, plan.cols[l], plan.rows[l], plan.cols[l], ZG_PIXEL_U8});
            sigmas.push_back(plan.sigma[l]);
            base += align256((size_t)plan.rows[l] * plan.cols[l]);
        }
    }
    if (levels.empty()) return ZG_OK;
    return zg_pyramid_build(src, levels.data(), sigmas.data(), (uint32_t)levels.size(), (zg_stream)s);
}

int describe(const OrbPyramid &P, const zg_keypoint *kps, const uint32_t *count, uint32_t limit, zg_binary_descriptor *out, hipStream_t s) {
    if (limit == 0) return ZG_OK;
    const uint32_t blocks = std::min<uint32_t>(ceil_div(limit, 4), 4096);
    hipLaunchKernelGGL(k_orb_describe, dim3(blocks), dim3(256), 0, s, P, kps, count, limit, out);
    return launch_ok("k_orb_describe");
}

int detect_and_compute(const zg_image *src, const zg_orb_params *p, const Plan &plan, zg_keypoint *keypoints, zg_binary_descriptor *descriptors,
                       uint32_t capacity, uint32_t *count, hipStream_t s) {
    int rc;
    if (p->orientation_weights && (rc = refuse_under_capture(s, "zg_orb_detect_and_compute with a caller's orientation_weights (a synchronous upload)")))
        return rc;
    OrbArgs a{};
    a.harris = p->score_type == ZG_ORB_HARRIS_SCORE;
    uint32_t sel_total = 0, max_cand = 0, max_sel = 0;
    for (uint32_t l = p->first_level; l < plan.n_levels; ++l) {
        if (plan.nd[l] == 0) continue; // :162
        OrbJob &J = a.job[a.n++];
        J.rows = (int32_t)plan.rows[l];
        J.cols = (int32_t)plan.cols[l];
        J.scale = plan.scale[l];
        J.margin = std::max(3.0f, (float)p->edge_threshold / plan.scale[l]); // :194-197
        J.nd = plan.nd[l];
        J.cand = (plan.rows[l] - 6) * (plan.cols[l] - 6);
        J.octave = (int32_t)l;
        J.sel_off = sel_total;
        const uint32_t cap = std::min(J.nd, J.cand);
        sel_total += cap;
        max_sel = std::max(max_sel, cap);
        max_cand = std::max(max_cand, J.cand);
    }
    if (a.n == 0) { // no level detects: an empty list
        return fill_async(count, 0, sizeof(uint32_t), s);
    }
    const uint32_t first = (uint32_t)a.job[0].octave;
    // scratch: [pyramid levels][per job: pos, key][counts][hist, sel_n (zeroed)][sel][tmp][weights]
    const size_t zero_words = (size_t)a.n * 8 * 256 + a.n;
    ScratchBlock sc(s);
    char *pyramid;
    float *weights;
    sc.take(pyramid, pyramid_bytes(plan, first));
    for (int j = 0; j < a.n; ++j) {
        sc.take(a.job[j].pos, a.job[j].cand);
        sc.take(a.job[j].key, a.job[j].cand);
    }
    sc.take(a.counts, a.n);
    sc.take(a.hist, zero_words);
    sc.take(a.sel, sel_total);
    sc.take(a.tmp, sel_total);
    sc.take(weights, PATCH * PATCH);
    if ((rc = sc.alloc())) return rc;
    if (p->orientation_weights) {
        if ((rc = upload_pageable(weights, p->orientation_weights, PATCH * PATCH * sizeof(float), s))) return rc;
        a.weights = weights;
    }
    OrbPyramid P{};
    if ((rc = build_pyramid(src, plan, first, pyramid, &P, s))) return rc;
    a.sel_n = a.hist + (size_t)a.n * 8 * 256;
    a.out = keypoints;
    a.capacity = capacity;
    a.count = count;
    std::vector<zg_image> images(a.n);
    std::vector<uint32_t> thresholds(a.n), caps(a.n);
    std::vector<uint32_t *> pos(a.n), key(a.n), cnt(a.n);
    for (int j = 0; j < a.n; ++j) {
        OrbJob &J = a.job[j];
        J.img = P.img[J.octave];
        J.stride = P.stride[J.octave];
        images[j] = zg_image{(void *)J.img, (size_t)J.stride, (uint32_t)J.rows, (uint32_t)J.cols, ZG_PIXEL_U8};
        thresholds[j] = plan.threshold[J.octave];
        caps[j] = J.cand;
        pos[j] = J.pos;
        key[j] = J.key;
        cnt[j] = a.counts + j;
    }
    if ((rc = fill_async(a.hist, 0, align256(zero_words * sizeof(uint32_t)), s))) return rc;
    if ((rc = fast_detect_compact(images.data(), (uint32_t)a.n, thresholds.data(), pos.data(), key.data(), caps.data(), cnt.data(), s))) return rc;
    const dim3 sweep(std::max(1u, std::min(ceil_div(max_cand, 256 * 8), 256u)), (unsigned)a.n);
    if (a.harris) {
        hipLaunchKernelGGL(k_orb_harris, sweep, dim3(256), 0, s, a);
        if ((rc = launch_ok("k_orb_harris"))) return rc;
    }
    for (int pass = 0; pass < 8; ++pass) {
        bool counted = false;
        for (int j = 0; j < a.n; ++j) counted = counted || fixed_digit(a.harris, a.job[j].cand, pass) < 0;
        if (!counted) continue;
        hipLaunchKernelGGL(k_orb_hist, sweep, dim3(256), 0, s, a, pass);
        if ((rc = launch_ok("k_orb_hist"))) return rc;
    }
    hipLaunchKernelGGL(k_orb_gather, sweep, dim3(256), 0, s, a);
    if ((rc = launch_ok("k_orb_gather"))) return rc;
    hipLaunchKernelGGL(k_orb_orient, dim3(ceil_div(max_sel, 64), (unsigned)a.n), dim3(64), 0, s, a);
    if ((rc = launch_ok("k_orb_orient"))) return rc;
    hipLaunchKernelGGL(k_orb_compact, dim3(1), dim3(256), 0, s, a);
    if ((rc = launch_ok("k_orb_compact"))) return rc;
    if (descriptors) rc = describe(P, keypoints, count, capacity, descriptors, s);
    return rc;
}

int compute(const zg_image *src, const Plan &plan, const zg_keypoint *keypoints, uint32_t n, zg_binary_descriptor *descriptors, hipStream_t s) {
    if (n == 0) return ZG_OK;
    ScratchBlock sc(s);
    int rc;
    const size_t bytes = pyramid_bytes(plan, 1);
    if (bytes && (rc = sc.alloc(bytes))) return rc;
    OrbPyramid P{};
    if ((rc = build_pyramid(src, plan, 1, sc.p, &P, s))) return rc;
    return describe(P, keypoints, nullptr, n, descriptors, s);
}

} // namespace
} // namespace zg

using namespace zg;

extern "C" {

void zg_orb_default_params(zg_orb_params *p) {
    if (!p) return;
    *p = zg_orb_params{500, 1.2f, 8, 15, 0, 2, 20, ZG_ORB_FAST_SCORE, nullptr};
}

int zg_orb_features_per_level(const zg_orb_params *params, uint32_t *out) {
    int rc;
    if ((rc = check_params(params))) return rc;
    ZG_REQUIRE(out != nullptr, ZG_ERR_INVALID_ARGUMENT, "orb: null out");
    ZG_REQUIRE(params->n_levels <= 85, ZG_ERR_INVALID_ARGUMENT, "orb: n_levels %u: n_levels * 3 overflows the reference's u8 (orb.zig:325)", params->n_levels);
    features_per_level(params, out);
    return ZG_OK;
}

int zg_orb_adaptive_threshold(const zg_orb_params *params, uint32_t level) {
    int rc;
    if ((rc = check_params(params))) return -rc;
    return (int)adaptive_threshold(params, level);
}

int zg_orb_detect_and_compute(const zg_image *src, const zg_orb_params *params, zg_keypoint *keypoints, zg_binary_descriptor *descriptors, uint32_t capacity,
                              uint32_t *count, zg_stream stream) {
    Plan plan;
    int rc;
    if ((rc = make_plan(src, params, true, &plan))) return rc;
    ZG_REQUIRE(count != nullptr, ZG_ERR_INVALID_ARGUMENT, "orb: null count");
    ZG_REQUIRE(keypoints != nullptr || capacity == 0, ZG_ERR_INVALID_ARGUMENT, "orb: null keypoints with capacity %u", capacity);
    return detect_and_compute(src, params, plan, keypoints, descriptors, capacity, count, as_stream(stream));
}

int zg_orb_compute(const zg_image *src, const zg_orb_params *params, const zg_keypoint *keypoints, uint32_t n, zg_binary_descriptor *descriptors,
                   zg_stream stream) {
    Plan plan;
    int rc;
    if ((rc = make_plan(src, params, true, &plan))) return rc;
    ZG_REQUIRE(n == 0 || (keypoints && descriptors), ZG_ERR_INVALID_ARGUMENT, "orb compute: null keypoints or descriptors with n = %u", n);
    return compute(src, plan, keypoints, n, descriptors, as_stream(stream));
}

int zg_orb_detect_and_compute_host(const zg_image *src, const zg_orb_params *params, zg_keypoint *keypoints, zg_binary_descriptor *descriptors,
                                   uint32_t capacity, uint32_t *count) {
    Plan plan;
    int rc;
    if ((rc = make_plan(src, params, false, &plan))) return rc;
    ZG_REQUIRE(count != nullptr, ZG_ERR_INVALID_ARGUMENT, "orb: null count");
    ZG_REQUIRE(keypoints != nullptr || capacity == 0, ZG_ERR_INVALID_ARGUMENT, "orb: null keypoints with capacity %u", capacity);
    HostStage in;
    if ((rc = in.upload(src, true, false))) return rc;
    // scratch: [keypoints][descriptors][count]
    ScratchBlock sc;
    zg_keypoint *dkp;
    zg_binary_descriptor *dde;
    uint32_t *dcount;
    sc.take(dkp, capacity);
    sc.take(dde, capacity);
    sc.take(dcount, 1);
    if ((rc = sc.alloc())) return rc;
    if (!capacity) dkp = nullptr;
    if (!capacity || !descriptors) dde = nullptr;
    if ((rc = detect_and_compute(&in.dev, params, plan, dkp, dde, capacity, dcount, nullptr))) return rc;
    if ((rc = download_counted(count, dcount, 1, keypoints, dkp, capacity)) || !dde) return rc;
    return download_pageable(descriptors, dde, (size_t)std::min(*count, capacity) * sizeof(zg_binary_descriptor), nullptr);
}

int zg_orb_compute_host(const zg_image *src, const zg_orb_params *params, const zg_keypoint *keypoints, uint32_t n, zg_binary_descriptor *descriptors) {
    Plan plan;
    int rc;
    if ((rc = make_plan(src, params, false, &plan))) return rc;
    ZG_REQUIRE(n == 0 || (keypoints && descriptors), ZG_ERR_INVALID_ARGUMENT, "orb compute: null keypoints or descriptors with n = %u", n);
    if (n == 0) return ZG_OK;
    HostStage in;
    if ((rc = in.upload(src, true, false))) return rc;
    // scratch: [keypoints][descriptors]
    ScratchBlock sc;
    zg_keypoint *dkp;
    zg_binary_descriptor *dde;
    sc.take(dkp, n);
    sc.take(dde, n);
    if ((rc = sc.alloc())) return rc;
    if ((rc = upload_pageable(dkp, keypoints, (size_t)n * sizeof(zg_keypoint), nullptr))) return rc;
    if ((rc = compute(&in.dev, plan, dkp, n, dde, nullptr))) return rc;
    return download_pageable(descriptors, dde, (size_t)n * sizeof(zg_binary_descriptor), nullptr);
}

} // extern "C"
