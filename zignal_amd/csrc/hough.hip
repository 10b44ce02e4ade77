// hough.hip — HoughTransform.compute / findLines (reference src/image/hough.zig:75-257) on the device, bit for bit.
//
// compute is i32 arithmetic on the two fixed-point tables and integer adds, which commute: the accumulator equals the reference's
// whatever the order of execution.
//   k_edge_list      the non-zero bytes of box ∩ image as (x_val, y_val) pairs, a workgroup appending its 4096 pixels' share with one
//                    atomic (order is free)
//   k_vote_lds       grid = theta strips x parts of the edge list. A workgroup owns `strip` theta columns whose strip x size counters fit in
//                    64 KiB of LDS, a lane per edge pixel votes with LDS integer atomics (the strip's cos / sin arrive by uniform
//                    loads), then every non-zero counter is one global integer atomic, a row segment of the strip per wave step
//   k_vote_direct    sizes above LDS_MAX_SIZE, or any size with ZIGNAL_HIP_HOUGH_DIRECT=1: every vote a global atomic
// findLines:
//   k_peak_rows      a workgroup per interior row: the row's number of candidates (votes >= threshold, no 8-neighbour strictly greater)
//   k_row_offsets    one workgroup: the exclusive sums of the row counts and counts[0], their total
//   k_peak_rows<emit> a workgroup per row again: candidates in column order at the row's offset — row-major order, no atomic decides
//                    a position. A candidate is the 64-bit key (~score << 32 | row * size + col): ascending keys are the stable sort's order
//   k_rank_sort      a lane per candidate counts the keys below its own (they arrive by uniform loads): the key is unique, so
//                    that count is its exact place
//   k_greedy         one workgroup walks the sorted list; each candidate is tested against the kept list 256 entries a step
//   k_lines          getLineProperties, createLine and clipLine in f32 for the kept candidates that fit the caller's capacity
// When counts[0] > max_candidates the later kernels see it and write counts[1] = 0 alone.
#include "zg_common.h"
#include "zg_devmath.h"
#include "zg_hostmath.h"
#include "zg_scan.h"

#include <algorithm>
#include <cstdlib>
#include <memory>
#include <vector>

struct zg_hough {
    uint32_t size, even_size;
    int32_t *tables; // device: cos[size], sin[size]
};

namespace zg {
namespace {

constexpr uint32_t LDS_COUNTERS = 16384; // 64 KiB of u32 counters a workgroup
constexpr uint32_t MIN_STRIP = 8;        // fewer theta columns a workgroup and the flush outweighs the votes
constexpr uint32_t LDS_MAX_SIZE = LDS_COUNTERS / MIN_STRIP - 1; // a column of the strip is size | 1 counters long
__host__ __device__ inline uint32_t lds_pitch(uint32_t size) { return size | 1u; } // odd: a row's strip entries lie in different banks
constexpr uint32_t PIXEL_CHUNK = 256;    // the edge list is shared out in multiples of it: a pixel a lane
constexpr uint32_t DIRECT_THETAS = 64;   // theta columns a thread of the direct form walks
constexpr uint32_t LDS_VOTE_GROUPS = 512;   // workgroups of k_vote_lds to aim for: two a CU, each pays for clearing and adding its strip once
constexpr uint32_t MAX_VOTE_GROUPS = 4096;

struct VoteArgs {
    const int32_t *cos_t, *sin_t;
    const uint32_t *list;  // [n] x_val | y_val << 16 (two i16)
    const uint32_t *n;
    uint32_t *acc;
    size_t acc_stride;
    uint32_t size, strip;
    int32_t offset2;       // offset << 1
};

struct ListArgs {
    const uint8_t *edges;
    size_t stride;
    uint32_t l, t, w, h;   // area = box ∩ image: first column and row, width, height
    int32_t x0, y0;        // x_val = 2 * col + x0, y_val = 2 * row + y0 (col, row relative to the area)
    uint32_t *list, *n;
};

constexpr uint32_t LIST_PER_THREAD = 16; // pixels a thread of k_edge_list looks at: a workgroup appends once for 4096 of them

// One returning atomic on the list's length word a workgroup: a wave-level append of 64 pixels spent three quarters of compute's time at
// size 1024 waiting for that one word (75 of 120 us).
__global__ __launch_bounds__(256) void k_edge_list(ListArgs a) {
    __shared__ uint32_t first_s;
    const uint32_t total = a.w * a.h, base = blockIdx.x * (256u * LIST_PER_THREAD); // the area has at most 2^30 pixels
    uint32_t on = 0; // bit k: pixel base + k * 256 + threadIdx.x is an edge
#pragma unroll 4
    for (uint32_t k = 0; k < LIST_PER_THREAD; ++k) {
        const uint32_t i = base + k * 256u + threadIdx.x;
        if (i < total) {
            const uint32_t r = i / a.w, c = i - r * a.w;
            on |= (a.edges[(size_t)(a.t + r) * a.stride + a.l + c] != 0 ? 1u : 0u) << k; // :103
        }
    }
    uint32_t sum;
    const uint32_t before = block_exclusive_sum((uint32_t)__popc(on), &sum);
    if (sum == 0) return; // uniform
    if (threadIdx.x == 0) first_s = atomicAdd(a.n, sum);
    __syncthreads();
    uint32_t at = first_s + before;
    for (uint32_t k = 0; k < LIST_PER_THREAD; ++k) {
        if (!(on >> k & 1u)) continue;
        const uint32_t i = base + k * 256u + threadIdx.x;
        const uint32_t r = i / a.w, c = i - r * a.w;
        const int32_t x = 2 * (int32_t)c + a.x0, y = 2 * (int32_t)r + a.y0; // :93, :105
        a.list[at++] = ((uint32_t)x & 0xFFFFu) | ((uint32_t)y << 16);
    }
}

// :110-112 / :131-133. No i32 expression here can overflow for size <= ZG_HOUGH_MAX_SIZE (the bound's derivation is in the header).
__device__ inline int32_t vote_row(int32_t x, int32_t y, int32_t c, int32_t s, int32_t offset2) {
    const int32_t rho = x * c + y * s;
    return ((rho >> 1) + offset2) >> 16;
}

__global__ __launch_bounds__(256) void k_vote_lds(VoteArgs a) {
    __shared__ uint32_t cnt[LDS_COUNTERS]; // [theta in the strip][row], lds_pitch apart: lanes are pixels, whose rows differ
    const uint32_t n = *a.n;
    // the list is known only here: gridDim.y workgroups share it in equal parts of whole chunks, and those left without a part return
    const uint32_t per = ((n + gridDim.y - 1) / gridDim.y + PIXEL_CHUNK - 1) / PIXEL_CHUNK * PIXEL_CHUNK, first = blockIdx.y * per;
    if (first >= n) return; // uniform
    const uint32_t t0 = blockIdx.x * a.strip, nt = min(a.strip, a.size - t0), pitch = lds_pitch(a.size), cells = a.size * a.strip;
    const uint32_t used = pitch * a.strip, end = min(n, first + per);
    for (uint32_t i = threadIdx.x; i < used; i += 256u) cnt[i] = 0;
    __syncthreads();
    for (uint32_t p = first + threadIdx.x; p < end; p += 256u) {
        const uint32_t xy = a.list[p];
        const int32_t x = (int16_t)(xy & 0xFFFFu), y = (int16_t)(xy >> 16);
        for (uint32_t tt = 0; tt < nt; ++tt) { // cos / sin of a step are the same for every lane: uniform loads
            const int32_t rr = vote_row(x, y, a.cos_t[t0 + tt], a.sin_t[t0 + tt], a.offset2);
            if (rr >= 0 && rr < (int32_t)a.size) atomicAdd(&cnt[tt * pitch + (uint32_t)rr], 1u);
        }
    }
    __syncthreads();
    for (uint32_t i = threadIdx.x; i < cells; i += 256u) { // theta fastest: a wave step adds to row segments of the strip
        const uint32_t rr = i / a.strip, tt = i - rr * a.strip;
        const uint32_t v = cnt[tt * pitch + rr];
        if (v != 0 && tt < nt) atomicAdd(a.acc + (size_t)rr * a.acc_stride + t0 + tt, v);
    }
}

__global__ __launch_bounds__(256) void k_vote_direct(VoteArgs a) {
    const uint32_t n = *a.n;
    const uint32_t t0 = blockIdx.y * DIRECT_THETAS, t1 = min(a.size, t0 + DIRECT_THETAS);
    for (uint32_t base = blockIdx.x * 256u; base < n; base += gridDim.x * 256u) {
        const uint32_t p = base + threadIdx.x;
        if (p >= n) continue;
        const uint32_t xy = a.list[p];
        const int32_t x = (int16_t)(xy & 0xFFFFu), y = (int16_t)(xy >> 16);
        for (uint32_t t = t0; t < t1; ++t) {
            const int32_t rr = vote_row(x, y, a.cos_t[t], a.sin_t[t], a.offset2);
            if (rr >= 0 && rr < (int32_t)a.size) atomicAdd(a.acc + (size_t)rr * a.acc_stride + t, 1u);
        }
    }
}

// ---- findLines ------------------------------------------------------------------------------------------------------------
struct PeakArgs {
    const uint32_t *acc;
    size_t acc_stride;
    uint32_t size;
    uint32_t threshold;
    const uint32_t *threshold_device;
    uint32_t max_candidates;
    uint32_t *row_counts;  // [size - 2]
    uint32_t *row_offsets; // [size - 2]
    uint64_t *cand;        // [max_candidates] keys in row-major order
    uint64_t *sorted;      // [max_candidates]
    uint32_t *counts;
};

// :158-170 for the interior cell (r, c)
__device__ inline bool is_candidate(const PeakArgs &a, uint32_t thr, uint32_t r, uint32_t c, uint32_t *votes) {
    const uint32_t *p = a.acc + (size_t)r * a.acc_stride + c;
    const uint32_t v = *p;
    *votes = v;
    if (v < thr) return false;
    const uint32_t *up = p - a.acc_stride, *dn = p + a.acc_stride;
    const uint32_t m = max(max(max(up[-1], up[0]), max(up[1], p[-1])), max(max(p[1], dn[-1]), max(dn[0], dn[1])));
    return !(m > v);
}

template <bool EMIT> __global__ __launch_bounds__(256) void k_peak_rows(PeakArgs a) {
    const uint32_t thr = a.threshold_device ? *a.threshold_device : a.threshold;
    const uint32_t r = blockIdx.x + 1u, inner = a.size - 2u;
    uint32_t before = EMIT ? a.row_offsets[blockIdx.x] : 0u;
    if (EMIT && (a.row_counts[blockIdx.x] == 0 || before >= a.max_candidates)) return;
    for (uint32_t c0 = 0; c0 < inner; c0 += 256u) { // uniform trip count: the sums below are workgroup-wide
        const uint32_t c = c0 + threadIdx.x + 1u;
        uint32_t votes = 0;
        const bool cand = c <= inner && is_candidate(a, thr, r, c, &votes);
        uint32_t total;
        const uint32_t pos = before + block_exclusive_sum(cand ? 1u : 0u, &total);
        if (EMIT && cand && pos < a.max_candidates) a.cand[pos] = ((uint64_t)(~votes) << 32) | (uint64_t)(r * a.size + c);
        before += total;
    }
    if (!EMIT && threadIdx.x == 0) a.row_counts[blockIdx.x] = before;
}

__global__ __launch_bounds__(256) void k_row_offsets(PeakArgs a) {
    const uint32_t inner = a.size - 2u;
    uint32_t before = 0;
    for (uint32_t i0 = 0; i0 < inner; i0 += 256u) {
        const uint32_t i = i0 + threadIdx.x;
        const uint32_t v = i < inner ? a.row_counts[i] : 0u;
        uint32_t total;
        const uint32_t off = before + block_exclusive_sum(v, &total);
        if (i < inner) a.row_offsets[i] = off;
        before += total; // at most (size - 2)^2 < 2^32
    }
    if (threadIdx.x == 0) a.counts[0] = before;
}

__global__ __launch_bounds__(256) void k_rank_sort(PeakArgs a) {
    const uint32_t n = a.counts[0];
    if (n > a.max_candidates || blockIdx.x * 256u >= n) return;
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    const uint64_t mine = a.cand[min(i, n - 1u)];
    uint32_t rank = 0;
#pragma unroll 8
    for (uint32_t j = 0; j < n; ++j) rank += a.cand[j] < mine ? 1u : 0u; // j is uniform: the key arrives through the scalar cache
    if (i < n) a.sorted[rank] = mine;
}

struct GreedyArgs {
    const uint64_t *sorted;
    uint32_t size, even_size;
    uint32_t max_candidates;
    float angle_thresh, radius_thresh;
    float *kept_angle, *kept_radius; // [max_candidates]
    uint32_t *kept;                  // [max_candidates] place in `sorted`
    zg_hough_line *lines;
    uint32_t capacity;
    uint32_t *counts;
};

// getLineProperties (:207-212)
__device__ inline void line_properties(uint32_t size, uint32_t even_size, uint32_t col, uint32_t row, float *angle, float *radius) {
    const float center_val = (float)(size - 1u) / 2.0f;
    *angle = 180.0f * ((float)col - center_val) / (float)even_size;
    *radius = ((float)row - center_val) * 1.41421356237309504880f;
}

__global__ __launch_bounds__(256) void k_greedy(GreedyArgs a) {
    const uint32_t n = a.counts[0];
    if (n > a.max_candidates) { // a greedy pass over a truncated set would not be the reference's: nothing is given
        if (threadIdx.x == 0) a.counts[1] = 0;
        return;
    }
    uint32_t nk = 0;
    for (uint32_t i = 0; i < n; ++i) { // :188-201
        const uint32_t idx = (uint32_t)a.sorted[i];
        float angle, radius;
        line_properties(a.size, a.even_size, idx % a.size, idx / a.size, &angle, &radius);
        int close = 0;
        for (uint32_t j = threadIdx.x; j < nk; j += 256u) {
            const float ea = a.kept_angle[j], er = a.kept_radius[j];
            const float da = fabsf(ea - angle), dr = fabsf(er - radius);
            if ((da < a.angle_thresh && dr < a.radius_thresh) || ((180.0f - da) < a.angle_thresh && fabsf(er + radius) < a.radius_thresh)) close = 1;
        }
        if (!__syncthreads_or(close)) {
            if (threadIdx.x == 0) {
                a.kept_angle[nk] = angle;
                a.kept_radius[nk] = radius;
                a.kept[nk] = i;
            }
            ++nk;
            __syncthreads(); // the new entry is read by the whole workgroup from the next candidate on
        }
    }
    if (threadIdx.x == 0) a.counts[1] = nk;
}

// clipLine (:232-257)
__device__ inline void clip_line(float rl, float rt, float rr, float rb, float *p1, float *p2) {
    float t0 = 0.0f, t1 = 1.0f;
    const float dx = p2[0] - p1[0], dy = p2[1] - p1[1];
    const float p[4] = {-dx, dx, -dy, dy};
    const float q[4] = {p1[0] - rl, rr - p1[0], p1[1] - rt, rb - p1[1]};
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        if (p[i] == 0.0f) {
            if (q[i] < 0.0f) return;
        } else {
            const float r = q[i] / p[i];
            if (p[i] < 0.0f) {
                if (r > t1) return;
                if (r > t0) t0 = r;
            } else {
                if (r < t0) return;
                if (r < t1) t1 = r;
            }
        }
    }
    if (t0 > t1) return;
    const float ox = p1[0], oy = p1[1];
    p1[0] = ox + t0 * dx;
    p1[1] = oy + t0 * dy;
    p2[0] = ox + t1 * dx;
    p2[1] = oy + t1 * dy;
}

__global__ __launch_bounds__(256) void k_lines(GreedyArgs a) {
    if (a.counts[0] > a.max_candidates) return;
    const uint32_t n = min(a.counts[1], a.capacity), i = blockIdx.x * 256u + threadIdx.x;
    if (i >= n) return;
    const uint64_t key = a.sorted[a.kept[i]];
    const uint32_t idx = (uint32_t)key, score = ~(uint32_t)(key >> 32);
    float angle, radius;
    line_properties(a.size, a.even_size, idx % a.size, idx / a.size, &angle, &radius);
    // createLine (:214-229)
    const float center = (float)(a.size - 1u) / 2.0f;
    const float theta_rad = (angle + 90.0f) * 3.14159265358979323846f / 180.0f;
    const float cos_t = dev_cosf(theta_rad), sin_t = dev_sinf(theta_rad);
    const float pcx = radius * cos_t, pcy = radius * sin_t;
    const float dir_x = -sin_t, dir_y = cos_t;
    const float huge = (float)a.size * 2.0f;
    zg_hough_line out;
    out.angle = angle;
    out.radius = radius;
    out.score = score;
    out.p1[0] = center + pcx + dir_x * huge;
    out.p1[1] = center + pcy + dir_y * huge;
    out.p2[0] = center + pcx - dir_x * huge;
    out.p2[1] = center + pcy - dir_y * huge;
    clip_line(0.0f, 0.0f, (float)a.size, (float)a.size, out.p1, out.p2);
    a.lines[i] = out;
}

// ---- host side -------------------------------------------------------------------------------------------------------------
bool direct_forced() { // the replaced form stays reachable: read once per process
    static const bool forced = [] {
        const char *e = std::getenv("ZIGNAL_HIP_HOUGH_DIRECT");
        return e && *e && *e != '0';
    }();
    return forced;
}

int check_size(uint32_t size) {
    ZG_REQUIRE(size > 1, ZG_ERR_INVALID_ARGUMENT, "hough: size %u (error.InvalidArgument: size <= 1)", size); // :39
    ZG_REQUIRE(size <= ZG_HOUGH_MAX_SIZE, ZG_ERR_UNSUPPORTED, "hough: size %u is above %u, where the reference's i32 arithmetic overflows", size,
               ZG_HOUGH_MAX_SIZE);
    return ZG_OK;
}

void tables(uint32_t size, int32_t *cos_table, int32_t *sin_table) { // :49-56
    const uint32_t even_size = size % 2 == 0 ? size : size - 1;
    const double scale = 65536.0, sqrt_2 = 1.4142135623730951, pi = 3.141592653589793;
    for (uint32_t t = 0; t < size; ++t) {
        const double theta = (double)t * pi / (double)even_size;
        cos_table[t] = (int32_t)(scale * hostmath::cos_f64(theta) / sqrt_2); // @trunc, then the cast: a C conversion truncates
        sin_table[t] = (int32_t)(scale * hostmath::sin_f64(theta) / sqrt_2);
    }
}

int create(uint32_t size, const int32_t *cos_table, const int32_t *sin_table, zg_hough_t *out) {
    std::unique_ptr<zg_hough> h(new zg_hough{size, size % 2 == 0 ? size : size - 1, nullptr});
    const size_t bytes = (size_t)size * sizeof(int32_t);
    int devices = 0;
    if (hipGetDeviceCount(&devices) != hipSuccess || devices == 0) { // a transform without a device still answers argument errors
        (void)hipGetLastError();
        *out = h.release();
        return ZG_OK;
    }
    ZG_HIP(hipMalloc((void **)&h->tables, 2 * bytes));
    int rc;
    if ((rc = upload_pageable(h->tables, cos_table, bytes, nullptr)) || (rc = upload_pageable(h->tables + size, sin_table, bytes, nullptr))) {
        (void)hipFree(h->tables);
        return rc;
    }
    *out = h.release();
    return ZG_OK;
}

int check_compute(zg_hough_t h, const zg_image *edges, uint32_t l, uint32_t t, uint32_t r, uint32_t b, const uint32_t *accumulator, size_t acc_stride,
                  bool device) {
    ZG_REQUIRE(h != nullptr, ZG_ERR_INVALID_ARGUMENT, "hough compute: null transform");
    int rc;
    if ((rc = check_image(edges, "edges", device))) return rc;
    ZG_REQUIRE(edges->pixel == ZG_PIXEL_U8, ZG_ERR_UNSUPPORTED, "hough compute: edges must be Image(u8), got pixel type %d", edges->pixel);
    ZG_REQUIRE(r >= l && b >= t && r - l == h->size && b - t == h->size, ZG_ERR_DIMENSION_MISMATCH,
               "hough compute: the box (%u, %u, %u, %u) is not %u x %u", l, t, r, b, h->size, h->size); // :76
    ZG_REQUIRE(accumulator != nullptr, ZG_ERR_INVALID_ARGUMENT, "hough compute: null accumulator");
    ZG_REQUIRE(acc_stride >= h->size, ZG_ERR_INVALID_ARGUMENT, "hough compute: accumulator stride %zu is below size %u", acc_stride, h->size);
    ZG_REQUIRE(h->tables != nullptr, ZG_ERR_HIP, "hough compute: the transform was created without a device");
    return ZG_OK;
}

int compute(zg_hough_t h, const zg_image *edges, uint32_t l, uint32_t t, uint32_t r, uint32_t b, uint32_t *accumulator, size_t acc_stride, hipStream_t s) {
    // area = box.intersect(edges.getRectangle()) orelse return (:79)
    const uint32_t al = l, at = t, ar = std::min(r, edges->cols), ab = std::min(b, edges->rows);
    if (al >= ar || at >= ab) return ZG_OK;
    const uint32_t w = ar - al, ht = ab - at, size = h->size;
    const uint64_t area = (uint64_t)w * ht;
    // scratch: [the list's length][the list]
    ScratchBlock sc(s);
    uint32_t *n, *list;
    sc.take(n, 1);
    sc.take(list, area);
    int rc;
    if ((rc = sc.alloc())) return rc;
    if ((rc = fill_async(n, 0, sizeof(uint32_t), s))) return rc;
    const int32_t size_minus_one = (int32_t)size - 1;
    ListArgs la{(const uint8_t *)edges->data, edges->stride, al, at, w, ht, -size_minus_one, -size_minus_one, list, n};
    // the area starts at the box's corner (l, t), so columns and rows relative to it are relative to the box
    hipLaunchKernelGGL(k_edge_list, dim3((unsigned)((area + 256 * LIST_PER_THREAD - 1) / (256 * LIST_PER_THREAD))), dim3(256), 0, s, la);
    if ((rc = launch_ok("k_edge_list"))) return rc;
    VoteArgs va{h->tables, h->tables + size, list, n, accumulator, acc_stride, size, 0, (int32_t)(16384u * h->even_size) << 1}; // :84
    if (size <= LDS_MAX_SIZE && !direct_forced()) {
        va.strip = std::min(size, LDS_COUNTERS / lds_pitch(size));
        const unsigned strips = ceil_div(size, va.strip);
        const unsigned chunks = (unsigned)std::min<uint64_t>((area + PIXEL_CHUNK - 1) / PIXEL_CHUNK, std::max(1u, LDS_VOTE_GROUPS / strips));
        hipLaunchKernelGGL(k_vote_lds, dim3(strips, chunks), dim3(256), 0, s, va);
        return launch_ok("k_vote_lds");
    }
    const unsigned groups = ceil_div(size, DIRECT_THETAS);
    const unsigned blocks = (unsigned)std::min<uint64_t>((area + 255) / 256, std::max(1u, 4 * MAX_VOTE_GROUPS / groups));
    hipLaunchKernelGGL(k_vote_direct, dim3(blocks, groups), dim3(256), 0, s, va);
    return launch_ok("k_vote_direct");
}

int check_find(zg_hough_t h, const uint32_t *accumulator, size_t acc_stride, uint32_t max_candidates, const zg_hough_line *lines, uint32_t capacity,
               const uint32_t *counts) {
    ZG_REQUIRE(h != nullptr, ZG_ERR_INVALID_ARGUMENT, "hough find_lines: null transform");
    ZG_REQUIRE(accumulator != nullptr, ZG_ERR_INVALID_ARGUMENT, "hough find_lines: null accumulator");
    ZG_REQUIRE(acc_stride >= h->size, ZG_ERR_INVALID_ARGUMENT, "hough find_lines: accumulator stride %zu is below size %u", acc_stride, h->size);
    ZG_REQUIRE(counts != nullptr, ZG_ERR_INVALID_ARGUMENT, "hough find_lines: null counts");
    ZG_REQUIRE(lines != nullptr || capacity == 0, ZG_ERR_INVALID_ARGUMENT, "hough find_lines: null lines with capacity %u", capacity);
    ZG_REQUIRE(max_candidates <= ZG_HOUGH_MAX_CANDIDATES, ZG_ERR_UNSUPPORTED, "hough find_lines: max_candidates %u is above %u", max_candidates,
               ZG_HOUGH_MAX_CANDIDATES);
    ZG_REQUIRE(h->tables != nullptr, ZG_ERR_HIP, "hough find_lines: the transform was created without a device");
    return ZG_OK;
}

int find_lines(zg_hough_t h, const uint32_t *accumulator, size_t acc_stride, uint32_t threshold, const uint32_t *threshold_device, float angle_thresh,
               float radius_thresh, uint32_t max_candidates, zg_hough_line *lines, uint32_t capacity, uint32_t *counts, hipStream_t s) {
    const uint32_t size = h->size;
    if (size < 3) return fill_async(counts, 0, 2 * sizeof(uint32_t), s); // :154
    const uint32_t inner = size - 2, maxc = std::max(max_candidates, 1u);
    // scratch: [row counts][row offsets][candidates][sorted][kept angle][kept radius][kept]
    PeakArgs pa{};
    GreedyArgs ga{};
    ScratchBlock sc(s);
    sc.take(pa.row_counts, inner);
    sc.take(pa.row_offsets, inner);
    sc.take(pa.cand, maxc);
    sc.take(pa.sorted, maxc);
    sc.take(ga.kept_angle, maxc);
    sc.take(ga.kept_radius, maxc);
    sc.take(ga.kept, maxc);
    int rc;
    if ((rc = sc.alloc())) return rc;
    pa.acc = accumulator;
    pa.acc_stride = acc_stride;
    pa.size = size;
    pa.threshold = threshold;
    pa.threshold_device = threshold_device;
    pa.max_candidates = max_candidates;
    pa.counts = counts;
    ga.sorted = pa.sorted;
    ga.size = size;
    ga.even_size = h->even_size;
    ga.max_candidates = max_candidates;
    ga.angle_thresh = angle_thresh;
    ga.radius_thresh = radius_thresh;
    ga.lines = lines;
    ga.capacity = capacity;
    ga.counts = counts;
    hipLaunchKernelGGL(k_peak_rows<false>, dim3(inner), dim3(256), 0, s, pa);
    if ((rc = launch_ok("k_peak_rows<count>"))) return rc;
    hipLaunchKernelGGL(k_row_offsets, dim3(1), dim3(256), 0, s, pa);
    if ((rc = launch_ok("k_row_offsets"))) return rc;
    if (max_candidates > 0) {
        hipLaunchKernelGGL(k_peak_rows<true>, dim3(inner), dim3(256), 0, s, pa);
        if ((rc = launch_ok("k_peak_rows<emit>"))) return rc;
        hipLaunchKernelGGL(k_rank_sort, dim3(ceil_div(max_candidates, 256)), dim3(256), 0, s, pa);
        if ((rc = launch_ok("k_rank_sort"))) return rc;
    }
    hipLaunchKernelGGL(k_greedy, dim3(1), dim3(256), 0, s, ga);
    if ((rc = launch_ok("k_greedy"))) return rc;
    const uint32_t room = std::min(capacity, max_candidates);
    if (room == 0) return ZG_OK;
    hipLaunchKernelGGL(k_lines, dim3(ceil_div(room, 256)), dim3(256), 0, s, ga);
    return launch_ok("k_lines");
}

} // namespace
} // namespace zg

using namespace zg;

extern "C" {

uint32_t zg_hough_lds_max_size(void) { return LDS_MAX_SIZE; }
uint32_t zg_hough_pixel_chunk(void) { return PIXEL_CHUNK; }

int zg_hough_tables_host(uint32_t size, int32_t *cos_table, int32_t *sin_table) {
    int rc;
    if ((rc = check_size(size))) return rc;
    ZG_REQUIRE(cos_table != nullptr && sin_table != nullptr, ZG_ERR_INVALID_ARGUMENT, "hough tables: null table");
    tables(size, cos_table, sin_table);
    return ZG_OK;
}

int zg_hough_create(uint32_t size, zg_hough_t *out) {
    int rc;
    if ((rc = check_size(size))) return rc;
    ZG_REQUIRE(out != nullptr, ZG_ERR_INVALID_ARGUMENT, "hough create: null out");
    std::vector<int32_t> t(2 * (size_t)size);
    tables(size, t.data(), t.data() + size);
    return create(size, t.data(), t.data() + size, out);
}

int zg_hough_create_with_tables(uint32_t size, const int32_t *cos_table, const int32_t *sin_table, zg_hough_t *out) {
    int rc;
    if ((rc = check_size(size))) return rc;
    ZG_REQUIRE(out != nullptr, ZG_ERR_INVALID_ARGUMENT, "hough create: null out");
    ZG_REQUIRE(cos_table != nullptr && sin_table != nullptr, ZG_ERR_INVALID_ARGUMENT, "hough create: null table");
    return create(size, cos_table, sin_table, out);
}

int zg_hough_destroy(zg_hough_t h) {
    if (!h) return ZG_OK;
    const hipError_t e = h->tables ? hipFree(h->tables) : hipSuccess;
    delete h;
    if (e != hipSuccess) return hip_fail(e, "hipFree(hough tables)", __FILE__, __LINE__);
    return ZG_OK;
}

uint32_t zg_hough_size(zg_hough_t h) { return h ? h->size : 0; }

int zg_hough_compute(zg_hough_t h, const zg_image *edges, uint32_t l, uint32_t t, uint32_t r, uint32_t b, uint32_t *accumulator, size_t acc_stride,
                     zg_stream stream) {
    int rc;
    if ((rc = check_compute(h, edges, l, t, r, b, accumulator, acc_stride, true))) return rc;
    return compute(h, edges, l, t, r, b, accumulator, acc_stride, as_stream(stream));
}

int zg_hough_find_lines(zg_hough_t h, const uint32_t *accumulator, size_t acc_stride, uint32_t threshold, const uint32_t *threshold_device,
                        float angle_nms_thresh, float radius_nms_thresh, uint32_t max_candidates, zg_hough_line *lines, uint32_t capacity,
                        uint32_t *counts, zg_stream stream) {
    int rc;
    if ((rc = check_find(h, accumulator, acc_stride, max_candidates, lines, capacity, counts))) return rc;
    return find_lines(h, accumulator, acc_stride, threshold, threshold_device, angle_nms_thresh, radius_nms_thresh, max_candidates, lines, capacity,
                      counts, as_stream(stream));
}

int zg_hough_compute_host(zg_hough_t h, const zg_image *edges, uint32_t l, uint32_t t, uint32_t r, uint32_t b, uint32_t *accumulator, size_t acc_stride) {
    int rc;
    if ((rc = check_compute(h, edges, l, t, r, b, accumulator, acc_stride, false))) return rc;
    const uint32_t size = h->size;
    const size_t row_b = (size_t)size * sizeof(uint32_t);
    HostStage e;
    if ((rc = e.upload(edges, true, false))) return rc;
    ScratchBlock sc;
    if ((rc = sc.alloc(row_b * size))) return rc;
    if ((rc = upload_pageable_rows(sc.p, accumulator, acc_stride * sizeof(uint32_t), row_b, size, nullptr))) return rc;
    if ((rc = compute(h, &e.dev, l, t, r, b, (uint32_t *)sc.p, size, nullptr))) return rc;
    return download_pageable_rows(accumulator, acc_stride * sizeof(uint32_t), sc.p, row_b, size, nullptr);
}

int zg_hough_find_lines_host(zg_hough_t h, const uint32_t *accumulator, size_t acc_stride, uint32_t threshold, float angle_nms_thresh,
                             float radius_nms_thresh, uint32_t max_candidates, zg_hough_line *lines, uint32_t capacity, uint32_t *counts) {
    int rc;
    if ((rc = check_find(h, accumulator, acc_stride, max_candidates, lines, capacity, counts))) return rc;
    const uint32_t size = h->size, cap = std::min(capacity, max_candidates);
    const size_t row_b = (size_t)size * sizeof(uint32_t);
    // scratch: [accumulator][lines][counts]
    ScratchBlock sc;
    uint32_t *dacc, *dcounts;
    zg_hough_line *dlines;
    sc.take(dacc, (size_t)size * size);
    sc.take(dlines, cap);
    sc.take(dcounts, 2);
    if ((rc = sc.alloc())) return rc;
    if ((rc = upload_pageable_rows(dacc, accumulator, acc_stride * sizeof(uint32_t), row_b, size, nullptr))) return rc;
    if ((rc = find_lines(h, dacc, size, threshold, nullptr, angle_nms_thresh, radius_nms_thresh, max_candidates, cap ? dlines : nullptr, cap, dcounts,
                         nullptr)))
        return rc;
    return download_counted(counts, dcounts, 2, lines, dlines, cap);
}

} // extern "C"
