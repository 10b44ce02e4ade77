// match.hip — BruteForceMatcher.match / knnMatch / radiusMatch (reference src/features/matcher.zig:44-233) on the device, bit for bit.
//
// A descriptor is eight dwords; a pair costs eight XORs and eight accumulating popcounts. Set sizes are read by the kernels from the
// callers' count words (grids are sized from the capacities), so a call enqueues without knowing them:
//   match    k_nearest        a lane per query, its descriptor in eight VGPRs; the train descriptor of a step is the same for the whole
//                             wave and arrives by uniform (scalar) loads. gridDim.y workgroups share the train set in chunks of
//                             TRAIN_CHUNK and each writes a partial (best, best index, second) per query
//            k_nearest        [cross_check] the same with the roles swapped: per train descriptor its nearest query
//            k_match_decide   a lane per query: merges the partials (best = min, lowest index among equals; second = min(max(b1, b2),
//                             s1, s2)), applies the distance and ratio tests and the cross-check, notes kept or not
//            k_match_emit     compaction in query order: a workgroup sums the flags before its 256 queries, scans its own, writes
//   knn      k_rows<KNN>      a wave per query, a lane per train entry: pass 1 counts the 257 possible distances in LDS, a wave scan turns
//                             them into first positions, pass 2 walks the train set in index order and places, per distinct distance
//                             of a 64-entry step, the lanes a ballot numbers — position = entries nearer + equals before it, which
//                             is the place a stable sort by distance gives it; kept when position < k and distance <= max_distance
//   radius   k_rows<COUNT>    pass 1 alone: the row lengths
//            k_row_offsets    their exclusive sums and the total
//            k_rows<RADIUS>   both passes, placing at the row's offset
// No atomic decides an order: the LDS counters are sums, every position is computed.
#include "zg_common.h"
#include "zg_scan.h"

#include <algorithm>
#include <cfloat>
#include <cmath>

namespace zg {
namespace {

constexpr uint32_t TRAIN_CHUNK = 128;   // train descriptors a workgroup of k_nearest takes at a time
constexpr uint32_t MAX_SPLIT = 64;      // workgroups sharing one train set (partials per query)
constexpr uint32_t NONE = 0xFFFFFFFFu;  // std.math.maxInt(u32): no distance yet (:59-60)
constexpr int BINS = 257;               // distances 0 .. 256

struct DSet { // zg_descriptor_set on the device side: dwords
    const uint32_t *data;
    uint32_t capacity;
    const uint32_t *count;
};
__device__ inline uint32_t set_size(const DSet &s) { return s.count ? min(*s.count, s.capacity) : s.capacity; }

struct Desc {
    uint32_t w[8];
};
__device__ inline Desc load_desc(const uint32_t *data, uint32_t i) {
    const uint32_t *p = data + (size_t)i * 8;
    Desc d;
#pragma unroll
    for (int j = 0; j < 8; ++j) d.w[j] = p[j];
    return d;
}
__device__ inline uint32_t hamming(const Desc &a, const uint32_t *b) {
    uint32_t d = 0;
#pragma unroll
    for (int j = 0; j < 8; ++j) d += (uint32_t)__popc(a.w[j] ^ b[j]);
    return d;
}

struct Partial {
    uint32_t best, idx, second;
};
// the reference's loop (:64-74) continued over a later part of the train set whose own result is p
__device__ inline void merge(Partial &a, const Partial &p) {
    const uint32_t hi = max(a.best, p.best);
    const bool take = p.best < a.best || (p.best == a.best && p.idx < a.idx);
    a.second = min(hi, min(a.second, p.second));
    if (take) {
        a.best = p.best;
        a.idx = p.idx;
    }
}

// ---- nearest and second nearest of every a in b -----------------------------------------------------------------------------
// The b descriptor of a step is the same for every lane: its address is uniform, so its eight dwords arrive through the scalar
// cache as operands of the XORs and no lane loads anything inside the loop. Within a chunk the pair (distance, index in the chunk)
// is one key, distance << 8 | index: its minimum is the nearest entry with the lowest index, and min over the steps of
// max(best key so far, key) carries the second smallest distance in its upper bits — three instructions a pair after the popcounts.
__global__ __launch_bounds__(64) void k_nearest(DSet a, DSet b, Partial *partials) {
    static_assert(TRAIN_CHUNK <= 256, "the index in the chunk has eight bits of the key");
    const uint32_t na = set_size(a), nb = set_size(b);
    const uint32_t q = blockIdx.x * 64u + threadIdx.x;
    if (blockIdx.x * 64u >= na) return; // uniform: no query of this workgroup counts
    const bool live = q < na;
    const Desc me = load_desc(a.data, live ? q : 0u);
    const uint32_t *__restrict__ others = b.data;
    Partial r{NONE, 0u, NONE};
    for (uint32_t t0 = blockIdx.y * TRAIN_CHUNK; t0 < nb; t0 += gridDim.y * TRAIN_CHUNK) { // ascending: merge keeps the lowest index
        const uint32_t m = min(TRAIN_CHUNK, nb - t0);
        const uint32_t *p = others + (size_t)t0 * 8;
        uint32_t best = NONE, second = NONE;
#pragma unroll 8
        for (uint32_t t = 0; t < m; ++t) {
            const uint32_t key = (hamming(me, p + t * 8u) << 8) | t;
            second = min(second, max(best, key)); // :71-72, and :68 when key becomes the best
            best = min(best, key);                // :67-70
        }
        merge(r, Partial{best >> 8, t0 + (best & 255u), second == NONE ? NONE : second >> 8});
    }
    if (live) partials[(size_t)blockIdx.y * a.capacity + q] = r;
}

__device__ inline Partial merged(const Partial *partials, uint32_t split, uint32_t capacity, uint32_t i) {
    Partial r = partials[i];
#pragma unroll 8
    for (uint32_t y = 1; y < split; ++y) merge(r, partials[(size_t)y * capacity + i]); // independent loads: several in flight
    return r;
}

struct MatchArgs {
    DSet query, train;
    const Partial *fwd, *rev; // rev: null without the cross-check
    uint32_t split_f, split_r;
    uint32_t max_distance;
    float ratio;
    uint2 *cand;      // [query capacity] train index, distance
    uint32_t *keep;   // [query capacity] 0 / 1
    zg_match *out;
    uint32_t capacity;
    uint32_t *count;
};

__global__ __launch_bounds__(64) void k_match_decide(MatchArgs a) { // a wave a workgroup: the merge is a chain of loads, so many small workgroups
    const uint32_t q = blockIdx.x * 64u + threadIdx.x;
    if (q >= a.query.capacity) return;
    const uint32_t nq = set_size(a.query), nt = set_size(a.train);
    uint32_t keep = 0;
    if (q < nq && nt > 0) { // :50
        const Partial r = merged(a.fwd, a.split_f, a.query.capacity, q);
        const float best_f = (float)r.best, second_f = (float)r.second;
        if (r.best <= a.max_distance && (r.second == NONE || best_f < a.ratio * second_f)) { // :80-82
            keep = 1;
            if (a.rev) keep = merged(a.rev, a.split_r, a.train.capacity, r.idx).idx == q; // :87-88
            a.cand[q] = make_uint2(r.idx, r.best);
        }
    }
    a.keep[q] = keep;
}

// The exclusive sum of v over the grid's threads in thread order, from values[0 .. n): every workgroup adds up what lies before
// its own 256 values and scans those. Returns the calling thread's sum; *total (when the workgroup is the last) the sum of all.
__device__ inline uint32_t grid_exclusive_sum(const uint32_t *values, uint32_t n, uint32_t *total) {
    __shared__ uint32_t wave_sum[4], before_sum[4];
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wv = tid >> 6, first = blockIdx.x * 256u;
    uint32_t before = 0;
    for (uint32_t i = tid; i < first; i += 256u) before += values[i];
    const uint32_t v = first + tid < n ? values[first + tid] : 0u, incl = wave_inclusive_sum(v);
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) before += __shfl_xor(before, off);
    if (lane == 63u) wave_sum[wv] = incl;
    if (lane == 0u) before_sum[wv] = before;
    __syncthreads();
    uint32_t base = 0, all = 0;
    for (uint32_t k = 0; k < 4; ++k) {
        base += before_sum[k] + (k < wv ? wave_sum[k] : 0u);
        all += before_sum[k] + wave_sum[k];
    }
    *total = all;
    return base + incl - v;
}

__global__ __launch_bounds__(256) void k_match_emit(MatchArgs a) {
    const uint32_t q = blockIdx.x * 256u + threadIdx.x;
    uint32_t total;
    const uint32_t pos = grid_exclusive_sum(a.keep, a.query.capacity, &total);
    if (q < a.query.capacity && a.keep[q] && pos < a.capacity) {
        const uint2 c = a.cand[q];
        a.out[pos] = zg_match{q, c.x, (float)c.y};
    }
    if (blockIdx.x == gridDim.x - 1 && threadIdx.x == 0) *a.count = total;
}

// ---- rows: knn and radius --------------------------------------------------------------------------------------------------
enum { ROWS_KNN = 0, ROWS_COUNT = 1, ROWS_RADIUS = 2 };
struct RowArgs {
    DSet query, train;
    uint32_t k;            // KNN
    uint32_t max_d;        // entries above it are left out: min(max_distance, 256), or floor(max_dist)
    zg_match *out;
    uint32_t capacity;     // RADIUS: entries of out
    uint32_t *row_counts;  // KNN, COUNT: written
    const uint32_t *offsets; // RADIUS: first entry of every row
};

template <int MODE> __global__ __launch_bounds__(256) void k_rows(RowArgs a) {
    __shared__ uint32_t hist_s[4][BINS + 3], first_s[4][BINS + 3];
    const uint32_t lane = threadIdx.x & 63u, wv = threadIdx.x >> 6;
    uint32_t *hist = hist_s[wv], *first = first_s[wv];
    const uint32_t nq = set_size(a.query), nt = set_size(a.train);
    const uint64_t below = (1ull << lane) - 1ull;
    for (uint32_t q = blockIdx.x * 4u + wv; q < a.query.capacity; q += gridDim.x * 4u) { // uniform per wave; a wave's LDS is its own
        if (q >= nq || nt == 0) {
            if (MODE != ROWS_RADIUS && lane == 0) a.row_counts[q] = 0;
            continue;
        }
        const Desc me = load_desc(a.query.data, q);
        for (uint32_t i = lane; i < (uint32_t)BINS; i += 64u) hist[i] = 0;
        __builtin_amdgcn_wave_barrier();
        for (uint32_t t0 = 0; t0 < nt; t0 += 64u) {
            const uint32_t t = t0 + lane;
            if (t < nt) {
                const Desc o = load_desc(a.train.data, t);
                const uint32_t d = hamming(me, o.w);
                if (d <= a.max_d) atomicAdd(&hist[d], 1u); // farther entries are never placed and never counted: no row position depends on them
            }
        }
        __builtin_amdgcn_wave_barrier();
        // first[d] = entries nearer than d: lane l owns bins 4 l .. 4 l + 3, bin 256 follows them all
        const uint32_t h0 = hist[4 * lane], h1 = hist[4 * lane + 1], h2 = hist[4 * lane + 2], h3 = hist[4 * lane + 3];
        const uint32_t mine = h0 + h1 + h2 + h3;
        const uint32_t incl = wave_inclusive_sum(mine), ex = incl - mine;
        first[4 * lane] = ex;
        first[4 * lane + 1] = ex + h0;
        first[4 * lane + 2] = ex + h0 + h1;
        first[4 * lane + 3] = ex + h0 + h1 + h2;
        if (lane == 63u) first[256] = incl;
        __builtin_amdgcn_wave_barrier();
        const uint32_t within = a.max_d >= 256u ? nt : first[a.max_d + 1]; // entries with distance <= max_d
        const uint32_t limit = MODE == ROWS_KNN ? min(a.k, nt) : nt;       // positions a row may hold (:150)
        const uint32_t length = min(limit, within);
        if (MODE != ROWS_RADIUS && lane == 0) a.row_counts[q] = length;
        if (MODE == ROWS_COUNT || length == 0) continue;
        const size_t base = MODE == ROWS_KNN ? (size_t)q * a.k : (size_t)a.offsets[q];
        // pass 2: first[d] becomes the next free position of distance d as the walk goes up the train indices
        for (uint32_t t0 = 0; t0 < nt; t0 += 64u) {
            const uint32_t t = t0 + lane;
            uint32_t d = NONE;
            if (t < nt) {
                const Desc o = load_desc(a.train.data, t);
                d = hamming(me, o.w);
            }
            bool todo = d <= a.max_d && first[min(d, 256u)] < length; // its distance still has room in the row
            uint64_t left = __ballot(todo);
            while (left) {
                const uint32_t dd = __shfl(d, __ffsll((long long)left) - 1);
                const uint64_t same = __ballot(todo && d == dd);
                const uint32_t start = first[dd];
                __builtin_amdgcn_wave_barrier();
                if (todo && d == dd) {
                    const uint32_t pos = start + (uint32_t)__popcll(same & below);
                    if (pos < length && (MODE == ROWS_KNN || base + pos < a.capacity)) a.out[base + pos] = zg_match{q, t, (float)d};
                    todo = false;
                }
                if (lane == 0) first[dd] = start + (uint32_t)__popcll(same);
                __builtin_amdgcn_wave_barrier();
                left &= ~same;
            }
        }
        __builtin_amdgcn_wave_barrier();
    }
}

struct OffsetArgs {
    const uint32_t *row_counts;
    uint32_t n;
    uint32_t *offsets, *count;
};
__global__ __launch_bounds__(256) void k_row_offsets(OffsetArgs a) {
    const uint32_t q = blockIdx.x * 256u + threadIdx.x;
    uint32_t total;
    const uint32_t off = grid_exclusive_sum(a.row_counts, a.n, &total);
    if (q < a.n) a.offsets[q] = off;
    if (blockIdx.x == gridDim.x - 1 && threadIdx.x == 0) *a.count = total;
}

// ---- host side -------------------------------------------------------------------------------------------------------------
int check_set(const zg_descriptor_set *s, const char *name) {
    ZG_REQUIRE(s != nullptr, ZG_ERR_INVALID_ARGUMENT, "match: null %s set", name);
    ZG_REQUIRE(s->data != nullptr || s->capacity == 0, ZG_ERR_INVALID_ARGUMENT, "match: %s has capacity %u and null data", name, s->capacity);
    ZG_REQUIRE(((uintptr_t)s->data & 3u) == 0, ZG_ERR_INVALID_ARGUMENT, "match: %s data %p is not 4-byte aligned", name, (const void *)s->data);
    return ZG_OK;
}
int check_params(const zg_matcher_params *p) {
    ZG_REQUIRE(p != nullptr, ZG_ERR_INVALID_ARGUMENT, "match: null params");
    return ZG_OK;
}
DSet dset(const zg_descriptor_set *s) { return DSet{(const uint32_t *)s->data, s->capacity, s->count}; }
uint32_t split_of(uint32_t capacity) { // workgroups per train set, each with the same number of chunks but the last
    const uint32_t chunks = std::max(1u, ceil_div(capacity, TRAIN_CHUNK));
    return ceil_div(chunks, ceil_div(chunks, MAX_SPLIT));
}
unsigned row_blocks(uint32_t capacity) { return std::min(ceil_div(capacity, 4), 1u << 16); }

int match(const zg_descriptor_set *query, const zg_descriptor_set *train, const zg_matcher_params *p, zg_match *matches, uint32_t capacity,
          uint32_t *count, hipStream_t s) {
    const uint32_t cq = query->capacity, ct = train->capacity;
    if (cq == 0 || ct == 0) return fill_async(count, 0, sizeof(uint32_t), s); // :50
    MatchArgs a{};
    a.query = dset(query);
    a.train = dset(train);
    a.split_f = split_of(ct);
    a.split_r = p->cross_check ? split_of(cq) : 0;
    a.max_distance = p->max_distance;
    a.ratio = p->ratio_threshold;
    a.out = matches;
    a.capacity = capacity;
    a.count = count;
    // scratch: [forward partials][reverse partials][cand][keep]
    ScratchBlock sc(s);
    Partial *fwd, *rev;
    sc.take(fwd, (size_t)a.split_f * cq);
    sc.take(rev, (size_t)a.split_r * ct);
    sc.take(a.cand, cq);
    sc.take(a.keep, cq);
    int rc;
    if ((rc = sc.alloc())) return rc;
    a.fwd = fwd;
    a.rev = p->cross_check ? rev : nullptr;
    hipLaunchKernelGGL(k_nearest, dim3(ceil_div(cq, 64), a.split_f), dim3(64), 0, s, a.query, a.train, fwd);
    if ((rc = launch_ok("k_nearest"))) return rc;
    if (p->cross_check) {
        hipLaunchKernelGGL(k_nearest, dim3(ceil_div(ct, 64), a.split_r), dim3(64), 0, s, a.train, a.query, rev);
        if ((rc = launch_ok("k_nearest (cross-check)"))) return rc;
    }
    hipLaunchKernelGGL(k_match_decide, dim3(ceil_div(cq, 64)), dim3(64), 0, s, a);
    if ((rc = launch_ok("k_match_decide"))) return rc;
    hipLaunchKernelGGL(k_match_emit, dim3(ceil_div(cq, 256)), dim3(256), 0, s, a);
    return launch_ok("k_match_emit");
}

int knn(const zg_descriptor_set *query, const zg_descriptor_set *train, const zg_matcher_params *p, uint32_t k, zg_match *matches,
        uint32_t *row_counts, hipStream_t s) {
    const uint32_t cq = query->capacity;
    if (cq == 0) return ZG_OK;
    if (k == 0 || train->capacity == 0) return fill_async(row_counts, 0, (size_t)cq * sizeof(uint32_t), s); // :116
    RowArgs a{};
    a.query = dset(query);
    a.train = dset(train);
    a.k = k;
    a.max_d = std::min(p->max_distance, 256u);
    a.out = matches;
    a.row_counts = row_counts;
    hipLaunchKernelGGL(k_rows<ROWS_KNN>, dim3(row_blocks(cq)), dim3(256), 0, s, a);
    return launch_ok("k_rows<knn>");
}

int radius(const zg_descriptor_set *query, const zg_descriptor_set *train, float max_dist, zg_match *matches, uint32_t capacity,
           uint32_t *row_counts, uint32_t *count, hipStream_t s) {
    const uint32_t cq = query->capacity;
    int rc;
    if (cq == 0) return fill_async(count, 0, sizeof(uint32_t), s);
    if (!(max_dist >= 0.0f) || train->capacity == 0) { // f32(dist) <= max_dist never holds (:195), or :173
        if ((rc = fill_async(row_counts, 0, (size_t)cq * sizeof(uint32_t), s))) return rc;
        return fill_async(count, 0, sizeof(uint32_t), s);
    }
    RowArgs a{};
    a.query = dset(query);
    a.train = dset(train);
    a.max_d = max_dist >= 256.0f ? 256u : (uint32_t)max_dist; // an integer d has f32(d) <= max_dist exactly when d <= floor(max_dist)
    a.out = matches;
    a.capacity = capacity;
    a.row_counts = row_counts;
    ScratchBlock sc(s);
    if ((rc = sc.alloc(align256((size_t)cq * sizeof(uint32_t))))) return rc;
    a.offsets = (const uint32_t *)sc.p;
    hipLaunchKernelGGL(k_rows<ROWS_COUNT>, dim3(row_blocks(cq)), dim3(256), 0, s, a);
    if ((rc = launch_ok("k_rows<count>"))) return rc;
    hipLaunchKernelGGL(k_row_offsets, dim3(ceil_div(cq, 256)), dim3(256), 0, s, OffsetArgs{row_counts, cq, (uint32_t *)sc.p, count});
    if ((rc = launch_ok("k_row_offsets"))) return rc;
    if (capacity == 0) return ZG_OK;
    hipLaunchKernelGGL(k_rows<ROWS_RADIUS>, dim3(row_blocks(cq)), dim3(256), 0, s, a);
    return launch_ok("k_rows<radius>");
}

int check_knn(const zg_descriptor_set *query, uint32_t k) {
    ZG_REQUIRE((uint64_t)query->capacity * k < (1ull << 32), ZG_ERR_UNSUPPORTED, "match knn: %u queries x k = %u is 2^32 entries or more", query->capacity, k);
    return ZG_OK;
}
int check_radius(const zg_descriptor_set *query, const zg_descriptor_set *train) {
    ZG_REQUIRE((uint64_t)query->capacity * train->capacity < (1ull << 32), ZG_ERR_UNSUPPORTED, "match radius: %u x %u descriptors is 2^32 pairs or more",
               query->capacity, train->capacity);
    return ZG_OK;
}

// A host set on the device: its first n = min(*count, capacity) descriptors, with the size settled here.
struct Staged {
    zg_descriptor_set set{};
    uint32_t n = 0;
};
uint32_t host_size(const zg_descriptor_set *s) { return s->count ? std::min(*s->count, s->capacity) : s->capacity; }
// Both sets at the head of a block whose other parts the caller has still to take: [query][train][the caller's parts]. stage_upload
// follows the block's alloc().
void stage(const zg_descriptor_set *query, const zg_descriptor_set *train, ScratchBlock *sc, Staged *q, Staged *t) {
    q->n = host_size(query);
    t->n = host_size(train);
    q->set = zg_descriptor_set{nullptr, q->n, nullptr};
    t->set = zg_descriptor_set{nullptr, t->n, nullptr};
    sc->take(q->set.data, q->n);
    sc->take(t->set.data, t->n);
}
int stage_upload(const zg_descriptor_set *query, const zg_descriptor_set *train, const Staged &q, const Staged &t) {
    if (const int rc = upload_pageable((void *)q.set.data, query->data, (size_t)q.n * 32, nullptr)) return rc;
    return upload_pageable((void *)t.set.data, train->data, (size_t)t.n * 32, nullptr);
}

} // namespace
} // namespace zg

using namespace zg;

extern "C" {

void zg_matcher_default_params(zg_matcher_params *p) {
    if (!p) return;
    *p = zg_matcher_params{0, 64, 0.8f};
}

uint32_t zg_match_train_chunk(void) { return TRAIN_CHUNK; }

int zg_match_descriptors(const zg_descriptor_set *query, const zg_descriptor_set *train, const zg_matcher_params *params, zg_match *matches,
                         uint32_t capacity, uint32_t *count, zg_stream stream) {
    int rc;
    if ((rc = check_set(query, "query")) || (rc = check_set(train, "train")) || (rc = check_params(params))) return rc;
    ZG_REQUIRE(count != nullptr, ZG_ERR_INVALID_ARGUMENT, "match: null count");
    ZG_REQUIRE(matches != nullptr || capacity == 0, ZG_ERR_INVALID_ARGUMENT, "match: null matches with capacity %u", capacity);
    return match(query, train, params, matches, capacity, count, as_stream(stream));
}

int zg_match_knn(const zg_descriptor_set *query, const zg_descriptor_set *train, const zg_matcher_params *params, uint32_t k, zg_match *matches,
                 uint32_t *row_counts, zg_stream stream) {
    int rc;
    if ((rc = check_set(query, "query")) || (rc = check_set(train, "train")) || (rc = check_params(params)) || (rc = check_knn(query, k))) return rc;
    ZG_REQUIRE(row_counts != nullptr || query->capacity == 0, ZG_ERR_INVALID_ARGUMENT, "match knn: null row_counts");
    ZG_REQUIRE(matches != nullptr || query->capacity == 0 || k == 0, ZG_ERR_INVALID_ARGUMENT, "match knn: null matches");
    return knn(query, train, params, k, matches, row_counts, as_stream(stream));
}

int zg_match_radius(const zg_descriptor_set *query, const zg_descriptor_set *train, float max_dist, zg_match *matches, uint32_t capacity,
                    uint32_t *row_counts, uint32_t *count, zg_stream stream) {
    int rc;
    if ((rc = check_set(query, "query")) || (rc = check_set(train, "train")) || (rc = check_radius(query, train))) return rc;
    ZG_REQUIRE(count != nullptr, ZG_ERR_INVALID_ARGUMENT, "match radius: null count");
    ZG_REQUIRE(row_counts != nullptr || query->capacity == 0, ZG_ERR_INVALID_ARGUMENT, "match radius: null row_counts");
    ZG_REQUIRE(matches != nullptr || capacity == 0, ZG_ERR_INVALID_ARGUMENT, "match radius: null matches with capacity %u", capacity);
    return radius(query, train, max_dist, matches, capacity, row_counts, count, as_stream(stream));
}

int zg_match_descriptors_host(const zg_descriptor_set *query, const zg_descriptor_set *train, const zg_matcher_params *params, zg_match *matches,
                              uint32_t capacity, uint32_t *count) {
    int rc;
    if ((rc = check_set(query, "query")) || (rc = check_set(train, "train")) || (rc = check_params(params))) return rc;
    ZG_REQUIRE(count != nullptr, ZG_ERR_INVALID_ARGUMENT, "match: null count");
    ZG_REQUIRE(matches != nullptr || capacity == 0, ZG_ERR_INVALID_ARGUMENT, "match: null matches with capacity %u", capacity);
    ScratchBlock sc;
    Staged q, t;
    stage(query, train, &sc, &q, &t);
    const uint32_t cap = std::min(capacity, q.n); // a match per query at the most
    zg_match *dout;
    uint32_t *dcount;
    sc.take(dout, cap);
    sc.take(dcount, 1);
    if ((rc = sc.alloc()) || (rc = stage_upload(query, train, q, t))) return rc;
    if ((rc = match(&q.set, &t.set, params, cap ? dout : nullptr, cap, dcount, nullptr))) return rc;
    return download_counted(count, dcount, 1, matches, dout, cap);
}

int zg_match_knn_host(const zg_descriptor_set *query, const zg_descriptor_set *train, const zg_matcher_params *params, uint32_t k, zg_match *matches,
                      uint32_t *row_counts) {
    int rc;
    if ((rc = check_set(query, "query")) || (rc = check_set(train, "train")) || (rc = check_params(params)) || (rc = check_knn(query, k))) return rc;
    ZG_REQUIRE(row_counts != nullptr || query->capacity == 0, ZG_ERR_INVALID_ARGUMENT, "match knn: null row_counts");
    ScratchBlock sc;
    Staged q, t;
    stage(query, train, &sc, &q, &t);
    const uint32_t nq = q.n;
    zg_match *dout;
    uint32_t *drows, *spare;
    sc.take(dout, (size_t)nq * k);
    sc.take(drows, nq);
    sc.take(spare, 1); // the radius form's layout, [query][train][matches][row counts][count]: the two share a cached block
    if ((rc = sc.alloc()) || (rc = stage_upload(query, train, q, t))) return rc;
    if ((rc = knn(&q.set, &t.set, params, k, dout, drows, nullptr))) return rc;
    for (uint32_t i = nq; i < query->capacity; ++i) row_counts[i] = 0;
    if (nq == 0) return ZG_OK;
    if ((rc = download_pageable(row_counts, drows, (size_t)nq * sizeof(uint32_t), nullptr))) return rc;
    if (!matches || k == 0) return ZG_OK;
    // rows are k apart and only their first row_counts[q] entries are defined: copy those
    std::unique_ptr<zg_match[]> all(new zg_match[(size_t)nq * k]);
    if ((rc = download_pageable(all.get(), dout, (size_t)nq * k * sizeof(zg_match), nullptr))) return rc;
    for (uint32_t i = 0; i < nq; ++i) std::copy_n(all.get() + (size_t)i * k, row_counts[i], matches + (size_t)i * k);
    return ZG_OK;
}

int zg_match_radius_host(const zg_descriptor_set *query, const zg_descriptor_set *train, float max_dist, zg_match *matches, uint32_t capacity,
                         uint32_t *row_counts, uint32_t *count) {
    int rc;
    if ((rc = check_set(query, "query")) || (rc = check_set(train, "train")) || (rc = check_radius(query, train))) return rc;
    ZG_REQUIRE(count != nullptr, ZG_ERR_INVALID_ARGUMENT, "match radius: null count");
    ZG_REQUIRE(matches != nullptr || capacity == 0, ZG_ERR_INVALID_ARGUMENT, "match radius: null matches with capacity %u", capacity);
    ScratchBlock sc;
    Staged q, t;
    stage(query, train, &sc, &q, &t);
    const uint32_t nq = q.n;
    const uint32_t cap = (uint32_t)std::min<uint64_t>(capacity, (uint64_t)nq * t.n);
    zg_match *dout;
    uint32_t *drows, *dcount;
    sc.take(dout, cap);
    sc.take(drows, nq);
    sc.take(dcount, 1);
    if ((rc = sc.alloc()) || (rc = stage_upload(query, train, q, t))) return rc;
    if ((rc = radius(&q.set, &t.set, max_dist, cap ? dout : nullptr, cap, drows, dcount, nullptr))) return rc;
    if (row_counts) {
        for (uint32_t i = nq; i < query->capacity; ++i) row_counts[i] = 0;
        if (nq && (rc = download_pageable(row_counts, drows, (size_t)nq * sizeof(uint32_t), nullptr))) return rc;
    }
    return download_counted(count, dcount, 1, matches, dout, cap);
}

int zg_match_stats(const zg_match *matches, size_t n, zg_match_statistics *out) {
    ZG_REQUIRE(out != nullptr, ZG_ERR_INVALID_ARGUMENT, "match stats: null out");
    ZG_REQUIRE(matches != nullptr || n == 0, ZG_ERR_INVALID_ARGUMENT, "match stats: null matches with n = %zu", n);
    *out = zg_match_statistics{0, 0.0f, 0.0f, 0.0f};
    if (n == 0) return ZG_OK; // :244-251
    float sum = 0.0f, lo = FLT_MAX, hi = 0.0f;
    for (size_t i = 0; i < n; ++i) {
        sum += matches[i].distance;
        lo = std::min(lo, matches[i].distance);
        hi = std::max(hi, matches[i].distance);
    }
    *out = zg_match_statistics{n, sum / (float)n, lo, hi};
    return ZG_OK;
}

} // extern "C"
