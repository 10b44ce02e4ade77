// tracer.hip — Tracer.trace (reference src/features/Tracer.zig:46-236) on the device: an Image(u8) edge map to polylines, the same
// paths in the same order with the same f32 bits, asynchronous, with no host synchronisation, recordable into a graph.
//
// The reference is one sequential loop. It splits because (Tracer)
//   * followPath only steps to an 8-neighbour that is an edge, so a path stays inside the 8-connected component of its start, and
//     `visited` outside that component is never read on its behalf; the raster scan starts every path at the component's raster-first
//     unvisited pixel. The result is therefore: the same procedure on every component alone, then all paths ordered by the raster
//     index of their first point (unique: a start is visited once).
//   * a Douglas-Peucker range's decision reads only the points and its own two ends, so keep[] does not depend on the order of ranges.
// Stages:
//   k_trace_links    a byte per pixel with the links it owns to E, S, SE, SW edge neighbours (what flood.hip's labelling reads), and
//                    `open` = edge and not yet visited, dense rows x cols: the only plane the walk reads. Nothing reads `edges` later.
//   flood_label_components (flood.hip)   roots = the smallest index of each component = its first start.
//   k_trace_count    flattens label[p] to the root, counts each component's pixels and its column range at the root's index.
//   scan             exclusive sums of the counts: a component's region of the raw point buffer is as long as the component, because a
//                    pixel is visited at most once.
//   k_trace_follow   a wave per component, components handed out 1024 pixel indices at a time through an atomic queue. Lanes 0-7 read
//                    the eight neighbours' `open` bytes together, a ballot makes the mask, zg_tracer_step.h chooses. When a path ends
//                    and the component still has unvisited pixels, the wave looks for the raster-next one from a cursor that only
//                    moves forward, 64 pixels of the component's column range at a time. A kept path is simplified in place by the
//                    same wave (argmax of a range across the lanes, ties to the lowest index; ranges left to right with keep[] as the
//                    only state) and compacted; its start pixel records where it lies and how many points it kept.
//   scans + k_trace_emit   paths ordered by start pixel: exclusive sums over the pixels of (is a kept start) and (kept points) give
//                    each path its index and point offset; whole paths are written while they fit both capacities.
#include "zg_common.h"
#include "zg_internal.h"
#include "zg_scan.h"
#include "zg_tracer_step.h"
#include "zg_unionfind.h"

#include <cstring>

#pragma clang fp contract(off)

namespace zg {
namespace {

constexpr uint32_t SCAN_PER = 8, SCAN_BLOCK = 256 * SCAN_PER; // items a thread / a workgroup scans
constexpr uint32_t FOLLOW_MAX_WAVES = 8192, FOLLOW_GRAB = 1024; // pixel indices a wave takes from the queue at a time

struct TraceBuf {
    // zeroed before every run, contiguous in this order
    uint32_t *cnt;   // n + 1: pixels of the component rooted here, then its region's offset; after the walk, the point offsets of the paths
    uint32_t *cmax;  // n: the largest column of the component rooted here
    uint32_t *pcnt;  // n: the points kept by the path that starts here, 0: none
    uint32_t *queue; // [0] the next pixel index to hand out
    // written before they are read
    uint32_t *cmin;  // n: the smallest column of the component rooted here (set to all ones first)
    uint8_t *links;  // n
    uint8_t *open;   // n
    uint8_t *keep;   // n, indexed like raw
    int *label;      // n + 1: parents, then roots; after the walk, the path indices
    uint32_t *poff;  // n: where in raw the path that starts here lies
    float2 *raw;     // n: the points of the paths, a region per component
    uint32_t *tmp;   // the scans' block sums
};

size_t scan_tmp_words(size_t m) {
    size_t words = 0;
    while (m > 1) {
        m = (m + SCAN_BLOCK - 1) / SCAN_BLOCK;
        words += align256(m * 4) / 4;
    }
    return words + 64;
}

void plan(ScratchBlock &sc, TraceBuf &b, size_t n) {
    sc.take(b.cnt, n + 1);
    sc.take(b.cmax, n);
    sc.take(b.pcnt, n);
    sc.take(b.queue, 64);
    sc.take(b.cmin, n);
    sc.take(b.links, n);
    sc.take(b.open, n);
    sc.take(b.keep, n);
    sc.take(b.label, n + 1);
    sc.take(b.poff, n);
    sc.take(b.raw, n);
    sc.take(b.tmp, scan_tmp_words(n + 1));
}

__global__ __launch_bounds__(256) void k_trace_links(const uint8_t *edges, uint64_t stride, int rows, int cols, uint8_t *links, uint8_t *open) {
    const int n = rows * cols;
    const int p = (int)(blockIdx.x * 256u + threadIdx.x);
    if (p >= n) return;
    const int r = p / cols, c = p - r * cols;
    auto edge = [&](int rr, int cc) { return edges[(size_t)rr * stride + (size_t)cc] > 0; };
    uint8_t bits = 0;
    const bool e = edge(r, c);
    if (e) {
        const bool has_e = c + 1 < cols, has_s = r + 1 < rows, has_w = c > 0;
        if (has_e && edge(r, c + 1)) bits |= FLOOD_LINK_E;
        if (has_s) {
            if (edge(r + 1, c)) bits |= FLOOD_LINK_S;
            if (has_e && edge(r + 1, c + 1)) bits |= FLOOD_LINK_SE;
            if (has_w && edge(r + 1, c - 1)) bits |= FLOOD_LINK_SW;
        }
    }
    links[p] = bits;
    open[p] = e ? 1 : 0;
}

__global__ __launch_bounds__(256) void k_trace_count(int *label, const uint8_t *open, int n, int cols, uint32_t *cnt, uint32_t *cmin, uint32_t *cmax) {
    const int p = (int)(blockIdx.x * 256u + threadIdx.x);
    if (p >= n || !open[p]) return;
    // The forest is final, so this is the root. The walk up writes nothing: cc_find's path halving stores a grandparent it read earlier,
    // and in this kernel that store could land after p's own thread had written the root, leaving label[p] short of it. With this one
    // store a pixel the only writes, a reader passing through p sees its old parent or its root, an ancestor either way.
    int root = p;
    for (int up = label[root]; up != root; up = label[root]) root = up;
    label[p] = root;
    const uint32_t c = (uint32_t)(p % cols);
    atomicAdd(&cnt[root], 1u);
    atomicMin(&cmin[root], c);
    atomicMax(&cmax[root], c);
}

// ---- exclusive sums of u32 over a whole array, in place: a workgroup scans SCAN_BLOCK items, the block totals are scanned the same way
__global__ __launch_bounds__(256) void k_trace_scan_block(uint32_t *data, uint32_t m, uint32_t *sums) {
    const uint32_t i0 = (blockIdx.x * 256u + threadIdx.x) * SCAN_PER;
    uint32_t v[SCAN_PER], local = 0;
#pragma unroll
    for (uint32_t j = 0; j < SCAN_PER; ++j) {
        v[j] = i0 + j < m ? data[i0 + j] : 0u;
        local += v[j];
    }
    uint32_t total;
    uint32_t run = block_exclusive_sum(local, &total);
#pragma unroll
    for (uint32_t j = 0; j < SCAN_PER; ++j) {
        if (i0 + j < m) data[i0 + j] = run;
        run += v[j];
    }
    if (threadIdx.x == 0) sums[blockIdx.x] = total;
}
__global__ __launch_bounds__(256) void k_trace_scan_add(uint32_t *data, uint32_t m, const uint32_t *sums) {
    const uint32_t i0 = (blockIdx.x * 256u + threadIdx.x) * SCAN_PER;
    const uint32_t add = sums[blockIdx.x];
#pragma unroll
    for (uint32_t j = 0; j < SCAN_PER; ++j)
        if (i0 + j < m) data[i0 + j] += add;
}
int scan_u32(uint32_t *data, size_t m, uint32_t *tmp, hipStream_t s) {
    const unsigned blocks = (unsigned)((m + SCAN_BLOCK - 1) / SCAN_BLOCK);
    k_trace_scan_block<<<blocks, 256, 0, s>>>(data, (uint32_t)m, tmp);
    int rc;
    if ((rc = launch_ok("k_trace_scan_block"))) return rc;
    if (blocks == 1) return ZG_OK;
    if ((rc = scan_u32(tmp, blocks, tmp + align256((size_t)blocks * 4) / 4, s))) return rc;
    k_trace_scan_add<<<blocks, 256, 0, s>>>(data, (uint32_t)m, tmp);
    return launch_ok("k_trace_scan_add");
}

// ---- the walk ----------------------------------------------------------------------------------------------------------------

struct FollowArgs {
    int rows, cols, n;
    uint32_t min_len;
    float eps;
    int simplify;
    const int *label;
    uint8_t *open, *keep;
    const uint32_t *cnt, *cmin, *cmax;
    uint32_t *poff, *pcnt, *queue;
    float2 *raw;
};

__device__ inline int first_lane(unsigned long long m) { return __ffsll((long long)m) - 1; }
// stores of one lane that other lanes of the wave load later: a wave's memory operations execute in order, this keeps the compiler to it
__device__ inline void wave_order() { __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront"); }

// simplifyPath + douglasPeucker (:176-236) on pts[0 .. len), len >= 3, by one wave; the kept points end up in pts[0 .. return value)
__device__ inline uint32_t simplify_wave(float2 *pts, uint8_t *keep, uint32_t len, float eps, uint32_t lane) {
    for (uint32_t i = lane; i < len; i += 64) keep[i] = (i == 0 || i == len - 1) ? 1 : 0;
    wave_order();
    uint32_t a = 0, b = len - 1;
    for (;;) {
        if (b > a + 1) {
            const float2 first = pts[a], last = pts[b];
            float best_d = 0.0f; // max_dist = 0, d > max_dist strict: a range whose distances are all 0 keeps nothing
            uint32_t best_i = 0;
            for (uint32_t i = a + 1 + lane; i < b; i += 64) {
                const float2 p = pts[i];
                const float d = tracer_distance_to_segment(p.x, p.y, first.x, first.y, last.x, last.y);
                if (d > best_d) {
                    best_d = d;
                    best_i = i;
                }
            }
#pragma unroll
            for (int off = 32; off >= 1; off >>= 1) { // the largest distance, the lowest index among equals
                const float od = __shfl_xor(best_d, off);
                const uint32_t oi = __shfl_xor(best_i, off);
                if (od > best_d || (od == best_d && oi < best_i)) {
                    best_d = od;
                    best_i = oi;
                }
            }
            if (best_d > eps) {
                if (lane == 0) keep[best_i] = 1;
                wave_order();
                b = best_i;
                continue;
            }
        }
        a = b; // everything up to b is final
        if (a == len - 1) break;
        b = len - 1;
        for (uint32_t j0 = a + 1; j0 < len; j0 += 64) { // the next kept point: keep[len - 1] is the last one there can be
            const uint32_t j = j0 + lane;
            const unsigned long long m = __ballot(j < len && keep[j] != 0);
            if (m) {
                b = j0 + (uint32_t)first_lane(m);
                break;
            }
        }
    }
    uint32_t out = 0;
    for (uint32_t j0 = 0; j0 < len; j0 += 64) { // a write lands at or before what this step read; later steps' points are untouched
        const uint32_t j = j0 + lane;
        const bool k = j < len && keep[j] != 0;
        float2 p = make_float2(0.0f, 0.0f);
        if (k) p = pts[j];
        const unsigned long long m = __ballot(k);
        wave_order();
        if (k) pts[out + (uint32_t)__popcll(m & ((1ull << lane) - 1ull))] = p;
        out += (uint32_t)__popcll(m);
    }
    wave_order();
    return out;
}

// everything the reference does between the first and the last start of one component
__device__ inline void trace_component(const FollowArgs &a, int root, uint32_t lane) {
    const uint32_t base = a.cnt[root], size = a.cnt[root + 1] - base;
    const int cmin = (int)a.cmin[root], cmax = (int)a.cmax[root];
    uint32_t visited = 0, used = 0;
    int start = root;
    const int kr = tracer_drow((int)(lane & 7)), kc = tracer_dcol((int)(lane & 7));
    for (;;) {
        // followPath from `start`
        float2 *pts = a.raw + base + used;
        const uint32_t room = size - used; // >= size - visited >= 1
        int r = start / a.cols, c = start - r * a.cols;
        uint32_t len = 0;
        int prev_k = -1;
        for (;;) {
            if (lane == 0) {
                pts[len] = make_float2((float)c, (float)r);
                a.open[r * a.cols + c] = 0;
            }
            ++len;
            wave_order();
            if (len >= room) break; // the component has no more pixels than its region has places
            const int rr = r + kr, cc = c + kc;
            const bool o = lane < 8 && rr >= 0 && rr < a.rows && cc >= 0 && cc < a.cols && a.open[rr * a.cols + cc] != 0;
            const int k = tracer_choose(prev_k, (uint32_t)__ballot(o));
            if (k < 0) break;
            r += tracer_drow(k);
            c += tracer_dcol(k);
            prev_k = k;
        }
        visited += len;
        if (len >= a.min_len) {
            uint32_t kept = len;
            if (a.simplify && len >= 3) kept = simplify_wave(pts, a.keep + base + used, len, a.eps, lane);
            if (lane == 0) {
                a.poff[start] = base + used;
                a.pcnt[start] = kept;
            }
            used += kept;
        }
        if (visited >= size) return;
        // the raster-next unvisited pixel of this component
        int row = start / a.cols, col = start - row * a.cols + 1;
        int found = -1;
        for (; row < a.rows && found < 0; ++row, col = 0) {
            for (int c0 = col > cmin ? col : cmin; c0 <= cmax; c0 += 64) {
                const int cc = c0 + (int)lane;
                const int q = row * a.cols + cc;
                const bool hit = cc <= cmax && a.open[q] != 0 && a.label[q] == root;
                const unsigned long long m = __ballot(hit);
                if (m) {
                    found = row * a.cols + c0 + first_lane(m);
                    break;
                }
            }
        }
        if (found < 0) return; // cannot be: visited < size
        start = found;
    }
}

__global__ __launch_bounds__(64) void k_trace_follow(FollowArgs a) {
    const uint32_t lane = threadIdx.x;
    for (;;) {
        uint32_t first = 0;
        if (lane == 0) first = atomicAdd(a.queue, FOLLOW_GRAB); // one address for every wave: a grab of 64 indices cost 100 ns and was most of a frame's time
        first = __shfl(first, 0);
        if (first >= (uint32_t)a.n) return;
        for (uint32_t p0 = first; p0 < first + FOLLOW_GRAB && p0 < (uint32_t)a.n; p0 += 64) {
            const int p = (int)(p0 + lane);
            unsigned long long roots = __ballot(p < a.n && a.open[p] != 0 && a.label[p] == p);
            while (roots) {
                const int j = first_lane(roots);
                roots &= roots - 1;
                trace_component(a, (int)p0 + j, lane);
            }
        }
    }
}

// ---- emit --------------------------------------------------------------------------------------------------------------------

__global__ __launch_bounds__(256) void k_trace_flags(const uint32_t *pcnt, int n, uint32_t *path_flag, uint32_t *path_points) {
    const int p = (int)(blockIdx.x * 256u + threadIdx.x);
    if (p > n) return;
    const uint32_t k = p < n ? pcnt[p] : 0u;
    path_flag[p] = k ? 1u : 0u;
    path_points[p] = k;
}

// path_index / point_offset: the exclusive sums of k_trace_flags's two arrays, entry n the totals. A wave takes 64 pixels and copies
// the paths that start there one after another, all lanes on one path.
__global__ __launch_bounds__(256) void k_trace_emit(const uint32_t *pcnt, const uint32_t *poff, const uint32_t *path_index, const uint32_t *point_offset,
                                                    const float2 *raw, int n, float2 *points, uint32_t point_capacity, uint32_t *path_offsets,
                                                    uint32_t path_capacity, uint32_t *counts) {
    const uint32_t lane = threadIdx.x & 63u;
    const int p = (int)(blockIdx.x * 256u + threadIdx.x);
    const uint32_t paths = path_index[n], total = point_offset[n];
    if (p == 0) {
        counts[0] = paths;
        counts[1] = total;
        if (paths <= path_capacity && total <= point_capacity) { // everything fits
            counts[2] = paths;
            counts[3] = total;
            path_offsets[paths] = total;
        }
    }
    const uint32_t k = p < n ? pcnt[p] : 0u;
    uint32_t i = 0, o = 0, src = 0;
    bool fits = false;
    if (k) {
        i = path_index[p];
        o = point_offset[p];
        src = poff[p];
        // the sums only grow, so the paths that fit are a prefix of the list
        fits = i < path_capacity && o + k <= point_capacity && o + k >= o;
        if (fits) {
            path_offsets[i] = o;
        } else if (i == 0 || (i - 1 < path_capacity && o <= point_capacity)) { // the first that does not fit: path i - 1 ended at o
            counts[2] = i;
            counts[3] = o;
            path_offsets[i] = o;
        }
    }
    unsigned long long m = __ballot(fits);
    while (m) {
        const int j = __ffsll((long long)m) - 1;
        m &= m - 1;
        const uint32_t kj = __shfl(k, j), oj = __shfl(o, j), sj = __shfl(src, j);
        for (uint32_t t = lane; t < kj; t += 64) points[oj + t] = raw[sj + t];
    }
}

__global__ void k_trace_empty(uint32_t *path_offsets, uint32_t *counts) {
    counts[0] = counts[1] = counts[2] = counts[3] = 0;
    path_offsets[0] = 0;
}

// A lane per written point j (the grid strides over them: their number is a device word): j is the first end of a segment unless it is
// its path's last point. The path of j by bisection over path_offsets (strictly increasing: every path has a point); the paths before
// it each have one segment fewer than points.
__global__ __launch_bounds__(256) void k_trace_build(const float2 *points, const uint32_t *path_offsets, const uint32_t *counts, uint32_t capacity, uint32_t color,
                                                     uint32_t width, int mode, zg_draw_cmd *out, uint32_t *count_out) {
    const uint32_t paths = counts[2], total = counts[3];
    if (blockIdx.x == 0 && threadIdx.x == 0) *count_out = min(total - paths, capacity);
    for (uint64_t j64 = blockIdx.x * 256u + threadIdx.x; j64 < total; j64 += (uint64_t)gridDim.x * 256u) {
        const uint32_t j = (uint32_t)j64;
        uint32_t lo = 0, hi = paths; // path_offsets[lo] <= j < path_offsets[hi]
        while (hi - lo > 1) {
            const uint32_t mid = lo + (hi - lo) / 2;
            if (path_offsets[mid] <= j) lo = mid; else hi = mid;
        }
        if (j + 1 >= path_offsets[lo + 1]) continue;
        const uint32_t at = j - lo;
        if (at >= capacity) continue;
        zg_draw_cmd c;
        c.kind = ZG_DRAW_LINE;
        c.mode = mode;
        c.width = width;
        c.color[0] = (uint8_t)color; c.color[1] = (uint8_t)(color >> 8); c.color[2] = (uint8_t)(color >> 16); c.color[3] = (uint8_t)(color >> 24);
        c.p[0] = points[j].x; c.p[1] = points[j].y; c.p[2] = points[j + 1].x; c.p[3] = points[j + 1].y;
        c.first_vertex = 0;
        c.n_vertices = 0;
        out[at] = c;
    }
}

// ---- host ----------------------------------------------------------------------------------------------------------------------

bool have_device() { // asked once per process
    static const bool ok = [] {
        int n = 0;
        const bool r = hipGetDeviceCount(&n) == hipSuccess && n > 0;
        if (!r) (void)hipGetLastError();
        return r;
    }();
    return ok;
}

const zg_tracer_options DEFAULTS{5u, 1.0f};

int check(const zg_image *edges, const uint32_t *path_offsets, const uint32_t *counts, const float *points, uint32_t point_capacity, uint32_t path_capacity,
          bool device) {
    int rc;
    if ((rc = check_image(edges, "trace_paths", device))) return rc;
    ZG_REQUIRE(edges->pixel == ZG_PIXEL_U8, ZG_ERR_UNSUPPORTED, "trace_paths: pixel type %d (Image(u8) only)", edges->pixel);
    ZG_REQUIRE((uint64_t)edges->rows * edges->cols < (1ull << 31), ZG_ERR_UNSUPPORTED, "trace_paths: %u x %u pixels, 2^31 or more", edges->rows, edges->cols);
    ZG_REQUIRE(counts != nullptr, ZG_ERR_INVALID_ARGUMENT, "trace_paths: null counts");
    ZG_REQUIRE(points != nullptr || point_capacity == 0, ZG_ERR_INVALID_ARGUMENT, "trace_paths: null points");
    ZG_REQUIRE(path_offsets != nullptr || (!device && path_capacity == 0), ZG_ERR_INVALID_ARGUMENT, "trace_paths: null path_offsets");
    ZG_REQUIRE(path_capacity < 0xffffffffu, ZG_ERR_INVALID_ARGUMENT, "trace_paths: path_capacity %u", path_capacity);
    ZG_REQUIRE(have_device(), ZG_ERR_HIP, "trace_paths: no device");
    return ZG_OK;
}

int trace(const zg_image *edges, const zg_tracer_options *opt, float *points, uint32_t point_capacity, uint32_t *path_offsets, uint32_t path_capacity,
          uint32_t *counts, hipStream_t s) {
    const size_t n = (size_t)edges->rows * edges->cols;
    int rc;
    if (n == 0) {
        k_trace_empty<<<1, 1, 0, s>>>(path_offsets, counts);
        return launch_ok("k_trace_empty");
    }
    ScratchBlock sc(s);
    TraceBuf b{};
    plan(sc, b, n);
    if ((rc = sc.alloc())) return rc;
    const int rows = (int)edges->rows, cols = (int)edges->cols;
    const unsigned pixel_blocks = (unsigned)((n + 255) / 256), pixel_blocks1 = (unsigned)((n + 1 + 255) / 256);
    if ((rc = fill_async(b.cnt, 0, (size_t)((char *)b.cmin - (char *)b.cnt), s))) return rc;
    if ((rc = fill_async(b.cmin, 0xff, n * sizeof(uint32_t), s))) return rc;
    k_trace_links<<<pixel_blocks, 256, 0, s>>>((const uint8_t *)edges->data, (uint64_t)edges->stride, rows, cols, b.links, b.open);
    if ((rc = launch_ok("k_trace_links"))) return rc;
    if ((rc = flood_label_components(b.links, b.label, edges->rows, edges->cols, s))) return rc;
    k_trace_count<<<pixel_blocks, 256, 0, s>>>(b.label, b.open, (int)n, cols, b.cnt, b.cmin, b.cmax);
    if ((rc = launch_ok("k_trace_count"))) return rc;
    if ((rc = scan_u32(b.cnt, n + 1, b.tmp, s))) return rc;
    FollowArgs a{};
    a.rows = rows; a.cols = cols; a.n = (int)n;
    a.min_len = opt->min_path_length;
    a.eps = opt->simplification_epsilon;
    a.simplify = opt->simplification_epsilon > 0.0f; // false for a NaN
    a.label = b.label; a.open = b.open; a.keep = b.keep;
    a.cnt = b.cnt; a.cmin = b.cmin; a.cmax = b.cmax;
    a.poff = b.poff; a.pcnt = b.pcnt; a.queue = b.queue;
    a.raw = b.raw;
    const size_t chunks = (n + FOLLOW_GRAB - 1) / FOLLOW_GRAB;
    k_trace_follow<<<(unsigned)(chunks < FOLLOW_MAX_WAVES ? chunks : FOLLOW_MAX_WAVES), 64, 0, s>>>(a);
    if ((rc = launch_ok("k_trace_follow"))) return rc;
    // the labels and the region offsets have done their work: their arrays take the two sums over the paths
    uint32_t *path_index = (uint32_t *)b.label, *point_offset = b.cnt;
    k_trace_flags<<<pixel_blocks1, 256, 0, s>>>(b.pcnt, (int)n, path_index, point_offset);
    if ((rc = launch_ok("k_trace_flags"))) return rc;
    if ((rc = scan_u32(path_index, n + 1, b.tmp, s))) return rc;
    if ((rc = scan_u32(point_offset, n + 1, b.tmp, s))) return rc;
    k_trace_emit<<<pixel_blocks, 256, 0, s>>>(b.pcnt, b.poff, path_index, point_offset, b.raw, (int)n, (float2 *)points, point_capacity, path_offsets,
                                             path_capacity, counts);
    return launch_ok("k_trace_emit");
}

} // namespace
} // namespace zg

using namespace zg;

extern "C" {

size_t zg_trace_scratch_bytes(uint32_t rows, uint32_t cols) {
    const size_t n = (size_t)rows * cols;
    if (n == 0 || n >= ((size_t)1 << 31)) return 0;
    // the sum of plan()'s parts, each rounded up to 256 bytes
    const size_t parts[] = {(n + 1) * 4, n * 4, n * 4, 64 * 4, n * 4, n, n, n, (n + 1) * 4, n * 4, n * 8, scan_tmp_words(n + 1) * 4};
    size_t bytes = 0;
    for (size_t p : parts) bytes += align256(p);
    return bytes;
}

int zg_trace_paths(const zg_image *edges, const zg_tracer_options *opt, float *points, uint32_t point_capacity, uint32_t *path_offsets, uint32_t path_capacity,
                   uint32_t *counts, zg_stream stream) {
    if (!opt) opt = &DEFAULTS;
    if (const int rc = check(edges, path_offsets, counts, points, point_capacity, path_capacity, true)) return rc;
    return trace(edges, opt, points, point_capacity, path_offsets, path_capacity, counts, as_stream(stream));
}

int zg_trace_paths_host(const zg_image *edges, const zg_tracer_options *opt, float *points, uint32_t point_capacity, uint32_t *path_offsets,
                        uint32_t path_capacity, uint32_t *counts) {
    if (!opt) opt = &DEFAULTS;
    int rc;
    if ((rc = check(edges, path_offsets, counts, points, point_capacity, path_capacity, false))) return rc;
    HostStage st;
    if ((rc = st.upload(edges, true, false))) return rc;
    ScratchBlock sc;
    float *d_points;
    uint32_t *d_offsets, *d_counts;
    sc.take(d_points, 2 * (size_t)point_capacity + 2);
    sc.take(d_offsets, (size_t)path_capacity + 1);
    sc.take(d_counts, 4);
    if ((rc = sc.alloc())) return rc;
    if ((rc = trace(&st.dev, opt, d_points, point_capacity, d_offsets, path_capacity, d_counts, nullptr))) return rc;
    if ((rc = download_pageable(counts, d_counts, 4 * sizeof(uint32_t), nullptr))) return rc; // waits for the stream
    if (path_offsets && (rc = download_pageable(path_offsets, d_offsets, ((size_t)counts[2] + 1) * sizeof(uint32_t), nullptr))) return rc;
    if (counts[3] && (rc = download_pageable(points, d_points, 2 * (size_t)counts[3] * sizeof(float), nullptr))) return rc;
    return ZG_OK;
}

int zg_canvas_cmds_from_paths(const float *points, const uint32_t *path_offsets, const uint32_t *counts, uint32_t capacity, const uint8_t *color, uint32_t width,
                              int mode, zg_draw_cmd *cmds_out, uint32_t *count_out, zg_stream stream) {
    const char *what = "canvas_cmds_from_paths";
    ZG_REQUIRE(counts != nullptr && count_out != nullptr && color != nullptr, ZG_ERR_INVALID_ARGUMENT, "%s: null count, count_out or color", what);
    ZG_REQUIRE(mode == ZG_DRAW_FAST || mode == ZG_DRAW_SOFT, ZG_ERR_INVALID_ARGUMENT, "%s: mode %d", what, mode);
    ZG_REQUIRE(width <= ZG_CANVAS_MAX_WIDTH, ZG_ERR_INVALID_ARGUMENT, "%s: width %u (at most %u)", what, width, ZG_CANVAS_MAX_WIDTH);
    ZG_REQUIRE(path_offsets != nullptr, ZG_ERR_INVALID_ARGUMENT, "%s: null path_offsets", what);
    ZG_REQUIRE(capacity == 0 || (points != nullptr && cmds_out != nullptr), ZG_ERR_INVALID_ARGUMENT, "%s: null points or cmds_out", what);
    uint32_t packed;
    std::memcpy(&packed, color, 4);
    const unsigned blocks = ceil_div(capacity ? capacity : 1u, 128); // two points a segment, when every path has several
    k_trace_build<<<blocks < 4096u ? blocks : 4096u, 256, 0, as_stream(stream)>>>((const float2 *)points, path_offsets, counts, capacity, packed, width, mode, cmds_out,
                                                                                  count_out);
    return launch_ok("k_trace_build");
}

} // extern "C"
