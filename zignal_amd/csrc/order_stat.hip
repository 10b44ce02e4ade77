// order_stat.hip — Image(T).medianBlur / percentileBlur / minBlur / maxBlur / midpointBlur / alphaTrimmedMeanBlur for u8 and
// all-u8 struct pixels (reference src/image.zig:653-783 -> src/image/order_statistic_blur.zig, stats.percentile at
// src/image/histogram.zig:586-610).
//
// Every result is a function of the multiset of the (2r+1)^2 window samples (out-of-image samples through
// border.resolveIndex, a dropped one counting as 0), so the reference's sliding histograms are an implementation detail.
// Here a workgroup stages its 64 x 4 tile plus the radius in LDS (border resolved once per staged pixel) and each lane
// evaluates its window directly: the k-th smallest sample by an 8-step bisection on the VALUE (count of samples <= mid),
// min / max for the midpoint, and for the alpha-trimmed mean the two trim boundaries by bisection plus one pass of sums.
// Cost ~ 8 (2r+1)^2 byte reads per channel: right for the radii these filters are used with (median 3x3 .. 7x7); the
// window area and the rank / trim counts are constants of the call, computed on the host in f64 as the reference does.
// That kernel, k_order_stat, takes radius 1..15. Radius 16..256 takes k_order_stat_hist below: a sliding histogram per lane, work linear in r.
#include "zg_internal.h"
#include "zg_order_stat_track.h"

#include <cmath>
#include <cstdlib>

namespace zg {

constexpr int OS_MAXR = 15;        // k_order_stat: largest radius
constexpr int OS_HIST_MAXR = 256;  // k_order_stat_hist: largest radius (the reference CLI's bound, src/cli/blur.zig:121-127)
constexpr int OS_HIST_U16_MAXR = 127; // (2r+1)^2 <= 65 025 fits a u16 counter
enum : int { OS_PERCENTILE = 0, OS_MIDPOINT = 1, OS_ALPHA_TRIMMED = 2 };

template <int PIX>
__global__ __launch_bounds__(256) void k_order_stat(DImg src, DImg dst, int radius, int border, int op, int rank, int trim_each, int tiles_x) {
    using P = Px<PIX>;
    constexpr int C = P::C;
    extern __shared__ uint8_t tile[]; // [C][lh][lw], lw = 64 + 2r, lh = 4 + 2r
    const int lw = 64 + 2 * radius, lh = 4 + 2 * radius;
    const int ty = blockIdx.x / tiles_x, tx = blockIdx.x - ty * tiles_x;
    const int x0 = tx * 64, y0 = ty * 4;
    for (int i = threadIdx.x; i < lh * lw; i += 256) {
        const int tr = i / lw, tc = i - tr * lw;
        const int gr = resolve_index(y0 - radius + tr, src.rows, border), gc = resolve_index(x0 - radius + tc, src.cols, border);
        typename P::Vec v = P::load(src.data, (size_t)max(gr, 0) * src.stride + (size_t)max(gc, 0)); // clamped, unpredicated
        if (gr < 0 || gc < 0) v = P::zero(); // dropped sample: value 0
#pragma unroll
        for (int ch = 0; ch < C; ++ch) tile[(ch * lh + tr) * lw + tc] = v[ch];
    }
    __syncthreads();
    const int lx = threadIdx.x & 63, ly = threadIdx.x >> 6;
    const int c = x0 + lx, r = y0 + ly;
    if (c >= dst.cols || r >= dst.rows) return;
    const int w = 2 * radius + 1, area = w * w;
    typename P::Vec out;
#pragma unroll
    for (int ch = 0; ch < C; ++ch) {
        const uint8_t *t = tile + (ch * lh + ly) * lw + lx; // window origin of this lane
        auto count_le = [&](int m) { // samples <= m
            int n = 0;
            for (int j = 0; j < w; ++j)
                for (int i = 0; i < w; ++i) n += t[j * lw + i] <= m ? 1 : 0;
            return n;
        };
        auto kth = [&](int k) { // value of the (k+1)-th smallest sample: smallest v with count(<= v) > k
            int lo = 0, hi = 255;
            while (lo < hi) {
                const int mid = (lo + hi) >> 1;
                if (count_le(mid) > k) hi = mid; else lo = mid + 1;
            }
            return lo;
        };
        int res;
        if (op == OS_PERCENTILE) {
            res = kth(rank);
        } else if (op == OS_MIDPOINT) {
            int mn = 255, mx = 0;
            for (int j = 0; j < w; ++j)
                for (int i = 0; i < w; ++i) { const int v = t[j * lw + i]; mn = min(mn, v); mx = max(mx, v); }
            res = (mn + mx + 1) / 2;
        } else { // alpha-trimmed mean: drop trim_each samples from each end (ties split by count), rounded mean of the rest
            int a = 0, b = 255;
            if (trim_each > 0) { a = kth(trim_each - 1); b = kth(area - trim_each); }
            long long total = 0, sum_lt = 0, sum_gt = 0;
            int cnt_lt = 0, cnt_gt = 0;
            for (int j = 0; j < w; ++j)
                for (int i = 0; i < w; ++i) {
                    const int v = t[j * lw + i];
                    total += v;
                    if (v < a) { sum_lt += v; ++cnt_lt; }
                    if (v > b) { sum_gt += v; ++cnt_gt; }
                }
            long long low = 0, high = 0;
            if (trim_each > 0) { low = sum_lt + (long long)(trim_each - cnt_lt) * a; high = sum_gt + (long long)(trim_each - cnt_gt) * b; }
            const long long kept = area - 2 * trim_each; // >= 1: area is odd and trim_each <= area / 2
            const long long rounded = ((total - low - high) + kept / 2) / kept;
            res = (int)(rounded > 255 ? 255 : rounded);
        }
        out[ch] = (uint8_t)res;
    }
    P::store(dst.data, (size_t)r * dst.stride + (size_t)c, out);
}

// ---- radius 16..256: one sliding histogram per lane ----------------------------------------------------------------------------------
// A workgroup is one wave. Lane l owns output column x0 + l of one channel (blockIdx.y) and walks down a strip of H rows (blockIdx.z),
// keeping the 256-bin histogram of its (2r+1)^2 window in LDS and the result as incremental rank trackers (zg_order_stat_track.h): per
// output row the 2r+1 samples of the row that leaves the window and the 2r+1 of the row that enters are exchanged pair by pair, then the
// trackers settle. That is 2(2r+1) byte reads and 2(2r+1) counter read-modify-writes per pixel and channel, against 8(2r+1)^2 reads of
// k_order_stat. No atomics: a counter belongs to one lane.
//   rows     each step the wave stages the entering and the leaving source row as 64 + 2r bytes in LDS, border resolved once per byte
//            (the column part once per workgroup, kept in registers), a dropped sample being 0. The leaving row is read again from global
//            memory, an L2 hit. The bytes of step t + 1 are loaded into registers before the counter loop of step t and stored to LDS
//            after it, so their latency hides behind the loop: with one wave per SIMD nothing else would hide it.
//   bins     CNT = u16 for r <= 127 (32 KiB a wave, 4 workgroups per CU), u32 for r = 128..256 (64 KiB, 2 per CU). Bin v of lane l is
//            element 64 v + slot(l): for u32 slot = l, for u16 slot = 2 (l & 31) + (l >> 5), so lanes l and l + 32 share a dword. LDS serves
//            4-byte-and-narrower accesses in lane groups 0..31 and 32..63, bank = dword address mod 32 = l & 31 whatever the bin: 64 lanes on
//            64 unrelated bins never conflict. The u16 counters are read and written with 16-bit LDS instructions only (uint16_t lvalues),
//            so the two lanes of a dword never touch each other's half.
//   strips   starting a strip costs 2r+1 add-only row steps, as much as 2r+1 output rows. H is chosen per call (hist_strip_rows):
//            strips of at least 4(2r+1) rows keep the start-up at a fifth of the work or less and are cut no finer than 2048 workgroups
//            (two full rounds of the u16 residency on 256 CUs); where that leaves fewer than 512 workgroups, two per CU, strips shrink
//            down to 2r+1 rows (start-up half of the work) until there are 512 or the frame is used up.
template <typename CNT> struct LaneHist {
    CNT *bins; // this lane's bin 0; consecutive bins are 64 elements apart
    __device__ uint32_t get(int v) const { return bins[v * 64]; }
    __device__ void set(int v, uint32_t c) const { bins[v * 64] = (CNT)c; }
};

template <typename CNT, int OP>
__global__ __launch_bounds__(64) void k_order_stat_hist(const uint8_t *__restrict__ src, size_t sstride, uint8_t *__restrict__ dst, size_t dstride, int rows,
                                                        int cols, int C, int radius, int border, uint32_t rank, uint32_t trim_each, int H) {
    constexpr int MAXR = sizeof(CNT) == 2 ? OS_HIST_U16_MAXR : OS_HIST_MAXR;
    constexpr int LW = 64 + 2 * MAXR;    // bytes of a staged row at the largest radius
    constexpr int NS = (LW + 63) / 64;   // staged bytes per lane
    __shared__ CNT hist[256 * 64];
    __shared__ uint8_t row_in[NS * 64], row_out[NS * 64];
    const int lane = threadIdx.x, ch = blockIdx.y;
    const int x0 = blockIdx.x * 64, y0 = blockIdx.z * H, y1 = min(rows, y0 + H);
    if (y0 >= rows) return;
    const int w = 2 * radius + 1, lw = 64 + 2 * radius;
    const uint32_t area = (uint32_t)w * (uint32_t)w;
    const LaneHist<CNT> h{hist + (sizeof(CNT) == 2 ? 2 * (lane & 31) + (lane >> 5) : lane)};
    for (int v = 0; v < 256; ++v) h.set(v, 0);
    // byte offset of staged column i * 64 + lane within a source row, or -1: dropped by the border, or past the staged width
    long long col_ofs[NS];
#pragma unroll
    for (int i = 0; i < NS; ++i) {
        const int idx = i * 64 + lane;
        const int gc = idx < lw ? resolve_index(x0 - radius + idx, cols, border) : -1;
        col_ofs[i] = gc < 0 ? -1 : (long long)gc * C + ch;
    }
    auto fetch = [&](int y, uint8_t (&px)[NS]) { // source row y (unresolved) into registers
        const int gr = resolve_index(y, rows, border);
        const uint8_t *line = src + (size_t)max(gr, 0) * sstride * (size_t)C;
#pragma unroll
        for (int i = 0; i < NS; ++i) {
            if (i * 64 >= lw) break; // uniform: the staged width at this radius
            const uint8_t v = line[max(col_ofs[i], 0ll)]; // clamped, unpredicated
            px[i] = (gr < 0 || col_ofs[i] < 0) ? (uint8_t)0 : v;
        }
    };
    OsTracker ta, tb; // percentile: ta at rank. midpoint: ta at 0, tb at area - 1. trimmed: ta at trim_each - 1, tb at area - trim_each
    constexpr bool SUM = OP == OS_ALPHA_TRIMMED;
    constexpr bool TWO = OP != OS_PERCENTILE;
    const bool track = OP != OS_ALPHA_TRIMMED || trim_each > 0;
    uint32_t total = 0;
    uint8_t pin[NS], pout[NS];
    const int nsteps = w - 1 + (y1 - y0); // step t brings source row y0 - r + t in; from t = w on, row y0 - r + t - w goes out
#pragma unroll
    for (int i = 0; i < NS; ++i) pin[i] = pout[i] = 0;
    fetch(y0 - radius, pin);
    for (int t = 0; t < nsteps; ++t) {
        __syncthreads(); // the previous step's readers are done
#pragma unroll
        for (int i = 0; i < NS; ++i) {
            if (i * 64 >= lw) break;
            row_in[i * 64 + lane] = pin[i];
            row_out[i * 64 + lane] = pout[i];
        }
        __syncthreads();
        if (t + 1 < nsteps) {
            fetch(y0 - radius + t + 1, pin);
            if (t + 1 >= w) fetch(y0 - radius + t + 1 - w, pout);
        }
        if (t < w) { // filling the first window of the strip
            for (int dx = 0; dx < w; ++dx) {
                const int a = row_in[lane + dx];
                os_hist_add(h, a);
                if (track) { os_add<SUM>(ta, a); if (TWO) os_add<SUM>(tb, a); }
                if (SUM) total += (uint32_t)a;
            }
        } else {
            for (int dx = 0; dx < w; ++dx) {
                const int a = row_in[lane + dx], b = row_out[lane + dx];
                os_hist_replace(h, b, a);
                if (track) {
                    os_add<SUM>(ta, a); os_remove<SUM>(ta, b);
                    if (TWO) { os_add<SUM>(tb, a); os_remove<SUM>(tb, b); }
                }
                if (SUM) total += (uint32_t)a - (uint32_t)b;
            }
        }
        if (t < w - 1) continue;
        int res;
        if (OP == OS_PERCENTILE) {
            os_settle<false>(ta, h, rank);
            res = ta.m;
        } else if (OP == OS_MIDPOINT) {
            os_settle<false>(ta, h, 0u);
            os_settle<false>(tb, h, area - 1u);
            res = os_midpoint(ta.m, tb.m);
        } else {
            if (track) { os_settle<true>(ta, h, trim_each - 1u); os_settle<true>(tb, h, area - trim_each); }
            res = os_trimmed_mean(ta, tb, h, total, area, trim_each);
        }
        const int y = y0 + t - (w - 1);
        if (x0 + lane < cols) dst[((size_t)y * dstride + (size_t)(x0 + lane)) * (size_t)C + ch] = (uint8_t)res;
    }
}

// Rows per strip of k_order_stat_hist for a frame of `rows` rows whose grid has `columns` workgroups per strip (column strips x channels):
// the rule in the kernel's head comment.
static int hist_strip_rows(uint32_t rows, uint32_t radius, uint64_t columns) {
    const uint64_t w = 2ull * radius + 1;
    uint64_t n = std::min<uint64_t>(std::max<uint64_t>(rows / (4 * w), 1), (2048 + columns - 1) / columns);
    if (columns * n < 512) n = std::min<uint64_t>((512 + columns - 1) / columns, std::max<uint64_t>(rows / w, 1));
    return (int)((rows + n - 1) / n);
}

// The smallest radius k_order_stat_hist takes: 16, or ZIGNAL_HIP_ORDER_STAT_HIST_MIN = 1..16 (an A/B hook: the sliding kernel at small radii
// against the oracle, and the crossover's timing; it changes no result). Read once per process.
static uint32_t hist_min_radius() {
    static const uint32_t v = [] {
        const char *e = getenv("ZIGNAL_HIP_ORDER_STAT_HIST_MIN");
        const long n = e ? strtol(e, nullptr, 10) : 0;
        return (uint32_t)(n >= 1 && n <= OS_MAXR + 1 ? n : OS_MAXR + 1);
    }();
    return v;
}

template <typename CNT>
static int launch_hist(const zg_image *in, const zg_image *dst, uint32_t radius, int op, int border, uint32_t rank, uint32_t trim_each, hipStream_t s) {
    const int C = pixel_channels(in->pixel);
    const unsigned strips_x = ceil_div(in->cols, 64);
    const int H = hist_strip_rows(in->rows, radius, (uint64_t)strips_x * (unsigned)C);
    const dim3 grid(strips_x, (unsigned)C, ceil_div(in->rows, (unsigned)H));
    const uint8_t *sp = (const uint8_t *)in->data;
    uint8_t *dp = (uint8_t *)dst->data;
#define ZG_OS_HIST(OP) \
    hipLaunchKernelGGL((k_order_stat_hist<CNT, OP>), grid, dim3(64), 0, s, sp, in->stride, dp, dst->stride, (int)in->rows, (int)in->cols, C, (int)radius, border, \
                       rank, trim_each, H)
    if (op == OS_PERCENTILE) ZG_OS_HIST(OS_PERCENTILE);
    else if (op == OS_MIDPOINT) ZG_OS_HIST(OS_MIDPOINT);
    else ZG_OS_HIST(OS_ALPHA_TRIMMED);
#undef ZG_OS_HIST
    return launch_ok("k_order_stat_hist");
}

static int order_stat_impl(const zg_image *src, const zg_image *dst, uint32_t radius, int op, double param, int border, hipStream_t s) {
    int rc;
    if ((rc = check_image(src, "src")) || (rc = check_image(dst, "dst"))) return rc;
    ZG_REQUIRE(src->rows == dst->rows && src->cols == dst->cols, ZG_ERR_DIMENSION_MISMATCH, "order-statistic blur: %ux%u vs %ux%u", src->rows, src->cols,
               dst->rows, dst->cols);
    ZG_REQUIRE(src->pixel == dst->pixel, ZG_ERR_INVALID_ARGUMENT, "order-statistic blur: pixel types differ");
    ZG_REQUIRE(!pixel_is_float(src->pixel), ZG_ERR_UNSUPPORTED, "order-statistic blur: UnsupportedPixelType (u8 and all-u8 structs only)");
    ZG_REQUIRE(border >= ZG_BORDER_ZERO && border <= ZG_BORDER_WRAP, ZG_ERR_INVALID_ARGUMENT, "invalid border %d", border);
    if (src->rows == 0 || src->cols == 0) return ZG_OK;
    if (op == OS_ALPHA_TRIMMED) ZG_REQUIRE(std::isfinite(param) && param >= 0.0 && param < 0.5, ZG_ERR_INVALID_ARGUMENT, "alphaTrimmedMeanBlur: InvalidTrim (%g)", param);
    if (radius == 0) return copy_impl(src, dst, s);
    if (op == OS_PERCENTILE) ZG_REQUIRE(param >= 0.0 && param <= 1.0, ZG_ERR_INVALID_ARGUMENT, "percentileBlur: InvalidPercentile (%g)", param);
    ZG_REQUIRE(radius <= (uint32_t)OS_HIST_MAXR, ZG_ERR_UNSUPPORTED, "order-statistic blur: radius %u (up to %d supported)", radius, OS_HIST_MAXR);
    const long long area = (long long)(2 * radius + 1) * (2 * radius + 1);
    int rank = 0, trim_each = 0;
    if (op == OS_PERCENTILE) { // stats.percentile, histogram.zig:595-599 (total = area: every window sample counts)
        const double rank_floor = std::floor(param * (double)(area - 1) + 1e-12);
        long long rk = (long long)std::trunc(rank_floor);
        rank = (int)std::min<long long>(std::max<long long>(rk, 0), area - 1);
    } else if (op == OS_ALPHA_TRIMMED) { // order_statistic_blur.zig:331-334
        const long long trimmed_each = (long long)std::trunc(std::floor(param * (double)area));
        trim_each = (int)std::min<long long>(trimmed_each, area / 2);
    }
    // in place, or a destination view that shares bytes with the source: other workgroups would read pixels this one has already replaced
    const zg_image *in = src;
    zg_image copy{};
    ScratchBlock scratch(s);
    const size_t ps = pixel_size(src->pixel);
    if (spans_overlap(src, dst)) {
        if ((rc = scratch.alloc((size_t)src->rows * src->cols * ps))) return rc;
        copy = zg_image{scratch.p, src->cols, src->rows, src->cols, src->pixel};
        if ((rc = copy_impl(src, &copy, s))) return rc;
        in = &copy;
    }
    if (radius >= hist_min_radius())
        return radius <= (uint32_t)OS_HIST_U16_MAXR ? launch_hist<uint16_t>(in, dst, radius, op, border, (uint32_t)rank, (uint32_t)trim_each, s)
                                                    : launch_hist<uint32_t>(in, dst, radius, op, border, (uint32_t)rank, (uint32_t)trim_each, s);
    const int tiles_x = (int)ceil_div(src->cols, 64), tiles_y = (int)ceil_div(src->rows, 4);
    const size_t lds = (size_t)pixel_channels(src->pixel) * (4 + 2 * radius) * (64 + 2 * radius);
    return dispatch_pixel(src->pixel, [&](auto tag) -> int {
        constexpr int PIX = decltype(tag)::value;
        if constexpr (!std::is_same<typename Px<PIX>::Elem, float>::value) {
            hipLaunchKernelGGL((k_order_stat<PIX>), dim3((unsigned)(tiles_x * tiles_y)), dim3(256), lds, s, dimg(in), dimg(dst), (int)radius, border, op, rank,
                               trim_each, tiles_x);
            if (const int e = launch_ok()) return e;
        }
        return ZG_OK;
    });
}

} // namespace zg

using namespace zg;

extern "C" {

int zg_order_statistic_blur(const zg_image *src, const zg_image *dst, uint32_t radius, int op, double param, int border, zg_stream stream) {
    ZG_REQUIRE(op >= OS_PERCENTILE && op <= OS_ALPHA_TRIMMED, ZG_ERR_INVALID_ARGUMENT, "order-statistic blur: op %d", op);
    return order_stat_impl(src, dst, radius, op, param, border, as_stream(stream));
}
int zg_order_statistic_blur_host(const zg_image *src, const zg_image *dst, uint32_t radius, int op, double param, int border) {
    ZG_REQUIRE(op >= OS_PERCENTILE && op <= OS_ALPHA_TRIMMED, ZG_ERR_INVALID_ARGUMENT, "order-statistic blur: op %d", op);
    return host_src_dst(src, dst, [&](const zg_image *a, const zg_image *b) { return order_stat_impl(a, b, radius, op, param, border, nullptr); });
}

} // extern "C"
