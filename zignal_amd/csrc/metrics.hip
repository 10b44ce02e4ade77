// metrics.hip — Image(T).psnr, ssim and meanPixelError (reference src/image/metrics.zig:10-166) on the device, bit for bit.
//
// Each of the three ends in a left-to-right f64 sum over every term (mse += diff * diff, :26,32; total_abs += diff, :131,140; ssim_sum
// += numerator / denominator, :106), which no reordered sum reproduces. On u8 fields every term is an integer and every partial sum is
// below 2^53, so the f64 sum IS the integer sum: k_int_terms adds integers in any order. Everywhere else the sum goes through
// sum_terms(), a speculative parallel form of the sequential sum that proves itself chunk by chunk:
//
//   While the running sum s stays strictly inside one binade [2^e, 2^(e+1)), g = 2^(e-52) its unit in the last place, s / g is an
//   integer S in (2^52, 2^53) and RN(s + v) = g * (S + q), q = v / g rounded to the nearest integer (v / g is exact: g is a power of
//   two). q depends on S only at an exact tie, v / g = k + 1/2: round-to-even takes k when S + k is even and k + 1 when it is odd, and
//   the sum is even afterwards. A run of terms is therefore a two-state transducer over the parity of S, transducers compose
//   associatively, and a chunk is summed up by a reduction (zg_scan.h: block_reduce_ordered) into, for each entering parity, the total
//   of its q and the smallest and largest prefix of that total.
//     k_chunk_sums     an approximate f64 sum per chunk (any parallel order), and whether every term of the chunk is a zero
//     k_chunk_guess    the approximate sum of all chunks before each chunk: the binade the true sum is guessed to enter the chunk in
//     k_chunk_records  the transducer of each chunk for its guessed binade
//     k_walk           one wave walks the chunks in order with the true s. A record is applied (s += g * total, exact, in integers) only
//                      if s is positive and in the guessed binade, S + min > 2^52 and S + max < 2^53 (every intermediate sum stayed
//                      strictly inside the binade; the empty prefix counts, so S = 2^52 itself never qualifies) and no term was too
//                      large for the integers used. A chunk of zeros leaves s alone whatever s is (s is never -0.0: it starts at +0.0,
//                      and x + y is -0.0 only for two negative zeros). Every other chunk is added term by term, in order, the wave
//                      fetching 64 terms at a time and adding them out of its lanes' registers.
//   By induction from s = +0.0 the result is the sequential sum for every input; speculation decides only how many terms are added
//   serially (counted in zg_metric_result.serial_terms).
#include "zg_common.h"
#include "zg_hostmath.h"
#include "zg_scan.h"

#include "../../include/zignal_hip_metrics.h"

#include <cmath>
#include <cstring>

#pragma clang fp contract(off)

namespace zg {
namespace {

constexpr uint32_t CHUNK_LOG2 = 12, CHUNK_LOG2_MIN = 6, CHUNK_LOG2_MAX = 16;
constexpr uint64_t MANT = (1ull << 52) - 1, ONE52 = 1ull << 52, ONE53 = 1ull << 53;
constexpr int E_MIN = 1, E_MAX = 2046; // the biased exponents a guess may have: every normal f64

enum { MODE_SUM = 0, MODE_MEAN = 1, MODE_MEAN_OVER_MAX = 2 };

__device__ inline uint64_t bits_of(double d) { return (uint64_t)__double_as_longlong(d); }
__device__ inline double double_of(uint64_t u) { return __longlong_as_double((long long)u); }

// ---- term generators: at(i) is a cursor on term i whose next() returns terms i, i + 1, ... ----------------------------------------

struct ArrayTerms {
    static constexpr bool ANY_ORDER_IS_CHEAP = true; // at(i) is an addition: a pass that may take the terms in any order strides over them
    const double *v;
    struct Cursor {
        const double *p;
        __device__ double next() { return *p++; }
    };
    __device__ Cursor at(uint64_t i) const { return Cursor{v + i}; }
};

// d = f64(a) - f64(b), then d * d (psnr, :25-26,31-32) or |d| (meanPixelError, :130-131,136-140), row-major, a pixel's fields in order:
// a row is cols * channels consecutive floats, and the floats between two rows are never read
template <bool SQ> struct ImageTerms {
    static constexpr bool ANY_ORDER_IS_CHEAP = false; // at(i) divides by the row length
    const float *a, *b;
    uint64_t stride_a, stride_b; // floats from one row to the next
    uint32_t row_len;            // cols * channels
    struct Cursor {
        const float *pa, *pb;
        uint64_t gap_a, gap_b;
        uint32_t left, row_len;
        __device__ double next() {
            const double d = (double)*pa - (double)*pb;
            ++pa;
            ++pb;
            if (--left == 0) {
                pa += gap_a;
                pb += gap_b;
                left = row_len;
            }
            return SQ ? d * d : fabs(d);
        }
    };
    __device__ Cursor at(uint64_t i) const {
        const uint64_t r = i / row_len;
        const uint32_t x = (uint32_t)(i - r * row_len);
        return Cursor{a + r * stride_a + x, b + r * stride_b + x, stride_a - row_len, stride_b - row_len, row_len - x, row_len};
    }
};

// ---- the sequential sum ------------------------------------------------------------------------------------------------------------

// a chunk's transducer: for the parity p of S on entry, the total of the q and the extremes of its prefixes (the empty one included)
struct Transducer {
    long long total[2], lo[2], hi[2];
    int bad, pad;
};
struct Compose { // a, then b
    __device__ Transducer operator()(const Transducer &a, const Transducer &b) const {
        Transducer r;
#pragma unroll
        for (int p = 0; p < 2; ++p) {
            const bool odd = ((p + a.total[p]) & 1) != 0; // the parity b is entered in; selects, not indices: the arrays stay in registers
            r.total[p] = odd ? a.total[p] + b.total[1] : a.total[p] + b.total[0];
            r.lo[p] = min(a.lo[p], odd ? a.total[p] + b.lo[1] : a.total[p] + b.lo[0]);
            r.hi[p] = max(a.hi[p], odd ? a.total[p] + b.hi[1] : a.total[p] + b.hi[0]);
        }
        r.bad = a.bad | b.bad;
        r.pad = 0;
        return r;
    }
};
struct ApproxSum {
    double sum;
    int nonzero, pad;
};
struct AddApprox {
    __device__ ApproxSum operator()(const ApproxSum &a, const ApproxSum &b) const { return ApproxSum{a.sum + b.sum, a.nonzero | b.nonzero, 0}; }
};

constexpr uint32_t REC_USABLE = 1, REC_ZERO = 2;
struct ChunkRecord { // 64 bytes
    long long total[2], lo[2], hi[2];
    int exponent; // the guessed biased exponent
    uint32_t flags;
    uint64_t pad;
};

struct SumArgs {
    uint64_t n;
    uint32_t chunk_log2;
    uint64_t n_chunks;
    double *chunk_sum;
    int *chunk_guess; // the biased exponent, 0: no guess; on the way in from k_chunk_sums, -1: a chunk of zeros
    ChunkRecord *records;
    // how the walker finishes: zg_metric_result's count and value
    int mode;
    uint64_t count;
    double max_value;
    zg_metric_result *result;
};

// thread t of a chunk's workgroup owns the terms [first, first + mine) of the whole sequence: consecutive ones, so that thread order is
// term order
__device__ inline void my_terms(const SumArgs &a, uint64_t &first, uint32_t &mine) {
    const uint32_t len = 1u << a.chunk_log2, per = len >= 256u ? len >> 8 : 1u;
    const uint32_t at = threadIdx.x * per;
    first = ((uint64_t)blockIdx.x << a.chunk_log2) + at;
    mine = (at < len && first < a.n) ? (uint32_t)min((uint64_t)per, a.n - first) : 0u;
}

template <typename Gen> __global__ __launch_bounds__(256) void k_chunk_sums(Gen gen, SumArgs a) {
    ApproxSum acc{0.0, 0, 0};
    auto take = [&](double v) {
        acc.sum += v;
        acc.nonzero |= (bits_of(v) << 1) != 0; // anything but +0.0 and -0.0, NaN included
    };
    if constexpr (Gen::ANY_ORDER_IS_CHEAP) { // neighbouring threads read neighbouring terms
        const uint64_t base = (uint64_t)blockIdx.x << a.chunk_log2, cnt = min(1ull << a.chunk_log2, a.n - base);
        for (uint64_t j = threadIdx.x; j < cnt; j += 256) take(gen.at(base + j).next());
    } else {
        uint64_t first;
        uint32_t mine;
        my_terms(a, first, mine);
        if (mine) {
            auto cur = gen.at(first);
            for (uint32_t i = 0; i < mine; ++i) take(cur.next());
        }
    }
    acc = block_reduce_ordered(acc, AddApprox{});
    if (threadIdx.x == 0) {
        a.chunk_sum[blockIdx.x] = acc.sum;
        a.chunk_guess[blockIdx.x] = acc.nonzero ? 0 : -1;
    }
}

// one workgroup: thread t owns the chunks [t * m, (t + 1) * m)
__global__ __launch_bounds__(256) void k_chunk_guess(SumArgs a) {
    const uint64_t m = (a.n_chunks + 255) / 256;
    const uint64_t c0 = min(a.n_chunks, threadIdx.x * m), c1 = min(a.n_chunks, c0 + m);
    double mine = 0.0;
    for (uint64_t c = c0; c < c1; ++c) mine += a.chunk_sum[c];
    double all;
    double before = block_exclusive_sum64(mine, &all);
    for (uint64_t c = c0; c < c1; ++c) {
        const uint64_t u = bits_of(before);
        const int e = (int)(u >> 52); // sign included: a negative prefix is out of range
        if (a.chunk_guess[c] == 0 && e >= E_MIN && e <= E_MAX) a.chunk_guess[c] = e;
        before += a.chunk_sum[c];
    }
}

template <typename Gen> __global__ __launch_bounds__(256) void k_chunk_records(Gen gen, SumArgs a) {
    const int e = a.chunk_guess[blockIdx.x];
    if (e <= 0) { // uniform: nothing to speculate on
        if (threadIdx.x == 0) {
            a.records[blockIdx.x].exponent = 0;
            a.records[blockIdx.x].flags = e < 0 ? REC_ZERO : 0; // the walker reads nothing else of such a record
        }
        return;
    }
    const int shift = 1075 - e; // v / g = v * 2^(52 - (e - 1023))
    // |q| stays below 2^52 (so q is exact) and a chunk's totals and prefixes below 2^62: a term past that has left the binade anyway
    const double limit = double_of((uint64_t)(1023 + min(52u, 62u - a.chunk_log2)) << 52);
    uint64_t first;
    uint32_t mine;
    my_terms(a, first, mine);
    Transducer t{};
    if (mine) {
        auto cur = gen.at(first);
        for (uint32_t i = 0; i < mine; ++i) {
            const double x = ldexp(cur.next(), shift); // exact, or too small to matter (or infinite: past the limit)
            if (!(fabs(x) < limit)) { // NaN and infinities too
                t.bad = 1;
                continue;
            }
            const double r = rint(x);
            const bool tie = fabs(x - r) == 0.5;
            const long long k = (long long)floor(x), nearest = (long long)r;
#pragma unroll
            for (int p = 0; p < 2; ++p) {
                const long long parity = (p + t.total[p]) & 1;
                t.total[p] += tie ? k + (parity ^ (k & 1)) : nearest;
                t.lo[p] = min(t.lo[p], t.total[p]);
                t.hi[p] = max(t.hi[p], t.total[p]);
            }
        }
    }
    t = block_reduce_ordered(t, Compose{});
    if (threadIdx.x == 0) {
        ChunkRecord *r = a.records + blockIdx.x;
#pragma unroll
        for (int p = 0; p < 2; ++p) {
            r->total[p] = t.total[p];
            r->lo[p] = t.lo[p];
            r->hi[p] = t.hi[p];
        }
        r->exponent = e;
        r->flags = t.bad ? 0 : REC_USABLE;
    }
}

// a value every lane of the wave holds, as the compiler may keep it in scalar registers
__device__ inline double wave_uniform(double d) {
    const uint64_t u = bits_of(d);
    const uint32_t lo = (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)u), hi = (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)(u >> 32));
    return double_of((uint64_t)hi << 32 | lo);
}
template <int LANE> __device__ inline double lane_value(double d) {
    const uint64_t u = bits_of(d);
    const uint32_t lo = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)u, LANE), hi = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)(u >> 32), LANE);
    return double_of((uint64_t)hi << 32 | lo);
}
template <int LANE> __device__ inline double add_lanes(double s, double v) {
    if constexpr (LANE < 64) return add_lanes<LANE + 1>(s + lane_value<LANE>(v), v);
    else return s;
}

__device__ inline void finish(const SumArgs &a, double sum, uint64_t serial) {
    zg_metric_result r;
    r.sum = sum;
    r.count = a.count;
    const double mean = sum / (double)a.count; // mse /= component_count (:48); ssim_sum / weight_sum (:111), weight_sum a sum of 1.0s
    r.value = a.mode == MODE_SUM ? sum : a.mode == MODE_MEAN ? mean : (a.count == 0 ? 0.0 : mean / a.max_value); // :159-165
    r.serial_terms = serial;
    *a.result = r;
}

// One wave. Everything it branches on is the same in all 64 lanes. A batch of 64 records is staged in LDS; the record after the one
// being decided is already on its way into registers (its address does not depend on s), and so are the next 256 terms of a chunk
// that is being added serially.
constexpr int WALK_STEP = 4; // 64-term groups fetched together
template <typename Gen> __global__ __launch_bounds__(64) void k_walk(Gen gen, SumArgs a) {
    __shared__ ChunkRecord recs[65];
    const uint32_t lane = threadIdx.x;
    const uint64_t len = 1ull << a.chunk_log2;
    double s = 0.0;
    uint64_t serial = 0;
    for (uint64_t c0 = 0; c0 < a.n_chunks; c0 += 64) {
        __syncthreads();
        if (c0 + lane < a.n_chunks) recs[lane] = a.records[c0 + lane];
        __syncthreads();
        const uint32_t batch = (uint32_t)min((uint64_t)64, a.n_chunks - c0);
        ChunkRecord cur = recs[0];
        for (uint32_t k = 0; k < batch; ++k) {
            const ChunkRecord rec = cur;
            cur = recs[k + 1]; // recs[64] is never used
            if (rec.flags & REC_ZERO) continue;
            const uint64_t u = bits_of(s);
            if ((rec.flags & REC_USABLE) && (int)(u >> 52) == rec.exponent) { // the sign bit is part of the comparison: s is positive
                const long long S = (long long)((u & MANT) | ONE52);
                const bool odd = (S & 1) != 0;
                const long long lo = odd ? rec.lo[1] : rec.lo[0], hi = odd ? rec.hi[1] : rec.hi[0], total = odd ? rec.total[1] : rec.total[0];
                if (S + lo > (long long)ONE52 && S + hi < (long long)ONE53) {
                    const uint64_t S1 = (uint64_t)(S + total); // in (2^52, 2^53): the same exponent
                    s = wave_uniform(double_of((u & ~MANT) | (S1 & MANT)));
                    continue;
                }
            }
            const uint64_t base = (c0 + k) << a.chunk_log2;
            const uint64_t cnt = min(len, a.n - base);
            // past the end of the chunk: -0.0, and s + -0.0 is s for every s
            auto fetch = [&](uint64_t j, double (&v)[WALK_STEP]) {
#pragma unroll
                for (int w = 0; w < WALK_STEP; ++w) {
                    const uint64_t i = j + (uint64_t)w * 64 + lane;
                    v[w] = i < cnt ? gen.at(base + i).next() : -0.0;
                }
            };
            double v[WALK_STEP];
            fetch(0, v);
            for (uint64_t j = 0; j < cnt; j += 64 * WALK_STEP) {
                double next[WALK_STEP];
                fetch(j + 64 * WALK_STEP, next);
#pragma unroll
                for (int w = 0; w < WALK_STEP; ++w) {
                    if (j + (uint64_t)w * 64 < cnt) s = wave_uniform(add_lanes<0>(s, v[w])); // uniform
                    v[w] = next[w];
                }
            }
            serial += cnt;
        }
    }
    if (lane == 0) finish(a, s, serial);
}

template <typename Gen> int sum_terms(const Gen &gen, uint64_t n, uint32_t chunk_log2, int mode, uint64_t count, double max_value, zg_metric_result *result,
                                      hipStream_t s) {
    SumArgs a{};
    a.n = n;
    a.chunk_log2 = chunk_log2 ? chunk_log2 : CHUNK_LOG2;
    a.n_chunks = (n + (1ull << a.chunk_log2) - 1) >> a.chunk_log2;
    a.mode = mode;
    a.count = count;
    a.max_value = max_value;
    a.result = result;
    ZG_REQUIRE(a.n_chunks < (1ull << 31), ZG_ERR_UNSUPPORTED, "sequential sum: %llu chunks, 2^31 or more", (unsigned long long)a.n_chunks);
    ScratchBlock sc(s); // [approximate sums][guesses][records]
    if (a.n_chunks) {
        sc.take(a.chunk_sum, a.n_chunks);
        sc.take(a.chunk_guess, a.n_chunks);
        sc.take(a.records, a.n_chunks);
        if (const int rc = sc.alloc()) return rc;
        int rc;
        hipLaunchKernelGGL(k_chunk_sums<Gen>, dim3((unsigned)a.n_chunks), dim3(256), 0, s, gen, a);
        if ((rc = launch_ok("k_chunk_sums"))) return rc;
        hipLaunchKernelGGL(k_chunk_guess, dim3(1), dim3(256), 0, s, a);
        if ((rc = launch_ok("k_chunk_guess"))) return rc;
        hipLaunchKernelGGL(k_chunk_records<Gen>, dim3((unsigned)a.n_chunks), dim3(256), 0, s, gen, a);
        if ((rc = launch_ok("k_chunk_records"))) return rc;
    }
    hipLaunchKernelGGL(k_walk<Gen>, dim3(1), dim3(64), 0, s, gen, a);
    return launch_ok("k_walk");
}

// ---- psnr and meanPixelError on u8 fields: integer sums ------------------------------------------------------------------------------

// the four byte pairs of two words
template <bool SQ> __device__ inline uint32_t word_terms(uint32_t a, uint32_t b) {
    uint32_t sum = 0;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int d = (int)((a >> (8 * k)) & 255u) - (int)((b >> (8 * k)) & 255u);
        sum += (uint32_t)(SQ ? d * d : (d < 0 ? -d : d));
    }
    return sum;
}

// A workgroup takes INT_SPAN bytes of one row, a thread 16 of them: as one 16-byte load from each image where both addresses allow and
// the 16 bytes are inside the row, byte by byte otherwise (a row is cols * channels bytes; the bytes up to the pitch are not read).
constexpr uint32_t INT_SPAN = 256 * 16;
template <bool SQ> __global__ __launch_bounds__(256) void k_int_terms(const uint8_t *pa, const uint8_t *pb, uint64_t pitch_a, uint64_t pitch_b, uint32_t row_bytes,
                                                                     uint32_t rows, unsigned long long *acc) {
    const uint32_t r = (uint32_t)grid_row();
    uint64_t sum = 0;
    const uint64_t x = (uint64_t)blockIdx.x * INT_SPAN + threadIdx.x * 16u;
    if (r < rows && x < row_bytes) {
        const uint8_t *ra = pa + (uint64_t)r * pitch_a + x, *rb = pb + (uint64_t)r * pitch_b + x;
        if (x + 16 <= row_bytes && (((uintptr_t)ra | (uintptr_t)rb) & 15) == 0) {
            const uint4 va = *(const uint4 *)ra, vb = *(const uint4 *)rb;
            sum = word_terms<SQ>(va.x, vb.x) + word_terms<SQ>(va.y, vb.y) + word_terms<SQ>(va.z, vb.z) + word_terms<SQ>(va.w, vb.w);
        } else {
            const uint32_t n = (uint32_t)min((uint64_t)16, row_bytes - x);
            for (uint32_t k = 0; k < n; ++k) {
                const int d = (int)ra[k] - (int)rb[k];
                sum += (uint64_t)(SQ ? d * d : (d < 0 ? -d : d));
            }
        }
    }
    sum = block_reduce_ordered(sum, [](uint64_t p, uint64_t q) { return p + q; });
    if (threadIdx.x == 0 && sum) atomicAdd(acc, (unsigned long long)sum);
}

__global__ void k_int_finish(const unsigned long long *acc, SumArgs a) {
    finish(a, (double)*acc, 0); // below 2^53: exact
}

// ---- ssim ------------------------------------------------------------------------------------------------------------------------------

constexpr int WIN = ZG_SSIM_WINDOW, HALO = WIN - 1;
constexpr int ST_W = 64, ST_PER = 4, ST_H = 4 * ST_PER;     // a workgroup's outputs: 64 columns x 16 rows, a lane owning 4 rows of one column
constexpr int ST_LW = ST_W + HALO, ST_LH = ST_H + HALO;       // the staged scalars

struct SsimWindow {
    double w[WIN * WIN];
};
struct SsimArgs {
    const void *a, *b;
    uint64_t stride_a, stride_b; // pixels
    int rows, cols;
    double c1, c2;
    double *out; // (rows - 10) x (cols - 10)
    uint32_t tiles_x;
};

// getPixelScalar (:188-203)
template <int PIX> __device__ inline double pixel_scalar(const void *base, size_t idx) {
    using P = Px<PIX>;
    const typename P::Vec v = P::load(base, idx);
    if constexpr (P::C == 1) {
        return (double)v[0];
    } else if constexpr (std::is_same<typename P::Elem, uint8_t>::value) {
        // rgbLuma(r, g, b) * max_val (:193-194; src/color.zig:1021-1027, luma_r, luma_g, luma_b :64-66); alpha is not looked at
        const double r = (double)v[0] / 255.0, g = (double)v[1] / 255.0, b = (double)v[2] / 255.0;
        return (0.2126 * r + 0.7152 * g + 0.0722 * b) * 255.0;
    } else {
        double sum = 0.0; // :196-202: meta.isRgb is false for f32 fields
#pragma unroll
        for (int i = 0; i < P::C; ++i) sum += (double)v[i];
        return sum / (double)P::C;
    }
}

template <int PIX> __global__ __launch_bounds__(256) void k_ssim(SsimArgs a, SsimWindow win) {
    __shared__ double sx[ST_LH][ST_LW], sy[ST_LH][ST_LW];
    const int t = (int)threadIdx.x, lane = t & 63, wv = t >> 6;
    const int ty = (int)(blockIdx.x / a.tiles_x), tx = (int)(blockIdx.x - (uint32_t)ty * a.tiles_x);
    const int x0 = tx * ST_W, y0 = ty * ST_H; // the tile's first output, and the first pixel of that output's window
    for (int i = t; i < ST_LH * ST_LW; i += 256) {
        const int r = i / ST_LW, c = i - r * ST_LW;
        const int gr = y0 + r, gc = x0 + c;
        const bool in = gr < a.rows && gc < a.cols;
        sx[r][c] = in ? pixel_scalar<PIX>(a.a, (size_t)gr * a.stride_a + (size_t)gc) : 0.0;
        sy[r][c] = in ? pixel_scalar<PIX>(a.b, (size_t)gr * a.stride_b + (size_t)gc) : 0.0;
    }
    __syncthreads();
    double mu_x[ST_PER], mu_y[ST_PER], mu_x_sq[ST_PER], mu_y_sq[ST_PER], mu_xy[ST_PER];
#pragma unroll
    for (int k = 0; k < ST_PER; ++k) mu_x[k] = mu_y[k] = mu_x_sq[k] = mu_y_sq[k] = mu_xy[k] = 0.0;
    // A staged row feeds the windows of up to four outputs; each output still meets its taps in dy, dx order (:85-98).
#pragma unroll 1
    for (int ry = 0; ry < ST_PER + HALO; ++ry) {
        const double *row_x = sx[wv * ST_PER + ry] + lane, *row_y = sy[wv * ST_PER + ry] + lane;
#pragma unroll
        for (int dx = 0; dx < WIN; ++dx) {
            const double val_x = row_x[dx], val_y = row_y[dx];
#pragma unroll
            for (int k = 0; k < ST_PER; ++k) {
                const int dy = ry - k;
                if (dy >= 0 && dy < WIN) { // uniform
                    const double weight = win.w[dy * WIN + dx];
                    mu_x[k] += weight * val_x;
                    mu_y[k] += weight * val_y;
                    mu_x_sq[k] += weight * val_x * val_x;
                    mu_y_sq[k] += weight * val_y * val_y;
                    mu_xy[k] += weight * val_x * val_y;
                }
            }
        }
    }
    const int ox = x0 + lane;
#pragma unroll
    for (int k = 0; k < ST_PER; ++k) {
        const int oy = y0 + wv * ST_PER + k;
        if (ox >= a.cols - HALO || oy >= a.rows - HALO) continue;
        const double sigma_x_sq = fmax(0.0, mu_x_sq[k] - mu_x[k] * mu_x[k]); // :100-102
        const double sigma_y_sq = fmax(0.0, mu_y_sq[k] - mu_y[k] * mu_y[k]);
        const double sigma_xy = mu_xy[k] - mu_x[k] * mu_y[k];
        const double numerator = (2.0 * mu_x[k] * mu_y[k] + a.c1) * (2.0 * sigma_xy + a.c2); // :104-105
        const double denominator = (mu_x[k] * mu_x[k] + mu_y[k] * mu_y[k] + a.c1) * (sigma_x_sq + sigma_y_sq + a.c2);
        a.out[(size_t)oy * (size_t)(a.cols - HALO) + (size_t)ox] = numerator / denominator;
    }
}

// ---- host ------------------------------------------------------------------------------------------------------------------------------

bool have_device() { // asked once per process
    static const bool ok = [] {
        int n = 0;
        const bool r = hipGetDeviceCount(&n) == hipSuccess && n > 0;
        if (!r) (void)hipGetLastError();
        return r;
    }();
    return ok;
}

double component_max(int pixel) { return pixel_is_float(pixel) ? 1.0 : 255.0; } // componentMaxValue (:177-186)

enum { PSNR = 0, MPE = 1, SSIM = 2 };
const char *const NAMES[] = {"psnr", "mean_pixel_error", "ssim"};

int check(int which, const zg_image *a, const zg_image *b, const void *result, bool device) {
    const char *name = NAMES[which];
    int rc;
    if ((rc = check_image(a, name, device))) return rc;
    if ((rc = check_image(b, name, device))) return rc;
    ZG_REQUIRE(result != nullptr, ZG_ERR_INVALID_ARGUMENT, "%s: null result", name);
    ZG_REQUIRE(a->pixel == b->pixel, ZG_ERR_INVALID_ARGUMENT, "%s: pixel types %d and %d differ", name, a->pixel, b->pixel);
    ZG_REQUIRE(a->rows == b->rows && a->cols == b->cols, ZG_ERR_DIMENSION_MISMATCH, "%s: %u x %u and %u x %u (error.DimensionMismatch)", name, a->rows,
               a->cols, b->rows, b->cols); // :11,57,115
    const uint64_t components = (uint64_t)a->rows * a->cols * pixel_channels(a->pixel);
    if (which == SSIM) {
        ZG_REQUIRE(a->rows >= (uint32_t)WIN && a->cols >= (uint32_t)WIN, ZG_ERR_INVALID_ARGUMENT, "ssim: %u x %u, below 11 x 11 (error.ImageTooSmall)", a->rows,
                   a->cols); // :60
        ZG_REQUIRE((uint64_t)a->rows * a->cols < (1ull << 31), ZG_ERR_UNSUPPORTED, "ssim: %u x %u pixels, 2^31 or more", a->rows, a->cols);
    } else if (!pixel_is_float(a->pixel)) {
        const uint64_t term_max = which == PSNR ? 255ull * 255ull : 255ull;
        ZG_REQUIRE(components < ONE53 / term_max, ZG_ERR_UNSUPPORTED, "%s: the sum over %llu components could reach 2^53", name, (unsigned long long)components);
    } else {
        ZG_REQUIRE(components < (1ull << 40), ZG_ERR_UNSUPPORTED, "%s: %llu components, 2^40 or more", name, (unsigned long long)components);
    }
    ZG_REQUIRE(have_device(), ZG_ERR_HIP, "%s: no device", name);
    return ZG_OK;
}

// psnr (mode MEAN: value is the mse) and meanPixelError (mode MEAN_OVER_MAX)
template <bool SQ> int difference_metric(const zg_image *a, const zg_image *b, zg_metric_result *result, hipStream_t s) {
    const uint32_t ch = (uint32_t)pixel_channels(a->pixel);
    const uint64_t components = (uint64_t)a->rows * a->cols * ch;
    const int mode = SQ ? MODE_MEAN : MODE_MEAN_OVER_MAX;
    const double max_value = component_max(a->pixel);
    if (pixel_is_float(a->pixel)) {
        const ImageTerms<SQ> gen{(const float *)a->data, (const float *)b->data, (uint64_t)a->stride * ch, (uint64_t)b->stride * ch, a->cols * ch};
        return sum_terms(gen, components, 0, mode, components, max_value, result, s);
    }
    SumArgs fin{};
    fin.mode = mode;
    fin.count = components;
    fin.max_value = max_value;
    fin.result = result;
    ScratchBlock sc(s);
    int rc;
    if ((rc = sc.alloc(256))) return rc;
    unsigned long long *acc = (unsigned long long *)sc.p;
    if ((rc = fill_async(acc, 0, sizeof *acc, s))) return rc;
    if (components) {
        const uint32_t row_bytes = a->cols * ch;
        hipLaunchKernelGGL(k_int_terms<SQ>, row_grid(ceil_div(row_bytes, INT_SPAN), a->rows), dim3(256), 0, s, (const uint8_t *)a->data, (const uint8_t *)b->data,
                           (uint64_t)a->stride * ch, (uint64_t)b->stride * ch, row_bytes, a->rows, acc);
        if ((rc = launch_ok("k_int_terms"))) return rc;
    }
    hipLaunchKernelGGL(k_int_finish, dim3(1), dim3(1), 0, s, (const unsigned long long *)acc, fin);
    return launch_ok("k_int_finish");
}

void ssim_window(double w[WIN * WIN]) { // generateSsimWindow (:230-249)
    const double sigma = 1.5;
    double sum = 0.0;
    for (int dy = 0; dy < WIN; ++dy) {
        for (int dx = 0; dx < WIN; ++dx) {
            const double y = (double)dy - (double)(WIN / 2), x = (double)dx - (double)(WIN / 2);
            const double gauss = hostmath::exp_f64(-(x * x + y * y) / (2.0 * sigma * sigma));
            w[dy * WIN + dx] = gauss;
            sum += gauss;
        }
    }
    for (int i = 0; i < WIN * WIN; ++i) w[i] /= sum;
}

int ssim(const zg_image *a, const zg_image *b, const double *window, double *map, zg_metric_result *result, hipStream_t s) {
    SsimWindow win;
    if (window) std::memcpy(win.w, window, sizeof win.w);
    else ssim_window(win.w);
    const uint32_t out_rows = a->rows - HALO, out_cols = a->cols - HALO;
    const uint64_t n = (uint64_t)out_rows * out_cols;
    ScratchBlock sc(s);
    if (!map) {
        sc.take(map, n);
        if (const int rc = sc.alloc()) return rc;
    }
    const double l = component_max(a->pixel), k1 = 0.01, k2 = 0.03; // :64-68
    SsimArgs g{};
    g.a = a->data;
    g.b = b->data;
    g.stride_a = a->stride;
    g.stride_b = b->stride;
    g.rows = (int)a->rows;
    g.cols = (int)a->cols;
    g.c1 = (k1 * l) * (k1 * l);
    g.c2 = (k2 * l) * (k2 * l);
    g.out = map;
    g.tiles_x = ceil_div(out_cols, (unsigned)ST_W);
    const unsigned tiles = g.tiles_x * ceil_div(out_rows, (unsigned)ST_H);
    int rc = dispatch_pixel(a->pixel, [&](auto tag) {
        hipLaunchKernelGGL(k_ssim<decltype(tag)::value>, dim3(tiles), dim3(256), 0, s, g, win);
        return launch_ok("k_ssim");
    });
    if (rc) return rc;
    return sum_terms(ArrayTerms{map}, n, 0, MODE_MEAN, n, 1.0, result, s);
}

const zg_metric_options DEFAULTS{nullptr, nullptr};

// the host forms: stage both images, run, bring the record (and the map) back
int host_metric(int which, const zg_image *a, const zg_image *b, const zg_metric_options *opt, double *value, zg_metric_result *result) {
    if (!opt) opt = &DEFAULTS;
    int rc;
    zg_metric_result res{};
    ZG_REQUIRE(value != nullptr, ZG_ERR_INVALID_ARGUMENT, "%s: null value", NAMES[which]);
    if ((rc = check(which, a, b, &res, false))) return rc;
    HostStage sa, sb;
    if ((rc = sa.upload(a, true, false))) return rc;
    if ((rc = sb.upload(b, true, false))) return rc;
    ScratchBlock sc;
    zg_metric_result *res_dev = nullptr;
    double *map_dev = nullptr;
    const uint64_t map_n = which == SSIM && opt->ssim_map ? (uint64_t)(a->rows - HALO) * (a->cols - HALO) : 0;
    sc.take(res_dev, 1);
    if (map_n) sc.take(map_dev, map_n);
    if ((rc = sc.alloc())) return rc;
    if (which == PSNR) rc = difference_metric<true>(&sa.dev, &sb.dev, res_dev, nullptr);
    else if (which == MPE) rc = difference_metric<false>(&sa.dev, &sb.dev, res_dev, nullptr);
    else rc = ssim(&sa.dev, &sb.dev, opt->ssim_window, map_dev, res_dev, nullptr);
    if (rc) return rc;
    if ((rc = download_pageable(&res, res_dev, sizeof res, nullptr))) return rc; // waits for the stream
    if (map_n && (rc = download_pageable(opt->ssim_map, map_dev, map_n * sizeof(double), nullptr))) return rc;
    *value = which == PSNR ? zg_psnr_from_mse(res.value, component_max(a->pixel)) : res.value;
    if (result) *result = res;
    return ZG_OK;
}

} // namespace
} // namespace zg

using namespace zg;

extern "C" {

uint32_t zg_sum_f64_chunk(void) { return 1u << CHUNK_LOG2; }

int zg_ssim_window_host(double w[121]) {
    ZG_REQUIRE(w != nullptr, ZG_ERR_INVALID_ARGUMENT, "ssim window: null table");
    ssim_window(w);
    return ZG_OK;
}

double zg_exp_f64_host(double x) { return hostmath::exp_f64(x); }
double zg_log10_f64_host(double x) { return hostmath::log10_f64(x); }

double zg_psnr_from_mse(double mse, double max_value) {
    if (mse == 0.0) return INFINITY;                                                   // :49
    return 20.0 * hostmath::log10_f64(max_value) - 10.0 * hostmath::log10_f64(mse); // :53
}

int zg_sum_f64_sequential(const double *values, uint64_t n, uint32_t chunk_log2, zg_metric_result *result, zg_stream stream) {
    ZG_REQUIRE(result != nullptr, ZG_ERR_INVALID_ARGUMENT, "sequential sum: null result");
    ZG_REQUIRE(values != nullptr || n == 0, ZG_ERR_INVALID_ARGUMENT, "sequential sum: null values");
    ZG_REQUIRE(chunk_log2 == 0 || (chunk_log2 >= CHUNK_LOG2_MIN && chunk_log2 <= CHUNK_LOG2_MAX), ZG_ERR_INVALID_ARGUMENT,
               "sequential sum: chunk_log2 %u (0, or %u .. %u)", chunk_log2, CHUNK_LOG2_MIN, CHUNK_LOG2_MAX);
    ZG_REQUIRE(n < (1ull << 40), ZG_ERR_UNSUPPORTED, "sequential sum: %llu values, 2^40 or more", (unsigned long long)n);
    ZG_REQUIRE(have_device(), ZG_ERR_HIP, "sequential sum: no device");
    return sum_terms(ArrayTerms{values}, n, chunk_log2, MODE_SUM, n, 1.0, result, as_stream(stream));
}

int zg_psnr(const zg_image *a, const zg_image *b, const zg_metric_options *, zg_metric_result *result, zg_stream stream) {
    if (const int rc = check(PSNR, a, b, result, true)) return rc;
    return difference_metric<true>(a, b, result, as_stream(stream));
}

int zg_mean_pixel_error(const zg_image *a, const zg_image *b, const zg_metric_options *, zg_metric_result *result, zg_stream stream) {
    if (const int rc = check(MPE, a, b, result, true)) return rc;
    return difference_metric<false>(a, b, result, as_stream(stream));
}

int zg_ssim(const zg_image *a, const zg_image *b, const zg_metric_options *opt, zg_metric_result *result, zg_stream stream) {
    if (!opt) opt = &DEFAULTS;
    if (const int rc = check(SSIM, a, b, result, true)) return rc;
    return ssim(a, b, opt->ssim_window, opt->ssim_map, result, as_stream(stream));
}

int zg_psnr_host(const zg_image *a, const zg_image *b, const zg_metric_options *opt, double *value, zg_metric_result *result) {
    return host_metric(PSNR, a, b, opt, value, result);
}
int zg_mean_pixel_error_host(const zg_image *a, const zg_image *b, const zg_metric_options *opt, double *value, zg_metric_result *result) {
    return host_metric(MPE, a, b, opt, value, result);
}
int zg_ssim_host(const zg_image *a, const zg_image *b, const zg_metric_options *opt, double *value, zg_metric_result *result) {
    return host_metric(SSIM, a, b, opt, value, result);
}

} // extern "C"
