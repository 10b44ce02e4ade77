// quantize.hip — palette quantisation and dithering (reference src/image/quantize.zig, src/image/dither.zig and mapImageToPalette,
// src/codecs/gif.zig:875-920) on the device, bit for bit. Everything here is integer arithmetic.
//
//   k_hist_init / k_hist   the 32768-cell colour histogram medianCut starts from, and for every cell the raster index of its first pixel
//                          (the reference appends a cell to touched_indices when the scan first meets it, and the unstable sort below
//                          makes the palette depend on that order). Counts are privatised in LDS (128 KiB, one workgroup a CU) and merged
//                          with global atomics; `first` is an atomic minimum behind a plain read that skips it once the cell has settled.
//   median_cut()           host code: the reference step by step, Zig's std.sort.heap restated (heap_sort below).
//   k_lut                  ColorLookupTable.init: a lane per cell, the palette in LDS, dist << 8 | index minimised.
//   k_ordered              applyOrdered: a lane per pixel.
//   k_dither_ed            applyErrorDiffusion, Floyd-Steinberg and Atkinson. Every update of the reference is
//                          clampToU8(value + divTruncPow2(err * weight, shift)), and the clamp after each update makes the order of the
//                          updates into one pixel part of the result. In raster order pixel (r, x) has received, before it is quantised,
//                            Floyd-Steinberg   (r-1, x-1) w 1, (r-1, x) w 5, (r-1, x+1) w 3, (r, x-1) w 7, all >> 4
//                            Atkinson          (r-2, x), (r-1, x-1), (r-1, x), (r-1, x+1), (r, x-2), (r, x-1), all w 1 >> 3
//                          in that order (the reference's interior branch and its bounds-checked branch apply the same entries in the same
//                          order), so the in-place scatter equals a gather per pixel: start from the source byte, apply the neighbours'
//                          errors in that order, clamp after each; a neighbour's error is its gathered value minus its palette colour.
//                          Row r needs row r-1 two columns ahead for both kernels: a lane owns a row and runs two columns behind the lane
//                          above. See the kernel for the bands, the phases and the ring.
//   k_to_rgb / k_map       mapImageToPalette's conversion to the Rgb work frame and its lookup with the transparent index.
#include "zg_common.h"

#include <algorithm>
#include <cstring>
#include <vector>

#include "../../include/zignal_hip_quantize.h"

namespace zg {
namespace {

constexpr uint32_t CELLS = ZG_HISTOGRAM_CELLS;

// convertColor(Rgb, pixel) of a byte pixel as r | g << 8 | b << 16: a u8 replicates, an Rgba drops its alpha
template <int PIX> __device__ inline uint32_t load_rgb(const uint8_t *base, size_t idx) {
    if constexpr (PIX == ZG_PIXEL_U8) {
        return (uint32_t)base[idx] * 0x010101u;
    } else {
        const uint8_t *p = base + idx * Px<PIX>::BYTES;
        return (uint32_t)p[0] | (uint32_t)p[1] << 8 | (uint32_t)p[2] << 16;
    }
}
// r5 << 10 | g5 << 5 | b5
__host__ __device__ inline uint32_t cell_of(uint32_t rgb) { return ((rgb & 0xf8u) << 7) | (((rgb >> 8) & 0xf8u) << 2) | ((rgb >> 19) & 0x1fu); }
__host__ __device__ inline uint32_t expand5(uint32_t v) { return (v << 3) | (v >> 2); }

// ---- histogram -------------------------------------------------------------------------------------------------------------------

constexpr int HIST_THREADS = 1024, HIST_PIXELS_PER_THREAD = 16, HIST_MAX_BLOCKS = 256;

__global__ __launch_bounds__(256) void k_hist_init(uint32_t *counts, uint32_t *first) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    counts[i] = 0;
    first[i] = ZG_HISTOGRAM_UNTOUCHED;
}

// Workgroup b owns the raster indices [b * span, min((b + 1) * span, n)); n < 2^32.
template <int PIX>
__global__ __launch_bounds__(HIST_THREADS) void k_hist(const uint8_t *data, uint64_t stride, uint32_t cols, uint64_t n, uint64_t span, uint32_t *counts,
                                                       uint32_t *first) {
    __shared__ uint32_t h[CELLS];
    const int tid = threadIdx.x, lane = tid & 63;
    for (uint32_t i = tid; i < CELLS; i += HIST_THREADS) h[i] = 0;
    __syncthreads();
    const uint64_t begin = (uint64_t)blockIdx.x * span, end = begin + span < n ? begin + span : n;
    for (uint64_t base = begin; base < end; base += HIST_THREADS) {
        const uint64_t i = base + (uint64_t)tid;
        const bool active = i < end;
        uint32_t key = 0;
        if (active) {
            const uint32_t idx = (uint32_t)i, r = idx / cols, c = idx - r * cols;
            key = cell_of(load_rgb<PIX>(data, (size_t)r * stride + c));
            if (first[key] > idx) atomicMin(&first[key], idx); // a stale read only costs an atomic
        }
        // a wave whose pixels share one cell (a flat frame) adds once
        const unsigned long long mask = __ballot(active);
        if (mask == 0) continue;
        const int leader = __ffsll((long long)mask) - 1;
        const uint32_t k0 = (uint32_t)__shfl((int)key, leader);
        if (__ballot(active && key == k0) == mask) {
            if (lane == leader) atomicAdd(&h[k0], (uint32_t)__popcll(mask));
        } else if (active) {
            atomicAdd(&h[key], 1u);
        }
    }
    __syncthreads();
    for (uint32_t i = tid; i < CELLS; i += HIST_THREADS) {
        const uint32_t v = h[i];
        if (v) atomicAdd(&counts[i], v);
    }
}

// ---- lookup table ----------------------------------------------------------------------------------------------------------------

__host__ __device__ inline uint8_t nearest(const uint32_t *pal, uint32_t n, uint32_t cell) {
    const int tr = (int)expand5(cell >> 10), tg = (int)expand5((cell >> 5) & 31u), tb = (int)expand5(cell & 31u);
    uint32_t best = 0xffffffffu;
    for (uint32_t i = 0; i < n; ++i) {
        const uint32_t p = pal[i];
        const int dr = (int)(p & 255u) - tr, dg = (int)((p >> 8) & 255u) - tg, db = (int)((p >> 16) & 255u) - tb;
        const uint32_t score = ((uint32_t)(dr * dr + dg * dg + db * db) << 8) | i;
        best = score < best ? score : best;
    }
    return (uint8_t)(best & 0xffu);
}

__global__ __launch_bounds__(256) void k_lut(const uint8_t *pal, uint32_t n, uint8_t *lut) {
    __shared__ uint32_t sp[256];
    const uint32_t t = threadIdx.x;
    if (t < n) sp[t] = (uint32_t)pal[3 * t] | (uint32_t)pal[3 * t + 1] << 8 | (uint32_t)pal[3 * t + 2] << 16;
    __syncthreads();
    const uint32_t cell = blockIdx.x * 256u + t;
    lut[cell] = nearest(sp, n, cell);
}

// ---- ordered dither --------------------------------------------------------------------------------------------------------------

struct DitherArgs {
    uint8_t *data;
    uint64_t stride; // pixels
    uint32_t rows, cols;
    size_t frame_bytes;
    const uint8_t *pal, *lut;
    uint32_t n;
};

__device__ const int8_t BAYER8[64] = {0,  32, 8,  40, 2,  34, 10, 42, 48, 16, 56, 24, 50, 18, 58, 26, 12, 44, 4,  36, 14, 46, 6,  38, 60, 28, 52, 20, 62, 30, 54, 22,
                                      3,  35, 11, 43, 1,  33, 9,  41, 51, 19, 59, 27, 49, 17, 57, 25, 15, 47, 7,  39, 13, 45, 5,  37, 63, 31, 55, 23, 61, 29, 53, 21};

// blockIdx.x = frame * col_chunks + column chunk; the row is grid_row()
__global__ __launch_bounds__(256) void k_ordered(DitherArgs a, uint32_t col_chunks) {
    const uint32_t frame = blockIdx.x / col_chunks, chunk = blockIdx.x - frame * col_chunks;
    const uint32_t c = chunk * 256u + threadIdx.x;
    const int r = grid_row();
    if (r >= (int)a.rows || c >= a.cols) return;
    uint8_t *p = a.data + (size_t)frame * a.frame_bytes + ((size_t)r * a.stride + c) * 3;
    const int offset = ((int)BAYER8[(r & 7) * 8 + (c & 7)] - 32) >> 1; // arithmetic shift, as the reference's i32
    const uint32_t r5 = (uint32_t)clamp_u8_i32((int)p[0] + offset) >> 3, g5 = (uint32_t)clamp_u8_i32((int)p[1] + offset) >> 3,
                   b5 = (uint32_t)clamp_u8_i32((int)p[2] + offset) >> 3;
    const uint8_t *q = a.pal + 3u * a.lut[r5 << 10 | g5 << 5 | b5];
    p[0] = q[0];
    p[1] = q[1];
    p[2] = q[2];
}

// ---- error diffusion -------------------------------------------------------------------------------------------------------------
//
// One workgroup of 16 waves per frame and launch. Wave w owns the band of rows row0 + 64 w .. + 63, lane l the row l of the band. At the
// wave's local step t lane l quantises column x = t - 2 l - 1, so the lane above is always two columns ahead and its last error is the
// one at (r-1, x+1): a lane keeps its own last four errors (h1 .. h4, three 10-bit signed fields in a word) and the last three it took
// from above; the row above is one cross-lane move away (DPP wave_shr:1), Atkinson's row r-2 another (its error at column x is h4 of lane
// l - 2). Nothing of that goes through memory.
// Between bands: lane 63 (Atkinson: 62 as well) of wave w writes its errors, by column, into the ring of wave w + 1, whose lanes 0 and 1
// read them. Wave w's local step t happens at the workgroup's step t + w * LAG, and the workgroup's steps are cut into phases of PHASE
// with a __syncthreads() between them and nothing else. The error at (r-1, x+1) that lane 0 of wave w + 1 takes at its step t was written
// at wave w's step t + 127, which with LAG = PHASE + 127 lies exactly one phase earlier: behind a barrier. A ring slot is reused RING = 512
// columns later, while writer and reader of one phase are at most 258 columns apart.
// Between launches (rows beyond ROWS_PER_LAUNCH): the last wave writes the same two rows of errors to scratch (carry_out) and wave 0 of
// the next launch, in stream order, copies the columns of a phase from there (carry_in) into its ring before the phase.
// Source pixels reach a lane through LDS: per CHUNK steps the wave copies the CHUNK pixels every lane needs with loads that run along
// rows (eight lanes a row) instead of 64 lanes pulling 64 lines a step, and writes the quantised pixels back the same way.

constexpr int BAND = 64, WAVES = 16, PHASE = 128, ROWS_PER_LAUNCH = BAND * WAVES;
constexpr int LAG = PHASE + 2 * BAND - 1;
constexpr int RING = 512, CHUNK = 8, STAGE_PITCH = CHUNK + 1; // the pitch keeps the lanes' reads on distinct banks
static_assert(CHUNK == 8 && PHASE % CHUNK == 0 && (RING & (RING - 1)) == 0 && RING > PHASE + 2 * BAND + 3, "see above");

struct EdArgs {
    DitherArgs d;
    uint32_t row0;            // first row of this launch
    uint32_t phases;
    const uint32_t *carry_in; // per frame 2 x (cols + 1) words: the errors of rows row0 - 2 and row0 - 1; null for the first launch
    uint32_t *carry_out;      // null for the last launch
};

__device__ inline void wave_sync() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier(); // LDS operations of one wave execute in order; this keeps the compiler from reordering them
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}
__device__ inline uint32_t pack_err(int r, int g, int b) { return ((uint32_t)r & 0x3ffu) | (((uint32_t)g & 0x3ffu) << 10) | (((uint32_t)b & 0x3ffu) << 20); }
template <int CH> __device__ inline int err_of(uint32_t e) { return (int)(e << (22 - 10 * CH)) >> 22; }
// divTruncPow2 (dither.zig:97-104)
template <int SHIFT> __device__ inline int div_trunc_pow2(int v) { return (v + ((v >> 31) & ((1 << SHIFT) - 1))) >> SHIFT; }
template <int WEIGHT, int SHIFT> __device__ inline void diffuse(int &r, int &g, int &b, uint32_t e) {
    r = clamp_u8_i32(r + div_trunc_pow2<SHIFT>(err_of<0>(e) * WEIGHT));
    g = clamp_u8_i32(g + div_trunc_pow2<SHIFT>(err_of<1>(e) * WEIGHT));
    b = clamp_u8_i32(b + div_trunc_pow2<SHIFT>(err_of<2>(e) * WEIGHT));
}
__device__ inline uint32_t ring_get(const uint32_t *ring_row, int col, int cols) { return (col >= 0 && col <= cols) ? ring_row[col & (RING - 1)] : 0u; }

template <bool ATK> __global__ __launch_bounds__(ROWS_PER_LAUNCH) void k_dither_ed(EdArgs a) {
    __shared__ uint8_t s_lut[CELLS];
    __shared__ uint32_t s_pal[256];
    __shared__ uint32_t s_ring[WAVES][2][RING];
    __shared__ uint32_t s_stage[WAVES][BAND * STAGE_PITCH];
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const uint32_t frame = blockIdx.x;
    const int rows = (int)a.d.rows, cols = (int)a.d.cols;
    uint8_t *data = a.d.data + (size_t)frame * a.d.frame_bytes;

    if (((uintptr_t)a.d.lut & 3u) == 0) {
        for (int i = tid; i < (int)CELLS / 4; i += ROWS_PER_LAUNCH) ((uint32_t *)s_lut)[i] = ((const uint32_t *)a.d.lut)[i];
    } else {
        for (int i = tid; i < (int)CELLS; i += ROWS_PER_LAUNCH) s_lut[i] = a.d.lut[i];
    }
    if (tid < 256)
        s_pal[tid] = (uint32_t)tid < a.d.n ? (uint32_t)a.d.pal[3 * tid] | (uint32_t)a.d.pal[3 * tid + 1] << 8 | (uint32_t)a.d.pal[3 * tid + 2] << 16 : 0u;
    for (int i = tid; i < WAVES * 2 * RING; i += ROWS_PER_LAUNCH) (&s_ring[0][0][0])[i] = 0u;
    __syncthreads();

    const int band_row = (int)a.row0 + w * BAND, row = band_row + lane;
    const bool band_live = band_row < rows, row_ok = row < rows;
    const size_t carry_words = 2 * ((size_t)cols + 1);
    const uint32_t *carry_in = a.carry_in ? a.carry_in + (size_t)frame * carry_words : nullptr;
    uint32_t *carry_out = a.carry_out ? a.carry_out + (size_t)frame * carry_words : nullptr;
    uint32_t *ring_in = &s_ring[w][0][0], *ring_out = &s_ring[(w + 1) & (WAVES - 1)][0][0];
    uint32_t *stage = s_stage[w];
    const int last_step = cols + 2 * BAND; // lane 63 hands down column `cols` (an error of zero) at this local step
    uint32_t h1 = 0, h2 = 0, h3 = 0, h4 = 0, up0 = 0, upm1 = 0;

    for (uint32_t g = 0; g < a.phases; ++g) {
        const int tp = (int)(g * PHASE) - w * LAG; // the wave's local step at the start of the phase
        if (band_live && tp + PHASE > 0 && tp <= last_step) {
            if (w == 0 && carry_in) { // columns tp - 3 .. tp + PHASE - 1 of both rows
                for (int i = lane; i < 2 * (PHASE + 3); i += 64) {
                    const int rr = i >= PHASE + 3, c = tp - 3 + (i - rr * (PHASE + 3));
                    if (c >= 0 && c <= cols) ring_in[rr * RING + (c & (RING - 1))] = carry_in[(size_t)rr * (cols + 1) + c];
                }
                wave_sync();
            }
#pragma unroll 1
            for (int ch = 0; ch < PHASE / CHUNK; ++ch) {
                const int t0 = tp + ch * CHUNK;
                if (t0 + CHUNK <= 0 || t0 > last_step) continue;
                // the CHUNK pixels of every lane: pixel i * 64 + lane of the 64 x CHUNK block, eight consecutive lanes a row
#pragma unroll
                for (int i = 0; i < CHUNK; ++i) {
                    const int j = i * 64 + lane, l2 = j >> 3, k = j & 7;
                    const int rr = band_row + l2, x = t0 + k - 2 * l2 - 1;
                    if (rr < rows && x >= 0 && x < cols) {
                        const uint8_t *p = data + ((size_t)rr * a.d.stride + (size_t)x) * 3;
                        stage[l2 * STAGE_PITCH + k] = (uint32_t)p[0] | (uint32_t)p[1] << 8 | (uint32_t)p[2] << 16;
                    }
                }
                wave_sync();
#pragma unroll
                for (int k = 0; k < CHUNK; ++k) {
                    const int x = t0 + k - 2 * lane - 1;
                    uint32_t above = (uint32_t)__builtin_amdgcn_update_dpp(0, (int)h1, 0x138, 0xf, 0xf, true); // wave_shr:1: (r-1, x+1)
                    uint32_t above2 = 0;                                                                         // Atkinson: (r-2, x)
                    if constexpr (ATK) above2 = (uint32_t)__shfl_up((int)h4, 2);
                    if (lane == 0) {
                        above = ring_get(ring_in + RING, x + 1, cols);
                        if constexpr (ATK) above2 = ring_get(ring_in, x, cols);
                    }
                    if constexpr (ATK) {
                        if (lane == 1) above2 = ring_get(ring_in + RING, x, cols);
                    }
                    uint32_t e = 0;
                    if (row_ok && x >= 0 && x < cols) {
                        const uint32_t px = stage[lane * STAGE_PITCH + k];
                        int r = (int)(px & 255u), gch = (int)((px >> 8) & 255u), b = (int)((px >> 16) & 255u);
                        if constexpr (ATK) {
                            diffuse<1, 3>(r, gch, b, above2);
                            diffuse<1, 3>(r, gch, b, upm1);
                            diffuse<1, 3>(r, gch, b, up0);
                            diffuse<1, 3>(r, gch, b, above);
                            diffuse<1, 3>(r, gch, b, h2);
                            diffuse<1, 3>(r, gch, b, h1);
                        } else {
                            diffuse<1, 4>(r, gch, b, upm1);
                            diffuse<5, 4>(r, gch, b, up0);
                            diffuse<3, 4>(r, gch, b, above);
                            diffuse<7, 4>(r, gch, b, h1);
                        }
                        const uint32_t q = s_pal[s_lut[(r >> 3) << 10 | (gch >> 3) << 5 | (b >> 3)]];
                        stage[lane * STAGE_PITCH + k] = q;
                        e = pack_err(r - (int)(q & 255u), gch - (int)((q >> 8) & 255u), b - (int)((q >> 16) & 255u));
                    }
                    if (lane >= (ATK ? BAND - 2 : BAND - 1) && x >= 0 && x <= cols) { // hand down: row 0 of the pair is the band's row 62
                        const int rr = lane - (BAND - 2);
                        if (w < WAVES - 1) ring_out[rr * RING + (x & (RING - 1))] = e;
                        else if (carry_out) carry_out[(size_t)rr * (cols + 1) + x] = e;
                    }
                    h4 = h3;
                    h3 = h2;
                    h2 = h1;
                    h1 = e;
                    upm1 = up0;
                    up0 = above;
                }
                wave_sync();
#pragma unroll
                for (int i = 0; i < CHUNK; ++i) {
                    const int j = i * 64 + lane, l2 = j >> 3, k = j & 7;
                    const int rr = band_row + l2, x = t0 + k - 2 * l2 - 1;
                    if (rr < rows && x >= 0 && x < cols) {
                        const uint32_t q = stage[l2 * STAGE_PITCH + k];
                        uint8_t *p = data + ((size_t)rr * a.d.stride + (size_t)x) * 3;
                        p[0] = (uint8_t)q;
                        p[1] = (uint8_t)(q >> 8);
                        p[2] = (uint8_t)(q >> 16);
                    }
                }
                wave_sync();
            }
        }
        __syncthreads();
    }
}

// ---- map to palette --------------------------------------------------------------------------------------------------------------

template <int PIX> __global__ __launch_bounds__(256) void k_to_rgb(const uint8_t *src, uint64_t stride, uint32_t rows, uint32_t cols, uint8_t *work) {
    const uint32_t c = blockIdx.x * 256u + threadIdx.x;
    const int r = grid_row();
    if (r >= (int)rows || c >= cols) return;
    const uint32_t rgb = load_rgb<PIX>(src, (size_t)r * stride + c);
    uint8_t *p = work + ((size_t)r * cols + c) * 3;
    p[0] = (uint8_t)rgb;
    p[1] = (uint8_t)(rgb >> 8);
    p[2] = (uint8_t)(rgb >> 16);
}

// `work`, when not null, is the dithered rows x cols Rgb frame that is looked up in place of src's pixels; src's alpha decides either way
template <int PIX>
__global__ __launch_bounds__(256) void k_map(const uint8_t *src, uint64_t stride, uint32_t rows, uint32_t cols, const uint8_t *work, uint8_t *indices,
                                             uint64_t indices_stride, const uint8_t *lut, int transparent) {
    const uint32_t c = blockIdx.x * 256u + threadIdx.x;
    const int r = grid_row();
    if (r >= (int)rows || c >= cols) return;
    uint8_t out;
    if (PIX == ZG_PIXEL_RGBA_U8 && transparent >= 0 && src[((size_t)r * stride + c) * 4 + 3] < 128) {
        out = (uint8_t)transparent;
    } else {
        const uint32_t rgb = work ? load_rgb<ZG_PIXEL_RGB_U8>(work, (size_t)r * cols + c) : load_rgb<PIX>(src, (size_t)r * stride + c);
        out = lut[cell_of(rgb)];
    }
    indices[(size_t)r * indices_stride + c] = out;
}

// ---- host ------------------------------------------------------------------------------------------------------------------------

bool have_device() { // asked once per process
    static const bool ok = [] {
        int n = 0;
        const bool r = hipGetDeviceCount(&n) == hipSuccess && n > 0;
        if (!r) (void)hipGetLastError();
        return r;
    }();
    return ok;
}

bool byte_pixel(int pixel) { return pixel == ZG_PIXEL_U8 || pixel == ZG_PIXEL_RGB_U8 || pixel == ZG_PIXEL_RGBA_U8; }

template <typename F> int dispatch_byte_pixel(int pixel, F &&f) {
    switch (pixel) {
    case ZG_PIXEL_U8: return f(std::integral_constant<int, ZG_PIXEL_U8>{});
    case ZG_PIXEL_RGB_U8: return f(std::integral_constant<int, ZG_PIXEL_RGB_U8>{});
    default: return f(std::integral_constant<int, ZG_PIXEL_RGBA_U8>{});
    }
}

int histogram(const zg_image *img, uint32_t *counts, uint32_t *first, hipStream_t s) {
    hipLaunchKernelGGL(k_hist_init, dim3(CELLS / 256), dim3(256), 0, s, counts, first);
    int rc;
    if ((rc = launch_ok("k_hist_init"))) return rc;
    const uint64_t n = (uint64_t)img->rows * img->cols;
    if (n == 0) return ZG_OK;
    const uint64_t per_block = (uint64_t)HIST_THREADS * HIST_PIXELS_PER_THREAD;
    uint64_t blocks = (n + per_block - 1) / per_block;
    if (blocks > HIST_MAX_BLOCKS) blocks = HIST_MAX_BLOCKS;
    uint64_t span = (n + blocks - 1) / blocks;
    span = (span + HIST_THREADS - 1) / HIST_THREADS * HIST_THREADS;
    blocks = (n + span - 1) / span;
    return dispatch_byte_pixel(img->pixel, [&](auto tag) {
        hipLaunchKernelGGL(k_hist<decltype(tag)::value>, dim3((unsigned)blocks), dim3(HIST_THREADS), 0, s, (const uint8_t *)img->data, (uint64_t)img->stride,
                           img->cols, n, span, counts, first);
        return launch_ok("k_hist");
    });
}

int check_histogram(const zg_image *img, const char *name) {
    int rc;
    if ((rc = check_image(img, name, true))) return rc;
    ZG_REQUIRE(byte_pixel(img->pixel), ZG_ERR_UNSUPPORTED, "%s: pixel type %d (u8, Rgb(u8) or Rgba(u8))", name, img->pixel);
    ZG_REQUIRE((uint64_t)img->rows * img->cols < (1ull << 32), ZG_ERR_UNSUPPORTED, "%s: %u x %u pixels, 2^32 or more", name, img->rows, img->cols);
    return ZG_OK;
}

// -- median cut: quantize.zig:175-412 step by step

struct ColorCount {
    uint8_t r, g, b;
    uint32_t count;
};
struct ColorBox { // :30-59; colors is [begin, end) of the colour list
    size_t begin, end;
    uint8_t r_min = 255, r_max = 0, g_min = 255, g_max = 0, b_min = 255, b_max = 0;
    uint32_t population = 0;
    size_t len() const { return end - begin; }
    uint32_t volume() const {
        if (r_max < r_min || g_max < g_min || b_max < b_min) return 0;
        return ((uint32_t)r_max - r_min + 1) * ((uint32_t)g_max - g_min + 1) * ((uint32_t)b_max - b_min + 1);
    }
    int largest_dimension() const {
        const int rr = r_max >= r_min ? r_max - r_min : 0, gr = g_max >= g_min ? g_max - g_min : 0, br = b_max >= b_min ? b_max - b_min : 0;
        if (gr >= rr && gr >= br) return 1;
        if (rr >= br) return 0;
        return 2;
    }
    void measure(const ColorCount *list) { // wrapping u32 population, as the reference's += in a release build never meets
        for (size_t i = begin; i < end; ++i) {
            const ColorCount &c = list[i];
            r_min = std::min(r_min, c.r), r_max = std::max(r_max, c.r);
            g_min = std::min(g_min, c.g), g_max = std::max(g_max, c.g);
            b_min = std::min(b_min, c.b), b_max = std::max(b_max, c.b);
            population += c.count;
        }
    }
};

inline bool less_than(const ColorCount &a, const ColorCount &b, int dim) { return dim == 0 ? a.r < b.r : dim == 1 ? a.g < b.g : a.b < b.b; }

// Zig's std.sort.heap over items[a, b), restated: unstable, and the order it leaves among equal keys is part of the palette
void sift_down(ColorCount *items, size_t a, size_t target, size_t b, int dim) {
    size_t cur = target;
    for (;;) {
        size_t child = 2 * (cur - a) + a + 1;
        if (!(child < b)) break;
        const size_t next = child + 1;
        if (next < b && less_than(items[child], items[next], dim)) child = next;
        if (less_than(items[child], items[cur], dim)) break;
        std::swap(items[child], items[cur]);
        cur = child;
    }
}
void heap_sort(ColorCount *items, size_t a, size_t b, int dim) {
    if (b - a < 2) return;
    size_t i = a + (b - a) / 2;
    while (i > a) {
        --i;
        sift_down(items, a, i, b, dim);
    }
    i = b;
    while (i > a) {
        --i;
        std::swap(items[a], items[i]);
        sift_down(items, a, a, i, dim);
    }
}

int median_cut(const uint32_t *counts, const uint32_t *first, uint32_t max_colors, uint32_t capacity, uint8_t *palette, uint32_t *n_out) {
    // the touched cells in the order the scan met them
    std::vector<std::pair<uint32_t, uint32_t>> touched; // (first, key)
    for (uint32_t key = 0; key < CELLS; ++key)
        if (counts[key]) touched.emplace_back(first[key], key);
    std::sort(touched.begin(), touched.end());
    std::vector<ColorCount> list;
    list.reserve(touched.size());
    for (const auto &t : touched) {
        const uint32_t key = t.second;
        list.push_back(ColorCount{(uint8_t)expand5((key >> 10) & 31u), (uint8_t)expand5((key >> 5) & 31u), (uint8_t)expand5(key & 31u), counts[key]});
    }
    const size_t palette_size = std::min(std::min(list.size(), (size_t)max_colors), (size_t)capacity);
    ZG_REQUIRE(palette_size != 0, ZG_ERR_INVALID_ARGUMENT, "NoPaletteColors: median cut over %zu colours, max_colors %u, capacity %u", list.size(), max_colors,
               capacity);
    if (list.size() == 1) {
        palette[0] = list[0].r, palette[1] = list[0].g, palette[2] = list[0].b;
        *n_out = 1;
        return ZG_OK;
    }
    std::vector<ColorBox> boxes;
    ColorBox initial{0, list.size()};
    initial.measure(list.data());
    boxes.push_back(initial);
    while (boxes.size() < palette_size) {
        ptrdiff_t largest = -1;
        uint64_t largest_score = 0;
        for (size_t i = 0; i < boxes.size(); ++i) {
            const ColorBox &box = boxes[i];
            if (box.len() <= 1) continue;
            if (box.r_max <= box.r_min && box.g_max <= box.g_min && box.b_max <= box.b_min) continue;
            const uint64_t score = (uint64_t)box.volume() * (uint64_t)box.population;
            if (score > largest_score) {
                largest_score = score;
                largest = (ptrdiff_t)i;
            }
        }
        if (largest < 0) break;
        const ColorBox split = boxes[(size_t)largest];
        boxes.erase(boxes.begin() + largest); // orderedRemove
        const int dim = split.largest_dimension();
        heap_sort(list.data(), split.begin, split.end, dim);
        uint64_t total = 0;
        for (size_t i = split.begin; i < split.end; ++i) total += list[i].count;
        const uint64_t half = total / 2;
        uint64_t acc = 0;
        size_t cut = 0;
        for (size_t i = 0; i < split.len(); ++i) {
            acc += list[split.begin + i].count;
            if (acc >= half) {
                cut = std::max((size_t)1, std::min(i + 1, split.len() - 1));
                break;
            }
        }
        ColorBox box1{split.begin, split.begin + cut}, box2{split.begin + cut, split.end};
        box1.measure(list.data());
        box2.measure(list.data());
        if (box1.len() > 0 && box1.r_max >= box1.r_min) boxes.push_back(box1);
        if (box2.len() > 0 && box2.r_max >= box2.r_min) boxes.push_back(box2);
    }
    const size_t actual = std::min(boxes.size(), (size_t)capacity);
    for (size_t i = 0; i < actual; ++i) {
        const ColorBox &box = boxes[i];
        uint64_t rs = 0, gs = 0, bs = 0, ws = 0;
        for (size_t j = box.begin; j < box.end; ++j) {
            const ColorCount &c = list[j];
            rs += (uint64_t)c.r * c.count, gs += (uint64_t)c.g * c.count, bs += (uint64_t)c.b * c.count, ws += c.count;
        }
        uint8_t *p = palette + 3 * i;
        if (ws > 0) {
            p[0] = (uint8_t)(rs / ws), p[1] = (uint8_t)(gs / ws), p[2] = (uint8_t)(bs / ws);
        } else {
            p[0] = (uint8_t)(((unsigned)box.r_min + box.r_max) / 2), p[1] = (uint8_t)(((unsigned)box.g_min + box.g_max) / 2),
            p[2] = (uint8_t)(((unsigned)box.b_min + box.b_max) / 2);
        }
    }
    *n_out = (uint32_t)actual;
    return ZG_OK;
}

// -- fixed palettes (quantize.zig:415-473)

const uint8_t VGA16[16][3] = {{0, 0, 0},       {128, 0, 0}, {0, 128, 0}, {128, 128, 0}, {0, 0, 128}, {128, 0, 128}, {0, 128, 128}, {192, 192, 192},
                              {128, 128, 128}, {255, 0, 0}, {0, 255, 0}, {255, 255, 0}, {0, 0, 255}, {255, 0, 255}, {0, 255, 255}, {255, 255, 255}};

uint32_t fixed_6x7x6(uint8_t *p) {
    for (unsigned r = 0; r < 6; ++r)
        for (unsigned g = 0; g < 7; ++g)
            for (unsigned b = 0; b < 6; ++b) *p++ = (uint8_t)((r * 255 + 2) / 5), *p++ = (uint8_t)((g * 255 + 3) / 6), *p++ = (uint8_t)((b * 255 + 2) / 5);
    return 252;
}
uint32_t fixed_web216(uint8_t *p) {
    for (unsigned r = 0; r < 6; ++r)
        for (unsigned g = 0; g < 6; ++g)
            for (unsigned b = 0; b < 6; ++b) *p++ = (uint8_t)(r * 51), *p++ = (uint8_t)(g * 51), *p++ = (uint8_t)(b * 51);
    return 216;
}

// -- dither

bool mode_valid(int mode) { return mode >= ZG_DITHER_NONE && mode <= ZG_DITHER_AUTO; }

int check_palette(const uint8_t *palette, uint32_t n, const char *name) {
    ZG_REQUIRE(palette != nullptr, ZG_ERR_INVALID_ARGUMENT, "%s: null palette", name);
    ZG_REQUIRE(n >= 1 && n <= 256, ZG_ERR_INVALID_ARGUMENT, "%s: %u palette entries (1 to 256)", name, n);
    return ZG_OK;
}

// Floyd-Steinberg or Atkinson over n_frames frames: a workgroup a frame, a launch per ROWS_PER_LAUNCH rows
int error_diffusion(const DitherArgs &d, uint32_t n_frames, bool atkinson, hipStream_t s) {
    const uint32_t launches = ceil_div(d.rows, (unsigned)ROWS_PER_LAUNCH);
    const size_t carry_words = 2 * ((size_t)d.cols + 1) * n_frames;
    ScratchBlock sc(s); // the two rows of errors that cross a launch boundary, double-buffered: a launch reads one half and writes the other
    uint32_t *carry[2] = {nullptr, nullptr};
    if (launches > 1) {
        sc.take(carry[0], carry_words);
        sc.take(carry[1], carry_words);
        if (const int rc = sc.alloc()) return rc;
    }
    for (uint32_t k = 0; k < launches; ++k) {
        EdArgs a{};
        a.d = d;
        a.row0 = k * ROWS_PER_LAUNCH;
        const uint32_t rows_here = std::min((uint32_t)ROWS_PER_LAUNCH, d.rows - a.row0), bands = ceil_div(rows_here, (unsigned)BAND);
        a.phases = (d.cols + 2 * BAND + (bands - 1) * LAG) / PHASE + 1; // the last band's local step cols + 128 is the workgroup's last
        a.carry_in = k > 0 ? carry[(k - 1) & 1] : nullptr;
        a.carry_out = k + 1 < launches ? carry[k & 1] : nullptr;
        if (atkinson) hipLaunchKernelGGL(k_dither_ed<true>, dim3(n_frames), dim3(ROWS_PER_LAUNCH), 0, s, a);
        else hipLaunchKernelGGL(k_dither_ed<false>, dim3(n_frames), dim3(ROWS_PER_LAUNCH), 0, s, a);
        if (const int rc = launch_ok("k_dither_ed")) return rc;
    }
    return ZG_OK;
}

int dither_frames(const zg_image *img, uint32_t n_frames, size_t frame_bytes, const uint8_t *palette, uint32_t n, const uint8_t *lut, int mode, hipStream_t s) {
    if (mode == ZG_DITHER_NONE || mode == ZG_DITHER_AUTO || img->rows == 0 || img->cols == 0 || n_frames == 0) return ZG_OK;
    DitherArgs d{(uint8_t *)img->data, (uint64_t)img->stride, img->rows, img->cols, frame_bytes, palette, lut, n};
    if (mode != ZG_DITHER_ORDERED) return error_diffusion(d, n_frames, mode == ZG_DITHER_ATKINSON, s);
    const uint32_t col_chunks = ceil_div(img->cols, 256u);
    const uint32_t frames_per_launch = std::max(1u, 0x7fffffffu / col_chunks);
    for (uint32_t f = 0; f < n_frames; f += frames_per_launch) {
        const uint32_t count = std::min(frames_per_launch, n_frames - f);
        DitherArgs part = d;
        part.data += (size_t)f * frame_bytes;
        const dim3 rg = row_grid(col_chunks * count, img->rows);
        hipLaunchKernelGGL(k_ordered, rg, dim3(256), 0, s, part, col_chunks);
        if (const int rc = launch_ok("k_ordered")) return rc;
    }
    return ZG_OK;
}

int check_dither(const zg_image *img, uint32_t n_frames, size_t frame_bytes, const uint8_t *palette, uint32_t n, const uint8_t *lut, int mode) {
    int rc;
    if ((rc = check_image(img, "dither", true))) return rc;
    if ((rc = check_palette(palette, n, "dither"))) return rc;
    ZG_REQUIRE(lut != nullptr, ZG_ERR_INVALID_ARGUMENT, "dither: null lookup table");
    ZG_REQUIRE(mode_valid(mode), ZG_ERR_INVALID_ARGUMENT, "dither: mode %d (0 none, 1 floyd_steinberg, 2 atkinson, 3 ordered, 4 auto)", mode);
    ZG_REQUIRE(img->pixel == ZG_PIXEL_RGB_U8, ZG_ERR_UNSUPPORTED, "dither: pixel type %d (Rgb(u8))", img->pixel);
    if (n_frames > 1 && img->rows && img->cols) {
        const size_t span = ((size_t)(img->rows - 1) * img->stride + img->cols) * 3;
        ZG_REQUIRE(frame_bytes >= span, ZG_ERR_INVALID_ARGUMENT, "dither: frames %zu bytes apart, one spans %zu", frame_bytes, span);
    }
    ZG_REQUIRE(have_device(), ZG_ERR_HIP, "dither: no device");
    return ZG_OK;
}

} // namespace
} // namespace zg

using namespace zg;

extern "C" {

int zg_color_histogram(const zg_image *img, uint32_t *counts_device, uint32_t *first_device, zg_stream stream) {
    int rc;
    if ((rc = check_histogram(img, "color_histogram"))) return rc;
    ZG_REQUIRE(counts_device != nullptr && first_device != nullptr, ZG_ERR_INVALID_ARGUMENT, "color_histogram: null counts or first");
    ZG_REQUIRE(have_device(), ZG_ERR_HIP, "color_histogram: no device");
    return histogram(img, counts_device, first_device, as_stream(stream));
}

int zg_median_cut_from_histogram_host(const uint32_t *counts, const uint32_t *first, uint32_t max_colors, uint32_t capacity, uint8_t *palette_rgb, uint32_t *n) {
    ZG_REQUIRE(counts != nullptr && first != nullptr && palette_rgb != nullptr && n != nullptr, ZG_ERR_INVALID_ARGUMENT, "median_cut: null argument");
    return median_cut(counts, first, max_colors, capacity, palette_rgb, n);
}

int zg_median_cut(const zg_image *img_device, uint32_t max_colors, uint32_t capacity, uint8_t *palette_rgb, uint32_t *n) {
    int rc;
    ZG_REQUIRE(palette_rgb != nullptr && n != nullptr, ZG_ERR_INVALID_ARGUMENT, "median_cut: null argument");
    if ((rc = check_histogram(img_device, "median_cut"))) return rc;
    ZG_REQUIRE(have_device(), ZG_ERR_HIP, "median_cut: no device");
    if ((rc = refuse_under_capture(nullptr, "median_cut (the histogram is read back to the host)"))) return rc;
    ScratchBlock sc;
    if ((rc = sc.alloc(2 * CELLS * sizeof(uint32_t)))) return rc;
    uint32_t *dev = (uint32_t *)sc.p;
    if ((rc = histogram(img_device, dev, dev + CELLS, nullptr))) return rc;
    std::vector<uint32_t> host(2 * CELLS);
    if ((rc = download_pageable(host.data(), dev, host.size() * sizeof(uint32_t), nullptr))) return rc; // waits for the stream
    return median_cut(host.data(), host.data() + CELLS, max_colors, capacity, palette_rgb, n);
}

int zg_build_palette(const zg_image *img_device, int mode, uint32_t max_colors, uint8_t *palette_rgb, uint32_t *n) {
    ZG_REQUIRE(palette_rgb != nullptr && n != nullptr, ZG_ERR_INVALID_ARGUMENT, "build_palette: null argument");
    switch (mode) {
    case ZG_PALETTE_FIXED_6X7X6: *n = fixed_6x7x6(palette_rgb); return ZG_OK;
    case ZG_PALETTE_FIXED_VGA16:
        std::memcpy(palette_rgb, VGA16, sizeof VGA16);
        *n = 16;
        return ZG_OK;
    case ZG_PALETTE_FIXED_WEB216: *n = fixed_web216(palette_rgb); return ZG_OK;
    case ZG_PALETTE_ADAPTIVE:
        if (zg_median_cut(img_device, max_colors, 256, palette_rgb, n) != ZG_OK) *n = fixed_6x7x6(palette_rgb); // the reference's catch
        return ZG_OK;
    }
    set_error("build_palette: mode %d (0 fixed_6x7x6, 1 fixed_vga16, 2 fixed_web216, 3 adaptive)", mode);
    return ZG_ERR_INVALID_ARGUMENT;
}

int zg_palette_lut(const uint8_t *palette_device, uint32_t n, uint8_t *lut_device, zg_stream stream) {
    int rc;
    if ((rc = check_palette(palette_device, n, "palette_lut"))) return rc;
    ZG_REQUIRE(lut_device != nullptr, ZG_ERR_INVALID_ARGUMENT, "palette_lut: null lookup table");
    ZG_REQUIRE(have_device(), ZG_ERR_HIP, "palette_lut: no device");
    hipLaunchKernelGGL(k_lut, dim3(CELLS / 256), dim3(256), 0, as_stream(stream), palette_device, n, lut_device);
    return launch_ok("k_lut");
}

int zg_palette_lut_host(const uint8_t *palette, uint32_t n, uint8_t *lut) {
    int rc;
    if ((rc = check_palette(palette, n, "palette_lut"))) return rc;
    ZG_REQUIRE(lut != nullptr, ZG_ERR_INVALID_ARGUMENT, "palette_lut: null lookup table");
    uint32_t packed[256];
    for (uint32_t i = 0; i < n; ++i) packed[i] = (uint32_t)palette[3 * i] | (uint32_t)palette[3 * i + 1] << 8 | (uint32_t)palette[3 * i + 2] << 16;
    for (uint32_t cell = 0; cell < CELLS; ++cell) lut[cell] = nearest(packed, n, cell);
    return ZG_OK;
}

void zg_dither_geometry(uint32_t *band_rows, uint32_t *phase_cols, uint32_t *rows_per_launch) {
    if (band_rows) *band_rows = BAND;
    if (phase_cols) *phase_cols = PHASE;
    if (rows_per_launch) *rows_per_launch = ROWS_PER_LAUNCH;
}

int zg_dither(const zg_image *img, const uint8_t *palette_device, uint32_t n, const uint8_t *lut_device, int mode, zg_stream stream) {
    int rc;
    if ((rc = check_dither(img, 1, 0, palette_device, n, lut_device, mode))) return rc;
    return dither_frames(img, 1, 0, palette_device, n, lut_device, mode, as_stream(stream));
}

int zg_dither_frames(const zg_image *img, uint32_t n_frames, size_t frame_bytes, const uint8_t *palette_device, uint32_t n, const uint8_t *lut_device, int mode,
                     zg_stream stream) {
    int rc;
    if ((rc = check_dither(img, n_frames, frame_bytes, palette_device, n, lut_device, mode))) return rc;
    return dither_frames(img, n_frames, frame_bytes, palette_device, n, lut_device, mode, as_stream(stream));
}

int zg_palette_map(const zg_image *src, const zg_image *indices, const uint8_t *palette_device, uint32_t n, int use_dither, int transparent_index,
                   zg_stream stream) {
    int rc;
    if ((rc = check_image(src, "palette_map", true))) return rc;
    if ((rc = check_image(indices, "palette_map", true))) return rc;
    if ((rc = check_palette(palette_device, n, "palette_map"))) return rc;
    ZG_REQUIRE(byte_pixel(src->pixel), ZG_ERR_UNSUPPORTED, "palette_map: source pixel type %d (u8, Rgb(u8) or Rgba(u8))", src->pixel);
    ZG_REQUIRE(indices->pixel == ZG_PIXEL_U8, ZG_ERR_INVALID_ARGUMENT, "palette_map: the index plane is u8, not pixel type %d", indices->pixel);
    ZG_REQUIRE(src->rows == indices->rows && src->cols == indices->cols, ZG_ERR_DIMENSION_MISMATCH, "palette_map: source %u x %u, indices %u x %u", src->rows,
               src->cols, indices->rows, indices->cols);
    ZG_REQUIRE(transparent_index <= 255, ZG_ERR_INVALID_ARGUMENT, "palette_map: transparent index %d (below 0: none, else 0 to 255)", transparent_index);
    ZG_REQUIRE(transparent_index < 0 || n >= 2, ZG_ERR_INVALID_ARGUMENT, "palette_map: a transparent index reserves the last of %u palette entries", n);
    ZG_REQUIRE(have_device(), ZG_ERR_HIP, "palette_map: no device");
    if (src->rows == 0 || src->cols == 0) return ZG_OK;
    hipStream_t s = as_stream(stream);
    const uint32_t lookup_n = transparent_index >= 0 ? n - 1 : n; // lookup_palette (gif.zig:884)
    ScratchBlock sc(s);
    uint8_t *lut = nullptr, *work = nullptr;
    sc.take(lut, CELLS);
    if (use_dither) sc.take(work, (size_t)src->rows * src->cols * 3);
    if ((rc = sc.alloc())) return rc;
    hipLaunchKernelGGL(k_lut, dim3(CELLS / 256), dim3(256), 0, s, palette_device, lookup_n, lut);
    if ((rc = launch_ok("k_lut"))) return rc;
    const dim3 grid = row_grid(ceil_div(src->cols, 256u), src->rows);
    if (use_dither) {
        rc = dispatch_byte_pixel(src->pixel, [&](auto tag) {
            hipLaunchKernelGGL(k_to_rgb<decltype(tag)::value>, grid, dim3(256), 0, s, (const uint8_t *)src->data, (uint64_t)src->stride, src->rows, src->cols, work);
            return launch_ok("k_to_rgb");
        });
        if (rc) return rc;
        const DitherArgs d{work, (uint64_t)src->cols, src->rows, src->cols, 0, palette_device, lut, lookup_n};
        if ((rc = error_diffusion(d, 1, false, s))) return rc;
    }
    return dispatch_byte_pixel(src->pixel, [&](auto tag) {
        hipLaunchKernelGGL(k_map<decltype(tag)::value>, grid, dim3(256), 0, s, (const uint8_t *)src->data, (uint64_t)src->stride, src->rows, src->cols,
                           (const uint8_t *)work, (uint8_t *)indices->data, (uint64_t)indices->stride, (const uint8_t *)lut, transparent_index);
        return launch_ok("k_map");
    });
}

} // extern "C"
