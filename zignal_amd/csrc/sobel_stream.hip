// sobel_stream.hip — Image(u8).sobel and Image(Rgba(u8)).sobel as a register-resident stream: one WAVE walks a 1024-byte-wide column
// strip from top to bottom (the strip walker of zg_stream.h), no LDS, no barrier.
//
// Contract (reference src/image/edges.zig:33-70): grey = as(f32, convertColor(u8, px)); gx, gy = the 3 x 3 Sobel sums of the grey plane
// with .replicate borders, in f32; out = @trunc(@max(0, @min(255, @sqrt(gx * gx + gy * gy) / 4))).
// Everything up to the square root is small integers in f32 — grey <= 255, |gx|, |gy| <= 1020, gx^2 + gy^2 <= 2 080 800 < 2^24 — so it is
// exact in any order and this kernel is free to
//   * take Rgba(u8) -> grey as three v_fma_f32 on bytes converted by v_cvt_f32_ubyteN: the BT.709 16.16 sum
//     (13933 R + 46871 G + 4732 B + 32768) <= 16 744 448 is exact in f32, and >> 16 is a multiplication by 2^-16 and a floor
//     (src/color.zig:1031-1042);
//   * form the Sobel sums separably: s = g[r-1] + 2 g[r] + g[r+1] and d = g[r+1] - g[r-1] per column, gx = s[x+1] - s[x-1],
//     gy = d[x-1] + 2 d[x] + d[x+1] (the reference's term order gives the same integers; a zero's sign disappears in the squares);
//   * replace the correctly rounded square root: the result byte is floor(sqrt(m) / 4) for an integer m, and sqrt(m) is never closer
//     than 1 / (8 * 255) = 4.9e-4 below a multiple of 4 unless it IS one; v_sqrt_f32 is good to one ulp (6.1e-5 below 1024), so
//     floor((v_sqrt_f32(m) + 2^-12) / 4) is that byte for every m (checked for all 2 080 801 values: tools/exp/sqrt_probe.hip,
//     profiles/r04_experiments.txt), and v_cvt_pk_u8_f32 saturates it at 255 and packs it.
// A lane owns 16 bytes of every source row: 4 Rgba pixels -> 4 output bytes (one dword store per lane), or 16 grey pixels -> 16
// output bytes. The neighbours' border columns cross the wave as grey FLOATS by DPP; the strip's outer columns come from a narrow
// second load that arrives as the DPP move's `old` operand (zg_stream.h).
//
// Preconditions (else k_sobel runs): source u8 or Rgba(u8), row bytes a multiple of 16, 16-byte aligned rows on both sides of the
// Rgba form (4-byte aligned destination rows), at least 64 pixels per row and 16 rows.
#include "zg_internal.h"
#include "zg_u8pack.h"
#include "zg_stream.h"

#include <algorithm>
#include <cstdlib>
#include <type_traits>

namespace zg {

template <int B> __device__ __forceinline__ float ubyte_f32(uint32_t dword) { return (float)((dword >> (8 * B)) & 0xffu); } // v_cvt_f32_ubyteB
__device__ __forceinline__ float dpp_below(float old, float v) { return __builtin_bit_cast(float, from_lane_below(__builtin_bit_cast(uint32_t, old), __builtin_bit_cast(uint32_t, v))); }
__device__ __forceinline__ float dpp_above(float old, float v) { return __builtin_bit_cast(float, from_lane_above(__builtin_bit_cast(uint32_t, old), __builtin_bit_cast(uint32_t, v))); }

// convertColor(u8, Rgba(u8)) as a float (color.zig:1031-1042): exact in f32, see the file comment
__device__ __forceinline__ float grey_of_rgba(uint32_t px) {
    float acc = __builtin_fmaf(ubyte_f32<0>(px), 13933.0f, 32768.0f);
    acc = __builtin_fmaf(ubyte_f32<1>(px), 46871.0f, acc);
    acc = __builtin_fmaf(ubyte_f32<2>(px), 4732.0f, acc);
    return __builtin_floorf(acc * 0x1p-16f);
}
// @trunc(@max(0, @min(255, @sqrt(m) / 4))) for an integer m in [0, 2^24) as a float, packed into byte `b` of `old`
__device__ __forceinline__ uint32_t sobel_byte(float m, uint32_t b, uint32_t old) {
    const float q = __builtin_floorf(__builtin_fmaf(__builtin_amdgcn_sqrtf(m), 0.25f, 0x1p-14f));
    return __builtin_amdgcn_cvt_pk_u8_f32(q, b, old);
}

template <int SP, int DM>
__global__ __launch_bounds__(64) void k_sobel_stream(StripArgs a) {
    static_assert(SP == 1 || SP == 4, "grey or Rgba(u8) sources");
    constexpr int NPX = 16 / SP;  // pixels a lane owns per row
    constexpr int HB = 1;         // one halo dword per side: one Rgba pixel, or the grey pixel in its byte 3 / byte 0
    constexpr int D = 3 * DM;     // source rows in flight = rows per unrolled block
    constexpr int NG = NPX + 2;   // grey columns a lane holds per row: x - 1 .. x + NPX

    const uint32_t w = xcd_major((uint32_t)blockIdx.x, (uint32_t)gridDim.x);
    const uint8_t *srcf = a.src + (size_t)blockIdx.y * a.src_frame;
    uint8_t *dstf = a.dst + (size_t)blockIdx.y * a.dst_frame;
    // the halo dword: lane 0 the one before the strip, every other lane the one after it (the last lane's); clamped into the row at the
    // image's ends, where .replicate takes the lane's own outer pixel instead
    const StripLane<HB> L(a, w, false);
    const int lx = L.lx, last_lane = L.last_lane, y0 = L.y0;
    const int out_rows = min(y0 + a.strip_rows, a.rows) - y0;
    const int n_in = (out_rows + 2 + D - 1) / D * D;
    const bool fast = a.fast_ok && y0 - 1 >= 0 && y0 - 1 + n_in + D <= a.rows;

    strip_dispatch(fast, L.edges, [&](auto fast_tag, auto edge_tag) {
        constexpr bool EDGE = decltype(edge_tag)::value;
        // .replicate rows; one output byte per source pixel: a lane's unit is 16 / SP bytes
        StripRows<HB, 1, decltype(fast_tag)::value, SP == 4 ? 2 : 0, 0, true> rows(a, L, srcf, dstf, ZG_BORDER_REPLICATE);
        // grey columns x - 1 .. x + NPX of one source row
        auto grey_row = [&](const RowIn<HB> &r, float (&g)[NG]) {
            float gh; // the strip's outer column this lane can supply: lane 0 its left one, the others the right one
            if constexpr (SP == 4) {
#pragma unroll
                for (int p = 0; p < 4; ++p) g[1 + p] = grey_of_rgba(r.v[p]);
                gh = grey_of_rgba(r.h[0]);
            } else {
#pragma unroll
                for (int d = 0; d < 4; ++d) {
                    g[1 + 4 * d] = ubyte_f32<0>(r.v[d]); g[2 + 4 * d] = ubyte_f32<1>(r.v[d]); g[3 + 4 * d] = ubyte_f32<2>(r.v[d]); g[4 + 4 * d] = ubyte_f32<3>(r.v[d]);
                }
                gh = lx == 0 ? ubyte_f32<3>(r.h[0]) : ubyte_f32<0>(r.h[0]);
            }
            g[0] = dpp_below(gh, g[NPX]);
            g[NG - 1] = dpp_above(gh, g[1]);
            if constexpr (EDGE) { // .replicate at the row's ends; a row that ends inside the strip
                if (L.left_edge) g[0] = lx == 0 ? g[1] : g[0];
                if (L.right_edge) g[NG - 1] = lx == last_lane ? g[NPX] : g[NG - 1];
            }
        };

        RowIn<HB> ahead[D];
#pragma unroll
        for (int i = 0; i < D; ++i) {
            ahead[i] = rows.load(y0 - 1 + i);
            __builtin_amdgcn_sched_barrier(0);
        }
        float G[3][NG]; // grey rows, source row q of the strip (row y0 - 1 + q of the image) in slot q % 3
#pragma unroll
        for (int s = 0; s < 3; ++s)
#pragma unroll
            for (int t = 0; t < NG; ++t) G[s][t] = 0.0f;
        for (int qb = 0; qb < n_in; qb += D) {
#pragma unroll
            for (int u = 0; u < D; ++u) {
                const int q = qb + u;
                grey_row(ahead[u], G[u % 3]);
                ahead[u] = rows.load(y0 - 1 + q + D);
                if (q < 2) continue; // wave-uniform
                const float(&top)[NG] = G[(u + 1) % 3], (&mid)[NG] = G[(u + 2) % 3], (&bot)[NG] = G[u % 3]; // rows q - 2, q - 1, q
                float sm[NG], df[NG];
#pragma unroll
                for (int t = 0; t < NG; ++t) {
                    sm[t] = __builtin_fmaf(mid[t], 2.0f, top[t]) + bot[t];
                    df[t] = bot[t] - top[t];
                }
                uint32_t o[NPX / 4];
#pragma unroll
                for (int d = 0; d < NPX / 4; ++d) {
                    uint32_t pk = 0;
#pragma unroll
                    for (int b = 0; b < 4; ++b) {
                        const int t = 1 + 4 * d + b; // column x + 4 d + b
                        const float gx = sm[t + 1] - sm[t - 1];
                        const float gy = __builtin_fmaf(df[t], 2.0f, df[t - 1]) + df[t + 1];
                        pk = sobel_byte(__builtin_fmaf(gx, gx, gy * gy), (uint32_t)b, pk);
                    }
                    o[d] = pk;
                }
                if constexpr (SP == 4) rows.store(o[0], y0 + q - 2);
                else rows.store(u32x4{o[0], o[1], o[2], o[3]}, y0 + q - 2);
            }
        }
    });
}

template <int SP>
static int launch_sobel_stream(const FrameBatch &b, hipStream_t s) {
    StripArgs a{};
    dim3 grid;
    int r = (int)std::min<uint64_t>(std::max<uint64_t>(((uint64_t)b.src->rows * strips_across(b.src, SP) * b.n + 4095) / 4096, 16), 64);
    while ((r + 2) % 3) ++r; // (strip rows + 2) % D == 0
    if (strip_args(a, grid, b, ZG_BORDER_REPLICATE, SP, 1, false, r, 0xffffffffu, true) != 0) return -1;
    hipLaunchKernelGGL((k_sobel_stream<SP, 1>), grid, dim3(64), 0, s, a);
    return launch_ok();
}

// Returns -1 when the preconditions do not hold (the caller runs k_sobel).
int try_sobel_stream(const FrameBatch &b, hipStream_t s) {
    const zg_image *src = b.src, *dst = b.dst;
    if (src->pixel != ZG_PIXEL_U8 && src->pixel != ZG_PIXEL_RGBA_U8) return -1;
    const int sp = src->pixel == ZG_PIXEL_U8 ? 1 : 4;
    const unsigned dalign = sp == 1 ? 16 : 4; // the lane's output unit
    if (!strip_shape_ok(b, sp, dst->stride)) return -1;
    if (dst->stride % dalign || b.dst_frame % dalign || ((uintptr_t)dst->data & (dalign - 1))) return -1;
    return sp == 1 ? launch_sobel_stream<1>(b, s) : launch_sobel_stream<4>(b, s);
}

} // namespace zg
