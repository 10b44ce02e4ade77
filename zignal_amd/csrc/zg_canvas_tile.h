// zg_canvas_tile.h — what every drawing kernel of the canvas shares (canvas.hip: k_canvas, canvas_text.hip: k_text): the pixel a lane
// keeps and setPixel's rule for writing it, the gather of a list's entries onto a tile in list order, and the host's checks and launch shape.
//
// The reference's result at a pixel is a fold, in call order, over every write any call makes to that pixel, and blending writes do not
// commute. So a drawing kernel gathers: one workgroup per CV_TILE x CV_TILE pixels, one lane per pixel. The lane keeps its pixel in
// registers (TilePixel), tile_gather hands it the list's entries that can reach the tile, in list order, and the pixel is loaded once
// before the first of them and stored once after the last if anything wrote it.
// Everything a kernel calls here is inlined: the canvas kernels have no calls and no stack.
#pragma once
#include "zg_internal.h"
#include "zg_blend.h"

#include <type_traits>

namespace zg {

constexpr int CV_TILE = 16;    // zg_canvas_tile()
constexpr int CV_CHUNK = 1024; // list entries a workgroup tests against its tile between two barriers
using Rgba8 = typename Px<ZG_PIXEL_RGBA_U8>::Vec;

__device__ __forceinline__ Rgba8 rgba_of(const uint8_t color[4]) {
    Rgba8 c;
    c[0] = color[0]; c[1] = color[1]; c[2] = color[2]; c[3] = color[3];
    return c;
}
__device__ __forceinline__ float clampf(float v, float lo, float hi) { return fmaxf(lo, fminf(v, hi)); } // std.math.clamp
__device__ __forceinline__ Rgba8 fade(Rgba8 c, float alpha) { // Rgba(u8).fade (color.zig:447-456)
    c[3] = (uint8_t)(int)truncf((float)c[3] * clampf(alpha, 0.0f, 1.0f));
    return c;
}
// Does the pixel box (l t r b, r and b exclusive; all 0: empty) reach into the tile whose first pixel is (tx0, ty0)?
__device__ __forceinline__ bool tile_meets_box(ushort4 b, int tx0, int ty0) {
    return (int)b.x < tx0 + CV_TILE && (int)b.z > tx0 && (int)b.y < ty0 + CV_TILE && (int)b.w > ty0;
}

// The pixel of lane threadIdx.x of the workgroup of tile (blockIdx.x, blockIdx.y), in registers
template <int PIX> struct TilePixel {
    using P = Px<PIX>;
    typename P::Vec px;
    bool dirty, inside; // written since it was loaded; inside the frame (the last tile of a row or column may reach past it)
    int col, row;

    __device__ __forceinline__ void place(const DImg &img) {
        col = (int)blockIdx.x * CV_TILE + ((int)threadIdx.x & 15); row = (int)blockIdx.y * CV_TILE + ((int)threadIdx.x >> 4);
        inside = col < img.cols && row < img.rows;
        dirty = false;
        px = P::zero();
    }
    __device__ __forceinline__ void solid(Rgba8 c) { // dest.* = convertColor(T, color)
        if (!inside) return;
        px = convert_px<ZG_PIXEL_RGBA_U8, PIX>(c);
        dirty = true;
    }
    // setPixel with an Rgba colour (Canvas.zig:504-514): it hands assignPixel (image.zig:67-94) convertColor(T, color), so only an Rgba
    // destination still has an Rgba sample to blend (when a != 255). On u8 and Rgb the converted sample has lost its alpha and is stored
    // whatever the alpha was, a faded alpha of 0 included. renderGlyphUnscaled's hoisted form (:1559-1579) is the same rule.
    __device__ __forceinline__ void pixel(Rgba8 c) {
        if (!inside) return;
        if constexpr (PIX == ZG_PIXEL_RGBA_U8) {
            if (c[3] != 255) blend_u8(px, c, 1); else px = c;
        } else {
            px = convert_px<ZG_PIXEL_RGBA_U8, PIX>(c);
        }
        dirty = true;
    }
};

// The gather, entered by all 256 lanes of the workgroup together. hits(i): can entry i of the list of n write into this tile? It is
// asked by one lane per entry. apply(i): make entry i's writes to this lane's pixel; it is called by all lanes together (i is uniform,
// so it may hold barriers), for the entries that hit only, in list order.
// CV_CHUNK entries at a time, in CV_CHUNK / 256 slices of 256 (slice j: entries base + 256 j + tid), with one pair of barriers per
// chunk: every wave counts each slice's hits with a ballot, and after the barrier a hit's place in s_list is the hits of earlier
// slices, then of earlier waves of its slice, then of earlier lanes of its wave. No atomics: the order of s_list is the list's by
// construction, and that order is the correctness argument of every kernel that draws through here.
template <int PIX, typename Hits, typename Apply>
__device__ __forceinline__ void tile_gather(const DImg &img, TilePixel<PIX> &t, uint32_t n, Hits hits, Apply apply) {
    using P = Px<PIX>;
    __shared__ uint16_t s_list[CV_CHUNK];
    __shared__ int s_wave_count[CV_CHUNK / 64];
    const int tid = (int)threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const size_t index = (size_t)t.row * img.stride + (size_t)t.col;
    bool loaded = false;
    for (uint32_t base = 0; base < n; base += CV_CHUNK) {
        bool hit[CV_CHUNK / 256];
        unsigned long long ballot[CV_CHUNK / 256];
#pragma unroll
        for (int j = 0; j < CV_CHUNK / 256; ++j) {
            const uint32_t i = base + 256u * j + (uint32_t)tid;
            hit[j] = false;
            if (i < n) hit[j] = hits(i);
            ballot[j] = __ballot(hit[j]);
            if (lane == 0) s_wave_count[4 * j + wave] = __popcll(ballot[j]);
        }
        __syncthreads();
        int total = 0;
#pragma unroll
        for (int j = 0; j < CV_CHUNK / 256; ++j) {
            int before = total;
            for (int w = 0; w < 4; ++w) {
                const int cnt = s_wave_count[4 * j + w];
                if (w < wave) before += cnt;
                total += cnt;
            }
            if (hit[j]) s_list[before + __popcll(ballot[j] & ((1ull << lane) - 1ull))] = (uint16_t)(256 * j + tid);
        }
        __syncthreads();
        if (total > 0 && !loaded) {
            if (t.inside) t.px = P::load(img.data, index);
            loaded = true;
        }
        for (int k = 0; k < total; ++k) apply(base + (uint32_t)__builtin_amdgcn_readfirstlane((int)s_list[k]));
        __syncthreads();
    }
    if (t.dirty && t.inside) P::store(img.data, index, t.px);
}

// ---- the host's side ----------------------------------------------------------------------------------------------------------------
// The image a drawing entry point takes; `who` is the entry point's name in the messages
inline int check_draw_image(const zg_image *img, bool device_pointer, const char *who) {
    if (const int rc = check_image(img, "img", device_pointer)) return rc;
    ZG_REQUIRE(img->pixel == ZG_PIXEL_U8 || img->pixel == ZG_PIXEL_RGB_U8 || img->pixel == ZG_PIXEL_RGBA_U8, ZG_ERR_UNSUPPORTED,
               "%s: pixel type %d (u8, Rgb(u8) and Rgba(u8) are drawn on)", who, img->pixel);
    ZG_REQUIRE(img->rows <= ZG_CANVAS_MAX_SIZE && img->cols <= ZG_CANVAS_MAX_SIZE, ZG_ERR_UNSUPPORTED, "%s: %u x %u image (at most %u each way)", who,
               img->rows, img->cols, ZG_CANVAS_MAX_SIZE);
    return ZG_OK;
}
inline dim3 tile_grid(const zg_image *img) { return dim3(ceil_div(img->cols, CV_TILE), ceil_div(img->rows, CV_TILE)); }
// f(std::integral_constant<int, PIX>) for the pixel type of an image that check_draw_image let through
template <typename F> inline void dispatch_u8_pixel(int pixel, F f) {
    switch (pixel) {
    case ZG_PIXEL_U8: f(std::integral_constant<int, ZG_PIXEL_U8>{}); break;
    case ZG_PIXEL_RGB_U8: f(std::integral_constant<int, ZG_PIXEL_RGB_U8>{}); break;
    default: f(std::integral_constant<int, ZG_PIXEL_RGBA_U8>{}); break;
    }
}

} // namespace zg
