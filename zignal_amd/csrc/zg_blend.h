// zg_blend.h — Rgba(u8).blend and convertColor between the image pixel types as device functions: what assignPixel (reference
// src/image.zig:67-94) applies to one pixel. Shared by Image.insert (geom.hip) and the Canvas (canvas.hip) so that both composite with the
// same bits by construction. No FMA may be formed from this arithmetic: the library is built with -ffp-contract=off (Makefile).
#pragma once
#include "zg_common.h"

namespace zg {

// Rgba(u8).blend(overlay, mode) — blendColors, reference src/blending.zig:27-157; mode = the Blending ordinal (none 0 ...
// exclusion 12). f32 per channel in the reference's operation order (its vector products are left-associative).
__device__ inline float blend_channel(int mode, float b, float o) {
    switch (mode) {
    case 1: return o;
    case 2: return b * o;
    case 3: return 1.0f - (1.0f - b) * (1.0f - o);
    case 4: return b < 0.5f ? (2.0f * b) * o : 1.0f - (2.0f * (1.0f - b)) * (1.0f - o);
    case 5: return o <= 0.5f ? b - ((1.0f - 2.0f * o) * b) * (1.0f - b) : b + (2.0f * o - 1.0f) * (sqrtf(b) - b);
    case 6: return o < 0.5f ? (2.0f * o) * b : 1.0f - (2.0f * (1.0f - o)) * (1.0f - b);
    case 7: { const float r = b / (1.0f - o); return b == 0.0f ? 0.0f : (o >= 1.0f ? 1.0f : fminf(1.0f, r)); }
    case 8: { const float r = 1.0f - (1.0f - b) / o; return b >= 1.0f ? 1.0f : (o <= 0.0f ? 0.0f : fmaxf(0.0f, r)); }
    case 9: return fminf(b, o);
    case 10: return fmaxf(b, o);
    case 11: return fabsf(b - o);
    case 12: return (b + o) - (2.0f * b) * o;
    }
    return o;
}
__device__ inline void blend_u8(typename Px<ZG_PIXEL_RGBA_U8>::Vec &base, typename Px<ZG_PIXEL_RGBA_U8>::Vec overlay, int mode) {
    if (overlay[3] == 0) return;
    if (base[3] == 0 || (mode == 1 && overlay[3] == 255)) { base = overlay; return; }
    float b[4], o[4], out[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) { b[i] = (float)base[i] / 255.0f; o[i] = (float)overlay[i] / 255.0f; }
    float blended[3];
#pragma unroll
    for (int i = 0; i < 3; ++i) blended[i] = blend_channel(mode, b[i], o[i]);
    if (overlay[3] == 255) {
        out[0] = blended[0]; out[1] = blended[1]; out[2] = blended[2]; out[3] = 1.0f;
    } else {
        const float result_a = o[3] + b[3] * (1.0f - o[3]);
        if (result_a <= 0) { base = Px<ZG_PIXEL_RGBA_U8>::zero(); return; }
        const float base_weight = b[3] * (1.0f - o[3]);
        const float inv = 1.0f / result_a;
#pragma unroll
        for (int i = 0; i < 3; ++i) out[i] = (blended[i] * o[3] + b[i] * base_weight) * inv;
        out[3] = result_a;
    }
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const float v = out[i] < 0.0f ? 0.0f : (out[i] > 1.0f ? 1.0f : out[i]);
        base[i] = (uint8_t)(int)roundf(255.0f * v);
    }
}

// convertColor between the six image pixel types (color.zig:108-151 with the scalar / Rgb / Rgba rules of :365-390, :484-512,
// :1031-1047): what assignPixel applies when source and destination types differ.
template <int SPIX, int DPIX> __device__ inline typename Px<DPIX>::Vec convert_px(typename Px<SPIX>::Vec sv) {
    using SP = Px<SPIX>;
    using DP = Px<DPIX>;
    constexpr bool SF = std::is_same<typename SP::Elem, float>::value, DF = std::is_same<typename DP::Elem, float>::value;
    constexpr int SC = SP::C, DC = DP::C;
    typename DP::Vec d = DP::zero();
    // std.math.clamp(v, 0, 1) = @max(0, @min(v, 1)), and @min / @max return the other operand when one is NaN: a NaN clamps to 1 (the byte 255)
    auto u8_of = [](float v) -> uint8_t { const float c = v != v ? 1.0f : (v < 0.0f ? 0.0f : (v > 1.0f ? 1.0f : v)); return (uint8_t)(int)roundf(255.0f * c); };
    if constexpr (DC == 1) {
        if constexpr (SC == 1) { // scalar <-> scalar (:113-119)
            if constexpr (SF == DF) d[0] = sv[0];
            else if constexpr (!SF) d[0] = (float)sv[0] / 255.0f;
            else { double v = (double)sv[0]; v = v != v ? 1.0 : (v < 0.0 ? 0.0 : (v > 1.0 ? 1.0 : v)); d[0] = (uint8_t)(int)round(v * 255.0); }
        } else if constexpr (!SF) { // colour(u8) -> luminance, BT.709 16.16 fixed point
            const int y0 = (13933 * (int)sv[0] + 46871 * (int)sv[1] + 4732 * (int)sv[2] + 32768) >> 16;
            const int y = y0 < 0 ? 0 : (y0 > 255 ? 255 : y0);
            if constexpr (DF) d[0] = (float)y / 255.0f; else d[0] = (uint8_t)y;
        } else {
            float y = 0.2126f * sv[0] + 0.7152f * sv[1] + 0.0722f * sv[2];
            y = y != y ? 1.0f : (y < 0.0f ? 0.0f : (y > 1.0f ? 1.0f : y)); // rgbToGray's clamp (color.zig:1045): NaN -> 1, for an f32 destination too
            if constexpr (DF) d[0] = y; else d[0] = u8_of(y);
        }
    } else if constexpr (SC == 1) { // scalar -> colour: Gray(Src).as(DestT), replicated, opaque
        typename DP::Elem g;
        if constexpr (SF == DF) g = sv[0];
        else if constexpr (!SF) g = (float)sv[0] / 255.0f;
        else g = u8_of(sv[0]);
        d[0] = g; d[1] = g; d[2] = g;
        if constexpr (DC == 4) d[3] = DF ? (typename DP::Elem)1 : (typename DP::Elem)255;
    } else { // colour -> colour: component type first (.as), then Rgb <-> Rgba
#pragma unroll
        for (int i = 0; i < 3; ++i) {
            if constexpr (SF == DF) d[i] = sv[i];
            else if constexpr (!SF) d[i] = (float)sv[i] / 255.0f;
            else d[i] = u8_of(sv[i]);
        }
        if constexpr (DC == 4) {
            if constexpr (SC == 4) {
                if constexpr (SF == DF) d[3] = sv[3];
                else if constexpr (!SF) d[3] = (float)sv[3] / 255.0f;
                else d[3] = u8_of(sv[3]);
            } else d[3] = DF ? (typename DP::Elem)1 : (typename DP::Elem)255;
        }
    }
    return d;
}

} // namespace zg
