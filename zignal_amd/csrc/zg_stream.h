// zg_stream.h — the register-resident stream kernels: one wave walks a 1024-byte-wide column strip from top to bottom, a lane owns 16
// consecutive bytes of every row, neighbours' bytes cross the wave with DPP wave shifts, the image's left / right border is synthesised
// in the wave's outer lanes. Here: the kernel arguments and the host code that fills and admits them (conv_sep_stream.hip,
// conv2d_stream.hip, sobel_stream.hip); the leaves every strip kernel uses (DPP shifts, HaloLoad, st_unit, synth_halo,
// resolve_row_near, RowIn); and the walker of conv2d_stream.hip and sobel_stream.hip — a lane's place in its strip, the twelve dwords
// around a lane's unit, the two ways to reach a row, the three-way dispatch. k_sep_stream keeps its own copy of the walker: every
// shared form tried cost it a scalar instruction or hazard padding in some loop (profiles/stream_walker_refactor.txt).
#pragma once
#include "zg_internal.h"
#include "zg_u8pack.h"

#include <type_traits>

namespace zg {

// What every strip kernel is launched with. A route that needs more wraps or extends it.
struct StripArgs {
    const uint8_t *src;
    uint8_t *dst;
    uint64_t src_pitch, dst_pitch; // bytes between rows
    uint64_t src_frame, dst_frame; // bytes between frames
    int32_t rows, row_bytes;       // source rows, bytes per source row
    int32_t strips_x, strips_y;    // work items per frame
    int32_t strip_rows;            // source rows per strip
    int32_t border;
    uint32_t src_span, dst_span;   // bytes from a frame's first byte to the end of its last row
    int32_t fast_ok;               // both spans fit the route's limit: whole-frame descriptors may be used
};

inline uint32_t strips_across(const zg_image *src, uint32_t src_px) { return ceil_div(src->cols * src_px, 1024u); }

// The shape every strip route asks for: rows of whole 16-byte units on 16-byte aligned pitches, frames and base, at least 64 pixels
// and 16 rows, offsets that fit the descriptors' 32 bits. The destination's alignment is the route's own affair (its unit differs).
inline bool strip_shape_ok(const FrameBatch &b, uint64_t src_px, uint64_t dst_pitch) {
    const zg_image &src = *b.src;
    const uint64_t rb = (uint64_t)src.cols * src_px, src_pitch = (uint64_t)src.stride * src_px;
    if (rb % 16 || src_pitch % 16 || b.src_frame % 16 || ((uintptr_t)src.data & 15)) return false;
    if (rb % 1024 == 16) return false; // the last strip would be one lane wide: that lane is first and last at once
    return src.cols >= 64 && src.rows >= 16 && rb <= 0x3fffffffu && src_pitch <= 0x7fffffffu && dst_pitch <= 0x7fffffffu;
}

// Fills `a` and the launch grid for the b.n frames of b: src_px / dst_px are the bytes of a source / destination pixel, `half` says
// that the destination has half the source's rows and columns. The frames go into the work-item number, or into gridDim.y
// (frames_in_y). Whole-frame descriptors are allowed up to spans of fast_limit bytes. Returns -1 when the grid cannot hold the work.
inline int strip_args(StripArgs &a, dim3 &grid, const FrameBatch &b, int border, uint32_t src_px, uint32_t dst_px, bool half, int strip_rows,
                      uint32_t fast_limit, bool frames_in_y) {
    const uint32_t rows = b.src->rows, cols = b.src->cols;
    a.src = (const uint8_t *)b.src->data;
    a.dst = (uint8_t *)b.dst->data;
    a.src_pitch = (uint64_t)b.src->stride * src_px;
    a.dst_pitch = (uint64_t)b.dst->stride * dst_px;
    a.src_frame = b.src_frame;
    a.dst_frame = b.dst_frame;
    a.rows = (int32_t)rows;
    a.row_bytes = (int32_t)(cols * src_px);
    a.strips_x = (int32_t)strips_across(b.src, src_px);
    a.strip_rows = strip_rows;
    a.strips_y = (int32_t)ceil_div(rows, (unsigned)strip_rows);
    a.border = border;
    const uint64_t sspan = (uint64_t)(rows - 1) * a.src_pitch + (uint64_t)a.row_bytes;
    const uint64_t dspan = (uint64_t)((half ? rows / 2 : rows) - 1) * a.dst_pitch + (uint64_t)(half ? cols / 2 : cols) * dst_px;
    a.fast_ok = sspan <= fast_limit && dspan <= fast_limit;
    a.src_span = (uint32_t)sspan;
    a.dst_span = (uint32_t)dspan;
    const uint64_t items = (uint64_t)a.strips_x * a.strips_y * (frames_in_y ? 1 : b.n);
    if (items > 0x7fffffffu || (frames_in_y && b.n > MAX_FRAMES_PER_LAUNCH)) return -1;
    grid = dim3((unsigned)items, frames_in_y ? b.n : 1);
    return 0;
}

// v of the lane below / above; the lane that has none (0 / 63) keeps `old`. Never call these under divergent control flow: a
// lane switched off by EXEC is no source either.
__device__ __forceinline__ uint32_t from_lane_below(uint32_t old, uint32_t v) { return (uint32_t)__builtin_amdgcn_update_dpp((int)old, (int)v, 0x138, 0xf, 0xf, false); } // wave_shr:1
__device__ __forceinline__ uint32_t from_lane_above(uint32_t old, uint32_t v) { return (uint32_t)__builtin_amdgcn_update_dpp((int)old, (int)v, 0x130, 0xf, 0xf, false); } // wave_shl:1

typedef uint32_t u32x2 __attribute__((ext_vector_type(2)));
typedef uint32_t u32x3 __attribute__((ext_vector_type(3)));
template <int HB> struct HaloLoad; // HB dwords at byte offset `off` (per lane) + `soff` (wave-uniform)
template <> struct HaloLoad<1> { __device__ static __forceinline__ void run(__amdgpu_buffer_rsrc_t r, int off, int soff, uint32_t (&h)[1]) { h[0] = __builtin_amdgcn_raw_buffer_load_b32(r, off, soff, 0); } };
template <> struct HaloLoad<2> { __device__ static __forceinline__ void run(__amdgpu_buffer_rsrc_t r, int off, int soff, uint32_t (&h)[2]) {
    const u32x2 v = __builtin_amdgcn_raw_buffer_load_b64(r, off, soff, 0); h[0] = v[0]; h[1] = v[1]; } };
template <> struct HaloLoad<3> { __device__ static __forceinline__ void run(__amdgpu_buffer_rsrc_t r, int off, int soff, uint32_t (&h)[3]) {
    const u32x3 v = __builtin_amdgcn_raw_buffer_load_b96(r, off, soff, 0); h[0] = v[0]; h[1] = v[1]; h[2] = v[2]; } };
template <> struct HaloLoad<4> { __device__ static __forceinline__ void run(__amdgpu_buffer_rsrc_t r, int off, int soff, uint32_t (&h)[4]) {
    const u32x4 v = __builtin_amdgcn_raw_buffer_load_b128(r, off, soff, 0); h[0] = v[0]; h[1] = v[1]; h[2] = v[2]; h[3] = v[3]; } };
__device__ __forceinline__ void st_unit(u32x4 o, __amdgpu_buffer_rsrc_t r, int off) { __builtin_amdgcn_raw_buffer_store_b128(o, r, off, 0, 2); } // nt: written once, never read here
__device__ __forceinline__ void st_unit(u32x2 o, __amdgpu_buffer_rsrc_t r, int off) { __builtin_amdgcn_raw_buffer_store_b64(o, r, off, 0, 2); }
__device__ __forceinline__ void st_unit(uint32_t o, __amdgpu_buffer_rsrc_t r, int off) { __builtin_amdgcn_raw_buffer_store_b32(o, r, off, 0, 2); }

// Byte j (0..15) of the outer lane's own unit that supplies halo byte `pos` of a border halo, or -1 when no tap reaches it.
// Left halo: HB dwords covering stream positions -4 HB .. -1. Right halo: positions rb .. rb + 4 HB - 1, the own unit being
// bytes rb - 16 .. rb - 1. Mirror is reflect-101 (border.zig:46-63): pixel -1 - m -> 1 + m, pixel cols + m -> cols - 2 - m.
template <int SP, int H> constexpr int halo_source(bool right, bool mirror, int byte_in_halo, int hb) {
    if (!right) {
        const int p = -4 * hb + byte_in_halo; // < 0
        const int k = -1 - p;
        if (k >= H * SP) return -1;
        const int m = k / SP, c = SP - 1 - (k % SP);
        return mirror ? (1 + m) * SP + c : c;
    }
    const int k = byte_in_halo;
    if (k >= H * SP) return -1;
    const int m = k / SP, c = k % SP;
    return mirror ? 16 - (2 + m) * SP + c : 16 - SP + c;
}
template <int SP, int H, int HB, bool RIGHT, bool MIRROR> __device__ __forceinline__ void synth_halo(const u32x4 &own, uint32_t (&out)[HB]) {
#pragma unroll
    for (int d = 0; d < HB; ++d) {
        uint32_t r = 0;
#pragma unroll
        for (int D = 0; D < 4; ++D) {
            uint32_t sel = 0;
            bool any = false;
#pragma unroll
            for (int b = 0; b < 4; ++b) {
                const int j = halo_source<SP, H>(RIGHT, MIRROR, 4 * d + b, HB);
                if (j >= 0 && (j >> 2) == D) {
                    sel |= (uint32_t)(j & 3) << (8 * b);
                    any = true;
                } else {
                    sel |= (uint32_t)(4 + b) << (8 * b); // keep what r holds
                }
            }
            if (any) r = __builtin_amdgcn_perm(r, own[D], sel);
        }
        out[d] = r;
    }
}

// border.resolveIndex for a row at most H outside the image, without the general rule's division (rows > 2H is a
// precondition of this kernel): one reflection / one wrap is the whole story there.
__device__ __forceinline__ int resolve_row_near(int y, int rows, int border) {
    if (y >= 0 && y < rows) return y;
    if (border == ZG_BORDER_ZERO) return -1;
    if (border == ZG_BORDER_REPLICATE) return y < 0 ? 0 : rows - 1;
    if (border == ZG_BORDER_MIRROR) return y < 0 ? -y : 2 * rows - 2 - y;
    return y < 0 ? y + rows : y - rows;
}

template <int HB> struct RowIn {
    u32x4 v;        // this lane's sixteen bytes
    uint32_t h[HB]; // lane 0: the 4 HB bytes before the strip's 1024; every other lane: the 4 HB bytes after them
};

// A lane's place in strip `item` of its frame (strips left to right, then down; a strip is a.strip_rows source rows high).
template <int HB> struct StripLane {
    int lx, rb, x0, y0;
    int voff;                    // byte offset of the lane's unit in a row
    int last_lane;               // of the strip: below 63 where the row ends inside it
    int end_lane;                // last_lane then, else no lane (-1)
    bool left_edge, right_edge;  // the strip holds the row's first / last byte
    bool edges;                  // anything but a full strip between two others
    int border;
    int off_h;                   // byte offset of the lane's halo load: always inside the row
    // ends_wrap: at the row's ends the halo load points at the row's other end (what .wrap wants; the other borders are synthesised);
    // else at the row's own end (a kernel that only replicates)
    __device__ __forceinline__ StripLane(const StripArgs &a, uint32_t item, bool ends_wrap = true) {
        const int sy = (int)(item / (uint32_t)a.strips_x), sx = (int)(item - (uint32_t)sy * (uint32_t)a.strips_x);
        lx = (int)threadIdx.x;
        rb = a.row_bytes;
        x0 = sx * 1024;
        y0 = sy * a.strip_rows;
        voff = x0 + 16 * lx;
        last_lane = (min(rb - x0, 1024) >> 4) - 1;
        end_lane = last_lane != 63 ? last_lane : -1;
        left_edge = sx == 0;
        right_edge = x0 + 1024 >= rb;
        edges = left_edge || right_edge || last_lane != 63;
        border = a.border;
        const int off_before = left_edge ? (ends_wrap ? rb - 4 * HB : 0) : x0 - 4 * HB, off_after = right_edge ? (ends_wrap ? 0 : rb - 4 * HB) : x0 + 1024;
        off_h = lx == 0 ? off_before : off_after;
    }
};

// The twelve dwords around a lane's unit of a row of SP-byte pixels: [4 - HB, 4) from the lane below, [4, 8) own, [8, 8 + HB) from
// the lane above; with EDGE the row's end inside the strip and the border rule at the row's two ends.
template <int SP, int H, int HB, bool EDGE> __device__ __forceinline__ void widen_bytes(const StripLane<HB> &L, const RowIn<HB> &r, uint32_t (&q)[12]) {
#pragma unroll
    for (int d = 0; d < 12; ++d) q[d] = 0;
#pragma unroll
    for (int d = 0; d < 4; ++d) q[4 + d] = r.v[d];
#pragma unroll
    for (int d = 0; d < HB; ++d) {
        q[4 - HB + d] = from_lane_below(r.h[d], r.v[4 - HB + d]);
        q[8 + d] = from_lane_above(r.h[d], r.v[d]);
    }
    if constexpr (!EDGE) return; // strips that touch neither end of the rows are done here
    const bool ends_here = L.lx == L.end_lane; // the row ends inside this strip: its last lane has a (zero) neighbour above
#pragma unroll
    for (int d = 0; d < HB; ++d) q[8 + d] = ends_here ? r.h[d] : q[8 + d];
    if (L.left_edge && L.border != ZG_BORDER_WRAP) { // wave-uniform
        uint32_t g[HB];
        if (L.border == ZG_BORDER_MIRROR) synth_halo<SP, H, HB, false, true>(r.v, g);
        else if (L.border == ZG_BORDER_REPLICATE) synth_halo<SP, H, HB, false, false>(r.v, g);
        else {
#pragma unroll
            for (int d = 0; d < HB; ++d) g[d] = 0;
        }
#pragma unroll
        for (int d = 0; d < HB; ++d) q[4 - HB + d] = L.lx == 0 ? g[d] : q[4 - HB + d];
    }
    if (L.right_edge && L.border != ZG_BORDER_WRAP) {
        uint32_t g[HB];
        if (L.border == ZG_BORDER_MIRROR) synth_halo<SP, H, HB, true, true>(r.v, g);
        else if (L.border == ZG_BORDER_REPLICATE) synth_halo<SP, H, HB, true, false>(r.v, g);
        else {
#pragma unroll
            for (int d = 0; d < HB; ++d) g[d] = 0;
        }
#pragma unroll
        for (int d = 0; d < HB; ++d) q[8 + d] = L.lx == L.last_lane ? g[d] : q[8 + d];
    }
}

// Two ways to reach a row. GENERAL: the border rule per row and a descriptor per row whose length clips the lanes past the
// row's end (and is 0 for a row the zero border drops, or a destination row past the last) — a dozen scalar instructions per row,
// which matters: these kernels are bound by instruction issue, scalar instructions included (profiles/r03_stream_kernel.txt).
// FAST, for the strips whose rows — read-ahead included — all lie inside the image (every strip but a frame's first and last): one
// descriptor for the whole frame and a running offset that advances by one addition per row; rows are asked for and written in
// ascending order, from y0 - H and y0 >> RSHIFT. A lane's destination unit is 16 >> DSHIFT bytes; the destination has rows >> RSHIFT rows.
// REPLICATE fixes the border rule of the rows (`border` is not looked at).
template <int HB, int H, bool FAST, int DSHIFT = 0, int RSHIFT = 0, bool REPLICATE = false> struct StripRows {
    const StripArgs &a;
    const StripLane<HB> &L;
    const uint8_t *srcf;
    uint8_t *dstf;
    const int border;
    __amdgpu_buffer_rsrc_t src_all, dst_all;
    uint32_t s_next, d_next; // FAST: byte offset of the next source row to ask for / of the next destination row
    int dvoff;               // byte offset of the lane's unit in a destination row
    // the strip's rows reach H rows above and below it, and at most that far outside the image, where `border` resolves them
    __device__ __forceinline__ StripRows(const StripArgs &a_, const StripLane<HB> &L_, const uint8_t *srcf_, uint8_t *dstf_, int border_)
        : a(a_), L(L_), srcf(srcf_), dstf(dstf_), border(border_),
          src_all(__builtin_amdgcn_make_buffer_rsrc((void *)srcf_, (short)0, (int)a_.src_span, 0x00020000)),
          dst_all(__builtin_amdgcn_make_buffer_rsrc((void *)dstf_, (short)0, (int)a_.dst_span, 0x00020000)),
          s_next((uint32_t)(L_.y0 - H) * (uint32_t)a_.src_pitch), d_next((uint32_t)(L_.y0 >> RSHIFT) * (uint32_t)a_.dst_pitch),
          dvoff(L_.voff >> DSHIFT) {}

    __device__ __forceinline__ RowIn<HB> load(int y) { // source row y
        RowIn<HB> r;
        if constexpr (FAST) { // the row goes into the load's scalar offset
            r.v = __builtin_amdgcn_raw_buffer_load_b128(src_all, L.voff, (int)s_next, 0);
            HaloLoad<HB>::run(src_all, L.off_h, (int)s_next, r.h);
            s_next += (uint32_t)a.src_pitch;
        } else {
            int gr = y;
            uint32_t keep = ~0u; // 0 for a row the zero border drops
            if constexpr (REPLICATE) gr = min(max(y, 0), a.rows - 1);
            else if (y < 0 || y >= a.rows) { // wave-uniform
                gr = resolve_row_near(min(y, a.rows - 1 + H), a.rows, border); // rows past that are read ahead and never used
                keep = gr >= 0 ? ~0u : 0u;
                gr = max(gr, 0);
            }
            const uint8_t *row = srcf + (size_t)(uint32_t)gr * a.src_pitch;
            const auto rsrc = __builtin_amdgcn_make_buffer_rsrc((void *)row, (short)0, (int)((uint32_t)L.rb & keep), 0x00020000);
            r.v = __builtin_amdgcn_raw_buffer_load_b128(rsrc, L.voff, 0, 0);
            HaloLoad<HB>::run(rsrc, L.off_h, 0, r.h);
        }
        return r;
    }
    // One destination row, gy: `o` is the lane's unit. A store of more than 64 bits keeps reading its data registers for a cycle after
    // it issues, and a VALU instruction that overwrites them right behind it corrupts what the last lanes of each 16 write (seen on
    // gfx950: an even row's store came out with dword 0 of the odd row in lanes 12-15, 28-31, ...). hipcc knows the hazard and pads
    // it — except when the store takes its scalar offset from a register, which its rule (inherited from older parts) exempts, wrongly
    // for this one. So a store never puts the row into soffset: FAST adds it to the lane's offset instead (one v_add), and hipcc pads
    // as usual. Loads have no such window and do use soffset.
    template <class Unit> __device__ __forceinline__ void store(Unit o, int gy) {
        if constexpr (FAST) {
            if (L.last_lane == 63) st_unit(o, dst_all, dvoff + (int)d_next);
            else if (L.lx <= L.last_lane) st_unit(o, dst_all, dvoff + (int)d_next); // the frame's descriptor does not clip a row
            d_next += (uint32_t)a.dst_pitch;
        } else {
            const uint32_t row_ok = (uint32_t)gy < (uint32_t)a.rows >> RSHIFT ? ~0u : 0u;
            uint8_t *row = dstf + (size_t)((uint32_t)gy & row_ok) * a.dst_pitch;
            const auto rsrc = __builtin_amdgcn_make_buffer_rsrc((void *)row, (short)0, (int)(((uint32_t)L.rb >> DSHIFT) & row_ok), 0x00020000);
            st_unit(o, rsrc, dvoff); // row bytes % 16 == 0: a unit is all in or all out
        }
    }
};

// What every strip kernel ends with: run(fast, edge) in the one of its three forms this strip needs (wave-uniform).
template <class Run> __device__ __forceinline__ void strip_dispatch(bool fast, bool edges, Run &&run) {
    if (fast && !edges) run(std::true_type{}, std::false_type{}); // nearly every strip of a frame
    else if (fast) run(std::true_type{}, std::true_type{});
    else run(std::false_type{}, std::true_type{});
}

} // namespace zg
