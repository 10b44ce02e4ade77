// shen_castan.hip — Image(T).shenCastan: the detector's own kernels. The grey plane and the hysteresis it shares with canny are
// edges.hip's (canny_gray_plane, run_hysteresis, launch_emit), the ISEF smoothing is isef.hip's (isef_plane).
#include "zg_internal.h"

#include <cmath>
#include <cstdlib>

#pragma clang fp contract(off)

namespace zg {

// ---- Shen-Castan (src/image.zig:1015-1027 -> src/image/edges.zig:83-196) -----------------------------------------------
// grey -> ISEF smoothing (rows, then columns; each a forward and a backward first-order recursion, edges.zig:283-349) ->
// BLI = (smoothed - grey >= 0) -> zero crossings -> adaptive gradient from three integral images (grey, BLI, grey * BLI)
// -> percentile threshold from a 256-bin histogram -> optional NMS -> strong-only emit or hysteresis.
// The recursions and the integral images are sequential f32 chains by contract (the reference's rounding order), one
// chain per row / column: they run as one lane per chain with LDS transposes (rows) or coalesced strided walks (columns),
// latency-bound like boxBlur's SAT. The histogram, its percentile and the thresholds stay on the device (integer atomics
// and a one-workgroup kernel), so nothing but the hysteresis fixed-point test synchronises the stream.

// BLI, grey * BLI and the zero-crossing candidates (edges.zig:111-128, 356-415). FORWARD: east / south / south-east /
// south-west neighbours; otherwise (NMS mode) any 4-neighbour, interior pixels only when the image is at least 3 x 3.
__global__ __launch_bounds__(256) void k_sc_bli(const float *gray, const float *sm, uint8_t *bli, float *gm, uint8_t *cand, int rows, int cols, int forward) {
    const int c = blockIdx.x * 64 + (threadIdx.x & 63), r = blockIdx.y * 4 + (threadIdx.x >> 6);
    if (c >= cols || r >= rows) return;
    auto B = [&](int rr, int cc) -> int { const size_t i = (size_t)rr * cols + cc; return (sm[i] - gray[i]) >= 0 ? 1 : 0; };
    const int ce = B(r, c);
    const size_t idx = (size_t)r * cols + c;
    bli[idx] = (uint8_t)ce;
    gm[idx] = gray[idx] * (float)ce;
    bool mark = false;
    if (forward) {
        if (!mark && c + 1 < cols) mark = ce != B(r, c + 1);
        if (!mark && r + 1 < rows) mark = ce != B(r + 1, c);
        if (!mark && r + 1 < rows && c + 1 < cols) mark = ce != B(r + 1, c + 1);
        if (!mark && r + 1 < rows && c > 0) mark = ce != B(r + 1, c - 1);
    } else if (rows >= 3 && cols >= 3) {
        if (r >= 1 && r < rows - 1 && c >= 1 && c < cols - 1) mark = ce != B(r, c - 1) || ce != B(r, c + 1) || ce != B(r - 1, c) || ce != B(r + 1, c);
    } else {
        if (!mark && c > 0) mark = ce != B(r, c - 1);
        if (!mark && c + 1 < cols) mark = ce != B(r, c + 1);
        if (!mark && r > 0) mark = ce != B(r - 1, c);
        if (!mark && r + 1 < rows) mark = ce != B(r + 1, c);
    }
    cand[idx] = mark ? 255 : 0;
}

constexpr int SC_HIST_COPIES = 64;
constexpr int SC_BLI_ROWS = 16; // rows a wave of k_sc_bli4 walks (+ one above and two below): 8 -> 31.8 us, 16 -> 31.2, 32 -> 49.3 (unrolled: code and registers)
// The same, four pixels per lane (cols % 4 == 0): a lane loads float4s, keeps the BLI of its columns and of the two beside
// them as six bits per row (the neighbours' come over with DPP wave shifts, a workgroup's outer columns with one extra load),
// and the marks of four pixels are a few bitwise operations on the rows above, at and below; dword and float4 stores.
// A wave walks 16 rows, two rows of loads ahead. MODE 0: forward; 1: four-neighbour, interior only; 2: four-neighbour, bounded.
// (The lane-per-pixel kernel evaluates BLI five times per pixel, ten loads: 97 us per 4096^2 frame against 45 us.)
template <int MODE>
__global__ __launch_bounds__(256) void k_sc_bli4(const uint8_t *gray, const float *sm, uint8_t *bli, uint8_t *gm, uint8_t *cand, int rows, int cols, unsigned int *hist_to_clear) { // gray, gm: bytes
    if (blockIdx.x == 0 && blockIdx.y == 0) // the gradient kernel's histogram copies start from zero: cleared here, two launches earlier, instead of by a memset of its own
        for (int i = threadIdx.x; i < SC_HIST_COPIES * 256; i += 256) hist_to_clear[i] = 0;
    constexpr int RW = SC_BLI_ROWS;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int x0 = blockIdx.x * 256 + lane * 4;
    const int y0 = (blockIdx.y * 4 + wave) * RW;
    if (y0 >= rows) return; // wave-uniform
    const bool live = x0 < cols;
    const int xc = live ? x0 : cols - 4;
    const bool is_edge = live && ((lane == 0 && x0 > 0) || (lane == 63 && x0 + 4 < cols));
    const int ecol = lane == 0 ? x0 - 1 : x0 + 4;
    uint32_t mE = 0, mW = 0, mI = 0; // bit j: column x0 + j has an east neighbour / a west neighbour / is interior
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        if (x0 + j + 1 < cols) mE |= 1u << j;
        if (x0 + j > 0) mW |= 1u << j;
        if (x0 + j >= 1 && x0 + j < cols - 1) mI |= 1u << j;
    }
    struct Raw { float4 s, g; float es, eg; uint32_t g8; };
    auto load = [&](int r, Raw &w) { // row clamped into the image: rows outside are masked where they are used
        r = r < 0 ? 0 : (r > rows - 1 ? rows - 1 : r);
        const size_t i = (size_t)r * cols;
        w.s = *(const float4 *)(sm + i + xc);
        const uint32_t g4 = *(const uint32_t *)(gray + i + xc);
        w.g8 = g4;
        w.g = make_float4((float)(g4 & 255u), (float)((g4 >> 8) & 255u), (float)((g4 >> 16) & 255u), (float)(g4 >> 24));
        w.es = 0.0f; w.eg = 0.0f;
        if (is_edge) { w.es = sm[i + ecol]; w.eg = (float)gray[i + ecol]; }
    };
    auto ext_of = [&](const Raw &w) -> uint32_t { // bit k: BLI of column x0 - 1 + k
        const uint32_t nib = ((w.s.x - w.g.x) >= 0 ? 1u : 0u) | ((w.s.y - w.g.y) >= 0 ? 2u : 0u) | ((w.s.z - w.g.z) >= 0 ? 4u : 0u) | ((w.s.w - w.g.w) >= 0 ? 8u : 0u);
        const uint32_t e = (w.es - w.eg) >= 0 ? 1u : 0u;
        uint32_t left = ((uint32_t)__builtin_amdgcn_update_dpp(0, (int)nib, 0x138, 0xf, 0xf, true) >> 3) & 1u; // wave_shr:1: lane - 1
        uint32_t right = (uint32_t)__builtin_amdgcn_update_dpp(0, (int)nib, 0x130, 0xf, 0xf, true) & 1u;      // wave_shl:1: lane + 1
        if (lane == 0) left = e;
        if (lane == 63) right = e;
        return left | (nib << 1) | (right << 5);
    };
    Raw q0, q1;
    load(y0 - 1, q0);
    load(y0, q1);
    uint32_t ext_n = ext_of(q0), ext_c = ext_of(q1);
    uint32_t g_c = q1.g8;
    load(y0 + 1, q0);
    load(y0 + 2, q1);
#pragma unroll
    for (int k = 0; k < RW; ++k) {
        const int r = y0 + k;
        if (r >= rows) break; // wave-uniform
        Raw &cur = (k & 1) ? q1 : q0; // row r + 1
        const uint32_t ext_s = ext_of(cur);
        const uint32_t g_s = cur.g8;
        load(r + 3, cur);
        const uint32_t C = (ext_c >> 1) & 15u, Eb = (ext_c >> 2) & 15u, Wb = ext_c & 15u;
        const uint32_t Sb = (ext_s >> 1) & 15u, Nb = (ext_n >> 1) & 15u;
        const uint32_t vS = r + 1 < rows ? 15u : 0u, vN = r > 0 ? 15u : 0u;
        uint32_t mark;
        if (MODE == 0) {
            const uint32_t SEb = (ext_s >> 2) & 15u, SWb = ext_s & 15u;
            mark = ((C ^ Eb) & mE) | (((C ^ Sb) | ((C ^ SEb) & mE) | ((C ^ SWb) & mW)) & vS);
        } else if (MODE == 1) {
            mark = ((C ^ Wb) | (C ^ Eb) | (C ^ Nb) | (C ^ Sb)) & mI & (vS & vN);
        } else {
            mark = ((C ^ Wb) & mW) | ((C ^ Eb) & mE) | ((C ^ Nb) & vN) | ((C ^ Sb) & vS);
        }
        if (live) {
            const size_t i = (size_t)r * cols + x0;
            const uint32_t cb = (C * 0x00204081u) & 0x01010101u; // bit j -> byte j
            *(uint32_t *)(bli + i) = cb;
            *(uint32_t *)(cand + i) = ((mark * 0x00204081u) & 0x01010101u) * 255u;
            *(uint32_t *)(gm + i) = g_c & (cb * 255u); // grey * BLI
        }
        ext_n = ext_c;
        ext_c = ext_s;
        g_c = g_s;
    }
}

// adaptive gradient at the candidates (edges.zig:462-496) + the histogram of its rounded values (:139-150)
// BUF: the planes are below 4 GiB, so a corner read is a buffer load (scalar row offset + per-lane column offset: no vector
// address arithmetic at all; with 64-bit pointers a third of the kernel's instructions computed addresses).
// CNT: sat_m is not an integral image but the window's count itself, one byte per pixel (k_sc_count below): one byte load per pixel instead of four
// corner loads, and one integral image fewer to build.
template <bool BUF, bool CNT = false>
__global__ __launch_bounds__(256) void k_sc_gradient(const uint8_t *cand, const float *sat_g, const float *sat_m, const float *sat_gm, float *grad,
                                                     unsigned int *hist, int rows, int cols, int hw) {
    // sixteen copies of the block histogram: neighbouring pixels have similar gradients, and 64 lanes hitting one LDS counter
    // serialise (measured 1086 us per 4096^2 frame of noise with a single copy)
    __shared__ unsigned int lh[16][256];
#pragma unroll
    for (int k = 0; k < 16; ++k) lh[k][threadIdx.x] = 0;
    __syncthreads();
    // a workgroup covers 64 columns x 64 rows (sixteen steps of four rows), so the 256 global histogram updates it ends
    // with are amortised over 4096 pixels (one update per 4-row block serialised 16.7 M atomics on 256 counters: 1.09 ms).
    // The kernel is latency-bound (one step at a time, the corner reads behind two branches: 150 us per 4096^2 frame), so the
    // sixteen candidate bytes of a thread are read first and the steps go four at a time, the 48 corner reads of a group
    // issued before anything is computed. The loads of a wave row are whole cache lines whichever lanes want them, so they are not
    // predicated on the candidate bit, only skipped when no lane of the wave has a candidate in the group.
    const int c = blockIdx.x * 64 + (threadIdx.x & 63), cc = min(c, cols - 1);
    const int wrow = blockIdx.y * 64 + __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6)); // a wave is one row: row arithmetic is scalar
    const int c1 = cc > hw ? cc - hw : 0, c2 = min(cc + hw, cols - 1);
    const int cl = c1 > 0 ? c1 - 1 : 0; // column of the two left-hand corners (read anyway, dropped when c1 == 0)
    const float *const planes[3] = {sat_m, sat_gm, sat_g};
    const uint32_t oc2 = (uint32_t)c2 * 4u, ocl = (uint32_t)cl * 4u;
    const uint32_t plane_bytes = BUF ? (uint32_t)((size_t)rows * cols * 4) : 0u;
    uint8_t cb[16];
    [[maybe_unused]] uint8_t cnt[16];
#pragma unroll
    for (int st = 0; st < 16; ++st) {
        cb[st] = cand[(size_t)min(wrow + st * 4, rows - 1) * cols + cc];
        if constexpr (CNT) cnt[st] = ((const uint8_t *)sat_m)[(size_t)min(wrow + st * 4, rows - 1) * cols + cc];
    }
    // out-of-range buffer offsets read as zero: the corners that do not exist (c1 == 0, r1 == 0) need no select afterwards
    constexpr uint32_t OOR = 0xfffffff0u;
    const uint32_t ocl_z = c1 > 0 ? ocl : OOR;
    constexpr int U = CNT ? 4 : 2, NG = 16 / U; // steps per group (two groups in flight): the counted form has the registers for four
    struct Group { float v[U][12]; };
    auto issue = [&](int grp, Group &g) { // the 24 corner reads of steps grp * U .. + U
        bool some = false;
#pragma unroll
        for (int u = 0; u < U; ++u) some = some || (c < cols && wrow + (grp * U + u) * 4 < rows && cb[grp * U + u] != 0);
        if (__ballot(some) != 0) { // wave-uniform
#pragma unroll
            for (int u = 0; u < U; ++u) {
                const int r = min(wrow + (grp * U + u) * 4, rows - 1);
                const int r1 = r > hw ? r - hw : 0, r2 = min(r + hw, rows - 1);
                const size_t bot = (size_t)r2 * cols, top = (size_t)(r1 > 0 ? r1 - 1 : 0) * cols;
#pragma unroll
                for (int p = CNT ? 1 : 0; p < 3; ++p) {
                    if constexpr (BUF) {
                        const auto rsrc = __builtin_amdgcn_make_buffer_rsrc((void *)planes[p], (short)0, (int)plane_bytes, 0x00020000);
                        // readfirstlane: the row offsets are wave-uniform, and saying so spares a waterfall loop around every load
                        const int sb = __builtin_amdgcn_readfirstlane((int)(uint32_t)(bot * 4)), stp = __builtin_amdgcn_readfirstlane((int)(uint32_t)(top * 4));
                        const uint32_t t2 = r1 > 0 ? oc2 : OOR, tl = r1 > 0 ? ocl_z : OOR;
                        g.v[u][p * 4 + 0] = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(rsrc, (int)oc2, sb, 0));
                        g.v[u][p * 4 + 1] = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(rsrc, (int)ocl_z, sb, 0));
                        g.v[u][p * 4 + 2] = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(rsrc, (int)t2, stp, 0));
                        g.v[u][p * 4 + 3] = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(rsrc, (int)tl, stp, 0));
                    } else {
                        g.v[u][p * 4 + 0] = planes[p][bot + c2];
                        g.v[u][p * 4 + 1] = c1 > 0 ? planes[p][bot + cl] : 0.0f;
                        g.v[u][p * 4 + 2] = r1 > 0 ? planes[p][top + c2] : 0.0f;
                        g.v[u][p * 4 + 3] = (r1 > 0 && c1 > 0) ? planes[p][top + cl] : 0.0f;
                    }
                }
            }
        } else {
#pragma unroll
            for (int u = 0; u < U; ++u)
#pragma unroll
                for (int k = 0; k < 12; ++k) g.v[u][k] = 0.0f;
        }
    };
    auto finish = [&](int grp, const Group &g) {
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const int r = wrow + (grp * U + u) * 4;
            if (c >= cols || r >= rows) continue;
            float gr = 0.0f;
            if (cb[grp * U + u] != 0) {
                const int r1 = r > hw ? r - hw : 0, r2 = min(r + hw, rows - 1);
                const float area = (float)((size_t)(r2 - r1 + 1) * (size_t)(c2 - c1 + 1));
                float sum[3];
#pragma unroll
                for (int p = CNT ? 1 : 0; p < 3; ++p) sum[p] = ((g.v[u][p * 4 + 0] - g.v[u][p * 4 + 1]) - g.v[u][p * 4 + 2]) + g.v[u][p * 4 + 3]; // integral.zig:85-90, in that order
                if constexpr (CNT) sum[0] = (float)cnt[grp * U + u];
                const float count1 = sum[0], count0 = area - count1;
                if (count0 > 0 && count1 > 0) {
                    const float sum1 = sum[1], sum_total = sum[2];
                    const float sum0 = sum_total - sum1;
                    const float mean0 = sum0 / count0, mean1 = sum1 / count1;
                    gr = fabsf(mean1 - mean0);
                }
                float hgv = gr;
                if (hgv < 0) hgv = 0;
                if (hgv > 255) hgv = 255;
                atomicAdd(&lh[threadIdx.x & 15][(int)roundf(hgv)], 1u);
            }
            grad[(size_t)r * cols + c] = gr;
        }
    };
    Group ga, gb; // two groups in flight: the reads of the next one are out before this one is computed
    issue(0, ga);
#pragma unroll
    for (int grp = 0; grp < NG; grp += 2) {
        issue(grp + 1, gb);
        finish(grp, ga);
        if (grp + 2 < NG) issue(grp + 2, ga);
        finish(grp + 1, gb);
    }
    __syncthreads();
    unsigned int total = 0;
#pragma unroll
    for (int k = 0; k < 16; ++k) total += lh[k][threadIdx.x];
    // SC_HIST_COPIES copies of the frame histogram, picked by workgroup: 4096 workgroups adding into one set of 256 counters queued
    // up at the L2 atomic units (about half of this kernel's time on a 4096^2 frame); k_sc_thresholds sums the copies
    if (total) atomicAdd(&hist[((blockIdx.y * gridDim.x + blockIdx.x) % SC_HIST_COPIES) * 256 + threadIdx.x], total);
}
// The number of BLI pixels in each pixel's clipped (2 hw + 1)^2 window, as a byte (hw <= 7: at most 225). The reference takes it from the integral
// image of the mask, ((A - B) - C) + D (integral.zig:85-90): on frames of at most 2^24 pixels every value of that image is an integer f32 holds
// exactly, so the four-corner expression IS the count — computed here directly (two 1-D sums through LDS), which spares the detector one of its
// three integral images (a third of k_sat_chain_planes' stores) and k_sc_gradient four of its twelve corner loads per pixel.
__global__ __launch_bounds__(256) void k_sc_count(const uint8_t *bli, uint8_t *cnt, int rows, int cols, int hw) {
    constexpr int TW = 64, TH = 32, HMAX = 7;
    __shared__ uint8_t in[TH + 2 * HMAX][TW + 2 * HMAX + 2];
    __shared__ uint8_t hs[TH + 2 * HMAX][TW];
    const int t = threadIdx.x, x0 = blockIdx.x * TW, y0 = blockIdx.y * TH;
    const int nr = TH + 2 * hw, nc = TW + 2 * hw;
    for (int i = t; i < nr * nc; i += 256) {
        const int rr = i / nc, cc = i - rr * nc, gy = y0 - hw + rr, gx = x0 - hw + cc;
        in[rr][cc] = (gy >= 0 && gy < rows && gx >= 0 && gx < cols) ? bli[(size_t)gy * cols + gx] : 0; // outside the frame: not in any clipped window
    }
    __syncthreads();
    for (int i = t; i < nr * TW; i += 256) {
        const int rr = i >> 6, cc = i & 63;
        int sum = 0;
        for (int k = 0; k <= 2 * hw; ++k) sum += in[rr][cc + k];
        hs[rr][cc] = (uint8_t)sum;
    }
    __syncthreads();
    for (int i = t; i < TH * TW; i += 256) {
        const int rr = i >> 6, cc = i & 63;
        int sum = 0;
        for (int k = 0; k <= 2 * hw; ++k) sum += hs[rr + k][cc];
        if (y0 + rr < rows && x0 + cc < cols) cnt[(size_t)(y0 + rr) * cols + x0 + cc] = (uint8_t)sum;
    }
}

// The same for windows up to 7 x 7 (cols % 4 == 0), streaming: a lane owns four adjacent columns as the bytes of a dword and walks down a 32-row
// segment. The horizontal sums of its four pixels are 2 HW + 1 byte-shifted copies of { left neighbour's dword, its own, right neighbour's } added
// as packed bytes (sums <= 7: no carry between bytes; the neighbours' dwords come over with DPP wave shifts, a wave's outer lanes fetch theirs);
// the vertical sum is a running packed sum over a ring of 2 HW + 1 rows (<= 49 per byte). One dword in, one dword out per four pixels.
constexpr int SC_COUNT_SEG = 32; // rows a wave walks (+ 2 HW of run-in)
template <int HW>
__global__ __launch_bounds__(256) void k_sc_count_stream(const uint8_t *bli, uint8_t *cnt, int rows, int cols) {
    constexpr int N = 2 * HW + 1, SEG = SC_COUNT_SEG;
    const int lane = threadIdx.x & 63, strip = (int)blockIdx.x * 4 + (int)(threadIdx.x >> 6);
    const int x0 = strip * 256 + lane * 4;
    if (strip * 256 >= cols) return; // wave-uniform
    const bool live = x0 < cols;
    const int y0 = (int)blockIdx.y * SEG, y1 = min(y0 + SEG, rows);
    const int ex = lane == 0 ? x0 - 4 : x0 + 4; // the dword beside the wave's columns that this lane fetches if it is an outer lane
    const bool outer = (lane == 0 || lane == 63) && ex >= 0 && ex < cols;
    uint32_t ring[N];
#pragma unroll
    for (int k = 0; k < N; ++k) ring[k] = 0;
    uint32_t v = 0;
    for (int rb = y0 - HW; rb < y1 + HW; rb += N) {
        uint32_t curs[N], sides[N]; // a ring's worth of rows asked for together: the walk is one memory round trip per N rows, not per row
#pragma unroll
        for (int j = 0; j < N; ++j) {
            const int r = rb + j;
            curs[j] = sides[j] = 0;
            if (r >= 0 && r < rows && r < y1 + HW) {
                if (live) curs[j] = *(const uint32_t *)(bli + (size_t)r * cols + x0);
                if (outer) sides[j] = *(const uint32_t *)(bli + (size_t)r * cols + ex);
            }
        }
#pragma unroll
        for (int j = 0; j < N; ++j) { // row rb + j goes into ring slot j: (rb - (y0 - HW)) is a multiple of N
            const int r = rb + j;
            const uint32_t cur = curs[j];
            uint32_t prev = (uint32_t)__builtin_amdgcn_update_dpp(0, (int)cur, 0x138, 0xf, 0xf, true); // wave_shr:1: lane - 1's dword
            uint32_t next = (uint32_t)__builtin_amdgcn_update_dpp(0, (int)cur, 0x130, 0xf, 0xf, true); // wave_shl:1: lane + 1's
            if (lane == 0) prev = sides[j];
            if (lane == 63) next = sides[j];
            uint32_t h = cur;
#pragma unroll
            for (int k = 1; k <= HW; ++k) h += __builtin_amdgcn_alignbyte(next, cur, k) + __builtin_amdgcn_alignbyte(cur, prev, 4 - k);
            v += h - ring[j]; // the row 2 HW + 1 above leaves the window, per byte: it was in the sum, so no borrow
            ring[j] = h;
            const int ro = r - HW; // the row whose window is now complete
            if (ro >= y0 && ro < y1 && live) *(uint32_t *)(cnt + (size_t)ro * cols + x0) = v;
        }
    }
}

// thr[0] = t_high, thr[1] = t_low (edges.zig:160-166): the reference walks the histogram until the running count reaches
// floor(total * high_ratio); the number of steps it takes is the number of bins whose EXCLUSIVE prefix is below that target.
// One workgroup of 256 threads, a bin each (a single thread walking 256 global loads took 12 us).
__global__ __launch_bounds__(256) void k_sc_thresholds(const unsigned int *hist, float *thr, float high_ratio, float low_rel) {
    __shared__ unsigned int wtot[4], below[4];
    const int t = threadIdx.x, lane = t & 63, w = t >> 6;
    unsigned int h = 0;
#pragma unroll 8
    for (int k = 0; k < SC_HIST_COPIES; ++k) h += hist[k * 256 + t];
    unsigned int y = h; // inclusive scan over the wave (counts sum to the pixel count, below 2^31)
    y += (unsigned int)__builtin_amdgcn_update_dpp(0, (int)y, 0x111, 0xf, 0xf, true);
    y += (unsigned int)__builtin_amdgcn_update_dpp(0, (int)y, 0x112, 0xf, 0xf, true);
    y += (unsigned int)__builtin_amdgcn_update_dpp(0, (int)y, 0x114, 0xf, 0xf, true);
    y += (unsigned int)__builtin_amdgcn_update_dpp(0, (int)y, 0x118, 0xf, 0xf, true);
    y += (unsigned int)__builtin_amdgcn_update_dpp(0, (int)y, 0x142, 0xa, 0xf, false);
    y += (unsigned int)__builtin_amdgcn_update_dpp(0, (int)y, 0x143, 0xc, 0xf, false);
    if (lane == 63) wtot[w] = y;
    __syncthreads();
    unsigned int before = 0;
    for (int k = 0; k < w; ++k) before += wtot[k];
    const unsigned long long total = (unsigned long long)wtot[0] + wtot[1] + wtot[2] + wtot[3];
    const unsigned long long target = (unsigned long long)floorf((float)total * high_ratio);
    const unsigned long long excl = (unsigned long long)before + (y - h);
    const unsigned long long m = __ballot(excl < target);
    if (lane == 0) below[w] = (unsigned int)__popcll(m);
    __syncthreads();
    if (t == 0) {
        const int idx = (int)(below[0] + below[1] + below[2] + below[3]);
        const float t_high = (float)min(idx, 255);
        thr[0] = t_high;
        thr[1] = low_rel * t_high;
    }
}
// NMS on central differences of the smoothed plane (edges.zig:582-661)
__global__ __launch_bounds__(256) void k_sc_nms(const float *sm, const float *grad, const uint8_t *cand, uint8_t *out, int rows, int cols) {
    const int c = blockIdx.x * 64 + (threadIdx.x & 63), r = blockIdx.y * 4 + (threadIdx.x >> 6);
    if (c >= cols || r >= rows) return;
    const size_t idx = (size_t)r * cols + c;
    uint8_t keep = 0;
    if (rows >= 3 && cols >= 3 && r >= 1 && r < rows - 1 && c >= 1 && c < cols - 1 && cand[idx] != 0) {
        const float K = 0.414213562f;
        const float gx = 0.5f * (sm[idx + 1] - sm[idx - 1]), gy = 0.5f * (sm[idx + cols] - sm[idx - cols]);
        const float ax = fabsf(gx), ay = fabsf(gy);
        int dr1, dc1, dr2, dc2;
        if (ay <= K * ax) { dr1 = 0; dc1 = -1; dr2 = 0; dc2 = 1; }
        else if (ax <= K * ay) { dr1 = -1; dc1 = 0; dr2 = 1; dc2 = 0; }
        else if (gx * gy > 0) { dr1 = -1; dc1 = 1; dr2 = 1; dc2 = -1; }
        else { dr1 = -1; dc1 = -1; dr2 = 1; dc2 = 1; }
        const float m = grad[idx], n1 = grad[(size_t)(r + dr1) * cols + (c + dc1)], n2 = grad[(size_t)(r + dr2) * cols + (c + dc2)];
        if (m >= n1 && m >= n2) keep = 255;
    }
    out[idx] = keep;
}
// 0 none / 1 weak / 2 strong against the device-resident thresholds; without hysteresis only strong survives. Flat planes,
// four pixels per lane (dword / float4 accesses; the planes start 16 bytes aligned).
__global__ __launch_bounds__(256) void k_sc_classify4(const uint8_t *cand, const float *grad, const float *thr, uint8_t *state, size_t n, int hysteresis) {
    const size_t i = ((size_t)blockIdx.x * 256 + threadIdx.x) * 4;
    if (i >= n) return;
    const float hi = thr[0], lo = thr[1];
    if (i + 4 <= n) {
        const uint32_t c = *(const uint32_t *)(cand + i);
        const float4 g = *(const float4 *)(grad + i);
        const float e[4] = {g.x, g.y, g.z, g.w};
        uint32_t out = 0;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            uint32_t st = 0;
            if ((c >> (8 * j)) & 0xffu) st = e[j] >= hi ? 2u : ((hysteresis && e[j] >= lo) ? 1u : 0u);
            out |= st << (8 * j);
        }
        *(uint32_t *)(state + i) = out;
    } else {
        for (size_t k = i; k < n; ++k) {
            uint8_t st = 0;
            if (cand[k] != 0) st = grad[k] >= hi ? 2 : ((hysteresis && grad[k] >= lo) ? 1 : 0);
            state[k] = st;
        }
    }
}

static int shen_castan_impl(const zg_image *src, const zg_image *dst, float smooth, uint32_t window_size, float high_ratio, float low_rel, int hysteresis,
                            int use_nms, zg_stream stream) {
    hipStream_t s = as_stream(stream);
    int rc;
    if ((rc = check_image(src, "src")) || (rc = check_image(dst, "dst"))) return rc;
    ZG_REQUIRE(src->rows == dst->rows && src->cols == dst->cols, ZG_ERR_DIMENSION_MISMATCH, "shenCastan: %ux%u vs %ux%u", src->rows, src->cols,
               dst->rows, dst->cols);
    ZG_REQUIRE(dst->pixel == ZG_PIXEL_U8, ZG_ERR_INVALID_ARGUMENT, "shenCastan: the output is Image(u8)");
    ZG_REQUIRE(smooth > 0 && smooth < 1, ZG_ERR_INVALID_ARGUMENT, "shenCastan: InvalidBParameter (smooth %g not in (0, 1))", (double)smooth);
    ZG_REQUIRE(window_size % 2 == 1, ZG_ERR_INVALID_ARGUMENT, "shenCastan: WindowSizeMustBeOdd (%u)", window_size);
    ZG_REQUIRE(window_size >= 3, ZG_ERR_INVALID_ARGUMENT, "shenCastan: WindowSizeTooSmall (%u)", window_size);
    ZG_REQUIRE(high_ratio > 0 && high_ratio < 1 && low_rel > 0 && low_rel < 1, ZG_ERR_INVALID_ARGUMENT, "shenCastan: InvalidThreshold (high_ratio %g, low_rel %g)",
               (double)high_ratio, (double)low_rel);
    if (src->rows == 0 || src->cols == 0) return ZG_OK;
    const uint32_t rows = src->rows, cols = src->cols;
    const size_t n = (size_t)rows * cols, nf = (n + 3) / 4 * 4;
    ZG_REQUIRE(!hysteresis || n <= 0x7fffffffu, ZG_ERR_UNSUPPORTED, "shenCastan: hysteresis labels are 32-bit (rows * cols must stay below 2^31)"); // as in canny_impl

    // scratch: f32 planes grey | smoothed | temp (ISEF) then grey*BLI | gradient | three SATs; u8 planes BLI | candidates | NMS | state;
    // histogram (256) | thresholds (2) | hysteresis work
    ScratchBlock block(s);
    const size_t f32_bytes = 7 * nf * sizeof(float), u8_off = f32_bytes, small_off = (u8_off + 6 * nf + 255) / 256 * 256;
    constexpr size_t small_bytes = SC_HIST_COPIES * 256 * sizeof(unsigned int) + 256; // histogram copies | thresholds
    const size_t check_off = (small_off + small_bytes + hysteresis_work_bytes(rows, cols) + 255) / 256 * 256; // the segmented ISEF's check words
    if ((rc = block.alloc(check_off + isef_check_bytes(rows, cols)))) return rc;
    char *scratch = block.p;
    float *gray = (float *)scratch, *sm = gray + nf, *temp = sm + nf, *grad = temp + nf, *sat_g = grad + nf, *sat_m = sat_g + nf, *sat_gm = sat_m + nf;
    uint8_t *bli = (uint8_t *)(scratch + u8_off), *cand = bli + nf, *nms = cand + nf, *state = nms + nf, *gray8 = state + nf, *gm8 = gray8 + nf;
    unsigned int *hist = (unsigned int *)(scratch + small_off);
    float *thr = (float *)(hist + SC_HIST_COPIES * 256);
    char *work = scratch + small_off + small_bytes;
    // Rows of whole dwords: grey and grey * BLI (integers 0 .. 255) also live as BYTES, and that is what the BLI kernel and the three integral
    // images read — a quarter of the f32 planes' traffic (the recursions keep the f32 plane).
    const bool bytes = cols % 4 == 0;
    const bool gray_f32 = !(bytes && isef_2d_applies(rows, cols)); // nothing reads the f32 grey when the recursions take the bytes too

    rc = canny_gray_plane(src, gray_f32 ? gray : nullptr, bytes ? gray8 : nullptr, s);
    const dim3 g64(ceil_div(cols, 64), ceil_div(rows, 4));
    if (rc == ZG_OK) {
        // the recursions in segments along the rows and then the columns (isef.hip); planes whose rows are not whole 16-byte chunks take round 3's
        // route: transpose, column recursions on the cols x rows plane (in place on `grad`, `sat_g` between the passes: both are free until
        // the gradient stage), transpose back into `sm`, then the columns proper
        isef_plane(gray_f32 ? gray : nullptr, bytes ? gray8 : nullptr, sm, temp, grad, sat_g, (uint32_t *)(scratch + check_off), rows, cols, smooth, s);
        if (cols % 4 == 0) { // four pixels per lane (the planes start 16 bytes aligned)
            const dim3 g4(ceil_div(cols, 256), ceil_div(rows, 4u * SC_BLI_ROWS));
            if (!use_nms) hipLaunchKernelGGL(k_sc_bli4<0>, g4, dim3(256), 0, s, (const uint8_t *)gray8, (const float *)sm, bli, gm8 /* grey * BLI */, cand, (int)rows, (int)cols, hist);
            else if (rows >= 3 && cols >= 3) hipLaunchKernelGGL(k_sc_bli4<1>, g4, dim3(256), 0, s, (const uint8_t *)gray8, (const float *)sm, bli, gm8, cand, (int)rows, (int)cols, hist);
            else hipLaunchKernelGGL(k_sc_bli4<2>, g4, dim3(256), 0, s, (const uint8_t *)gray8, (const float *)sm, bli, gm8, cand, (int)rows, (int)cols, hist);
        } else {
            hipLaunchKernelGGL(k_sc_bli, g64, dim3(256), 0, s, (const float *)gray, (const float *)sm, bli, temp /* grey * BLI */, cand, (int)rows, (int)cols, use_nms ? 0 : 1);
        }
        rc = launch_ok("k_sc_bli");
    }
    // frames of at most 2^24 pixels, windows up to 15 x 15: the mask's window count is exact in the reference's f32 integral image, so it is
    // counted directly (k_sc_count) and only grey and grey * BLI go through integral images
    static const bool three_sats = getenv("ZIGNAL_HIP_SC_THREE_SATS") != nullptr; // tuning hook: the mask's integral image as well
    const bool counted = bytes && !three_sats && n <= ((size_t)1 << 24) && window_size / 2 <= 7 && n < (1u << 30);
    uint8_t *cnt8 = (uint8_t *)sat_m; // the plane the mask's integral image would take
    if (rc == ZG_OK) {
        const zg_image gi{bytes ? (void *)gray8 : (void *)gray, cols, rows, cols, bytes ? ZG_PIXEL_U8 : ZG_PIXEL_F32}, mi{bli, cols, rows, cols, ZG_PIXEL_U8},
            gmi{bytes ? (void *)gm8 : (void *)temp, cols, rows, cols, bytes ? ZG_PIXEL_U8 : ZG_PIXEL_F32};
        // grey is as(f32, u8), BLI is 0 / 1, grey * BLI is their product: integer-valued planes, exact row sums
        if (counted) {
            const zg_image *srcs[2] = {&gi, &gmi};
            float *sats[2] = {sat_g, sat_gm};
            rc = sat_planes_multi(srcs, sats, 2, s);
            const dim3 gs(ceil_div(cols, 1024), ceil_div(rows, (uint32_t)SC_COUNT_SEG));
            switch (window_size / 2) { // cols % 4 == 0 here
            case 1: hipLaunchKernelGGL(k_sc_count_stream<1>, gs, dim3(256), 0, s, (const uint8_t *)bli, cnt8, (int)rows, (int)cols); break;
            case 2: hipLaunchKernelGGL(k_sc_count_stream<2>, gs, dim3(256), 0, s, (const uint8_t *)bli, cnt8, (int)rows, (int)cols); break;
            case 3: hipLaunchKernelGGL(k_sc_count_stream<3>, gs, dim3(256), 0, s, (const uint8_t *)bli, cnt8, (int)rows, (int)cols); break;
            default: hipLaunchKernelGGL(k_sc_count, dim3(ceil_div(cols, 64), ceil_div(rows, 32)), dim3(256), 0, s, (const uint8_t *)bli, cnt8, (int)rows, (int)cols, (int)(window_size / 2));
            }
        } else {
            const zg_image *srcs[3] = {&gi, &mi, &gmi};
            float *sats[3] = {sat_g, sat_m, sat_gm};
            rc = sat_planes_multi(srcs, sats, 3, s);
        }
    }
    if (rc == ZG_OK) {
        if (!bytes) rc = fill_async(hist, 0, SC_HIST_COPIES * 256 * sizeof(unsigned int), s); // (k_sc_bli4 cleared it otherwise)
        if (counted)
            hipLaunchKernelGGL((k_sc_gradient<true, true>), dim3(ceil_div(cols, 64), ceil_div(rows, 64)), dim3(256), 0, s, (const uint8_t *)cand, (const float *)sat_g, (const float *)cnt8, (const float *)sat_gm, grad, hist,
                               (int)rows, (int)cols, (int)(window_size / 2));
        else if (n < (1u << 30))
            hipLaunchKernelGGL(k_sc_gradient<true>, dim3(ceil_div(cols, 64), ceil_div(rows, 64)), dim3(256), 0, s, (const uint8_t *)cand, (const float *)sat_g, (const float *)sat_m, (const float *)sat_gm, grad, hist,
                               (int)rows, (int)cols, (int)(window_size / 2));
        else
            hipLaunchKernelGGL(k_sc_gradient<false>, dim3(ceil_div(cols, 64), ceil_div(rows, 64)), dim3(256), 0, s, (const uint8_t *)cand, (const float *)sat_g, (const float *)sat_m, (const float *)sat_gm, grad, hist,
                               (int)rows, (int)cols, (int)(window_size / 2));
        hipLaunchKernelGGL(k_sc_thresholds, dim3(1), dim3(256), 0, s, (const unsigned int *)hist, thr, high_ratio, low_rel);
        const uint8_t *final_cand = cand;
        if (use_nms) {
            hipLaunchKernelGGL(k_sc_nms, g64, dim3(256), 0, s, (const float *)sm, (const float *)grad, (const uint8_t *)cand, nms, (int)rows, (int)cols);
            final_cand = nms;
        }
        hipLaunchKernelGGL(k_sc_classify4, dim3((unsigned)((n + 1023) / 1024)), dim3(256), 0, s, final_cand, (const float *)grad, (const float *)thr, state, n, hysteresis ? 1 : 0);
        if (const int e = launch_ok("k_sc_classify4")) rc = e; // a failed fill_async above stays reported
    }
    if (rc == ZG_OK) rc = hysteresis ? run_hysteresis(state, rows, cols, work, dst, s, "shenCastan") : launch_emit(state, nullptr, nullptr, dst, s);
    return rc;
}

} // namespace zg

using namespace zg;

extern "C" {

int zg_shen_castan(const zg_image *src, const zg_image *dst, float smooth, uint32_t window_size, float high_ratio, float low_rel, int hysteresis,
                   int use_nms, zg_stream stream) {
    return shen_castan_impl(src, dst, smooth, window_size, high_ratio, low_rel, hysteresis, use_nms, stream);
}

int zg_shen_castan_host(const zg_image *src, const zg_image *dst, float smooth, uint32_t window_size, float high_ratio, float low_rel, int hysteresis,
                        int use_nms) {
    return host_src_dst(src, dst, [&](const zg_image *a, const zg_image *b) { return shen_castan_impl(a, b, smooth, window_size, high_ratio, low_rel, hysteresis, use_nms, nullptr); });
}

} // extern "C"
