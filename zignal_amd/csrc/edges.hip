// edges.hip — Image(T).sobel as ONE kernel and Image(T).canny, with the grey plane and the hysteresis that
// shen_castan.hip shares with canny (canny_gray_plane, run_hysteresis, launch_emit: zg_internal.h).
//
// Replaces reference src/image.zig:1001-1010 -> src/image/edges.zig:33-70: grey f32 plane (as(f32, convertColor(u8, px)),
// scalar f32 input used as is) -> convolve(sobel_x, .replicate) and convolve(sobel_y, .replicate) in f32 (ky-major, every
// tap including the zero ones, separate mul and add: src/image/convolution.zig:158-169) -> sqrt(gx^2 + gy^2) / 4 ->
// @trunc(@max(0, @min(255, .))). The reference materialises three full f32 planes; here a workgroup stages the grey values
// of its 64 x 4 tile plus a one-pixel replicate halo in LDS and writes only the u8 result: traffic = source once + 1 B/px.
#include "zg_internal.h"
#include "zg_hostmath.h"
#include "zg_unionfind.h"

#include <cmath>
#include <vector>

#pragma clang fp contract(off)

namespace zg {

__device__ inline float gray_as_f32(uint8_t v) { return (float)v; }

template <int PIX> __device__ inline float sobel_gray(typename Px<PIX>::Vec v) {
    using P = Px<PIX>;
    if constexpr (PIX == ZG_PIXEL_F32) return v[0];
    else if constexpr (PIX == ZG_PIXEL_U8) return (float)v[0];
    else if constexpr (!std::is_same<typename P::Elem, float>::value) { // Rgb(u8) / Rgba(u8): BT.709 16.16 fixed point (color.zig:1031-1042)
        const int y = (13933 * (int)v[0] + 46871 * (int)v[1] + 4732 * (int)v[2] + 32768) >> 16;
        return (float)(y < 0 ? 0 : (y > 255 ? 255 : y));
    } else { // Rgb(f32) / Rgba(f32): clamp(dot, 0, 1) then .as(u8) = @round(255 * clamp) (color.zig:1043-1046, :528-546)
        float y = 0.2126f * v[0] + 0.7152f * v[1] + 0.0722f * v[2];
        y = y != y ? 1.0f : (y < 0.0f ? 0.0f : (y > 1.0f ? 1.0f : y)); // std.math.clamp = @max(0, @min(y, 1)): a NaN clamps to 1
        const float s = 255.0f * y;
        return (float)(int)roundf(s);
    }
}

// Sobel sums of a 3 x 3 window in the reference's term order (edges.zig:255-262 / image.zig sobel): the zero weights are skipped
// and the +-1 / +-2 weights folded into additions; the products are exact, so only the sign of a zero can differ.
// ANY_F32: the grey values are an Image(f32)'s own pixels and may be infinite or NaN. convolution.zig:158-169 multiplies every tap, the
// zero ones too, so an infinity under a zero weight makes the sum NaN (and the byte 255): the three zero products of each sum are kept,
// in the reference's place. Grey values that came from bytes are finite, and a finite value times zero changes no sum.
template <bool ANY_F32> __device__ inline void sobel_3x3(const float (&p)[3][3], float &gx, float &gy) {
    if constexpr (ANY_F32) {
        gx = (((((((-p[0][0] + p[0][1] * 0.0f) + p[0][2]) - 2.0f * p[1][0]) + p[1][1] * 0.0f) + 2.0f * p[1][2]) - p[2][0]) + p[2][1] * 0.0f) + p[2][2];
        gy = (((((((-p[0][0] - 2.0f * p[0][1]) - p[0][2]) + p[1][0] * 0.0f) + p[1][1] * 0.0f) + p[1][2] * 0.0f) + p[2][0]) + 2.0f * p[2][1]) + p[2][2];
    } else {
        gx = ((((-p[0][0] + p[0][2]) - 2.0f * p[1][0]) + 2.0f * p[1][2]) - p[2][0]) + p[2][2];
        gy = ((((-p[0][0] - 2.0f * p[0][1]) - p[0][2]) + p[2][0]) + 2.0f * p[2][1]) + p[2][2];
    }
}

// Tile 64 x 16 outputs, grey values one pixel around it in LDS (a wave per row, .replicate by clamped coordinates); a thread owns
// four consecutive rows of one column, whose windows share six rows of three values; output bytes leave as dwords through LDS.
// (Round 1: 64 x 4 tile, nine clamped taps per pixel, byte stores: 67 us per 4096^2 Rgba(u8) frame.)
template <int PIX>
__global__ __launch_bounds__(256) void k_sobel(DImg src, DImg dst, int tiles_x, FrameSpan fr) {
    using P = Px<PIX>;
    constexpr int TH = 16;
    __shared__ float g[TH + 2][68];
    __shared__ uint8_t ob[TH][64];
    src.data = (char *)src.data + (size_t)blockIdx.y * fr.src_frame; // a batch of equally shaped frames (zg_batch_pipeline's edges step)
    dst.data = (char *)dst.data + (size_t)blockIdx.y * fr.dst_frame;
    const int wg = xcd_major((int)blockIdx.x, (int)gridDim.x);
    const int ty = wg / tiles_x, tx = wg - ty * tiles_x;
    const int x0 = tx * 64, y0 = ty * TH;
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    {
        const int gc = min(max(x0 - 1 + lane, 0), src.cols - 1), gc2 = min(max(x0 + 63 + lane, 0), src.cols - 1);
        for (int rr = w; rr < TH + 2; rr += 4) {
            const size_t row = (size_t)min(max(y0 - 1 + rr, 0), src.rows - 1) * src.stride;
            g[rr][lane] = sobel_gray<PIX>(P::load(src.data, row + (size_t)gc));
            if (lane < 2) g[rr][64 + lane] = sobel_gray<PIX>(P::load(src.data, row + (size_t)gc2));
        }
    }
    __syncthreads();
    float p[6][3];
#pragma unroll
    for (int j = 0; j < 6; ++j)
#pragma unroll
        for (int i = 0; i < 3; ++i) p[j][i] = g[4 * w + j][lane + i];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const float win[3][3] = {{p[k][0], p[k][1], p[k][2]}, {p[k + 1][0], p[k + 1][1], p[k + 1][2]}, {p[k + 2][0], p[k + 2][1], p[k + 2][2]}};
        float ax, ay;
        sobel_3x3<PIX == ZG_PIXEL_F32>(win, ax, ay);
        const float sx = ax * ax, sy = ay * ay;
        const float magnitude = sqrtf(sx + sy);
        const float scaled = magnitude / 4.0f;
        const float clamped = fmaxf(0.0f, fminf(255.0f, scaled));
        ob[4 * w + k][lane] = (uint8_t)(int)truncf(clamped);
    }
    __syncthreads();
    const int lr = threadIdx.x >> 4, q = (threadIdx.x & 15) * 4, r = y0 + lr;
    if (r < dst.rows && x0 + q < dst.cols) {
        uint8_t *o = (uint8_t *)dst.data + (size_t)r * dst.stride + x0 + q;
        if (x0 + q + 4 <= dst.cols && (dst.stride & 3) == 0 && ((uintptr_t)dst.data & 3) == 0) {
            *(uint32_t *)o = *(const uint32_t *)&ob[lr][q];
        } else {
            for (int j = 0; j < 4 && x0 + q + j < dst.cols; ++j) o[j] = ob[lr][q + j];
        }
    }
}

// Image.sobel of n equally shaped frames in one launch (-1: too many frames for one grid)
int sobel_frames(const FrameBatch &b, hipStream_t s) {
    const zg_image *src = b.src, *dst = b.dst;
    const uint32_t n = b.n;
    int rc;
    if ((rc = check_image(src, "src")) || (rc = check_image(dst, "dst"))) return rc;
    ZG_REQUIRE(src->rows == dst->rows && src->cols == dst->cols, ZG_ERR_DIMENSION_MISMATCH, "sobel: %ux%u vs %ux%u",
               src->rows, src->cols, dst->rows, dst->cols);
    ZG_REQUIRE(dst->pixel == ZG_PIXEL_U8, ZG_ERR_INVALID_ARGUMENT, "sobel: the output is Image(u8)");
    if (src->rows == 0 || src->cols == 0) return ZG_OK;
    // in place on an Image(u8), or a destination view that shares bytes with the source: a lane reads its neighbours' pixels, so the source is copied first.
    // One image only: a batch (n > 1, sobel_frames) comes from the pipeline, whose source and destination frames are separate buffers; other
    // callers of the frames entry must keep theirs disjoint.
    zg_image copy{};
    ScratchBlock aside(s);
    if (n == 1 && spans_overlap(src, dst)) {
        if ((rc = aside.alloc((size_t)src->rows * src->cols * pixel_size(src->pixel)))) return rc;
        copy = zg_image{aside.p, src->cols, src->rows, src->cols, src->pixel};
        if ((rc = copy_impl(src, &copy, s))) return rc;
        src = &copy;
    }
    if (const int rcs = try_sobel_stream(FrameBatch{src, dst, n, b.src_frame, b.dst_frame}, s); rcs >= 0) return rcs; // u8 / Rgba(u8): one wave per column strip
    const int tiles_x = (int)ceil_div(src->cols, 64), tiles_y = (int)ceil_div(src->rows, 16);
    if (n > MAX_FRAMES_PER_LAUNCH) return -1; // the caller goes frame by frame
    const FrameSpan fr = b.span();
    return dispatch_pixel(src->pixel, [&](auto tag) -> int {
        constexpr int PIX = decltype(tag)::value;
        hipLaunchKernelGGL((k_sobel<PIX>), dim3((unsigned)(tiles_x * tiles_y), n), dim3(256), 0, s, dimg(src), dimg(dst), tiles_x, fr);
        return launch_ok();
    });
}


// ---- Canny (src/image.zig:1047-1063 -> src/image/edges.zig:212-277) --------------------------------------------------
// grey plane as(f32, convertColor(u8, px)) -> the detector's own Gaussian (.replicate) -> Sobel gradients -> magnitude ->
// non-maximum suppression -> double threshold + hysteresis. The reference materialises six full planes and walks a BFS
// queue; here: one grey kernel, the library's separable convolution, ONE fused kernel for gradients + magnitude + NMS +
// classification (a 2-pixel halo of the blurred plane in LDS; its output is a single byte per pixel: 0 none, 1 weak, 2
// strong), and hysteresis as connected-component labelling (see run_hysteresis): the BFS's reachable set, in a fixed
// number of kernels.

template <int PIX> __device__ inline float canny_gray(typename Px<PIX>::Vec v) { // as(f32, convertColor(u8, px)), edges.zig:231-240
    if constexpr (PIX == ZG_PIXEL_F32) { // scalar float -> u8 in f64 (color.zig:114-118)
        double d = (double)v[0];
        d = d != d ? 1.0 : (d < 0.0 ? 0.0 : (d > 1.0 ? 1.0 : d)); // std.math.clamp = @max(0, @min(d, 1)): a NaN clamps to 1, the byte is 255
        return (float)(int)round(d * 255.0);
    } else return sobel_gray<PIX>(v);
}

template <int PIX>
__global__ __launch_bounds__(256) void k_canny_gray(DImg src, float *gray) {
    using P = Px<PIX>;
    const int c = blockIdx.x * 256 + threadIdx.x, r = grid_row();
    if (c >= src.cols || r >= src.rows) return;
    gray[(size_t)r * src.cols + c] = canny_gray<PIX>(P::load(src.data, (size_t)r * src.stride + (size_t)c));
}

// four pixels per lane: one 16-byte load of Rgba(u8) (when the rows are 16-byte aligned), one float4 store
template <int PIX>
__global__ __launch_bounds__(256) void k_canny_gray4(DImg src, float *gray, uint8_t *gray8, int wide) { // cols % 4 == 0, gray 16-byte aligned; gray8: the same values as bytes; either may be null
    using P = Px<PIX>;
    const int c = (blockIdx.x * 256 + threadIdx.x) * 4, r = grid_row();
    if (c >= src.cols || r >= src.rows) return;
    typename P::Vec v[4];
    if constexpr (PIX == ZG_PIXEL_RGBA_U8) {
        if (wide) {
            const uint4 q = *(const uint4 *)((const uint8_t *)src.data + ((size_t)r * src.stride + (size_t)c) * 4);
            v[0] = __builtin_bit_cast(typename P::Vec, q.x); v[1] = __builtin_bit_cast(typename P::Vec, q.y);
            v[2] = __builtin_bit_cast(typename P::Vec, q.z); v[3] = __builtin_bit_cast(typename P::Vec, q.w);
        } else {
#pragma unroll
            for (int k = 0; k < 4; ++k) v[k] = P::load(src.data, (size_t)r * src.stride + (size_t)(c + k));
        }
    } else {
#pragma unroll
        for (int k = 0; k < 4; ++k) v[k] = P::load(src.data, (size_t)r * src.stride + (size_t)(c + k));
    }
    const float4 g = make_float4(canny_gray<PIX>(v[0]), canny_gray<PIX>(v[1]), canny_gray<PIX>(v[2]), canny_gray<PIX>(v[3]));
    if (gray) *(float4 *)(gray + (size_t)r * src.cols + c) = g;
    if (gray8) *(uint32_t *)(gray8 + (size_t)r * src.cols + c) = (uint32_t)g.x | ((uint32_t)g.y << 8) | ((uint32_t)g.z << 16) | ((uint32_t)g.w << 24); // integers 0 .. 255
}
// The grey plane of both detectors and of zg_isef_smooth's byte sources: f32 into `gray`, the same values as bytes into `gray8`.
// gray8 (and a null gray) only where cols % 4 == 0.
int canny_gray_plane(const zg_image *src, float *gray, uint8_t *gray8, hipStream_t s) {
    return dispatch_pixel(src->pixel, [&](auto tag) -> int {
        constexpr int PIX = decltype(tag)::value;
        if (src->cols % 4 == 0 && ((uintptr_t)gray & 15) == 0) {
            const int wide = ((size_t)src->stride * 4) % 16 == 0 && ((uintptr_t)src->data & 15) == 0;
            hipLaunchKernelGGL((k_canny_gray4<PIX>), row_grid(ceil_div(src->cols, 1024), src->rows), dim3(256), 0, s, dimg(src), gray, gray8, wide);
        } else {
            hipLaunchKernelGGL((k_canny_gray<PIX>), row_grid(ceil_div(src->cols, 256), src->rows), dim3(256), 0, s, dimg(src), gray);
        }
        return launch_ok();
    });
}

// blurred plane -> state plane. Tile 64 x 16 outputs; magnitudes are needed one pixel around it, blurred values two.
// A thread owns four consecutive rows of one column: their 3 x 3 windows share six rows of three blurred values, and the Sobel sums
// skip the zero weights and fold the +-1 / +-2 weights into additions (exact products, so the reference's nine-term sums in the
// reference's order, edges.zig:255-262, up to the sign of a zero); only the magnitude goes back to LDS, plus the ring of magnitudes
// around the tile (164 positions, one each for the first threads). The round-1 form (64 x 4 tile, every gradient through a clamped
// nine-tap loop and three LDS planes) took 111 us per 4096^2 frame.
__global__ __launch_bounds__(256) void k_canny_nms(const float *blur, uint8_t *state, int rows, int cols, float low, float high, int tiles_x) {
    constexpr int TH = 16;
    __shared__ float b[TH + 4][68];   // blurred: tile row r, column c at [r + 2][c + 2]
    __shared__ float mag[TH + 2][68]; // magnitude: at [r + 1][c + 1]
    __shared__ uint8_t st[TH][64];
    const int wg = xcd_major((int)blockIdx.x, (int)gridDim.x);
    const int ty = wg / tiles_x, tx = wg - ty * tiles_x;
    const int x0 = tx * 64, y0 = ty * TH;
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    { // .replicate of the 3 x 3 convolutions: clamped coordinates; a wave per row, the four columns beyond 64 by its first lanes
        const int gc = min(max(x0 - 2 + lane, 0), cols - 1), gc2 = min(max(x0 + 62 + lane, 0), cols - 1);
        for (int rr = w; rr < TH + 4; rr += 4) {
            const size_t row = (size_t)min(max(y0 - 2 + rr, 0), rows - 1) * cols;
            b[rr][lane] = blur[row + gc];
            if (lane < 4) b[rr][64 + lane] = blur[row + gc2];
        }
    }
    __syncthreads();
    float gx[4], gy[4], m[4];
    {
        float p[6][3];
#pragma unroll
        for (int j = 0; j < 6; ++j)
#pragma unroll
            for (int i = 0; i < 3; ++i) p[j][i] = b[4 * w + 1 + j][lane + 1 + i];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const float win[3][3] = {{p[k][0], p[k][1], p[k][2]}, {p[k + 1][0], p[k + 1][1], p[k + 1][2]}, {p[k + 2][0], p[k + 2][1], p[k + 2][2]}};
            sobel_3x3<false>(win, gx[k], gy[k]); // finite: every canny source, Image(f32) included, is clamped into a byte by canny_gray first
            const float sx = gx[k] * gx[k], sy = gy[k] * gy[k];
            m[k] = sqrtf(sx + sy);
            mag[4 * w + k + 1][lane + 1] = m[k];
        }
    }
    if (threadIdx.x < 2 * 66 + 2 * TH) { // the ring: row -1, row TH (columns -1 .. 64), column -1, column 64 (rows 0 .. TH - 1)
        const int t = threadIdx.x;
        int hr, hc;
        if (t < 66) { hr = -1; hc = t - 1; }
        else if (t < 132) { hr = TH; hc = t - 67; }
        else if (t < 132 + TH) { hr = t - 132; hc = -1; }
        else { hr = t - 132 - TH; hc = 64; }
        float win[3][3];
#pragma unroll
        for (int j = 0; j < 3; ++j)
#pragma unroll
            for (int i = 0; i < 3; ++i) win[j][i] = b[hr + 1 + j][hc + 1 + i];
        float hx, hy;
        sobel_3x3<false>(win, hx, hy); // as above: grey bytes blurred with finite taps
        const float sx = hx * hx, sy = hy * hy;
        mag[hr + 1][hc + 1] = sqrtf(sx + sy);
    }
    __syncthreads();
    const int c = x0 + lane;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int lr = 4 * w + k, r = y0 + lr;
        uint8_t s = 0;
        if (rows >= 3 && cols >= 3 && r >= 1 && r < rows - 1 && c >= 1 && c < cols - 1) { // edges.zig:710-715
            const float K = 0.414213562f; // tan(22.5 deg)
            const float ax = fabsf(gx[k]), ay = fabsf(gy[k]);
            int dr1, dc1, dr2, dc2;
            if (ay <= K * ax) { dr1 = 0; dc1 = -1; dr2 = 0; dc2 = 1; }
            else if (ax <= K * ay) { dr1 = -1; dc1 = 0; dr2 = 1; dc2 = 0; }
            else if (gx[k] * gy[k] > 0) { dr1 = -1; dc1 = 1; dr2 = 1; dc2 = -1; }
            else { dr1 = -1; dc1 = -1; dr2 = 1; dc2 = 1; }
            const float n1 = mag[lr + 1 + dr1][lane + 1 + dc1], n2 = mag[lr + 1 + dr2][lane + 1 + dc2];
            if (m[k] >= n1 && m[k] >= n2) s = m[k] >= high ? 2 : (m[k] >= low ? 1 : 0); // edges.zig:541, :566
        }
        st[lr][lane] = s;
    }
    __syncthreads();
    { // the tile's state bytes, four columns per thread
        const int lr = threadIdx.x >> 4, q = (threadIdx.x & 15) * 4, r = y0 + lr;
        if (r < rows && x0 + q < cols) {
            uint8_t *o = state + (size_t)r * cols + x0 + q;
            if ((cols & 3) == 0 && ((uintptr_t)state & 3) == 0) {
                *(uint32_t *)o = *(const uint32_t *)&st[lr][q];
            } else {
                for (int j = 0; j < 4 && x0 + q + j < cols; ++j) o[j] = st[lr][q + j];
            }
        }
    }
}

// Hysteresis (edges.zig:499-576): a weak candidate becomes an edge iff it is 8-connected, through candidates, to a strong
// one. The reference grows the set with a BFS queue; the set itself is "the connected components of the candidate mask
// that contain a strong pixel", which a lock-free union-find labels in a fixed number of kernels (no convergence loop, no
// host synchronisation, so the detectors stay asynchronous and graph-capturable):
//   k_cc_tile    a workgroup labels one 64 x 64 tile entirely in LDS (runs from a ballot, unions with LDS atomics). A component that
//                does not reach the tile's edge is finished there and then: its pixels are written to the output (strong, or weak with
//                a strong pixel in the component) and leave the state plane. Only the components on a tile edge stay PENDING: their
//                pixels keep their state and get a label (the global index of the tile root), their roots a cleared flag and CC_ROOT (| CC_ROOT_STRONG) in their state byte.
//   k_cc_border  the pixels on tile edges are united with their neighbours in the next tile through global memory: 1/32 of
//                the pixels; roots only ever move to smaller indices (atomicMin), so the structure stays a forest whatever
//                the interleaving
//   k_cc_mark    the root of every pending tile component that holds a strong pixel marks the root of its global component
//   k_cc_emit_tile  a tile's roots look their global verdicts up; every pending weak pixel reads its own root's in LDS
// The label plane is only touched where components cross tiles, and the two last passes read a byte per pixel.
// (Round 1 united every pixel pair through global memory: 177 - 296 us of the detectors' time on 4096^2 noise; labelling tiles but
// still writing a label per pixel and resolving every weak pixel in a separate pass took 149 us on canny's frame.)
// Links to the row below (SW / S / SE; the upward directions are the same pairs seen from the other side). Links the run
// structure already implies are skipped: with S a candidate, SW and SE hang off S's run, and S itself is implied when W and
// SW are both candidates (the pixel to the left makes the same link); without S, SW is implied by W and SE by E.
constexpr int CC_T = 64; // tile edge
// state bytes after k_cc_tile: 0 resolved / not a candidate, 1 weak and pending, 2 strong and pending; on the root pixel of a pending tile component also:
constexpr uint8_t CC_ROOT = 0x80, CC_ROOT_STRONG = 0x40;
__global__ __launch_bounds__(256) void k_cc_tile(uint8_t *state, int *label, uint16_t *label16, uint8_t *flag, DImg dst, int rows, int cols) {
    __shared__ int lab[CC_T * CC_T];
    __shared__ uint8_t st[CC_T + 1][CC_T]; // one spare row of zeros below
    __shared__ uint8_t out[CC_T][CC_T];
    const int t = threadIdx.x, lane = t & 63, w = t >> 6;
    const int x0 = blockIdx.x * CC_T, y0 = blockIdx.y * CC_T;
    const bool whole = x0 + CC_T <= cols && y0 + CC_T <= rows && (((uintptr_t)state | (uintptr_t)cols) & 3) == 0;
    if (whole) { // 16 rows of 64 bytes per instruction
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const int r = k * 16 + (t >> 4), c = (t & 15) * 4;
            *(uint32_t *)&st[r][c] = *(const uint32_t *)(state + (size_t)(y0 + r) * cols + x0 + c);
        }
    } else {
        for (int i = t; i < CC_T * CC_T; i += 256) {
            const int r = i >> 6, c = i & 63;
            st[r][c] = (y0 + r < rows && x0 + c < cols) ? state[(size_t)(y0 + r) * cols + x0 + c] : 0;
        }
    }
    if (t < CC_T) st[CC_T][t] = 0;
    __syncthreads();
    // a candidate starts under the first pixel of its horizontal run (ballot + count-leading-zeros)
    uint32_t mine = 0; // bit k: my pixel of row w * 16 + k is a candidate
    unsigned long long rowm[17]; // the candidates of my sixteen rows and of the row below them, a bit a column: wave-uniform
#pragma unroll
    for (int k = 0; k < 16; ++k) {
        const int r = w * 16 + k;
        const bool cand = st[r][lane] != 0;
        rowm[k] = __ballot(cand);
        const unsigned long long gaps = ~rowm[k] & ((1ull << lane) - 1); // non-candidates to my left
        const int start = gaps ? 64 - __clzll(gaps) : 0;
        lab[r * CC_T + lane] = r * CC_T + (cand ? start : lane);
        mine |= (uint32_t)cand << k;
    }
    rowm[16] = __ballot(st[w * 16 + 16][lane] != 0); // row 64 is zeros
    __syncthreads();
    // The links of a row are bit operations on two row masks (scalar): which pixels link to S, to SW, to SE under the skip rules above. Rows
    // without a link cost nothing, and no pixel reads its neighbours' bytes.
    const unsigned long long me = 1ull << lane;
#pragma unroll
    for (int k = 0; k < 16; ++k) {
        const unsigned long long C = rowm[k], S = rowm[k + 1], W = C << 1, E = C >> 1, SW = S << 1, SE = S >> 1;
        const unsigned long long to_s = C & S & ~(W & SW), to_sw = C & ~S & SW & ~W, to_se = C & ~S & SE & ~E;
        if ((to_s | to_sw | to_se) == 0) continue; // wave-uniform
        const int i = (w * 16 + k) * CC_T + lane;
        // one pass of the union loop serves all three directions (a lane has S, or SW and / or SE); the few lanes with both diagonals go again
        const bool d_s = (to_s & me) != 0, d_sw = (to_sw & me) != 0, d_se = (to_se & me) != 0;
        if (d_s | d_sw | d_se) cc_unite(lab, i, i + CC_T + (d_s ? 0 : (d_sw ? -1 : 1)));
        if ((to_sw & to_se) != 0 && d_sw && d_se) cc_unite(lab, i, i + CC_T + 1);
    }
    __syncthreads();
    // every candidate straight under its root ...
    int root[16];
#pragma unroll
    for (int k = 0; k < 16; ++k) root[k] = ((mine >> k) & 1) ? cc_find(lab, (w * 16 + k) * CC_T + lane) : 0;
    __syncthreads();
#pragma unroll
    for (int k = 0; k < 16; ++k)
        if ((mine >> k) & 1) lab[(w * 16 + k) * CC_T + lane] = root[k];
    __syncthreads();
    // ... then what the component holds goes into the top bits of the root's entry (entries are < 4096): STRONG, EDGE (of the tile)
    constexpr int STRONG = 1 << 16, EDGE = 1 << 17;
    if (mine) {
        for (int k = 0; k < 16; ++k) {
            if (!((mine >> k) & 1)) continue;
            const int r = w * 16 + k;
            int a = st[r][lane] == 2 ? STRONG : 0;
            if (r == 0 || r == CC_T - 1 || lane == 0 || lane == CC_T - 1) a |= EDGE;
            if (a) atomicOr(&lab[root[k]], a);
        }
    }
    __syncthreads();
    const bool col_ok = x0 + lane < cols;
#pragma unroll 4
    for (int k = 0; k < 16; ++k) {
        const int r = w * 16 + k;
        uint8_t o = 0, ns = 0;
        if ((mine >> k) & 1) {
            const int a = lab[root[k]];
            const uint8_t s = st[r][lane];
            if (a & EDGE) { // pending: keeps its state, gets a label; a strong pixel is an edge whatever happens
                ns = s;
                o = s == 2 ? 255 : 0;
                if (col_ok && y0 + r < rows) {
                    const size_t gi = (size_t)(y0 + r) * cols + x0 + lane;
                    const int groot = (y0 + (root[k] >> 6)) * cols + x0 + (root[k] & 63);
                    // every pending pixel: its root's place IN THE TILE (two bytes; what k_cc_emit_tile reads). The global label — a node of the forest the
                    // border links build — only where the forest can touch it: the tile's edge pixels (a find starts there) and the root itself.
                    label16[gi] = (uint16_t)root[k];
                    const bool is_root = (int)gi == groot;
                    if (is_root || r == 0 || r == CC_T - 1 || lane == 0 || lane == CC_T - 1) label[gi] = groot;
                    if (is_root) { // the root pixel of a pending tile component says so in its state byte, and whether the component holds a strong pixel
                        ns = s | CC_ROOT | ((a & STRONG) ? CC_ROOT_STRONG : 0);
                        flag[gi] = 0;
                    }
                }
            } else {
                o = (s == 2 || (a & STRONG)) ? 255 : 0;
            }
        }
        st[r][lane] = ns; // my own pixel: nobody else reads it any more
        out[r][lane] = o;
    }
    __syncthreads();
    const bool vec = whole && (dst.stride & 3) == 0 && ((uintptr_t)dst.data & 3) == 0;
    if (vec) {
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const int r = k * 16 + (t >> 4), c = (t & 15) * 4;
            *(uint32_t *)(state + (size_t)(y0 + r) * cols + x0 + c) = *(const uint32_t *)&st[r][c];
            *(uint32_t *)((uint8_t *)dst.data + (size_t)(y0 + r) * dst.stride + x0 + c) = *(const uint32_t *)&out[r][c];
        }
    } else {
        for (int i = t; i < CC_T * CC_T; i += 256) {
            const int r = i >> 6, c = i & 63;
            if (y0 + r < rows && x0 + c < cols) {
                state[(size_t)(y0 + r) * cols + x0 + c] = st[r][c];
                ((uint8_t *)dst.data)[(size_t)(y0 + r) * dst.stride + x0 + c] = out[r][c];
            }
        }
    }
}
// blockIdx.y < nvb: the right-hand column of a tile column (pixel with E / NE / SE in the next tile); otherwise the bottom row
// of a tile row (SW / S / SE below). The skip rules above hold across tiles for the same reasons: the link they rely on is
// either inside a tile or another border link. A candidate on a tile edge is pending by construction, so `state` still has it.
__global__ __launch_bounds__(256) void k_cc_border(const uint8_t *state, int *label, int rows, int cols, int nvb) {
    const int j = blockIdx.x * 256 + threadIdx.x;
    int b = blockIdx.y;
    if (b < nvb) {
        const int x = b * CC_T + CC_T - 1, r = j; // x + 1 < cols by construction
        if (r >= rows) return;
        const int i = r * cols + x;
        if (!state[i]) return;
        if (state[i + 1]) { cc_unite_global(label, i, i + 1); return; } // NE and SE hang off E
        if (r > 0 && state[i - cols + 1] && !state[i - cols]) cc_unite_global(label, i, i - cols + 1);
        if (r + 1 < rows && state[i + cols + 1] && !state[i + cols]) cc_unite_global(label, i, i + cols + 1);
    } else {
        b -= nvb;
        const int y = b * CC_T + CC_T - 1, c = j; // y + 1 < rows by construction
        if (c >= cols) return;
        const int i = y * cols + c;
        if (!state[i]) return;
        const bool wc = c > 0 && state[i - 1], ec = c + 1 < cols && state[i + 1];
        const bool sw = c > 0 && state[i + cols - 1], so = state[i + cols], se = c + 1 < cols && state[i + cols + 1];
        if (so) {
            if (!(wc && sw)) cc_unite_global(label, i, i + cols);
        } else {
            if (sw && !wc) cc_unite_global(label, i, i + cols - 1);
            if (se && !ec) cc_unite_global(label, i, i + cols + 1);
        }
    }
}
// After the border links: every pending tile component that holds a strong pixel marks the root of its global component (flag[root] = 1; the flags of
// all tile roots were cleared by k_cc_tile). Four state bytes per lane; most dwords have no root.
__global__ __launch_bounds__(256) void k_cc_mark(const uint8_t *state, int *label, uint8_t *flag, size_t n) {
    const size_t i0 = ((size_t)blockIdx.x * 256 + threadIdx.x) * 4;
    if (i0 >= n) return;
    uint32_t s4 = 0;
    if (i0 + 4 <= n && ((uintptr_t)state & 3) == 0) s4 = *(const uint32_t *)(state + i0);
    else for (size_t k = i0; k < n; ++k) s4 |= (uint32_t)state[k] << (8 * (k - i0));
    if ((s4 & (0x01010101u * CC_ROOT_STRONG)) == 0) return;
#pragma unroll
    for (int j = 0; j < 4; ++j)
        if ((s4 >> (8 * j)) & CC_ROOT_STRONG) flag[cc_find(label, (int)(i0 + j))] = 1;
}
// The weak pending pixels of a 64 x 64 tile become edges where their global component is marked. The roots of the tile's pending components look
// their global roots up once (that is where the tree walks are: a few dozen per tile instead of one per pixel) and leave the verdicts in LDS at
// the roots' places; a weak pixel reads the verdict at the place its two-byte label names. The pixels' labels are asked for before the roots walk,
// so the two round trips overlap. (One find per weak pixel through global memory: 56 us per 4096^2 frame of noise, 39 on a photo-like frame;
// with four-byte global labels decoded per pixel: 37 / 22.)
__global__ __launch_bounds__(256) void k_cc_emit_tile(const uint8_t *state, int *label, const uint16_t *label16, const uint8_t *flag, DImg dst, int rows, int cols) {
    __shared__ uint8_t verdict[CC_T][CC_T];
    const int t = threadIdx.x;
    const int x0 = blockIdx.x * CC_T, y0 = blockIdx.y * CC_T;
    const bool whole = x0 + CC_T <= cols && y0 + CC_T <= rows && (((uintptr_t)state | (uintptr_t)cols) & 3) == 0;
    const int c = (t & 15) * 4; // this lane's pixels: rows k * 16 + (t >> 4), columns c .. c + 4
    uint32_t st4[4];
    uint16_t l16[4][4];
    bool any_weak = false;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int r = k * 16 + (t >> 4);
        const size_t gi = (size_t)(y0 + r) * cols + x0 + c;
        st4[k] = 0;
        if (whole) st4[k] = *(const uint32_t *)(state + gi);
        else if (y0 + r < rows)
            for (int j = 0; j < 4 && x0 + c + j < cols; ++j) st4[k] |= (uint32_t)state[gi + j] << (8 * j);
    }
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int r = k * 16 + (t >> 4);
        const size_t gi = (size_t)(y0 + r) * cols + x0 + c;
        const uint32_t weak = (st4[k] & 0x01010101u) & ~((st4[k] >> 1) & 0x01010101u); // a byte is 1 exactly where the pixel is weak and pending
#pragma unroll
        for (int j = 0; j < 4; ++j) l16[k][j] = 0;
        if (weak) {
            any_weak = true;
            if (whole && ((uintptr_t)label16 & 7) == 0) { // four labels in one load (cols % 4 == 0)
                typedef uint32_t u32x2 __attribute__((ext_vector_type(2)));
                const u32x2 v = *(const u32x2 *)(label16 + gi);
                const uint32_t v0 = v[0], v1 = v[1];
                l16[k][0] = (uint16_t)v0; l16[k][1] = (uint16_t)(v0 >> 16); l16[k][2] = (uint16_t)v1; l16[k][3] = (uint16_t)(v1 >> 16);
            } else {
#pragma unroll
                for (int j = 0; j < 4; ++j)
                    if ((weak >> (8 * j)) & 1u) l16[k][j] = label16[gi + j];
            }
        }
    }
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        if ((st4[k] & (0x01010101u * CC_ROOT)) == 0) continue;
        const int r = k * 16 + (t >> 4);
#pragma unroll
        for (int j = 0; j < 4; ++j)
            if ((st4[k] >> (8 * j)) & CC_ROOT) verdict[r][c + j] = flag[cc_find(label, (y0 + r) * cols + x0 + c + j)];
    }
    if (!__syncthreads_or(any_weak)) return;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const uint32_t weak = (st4[k] & 0x01010101u) & ~((st4[k] >> 1) & 0x01010101u);
        if (!weak) continue;
        const int r = k * 16 + (t >> 4);
        uint8_t *drow = (uint8_t *)dst.data + (size_t)(y0 + r) * dst.stride + x0 + c;
#pragma unroll
        for (int j = 0; j < 4; ++j)
            if (((weak >> (8 * j)) & 1u) && (&verdict[0][0])[l16[k][j]] != 0) drow[j] = 255;
    }
}
// Writes the edge map of `state` (0 none / 1 weak / 2 strong) into dst; `state` is consumed. `work` holds an int label, a two-byte in-tile
// label and a flag byte per pixel (touched only where components cross tiles).
int run_hysteresis(uint8_t *state, uint32_t rows, uint32_t cols, char *work, const zg_image *dst, hipStream_t s, const char *who) {
    const size_t n = (size_t)rows * cols;
    if (n > 0x7fffffffu) { set_error("%s: hysteresis labels are 32-bit (rows * cols must stay below 2^31)", who); return ZG_ERR_UNSUPPORTED; }
    int *label = (int *)work;
    uint16_t *label16 = (uint16_t *)(label + n);
    uint8_t *flag = (uint8_t *)(label16 + (n + 3) / 4 * 4);
    const unsigned nb = (unsigned)((n + 1023) / 1024);
    const unsigned nvb = (cols - 1) / CC_T, nhb = (rows - 1) / CC_T;
    const dim3 tiles(ceil_div(cols, (unsigned)CC_T), ceil_div(rows, (unsigned)CC_T));
    hipLaunchKernelGGL(k_cc_tile, tiles, dim3(256), 0, s, state, label, label16, flag, dimg(dst), (int)rows, (int)cols);
    if (nvb + nhb)
        hipLaunchKernelGGL(k_cc_border, dim3(ceil_div(rows > cols ? rows : cols, 256u), nvb + nhb), dim3(256), 0, s, (const uint8_t *)state, label, (int)rows, (int)cols, (int)nvb);
    hipLaunchKernelGGL(k_cc_mark, dim3(nb), dim3(256), 0, s, (const uint8_t *)state, label, flag, n);
    hipLaunchKernelGGL(k_cc_emit_tile, tiles, dim3(256), 0, s, (const uint8_t *)state, label, (const uint16_t *)label16, (const uint8_t *)flag, dimg(dst), (int)rows, (int)cols);
    if (launch_ok("hysteresis")) { set_error("%s: hysteresis launch failed", who); return ZG_ERR_HIP; }
    return ZG_OK;
}
size_t hysteresis_work_bytes(uint32_t rows, uint32_t cols) {
    const size_t n = (size_t)rows * cols;
    return n * sizeof(int) + (n + 3) / 4 * 4 * sizeof(uint16_t) + n + 64; // global labels | two-byte in-tile labels | flags
}

// out = 255 on edges, 0 elsewhere (edges.zig:511-515). A strong pixel is an edge; a weak one is an edge when hysteresis
// ran (label != nullptr) and its component's root is flagged. Four pixels per lane; VEC moves them as one dword.
template <bool VEC>
__global__ __launch_bounds__(256) void k_canny_emit(const uint8_t *state, int *label, const uint8_t *flag, DImg dst) {
    const int c0 = (blockIdx.x * 256 + threadIdx.x) * 4, r = grid_row();
    if (c0 >= dst.cols || r >= dst.rows) return;
    const size_t i0 = (size_t)r * dst.cols + c0;
    uint8_t *out = (uint8_t *)dst.data + (size_t)r * dst.stride + c0;
    uint8_t st[4];
    const int nvalid = dst.cols - c0 < 4 ? dst.cols - c0 : 4;
    if (VEC) {
        *(uint32_t *)st = *(const uint32_t *)(state + i0);
    } else {
        for (int j = 0; j < 4; ++j) st[j] = j < nvalid ? state[i0 + j] : 0;
    }
    uint8_t px[4];
    for (int j = 0; j < 4; ++j) {
        bool edge = st[j] == 2;
        if (st[j] == 1 && label) edge = flag[cc_find(label, (int)(i0 + j))] != 0;
        px[j] = edge ? 255 : 0;
    }
    if (VEC) {
        *(uint32_t *)out = *(const uint32_t *)px;
    } else {
        for (int j = 0; j < nvalid; ++j) out[j] = px[j];
    }
}
int launch_emit(const uint8_t *state, int *label, const uint8_t *flag, const zg_image *dst, hipStream_t s) {
    const dim3 grid = row_grid(ceil_div(dst->cols, 1024), dst->rows);
    const bool vec = dst->cols % 4 == 0 && dst->stride % 4 == 0 && (uintptr_t)dst->data % 4 == 0;
    if (vec) hipLaunchKernelGGL(k_canny_emit<true>, grid, dim3(256), 0, s, state, label, flag, dimg(dst));
    else hipLaunchKernelGGL(k_canny_emit<false>, grid, dim3(256), 0, s, state, label, flag, dimg(dst));
    return launch_ok("k_canny_emit");
}

static int canny_impl(const zg_image *src, const zg_image *dst, float sigma, float low, float high, zg_stream stream) {
    hipStream_t s = as_stream(stream);
    int rc;
    if ((rc = check_image(src, "src")) || (rc = check_image(dst, "dst"))) return rc;
    ZG_REQUIRE(src->rows == dst->rows && src->cols == dst->cols, ZG_ERR_DIMENSION_MISMATCH, "canny: %ux%u vs %ux%u",
               src->rows, src->cols, dst->rows, dst->cols);
    ZG_REQUIRE(dst->pixel == ZG_PIXEL_U8, ZG_ERR_INVALID_ARGUMENT, "canny: the output is Image(u8)");
    ZG_REQUIRE(std::isfinite(sigma) && std::isfinite(low) && std::isfinite(high), ZG_ERR_INVALID_ARGUMENT, "canny: InvalidParameter (non-finite)");
    ZG_REQUIRE(sigma >= 0, ZG_ERR_INVALID_ARGUMENT, "canny: InvalidSigma (%g)", (double)sigma);
    ZG_REQUIRE(low >= 0 && high >= 0 && low < high, ZG_ERR_INVALID_ARGUMENT, "canny: InvalidThreshold (low %g, high %g)", (double)low, (double)high);
    if (src->rows == 0 || src->cols == 0) return ZG_OK;
    const uint32_t rows = src->rows, cols = src->cols;
    const size_t n = (size_t)rows * cols;
    // run_hysteresis's limit, checked before any scratch or launch: the frame's stages would otherwise run (and allocate 16 bytes a pixel) to be refused at the end
    ZG_REQUIRE(n <= 0x7fffffffu, ZG_ERR_UNSUPPORTED, "canny: hysteresis labels are 32-bit (rows * cols must stay below 2^31)");

    // scratch: grey f32 | blurred f32 | state u8 | hysteresis work
    ScratchBlock scratch(s);
    char *planes, *work;
    scratch.take(planes, 2 * n * sizeof(float) + n);
    scratch.take(work, hysteresis_work_bytes(rows, cols));
    if ((rc = scratch.alloc())) return rc;
    float *gray = (float *)planes, *blur = gray + n;
    uint8_t *state = (uint8_t *)(blur + n);

    const float *blurred = gray;
    if (sigma == 0) rc = canny_gray_plane(src, gray, nullptr, s);
    if (rc == ZG_OK && sigma != 0) { // blurGaussian (edges.zig:663-687): its own taps, .replicate
        const size_t radius = (size_t)std::ceil(3.0f * sigma), ks = 2 * radius + 1;
        // any length the separable convolution takes (kernels past 255 taps are read from device memory); the reference has no limit
        ZG_REQUIRE(3.0f * sigma < 2000000.0f, ZG_ERR_INVALID_ARGUMENT, "canny: sigma %g is out of range", (double)sigma);
        std::vector<float> k(ks);
        float sum = 0;
        for (size_t i = 0; i < ks; ++i) {
            const float x = (float)i - (float)radius;
            k[i] = hostmath::exp_f32(-(x * x) / (2.0f * sigma * sigma));
            sum += k[i];
        }
        for (size_t i = 0; i < ks; ++i) k[i] /= sum;
        const zg_image gi{gray, cols, rows, cols, ZG_PIXEL_F32}, bi{blur, cols, rows, cols, ZG_PIXEL_F32};
        // Image(u8) / Image(Rgba(u8)) sources, up to 65 taps: the blur's row pass takes the grey straight from the source
        rc = ks <= 65 ? try_sep_f32long_grey(src, &bi, k.data(), (int)ks, k.data(), (int)ks, ZG_BORDER_REPLICATE, s) : -1;
        if (rc == -1) {
            rc = canny_gray_plane(src, gray, nullptr, s);
            if (rc == ZG_OK) rc = zg_conv_separable(&gi, &bi, k.data(), (uint32_t)ks, k.data(), (uint32_t)ks, ZG_BORDER_REPLICATE, stream);
        }
        blurred = blur;
    }
    if (rc == ZG_OK) {
        const int tiles_x = (int)ceil_div(cols, 64), tiles_y = (int)ceil_div(rows, 16);
        hipLaunchKernelGGL(k_canny_nms, dim3((unsigned)(tiles_x * tiles_y)), dim3(256), 0, s, blurred, state, (int)rows, (int)cols, low, high, tiles_x);
        rc = run_hysteresis(state, rows, cols, work, dst, s, "canny");
    }
    return rc;
}

} // namespace zg

using namespace zg;

extern "C" {

int zg_sobel(const zg_image *src, const zg_image *dst, zg_stream stream) { return sobel_frames(FrameBatch{src, dst}, as_stream(stream)); }

int zg_sobel_host(const zg_image *src, const zg_image *dst) {
    return host_src_dst(src, dst, [&](const zg_image *a, const zg_image *b) { return sobel_frames(FrameBatch{a, b}, nullptr); });
}

int zg_canny(const zg_image *src, const zg_image *dst, float sigma, float low_threshold, float high_threshold, zg_stream stream) {
    return canny_impl(src, dst, sigma, low_threshold, high_threshold, stream);
}

int zg_canny_host(const zg_image *src, const zg_image *dst, float sigma, float low_threshold, float high_threshold) {
    return host_src_dst(src, dst, [&](const zg_image *a, const zg_image *b) { return canny_impl(a, b, sigma, low_threshold, high_threshold, nullptr); });
}

} // extern "C"
