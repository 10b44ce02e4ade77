// fdm.hip — FeatureDistributionMatching(T) (reference src/fdm.zig) for T = u8, Rgb(u8), Rgba(u8) on the device, in three stages
// (include/zignal_hip_fdm.h):
//   k_moments     one read of the frame into exact integer sums: n, the three channel sums, the six sums of products, the sum and sum of
//                 squares of the luminance byte, and whether any pixel is not grey. Integer adds commute: every order gives the same words.
//                 A workgroup leaves its sums in a slot of scratch; k_moments_finish, one workgroup a frame, adds the slots up.
//   k_target,     one lane per record around zg_fdm_solve.h, the header the host forms compile too: moments -> mean and covariance (exact
//   k_transform   128-bit numerator and denominator, one rounding each, one division) -> the reference's SVD and products.
//   k_apply       the per-pixel map in place, the reference's roundings: byte / 255.0 out of a 256-entry LDS table of those quotients, the
//                 3 x 3 affine map in f64 as written in fdm.zig:264-270; the two scalar routes out of a 256-entry byte table.
// A lane takes one group of neighbouring pixels (4 of a colour frame, 16 of a u8 frame) in every row_groups-th row of a strip of 256
// groups; the frame of a batch is blockIdx.y, and the frames' descriptors are kernel arguments, so nothing is uploaded.
// The statistics are where the device leaves the reference's bits (it runs Welford's recurrence): see the header and DESIGN.md section 8.
#include "zg_common.h"
#include "zg_scan.h"
#include "zg_fdm_solve.h"

#include "../../include/zignal_hip_fdm.h"

#include <algorithm>
#include <cstring>

#pragma clang fp contract(off)

namespace zg {
namespace {

constexpr uint32_t LANE_RUN = 2048;         // steps between two flushes of a lane's u32 partial sums: 2048 * 16 * 255^2 < 2^31
constexpr uint32_t TARGET_BLOCKS = 2048;    // workgroups a large frame is cut into: 8 per CU
constexpr uint32_t FRAMES_PER_LAUNCH = 32;  // descriptors in one kernel argument block

static_assert(sizeof(zg_fdm_moments) == 104 && sizeof(zg_fdm_target) == 136 && sizeof(zg_fdm_transform) == 120, "the records of zignal_hip_fdm.h");
static_assert((uint64_t)LANE_RUN * 16 * 255 * 255 < (1ull << 32), "a lane's partial sums cannot wrap inside a run");

struct Frame {
    uint8_t *data;
    uint64_t pitch; // bytes from one row to the next
    uint32_t rows, cols;
    int32_t pixel;
    uint32_t pad;
};
struct FrameList {
    Frame f[FRAMES_PER_LAUNCH];
};

template <int PIX> struct Group; // pixels a lane takes per step, and the 32-bit words they fill
template <> struct Group<ZG_PIXEL_U8> { static constexpr uint32_t G = 16, NW = 4, BPP = 1; };
template <> struct Group<ZG_PIXEL_RGB_U8> { static constexpr uint32_t G = 4, NW = 3, BPP = 3; };
template <> struct Group<ZG_PIXEL_RGBA_U8> { static constexpr uint32_t G = 4, NW = 4, BPP = 4; };

__host__ __device__ inline uint32_t group_pixels(int pixel) { return pixel == ZG_PIXEL_U8 ? 16u : 4u; }
// strips of 256 groups a row is cut into
__host__ __device__ inline uint32_t strips_of(uint32_t cols, int pixel) {
    const uint32_t g = group_pixels(pixel);
    return ((cols + g - 1) / g + 255) / 256;
}

// The block's strip and first row; rows go on in steps of row_groups. False: this block has no part of the frame.
__device__ inline bool block_strip(const Frame &f, uint32_t &strip, uint32_t &row0, uint32_t &row_groups) {
    const uint32_t strips = strips_of(f.cols, f.pixel);
    if (strips == 0 || f.rows == 0) return false;
    row_groups = gridDim.x / strips; // the host sized the grid to at least every frame's strips
    if (row_groups == 0) return false;
    strip = blockIdx.x % strips;
    row0 = blockIdx.x / strips;
    return row0 < row_groups;
}

// `count` pixels (1 .. G) at p into words, the rest zero. Whole groups whose address allows it move as words.
template <int PIX> __device__ inline void load_group(const uint8_t *p, uint32_t count, uint32_t (&w)[Group<PIX>::NW]) {
    using GR = Group<PIX>;
    if (count == GR::G && ((uintptr_t)p & 3) == 0) {
        if constexpr (GR::NW == 4) {
            if (((uintptr_t)p & 15) == 0) {
                const uint4 v = *(const uint4 *)p;
                w[0] = v.x; w[1] = v.y; w[2] = v.z; w[3] = v.w;
                return;
            }
        }
#pragma unroll
        for (uint32_t i = 0; i < GR::NW; ++i) w[i] = ((const uint32_t *)p)[i];
        return;
    }
#pragma unroll
    for (uint32_t i = 0; i < GR::NW; ++i) w[i] = 0;
    const uint32_t bytes = count * GR::BPP;
#pragma unroll
    for (uint32_t i = 0; i < GR::NW * 4; ++i) {
        if (i < bytes) w[i >> 2] |= (uint32_t)p[i] << (8 * (i & 3));
    }
}
// the first `count` pixels of the words back to p: never a byte past them
template <int PIX> __device__ inline void store_group(uint8_t *p, uint32_t count, const uint32_t (&w)[Group<PIX>::NW]) {
    using GR = Group<PIX>;
    if (count == GR::G && ((uintptr_t)p & 3) == 0) {
        if constexpr (GR::NW == 4) {
            if (((uintptr_t)p & 15) == 0) {
                *(uint4 *)p = make_uint4(w[0], w[1], w[2], w[3]);
                return;
            }
        }
#pragma unroll
        for (uint32_t i = 0; i < GR::NW; ++i) ((uint32_t *)p)[i] = w[i];
        return;
    }
    const uint32_t bytes = count * GR::BPP;
#pragma unroll
    for (uint32_t i = 0; i < GR::NW * 4; ++i) {
        if (i < bytes) p[i] = (uint8_t)(w[i >> 2] >> (8 * (i & 3)));
    }
}
// byte i of a group's words, i a constant
template <uint32_t NW> __device__ inline uint32_t byte_at(const uint32_t (&w)[NW], uint32_t i) { return (w[i >> 2] >> (8 * (i & 3))) & 255u; }

// a . b over four bytes, plus c (v_dot4_u32_u8)
__device__ inline uint32_t dot4(uint32_t a, uint32_t b, uint32_t c) {
#if __has_builtin(__builtin_amdgcn_udot4)
    return __builtin_amdgcn_udot4(a, b, c, false);
#else
    for (int k = 0; k < 4; ++k) c += ((a >> (8 * k)) & 255u) * ((b >> (8 * k)) & 255u);
    return c;
#endif
}
// convertColor(u8, pixel): BT.709 in 16.16 fixed point (src/color.zig:1031-1041, as convert_px of zg_blend.h); at most 255, so the
// reference's clamp never acts
__device__ inline uint32_t luminance(uint32_t r, uint32_t g, uint32_t b) { return (13933u * r + 46871u * g + 4732u * b + 32768u) >> 16; }

// ---- moments ---------------------------------------------------------------------------------------------------------------------------

enum { M_SUM = 0, M_PROD = 3, M_LUM = 9, M_LUM_SQ = 10, M_NOT_GRAY = 11, M_WORDS = 12 };
struct Sums {
    uint64_t v[M_WORDS];
};
struct AddSums {
    __device__ Sums operator()(const Sums &a, const Sums &b) const {
        Sums r;
#pragma unroll
        for (int i = 0; i < M_WORDS; ++i) r.v[i] = a.v[i] + b.v[i];
        return r;
    }
};

template <int PIX> __device__ inline void moments_lane(const Frame &f, uint32_t strip, uint32_t row0, uint32_t row_groups, Sums &acc) {
    using GR = Group<PIX>;
    const uint32_t x0 = (strip * 256u + threadIdx.x) * GR::G; // below 2^31: cols <= 0x3fffffff
    if (x0 >= f.cols) return;
    const uint32_t count = min(GR::G, f.cols - x0);
    uint32_t part[M_WORDS];
#pragma unroll
    for (int i = 0; i < M_WORDS; ++i) part[i] = 0;
    uint32_t steps = 0;
    for (uint32_t r = row0; r < f.rows; r += row_groups) {
        uint32_t w[GR::NW];
        load_group<PIX>(f.data + (uint64_t)r * f.pitch + (uint64_t)x0 * GR::BPP, count, w);
        if constexpr (PIX == ZG_PIXEL_U8) {
#pragma unroll
            for (uint32_t i = 0; i < 4; ++i) {
                part[M_LUM] = dot4(w[i], 0x01010101u, part[M_LUM]);
                part[M_LUM_SQ] = dot4(w[i], w[i], part[M_LUM_SQ]);
            }
        } else {
            // one channel of the four pixels in a word each, so that a sum of products is one dot product
            uint32_t ch[3] = {0, 0, 0}, y = 0;
#pragma unroll
            for (uint32_t k = 0; k < 4; ++k) {
#pragma unroll
                for (uint32_t c = 0; c < 3; ++c) ch[c] |= byte_at<GR::NW>(w, k * GR::BPP + c) << (8 * k);
                y |= luminance(byte_at<GR::NW>(w, k * GR::BPP), byte_at<GR::NW>(w, k * GR::BPP + 1), byte_at<GR::NW>(w, k * GR::BPP + 2)) << (8 * k);
            }
            int t = M_PROD;
#pragma unroll
            for (int i = 0; i < 3; ++i) {
                part[M_SUM + i] = dot4(ch[i], 0x01010101u, part[M_SUM + i]);
#pragma unroll
                for (int j = i; j < 3; ++j, ++t) part[t] = dot4(ch[i], ch[j], part[t]);
            }
            part[M_LUM] = dot4(y, 0x01010101u, part[M_LUM]);
            part[M_LUM_SQ] = dot4(y, y, part[M_LUM_SQ]);
            part[M_NOT_GRAY] |= (ch[0] ^ ch[1]) | (ch[1] ^ ch[2]);
        }
        if (++steps == LANE_RUN) { // widen before anything can wrap
#pragma unroll
            for (int i = 0; i < M_NOT_GRAY; ++i) {
                acc.v[i] += part[i];
                part[i] = 0;
            }
            steps = 0;
        }
    }
#pragma unroll
    for (int i = 0; i < M_NOT_GRAY; ++i) acc.v[i] += part[i];
    acc.v[M_NOT_GRAY] = part[M_NOT_GRAY] != 0 ? 1u : 0u;
}

// A workgroup leaves its sums in its own slot of `partials` ([frame][gridDim.x]); k_moments_finish adds a frame's slots up. A first version ended in one
// 64-bit atomic per quantity per workgroup into the record itself: 2048 workgroups times eleven atomics on one or two cache lines took 190 µs on any
// frame, ten times the read of a 4096 x 4096 Rgba(u8) frame (profiles/fdm_bench.txt).
__global__ __launch_bounds__(256) void k_moments(FrameList list, Sums *partials) {
    const Frame f = list.f[blockIdx.y];
    uint32_t strip, row0, row_groups;
    if (!block_strip(f, strip, row0, row_groups)) return; // the whole block; the finish does not read its slot
    Sums acc;
#pragma unroll
    for (int i = 0; i < M_WORDS; ++i) acc.v[i] = 0;
    if (f.pixel == ZG_PIXEL_U8) moments_lane<ZG_PIXEL_U8>(f, strip, row0, row_groups, acc);
    else if (f.pixel == ZG_PIXEL_RGB_U8) moments_lane<ZG_PIXEL_RGB_U8>(f, strip, row0, row_groups, acc);
    else moments_lane<ZG_PIXEL_RGBA_U8>(f, strip, row0, row_groups, acc);
    acc = block_reduce_ordered(acc, AddSums{});
    if (threadIdx.x == 0) partials[(size_t)blockIdx.y * gridDim.x + blockIdx.x] = acc;
}

// one workgroup a frame: the slots of the workgroups that had a part of the frame (block_strip, with k_moments' gridDim.x in gx), then every word of
// the record, so nothing has to be cleared first
__global__ __launch_bounds__(256) void k_moments_finish(FrameList list, const Sums *partials, uint32_t gx, zg_fdm_moments *out) {
    const Frame f = list.f[blockIdx.x];
    const uint32_t strips = strips_of(f.cols, f.pixel);
    const uint32_t slots = (strips == 0 || f.rows == 0) ? 0u : strips * (gx / strips);
    Sums acc;
#pragma unroll
    for (int i = 0; i < M_WORDS; ++i) acc.v[i] = 0;
    for (uint32_t b = threadIdx.x; b < slots; b += 256) acc = AddSums{}(acc, partials[(size_t)blockIdx.x * gx + b]);
    acc = block_reduce_ordered(acc, AddSums{});
    if (threadIdx.x == 0) {
        zg_fdm_moments m;
        m.n = (uint64_t)f.rows * f.cols;
#pragma unroll
        for (int i = 0; i < 3; ++i) m.sum[i] = acc.v[M_SUM + i];
#pragma unroll
        for (int i = 0; i < 6; ++i) m.prod[i] = acc.v[M_PROD + i];
        m.lum_sum = acc.v[M_LUM];
        m.lum_sq = acc.v[M_LUM_SQ];
        m.not_gray = acc.v[M_NOT_GRAY] != 0 ? 1u : 0u;
        m.pixel = f.pixel;
        out[blockIdx.x] = m;
    }
}

// ---- solve -----------------------------------------------------------------------------------------------------------------------------

// everything a lane's solve indexes at run time lives here, in LDS: no array on the stack
struct Work {
    double mean[3], cov[9];
    zg_fdm::Target t;
    zg_fdm::Transform x;
    zg_fdm::Scratch k;
};

__host__ __device__ inline void moments_stats(const zg_fdm_moments &m, bool lum, double mean[3], double cov[9]) {
    if (lum) zg_fdm::stats_from_scalar_moments(m.n, m.lum_sum, m.lum_sq, mean, cov);
    else zg_fdm::stats_from_moments(m.n, m.sum, m.prod, mean, cov);
}
__host__ __device__ inline void target_out(const zg_fdm::Target &t, int pixel, zg_fdm_target *o) {
    for (int i = 0; i < 3; ++i) o->mean[i] = t.mean[i];
    for (int i = 0; i < 9; ++i) o->u[i] = t.u[i];
    for (int i = 0; i < 3; ++i) o->s[i] = t.s[i];
    o->is_gray = t.is_gray;
    o->status = t.status;
    o->pixel = pixel;
    o->reserved = 0;
}
__host__ __device__ inline void target_in(const zg_fdm_target *i, zg_fdm::Target &t) {
    for (int k = 0; k < 3; ++k) t.mean[k] = i->mean[k];
    for (int k = 0; k < 9; ++k) t.u[k] = i->u[k];
    for (int k = 0; k < 3; ++k) t.s[k] = i->s[k];
    t.is_gray = i->is_gray;
    t.status = i->status;
}
__host__ __device__ inline void transform_out(const zg_fdm::Transform &x, zg_fdm_transform *o) {
    o->route = x.route;
    o->status = x.status;
    for (int i = 0; i < 9; ++i) o->w[i] = x.w[i];
    for (int i = 0; i < 3; ++i) o->bias[i] = x.bias[i];
    o->scale = x.scale;
    o->offset = x.offset;
}

__global__ __launch_bounds__(64) void k_target(const zg_fdm_moments *moments, zg_fdm_target *out) {
    __shared__ Work work;
    if (threadIdx.x != 0) return;
    const zg_fdm_moments m = *moments;
    const bool gray = m.pixel == ZG_PIXEL_U8 || m.not_gray == 0;
    moments_stats(m, m.pixel == ZG_PIXEL_U8, work.mean, work.cov);
    zg_fdm::target_from_stats(work.mean, work.cov, gray, &work.t, &work.k);
    target_out(work.t, m.pixel, out);
}

// pixel < 0: each record's own
__global__ __launch_bounds__(64) void k_transform(const zg_fdm_moments *moments, uint32_t n, int pixel, const zg_fdm_target *target, zg_fdm_transform *out) {
    __shared__ Work works[64];
    const uint32_t i = blockIdx.x * 64u + threadIdx.x;
    if (i >= n) return;
    Work &work = works[threadIdx.x];
    const zg_fdm_moments m = moments[i];
    const int pix = pixel < 0 ? m.pixel : pixel;
    target_in(target, work.t);
    if (pix != target->pixel || pix != m.pixel) {
        zg_fdm_transform bad;
        bad.route = 0;
        bad.status = ZG_FDM_STATUS_TYPE_MISMATCH;
        for (int k = 0; k < 9; ++k) bad.w[k] = 0.0;
        for (int k = 0; k < 3; ++k) bad.bias[k] = 0.0;
        bad.scale = 1.0;
        bad.offset = 0.0;
        out[i] = bad;
        return;
    }
    moments_stats(m, pix == ZG_PIXEL_U8 || work.t.is_gray != 0, work.mean, work.cov);
    zg_fdm::transform_from_stats(pix, &work.t, work.mean, work.cov, &work.x, &work.k);
    transform_out(work.x, out + i);
}

// ---- apply -----------------------------------------------------------------------------------------------------------------------------

template <int PIX> __device__ inline void apply_lane(const Frame &f, uint32_t strip, uint32_t row0, uint32_t row_groups, const zg_fdm_transform &x,
                                                     const double *unit, const uint8_t *map) {
    using GR = Group<PIX>;
    const uint32_t x0 = (strip * 256u + threadIdx.x) * GR::G;
    if (x0 >= f.cols) return;
    const uint32_t count = min(GR::G, f.cols - x0);
    for (uint32_t r = row0; r < f.rows; r += row_groups) {
        uint8_t *p = f.data + (uint64_t)r * f.pitch + (uint64_t)x0 * GR::BPP;
        uint32_t w[GR::NW], o[GR::NW];
        load_group<PIX>(p, count, w);
#pragma unroll
        for (uint32_t i = 0; i < GR::NW; ++i) o[i] = 0;
        if constexpr (PIX == ZG_PIXEL_U8) {
#pragma unroll
            for (uint32_t i = 0; i < 16; ++i) o[i >> 2] |= (uint32_t)map[byte_at<GR::NW>(w, i)] << (8 * (i & 3));
        } else {
#pragma unroll
            for (uint32_t k = 0; k < 4; ++k) {
                const uint32_t rb = byte_at<GR::NW>(w, k * GR::BPP), gb = byte_at<GR::NW>(w, k * GR::BPP + 1), bb = byte_at<GR::NW>(w, k * GR::BPP + 2);
                uint32_t out[3];
                if (x.route == ZG_FDM_ROUTE_COLOR) { // uniform
                    const double rr = unit[rb], gg = unit[gb], bl = unit[bb]; // byte / 255.0 (fdm.zig:258-260)
#pragma unroll
                    for (int j = 0; j < 3; ++j) out[j] = zg_fdm::unit_to_byte(rr * x.w[j] + gg * x.w[3 + j] + bl * x.w[6 + j] + x.bias[j]); // :264-270
                } else {
                    out[0] = out[1] = out[2] = map[luminance(rb, gb, bb)]; // :193-196
                }
#pragma unroll
                for (uint32_t c = 0; c < 3; ++c) {
                    const uint32_t at = k * GR::BPP + c;
                    o[at >> 2] |= out[c] << (8 * (at & 3));
                }
                // Rgba(u8): the colour route keeps alpha; the grey-target route's struct literal leaves it at the field default, 0
                if constexpr (PIX == ZG_PIXEL_RGBA_U8) {
                    if (x.route == ZG_FDM_ROUTE_COLOR) o[k] |= w[k] & 0xff000000u;
                }
            }
        }
        store_group<PIX>(p, count, o);
    }
}

__global__ __launch_bounds__(256) void k_apply(FrameList list, const zg_fdm_transform *transforms) {
    __shared__ double unit[256];
    __shared__ uint8_t map[256];
    const Frame f = list.f[blockIdx.y];
    const zg_fdm_transform x = transforms[blockIdx.y];
    if (x.status != 0) return; // the frame stays as it is
    const bool scalar = x.route != ZG_FDM_ROUTE_COLOR;
    // a transform of another family than the frame's type leaves the frame alone as well
    if (f.pixel == ZG_PIXEL_U8 ? x.route != ZG_FDM_ROUTE_SCALAR : (x.route != ZG_FDM_ROUTE_COLOR && x.route != ZG_FDM_ROUTE_GRAY_TARGET)) return;
    uint32_t strip, row0, row_groups;
    if (!block_strip(f, strip, row0, row_groups)) return;
    if (scalar) map[threadIdx.x] = zg_fdm::scalar_map((uint8_t)threadIdx.x, x.scale, x.offset); // fdm.zig:186-188, :193-195
    else unit[threadIdx.x] = (double)threadIdx.x / 255.0;
    __syncthreads();
    if (f.pixel == ZG_PIXEL_U8) apply_lane<ZG_PIXEL_U8>(f, strip, row0, row_groups, x, unit, map);
    else if (f.pixel == ZG_PIXEL_RGB_U8) apply_lane<ZG_PIXEL_RGB_U8>(f, strip, row0, row_groups, x, unit, map);
    else apply_lane<ZG_PIXEL_RGBA_U8>(f, strip, row0, row_groups, x, unit, map);
}

// ---- host ------------------------------------------------------------------------------------------------------------------------------

bool supported(int pixel) { return pixel == ZG_PIXEL_U8 || pixel == ZG_PIXEL_RGB_U8 || pixel == ZG_PIXEL_RGBA_U8; }

int check_frame(const zg_image *im, const char *who, bool device) {
    if (const int rc = check_image(im, who, device)) return rc;
    ZG_REQUIRE(supported(im->pixel), ZG_ERR_UNSUPPORTED, "%s: pixel type %d; feature distribution matching takes u8, Rgb(u8) and Rgba(u8) (fdm.zig:20)", who,
               im->pixel);
    ZG_REQUIRE((uint64_t)im->rows * im->cols < (1ull << 32), ZG_ERR_UNSUPPORTED, "%s: %u x %u pixels, 2^32 or more", who, im->rows, im->cols);
    return ZG_OK;
}
int check_frames(const zg_image *frames, uint32_t n, const char *who, bool device) {
    ZG_REQUIRE(frames != nullptr || n == 0, ZG_ERR_INVALID_ARGUMENT, "%s: null frames", who);
    for (uint32_t i = 0; i < n; ++i) {
        if (const int rc = check_frame(frames + i, who, device)) return rc;
    }
    return ZG_OK;
}

Frame frame_of(const zg_image *im) {
    const bool empty = im->rows == 0 || im->cols == 0;
    return Frame{(uint8_t *)im->data, (uint64_t)im->stride * pixel_size(im->pixel), empty ? 0u : im->rows, empty ? 0u : im->cols, im->pixel, 0u};
}
// workgroups for one frame: its strips times the row groups that bring it to about TARGET_BLOCKS
uint32_t blocks_of(const zg_image *im) {
    const uint32_t strips = strips_of(im->cols, im->pixel);
    if (strips == 0 || im->rows == 0) return 1;
    return strips * std::min(im->rows, std::max(1u, TARGET_BLOCKS / strips));
}

// `launch(list, first, count, grid_x)` for every FRAMES_PER_LAUNCH frames
template <typename F> int for_frame_lists(const zg_image *frames, uint32_t n, F &&launch) {
    for (uint32_t first = 0; first < n; first += FRAMES_PER_LAUNCH) {
        const uint32_t count = std::min(FRAMES_PER_LAUNCH, n - first);
        FrameList list{};
        uint32_t gx = 1;
        for (uint32_t i = 0; i < count; ++i) {
            list.f[i] = frame_of(frames + first + i);
            gx = std::max(gx, blocks_of(frames + first + i));
        }
        if (const int rc = launch(list, first, count, gx)) return rc;
    }
    return ZG_OK;
}

int moments_frames(const zg_image *frames, uint32_t n, zg_fdm_moments *out, hipStream_t s) {
    return for_frame_lists(frames, n, [&](const FrameList &list, uint32_t first, uint32_t count, uint32_t gx) {
        ScratchBlock sc(s);
        Sums *partials = nullptr;
        sc.take(partials, (size_t)count * gx);
        if (const int rc = sc.alloc()) return rc;
        hipLaunchKernelGGL(k_moments, dim3(gx, count), dim3(256), 0, s, list, partials);
        if (const int rc = launch_ok("k_moments")) return rc;
        hipLaunchKernelGGL(k_moments_finish, dim3(count), dim3(256), 0, s, list, (const Sums *)partials, gx, out + first);
        return launch_ok("k_moments_finish");
    });
}
int apply_frames(const zg_image *frames, uint32_t n, const zg_fdm_transform *transforms, hipStream_t s) {
    return for_frame_lists(frames, n, [&](const FrameList &list, uint32_t first, uint32_t count, uint32_t gx) {
        hipLaunchKernelGGL(k_apply, dim3(gx, count), dim3(256), 0, s, list, transforms + first);
        return launch_ok("k_apply");
    });
}
int target_from_moments(const zg_fdm_moments *m, zg_fdm_target *t, hipStream_t s) {
    hipLaunchKernelGGL(k_target, dim3(1), dim3(64), 0, s, m, t);
    return launch_ok("k_target");
}
int transform_from_moments(const zg_fdm_moments *m, uint32_t n, int pixel, const zg_fdm_target *t, zg_fdm_transform *x, hipStream_t s) {
    if (n == 0) return ZG_OK;
    hipLaunchKernelGGL(k_transform, dim3(ceil_div(n, 64u)), dim3(64), 0, s, m, n, pixel, t, x);
    return launch_ok("k_transform");
}

// n frames (device) against a target image or a prepared device target: one scratch block holds every record
int match_frames(const zg_image *frames, uint32_t n, const zg_image *target, const zg_fdm_target *prepared, hipStream_t s) {
    if (n == 0) return ZG_OK;
    ScratchBlock sc(s);
    zg_fdm_moments *m = nullptr;
    zg_fdm_transform *x = nullptr;
    zg_fdm_target *t = nullptr;
    sc.take(m, (size_t)n + 1); // the target's moments last
    sc.take(x, n);
    sc.take(t, 1);
    int rc;
    if ((rc = sc.alloc())) return rc;
    if ((rc = moments_frames(frames, n, m, s))) return rc;
    if (target) {
        if ((rc = moments_frames(target, 1, m + n, s))) return rc;
        if ((rc = target_from_moments(m + n, t, s))) return rc;
        prepared = t;
    }
    if ((rc = transform_from_moments(m, n, -1, prepared, x, s))) return rc;
    return apply_frames(frames, n, x, s);
}

int check_match(const zg_image *frames, uint32_t n, const zg_image *target, const zg_fdm_target *prepared, const char *who, bool device) {
    int rc;
    if ((rc = check_frames(frames, n, who, device))) return rc;
    ZG_REQUIRE(target != nullptr || prepared != nullptr, ZG_ERR_INVALID_ARGUMENT, "%s: neither a target image nor a prepared target", who);
    if (target) {
        if ((rc = check_frame(target, who, device))) return rc;
        for (uint32_t i = 0; i < n; ++i) {
            ZG_REQUIRE(frames[i].pixel == target->pixel, ZG_ERR_INVALID_ARGUMENT, "%s: frame %u has pixel type %d, the target %d", who, i, frames[i].pixel,
                       target->pixel);
        }
    }
    for (uint32_t i = 1; i < n; ++i) {
        ZG_REQUIRE(frames[i].pixel == frames[0].pixel, ZG_ERR_INVALID_ARGUMENT, "%s: frame %u has pixel type %d, frame 0 %d", who, i, frames[i].pixel, frames[0].pixel);
    }
    return ZG_OK;
}

int not_converged(int status, const char *who) {
    ZG_REQUIRE(status == 0, ZG_ERR_INVALID_ARGUMENT, "NotConverged: %s: the SVD stopped at singular value %d after 300 iterations", who, status);
    return ZG_OK;
}

// the host chain: stage every frame and the target, run the device chain on the default stream, look at the statuses, copy back
int match_frames_host(const zg_image *frames, uint32_t n, const zg_image *target) {
    int rc;
    if ((rc = check_match(frames, n, target, nullptr, "fdm_match_host", false))) return rc;
    ZG_REQUIRE(target != nullptr, ZG_ERR_INVALID_ARGUMENT, "fdm_match_host: null target");
    if (n == 0) return ZG_OK;
    std::vector<std::unique_ptr<HostStage>> stages;
    std::vector<zg_image> dev(n);
    for (uint32_t i = 0; i < n; ++i) {
        stages.emplace_back(new HostStage);
        if ((rc = stages.back()->upload(frames + i, true, true))) return rc;
        dev[i] = stages.back()->dev;
    }
    HostStage tg;
    if ((rc = tg.upload(target, true, false))) return rc;
    ScratchBlock sc;
    zg_fdm_moments *m = nullptr;
    zg_fdm_transform *x = nullptr;
    zg_fdm_target *t = nullptr;
    sc.take(m, (size_t)n + 1);
    sc.take(x, n);
    sc.take(t, 1);
    if ((rc = sc.alloc())) return rc;
    if ((rc = moments_frames(dev.data(), n, m, nullptr))) return rc;
    if ((rc = moments_frames(&tg.dev, 1, m + n, nullptr))) return rc;
    if ((rc = target_from_moments(m + n, t, nullptr))) return rc;
    if ((rc = transform_from_moments(m, n, -1, t, x, nullptr))) return rc;
    if ((rc = apply_frames(dev.data(), n, x, nullptr))) return rc;
    std::vector<zg_fdm_transform> xs(n);
    if ((rc = download_pageable(xs.data(), x, (size_t)n * sizeof(zg_fdm_transform), nullptr))) return rc; // waits for the stream
    for (uint32_t i = 0; i < n; ++i) {
        if ((rc = not_converged(xs[i].status, "fdm_match_host"))) return rc; // before anything is written back
    }
    for (uint32_t i = 0; i < n; ++i) {
        if ((rc = stages[i]->finish())) return rc;
    }
    return ZG_OK;
}

} // namespace
} // namespace zg

using namespace zg;

extern "C" {

size_t zg_fdm_sizeof_moments(void) { return sizeof(zg_fdm_moments); }
size_t zg_fdm_sizeof_target(void) { return sizeof(zg_fdm_target); }
size_t zg_fdm_sizeof_transform(void) { return sizeof(zg_fdm_transform); }
uint32_t zg_fdm_lane_run(void) { return LANE_RUN; }
uint32_t zg_fdm_frames_per_launch(void) { return FRAMES_PER_LAUNCH; }

int zg_fdm_compute_moments(const zg_image *img, zg_fdm_moments *moments_dev, zg_stream stream) {
    if (const int rc = check_frame(img, "fdm_moments", true)) return rc;
    ZG_REQUIRE(moments_dev != nullptr, ZG_ERR_INVALID_ARGUMENT, "fdm_moments: null moments");
    return moments_frames(img, 1, moments_dev, as_stream(stream));
}

int zg_fdm_compute_moments_frames(const zg_image *frames, uint32_t n, zg_fdm_moments *moments_dev, zg_stream stream) {
    if (const int rc = check_frames(frames, n, "fdm_moments_frames", true)) return rc;
    ZG_REQUIRE(moments_dev != nullptr || n == 0, ZG_ERR_INVALID_ARGUMENT, "fdm_moments_frames: null moments");
    return moments_frames(frames, n, moments_dev, as_stream(stream));
}

int zg_fdm_target_from_moments(const zg_fdm_moments *moments_dev, zg_fdm_target *target_dev, zg_stream stream) {
    ZG_REQUIRE(moments_dev != nullptr && target_dev != nullptr, ZG_ERR_INVALID_ARGUMENT, "fdm_target_from_moments: null pointer");
    return target_from_moments(moments_dev, target_dev, as_stream(stream));
}

int zg_fdm_transform_from_moments(const zg_fdm_moments *moments_dev, int pixel, const zg_fdm_target *target_dev, zg_fdm_transform *transform_dev,
                                  zg_stream stream) {
    ZG_REQUIRE(moments_dev != nullptr && target_dev != nullptr && transform_dev != nullptr, ZG_ERR_INVALID_ARGUMENT, "fdm_transform_from_moments: null pointer");
    ZG_REQUIRE(supported(pixel), ZG_ERR_UNSUPPORTED, "fdm_transform_from_moments: pixel type %d (fdm.zig:20)", pixel);
    return transform_from_moments(moments_dev, 1, pixel, target_dev, transform_dev, as_stream(stream));
}

int zg_fdm_transform_from_moments_frames(const zg_fdm_moments *moments_dev, uint32_t n, const zg_fdm_target *target_dev, zg_fdm_transform *transforms_dev,
                                         zg_stream stream) {
    ZG_REQUIRE(n == 0 || (moments_dev != nullptr && target_dev != nullptr && transforms_dev != nullptr), ZG_ERR_INVALID_ARGUMENT,
               "fdm_transform_from_moments_frames: null pointer");
    return transform_from_moments(moments_dev, n, -1, target_dev, transforms_dev, as_stream(stream));
}

int zg_fdm_target_host(int pixel, const double mean[3], const double cov[9], int is_gray, zg_fdm_target *out) {
    ZG_REQUIRE(mean != nullptr && cov != nullptr && out != nullptr, ZG_ERR_INVALID_ARGUMENT, "fdm_target_host: null pointer");
    ZG_REQUIRE(supported(pixel), ZG_ERR_UNSUPPORTED, "fdm_target_host: pixel type %d (fdm.zig:20)", pixel);
    zg_fdm::Target t;
    zg_fdm::Scratch k;
    zg_fdm::target_from_stats(mean, cov, pixel == ZG_PIXEL_U8 || is_gray != 0, &t, &k);
    target_out(t, pixel, out);
    return not_converged(t.status, "fdm_target_host");
}

int zg_fdm_transform_host(int pixel, const zg_fdm_target *target, const double mean[3], const double cov[9], zg_fdm_transform *out) {
    ZG_REQUIRE(target != nullptr && mean != nullptr && cov != nullptr && out != nullptr, ZG_ERR_INVALID_ARGUMENT, "fdm_transform_host: null pointer");
    ZG_REQUIRE(supported(pixel), ZG_ERR_UNSUPPORTED, "fdm_transform_host: pixel type %d (fdm.zig:20)", pixel);
    ZG_REQUIRE(pixel == target->pixel, ZG_ERR_INVALID_ARGUMENT, "fdm_transform_host: pixel type %d, the target's %d", pixel, target->pixel);
    zg_fdm::Target t;
    zg_fdm::Transform x;
    zg_fdm::Scratch k;
    target_in(target, t);
    zg_fdm::transform_from_stats(pixel, &t, mean, cov, &x, &k);
    transform_out(x, out);
    return not_converged(x.status, "fdm_transform_host");
}

int zg_fdm_stats_from_moments_host(const zg_fdm_moments *moments, int luminance, double mean[3], double cov[9]) {
    ZG_REQUIRE(moments != nullptr && mean != nullptr && cov != nullptr, ZG_ERR_INVALID_ARGUMENT, "fdm_stats_from_moments_host: null pointer");
    ZG_REQUIRE(moments->n < (1ull << 32), ZG_ERR_UNSUPPORTED, "fdm_stats_from_moments_host: n is 2^32 or more");
    moments_stats(*moments, luminance != 0, mean, cov);
    return ZG_OK;
}

int zg_fdm_apply(const zg_image *img, const zg_fdm_transform *transform_dev, zg_stream stream) {
    if (const int rc = check_frame(img, "fdm_apply", true)) return rc;
    ZG_REQUIRE(transform_dev != nullptr, ZG_ERR_INVALID_ARGUMENT, "fdm_apply: null transform");
    return apply_frames(img, 1, transform_dev, as_stream(stream));
}

int zg_fdm_apply_frames(const zg_image *frames, uint32_t n, const zg_fdm_transform *transforms_dev, zg_stream stream) {
    if (const int rc = check_frames(frames, n, "fdm_apply_frames", true)) return rc;
    ZG_REQUIRE(transforms_dev != nullptr || n == 0, ZG_ERR_INVALID_ARGUMENT, "fdm_apply_frames: null transforms");
    return apply_frames(frames, n, transforms_dev, as_stream(stream));
}

int zg_fdm_match(const zg_image *src, const zg_image *target, zg_stream stream) {
    ZG_REQUIRE(target != nullptr, ZG_ERR_INVALID_ARGUMENT, "fdm_match: null target");
    if (const int rc = check_match(src, 1, target, nullptr, "fdm_match", true)) return rc;
    return match_frames(src, 1, target, nullptr, as_stream(stream));
}

int zg_fdm_match_frames(const zg_image *frames, uint32_t n, const zg_image *target, const zg_fdm_target *prepared_dev, zg_stream stream) {
    if (const int rc = check_match(frames, n, target, prepared_dev, "fdm_match_frames", true)) return rc;
    return match_frames(frames, n, target, prepared_dev, as_stream(stream));
}

int zg_fdm_match_host(const zg_image *src, const zg_image *target) { return match_frames_host(src, 1, target); }

int zg_fdm_match_frames_host(const zg_image *frames, uint32_t n, const zg_image *target) { return match_frames_host(frames, n, target); }

} // extern "C"
