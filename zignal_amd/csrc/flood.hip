// flood.hip — Image(T).floodFill (reference src/image/flood_fill.zig:28-131) on the device, in place, bit for bit.
//
// The reference grows the region with a stack: it marks `visited` before it pushes and writes fill_value when it pops, so every pixel
// value it compares is an original one, and both distances are symmetric. The filled set is therefore the connected component of the
// seed in an undirected graph over adjacent pixels (seed mode: both ends within the threshold of the seed's value, the seed always;
// neighbor mode: the two ends within the threshold of each other), whatever the order of traversal. That component is labelled with
// the lock-free union-find of the edge detectors' hysteresis (zg_unionfind.h) in a fixed number of launches, with no convergence loop
// and no host synchronisation, so the call is asynchronous and recordable into a graph:
//   k_flood_links   one pass over the pixels writes a byte per pixel with the links it owns: E, S and, for 8-connectivity, SE and SW
//                   (the other directions are the same pairs seen from the other end). Seed mode reads the seed's value from the
//                   image here. Nothing reads a pixel value after this pass, which is what makes the in-place write safe.
//   k_flood_tile    a workgroup labels one 64 x 64 tile in LDS: a pixel starts under the first pixel of its horizontal run of E links
//                   (ballot + count-leading-zeros), the links to the row below are LDS unions; every pixel's label becomes the global
//                   index of its tile root (the smallest index of its tile component).
//   k_flood_border  the links that cross a tile edge (E across a vertical edge, S / SE / SW across a horizontal one, the diagonals across
//                   a vertical edge, and the single diagonal across a tile corner) are united through global memory; roots only ever
//                   move to smaller indices.
//   k_flood_fill    a pixel is written iff find(p) == find(seed); one atomic add per workgroup counts them.
// Distances (pixelDistance, :28-51) take no square root here: the host turns the threshold into one constant (bound() below).
#include "zg_common.h"
#include "zg_internal.h"
#include "zg_unionfind.h"

#include <cmath>
#include <cstring>

#pragma clang fp contract(off)

namespace zg {
namespace {

constexpr int FT = 64; // tile side
constexpr uint8_t LK_E = 1, LK_S = 2, LK_SE = 4, LK_SW = 8;
constexpr int MAX_SUM_SQ_U8 = 4 * 255 * 255;

struct FloodArgs {
    void *data;
    uint64_t stride; // pixels
    int rows, cols;
    uint32_t seed_row, seed_col;
    const uint32_t *seed_device; // (row, col) in place of the two above when not null
    double bound_f;              // float pixels: |a - b| <= bound_f, or the f64 sum of squares <= bound_f; -1: nothing joins
    int bound_i;                 // byte pixels: |a - b| <= bound_i, or the integer sum of squares <= bound_i; -1: nothing joins
    int eight, mode;
    uint8_t *links;
    int *label;
    uint32_t *count;
    uint32_t fill[4]; // fill_value's bytes
};

// the seed's index in the dense rows x cols numbering, or -1 when it is outside the image (only a device seed can be)
__device__ inline int seed_index(const FloodArgs &a) {
    uint32_t r = a.seed_row, c = a.seed_col;
    if (a.seed_device) {
        r = a.seed_device[0];
        c = a.seed_device[1];
    }
    return (r < (uint32_t)a.rows && c < (uint32_t)a.cols) ? (int)(r * (uint32_t)a.cols + c) : -1;
}

// pixelDistance(p, q) <= threshold, with the threshold already turned into the bound of the pixel type
template <int PIX> __device__ inline bool within(typename Px<PIX>::Vec p, typename Px<PIX>::Vec q, double bound_f, int bound_i) {
    using P = Px<PIX>;
    if constexpr (std::is_same<typename P::Elem, float>::value) {
        if constexpr (P::C == 1) {
            return fabs((double)p[0] - (double)q[0]) <= bound_f; // a NaN difference is not <= anything
        } else {
            double sum_sq = 0.0;
#pragma unroll
            for (int i = 0; i < P::C; ++i) {
                const double diff = (double)p[i] - (double)q[i];
                sum_sq += diff * diff;
            }
            return sum_sq <= bound_f;
        }
    } else {
        if constexpr (P::C == 1) {
            const int d = (int)p[0] - (int)q[0];
            return (d < 0 ? -d : d) <= bound_i;
        } else {
            int sum_sq = 0;
#pragma unroll
            for (int i = 0; i < P::C; ++i) {
                const int diff = (int)p[i] - (int)q[i];
                sum_sq += diff * diff;
            }
            return sum_sq <= bound_i;
        }
    }
}

template <int PIX> __global__ __launch_bounds__(256) void k_flood_links(FloodArgs a) {
    using P = Px<PIX>;
    const int n = a.rows * a.cols, cols = a.cols;
    const int p = (int)(blockIdx.x * 256u + threadIdx.x);
    if (p >= n) return;
    const int seed = seed_index(a);
    uint8_t bits = 0;
    if (seed >= 0) { // a seed outside the image: no links, and k_flood_fill writes nothing
        const int r = p / cols, c = p - r * cols;
        const bool has_e = c + 1 < cols, has_s = r + 1 < a.rows, has_w = c > 0;
        auto px = [&](int rr, int cc) { return P::load(a.data, (size_t)rr * a.stride + (size_t)cc); };
        if (a.mode == ZG_FLOOD_MODE_SEED) {
            const int sr = seed / cols;
            const typename P::Vec sv = px(sr, seed - sr * cols);
            auto pass = [&](int rr, int cc) { return rr * cols + cc == seed || within<PIX>(px(rr, cc), sv, a.bound_f, a.bound_i); };
            if (pass(r, c)) {
                if (has_e && pass(r, c + 1)) bits |= LK_E;
                if (has_s) {
                    if (pass(r + 1, c)) bits |= LK_S;
                    if (a.eight) {
                        if (has_e && pass(r + 1, c + 1)) bits |= LK_SE;
                        if (has_w && pass(r + 1, c - 1)) bits |= LK_SW;
                    }
                }
            }
        } else {
            const typename P::Vec v = px(r, c);
            auto near = [&](int rr, int cc) { return within<PIX>(px(rr, cc), v, a.bound_f, a.bound_i); };
            if (has_e && near(r, c + 1)) bits |= LK_E;
            if (has_s) {
                if (near(r + 1, c)) bits |= LK_S;
                if (a.eight) {
                    if (has_e && near(r + 1, c + 1)) bits |= LK_SE;
                    if (has_w && near(r + 1, c - 1)) bits |= LK_SW;
                }
            }
        }
    }
    a.links[p] = bits;
}

// One workgroup per tile (blockIdx.x = tile row * tiles_x + tile column), wave w owns rows 16 w .. 16 w + 15, a lane a column.
__global__ __launch_bounds__(256) void k_flood_tile(const uint8_t *links, int *label, int rows, int cols, int tiles_x) {
    __shared__ int lab[FT * FT];
    __shared__ uint8_t lk[FT][FT];
    const int t = threadIdx.x, lane = t & 63, w = t >> 6;
    const int ty = (int)blockIdx.x / tiles_x, tx = (int)blockIdx.x - ty * tiles_x;
    const int x0 = tx * FT, y0 = ty * FT;
    for (int i = t; i < FT * FT; i += 256) {
        const int r = i >> 6, c = i & 63;
        lk[r][c] = (y0 + r < rows && x0 + c < cols) ? links[(size_t)(y0 + r) * cols + x0 + c] : 0;
    }
    __syncthreads();
    // a pixel starts under the first pixel of its horizontal run: lane j and j + 1 are in one run iff j has its E link (lane 63's leaves the tile)
#pragma unroll
    for (int k = 0; k < 16; ++k) {
        const int r = w * 16 + k;
        const unsigned long long e = __ballot((lk[r][lane] & LK_E) != 0);
        const unsigned long long gaps = ~e & ((1ull << lane) - 1); // the lanes to my left without an E link
        const int start = gaps ? 64 - __clzll(gaps) : 0;
        lab[r * FT + lane] = r * FT + start;
    }
    __syncthreads();
    // the links to the row below, inside the tile
#pragma unroll 1
    for (int k = 0; k < 16; ++k) {
        const int r = w * 16 + k;
        if (r == FT - 1) break;
        const uint8_t bits = lk[r][lane];
        const int i = r * FT + lane;
        if (bits & LK_S) cc_unite(lab, i, i + FT);
        if ((bits & LK_SE) && lane < FT - 1) cc_unite(lab, i, i + FT + 1);
        if ((bits & LK_SW) && lane > 0) cc_unite(lab, i, i + FT - 1);
    }
    __syncthreads();
    // every pixel's label: the global index of its tile root (row-major in the tile and in the image alike: the smallest of its component)
    const bool col_ok = x0 + lane < cols;
#pragma unroll 4
    for (int k = 0; k < 16; ++k) {
        const int r = w * 16 + k;
        if (!col_ok || y0 + r >= rows) continue;
        const int root = cc_find(lab, r * FT + lane);
        label[(size_t)(y0 + r) * cols + x0 + lane] = (y0 + (root >> 6)) * cols + x0 + (root & 63);
    }
}

// A thread per pixel of a tile's last column that has a next tile column (j < nvb * rows), then per pixel of a tile's last row that has
// a next tile row. The last row takes every link to the row below, the diagonals across the tile's corners among them; the last column
// takes E and the diagonals that cross the vertical edge alone. A link bit is only ever set when its other end is inside the image.
__global__ __launch_bounds__(256) void k_flood_border(const uint8_t *links, int *label, int rows, int cols, int nvb, int nhb) {
    int j = (int)(blockIdx.x * 256u + threadIdx.x);
    if (j < nvb * rows) {
        const int b = j / rows, r = j - b * rows;
        const int x = b * FT + FT - 1; // x + 1 < cols by construction
        const int i = r * cols + x;
        const uint8_t bits = links[i];
        if (bits & LK_E) cc_unite_global(label, i, i + 1);
        if ((r & (FT - 1)) != FT - 1) { // otherwise the row below is another tile row's: the horizontal pass has these
            if (bits & LK_SE) cc_unite_global(label, i, i + cols + 1);
            if (links[i + 1] & LK_SW) cc_unite_global(label, i + 1, i + cols);
        }
        return;
    }
    j -= nvb * rows;
    if (j >= nhb * cols) return;
    const int b = j / cols, c = j - b * cols;
    const int y = b * FT + FT - 1; // y + 1 < rows by construction
    const int i = y * cols + c;
    const uint8_t bits = links[i];
    if (bits & LK_S) cc_unite_global(label, i, i + cols);
    if (bits & LK_SE) cc_unite_global(label, i, i + cols + 1);
    if (bits & LK_SW) cc_unite_global(label, i, i + cols - 1);
}

// PER pixels per thread: four for u8 (one 32-bit store when all four are filled, lie in one row and the address allows), one otherwise.
template <int PIX> __global__ __launch_bounds__(256) void k_flood_fill(FloodArgs a) {
    using P = Px<PIX>;
    constexpr int PER = PIX == ZG_PIXEL_U8 ? 4 : 1;
    __shared__ int s_root;
    __shared__ uint32_t s_count;
    const int seed = seed_index(a);
    if (seed < 0) return; // uniform
    if (threadIdx.x == 0) {
        s_root = cc_find(a.label, seed);
        s_count = 0;
    }
    __syncthreads();
    const int root = s_root, n = a.rows * a.cols, cols = a.cols;
    const long long p0 = ((long long)blockIdx.x * 256 + threadIdx.x) * PER;
    uint32_t filled = 0;
    bool mine[PER];
#pragma unroll
    for (int k = 0; k < PER; ++k) {
        mine[k] = p0 + k < n && cc_find(a.label, (int)(p0 + k)) == root;
        filled += mine[k];
    }
    if (filled) {
        typename P::Vec v;
        __builtin_memcpy(&v, a.fill, P::BYTES);
        const int r0 = (int)p0 / cols, c0 = (int)p0 - r0 * cols;
        bool done = false;
        if constexpr (PER == 4) {
            uint8_t *at = (uint8_t *)a.data + (size_t)r0 * a.stride + c0;
            if (filled == 4 && c0 + 3 < cols && ((uintptr_t)at & 3) == 0) {
                *(uint32_t *)at = (a.fill[0] & 0xffu) * 0x01010101u;
                done = true;
            }
        }
        if (!done) {
            int r = r0, c = c0;
#pragma unroll
            for (int k = 0; k < PER; ++k) {
                if (mine[k]) P::store(a.data, (size_t)r * a.stride + (size_t)c, v);
                if (++c == cols) { c = 0; ++r; }
            }
        }
        atomicAdd(&s_count, filled);
    }
    __syncthreads();
    if (threadIdx.x == 0 && a.count && s_count) atomicAdd(a.count, s_count);
}

// ---- host ------------------------------------------------------------------------------------------------------------------

bool have_device() { // asked once per process
    static const bool ok = [] {
        int n = 0;
        const bool r = hipGetDeviceCount(&n) == hipSuccess && n > 0;
        if (!r) (void)hipGetLastError();
        return r;
    }();
    return ok;
}

// S(t): the largest f64 whose correctly rounded square root is <= t, by bisection over the bit patterns of the non-negative doubles
// (their order is the order of their values). -1 for a negative or NaN t: no sum of squares is <= it.
double sqrt_bound(double t) {
    if (!(t >= 0.0)) return -1.0;
    if (t == 0.0) return 0.0; // -0.0 too
    if (std::isinf(t)) return t;
    uint64_t lo = 0, hi = 0x7ff0000000000000ull; // sqrt(lo) <= t < sqrt(hi)
    while (hi - lo > 1) {
        const uint64_t mid = lo + (hi - lo) / 2;
        double m;
        std::memcpy(&m, &mid, sizeof m);
        if (std::sqrt(m) <= t) lo = mid; else hi = mid;
    }
    double s;
    std::memcpy(&s, &lo, sizeof s);
    return s;
}

double bound(int pixel, double t) {
    switch (pixel) {
    case ZG_PIXEL_U8:
        if (!(t >= 0.0)) return -1.0;
        return t >= 255.0 ? 255.0 : std::floor(t) + 0.0; // -0.0 + 0.0 is 0.0
    case ZG_PIXEL_F32:
        if (!(t >= 0.0)) return -1.0;
        return t == 0.0 ? 0.0 : t;
    case ZG_PIXEL_RGB_U8: case ZG_PIXEL_RGBA_U8: {
        const double s = sqrt_bound(t);
        if (s < 0.0) return -1.0;
        return s >= (double)MAX_SUM_SQ_U8 ? (double)MAX_SUM_SQ_U8 : std::floor(s);
    }
    default:
        return sqrt_bound(t);
    }
}

const zg_flood_fill_options DEFAULTS{0.0, 4, ZG_FLOOD_MODE_SEED};

int check(const zg_image *img, uint32_t row, uint32_t col, bool seed_on_device, const void *fill_value, const zg_flood_fill_options *opt, bool device) {
    int rc;
    if ((rc = check_image(img, "flood_fill", device))) return rc;
    ZG_REQUIRE(fill_value != nullptr, ZG_ERR_INVALID_ARGUMENT, "flood_fill: null fill_value");
    ZG_REQUIRE(opt->connectivity == 4 || opt->connectivity == 8, ZG_ERR_INVALID_ARGUMENT, "flood_fill: connectivity %d (4 or 8)", opt->connectivity);
    ZG_REQUIRE(opt->mode == ZG_FLOOD_MODE_SEED || opt->mode == ZG_FLOOD_MODE_NEIGHBOR, ZG_ERR_INVALID_ARGUMENT, "flood_fill: mode %d (0 seed, 1 neighbor)",
               opt->mode);
    ZG_REQUIRE(seed_on_device || (row < img->rows && col < img->cols), ZG_ERR_INVALID_ARGUMENT,
               "flood_fill: seed (%u, %u) is outside the %u x %u image (error.OutOfBounds)", row, col, img->rows, img->cols); // :68
    ZG_REQUIRE((uint64_t)img->rows * img->cols < (1ull << 31), ZG_ERR_UNSUPPORTED, "flood_fill: %u x %u pixels, 2^31 or more", img->rows, img->cols);
    ZG_REQUIRE(have_device(), ZG_ERR_HIP, "flood_fill: no device");
    return ZG_OK;
}

int flood(const zg_image *img, uint32_t row, uint32_t col, const uint32_t *seed_device, const void *fill_value, const zg_flood_fill_options *opt,
          uint32_t *count, hipStream_t s) {
    int rc;
    if (count && (rc = fill_async(count, 0, sizeof(uint32_t), s))) return rc;
    const size_t n = (size_t)img->rows * img->cols;
    if (n == 0) return ZG_OK; // only a device seed gets here: it is outside
    FloodArgs a{};
    ScratchBlock sc(s); // scratch: [links][labels]
    sc.take(a.links, n);
    sc.take(a.label, n);
    if ((rc = sc.alloc())) return rc;
    a.data = img->data;
    a.stride = img->stride;
    a.rows = (int)img->rows;
    a.cols = (int)img->cols;
    a.seed_row = row;
    a.seed_col = col;
    a.seed_device = seed_device;
    const double b = bound(img->pixel, opt->threshold);
    a.bound_f = b;
    a.bound_i = pixel_is_float(img->pixel) ? -1 : (int)b;
    a.eight = opt->connectivity == 8;
    a.mode = opt->mode;
    a.count = count;
    std::memcpy(a.fill, fill_value, pixel_size(img->pixel));
    const unsigned pixel_blocks = (unsigned)((n + 255) / 256);
    rc = dispatch_pixel(img->pixel, [&](auto tag) {
        hipLaunchKernelGGL(k_flood_links<decltype(tag)::value>, dim3(pixel_blocks), dim3(256), 0, s, a);
        return launch_ok("k_flood_links");
    });
    if (rc) return rc;
    if ((rc = flood_label_components(a.links, a.label, img->rows, img->cols, s))) return rc;
    return dispatch_pixel(img->pixel, [&](auto tag) {
        constexpr int PIX = decltype(tag)::value;
        const unsigned per = PIX == ZG_PIXEL_U8 ? 4 : 1;
        hipLaunchKernelGGL(k_flood_fill<PIX>, dim3((unsigned)((n + 256 * per - 1) / (256 * per))), dim3(256), 0, s, a);
        return launch_ok("k_flood_fill");
    });
}

} // namespace

// k_flood_tile and k_flood_border over a plane of link bytes (zg_internal.h): what flood() above runs, and tracer.hip on the links of an edge map
int flood_label_components(const uint8_t *links, int *label, uint32_t rows, uint32_t cols, hipStream_t s) {
    int rc;
    const unsigned tiles_x = ceil_div(cols, (unsigned)FT), tiles_y = ceil_div(rows, (unsigned)FT);
    hipLaunchKernelGGL(k_flood_tile, dim3(tiles_x * tiles_y), dim3(256), 0, s, links, label, (int)rows, (int)cols, (int)tiles_x);
    if ((rc = launch_ok("k_flood_tile"))) return rc;
    const unsigned nvb = tiles_x - 1, nhb = tiles_y - 1;
    const size_t border = (size_t)nvb * rows + (size_t)nhb * cols;
    if (border) {
        hipLaunchKernelGGL(k_flood_border, dim3((unsigned)((border + 255) / 256)), dim3(256), 0, s, links, label, (int)rows, (int)cols, (int)nvb,
                           (int)nhb);
        if ((rc = launch_ok("k_flood_border"))) return rc;
    }
    return ZG_OK;
}

} // namespace zg

using namespace zg;

extern "C" {

uint32_t zg_flood_fill_tile(void) { return FT; }

int zg_flood_fill_bound_host(int pixel, double threshold, double *out) {
    ZG_REQUIRE(pixel_valid(pixel), ZG_ERR_INVALID_ARGUMENT, "flood_fill bound: invalid pixel type %d", pixel);
    ZG_REQUIRE(out != nullptr, ZG_ERR_INVALID_ARGUMENT, "flood_fill bound: null bound");
    *out = bound(pixel, threshold);
    return ZG_OK;
}

int zg_flood_fill(const zg_image *img, uint32_t row, uint32_t col, const uint32_t *seed_device, const void *fill_value, const zg_flood_fill_options *opt,
                  uint32_t *filled_count_device, zg_stream stream) {
    if (!opt) opt = &DEFAULTS;
    int rc;
    if ((rc = check(img, row, col, seed_device != nullptr, fill_value, opt, true))) return rc;
    return flood(img, row, col, seed_device, fill_value, opt, filled_count_device, as_stream(stream));
}

int zg_flood_fill_host(const zg_image *img, uint32_t row, uint32_t col, const void *fill_value, const zg_flood_fill_options *opt, uint32_t *filled_count) {
    if (!opt) opt = &DEFAULTS;
    int rc;
    if ((rc = check(img, row, col, false, fill_value, opt, false))) return rc;
    HostStage st;
    if ((rc = st.upload(img, true, true))) return rc;
    ScratchBlock sc;
    if ((rc = sc.alloc(256))) return rc;
    if ((rc = flood(&st.dev, row, col, nullptr, fill_value, opt, (uint32_t *)sc.p, nullptr))) return rc;
    uint32_t n = 0;
    if ((rc = download_pageable(&n, sc.p, sizeof n, nullptr))) return rc; // waits for the stream
    if (filled_count) *filled_count = n;
    return st.finish();
}

} // extern "C"
