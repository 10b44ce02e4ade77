// seam.hip — the reference's seam_carve example (examples/src/seam_carving.zig:22-144) on the device, bit for bit: computeEnergy,
// computeSeam, removeSeam, and the iteration sobel -> energy -> seam -> removal that never leaves the device.
//
// Everything after Image.sobel (edges.hip, reached through sobel_frames) is integer work with a fixed tie order:
//   k_seam_energy     the dynamic programme down the rows, as banded trapezoids. A launch covers a band of SB rows; a wave owns a window of
//                     SW = 4 * 64 columns, four per lane, of which the middle SS = SW - 2 SB are its strip. It reads the SW sums of the row
//                     above the band and all of the band's edge bytes (SB packed words a lane: every load of the band is in flight before
//                     the first sum), then walks the SB rows in registers; a lane's outer columns come from its neighbours by a
//                     cross-lane move. The window's outer SB columns a side lose one column of validity per row (the dependency cone is
//                     one column wide a row) and are never stored. The frame's own borders are exact inside the window: a column outside
//                     the frame holds the largest u32, which is computeEnergy's skip at column -1, and also its rule at column `cols`
//                     (that one reads column cols - 1 again, the centre, so it never lowers the minimum). No workgroup waits for
//                     another: the bands are separate launches.
//   k_seam_jumps,     computeSeam. The walk up is rows - 1 dependent steps, so it is cut into bands of FR rows. k_seam_jumps takes every
//   k_seam_walk       column of a band's bottom row to the column reached at its top (FR steps in LDS, a lane a column, all bands at
//                     once); k_seam_walk, a workgroup a band, finds the bottom row's first minimum (a reduction over (sum, column)
//                     keys), follows the jumps below its band with one lane, and takes its band's own FR steps in LDS for the one
//                     column that matters. The depth is FR + rows / FR + FR steps instead of rows. The rule is computeSeam's, which
//                     is not the argmin computeEnergy took: the centre wins ties, then the left.
//   k_seam_remove     a lane per destination pixel, dst[r][c] = src[r][c + (c >= seam[r])], any pixel type.
//   k_seam_transpose  an LDS tile transpose, for the horizontal axis (the library's own definition: carve the transposed frame).
#include "zg_common.h"
#include "zg_internal.h"

#include <cstdlib>
#include <cstring>

namespace zg {
namespace {

constexpr int SB = 32;           // rows of a band
constexpr int SW = 256;          // columns of a wave's window: four a lane
constexpr int SS = SW - 2 * SB;  // columns of a strip: what a wave stores
constexpr int FR = 32;           // rows the walk stages in LDS at a time
constexpr int FWIN = 2 * FR + 1; // and their columns
constexpr uint32_t NO_SUM = 0xffffffffu;

__device__ inline uint32_t min3(uint32_t a, uint32_t b, uint32_t c) { return min(min(a, b), c); }

// blockIdx.x is the strip, one wave a workgroup. energy is rows * cols packed words; r0 >= 1 is the band's first row; `first`: the row above
// is row 0, which comes from the edge map and is stored too. The two planes never share bytes (__restrict__): without that promise every
// edge load waits for the stores of the row before it, a memory latency a row.
__global__ __launch_bounds__(64) void k_seam_energy(const uint8_t *__restrict__ edges, uint64_t stride, uint32_t *__restrict__ energy, int rows, int cols,
                                                    int r0, int first) {
    const int lane = (int)threadIdx.x;
    const int out0 = (int)blockIdx.x * SS;
    const int x = out0 - SB + lane * 4; // the first of this lane's four columns
    const bool stores = lane >= SB / 4 && lane < (SB + SS) / 4;
    const int nr = min(SB, rows - r0);
    // The band's edge bytes of the four columns, a word a row, without a branch: one 32-bit load a row from an address clamped into the row
    // (and the row clamped into the frame), shifted so that byte i is column x + i. What a clamp brought in belongs to a column or a row
    // outside the frame, and those are never summed. Every load of the band is issued before the first sum is taken.
    uint32_t e[SB];
    uint32_t p[4]; // the sums of the row above, from clamped addresses in the same way; the columns outside the frame are set below
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int xc = min(max(x + i, 0), cols - 1);
        p[i] = first ? (uint32_t)edges[xc] : energy[(size_t)(r0 - 1) * cols + xc];
    }
    if (cols >= 4) {
        const int xb = min(max(x, 0), cols - 4), d = min(max(x - xb, -4), 4);
        const int shr = d > 0 ? 8 * d : 0, shl = d < 0 ? -8 * d : 0;
#pragma unroll
        for (int k = 0; k < SB; ++k) __builtin_memcpy(&e[k], edges + (size_t)min(r0 + k, rows - 1) * stride + xb, 4);
        asm volatile("" ::: "memory"); // the loads stay above this line and their first use below it: one wait for all of them
#pragma unroll
        for (int k = 0; k < SB; ++k) e[k] = (uint32_t)(((uint64_t)e[k] >> shr) << shl);
    } else { // a frame narrower than a word
#pragma unroll
        for (int k = 0; k < SB; ++k) {
            const uint8_t *row = edges + (size_t)min(r0 + k, rows - 1) * stride;
            uint32_t w = 0;
#pragma unroll
            for (int i = 0; i < 4; ++i) w |= (uint32_t)row[min(max(x + i, 0), cols - 1)] << (8 * i);
            e[k] = w;
        }
    }
#pragma unroll
    for (int i = 0; i < 4; ++i)
        if (x + i < 0 || x + i >= cols) p[i] = NO_SUM;
    if (first && stores) {
#pragma unroll
        for (int i = 0; i < 4; ++i)
            if (x + i < cols) energy[x + i] = p[i];
    }
#pragma unroll
    for (int k = 0; k < SB; ++k) {
        if (k < nr) { // uniform
            uint32_t left = __shfl_up(p[3], 1), right = __shfl_down(p[0], 1);
            if (lane == 0) left = NO_SUM;
            if (lane == 63) right = NO_SUM;
            const uint32_t q0 = min3(left, p[0], p[1]), q1 = min3(p[0], p[1], p[2]), q2 = min3(p[1], p[2], p[3]), q3 = min3(p[2], p[3], right);
            const uint32_t q[4] = {q0, q1, q2, q3};
            uint32_t *out = energy + (size_t)(r0 + k) * cols;
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const int xi = x + i;
                const bool in = xi >= 0 && xi < cols;
                p[i] = in ? q[i] + ((e[k] >> (8 * i)) & 0xffu) : NO_SUM; // an in-frame column's centre is a real sum: q is one too
                if (stores && in) out[xi] = p[i];
            }
        }
    }
}

// The bottom row's first minimum, by a whole workgroup of 256: the smallest (sum, column) key. Every thread gets it.
__device__ inline int first_minimum(const uint32_t *last, int cols) {
    __shared__ unsigned long long wave_best[4];
    const int t = (int)threadIdx.x;
    unsigned long long best = ~0ull;
    for (int c = t; c < cols; c += 256) {
        const unsigned long long key = ((unsigned long long)last[c] << 32) | (uint32_t)c;
        best = key < best ? key : best;
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        const unsigned long long other = __shfl_down(best, off);
        best = other < best ? other : best;
    }
    if ((t & 63) == 0) wave_best[t >> 6] = best;
    __syncthreads();
    best = wave_best[0];
    for (int k = 1; k < 4; ++k) best = wave_best[k] < best ? wave_best[k] : best;
    return (int)(uint32_t)best;
}

// One step of computeSeam's walk in a row of sums: `row` is indexed by j = the column s moved into the row's window. The centre is the
// start, the left replaces it when strictly below, the right when strictly below whichever is current; the centre's own turn in between
// cannot win, and column `cols` stands for cols - 1, the centre again. Returns the move, -1 / 0 / +1.
template <typename Row> __device__ inline int seam_step(const Row &row, int j, int s, int cols) {
    int b = j;
    if (s >= 1 && row[j - 1] < row[b]) b = j - 1;
    if (s + 1 < cols && row[j + 1] < row[b]) b = j + 1;
    return b - j;
}

// The walk is rows - 1 dependent steps, so it is cut into bands of FR steps, counted from the bottom row: band j starts at row
// t = rows - 1 - j FR and ends FR rows higher. k_seam_jumps takes every column of a band's bottom row to the column the walk reaches at
// the band's top: blockIdx.y is the band, blockIdx.x a tile of JT columns, whose FR rows by JT + 2 FR columns of sums are staged in LDS
// (a walk moves one column a row at the most), and a lane a column takes the FR steps there. The last band needs no jumps.
constexpr int JT = 192;
__global__ __launch_bounds__(256) void k_seam_jumps(const uint32_t *__restrict__ energy, int rows, int cols, uint32_t *__restrict__ jumps) {
    __shared__ uint32_t win[FR][JT + 2 * FR];
    const int t = (int)threadIdx.x;
    const int bottom = rows - 1 - (int)blockIdx.y * FR; // > FR by the grid's construction
    const int w0 = (int)blockIdx.x * JT - FR;           // the window's first column
#pragma unroll 8
    for (int k = 0; k < FR; ++k) {
        const int xx = w0 + t;
        win[k][t] = (xx >= 0 && xx < cols) ? energy[(size_t)(bottom - 1 - k) * cols + xx] : 0u;
    }
    __syncthreads();
    const int c = w0 + FR + t;
    if (t >= JT || c >= cols) return;
    int s = c; // after k steps |s - c| <= k, and a step reads s - 1 .. s + 1: inside the window
    for (int k = 0; k < FR; ++k) s += seam_step(win[k], s - w0, s, cols);
    jumps[(size_t)blockIdx.y * cols + c] = (uint32_t)s;
}

// blockIdx.x is the band. The workgroup finds the bottom row's first minimum (every band does: a row of loads), one lane follows the
// jumps of the bands below its own, and then the band's own FR steps are taken as in k_seam_jumps, for the one column that matters:
// FR rows by 2 FR + 1 columns in LDS, one lane walking, the FR entries stored together.
__global__ __launch_bounds__(256) void k_seam_walk(const uint32_t *__restrict__ energy, int rows, int cols, const uint32_t *__restrict__ jumps,
                                                   uint32_t *__restrict__ seam) {
    __shared__ uint32_t win[FR][FWIN];
    __shared__ uint32_t s_seam[FR];
    __shared__ int s_col;
    const int t = (int)threadIdx.x, band = (int)blockIdx.x;
    const int first = first_minimum(energy + (size_t)(rows - 1) * cols, cols);
    if (t == 0) {
        int c = first;
        for (int j = 0; j < band; ++j) c = (int)jumps[(size_t)j * cols + c];
        s_col = c;
        if (band == 0) seam[rows - 1] = (uint32_t)first;
    }
    __syncthreads();
    const int bottom = rows - 1 - band * FR, nr = min(FR, bottom), c0 = s_col;
    for (int i = t; i < nr * FWIN; i += 256) {
        const int k = i / FWIN, j = i - k * FWIN;
        const int xx = c0 - FR + j;
        win[k][j] = (xx >= 0 && xx < cols) ? energy[(size_t)(bottom - 1 - k) * cols + xx] : 0u;
    }
    __syncthreads();
    if (t == 0) {
        int s = c0;
        for (int k = 0; k < nr; ++k) {
            s += seam_step(win[k], s - c0 + FR, s, cols);
            s_seam[k] = (uint32_t)s;
        }
    }
    __syncthreads();
    if (t < nr) seam[bottom - 1 - t] = s_seam[t];
}

// The baseline the banded walk is measured against: one lane chases the sums through global memory, a dependent load a row.
__global__ __launch_bounds__(256) void k_seam_walk_plain(const uint32_t *energy, int rows, int cols, uint32_t *seam) {
    const int first = first_minimum(energy + (size_t)(rows - 1) * cols, cols);
    if (threadIdx.x != 0) return;
    int s = first;
    seam[rows - 1] = (uint32_t)s;
    for (int r = rows - 2; r >= 0; --r) {
        const uint32_t *row = energy + (size_t)r * cols;
        s += seam_step(row, s, s, cols);
        seam[r] = (uint32_t)s;
    }
}

template <int PIX> __global__ __launch_bounds__(256) void k_seam_remove(DImg src, DImg dst, const uint32_t *seam) {
    using P = Px<PIX>;
    const int r = grid_row();
    const int c = (int)(blockIdx.x * 256u + threadIdx.x);
    if (r >= dst.rows || c >= dst.cols) return;
    const uint32_t skip = (uint32_t)c >= seam[r] ? 1u : 0u;
    P::store(dst.data, (size_t)r * dst.stride + (size_t)c, P::load(src.data, (size_t)r * src.stride + (size_t)c + skip));
}

// dst[c][r] = src[r][c]; blockIdx.x numbers the 32 x 32 tiles of src row-major
template <int PIX> __global__ __launch_bounds__(256) void k_seam_transpose(DImg src, DImg dst, int tiles_x) {
    using P = Px<PIX>;
    __shared__ typename P::Vec tile[32][33];
    const int tx = (int)threadIdx.x & 31, ty = (int)threadIdx.x >> 5;
    const int by = (int)blockIdx.x / tiles_x, bx = (int)blockIdx.x - by * tiles_x;
    const int r0 = by * 32, c0 = bx * 32;
    for (int j = ty; j < 32; j += 8)
        if (r0 + j < src.rows && c0 + tx < src.cols) tile[j][tx] = P::load(src.data, (size_t)(r0 + j) * src.stride + (size_t)(c0 + tx));
    __syncthreads();
    for (int j = ty; j < 32; j += 8)
        if (c0 + j < src.cols && r0 + tx < src.rows) P::store(dst.data, (size_t)(c0 + j) * dst.stride + (size_t)(r0 + tx), tile[tx][j]);
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

bool fits_31_bits(uint32_t rows, uint32_t cols) { return (uint64_t)rows * cols < (1ull << 31); }

int energy_impl(const zg_image *edges, uint32_t *energy, hipStream_t s) {
    if (edges->rows == 0 || edges->cols == 0) return ZG_OK;
    const unsigned strips = ceil_div(edges->cols, (unsigned)SS);
    const int rows = (int)edges->rows;
    int r0 = 1, first = 1;
    do { // a frame of one row still takes the launch that stores row 0
        hipLaunchKernelGGL(k_seam_energy, dim3(strips), dim3(64), 0, s, (const uint8_t *)edges->data, (uint64_t)edges->stride, energy, rows, (int)edges->cols, r0,
                           first);
        if (const int rc = launch_ok("k_seam_energy")) return rc;
        r0 += SB;
        first = 0;
    } while (r0 < rows);
    return ZG_OK;
}

int find_impl(const uint32_t *energy, uint32_t rows, uint32_t cols, uint32_t *seam, hipStream_t s) {
    // for one round (tuning hooks): ZIGNAL_HIP_SEAM_PLAIN_WALK=1 takes the one-lane walk through global memory instead
    static const bool plain = [] {
        const char *v = getenv("ZIGNAL_HIP_SEAM_PLAIN_WALK");
        return v && v[0] == '1';
    }();
    const unsigned bands = rows > 1 ? ceil_div(rows - 1, (unsigned)FR) : 1; // a map of one row still takes the launch that stores its minimum
    if (plain || bands - 1 > GRID_Y_MAX) { // more than two million rows: the bands do not fit a grid, and such a map is a few columns wide
        hipLaunchKernelGGL(k_seam_walk_plain, dim3(1), dim3(256), 0, s, energy, (int)rows, (int)cols, seam);
        return launch_ok("k_seam_walk_plain");
    }
    ScratchBlock sc(s); // scratch: [jumps], a word a column for every band but the last
    uint32_t *jumps = nullptr;
    if (bands > 1) {
        sc.take(jumps, (size_t)(bands - 1) * cols);
        if (const int rc = sc.alloc()) return rc;
        hipLaunchKernelGGL(k_seam_jumps, dim3(ceil_div(cols, (unsigned)JT), bands - 1), dim3(256), 0, s, energy, (int)rows, (int)cols, jumps);
        if (const int rc = launch_ok("k_seam_jumps")) return rc;
    }
    hipLaunchKernelGGL(k_seam_walk, dim3(bands), dim3(256), 0, s, energy, (int)rows, (int)cols, (const uint32_t *)jumps, seam);
    return launch_ok("k_seam_walk");
}

int remove_impl(const zg_image *src, const uint32_t *seam, const zg_image *dst, hipStream_t s) {
    if (dst->rows == 0 || dst->cols == 0) return ZG_OK;
    return dispatch_pixel(src->pixel, [&](auto tag) {
        hipLaunchKernelGGL(k_seam_remove<decltype(tag)::value>, row_grid(ceil_div(dst->cols, 256u), dst->rows), dim3(256), 0, s, dimg(src), dimg(dst), seam);
        return launch_ok("k_seam_remove");
    });
}

int transpose_impl(const zg_image *src, const zg_image *dst, hipStream_t s) {
    const unsigned tiles_x = ceil_div(src->cols, 32u), tiles_y = ceil_div(src->rows, 32u);
    return dispatch_pixel(src->pixel, [&](auto tag) {
        hipLaunchKernelGGL(k_seam_transpose<decltype(tag)::value>, dim3(tiles_x * tiles_y), dim3(256), 0, s, dimg(src), dimg(dst), (int)tiles_x);
        return launch_ok("k_seam_transpose");
    });
}

zg_image packed(void *data, uint32_t rows, uint32_t cols, int pixel) { return zg_image{data, cols, rows, cols, pixel}; }

// n iterations on device images; the frame of iteration k comes from src (k = 0) or a working frame and goes to the other working
// frame or, at the end, to dst
int carve_columns(const zg_image *src, const zg_image *dst, uint32_t n, uint32_t *seams, hipStream_t s) {
    const uint32_t rows = src->rows, cols = src->cols;
    const size_t px = pixel_size(src->pixel);
    ScratchBlock sc(s); // scratch: [frame a][frame b][edges][energy][seam]
    char *frame[2] = {nullptr, nullptr};
    uint8_t *edges = nullptr;
    uint32_t *energy = nullptr, *seam = nullptr;
    if (n >= 2) sc.take(frame[0], (size_t)rows * (cols - 1) * px);
    if (n >= 3) sc.take(frame[1], (size_t)rows * (cols - 2) * px);
    sc.take(edges, (size_t)rows * cols);
    sc.take(energy, (size_t)rows * cols);
    if (!seams) sc.take(seam, rows);
    int rc;
    if ((rc = sc.alloc())) return rc;
    zg_image in = *src;
    for (uint32_t k = 0; k < n; ++k) {
        const zg_image out = k + 1 == n ? *dst : packed(frame[k & 1], rows, cols - k - 1, src->pixel);
        const zg_image e = packed(edges, rows, in.cols, ZG_PIXEL_U8);
        uint32_t *seam_k = seams ? seams + (size_t)k * rows : seam;
        if ((rc = sobel_frames(FrameBatch{&in, &e}, s))) return rc;
        if ((rc = energy_impl(&e, energy, s))) return rc;
        if ((rc = find_impl(energy, rows, in.cols, seam_k, s))) return rc;
        if ((rc = remove_impl(&in, seam_k, &out, s))) return rc;
        in = out;
    }
    return ZG_OK;
}

int carve_impl(const zg_image *src, const zg_image *dst, uint32_t n, int axis, uint32_t *seams, hipStream_t s) {
    if (axis == ZG_SEAM_VERTICAL) return carve_columns(src, dst, n, seams, s);
    const size_t px = pixel_size(src->pixel);
    ScratchBlock sc(s); // scratch: [the transposed frame][the transposed result]
    char *turned = nullptr, *carved = nullptr;
    sc.take(turned, (size_t)src->rows * src->cols * px);
    sc.take(carved, (size_t)dst->rows * dst->cols * px);
    int rc;
    if ((rc = sc.alloc())) return rc;
    const zg_image t = packed(turned, src->cols, src->rows, src->pixel), c = packed(carved, dst->cols, dst->rows, src->pixel);
    if ((rc = transpose_impl(src, &t, s))) return rc;
    if ((rc = carve_columns(&t, &c, n, seams, s))) return rc;
    return transpose_impl(&c, dst, s);
}

// ---- the argument checks: everything is decided here, before anything is enqueued, and the missing device comes last

int check_energy(const zg_image *edges, const uint32_t *energy, bool device) {
    int rc;
    if ((rc = check_image(edges, "seam_energy", device))) return rc;
    ZG_REQUIRE(edges->pixel == ZG_PIXEL_U8, ZG_ERR_INVALID_ARGUMENT, "seam_energy: the edge map is Image(u8)");
    ZG_REQUIRE(energy != nullptr, ZG_ERR_INVALID_ARGUMENT, "seam_energy: null energy");
    ZG_REQUIRE(fits_31_bits(edges->rows, edges->cols), ZG_ERR_UNSUPPORTED, "seam_energy: %u x %u pixels, 2^31 or more", edges->rows, edges->cols);
    ZG_REQUIRE(have_device(), ZG_ERR_HIP, "seam_energy: no device");
    return ZG_OK;
}

int check_find(const uint32_t *energy, uint32_t rows, uint32_t cols, const uint32_t *seam) {
    ZG_REQUIRE(energy != nullptr && seam != nullptr, ZG_ERR_INVALID_ARGUMENT, "seam_find: null %s", energy ? "seam" : "energy");
    ZG_REQUIRE(rows >= 1 && cols >= 1, ZG_ERR_INVALID_ARGUMENT, "seam_find: an empty %u x %u map has no seam", rows, cols);
    ZG_REQUIRE(fits_31_bits(rows, cols), ZG_ERR_UNSUPPORTED, "seam_find: %u x %u sums, 2^31 or more", rows, cols);
    ZG_REQUIRE(have_device(), ZG_ERR_HIP, "seam_find: no device");
    return ZG_OK;
}

int check_remove(const zg_image *src, const uint32_t *seam, const zg_image *dst, bool device) {
    int rc;
    if ((rc = check_image(src, "seam_remove: src", device)) || (rc = check_image(dst, "seam_remove: dst", device))) return rc;
    ZG_REQUIRE(seam != nullptr, ZG_ERR_INVALID_ARGUMENT, "seam_remove: null seam");
    ZG_REQUIRE(src->pixel == dst->pixel, ZG_ERR_INVALID_ARGUMENT, "seam_remove: pixel types %d and %d differ", src->pixel, dst->pixel);
    ZG_REQUIRE(src->cols >= 1, ZG_ERR_INVALID_ARGUMENT, "seam_remove: the image has no column to lose");
    ZG_REQUIRE(dst->rows == src->rows && dst->cols == src->cols - 1, ZG_ERR_DIMENSION_MISMATCH, "seam_remove: %ux%u needs a %ux%u destination, got %ux%u",
               src->rows, src->cols, src->rows, src->cols - 1, dst->rows, dst->cols);
    ZG_REQUIRE(!spans_overlap(src, dst), ZG_ERR_INVALID_ARGUMENT, "seam_remove: src and dst share bytes");
    ZG_REQUIRE(have_device(), ZG_ERR_HIP, "seam_remove: no device");
    return ZG_OK;
}

int check_carve(const zg_image *src, const zg_image *dst, uint32_t n, int axis, const zg_image *energy_source, bool device) {
    int rc;
    if ((rc = check_image(src, "seam_carve: src", device)) || (rc = check_image(dst, "seam_carve: dst", device))) return rc;
    ZG_REQUIRE(src->pixel == dst->pixel, ZG_ERR_INVALID_ARGUMENT, "seam_carve: pixel types %d and %d differ", src->pixel, dst->pixel);
    ZG_REQUIRE(axis == ZG_SEAM_VERTICAL || axis == ZG_SEAM_HORIZONTAL, ZG_ERR_INVALID_ARGUMENT, "seam_carve: axis %d (0 vertical, 1 horizontal)", axis);
    const bool v = axis == ZG_SEAM_VERTICAL;
    const uint32_t along = v ? src->rows : src->cols, across = v ? src->cols : src->rows;
    ZG_REQUIRE(along >= 1, ZG_ERR_INVALID_ARGUMENT, "seam_carve: an empty %u x %u image", src->rows, src->cols);
    ZG_REQUIRE(n >= 1 && n < across, ZG_ERR_INVALID_ARGUMENT, "seam_carve: n = %u seams of a %u x %u image (1 <= n < %u)", n, src->rows, src->cols, across);
    ZG_REQUIRE(energy_source == nullptr, ZG_ERR_UNSUPPORTED, "seam_carve: energy_source is reserved and must be NULL");
    const uint32_t want_rows = v ? src->rows : src->rows - n, want_cols = v ? src->cols - n : src->cols;
    ZG_REQUIRE(dst->rows == want_rows && dst->cols == want_cols, ZG_ERR_DIMENSION_MISMATCH, "seam_carve: %ux%u less %u seams is %ux%u, dst is %ux%u", src->rows,
               src->cols, n, want_rows, want_cols, dst->rows, dst->cols);
    ZG_REQUIRE(fits_31_bits(src->rows, src->cols), ZG_ERR_UNSUPPORTED, "seam_carve: %u x %u pixels, 2^31 or more", src->rows, src->cols);
    ZG_REQUIRE(!spans_overlap(src, dst), ZG_ERR_INVALID_ARGUMENT, "seam_carve: src and dst share bytes");
    ZG_REQUIRE(have_device(), ZG_ERR_HIP, "seam_carve: no device");
    return ZG_OK;
}

} // namespace
} // namespace zg

using namespace zg;

extern "C" {

uint32_t zg_seam_band_rows(void) { return SB; }
uint32_t zg_seam_strip_cols(void) { return SS; }

int zg_seam_energy(const zg_image *edges, uint32_t *energy, zg_stream stream) {
    if (const int rc = check_energy(edges, energy, true)) return rc;
    return energy_impl(edges, energy, as_stream(stream));
}

int zg_seam_find(const uint32_t *energy, uint32_t rows, uint32_t cols, uint32_t *seam, zg_stream stream) {
    if (const int rc = check_find(energy, rows, cols, seam)) return rc;
    return find_impl(energy, rows, cols, seam, as_stream(stream));
}

int zg_seam_remove(const zg_image *src, const uint32_t *seam, const zg_image *dst, zg_stream stream) {
    if (const int rc = check_remove(src, seam, dst, true)) return rc;
    return remove_impl(src, seam, dst, as_stream(stream));
}

int zg_seam_carve(const zg_image *src, const zg_image *dst, uint32_t n, int axis, const zg_image *energy_source, uint32_t *seams_device, zg_stream stream) {
    if (const int rc = check_carve(src, dst, n, axis, energy_source, true)) return rc;
    return carve_impl(src, dst, n, axis, seams_device, as_stream(stream));
}

int zg_seam_energy_host(const zg_image *edges, uint32_t *energy) {
    int rc;
    if ((rc = check_energy(edges, energy, false))) return rc;
    const size_t n = (size_t)edges->rows * edges->cols;
    if (n == 0) return ZG_OK;
    HostStage st;
    if ((rc = st.upload(edges, true, false))) return rc;
    ScratchBlock sc;
    if ((rc = sc.alloc(n * sizeof(uint32_t)))) return rc;
    if ((rc = energy_impl(&st.dev, (uint32_t *)sc.p, nullptr))) return rc;
    return download_pageable(energy, sc.p, n * sizeof(uint32_t), nullptr); // waits for the stream
}

int zg_seam_find_host(const uint32_t *energy, uint32_t rows, uint32_t cols, uint32_t *seam) {
    int rc;
    if ((rc = check_find(energy, rows, cols, seam))) return rc;
    ScratchBlock sc;
    uint32_t *e = nullptr, *sm = nullptr;
    sc.take(e, (size_t)rows * cols);
    sc.take(sm, rows);
    if ((rc = sc.alloc())) return rc;
    if ((rc = upload_pageable(e, energy, (size_t)rows * cols * sizeof(uint32_t), nullptr))) return rc;
    if ((rc = find_impl(e, rows, cols, sm, nullptr))) return rc;
    return download_pageable(seam, sm, (size_t)rows * sizeof(uint32_t), nullptr);
}

int zg_seam_remove_host(const zg_image *src, const uint32_t *seam, const zg_image *dst) {
    int rc;
    if ((rc = check_remove(src, seam, dst, false))) return rc;
    if (dst->rows == 0 || dst->cols == 0) return ZG_OK;
    ScratchBlock sc;
    if ((rc = sc.alloc((size_t)src->rows * sizeof(uint32_t)))) return rc;
    if ((rc = upload_pageable(sc.p, seam, (size_t)src->rows * sizeof(uint32_t), nullptr))) return rc;
    return host_src_dst(src, dst, [&](const zg_image *a, const zg_image *b) { return remove_impl(a, (const uint32_t *)sc.p, b, nullptr); });
}

int zg_seam_carve_host(const zg_image *src, const zg_image *dst, uint32_t n, int axis, const zg_image *energy_source, uint32_t *seams) {
    int rc;
    if ((rc = check_carve(src, dst, n, axis, energy_source, false))) return rc;
    const size_t words = (size_t)n * (axis == ZG_SEAM_VERTICAL ? src->rows : src->cols);
    ScratchBlock sc;
    if (seams && (rc = sc.alloc(words * sizeof(uint32_t)))) return rc;
    rc = host_src_dst(src, dst, [&](const zg_image *a, const zg_image *b) { return carve_impl(a, b, n, axis, (uint32_t *)sc.p, nullptr); });
    if (rc || !seams) return rc;
    return download_pageable(seams, sc.p, words * sizeof(uint32_t), nullptr);
}

} // extern "C"
