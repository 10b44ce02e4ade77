// fast.hip — Fast.detect (reference src/features/Fast.zig:38-254) on the device, bit for bit.
//
// The detector is integer arithmetic from end to end (compares, a sum of at most 16 x 255, compares of those sums), so the
// device list equals the reference's byte for byte, order included. Three launches per call (after a memset of a few words), none of
// which the host waits on:
//   1. k_fast_detect   64 x 16 candidates per workgroup from an LDS tile with a 3-pixel halo: bright / dark masks as bits, the
//                      quick reject (:81-102), the arc by shifted ANDs (:104-132), the score (:135-152). Writes a u16 score map
//                      over the candidate rectangle (0 = no corner; every corner scores 3..4080) and, with NMS, folds the smallest
//                      row and column of any corner into two device words (one integer atomicMin per workgroup: order-free).
//   2. k_fast_nms_count  NMS (:155-254): one workgroup per 20 x 20 cell of the reference's grid, anchored at those two words,
//                      over the cell grid's upper bound; a corner is kept iff none of its 68 neighbours at dx^2 + dy^2 < 25 has a
//                      strictly greater score. Counts the kept corners per cell, and adds the count into its GROUP's total
//                      (a row of cells; integer atomics: order-free).   (no NMS: k_fast_row_count, corners per row, 64 rows a group)
//   3. k_fast_nms_write  a cell with kept corners: its offset in the list is the sum of the group totals before its group plus
//                      the counts of the cells before it in its group (a block-wide sum, no scan launch: a one-workgroup scan
//                      over 42 K cells was 62 us of latency); then its kept corners, sorted by the unique key
//                      (4095 - score) << 9 | local raster index (descending response, ties in raster order: std.mem.sort is
//                      stable, :218), are written there; slots past `capacity` are skipped; workgroup 0 writes *count.
//                      (no NMS: k_fast_row_write, raster-order compaction of a row)
// A batch of images (a pyramid's levels) runs the same three launches: a job table in the kernel arguments, workgroups of all
// jobs in one grid, each finding its job from the per-stage first-workgroup table.
#include "zg_internal.h"
#include "zg_scan.h"

#include <algorithm>
#include <vector>

#pragma clang fp contract(off)

namespace zg {
namespace {

constexpr int FAST_MAX_JOBS = 8;                 // jobs per launch: ORB's default pyramid (orb.zig nlevels = 8)
constexpr int DET_W = 64, DET_H = 16;            // candidates per k_fast_detect workgroup (64 x 4 threads, four rows each)
constexpr int DET_LW = DET_W + 6, DET_LH = DET_H + 6;
constexpr int CELL = 20;                         // the reference's grid_size (:172)
constexpr int NMS_R = 4;                         // dx^2 + dy^2 < 25 reaches 4 pixels
constexpr int CELL_L = CELL + 2 * NMS_R;

struct FastJob {
    const uint8_t *src;
    uint64_t stride;          // pixels
    int32_t rows, cols;
    int32_t ih, iw;           // candidate rectangle: rows 3 .. rows - 4, cols 3 .. cols - 4 (:45-52)
    uint32_t threshold, capacity;
    uint16_t *score;          // ih x iw
    uint32_t *minrc;          // {min row, min col} of the corners, candidate coordinates; UINT32_MAX = none
    uint32_t *counts;         // per cell (NMS) or per candidate row
    uint32_t *gtot;           // per group of `group` consecutive cells: the sum of their counts (zeroed before the call)
    zg_keypoint *out;
    uint32_t *out_pos, *out_key; // the compact list instead of `out` (fast_detect_compact): pixel index row * cols + col, and the score
    uint32_t *count;
    int32_t cells_x, cells_y; // NMS: the cell grid's upper bound; no NMS: 1 x ih (a "cell" per row)
    int32_t tiles_x;          // k_fast_detect workgroups per tile row
    int32_t group, ngroups;
};
struct FastBatch {
    FastJob job[FAST_MAX_JOBS];
    uint32_t first[FAST_MAX_JOBS + 1]; // first workgroup of each job in this launch's grid
    int32_t n;
    uint32_t min_contiguous;
};

__device__ inline int job_of(const FastBatch &b, uint32_t blk) {
    int j = 0;
    while (j + 1 < b.n && blk >= b.first[j + 1]) ++j;
    return j;
}

// Circle offsets (dx, dy), clockwise from (0, -3) (Fast.zig:30-35).
__device__ constexpr int CIRCLE_DX[16] = {0, 1, 2, 3, 3, 3, 2, 1, 0, -1, -2, -3, -3, -3, -2, -1};
__device__ constexpr int CIRCLE_DY[16] = {-3, -3, -2, -1, 0, 1, 2, 3, 3, 3, 2, 1, 0, -1, -2, -3};

// isCorner's arc (:104-132) on a 16-bit mask: a full circle counts 32 (the walk goes round twice), any other mask its longest
// circular run (<= 15). "Some run of length >= mc" is a nonzero AND of mc shifted copies of the mask doubled to 32 bits.
__device__ inline bool arc_reaches(uint32_t m, uint32_t mc) {
    if (m == 0xFFFFu) return mc <= 32;
    if (mc == 0) return true;
    if (mc >= 16) return false;
    const uint32_t x = m | (m << 16);
    uint32_t y = x;
    for (uint32_t k = 1; k < mc; ++k) y &= x >> k;
    return (y & 0xFFFFu) != 0;
}

// ---- 1. detect ------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_fast_detect(FastBatch b, int nms) {
    const int j = job_of(b, blockIdx.x);
    const FastJob &J = b.job[j];
    const uint32_t blk = blockIdx.x - b.first[j];
    const int y0 = (int)(blk / (uint32_t)J.tiles_x) * DET_H, x0 = (int)(blk % (uint32_t)J.tiles_x) * DET_W;
    __shared__ uint8_t tile[DET_LH][DET_LW + 2];
    __shared__ uint32_t smin[2];
    const int tid = threadIdx.x;
    if (tid < 2) smin[tid] = 0xFFFFFFFFu;
    // candidate (y, x) is image pixel (y + 3, x + 3): the tile's first image row / col is y0 / x0
    for (int i = tid; i < DET_LH * DET_LW; i += 256) {
        const int r = i / DET_LW, c = i - r * DET_LW;
        const int gr = y0 + r, gc = x0 + c;
        tile[r][c] = (gr < J.rows && gc < J.cols) ? J.src[(size_t)gr * J.stride + gc] : (uint8_t)0;
    }
    __syncthreads();
    const int t = (int)J.threshold;
    const int lx = tid & 63;
    uint32_t my_r = 0xFFFFFFFFu, my_c = 0xFFFFFFFFu;
#pragma unroll
    for (int k = 0; k < DET_H / 4; ++k) {
        const int ly = (tid >> 6) + 4 * k;
        const int y = y0 + ly, x = x0 + lx;
        if (y >= J.ih || x >= J.iw) continue;
        const int c = tile[ly + 3][lx + 3];
        const int bright = min(c + t, 255), dark = max(c - t, 0); // saturating +| / -| on u8 (:76-79)
        // quick reject on circle pixels 0, 4, 8, 12 (:81-102): at least 3 bright or at least 3 dark. Most pixels of a photo stop
        // here, and a wave whose lanes all stop skips the rest.
        int nb = 0, nd = 0;
#pragma unroll
        for (int i = 0; i < 16; i += 4) {
            const int p = tile[ly + 3 + CIRCLE_DY[i]][lx + 3 + CIRCLE_DX[i]];
            nb += p > bright;
            nd += p < dark;
        }
        bool corner = false;
        int score = 0;
        if (nb >= 3 || nd >= 3) {
            uint32_t bm = 0, dm = 0;
#pragma unroll
            for (int i = 0; i < 16; ++i) {
                const int p = tile[ly + 3 + CIRCLE_DY[i]][lx + 3 + CIRCLE_DX[i]];
                bm |= (uint32_t)(p > bright) << i;
                dm |= (uint32_t)(p < dark) << i;
            }
            corner = arc_reaches(bm, b.min_contiguous) || arc_reaches(dm, b.min_contiguous);
            if (corner) {
#pragma unroll
                for (int i = 0; i < 16; ++i) {
                    const int d = abs((int)tile[ly + 3 + CIRCLE_DY[i]][lx + 3 + CIRCLE_DX[i]] - c);
                    score += d > t ? d : 0; // cornerScore (:135-152): every term above the threshold, whatever the arc
                }
            }
        }
        J.score[(size_t)y * J.iw + x] = corner ? (uint16_t)score : (uint16_t)0;
        if (corner) {
            my_r = min(my_r, (uint32_t)y);
            my_c = min(my_c, (uint32_t)x);
        }
    }
    if (!nms) return;
    if (my_r != 0xFFFFFFFFu) {
        atomicMin(&smin[0], my_r);
        atomicMin(&smin[1], my_c);
    }
    __syncthreads();
    if (tid < 2 && smin[tid] != 0xFFFFFFFFu) atomicMin(&J.minrc[tid], smin[tid]);
}

// ---- 2 / 4 with NMS: one workgroup per cell ---------------------------------------------------------------------------
struct CellGeom {
    int y0, x0;  // the cell's first candidate row / col
    bool empty;
};
__device__ inline CellGeom cell_geom(const FastJob &J, uint32_t blk) {
    const uint32_t mr = J.minrc[0], mc = J.minrc[1];
    CellGeom g;
    g.empty = mr == 0xFFFFFFFFu;
    g.y0 = (int)mr + (int)(blk / (uint32_t)J.cells_x) * CELL;
    g.x0 = (int)mc + (int)(blk % (uint32_t)J.cells_x) * CELL;
    if (!g.empty) g.empty = g.y0 >= J.ih || g.x0 >= J.iw;
    return g;
}
// The cell's scores into LDS; when none of them is a corner (uniform) that is all: false. Otherwise the 4-pixel ring too, and
// this thread's two pixels of the cell (p = tid, tid + 256 < 400) get their score when kept, else 0. The 68 neighbours are
// rows of a disc: |dy| <= 2 spans |dx| <= 4, |dy| = 3 spans 3, |dy| = 4 spans 2; the row maxima of widths 9, 7, 5 are formed
// once per tile row, and a pixel takes the largest of nine of them (its own score among them, which changes nothing).
struct CellLds {
    uint16_t st[CELL_L][CELL_L + 1];
    uint16_t m9[CELL_L][CELL], m7[CELL_L][CELL], m5[CELL_L][CELL];
};
__device__ inline bool cell_kept(const FastJob &J, const CellGeom &g, CellLds &L, int tid, int kept[2]) {
    int any = 0;
#pragma unroll
    for (int h = 0; h < 2; ++h) {
        const int p = tid + 256 * h;
        if (p >= CELL * CELL) continue;
        const int ly = p / CELL, lx = p - ly * CELL;
        const int y = g.y0 + ly, x = g.x0 + lx;
        const uint16_t v = (y < J.ih && x < J.iw) ? J.score[(size_t)y * J.iw + x] : (uint16_t)0;
        L.st[ly + NMS_R][lx + NMS_R] = v;
        any |= v;
    }
    kept[0] = kept[1] = 0;
    if (!__syncthreads_or(any)) return false;
    for (int i = tid; i < CELL_L * CELL_L; i += 256) {
        const int r = i / CELL_L, c = i - r * CELL_L;
        if (r >= NMS_R && r < NMS_R + CELL && c >= NMS_R && c < NMS_R + CELL) continue; // the cell itself is in already
        const int y = g.y0 - NMS_R + r, x = g.x0 - NMS_R + c;
        L.st[r][c] = (y >= 0 && y < J.ih && x >= 0 && x < J.iw) ? J.score[(size_t)y * J.iw + x] : (uint16_t)0;
    }
    __syncthreads();
    for (int i = tid; i < CELL_L * CELL; i += 256) {
        const int r = i / CELL, c = i - r * CELL; // centre column c + 4 of tile row r
        const uint16_t *row = L.st[r];
        uint16_t m = max(max(max(row[c + 2], row[c + 3]), max(row[c + 4], row[c + 5])), row[c + 6]);
        L.m5[r][c] = m;
        m = max(m, max(row[c + 1], row[c + 7]));
        L.m7[r][c] = m;
        L.m9[r][c] = max(m, max(row[c], row[c + 8]));
    }
    __syncthreads();
#pragma unroll
    for (int h = 0; h < 2; ++h) {
        const int p = tid + 256 * h;
        if (p >= CELL * CELL) continue;
        const int ly = p / CELL, lx = p - ly * CELL, r = ly + NMS_R;
        const int s = L.st[r][lx + NMS_R];
        if (s == 0) continue;
        int most = max(max(L.m5[r - 4][lx], L.m5[r + 4][lx]), max(L.m7[r - 3][lx], L.m7[r + 3][lx]));
#pragma unroll
        for (int dy = -2; dy <= 2; ++dy) most = max(most, (int)L.m9[r + dy][lx]);
        kept[h] = most <= s ? s : 0;
    }
    return true;
}

__global__ __launch_bounds__(256) void k_fast_nms_count(FastBatch b) {
    const int j = job_of(b, blockIdx.x);
    const FastJob &J = b.job[j];
    const uint32_t blk = blockIdx.x - b.first[j];
    const CellGeom g = cell_geom(J, blk);
    if (g.empty) { // uniform: every thread of the workgroup leaves here
        if (threadIdx.x == 0) J.counts[blk] = 0;
        return;
    }
    __shared__ CellLds L;
    int kept[2];
    if (!cell_kept(J, g, L, threadIdx.x, kept)) {
        if (threadIdx.x == 0) J.counts[blk] = 0;
        return;
    }
    const int n = __syncthreads_count(kept[0] != 0) + __syncthreads_count(kept[1] != 0);
    if (threadIdx.x == 0) {
        J.counts[blk] = (uint32_t)n;
        if (n) atomicAdd(&J.gtot[blk / (uint32_t)J.group], (uint32_t)n);
    }
}

// Sum of v over the workgroup (every thread calls it; acc is the caller's LDS word).
__device__ inline uint32_t block_sum(uint32_t v, uint32_t *acc) {
    if (threadIdx.x == 0) *acc = 0;
    __syncthreads();
    if (v) atomicAdd(acc, v);
    __syncthreads();
    const uint32_t r = *acc;
    __syncthreads(); // acc is reused by the next call
    return r;
}
// Workgroup 0 of a job writes the list's length; every workgroup with keypoints finds its offset in the list: the group totals
// before its group plus the counts of the cells before it in its group.
__device__ inline void write_total(const FastJob &J, uint32_t *acc) {
    uint32_t v = 0;
    for (int i = threadIdx.x; i < J.ngroups; i += 256) v += J.gtot[i];
    v = block_sum(v, acc);
    if (threadIdx.x == 0) *J.count = v;
}
__device__ inline uint32_t cell_offset(const FastJob &J, uint32_t blk, uint32_t *acc) {
    const uint32_t g = blk / (uint32_t)J.group;
    uint32_t v = 0;
    for (uint32_t i = threadIdx.x; i < g; i += 256) v += J.gtot[i];
    for (uint32_t i = g * (uint32_t)J.group + threadIdx.x; i < blk; i += 256) v += J.counts[i];
    return block_sum(v, acc);
}

__device__ inline void write_keypoint(const FastJob &J, uint32_t slot, int row, int col, int score) {
    if (slot >= J.capacity) return;
    if (J.out_pos) { // uniform over the launch
        J.out_pos[slot] = (uint32_t)row * (uint32_t)J.cols + (uint32_t)col;
        J.out_key[slot] = (uint32_t)score;
        return;
    }
    zg_keypoint kp;
    kp.x = (float)col;       // KeyPoint.zig:9-28; Fast.zig:56-62
    kp.y = (float)row;
    kp.size = 7.0f;
    kp.angle = -1.0f;
    kp.response = (float)score;
    kp.octave = 0;
    kp.class_id = -1;
    J.out[slot] = kp;
}

__global__ __launch_bounds__(256) void k_fast_nms_write(FastBatch b) {
    const int j = job_of(b, blockIdx.x);
    const FastJob &J = b.job[j];
    const uint32_t blk = blockIdx.x - b.first[j];
    __shared__ uint32_t acc;
    if (blk == 0) write_total(J, &acc); // uniform
    if (J.counts[blk] == 0) return;      // also every cell of a list without corners
    const CellGeom g = cell_geom(J, blk);
    const uint32_t base = cell_offset(J, blk, &acc);
    if (base >= J.capacity) return;
    __shared__ CellLds L;
    __shared__ uint32_t keys[CELL * CELL];
    __shared__ uint32_t nkeys;
    const int tid = threadIdx.x;
    if (tid == 0) nkeys = 0;
    int kept[2];
    cell_kept(J, g, L, tid, kept); // true here (the cell has kept corners); its barriers order nkeys = 0 before the atomics below
    uint32_t mine[2] = {0xFFFFFFFFu, 0xFFFFFFFFu};
#pragma unroll
    for (int h = 0; h < 2; ++h)
        if (kept[h]) {
            mine[h] = (uint32_t)(4095 - kept[h]) << 9 | (uint32_t)(tid + 256 * h);
            keys[atomicAdd(&nkeys, 1u)] = mine[h]; // slot order is arbitrary; the rank below is not
        }
    __syncthreads();
    const uint32_t n = nkeys;
#pragma unroll
    for (int h = 0; h < 2; ++h) {
        if (mine[h] == 0xFFFFFFFFu) continue;
        uint32_t rank = 0;
        for (uint32_t i = 0; i < n; ++i) rank += keys[i] < mine[h];
        const int p = tid + 256 * h, ly = p / CELL, lx = p - ly * CELL;
        write_keypoint(J, base + rank, g.y0 + ly + 3, g.x0 + lx + 3, kept[h]);
    }
}

// ---- 2 / 4 without NMS: one workgroup per candidate row, raster order -------------------------------------------------
__global__ __launch_bounds__(256) void k_fast_row_count(FastBatch b) {
    const int j = job_of(b, blockIdx.x);
    const FastJob &J = b.job[j];
    const uint32_t y = blockIdx.x - b.first[j];
    const uint16_t *row = J.score + (size_t)y * J.iw;
    int n = 0;
    for (int x0 = 0; x0 < J.iw; x0 += 256) {
        const int x = x0 + (int)threadIdx.x;
        n += __syncthreads_count(x < J.iw && row[x] != 0);
    }
    if (threadIdx.x == 0) {
        J.counts[y] = (uint32_t)n;
        if (n) atomicAdd(&J.gtot[y / (uint32_t)J.group], (uint32_t)n);
    }
}

__global__ __launch_bounds__(256) void k_fast_row_write(FastBatch b) {
    const int j = job_of(b, blockIdx.x);
    const FastJob &J = b.job[j];
    const uint32_t y = blockIdx.x - b.first[j];
    const uint16_t *row = J.score + (size_t)y * J.iw;
    __shared__ uint32_t acc;
    const int tid = threadIdx.x;
    if (y == 0) write_total(J, &acc); // uniform
    if (J.counts[y] == 0) return;
    uint32_t base = cell_offset(J, y, &acc);
    for (int x0 = 0; x0 < J.iw && base < J.capacity; x0 += 256) {
        const int x = x0 + tid;
        const int s = x < J.iw ? row[x] : 0;
        uint32_t total;
        const uint32_t before = block_exclusive_count(s != 0, &total);
        if (s) write_keypoint(J, base + before, (int)y + 3, x + 3, s);
        base += total;
    }
}

int check_fast_image(const zg_image *im, const char *name, bool device_pointer = true) {
    int rc;
    if ((rc = check_image(im, name, device_pointer))) return rc;
    ZG_REQUIRE(im->pixel == ZG_PIXEL_U8, ZG_ERR_UNSUPPORTED, "fast: %s is not Image(u8) (Fast.detect takes Image(u8) only)", name);
    ZG_REQUIRE(im->rows > 7 && im->cols > 7, ZG_ERR_INVALID_ARGUMENT, "fast: %s is %ux%u; Fast.detect needs rows > 7 and cols > 7 (Fast.zig:39)",
               name, im->rows, im->cols);
    return ZG_OK;
}

// n independent Fast.detect calls (validated), scratch from the caching allocator, three launches per group of FAST_MAX_JOBS.
int fast_run(const zg_image *images, uint32_t n, const uint32_t *thresholds, uint32_t min_contiguous, int nms, zg_keypoint *const *outs,
             const uint32_t *capacities, uint32_t *const *counts, hipStream_t s, uint32_t *const *pos_outs = nullptr,
             uint32_t *const *key_outs = nullptr) {
    std::vector<FastJob> jobs(n);
    // scratch: the minrc words of every job (set to 0xFF), the group totals of every job (zeroed), then per job its score map
    // and cell counts
    size_t gtot_words = 0;
    std::vector<size_t> goff(n);
    for (uint32_t i = 0; i < n; ++i) {
        const zg_image &im = images[i];
        FastJob &J = jobs[i];
        J.src = (const uint8_t *)im.data;
        J.stride = im.stride;
        J.rows = (int32_t)im.rows;
        J.cols = (int32_t)im.cols;
        J.ih = J.rows - 6;
        J.iw = J.cols - 6;
        J.threshold = thresholds[i];
        J.capacity = capacities[i];
        J.out = outs ? outs[i] : nullptr;
        J.out_pos = pos_outs ? pos_outs[i] : nullptr;
        J.out_key = key_outs ? key_outs[i] : nullptr;
        J.count = counts[i];
        J.cells_y = nms ? (int32_t)ceil_div((unsigned)J.ih, CELL) : J.ih;
        J.cells_x = nms ? (int32_t)ceil_div((unsigned)J.iw, CELL) : 1;
        J.tiles_x = (int32_t)ceil_div((unsigned)J.iw, DET_W);
        J.group = nms ? J.cells_x : 64; // NMS: a row of cells; no NMS: 64 candidate rows
        J.ngroups = (int32_t)ceil_div((unsigned)(J.cells_x * J.cells_y), (unsigned)J.group);
        goff[i] = gtot_words;
        gtot_words += (size_t)J.ngroups;
    }
    ScratchBlock sc(s);
    uint32_t *minrc, *gtot;
    sc.take(minrc, (size_t)n * 2);
    sc.take(gtot, gtot_words);
    for (FastJob &J : jobs) {
        sc.take(J.score, (size_t)J.ih * J.iw);
        sc.take(J.counts, (size_t)J.cells_x * J.cells_y);
    }
    int rc;
    if ((rc = sc.alloc())) return rc;
    for (uint32_t i = 0; i < n; ++i) {
        jobs[i].minrc = minrc + 2 * i;
        jobs[i].gtot = gtot + goff[i];
    }
    rc = fill_async(gtot, 0, gtot_words * sizeof(uint32_t), s);
    if (rc == ZG_OK && nms) rc = fill_async(minrc, 0xFF, (size_t)n * 2 * sizeof(uint32_t), s);
    for (uint32_t g = 0; g < n && rc == ZG_OK; g += FAST_MAX_JOBS) {
        FastBatch b{};
        b.n = (int32_t)std::min<uint32_t>(FAST_MAX_JOBS, n - g);
        b.min_contiguous = min_contiguous;
        for (int k = 0; k < b.n; ++k) b.job[k] = jobs[g + k];
        auto table = [&](auto blocks_of) {
            b.first[0] = 0;
            for (int k = 0; k < b.n; ++k) b.first[k + 1] = b.first[k] + blocks_of(b.job[k]);
            return b.first[b.n];
        };
        const uint32_t det = table([](const FastJob &J) { return (uint32_t)J.tiles_x * ceil_div((unsigned)J.ih, DET_H); });
        hipLaunchKernelGGL(k_fast_detect, dim3(det), dim3(256), 0, s, b, nms);
        if ((rc = launch_ok("k_fast_detect"))) break;
        const uint32_t cells = table([](const FastJob &J) { return (uint32_t)J.cells_x * (uint32_t)J.cells_y; });
        if (nms) hipLaunchKernelGGL(k_fast_nms_count, dim3(cells), dim3(256), 0, s, b);
        else hipLaunchKernelGGL(k_fast_row_count, dim3(cells), dim3(256), 0, s, b);
        if ((rc = launch_ok("k_fast_count"))) break;
        if (nms) hipLaunchKernelGGL(k_fast_nms_write, dim3(cells), dim3(256), 0, s, b);
        else hipLaunchKernelGGL(k_fast_row_write, dim3(cells), dim3(256), 0, s, b);
        rc = launch_ok("k_fast_write");
    }
    return rc;
}

int check_fast_options(uint32_t threshold, uint32_t min_contiguous) {
    ZG_REQUIRE(threshold <= 255, ZG_ERR_INVALID_ARGUMENT, "fast: threshold %u does not fit the reference's u8 (Fast.zig:17)", threshold);
    ZG_REQUIRE(min_contiguous <= 255, ZG_ERR_INVALID_ARGUMENT, "fast: min_contiguous %u does not fit the reference's u8 (Fast.zig:24)", min_contiguous);
    return ZG_OK;
}

} // namespace

// Fast.detect with NMS and min_contiguous 9 on n Image(u8) levels (validated by the caller) for ORB (orb.hip): the same launches and the
// same list order as zg_fast_detect_batch, each entry as 8 bytes (pixel index row * cols + col in pos, the integer score in key)
// instead of a 28-byte keypoint, so a list as long as the level has candidates costs 8 bytes a pixel.
int fast_detect_compact(const zg_image *images, uint32_t n, const uint32_t *thresholds, uint32_t *const *pos, uint32_t *const *key,
                        const uint32_t *capacities, uint32_t *const *counts, hipStream_t s) {
    return fast_run(images, n, thresholds, 9, 1, nullptr, capacities, counts, s, pos, key);
}
} // namespace zg

using namespace zg;

extern "C" {

int zg_fast_detect(const zg_image *src, uint32_t threshold, uint32_t min_contiguous, int nonmax_suppression, zg_keypoint *keypoints, uint32_t capacity,
                   uint32_t *count, zg_stream stream) {
    int rc;
    if ((rc = check_fast_options(threshold, min_contiguous)) || (rc = check_fast_image(src, "src"))) return rc;
    ZG_REQUIRE(count != nullptr, ZG_ERR_INVALID_ARGUMENT, "fast: null count");
    ZG_REQUIRE(keypoints != nullptr || capacity == 0, ZG_ERR_INVALID_ARGUMENT, "fast: null keypoints with capacity %u", capacity);
    return fast_run(src, 1, &threshold, min_contiguous, nonmax_suppression != 0, &keypoints, &capacity, &count, as_stream(stream));
}

int zg_fast_detect_host(const zg_image *src, uint32_t threshold, uint32_t min_contiguous, int nonmax_suppression, zg_keypoint *keypoints, uint32_t capacity,
                        uint32_t *count) {
    int rc;
    if ((rc = check_fast_options(threshold, min_contiguous)) || (rc = check_fast_image(src, "src", false))) return rc;
    ZG_REQUIRE(count != nullptr, ZG_ERR_INVALID_ARGUMENT, "fast: null count");
    ZG_REQUIRE(keypoints != nullptr || capacity == 0, ZG_ERR_INVALID_ARGUMENT, "fast: null keypoints with capacity %u", capacity);
    HostStage a;
    if ((rc = a.upload(src, true, false))) return rc;
    // scratch: [keypoints][count]
    ScratchBlock sc;
    zg_keypoint *dkp;
    uint32_t *dcount;
    sc.take(dkp, capacity);
    sc.take(dcount, 1);
    if ((rc = sc.alloc())) return rc;
    if (!capacity) dkp = nullptr;
    if ((rc = fast_run(&a.dev, 1, &threshold, min_contiguous, nonmax_suppression != 0, &dkp, &capacity, &dcount, nullptr))) return rc;
    return download_counted(count, dcount, 1, keypoints, dkp, capacity);
}

int zg_fast_detect_batch(const zg_image *images, uint32_t n, const uint32_t *thresholds, uint32_t min_contiguous, int nonmax_suppression,
                         zg_keypoint *keypoints, const uint32_t *capacities, const uint64_t *offsets, uint32_t *counts, zg_stream stream) {
    if (n == 0) return ZG_OK;
    ZG_REQUIRE(images && thresholds && capacities && offsets && counts, ZG_ERR_INVALID_ARGUMENT, "fast batch: null argument");
    int rc;
    std::vector<zg_keypoint *> outs(n);
    std::vector<uint32_t *> cnts(n);
    for (uint32_t i = 0; i < n; ++i) {
        if ((rc = check_fast_options(thresholds[i], min_contiguous)) || (rc = check_fast_image(&images[i], "image"))) return rc;
        ZG_REQUIRE(keypoints != nullptr || capacities[i] == 0, ZG_ERR_INVALID_ARGUMENT, "fast batch: null keypoints with capacity %u", capacities[i]);
        outs[i] = keypoints ? keypoints + offsets[i] : nullptr;
        cnts[i] = counts + i;
    }
    return fast_run(images, n, thresholds, min_contiguous, nonmax_suppression != 0, outs.data(), capacities, cnts.data(), as_stream(stream));
}

} // extern "C"
