// qr.hip — the QR detector (reference src/qrcode/detector.zig:57-641) on the device: a frame to the sampled module grids and their
// corners, every trial of the reference's loops in the reference's order, with the same f32 and f64 bits, asynchronous, with no host
// synchronisation, recordable into a graph. The arithmetic that has to match is zg_qr_geom.h (also compiled by plain g++ for the tests).
//
// The reference is sequential in three places only: addCandidate's running average (order dependent), insertNearest, and the list of
// version candidates that grows while it is walked. Everything else is independent per pixel, per triple, per probe or per module.
//   [zg_convert]        a source that is not Image(u8) to u8 (:50-55)
//   [zg_threshold_*]    the binary map (:73-79), unless the caller's frame is one
//   k_qr_hits<false>    a lane per pixel, workgroups never straddle a row. The lane at the last pixel of a dark run walks left over five
//                       runs (giving up only where checkRatio's rejection is certain: the last run d passes only if total <= 14 d up to
//                       rounding, so beyond 15 d), runs the reference's checkRatio, and confirms (:286-307). Rows come in the order the
//                       reference consumes them: residue 0 mod 3 first when rows > 300, then 1, then 2. A count per workgroup.
//   k_qr_scan           exclusive sums of the counts, one workgroup.
//   k_qr_hits<true>     the same lanes again; the confirmed patterns land in (residue pass, row, column) order. Count first, then
//                       write: there is no capacity to overflow.
//   k_qr_tail           one workgroup: lane 0 folds the hits into the 64-entry buffer (:309-326) and filters (:102-109); all lanes
//                       score the triples (argmin under strict <, ties to the lowest (i, j, k)); lane 0 makes the probe positions by
//                       the f32 recurrences, all lanes probe, lane 0 folds insertNearest in probe order; then the trials in order,
//                       a lane per module inside one.
#include "zg_common.h"
#include "zg_internal.h"
#include "zg_qr_geom.h"
#include "zg_scan.h"

#include <cstring>

#pragma clang fp contract(off)

namespace zg {
namespace {

using qr::Finder;

struct Bin { // the binary map: a pixel is dark iff its byte is 0
    const uint8_t *p;
    size_t stride;
    int rows, cols;
    __device__ bool dark(int r, int c) const { return p[(size_t)r * stride + (size_t)c] == 0; }
    __device__ bool inside(int r, int c) const { return r >= 0 && r < rows && c >= 0 && c < cols; }
};

struct Hit { float x, y, ms; };

// traceRuns (:231-257)
__device__ bool trace_runs(const Bin &b, int r, int c, int dr, int dc, bool limited, uint32_t max_run, uint32_t runs[3]) {
    uint32_t r0 = 0, r1 = 0, r2 = 0; // three words, not an array indexed by the state: that would live in scratch memory
    int state = 0;
    bool early = false;
    while (b.inside(r, c)) {
        const bool dark = b.dark(r, c);
        if (dark != (state != 1)) {
            if (state == 2) break;
            ++state; // this pixel again, as part of the next run
            continue;
        }
        const uint32_t now = state == 0 ? ++r0 : (state == 1 ? ++r1 : ++r2);
        if (limited) {
            if (state == 2) {
                early = true;
                break;
            }
            if (now > max_run) return false;
        }
        r += dr;
        c += dc;
    }
    runs[0] = r0; runs[1] = r1; runs[2] = r2;
    return early || (r1 != 0 && r2 != 0);
}

// crossCheck (:274-282)
__device__ bool cross_check(const Bin &b, int row, int col, int dr, int dc, float tolerance, uint32_t *total, uint32_t *forward) {
    uint32_t back[3], fwd[3];
    if (!trace_runs(b, row, col, -dr, -dc, false, 0, back)) return false;
    if (!trace_runs(b, row + dr, col + dc, dr, dc, false, 0, fwd)) return false;
    const uint32_t runs[5] = {back[2], back[1], back[0] + fwd[0], fwd[1], fwd[2]};
    if (!qr::check_ratio(runs, tolerance)) return false;
    *total = runs[0] + runs[1] + runs[2] + runs[3] + runs[4];
    *forward = fwd[0] + fwd[1] + fwd[2];
    return true;
}

// confirmCandidate (:286-307). The two centres lie inside their patterns' extents, which lie inside the frame: the range tests on crow
// and ccol never fail, they only keep a read inside the view whatever happens.
__device__ bool confirm(const Bin &b, int row, int col, Hit *out) {
    if (col >= b.cols || !b.dark(row, col)) return false;
    uint32_t vt, vf, ht, hf, dt, df;
    if (!cross_check(b, row, col, 1, 0, qr::CROSS_TOL, &vt, &vf)) return false;
    const float center_row = qr::cross_center((uint32_t)row, vf, vt);
    const int crow = (int)center_row;
    if (!b.inside(crow, col) || !b.dark(crow, col)) return false;
    if (!cross_check(b, crow, col, 0, 1, qr::CROSS_TOL, &ht, &hf)) return false;
    const float center_col = qr::cross_center((uint32_t)col, hf, ht);
    const int ccol = (int)center_col;
    if (!b.inside(crow, ccol) || !b.dark(crow, ccol)) return false;
    if (!cross_check(b, crow, ccol, 1, 1, qr::DIAG_TOL, &dt, &df)) return false;
    out->x = center_col;
    out->y = center_row;
    out->ms = (float)(vt + ht) / 14.0f;
    return true;
}

// The window the reference tests when the dark run that ends with pixel (row, c) ends (:187-205), and its confirmation.
__device__ bool scan_hit(const Bin &b, int row, int c, Hit *out) {
    if (!b.dark(row, c) || (c + 1 < b.cols && b.dark(row, c + 1))) return false;
    uint32_t runs[5];
    uint64_t total = 0, give_up = 0;
    int x = c;
#pragma unroll
    for (int k = 4; k >= 0; --k) {
        const bool want = (k & 1) == 0;
        uint32_t len = 0;
        while (x >= 0 && b.dark(row, x) == want) {
            ++len;
            --x;
            if (k < 4 && total + len > give_up) return false;
        }
        if (len == 0) return false; // the row began before five runs had ended: a zero in the window
        runs[k] = len;
        total += len;
        if (k == 4) give_up = 15ull * len;
    }
    if (!qr::check_ratio(runs, qr::SCAN_TOL)) return false;
    const int mid_start = c + 1 - (int)runs[4] - (int)runs[3] - (int)runs[2];
    return confirm(b, row, mid_start + (int)(runs[2] / 2), out);
}

// the row a workgroup row stands for: every row in order, or residue 0 mod 3 first, then 1, then 2 (:89-96)
__device__ int rank_row(int rank, int rows) {
    if (rows <= 300) return rank;
    const int n0 = (rows + 2) / 3, n1 = (rows + 1) / 3;
    if (rank < n0) return 3 * rank;
    if (rank < n0 + n1) return 3 * (rank - n0) + 1;
    return 3 * (rank - n0 - n1) + 2;
}

template <bool WRITE> __global__ __launch_bounds__(256) void k_qr_hits(Bin b, uint32_t chunks, uint32_t *cnt, Hit *rec) {
    const int rank = grid_row();
    if (rank >= b.rows) return;
    const int row = rank_row(rank, b.rows), c = (int)(blockIdx.x * 256u + threadIdx.x);
    Hit h;
    const bool hit = c < b.cols && scan_hit(b, row, c, &h);
    uint32_t total;
    const uint32_t before = block_exclusive_count(hit, &total);
    const size_t wg = (size_t)rank * chunks + blockIdx.x;
    if (WRITE) {
        if (hit) rec[cnt[wg] + before] = h;
    } else if (threadIdx.x == 0) {
        cnt[wg] = total;
    }
}

// cnt[0 .. n) to its exclusive sums, cnt[n] the sum of all
__global__ __launch_bounds__(256) void k_qr_scan(uint32_t *cnt, uint32_t n) {
    uint32_t base = 0;
    for (uint32_t i0 = 0; i0 < n; i0 += 256u) {
        const uint32_t i = i0 + threadIdx.x;
        const uint32_t v = i < n ? cnt[i] : 0u;
        uint32_t total;
        const uint32_t ex = block_exclusive_sum(v, &total);
        if (i < n) cnt[i] = base + ex;
        base += total;
    }
    if (threadIdx.x == 0) cnt[n] = base;
}

// addCandidate (:309-326)
__device__ void add_candidate(zg_qr_finder *buf, uint32_t *count, const Hit &p) {
    for (uint32_t i = 0; i < *count; ++i) {
        zg_qr_finder &e = buf[i];
        const float near = 2.0f * e.module_size;
        if (fabsf(e.x - p.x) < near && fabsf(e.y - p.y) < near) {
            const float w = e.hits, s = 1.0f / (w + 1.0f);
            e.x = (e.x * w + p.x) * s;
            e.y = (e.y * w + p.y) * s;
            e.module_size = (e.module_size * w + p.ms) / (w + 1.0f);
            e.hits = e.hits + 1.0f;
            return;
        }
    }
    if (*count < ZG_QR_MAX_FINDERS) {
        buf[*count] = zg_qr_finder{p.x, p.y, p.ms, 1.0f};
        ++*count;
    }
}

__device__ Finder as_finder(const zg_qr_finder &f) { return Finder{f.x, f.y, f.module_size, f.hits}; }

// alignmentAxis (:523-532)
__device__ bool alignment_axis(const Bin &b, int row, int col, int dr, int dc, float ms, uint32_t limit, float *center, uint32_t *extent) {
    uint32_t back[3], fwd[3];
    if (!trace_runs(b, row, col, -dr, -dc, true, limit, back)) return false;
    if (!qr::near_module(back[1], ms)) return false;
    if (!trace_runs(b, row + dr, col + dc, dr, dc, true, limit, fwd)) return false;
    if (!qr::near_module(back[0] + fwd[0], ms) || !qr::near_module(fwd[1], ms)) return false;
    const float base = (float)(dc != 0 ? col : row);
    *center = base + ((float)fwd[0] - (float)back[0]) / 2.0f + 1.0f;
    *extent = back[0] + fwd[0];
    return true;
}

// checkAlignment (:536-562). An axis centre is above 0 (the dark run holds the base pixel), so its cast is defined.
__device__ bool check_alignment(const Bin &b, int row, int col, float ms, float *cx, float *cy) {
    const uint32_t limit = (uint32_t)(ms * 1.6f + 1.0f);
    float hc, vc;
    uint32_t he, ve;
    if (!alignment_axis(b, row, col, 0, 1, ms, limit, &hc, &he)) return false;
    if (!(hc < 2147483648.0f)) return false;
    const int ccol = (int)hc;
    if (ccol >= b.cols || !b.dark(row, ccol)) return false;
    if (!alignment_axis(b, row, ccol, 1, 0, ms, limit, &vc, &ve)) return false;
    const float local_ms = (float)(he + ve) / 2.0f;
    const float right = (float)b.cols, bottom = (float)b.rows;
    for (int d = 0; d < 4; ++d) {
        const float d0 = d < 2 ? 1.0f : -1.0f, d1 = (d & 1) ? -1.0f : 1.0f;
        for (int k = 1; k <= 2; ++k) {
            const float pr = vc + d0 * (float)k * local_ms, pc = hc + d1 * (float)k * local_ms;
            if (!(pc >= 0.0f && pc < right && pr >= 0.0f && pr < bottom)) return false; // Rectangle.contains: half-open, NaN outside
            if (b.dark((int)pr, (int)pc) != (k == 2)) return false;
        }
    }
    *cx = hc;
    *cy = vc;
    return true;
}

// sampleModule (:567-584) without its early exits, which do not change the result: 0 or 1, or 2 where the centre leaves the frame.
__device__ uint32_t sample_module(const Bin &b, const double *m, uint32_t row, uint32_t col) {
    const double off[5][2] = {{0, 0}, {0.25, 0}, {-0.25, 0}, {0, 0.25}, {0, -0.25}};
    const double right = (double)b.cols, bottom = (double)b.rows;
    uint32_t votes = 0;
#pragma unroll
    for (int k = 0; k < 5; ++k) {
        double px, py;
        qr::project(m, (double)col + 0.5 + off[k][0], (double)row + 0.5 + off[k][1], &px, &py);
        if (!(px >= 0.0 && px < right && py >= 0.0 && py < bottom)) {
            if (k == 0) return 2u;
            continue;
        }
        if (b.dark((int)py, (int)px)) ++votes;
    }
    return votes >= 3u ? 1u : 0u;
}

struct Scored { float x, y, d2; };

// insertNearest (:492-507)
__device__ void insert_nearest(Scored found[4], uint32_t *count, const Scored &c, float ms) {
    for (uint32_t i = 0; i < *count; ++i) {
        if (fabsf(found[i].x - c.x) < ms && fabsf(found[i].y - c.y) < ms) {
            if (c.d2 < found[i].d2) found[i] = c;
            return;
        }
    }
    uint32_t at = *count;
    while (at > 0 && c.d2 < found[at - 1].d2) --at;
    if (at >= 4) return;
    uint32_t back = *count < 3u ? *count : 3u;
    for (; back > at; --back) found[back] = found[back - 1];
    found[at] = c;
    if (*count < 4) ++*count;
}

__device__ void append_version(zg_qr_detection &d, uint32_t v) {
    for (uint32_t i = 0; i < d.version_count; ++i)
        if (d.versions[i] == v) return;
    if (d.version_count < ZG_QR_MAX_VERSIONS) d.versions[d.version_count++] = (uint8_t)v;
}

constexpr uint32_t MAX_POS = 1024;   // probe positions an axis: at most 2 radius / step + 1 < 270 (radius <= 33.4 ms, step >= max(1, ms / 4))
constexpr uint32_t MAX_STEPS = 4096; // of a recurrence, the skipped negative positions included

// y = start; while (y <= end) : (y += step) { if (y < 0) continue; p = int(y); if (p >= size) break; ... } (:460-469): the positions the
// body is reached with
__device__ uint32_t probe_positions(float start, float end, float step, int size, int *pos) {
    uint32_t n = 0, it = 0;
    for (float y = start; y <= end && it < MAX_STEPS; y += step, ++it) {
        if (y < 0.0f) continue;
        if (!(y < 2147483648.0f)) break; // past every frame, and the cast stays defined
        const int p = (int)y;
        if (p >= size || n >= MAX_POS) break;
        pos[n++] = p;
    }
    return n;
}

__global__ __launch_bounds__(256) void k_qr_tail(Bin b, const uint32_t *cnt, const Hit *rec, uint32_t chunks, zg_qr_detection *det_out, zg_qr_grid *grids,
                                                 uint32_t grid_capacity, uint8_t *modules, uint32_t module_capacity) {
    __shared__ zg_qr_detection det;
    __shared__ __attribute__((aligned(16))) uint8_t grid[(ZG_QR_MAX_MODULES + 15) / 16 * 16];
    __shared__ double M[9], A[8][9], PTS[2][4][2];
    __shared__ Scored found[4];
    __shared__ int ys[MAX_POS], xs[MAX_POS];
    __shared__ float red_score[256], res_x[256], res_y[256];
    __shared__ uint32_t red_idx[256];
    __shared__ unsigned long long masks[4];
    __shared__ uint32_t ny, nx, flag, go, stopped;
    __shared__ float s_ms, s_px, s_py;
    const uint32_t tid = threadIdx.x;
    for (uint32_t i = tid; i < sizeof(det) / 4; i += 256u) ((uint32_t *)&det)[i] = 0u;
    if (tid == 0) stopped = 0;
    __syncthreads();

    // ---- merge (:87-109)
    if (tid == 0) {
        const bool coarse = b.rows > 300;
        const uint32_t n0 = cnt[(size_t)(coarse ? (b.rows + 2) / 3 : b.rows) * chunks], total = cnt[(size_t)b.rows * chunks];
        uint32_t count = 0;
        for (uint32_t h = 0; h < n0; ++h) add_candidate(det.finders, &count, rec[h]);
        if (count < 3 && coarse)
            for (uint32_t h = n0; h < total; ++h) add_candidate(det.finders, &count, rec[h]);
        det.merged_count = det.finder_count = count;
        if (count >= 3) {
            uint32_t confirmed = 0;
            for (uint32_t i = 0; i < count; ++i)
                if (det.finders[i].hits >= 2.0f) det.finders[confirmed++] = det.finders[i];
            if (confirmed >= 3) det.finder_count = confirmed;
        }
    }
    __syncthreads();
    const uint32_t nf = det.finder_count;

    // ---- triple (:342-398): a lane per (i, j), k inside; ties to the lowest (i, j, k)
    if (det.merged_count >= 3) {
        float best = 3.4028234663852886e38f;
        uint32_t best_idx = 0xffffffffu;
        for (uint32_t ij = tid; ij < nf * nf; ij += 256u) {
            const uint32_t i = ij / nf, j = ij - i * nf;
            if (i >= j) continue;
            const Finder fa = as_finder(det.finders[i]), fb = as_finder(det.finders[j]);
            for (uint32_t k = j + 1; k < nf; ++k) {
                float score;
                int order[3];
                if (!qr::triple_score(fa, fb, as_finder(det.finders[k]), &score, order)) continue;
                const uint32_t idx = i << 12 | j << 6 | k;
                if (score < best || (score == best && idx < best_idx && best_idx != 0xffffffffu)) {
                    best = score;
                    best_idx = idx;
                }
            }
        }
        red_score[tid] = best;
        red_idx[tid] = best_idx;
        __syncthreads();
        for (uint32_t s = 128; s > 0; s >>= 1) {
            if (tid < s) {
                const float os = red_score[tid + s];
                const uint32_t oi = red_idx[tid + s];
                if (oi != 0xffffffffu && (red_idx[tid] == 0xffffffffu || os < red_score[tid] || (os == red_score[tid] && oi < red_idx[tid]))) {
                    red_score[tid] = os;
                    red_idx[tid] = oi;
                }
            }
            __syncthreads();
        }
        if (tid == 0 && red_idx[0] != 0xffffffffu) {
            const uint32_t t0 = red_idx[0] >> 12, t1 = (red_idx[0] >> 6) & 63u, t2 = red_idx[0] & 63u;
            float score;
            int order[3];
            qr::triple_score(as_finder(det.finders[t0]), as_finder(det.finders[t1]), as_finder(det.finders[t2]), &score, order);
            det.triple_found = 1;
#pragma unroll
            for (int q = 0; q < 3; ++q) det.triple[q] = det.finders[order[q] == 0 ? t0 : (order[q] == 1 ? t1 : t2)];
        }
    }
    __syncthreads();

    if (det.triple_found) { // uniform: every lane reads the same word
        const Finder tl = as_finder(det.triple[0]), tr = as_finder(det.triple[1]), bl = as_finder(det.triple[2]);
        // ---- version candidates (:112-117) and the probe positions (:442-460)
        if (tid == 0) {
            const uint32_t estimate = qr::estimate_version(tl, tr, bl);
            det.version_estimate = estimate;
            append_version(det, estimate);
            if (estimate > 1) append_version(det, estimate - 1);
            if (estimate < 40) append_version(det, estimate + 1);
            const uint32_t scan_version = estimate + 1 < 40 ? estimate + 1 : 40, dim = 17 + 4 * scan_version;
            ny = nx = 0;
            if (dim >= 25) {
                const float span = (float)(dim - 7), steps = (float)(dim - 10), inv = 1.0f / span;
                const float pmx = ((tr.x - tl.x) + (bl.x - tl.x)) * inv, pmy = ((tr.y - tl.y) + (bl.y - tl.y)) * inv;
                const float px = tl.x + pmx * steps, py = tl.y + pmy * steps;
                const float ms = qr::triple_module_size(tl, tr, bl);
                const float radius = ms * fmaxf(5.0f, 0.2f * steps);
                const float step = truncf(fmaxf(1.0f, ms / 2.0f));
                ny = probe_positions(py - radius, py + radius, step, b.rows, ys);
                nx = probe_positions(px - radius, px + radius, step, b.cols, xs);
                s_ms = ms;
                s_px = px;
                s_py = py;
            }
        }
        __syncthreads();
        // ---- fourth (:461-484): a lane per probe, 256 at a time in probe order (y outer, x inner); lane 0 folds each batch in order
        uint32_t found_count = 0; // lane 0's
        const uint32_t probes = ny * nx;
        for (uint32_t base = 0; base < probes; base += 256u) {
            const uint32_t p = base + tid;
            bool ok = false;
            if (p < probes) {
                const int py = ys[p / nx], px = xs[p % nx];
                float cx, cy;
                if (b.dark(py, px) && check_alignment(b, py, px, s_ms, &cx, &cy)) {
                    ok = true;
                    res_x[tid] = cx;
                    res_y[tid] = cy;
                }
            }
            const unsigned long long m = __ballot(ok);
            if ((tid & 63u) == 0) masks[tid >> 6] = m;
            __syncthreads();
            if (tid == 0) {
                for (uint32_t w = 0; w < 4; ++w) {
                    unsigned long long mm = masks[w];
                    while (mm) {
                        const uint32_t l = w * 64u + (uint32_t)(__ffsll((long long)mm) - 1);
                        mm &= mm - 1;
                        const float dx = res_x[l] - s_px, dy = res_y[l] - s_py;
                        insert_nearest(found, &found_count, Scored{res_x[l], res_y[l], dx * dx + dy * dy}, s_ms);
                    }
                }
            }
            __syncthreads();
        }
        if (tid == 0) {
            for (uint32_t i = 0; i < found_count; ++i) det.fourths[i] = zg_qr_fourth{found[i].x, found[i].y, 1u};
            det.fourths[found_count] = zg_qr_fourth{(tr.x + bl.x) - tl.x, (tr.y + bl.y) - tl.y, 0u};
            det.fourth_count = found_count + 1;
        }
        __syncthreads();

        // ---- trials (:126-153), in order: the candidate list grows while it is walked
        for (uint32_t vi = 0; vi < det.version_count; ++vi) {
            const uint32_t version = det.versions[vi], dim = 17 + 4 * version, nm = dim * dim;
            for (uint32_t fi = 0; fi < det.fourth_count; ++fi) {
                const zg_qr_fourth fourth = det.fourths[fi];
                if (fourth.is_alignment && version < 2) continue;
                __syncthreads(); // the previous trial's reads of go, flag and M are done
                if (tid == 0) {
                    go = qr::build_transform(tl, tr, bl, fourth.x, fourth.y, fourth.is_alignment != 0, dim, PTS, A, M) ? 1u : 0u;
                    flag = 0;
                }
                __syncthreads();
                if (!go) continue;
                double m[9];
#pragma unroll
                for (int q = 0; q < 9; ++q) m[q] = M[q];
                // sampleTimingLines (:598-607)
                const uint32_t n = dim - 16;
                for (uint32_t t = tid; t < 4 * n; t += 256u) {
                    const uint32_t line = t / (2 * n) ? dim - 7 : 6, rem = t % (2 * n), i = 8 + rem / 2;
                    const uint32_t row = (rem & 1u) ? i : line, col = (rem & 1u) ? line : i;
                    const uint32_t v = sample_module(b, m, row, col);
                    if (v == 2u) flag = 1; // every writer writes the same value
                    grid[row * dim + col] = (uint8_t)v;
                }
                __syncthreads();
                if (tid == 0) go = !flag && qr::timing_ok(grid, dim) ? 1u : 0u;
                __syncthreads();
                if (!go) continue;
                // sampleGrid (:587-595)
                for (uint32_t t = tid; t < nm; t += 256u) {
                    const uint32_t v = sample_module(b, m, t / dim, t % dim);
                    if (v == 2u) flag = 1;
                    grid[t] = (uint8_t)v;
                }
                __syncthreads();
                if (flag) continue;
                if (tid == 0) {
                    int hint = -1;
                    if (version >= 7) {
                        hint = qr::read_version(grid, dim);
                        if (hint >= 0) append_version(det, (uint32_t)hint);
                    }
                    ++det.grids_total;
                    const bool fits = !stopped && det.grids_written < grid_capacity && nm <= module_capacity - det.modules_written;
                    go = fits ? 1u : 0u;
                    if (fits) {
                        zg_qr_grid &g = grids[det.grids_written];
                        g.version = version;
                        g.dim = dim;
                        g.fourth_index = fi;
                        g.modules_offset = det.modules_written;
                        g.version_hint = hint;
                        g.reserved = 0;
                        const double d = (double)dim;
#pragma unroll
                        for (int q = 0; q < 4; ++q) { // symbolCorners (:611-619)
                            double x, y;
                            qr::project(m, (q & 1) ? d : 0.0, (q & 2) ? d : 0.0, &x, &y);
                            g.corners[2 * q] = (float)x;
                            g.corners[2 * q + 1] = (float)y;
                        }
#pragma unroll
                        for (int q = 0; q < 9; ++q) g.transform[q] = m[q];
                    } else {
                        stopped = 1;
                    }
                }
                __syncthreads();
                if (go) {
                    uint8_t *dst = modules + det.modules_written;
                    for (uint32_t t = tid; t < nm; t += 256u) dst[t] = grid[t];
                    __syncthreads(); // every lane has read modules_written
                    if (tid == 0) {
                        ++det.grids_written;
                        det.modules_written += nm;
                    }
                }
            }
        }
    }
    __syncthreads();
    for (uint32_t i = tid; i < sizeof(det) / 4; i += 256u) ((uint32_t *)det_out)[i] = ((const uint32_t *)&det)[i];
}

__global__ __launch_bounds__(256) void k_qr_empty(zg_qr_detection *det) {
    for (uint32_t i = threadIdx.x; i < sizeof(zg_qr_detection) / 4; i += 256u) ((uint32_t *)det)[i] = 0u;
}

// A lane per edge of a written grid: corners TL -> TR -> BR -> BL -> TL.
__global__ __launch_bounds__(256) void k_qr_build(const zg_qr_grid *grids, const zg_qr_detection *det, uint32_t capacity, uint32_t color, uint32_t width, int mode,
                                                  zg_draw_cmd *out, uint32_t *count_out) {
    const uint32_t edges = 4u * det->grids_written, n = edges < capacity ? edges : capacity;
    if (blockIdx.x == 0 && threadIdx.x == 0) *count_out = n;
    for (uint32_t e = blockIdx.x * 256u + threadIdx.x; e < n; e += gridDim.x * 256u) {
        const float *c = grids[e / 4].corners;
        const uint32_t q = e % 4u, q1 = (q + 1u) % 4u, a = q ^ (q >> 1), z = q1 ^ (q1 >> 1); // the ring 0, 1, 3, 2 over TL, TR, BL, BR
        zg_draw_cmd cmd;
        cmd.kind = ZG_DRAW_LINE;
        cmd.mode = mode;
        cmd.width = width;
        cmd.color[0] = (uint8_t)color; cmd.color[1] = (uint8_t)(color >> 8); cmd.color[2] = (uint8_t)(color >> 16); cmd.color[3] = (uint8_t)(color >> 24);
        cmd.p[0] = c[2 * a]; cmd.p[1] = c[2 * a + 1]; cmd.p[2] = c[2 * z]; cmd.p[3] = c[2 * z + 1];
        cmd.first_vertex = 0;
        cmd.n_vertices = 0;
        out[e] = cmd;
    }
}

// ---- host ----------------------------------------------------------------------------------------------------------------------

bool have_device() { // asked once per process
    static const bool ok = [] {
        int n = 0;
        const bool r = hipGetDeviceCount(&n) == hipSuccess && n > 0;
        if (!r) (void)hipGetLastError();
        return r;
    }();
    return ok;
}

int source_space(int pixel) {
    switch (pixel) {
    case ZG_PIXEL_RGB_U8: case ZG_PIXEL_RGB_F32: return ZG_CS_RGB;
    case ZG_PIXEL_RGBA_U8: case ZG_PIXEL_RGBA_F32: return ZG_CS_RGBA;
    default: return ZG_CS_GRAY;
    }
}

bool empty_frame(const zg_image *src) { return src->rows < 21 || src->cols < 21; } // :58

uint32_t hit_capacity(size_t rows, size_t cols) { return (uint32_t)(rows * ((cols + 1) / 2) + 1); } // a hit per dark run, a light pixel between two

int check(const zg_image *src, int binarize, const zg_qr_detection *detection, const zg_qr_grid *grids, uint32_t grid_capacity, const uint8_t *modules,
          uint32_t module_capacity, bool device) {
    int rc;
    if ((rc = check_image(src, "qr_detect", device))) return rc;
    ZG_REQUIRE(binarize >= ZG_QR_ADAPTIVE && binarize <= ZG_QR_BINARY, ZG_ERR_INVALID_ARGUMENT, "qr_detect: binarize %d", binarize);
    ZG_REQUIRE(binarize != ZG_QR_BINARY || src->pixel == ZG_PIXEL_U8, ZG_ERR_UNSUPPORTED, "qr_detect: pixel type %d as a binary map (Image(u8) only)", src->pixel);
    ZG_REQUIRE((uint64_t)src->rows * src->cols < (1ull << 31), ZG_ERR_UNSUPPORTED, "qr_detect: %u x %u pixels, 2^31 or more", src->rows, src->cols);
    ZG_REQUIRE(detection != nullptr, ZG_ERR_INVALID_ARGUMENT, "qr_detect: null detection");
    ZG_REQUIRE(grids != nullptr || grid_capacity == 0, ZG_ERR_INVALID_ARGUMENT, "qr_detect: null grids");
    ZG_REQUIRE(modules != nullptr || module_capacity == 0, ZG_ERR_INVALID_ARGUMENT, "qr_detect: null modules");
    ZG_REQUIRE(have_device(), ZG_ERR_HIP, "qr_detect: no device");
    return ZG_OK;
}

int detect(const zg_image *src, int binarize, zg_qr_detection *detection, zg_qr_grid *grids, uint32_t grid_capacity, uint8_t *modules, uint32_t module_capacity,
           zg_stream stream) {
    hipStream_t s = as_stream(stream);
    if (empty_frame(src)) {
        k_qr_empty<<<1, 256, 0, s>>>(detection);
        return launch_ok("k_qr_empty");
    }
    const size_t n = (size_t)src->rows * src->cols;
    const uint32_t chunks = ceil_div(src->cols, 256);
    const size_t groups = (size_t)src->rows * chunks;
    ScratchBlock sc(s);
    uint8_t *gray = nullptr, *binary = nullptr;
    uint32_t *cnt;
    Hit *rec;
    if (src->pixel != ZG_PIXEL_U8) sc.take(gray, n);
    if (binarize != ZG_QR_BINARY) sc.take(binary, n);
    sc.take(cnt, groups + 1);
    sc.take(rec, hit_capacity(src->rows, src->cols));
    int rc;
    if ((rc = sc.alloc())) return rc;
    zg_image g = *src;
    if (gray) {
        g = zg_image{gray, src->cols, src->rows, src->cols, ZG_PIXEL_U8};
        if ((rc = zg_convert(src, source_space(src->pixel), &g, ZG_CS_GRAY, nullptr, stream))) return rc;
    }
    zg_image bin = g;
    if (binary) {
        bin = zg_image{binary, src->cols, src->rows, src->cols, ZG_PIXEL_U8};
        if (binarize == ZG_QR_ADAPTIVE) {
            const uint32_t side = src->rows < src->cols ? src->rows : src->cols, radius = side / 16 > 8 ? side / 16 : 8; // :73
            rc = zg_threshold_adaptive_mean(&g, &bin, radius, 4.0f, stream);
        } else {
            rc = zg_threshold_otsu(&g, &bin, nullptr, stream);
        }
        if (rc) return rc;
    }
    const Bin b{(const uint8_t *)bin.data, bin.stride, (int)bin.rows, (int)bin.cols};
    const dim3 hits_grid = row_grid(chunks, src->rows);
    k_qr_hits<false><<<hits_grid, 256, 0, s>>>(b, chunks, cnt, rec);
    if ((rc = launch_ok("k_qr_hits (count)"))) return rc;
    k_qr_scan<<<1, 256, 0, s>>>(cnt, (uint32_t)groups);
    if ((rc = launch_ok("k_qr_scan"))) return rc;
    k_qr_hits<true><<<hits_grid, 256, 0, s>>>(b, chunks, cnt, rec);
    if ((rc = launch_ok("k_qr_hits (write)"))) return rc;
    k_qr_tail<<<1, 256, 0, s>>>(b, cnt, rec, chunks, detection, grids, grid_capacity, modules, module_capacity);
    return launch_ok("k_qr_tail");
}

} // namespace
} // namespace zg

using namespace zg;

extern "C" {

size_t zg_qr_sizeof_detection(void) { return sizeof(zg_qr_detection); }
size_t zg_qr_sizeof_grid(void) { return sizeof(zg_qr_grid); }

size_t zg_qr_scratch_bytes(uint32_t rows, uint32_t cols) {
    const size_t n = (size_t)rows * cols;
    if (rows < 21 || cols < 21 || n >= ((size_t)1 << 31)) return 0;
    // the sum of detect()'s parts at their largest (a source that is converted and thresholded), each rounded up to 256 bytes
    return align256(n) + align256(n) + align256(((size_t)rows * ceil_div(cols, 256) + 1) * 4) + align256((size_t)hit_capacity(rows, cols) * sizeof(Hit));
}

int zg_qr_detect(const zg_image *src, int binarize, zg_qr_detection *detection, zg_qr_grid *grids, uint32_t grid_capacity, uint8_t *modules,
                 uint32_t module_capacity, zg_stream stream) {
    if (const int rc = check(src, binarize, detection, grids, grid_capacity, modules, module_capacity, true)) return rc;
    return detect(src, binarize, detection, grids, grid_capacity, modules, module_capacity, stream);
}

int zg_qr_detect_host(const zg_image *src, int binarize, zg_qr_detection *detection, zg_qr_grid *grids, uint32_t grid_capacity, uint8_t *modules,
                      uint32_t module_capacity) {
    int rc;
    if ((rc = check(src, binarize, detection, grids, grid_capacity, modules, module_capacity, false))) return rc;
    HostStage st;
    if ((rc = st.upload(src, true, false))) return rc;
    ScratchBlock sc;
    zg_qr_detection *d_det;
    zg_qr_grid *d_grids;
    uint8_t *d_modules;
    sc.take(d_det, 1);
    sc.take(d_grids, (size_t)grid_capacity + 1);
    sc.take(d_modules, (size_t)module_capacity + 1);
    if ((rc = sc.alloc())) return rc;
    if ((rc = detect(&st.dev, binarize, d_det, d_grids, grid_capacity, d_modules, module_capacity, nullptr))) return rc;
    if ((rc = download_pageable(detection, d_det, sizeof(zg_qr_detection), nullptr))) return rc; // waits for the stream
    if (detection->grids_written && (rc = download_pageable(grids, d_grids, (size_t)detection->grids_written * sizeof(zg_qr_grid), nullptr))) return rc;
    if (detection->modules_written && (rc = download_pageable(modules, d_modules, detection->modules_written, nullptr))) return rc;
    return ZG_OK;
}

int zg_canvas_cmds_from_qr(const zg_qr_grid *grids, const zg_qr_detection *detection, uint32_t capacity, const uint8_t *color, uint32_t width, int mode,
                           zg_draw_cmd *cmds_out, uint32_t *count_out, zg_stream stream) {
    const char *what = "canvas_cmds_from_qr";
    ZG_REQUIRE(detection != nullptr && count_out != nullptr && color != nullptr, ZG_ERR_INVALID_ARGUMENT, "%s: null detection, count_out or color", what);
    ZG_REQUIRE(mode == ZG_DRAW_FAST || mode == ZG_DRAW_SOFT, ZG_ERR_INVALID_ARGUMENT, "%s: mode %d", what, mode);
    ZG_REQUIRE(width <= ZG_CANVAS_MAX_WIDTH, ZG_ERR_INVALID_ARGUMENT, "%s: width %u (at most %u)", what, width, ZG_CANVAS_MAX_WIDTH);
    ZG_REQUIRE(capacity == 0 || (grids != nullptr && cmds_out != nullptr), ZG_ERR_INVALID_ARGUMENT, "%s: null grids or cmds_out", what);
    uint32_t packed;
    std::memcpy(&packed, color, 4);
    const unsigned blocks = ceil_div(capacity ? capacity : 1u, 256);
    k_qr_build<<<blocks < 64u ? blocks : 64u, 256, 0, as_stream(stream)>>>(grids, detection, capacity, packed, width, mode, cmds_out, count_out);
    return launch_ok("k_qr_build");
}

} // extern "C"
