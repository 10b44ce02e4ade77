// The rank tracker of the sliding-histogram order-statistic kernel (zignal_amd/csrc/zg_order_stat_track.h) on the CPU, against a sort of
// the window. Built by tests/test_order_stat_track.py with -fsanitize=address,undefined and -D__host__= -D__device__=; includes nothing of
// the library but that header.
//
// A window of w = 2r + 1 rows of w samples slides down a column of rows, as one lane's window does in the kernel: the first w rows are added
// (os_hist_add), then each step takes the oldest row out and a new row in, alternately sample pair by sample pair (os_hist_replace, the
// kernel's form) and as w removes followed by w adds. After every step: the percentile at ranks 0, area / 2, area - 1 and one odd rank, the
// midpoint, and the alpha-trimmed mean for trim 0, 0.12 and 0.49. Rows of noise, of a 0 / 255 checkerboard in time (whole rows of 0 and of
// 255 alternate, so the median and both trim boundaries cross the whole value range at every step), of a constant, and of ramps.
// Radii 1, 2, 16 and 127 with u16 counters, 128 with u32 counters.
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <deque>
#include <vector>

#include "../../zignal_amd/csrc/zg_order_stat_track.h"

using namespace zg;

template <typename CNT> struct ArrayHist {
    CNT *bins;
    uint32_t get(int v) const { return bins[v]; }
    void set(int v, uint32_t c) const { bins[v] = (CNT)c; }
};

static uint32_t rng_state = 99;
static uint8_t noise() { rng_state = rng_state * 1664525u + 1013904223u; return (uint8_t)(rng_state >> 24); }

enum Pattern { NOISE, CHECKER, CONSTANT, RAMP_X, RAMP_T, N_PATTERNS };
static const char *const pattern_name[] = {"noise", "checker", "constant", "ramp-x", "ramp-t"};

static void make_row(std::vector<uint8_t> &row, int pattern, int t) {
    for (size_t i = 0; i < row.size(); ++i) {
        switch (pattern) {
        case NOISE: row[i] = noise(); break;
        case CHECKER: row[i] = (t & 1) ? 255 : 0; break;
        case CONSTANT: row[i] = 255; break;
        case RAMP_X: row[i] = (uint8_t)(i * 255 / (row.size() - 1)); break;
        default: row[i] = (uint8_t)(t * 7); break;
        }
    }
}

static int failures = 0;
static void expect(int got, int want, const char *what, int r, int pattern, int step) {
    if (got == want) return;
    if (++failures <= 20) std::printf("FAIL r=%d %s step %d: %s = %d, the sorted window gives %d\n", r, pattern_name[pattern], step, what, got, want);
}

template <typename CNT> static void slide(int r, int pattern, int steps) {
    const int w = 2 * r + 1;
    const uint32_t area = (uint32_t)w * (uint32_t)w;
    std::vector<CNT> bins(256, 0);
    const ArrayHist<CNT> h{bins.data()};
    const uint32_t ranks[4] = {0, area / 2, area - 1, (area / 3) | 1u};
    const double trims[3] = {0.0, 0.12, 0.49};
    uint32_t trim_each[3];
    for (int i = 0; i < 3; ++i) trim_each[i] = std::min<uint32_t>((uint32_t)std::floor(trims[i] * (double)area), area / 2);
    OsTracker pt[4], ta[3], tb[3];
    uint32_t total = 0;
    auto add = [&](int v) {
        for (auto &t : pt) os_add<false>(t, v);
        for (int i = 0; i < 3; ++i) { os_add<true>(ta[i], v); os_add<true>(tb[i], v); }
        total += (uint32_t)v;
    };
    auto remove = [&](int v) {
        for (auto &t : pt) os_remove<false>(t, v);
        for (int i = 0; i < 3; ++i) { os_remove<true>(ta[i], v); os_remove<true>(tb[i], v); }
        total -= (uint32_t)v;
    };
    std::deque<std::vector<uint8_t>> rows;
    std::vector<uint8_t> row((size_t)w), sorted;
    for (int t = 0; t < w + steps; ++t) {
        make_row(row, pattern, t);
        if (t < w) {
            for (int v : row) { os_hist_add(h, v); add(v); }
        } else if (t & 1) {
            const std::vector<uint8_t> &old = rows.front();
            for (int i = 0; i < w; ++i) { os_hist_replace(h, old[(size_t)i], row[(size_t)i]); add(row[(size_t)i]); remove(old[(size_t)i]); }
        } else {
            for (int v : rows.front()) { os_hist_remove(h, v); remove(v); }
            for (int v : row) { os_hist_add(h, v); add(v); }
        }
        if (t >= w) rows.pop_front();
        rows.push_back(row);
        if (t < w - 1) continue;
        for (int i = 0; i < 4; ++i) os_settle<false>(pt[i], h, ranks[i]);
        for (int i = 0; i < 3; ++i)
            if (trim_each[i] > 0) { os_settle<true>(ta[i], h, trim_each[i] - 1); os_settle<true>(tb[i], h, area - trim_each[i]); }
        sorted.clear();
        for (const auto &rw : rows) sorted.insert(sorted.end(), rw.begin(), rw.end());
        std::sort(sorted.begin(), sorted.end());
        if (sorted.size() != area) { ++failures; std::printf("FAIL window size\n"); return; }
        const char *const rank_name[4] = {"percentile rank 0", "percentile rank area/2", "percentile rank area-1", "percentile odd rank"};
        for (int i = 0; i < 4; ++i) expect(pt[i].m, sorted[ranks[i]], rank_name[i], r, pattern, t);
        expect(os_midpoint(pt[0].m, pt[2].m), (sorted.front() + sorted.back() + 1) / 2, "midpoint", r, pattern, t);
        const char *const trim_name[3] = {"trimmed mean 0", "trimmed mean 0.12", "trimmed mean 0.49"};
        for (int i = 0; i < 3; ++i) {
            uint64_t sum = 0;
            for (uint32_t k = trim_each[i]; k < area - trim_each[i]; ++k) sum += sorted[k];
            const uint64_t kept = area - 2 * trim_each[i];
            const uint64_t want = std::min<uint64_t>((sum + kept / 2) / kept, 255);
            expect(os_trimmed_mean(ta[i], tb[i], h, total, area, trim_each[i]), (int)want, trim_name[i], r, pattern, t);
        }
    }
}

int main() {
    for (int pattern = 0; pattern < N_PATTERNS; ++pattern) {
        slide<uint16_t>(1, pattern, 300);
        slide<uint16_t>(2, pattern, 300);
        slide<uint16_t>(16, pattern, 120);
        slide<uint16_t>(127, pattern, 12); // one bin reaches 65 025 on the constant rows: the largest count a u16 counter is asked to hold
        slide<uint32_t>(128, pattern, 12); // 66 049 there
    }
    if (failures) { std::printf("order-stat tracker: %d failure(s)\n", failures); return 1; }
    std::printf("order-stat tracker ok\n");
    return 0;
}
