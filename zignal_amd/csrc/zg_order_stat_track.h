// zg_order_stat_track.h — the incremental rank tracker of the sliding-histogram order-statistic kernel (order_stat.hip, k_order_stat_hist),
// written once for the device and the host: tests/c/order_stat_track.cpp compiles this header with plain g++ (-D__host__= -D__device__=)
// and checks every function against a sort of the window, so the CPU test runs the code the kernel runs. Nothing here includes anything
// of HIP or of this library.
//
// A histogram is anything with `uint32_t get(int v) const` and `void set(int v, uint32_t count) const` over v = 0..255 (the kernel: one
// lane's 256 bins in LDS, u16 or u32 counters; the test: an array). A tracker for rank k (0-based, k < number of samples) is (m, below,
// below_sum) with the invariant below = #samples < m and below_sum = their sum; os_add / os_remove keep the invariant when a sample
// enters or leaves, os_settle then moves m to the value of the (k+1)-th smallest sample: the smallest m with below + hist[m] > k.
// Counts and sums fit 32 bits up to radius 256: 255 * 513^2 < 2^27.
#pragma once
#include <stdint.h>

namespace zg {

struct OsTracker {
    int m = 0;               // the tracked value, 0..255
    uint32_t below = 0;      // samples < m
    uint32_t below_sum = 0;  // their sum (kept only where SUM is set)
};

template <class Hist> __host__ __device__ inline void os_hist_add(const Hist &h, int v) { h.set(v, h.get(v) + 1u); }
template <class Hist> __host__ __device__ inline void os_hist_remove(const Hist &h, int v) { h.set(v, h.get(v) - 1u); }
// One sample leaves and one enters: both counters are read before either is written (two independent reads instead of a chain of two
// read-modify-writes), and when the two values are equal the second store puts the unchanged count back.
template <class Hist> __host__ __device__ inline void os_hist_replace(const Hist &h, int leaving, int entering) {
    const uint32_t cl = h.get(leaving), ce = h.get(entering);
    h.set(leaving, cl - 1u);
    h.set(entering, ce + (entering == leaving ? 0u : 1u));
}

template <bool SUM> __host__ __device__ inline void os_add(OsTracker &t, int v) {
    const uint32_t lt = v < t.m ? 1u : 0u;
    t.below += lt;
    if (SUM) t.below_sum += lt * (uint32_t)v;
}
template <bool SUM> __host__ __device__ inline void os_remove(OsTracker &t, int v) {
    const uint32_t lt = v < t.m ? 1u : 0u;
    t.below -= lt;
    if (SUM) t.below_sum -= lt * (uint32_t)v;
}

// After any number of adds and removes: m becomes the value at rank k. The bounds on m never bind while the invariant holds (below > k >= 0
// needs m > 0; at m = 255, below + hist[255] is the number of samples, which exceeds k); they keep a broken invariant from walking off the bins.
template <bool SUM, class Hist> __host__ __device__ inline void os_settle(OsTracker &t, const Hist &h, uint32_t k) {
    while (t.below > k && t.m > 0) {
        --t.m;
        const uint32_t c = h.get(t.m);
        t.below -= c;
        if (SUM) t.below_sum -= c * (uint32_t)t.m;
    }
    for (;;) {
        const uint32_t c = h.get(t.m);
        if (t.below + c > k || t.m >= 255) break;
        t.below += c;
        if (SUM) t.below_sum += c * (uint32_t)t.m;
        ++t.m;
    }
}

// midpoint of the window from its smallest and largest value (order_statistic_blur.zig:318-325)
__host__ __device__ inline int os_midpoint(int mn, int mx) { return (mn + mx + 1) / 2; }

// Alpha-trimmed mean (order_statistic_blur.zig:327-375) from the window's total, and for trim_each > 0 from two settled trackers: a at rank
// trim_each - 1 and b at rank area - trim_each. The trim_each smallest samples are all those below a plus as many copies of a as are
// missing; the trim_each largest likewise from above b. trim_each <= area / 2 and area is odd, so at least one sample is kept.
template <class Hist>
__host__ __device__ inline int os_trimmed_mean(const OsTracker &a, const OsTracker &b, const Hist &h, uint32_t total, uint32_t area, uint32_t trim_each) {
    uint32_t low = 0, high = 0;
    if (trim_each > 0) {
        low = a.below_sum + (trim_each - a.below) * (uint32_t)a.m;
        const uint32_t hb = h.get(b.m);
        const uint32_t cnt_gt = area - b.below - hb;
        const uint32_t sum_gt = total - b.below_sum - hb * (uint32_t)b.m;
        high = sum_gt + (trim_each - cnt_gt) * (uint32_t)b.m;
    }
    const uint32_t kept = area - 2u * trim_each;
    const uint32_t rounded = ((total - low - high) + kept / 2u) / kept;
    return (int)(rounded > 255u ? 255u : rounded);
}

} // namespace zg
