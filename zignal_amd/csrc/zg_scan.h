// zg_scan.h — prefix sums over a wave and over a workgroup of 256 threads (four waves), for the kernels that place list entries.
#pragma once
#include "zg_common.h"

namespace zg {

// the calling lane's inclusive sum of v over its wave's 64 lanes
__device__ inline uint32_t wave_inclusive_sum(uint32_t v) {
    const uint32_t lane = threadIdx.x & 63u;
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        const uint32_t up = __shfl_up(v, off);
        if ((int)lane >= off) v += up;
    }
    return v;
}

// the calling thread's exclusive sum of v over the workgroup's 256 threads, and the sum of all in *total
__device__ inline uint32_t block_exclusive_sum(uint32_t v, uint32_t *total) {
    __shared__ uint32_t wave_sum[4];
    const uint32_t lane = threadIdx.x & 63u, wv = threadIdx.x >> 6;
    const uint32_t incl = wave_inclusive_sum(v);
    __syncthreads(); // the previous call's reads of wave_sum are done
    if (lane == 63u) wave_sum[wv] = incl;
    __syncthreads();
    uint32_t base = 0, all = 0;
    for (uint32_t k = 0; k < 4; ++k) {
        base += k < wv ? wave_sum[k] : 0u;
        all += wave_sum[k];
    }
    *total = all;
    return base + incl - v;
}

// The same for a flag a thread: how many threads before the calling one have pred set, and how many have in all. A ballot and a
// population count stand for the wave's scan. The second barrier ends the call: the next one may write wave_n at once.
__device__ inline uint32_t block_exclusive_count(bool pred, uint32_t *total) {
    __shared__ uint32_t wave_n[4];
    const uint32_t lane = threadIdx.x & 63u, wv = threadIdx.x >> 6;
    const uint64_t ballot = __ballot(pred);
    if (lane == 0) wave_n[wv] = (uint32_t)__popcll(ballot);
    __syncthreads();
    uint32_t before = 0, all = 0;
    for (uint32_t k = 0; k < 4; ++k) {
        before += k < wv ? wave_n[k] : 0u;
        all += wave_n[k];
    }
    __syncthreads();
    *total = all;
    return before + (uint32_t)__popcll(ballot & ((1ull << lane) - 1ull));
}

} // namespace zg
