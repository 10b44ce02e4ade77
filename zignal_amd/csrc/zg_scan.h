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

// ---- 64-bit values and operators that do not commute (metrics.hip) ---------------------------------------------------------------

// the calling thread's exclusive sum of a 64-bit v (uint64_t, int64_t or double) over the workgroup's 256 threads, and the sum of all in
// *total. A double is added in thread order inside a wave and in wave order across them: deterministic, not the sequential sum's bits.
template <typename T> __device__ inline T block_exclusive_sum64(T v, T *total) {
    static_assert(sizeof(T) == 8, "64-bit values");
    __shared__ T wave_sum[4];
    const uint32_t lane = threadIdx.x & 63u, wv = threadIdx.x >> 6;
    T incl = v;
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        const T up = __shfl_up(incl, off);
        if ((int)lane >= off) incl = up + incl;
    }
    __syncthreads(); // the previous call's reads of wave_sum are done
    if (lane == 63u) wave_sum[wv] = incl;
    __syncthreads();
    T base = 0, all = 0;
    for (uint32_t k = 0; k < 4; ++k) {
        if (k < wv) base += wave_sum[k];
        all += wave_sum[k];
    }
    *total = all;
    return base + (incl - v);
}

// v of the lane `off` above the calling one, for any value made of 32-bit words
template <typename T> __device__ inline T shfl_down_words(const T &v, int off) {
    static_assert(sizeof(T) % 4 == 0, "whole 32-bit words");
    constexpr int N = (int)(sizeof(T) / 4);
    int w[N];
    __builtin_memcpy(w, &v, sizeof(T));
#pragma unroll
    for (int i = 0; i < N; ++i) w[i] = __shfl_down(w[i], off);
    T r;
    __builtin_memcpy(&r, w, sizeof(T));
    return r;
}

// op(v[0], op(v[1], ...)) over the 256 threads of the workgroup IN THREAD ORDER, for an associative op that need not commute (a sum, or
// the composition of transducers): a lane's value stands for the threads [lane, lane + width) of its wave and takes in the next width
// at every step. The result is thread 0's return value; every other thread's is unspecified. Whole workgroups call it (two barriers).
template <typename T, typename Op> __device__ inline T block_reduce_ordered(T v, Op op) {
    __shared__ T wave_value[4];
    const uint32_t lane = threadIdx.x & 63u, wv = threadIdx.x >> 6;
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        const T next = shfl_down_words(v, off);
        if ((int)lane + off < 64) v = op(v, next);
    }
    __syncthreads(); // the previous call's reads of wave_value are done
    if (lane == 0) wave_value[wv] = v;
    __syncthreads();
    if (threadIdx.x == 0) {
#pragma unroll
        for (int k = 1; k < 4; ++k) v = op(v, wave_value[k]);
    }
    return v;
}

} // namespace zg
