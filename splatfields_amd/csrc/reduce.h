// The fixed-order sums of the fused ops (loss, Moran, metrics, objective, plane generator): the promise "bit-identical from
// call to call" of those ops rests on the order of addition here, and on nothing else.  Two orders, one name each:
//
//   wave_sum / block_sum   a shuffle tree inside each wavefront, then the wavefronts' sums added in index order;
//   block_tree_sum         a halving tree over one LDS slot per thread.
//
// The DPP sums of the rasterizer (common.h) are a third order with another purpose and stay there.
#pragma once
#include "common.h"

namespace sr {

// sum over the wavefront: lane l adds lane l + 32, l + 16, ... l + 1; valid in lane 0.  No LDS, no barrier.
template <typename T>
__device__ __forceinline__ T wave_sum(T v) {
#pragma unroll
    for (int d = kWave / 2; d > 0; d >>= 1) v += __shfl_down(v, d, kWave);
    return v;
}

// sum over a workgroup of kBlock threads: wave_sum, then wavefront 0, 1, 2, 3 in this order; valid in thread 0 (T(0) in
// every other thread).  `s_red` holds kBlock / kWave entries.  Two barriers: every thread of the workgroup calls it, and
// `s_red` is free again on return.
template <typename T>
__device__ __forceinline__ T block_sum(T v, T* s_red) {
    v = wave_sum(v);
    if ((threadIdx.x & (kWave - 1)) == 0) s_red[threadIdx.x / kWave] = v;
    __syncthreads();
    T r = T(0);
    if (threadIdx.x == 0) {
#pragma unroll
        for (int w = 0; w < kBlock / kWave; ++w) r += s_red[w];
    }
    __syncthreads();
    return r;
}

// sum over a workgroup of kThreads threads (a power of two) by halving: slot t adds slot t + kThreads / 2, then
// t + kThreads / 4, ...; valid in every thread.  `red` holds kThreads entries.  2 + log2(kThreads) barriers: every thread
// of the workgroup calls it, and `red` is free again on return.
template <typename T, int kThreads>
__device__ __forceinline__ T block_tree_sum(T v, T* red) {
    const int tid = threadIdx.x;
    red[tid] = v;
    __syncthreads();
#pragma unroll
    for (int s = kThreads / 2; s > 0; s >>= 1) {
        if (tid < s) red[tid] += red[tid + s];
        __syncthreads();
    }
    const T r = red[0];
    __syncthreads();
    return r;
}

}  // namespace sr
