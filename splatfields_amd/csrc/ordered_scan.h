// The middle launch of an ordered compaction (hull.hip, depth_init.hip): ONE workgroup of kScanBlock threads turns the survivor
// counts of the marking pass's workgroups into exclusive offsets, in index order.  No atomics: the same counts give the same bytes.
#pragma once
#include "common.h"

namespace sr {

constexpr int kScanBlock = 1024;

#ifdef __HIPCC__

// exclusive prefix over block_counts[0 .. blocks), in place; returns the total to every thread.  Called by all kScanBlock threads
// of the workgroup; contains barriers
__device__ __forceinline__ uint32_t ordered_scan_counts(long long blocks, uint32_t* __restrict__ block_counts) {
    __shared__ uint32_t s_wave[kScanBlock / kWave];
    uint32_t carry = 0u;                                  // the same value in every thread
    for (long long base = 0; base < blocks; base += kScanBlock) {
        const long long j = base + threadIdx.x;
        const uint32_t v = j < blocks ? block_counts[j] : 0u;
        const uint32_t inc = wave_inclusive_scan(v);
        __syncthreads();                                  // s_wave of the previous round has been read
        if (lane_id() == 63) s_wave[wave_id()] = inc;
        __syncthreads();
        uint32_t before = 0u, all = 0u;
#pragma unroll
        for (int w = 0; w < kScanBlock / kWave; ++w) {
            const uint32_t s = s_wave[w];
            if (w < wave_id()) before += s;
            all += s;
        }
        if (j < blocks) block_counts[j] = carry + before + inc - v;
        carry += all;
    }
    return carry;
}

#endif  // __HIPCC__

}  // namespace sr
