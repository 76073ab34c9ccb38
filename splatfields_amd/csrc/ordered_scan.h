// Ordered scans and compaction without atomics: the same counts give the same bytes from call to call.
//
//   ordered_scan       ONE workgroup of kScanBlock threads turns n integer counts into exclusive offsets, in index order.  Every
//                      single-workgroup scan outside the rasterizer is this routine: the hull's and the depth op's workgroup
//                      counts, the densify plan's [kind][workgroup] counts, the k-NN's cells and reverse edges, the tri-plane's bins.
//   compaction_mark    the marking pass of an ordered compaction (hull.hip, depth_init.hip): one bit per item, one count per workgroup;
//   compaction_rank    its gathering pass: the rank of an item among the survivors, from those bits and the scanned counts.
#pragma once
#include "common.h"

namespace sr {

constexpr int kScanBlock = 1024;
constexpr int kScanRound = 4096;                          // counts per round of ordered_scan (tests read this line)
constexpr int kScanItems = kScanRound / kScanBlock;       // consecutive counts per thread and round

#ifdef __HIPCC__

// Exclusive prefix over n counts: count i is load(i), and store(i, prefix) receives the sum of the counts in front of it.  Returns
// the total to every thread.  Called by ALL kScanBlock threads of a single workgroup.
//
// A thread reads the kScanItems counts it owns in a round before it stores any of them, and no thread touches another's, so
// load and store may name the same array (a scan in place).
//
// Barriers: two per round.  The trip count depends on n alone, which is the same in every thread, and neither barrier stands under
// a condition: every thread reaches every barrier.  The second one closes the round, so the routine's LDS is free again on return
// (and what `store` wrote is visible to the workgroup once the caller has passed a barrier of its own).
template <typename Load, typename Store>
__device__ __forceinline__ uint32_t ordered_scan(long long n, Load&& load, Store&& store) {
    __shared__ uint32_t s_wave[kScanBlock / kWave];
    uint32_t carry = 0u;                                  // the same value in every thread
    for (long long base = 0; base < n; base += kScanRound) {
        const long long i = base + (long long)kScanItems * threadIdx.x;
        uint32_t v[kScanItems];
        if (i + kScanItems <= n) {                        // the whole group lies inside: plain loads, which the compiler may merge
#pragma unroll
            for (int k = 0; k < kScanItems; ++k) v[k] = load(i + k);
        } else {
#pragma unroll
            for (int k = 0; k < kScanItems; ++k) v[k] = i + k < n ? load(i + k) : 0u;
        }
        uint32_t sum = 0u;
#pragma unroll
        for (int k = 0; k < kScanItems; ++k) sum += v[k];
        const uint32_t inc = wave_inclusive_scan(sum);
        if (lane_id() == 63) s_wave[wave_id()] = inc;
        __syncthreads();
        uint32_t before = 0u, all = 0u;
#pragma unroll
        for (int w = 0; w < kScanBlock / kWave; ++w) {
            const uint32_t s = s_wave[w];
            if (w < wave_id()) before += s;
            all += s;
        }
        uint32_t prefix = carry + before + inc - sum;
        if (i + kScanItems <= n) {
#pragma unroll
            for (int k = 0; k < kScanItems; ++k) { store(i + k, prefix); prefix += v[k]; }
        } else {
#pragma unroll
            for (int k = 0; k < kScanItems; ++k) { if (i + k < n) store(i + k, prefix); prefix += v[k]; }
        }
        carry += all;
        __syncthreads();                                  // s_wave has been read: the next round, or the caller, may write LDS
    }
    return carry;
}

// Marking pass, item i = blockIdx.x * kBlock + threadIdx.x of a kBlock-thread workgroup: the wavefront's survivors become one
// 64-bit word at words[i / kWave] (= 4 blockIdx + wave: the word array holds whole workgroups, so the waves of the last one that
// start past n have their slot too), the workgroup's count goes to block_counts[blockIdx.x].
// Precondition: EVERY lane of the workgroup calls it, and lanes past n vote 0.  One barrier between the waves' stores and the
// count; LDS that the caller wrote before the call may be read after it.
__device__ __forceinline__ void compaction_mark(bool alive, long long i, unsigned long long* __restrict__ words,
                                                uint32_t* __restrict__ block_counts) {
    __shared__ uint32_t s_count[kBlock / kWave];
    const unsigned long long word = __ballot(alive);
    if (lane_id() == 0) {
        words[i / kWave] = word;
        s_count[wave_id()] = (uint32_t)__popcll(word);
    }
    __syncthreads();
    if (threadIdx.x == 0) block_counts[blockIdx.x] = s_count[0] + s_count[1] + s_count[2] + s_count[3];
}

// Gathering pass, the same item numbering: false for a lane whose bit is clear; otherwise `rank` = the rank of this lane's item among
// all survivors = its workgroup's offset (the scanned block_counts) + the bits of the workgroup's earlier words + the bits of the
// lower lanes.  (A flag, not a negative rank: the caller then tests nothing on the survivors' path, and a wavefront without a
// survivor leaves after one load -- instruction for instruction what the two gather kernels were before they shared this.)
__device__ __forceinline__ bool compaction_rank(const unsigned long long* __restrict__ words, const uint32_t* __restrict__ block_offsets, long long& rank) {
    const long long w0 = (long long)blockIdx.x * (kBlock / kWave);
    const int w = wave_id(), lane = lane_id();
    const unsigned long long word = words[w0 + w];
    if (!((word >> lane) & 1ull)) return false;
    rank = block_offsets[blockIdx.x];
    for (int k = 0; k < w; ++k) rank += __popcll(words[w0 + k]);
    rank += __popcll(word & ((1ull << lane) - 1ull));
    return true;
}

#endif  // __HIPCC__

}  // namespace sr
