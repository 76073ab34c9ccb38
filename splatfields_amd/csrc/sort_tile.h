// Device-side bodies of the per-tile depth sort (one workgroup of 256 threads per list), shared by the standalone sort kernels
// (binning.hip) and the forward blend (render.hip), which sorts the list of its own tile before it blends it: ONE copy of
// the network.
#pragma once
#include "common.h"

namespace sr {

// ---- per-tile sort: register-resident bitonic network ---------------------------------------------------------
// 256 threads, E consecutive elements per thread (N = 256*E).  A compare-exchange at distance j is
//   j < E        : inside one thread's registers,
//   j < 64*E     : with lane (lane ^ j/E) of the same wavefront through a cross-lane shuffle,
//   otherwise    : with another wavefront through LDS -- exactly 3 such stages for every N.
// (A network living entirely in LDS moves all 12 bytes/entry through LDS log2(N)(log2(N)+1)/2 times -- 55 for N = 1024 --
// and was LDS-bandwidth bound in the first version; this one touches LDS 3 times.)
// Value of lane (lane ^ D) without touching LDS (ds_bpermute_b32 measured at ~24 cycles per wave-instruction
// per SIMD on MI355X, DPP adds/moves at ~4, v_permlane*_swap at ~8):
//   D = 1, 2 : DPP quad_perm          D = 8 : DPP row_ror:8 (rotation by 8 in a row of 16 is xor 8)
//   D = 4    : row_ror:4 for lanes with bit 2 set, row_ror:12 for the others
//   D = 16/32: v_permlane16_swap / v_permlane32_swap of the value with itself, then pick the swapped half
template <int D>
__device__ __forceinline__ uint32_t lane_xor(uint32_t x) {
    if constexpr (D == 1) return (uint32_t)__builtin_amdgcn_update_dpp(0, (int)x, 0xB1, 0xf, 0xf, false);
    else if constexpr (D == 2) return (uint32_t)__builtin_amdgcn_update_dpp(0, (int)x, 0x4E, 0xf, 0xf, false);
    else if constexpr (D == 8) return (uint32_t)__builtin_amdgcn_update_dpp(0, (int)x, 0x128, 0xf, 0xf, false);
    else if constexpr (D == 4) {
        const uint32_t a = (uint32_t)__builtin_amdgcn_update_dpp(0, (int)x, 0x124, 0xf, 0xf, false);  // from lane-4 (mod 16)
        const uint32_t b = (uint32_t)__builtin_amdgcn_update_dpp(0, (int)x, 0x12C, 0xf, 0xf, false);  // from lane+4 (mod 16)
        return (threadIdx.x & 4u) ? a : b;
    } else if constexpr (D == 16) {
        typedef unsigned int u2 __attribute__((ext_vector_type(2)));
        const u2 r = __builtin_amdgcn_permlane16_swap(x, x, false, false);  // r.x rows = (x0,x0,x2,x2), r.y rows = (x1,x1,x3,x3)
        return (threadIdx.x & 16u) ? r.x : r.y;
    } else {
        typedef unsigned int u2 __attribute__((ext_vector_type(2)));
        const u2 r = __builtin_amdgcn_permlane32_swap(x, x, false, false);  // r.x = (lo,lo), r.y = (hi,hi)
        return (threadIdx.x & 32u) ? r.x : r.y;
    }
}

// d is a compile-time constant after the network loops are unrolled; the dead branches fold away
__device__ __forceinline__ uint32_t lane_xor_d(uint32_t x, int d) {
    switch (d) {
        case 1: return lane_xor<1>(x);
        case 2: return lane_xor<2>(x);
        case 4: return lane_xor<4>(x);
        case 8: return lane_xor<8>(x);
        case 16: return lane_xor<16>(x);
        default: return lane_xor<32>(x);
    }
}

// The sort key is (view-depth bits << 32) | splat index: unique inside a tile (a splat appears once per tile), equal
// depths are ordered by splat index like the stable radix sort of the published pipeline.  The payload IS the low half
// of the key, so the network moves 8 bytes per entry and nothing else.
__device__ __forceinline__ void exchange_select(uint64_t& k, uint64_t pk, bool keep_min) {
    // keys are unique except for the +inf padding, where either choice is fine: one compare, mask xnor, 2 selects
    const bool take = (pk < k) == keep_min;
    k = take ? pk : k;
}

// `tid` is the thread's index inside its 256-thread group (several groups of one workgroup may run the same network
// side by side on different data; the barriers inside are workgroup-wide, so all groups must call it together).
template <int N, int E>
__device__ __forceinline__ void bitonic_regs(uint64_t (&k)[E], uint64_t* skey, uint32_t tid) {
#pragma unroll
    for (int kk = 2; kk <= N; kk <<= 1) {
#pragma unroll
        for (int j = kk >> 1; j > 0; j >>= 1) {
            if (j < E) {
#pragma unroll
                for (int e = 0; e < E; ++e) {
                    if ((e & j) == 0) {
                        const uint32_t i = tid * E + e;
                        const bool asc = (i & kk) == 0;
                        const bool swap = (k[e] > k[e | j]) == asc;
                        const uint64_t ka = k[e], kb = k[e | j];
                        k[e] = swap ? kb : ka; k[e | j] = swap ? ka : kb;
                    }
                }
            } else if (j < 64 * E) {
                const int d = j / E;
                const bool lower = (tid & d) == 0;
                // kk >= 2j > E here, so the direction bit (i & kk) depends on the thread only
                const bool keep_min = lower == (((tid * E) & kk) == 0);
                uint32_t plo[E], phi[E];
#pragma unroll
                for (int e = 0; e < E; ++e) {
                    plo[e] = lane_xor_d((uint32_t)k[e], d);
                    phi[e] = lane_xor_d((uint32_t)(k[e] >> 32), d);
                }
#pragma unroll
                for (int e = 0; e < E; ++e) exchange_select(k[e], ((uint64_t)phi[e] << 32) | plo[e], keep_min);
            } else {
                __syncthreads();
#pragma unroll
                for (int e = 0; e < E; ++e) skey[tid * E + e] = k[e];
                __syncthreads();
#pragma unroll
                for (int e = 0; e < E; ++e) {
                    const uint32_t i = tid * E + e;
                    const bool asc = (i & kk) == 0;
                    const bool lower = (i & j) == 0;
                    exchange_select(k[e], skey[i ^ j], lower == asc);
                }
            }
        }
    }
}

// Loads up to N = 256*E consecutive entries (padding with +inf keys), sorts them in registers; afterwards
// thread t holds the entries of rank t*E .. t*E+E-1.
template <int N, int E>
__device__ __forceinline__ void load_sort_chunk(const Binning& b, uint32_t first, uint32_t m, uint64_t (&k)[E], uint64_t* scratch_key, uint32_t tid) {
#pragma unroll
    for (int e = 0; e < E; ++e) {
        const uint32_t i = tid * E + e;
        k[e] = i < m ? b.ent[first + i] : ~0ull;
    }
    bitonic_regs<N, E>(k, scratch_key, tid);
}

template <int N, int E>
__device__ __forceinline__ void sort_tile_regs(const Binning& b, uint32_t start, uint32_t n, uint64_t* skey) {
    uint64_t k[E];
    load_sort_chunk<N, E>(b, start, n, k, skey, threadIdx.x);
#pragma unroll
    for (int e = 0; e < E; ++e) {
        const uint32_t i = threadIdx.x * E + e;
        if (i < n) b.sorted_id[start + i] = (uint32_t)k[e];
    }
}

// One merge pass in LDS: src[0, n) holds sorted runs of `width` entries (the last one may be short); adjacent pairs are
// merged, out(position, key) receives every entry with its position after the pass.  Merge path: a thread produces E
// consecutive outputs of its pair -- one binary search along the diagonal for where they start in the two runs
// (log2(width) probes per THREAD), then E sequential compare-and-advance steps with one LDS read each.  (Ranking every
// entry by its own binary search in the other run costs log2(width) dependent probes per ENTRY: a quarter to a third of the
// whole sort at lists of 2000-3000 entries.)  Keys are unique.  E divides 2 * width.
// merge_run_pairs_at: the thread's E outputs start at position o (a multiple of E).
template <int E, typename Out>
__device__ __forceinline__ void merge_run_pairs_at(const uint64_t* src, uint32_t n, uint32_t width, uint32_t o, Out&& out) {
    if (o >= n) return;
    const uint32_t base = o & ~(2u * width - 1u);  // start of the pair
    const uint64_t* A = src + base;                 // run B follows run A at A + width
    const uint32_t a = min(width, n - base);
    const uint32_t b = n - base - a < width ? n - base - a : width;
    const uint32_t d = o - base;                    // outputs of the pair before this thread's
    uint32_t lo = d > b ? d - b : 0u, hi = min(d, a);
    while (lo < hi) {                               // smallest ai with A[ai] > B[d - 1 - ai]
        const uint32_t mid = (lo + hi) >> 1;
        if (A[mid] < A[width + d - 1u - mid]) lo = mid + 1u; else hi = mid;
    }
    uint32_t ai = lo, bi = d - lo;
    constexpr uint64_t kInf = ~0ull;
    uint64_t ka = ai < a ? A[ai] : kInf;
    uint64_t kb = bi < b ? A[width + bi] : kInf;
#pragma unroll
    for (int e = 0; e < E; ++e) {
        const bool take_a = ka < kb;
        const uint64_t key = take_a ? ka : kb;
        if (d + (uint32_t)e < a + b) out(o + (uint32_t)e, key);
        ai += take_a ? 1u : 0u;
        bi += take_a ? 0u : 1u;
        const bool more = take_a ? ai < a : bi < b;
        const uint64_t nxt = A[take_a ? min(ai, a - 1u) : width + min(bi, max(b, 1u) - 1u)];
        if (take_a) ka = more ? nxt : kInf; else kb = more ? nxt : kInf;
    }
}

template <int E, typename Out>
__device__ __forceinline__ void merge_run_pairs(const uint64_t* src, uint32_t n, uint32_t width, Out&& out) {
    merge_run_pairs_at<E>(src, n, width, threadIdx.x * (uint32_t)E, out);   // first output of this thread
}

// Sorts n <= CAP entries starting at b.ent[first]: runs of 1024 are sorted by the register network into LDS (one
// 256-thread group per run, side by side), then merged pairwise (merge_run_pairs) until one run is left.  A list of 1100
// entries costs a 1024- and a 256-network instead of the 2048-network of a power-of-two bitonic sort.
// emit(rank, key) receives every entry with its final rank.  run_key: CAP entries, + CAP more when n > 2048.
// Ends with a workgroup barrier.
template <int CAP, int THREADS, typename Emit>
__device__ __forceinline__ void sort_block_lds(const Binning& b, uint32_t first, uint32_t n, uint64_t* run_key, Emit&& emit) {
    constexpr int GROUPS = THREADS / 256;
    const uint32_t group = threadIdx.x >> 8, tid = threadIdx.x & 255u;
    const uint32_t n_runs = (n + 1023u) / 1024u;
    for (uint32_t r0 = 0; r0 < n_runs; r0 += GROUPS) {  // uniform trip count: the barriers below are workgroup-wide
        const uint32_t r = r0 + group;
        const uint32_t m = r < n_runs ? min(1024u, n - r * 1024u) : 0u;
        __syncthreads();  // scratch reuse
        // Every network size has exactly 3 cross-wavefront (LDS) stages = 6 workgroup barriers, so groups may run
        // differently sized networks side by side: a short last run does not pay for a 1024-network.  A group uses the
        // 1024-entry area of its run as the scratch of those stages and then leaves the sorted run there.
        // r < CAP/1024 always (CAP/1024 is a multiple of GROUPS); an idle group (m = 0) sorts padding in its own free slot.
        uint64_t* rk = run_key + r * 1024u;
        uint64_t k[4];  // a 256- / 512-network uses the first 1 / 2 of them
        if (m <= 256u) {
            uint64_t k1[1];
            load_sort_chunk<256, 1>(b, first + r * 1024u, m, k1, rk, tid);
            k[0] = k1[0];
        } else if (m <= 512u) {
            uint64_t k2[2];
            load_sort_chunk<512, 2>(b, first + r * 1024u, m, k2, rk, tid);
            k[0] = k2[0]; k[1] = k2[1];
        } else {
            load_sort_chunk<1024, 4>(b, first + r * 1024u, m, k, rk, tid);
        }
        __syncthreads();  // every wavefront is past the last LDS stage of its network before the area is overwritten
        const uint32_t per = m <= 256u ? 1u : (m <= 512u ? 2u : 4u);
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const uint32_t i = tid * per + e;
            if ((uint32_t)e < per && i < m) rk[i] = k[e];
        }
    }
    __syncthreads();
    // Pairwise merge passes over the runs (1024 -> 2048 -> ...); the last one hands the entries to emit().  Lists of up
    // to 2048 entries (two runs) need one pass and no second buffer; longer ones ping-pong with run_key + CAP.
    uint64_t* src = run_key;
    uint64_t* dst = run_key + CAP;
    for (uint32_t width = 1024u;; width <<= 1) {
        if (2u * width >= n) {
            merge_run_pairs<CAP / THREADS>(src, n, width, emit);
            break;
        }
        merge_run_pairs<CAP / THREADS>(src, n, width, [&](uint32_t pos, uint64_t key) { dst[pos] = key; });
        __syncthreads();
        uint64_t* t = src; src = dst; dst = t;
    }
    __syncthreads();
}

// A list of 1..kSortSmallMax entries, sorted by ONE workgroup of 256 threads into b.sorted_id[start, start + n): up to 1024
// entries one register network; 1025..2048 two runs sorted one after the other + the merge pass.  skey: 2048 keys (16 KiB)
// of LDS.  Callers: the forward blend, for the list of its own tile, and k_sort_tiles_regs (the standalone switch).
constexpr uint32_t kSortSmallMax = 2048u;
__device__ __forceinline__ void sort_tile_small(const Binning& b, uint32_t start, uint32_t n, uint64_t* skey) {
    if (n <= 256u) sort_tile_regs<256, 1>(b, start, n, skey);
    else if (n <= 512u) sort_tile_regs<512, 2>(b, start, n, skey);
    else if (n <= 1024u) sort_tile_regs<1024, 4>(b, start, n, skey);
    else sort_block_lds<2048, 256>(b, start, n, skey, [&](uint32_t rank, uint64_t key) { b.sorted_id[start + rank] = (uint32_t)key; });
}

// The forward blend's version: a list of 1..kSortInlineMax (4096) entries with the SAME 16 KiB of LDS.  Up to 2048 entries it
// is sort_tile_small.  A longer list is sorted in two halves of up to 2048 (each as above: runs of 1024 + one merge pass in
// LDS) that go, as whole keys, to the global key buffer b.keys; one merge-path pass over those two runs through memory then
// writes b.sorted_id (a thread produces twice 8 consecutive outputs).  The workgroup's own stores are read back by its other
// wavefronts: release, barrier, acquire at workgroup scope.  One instance of sort_block_lds serves both cases (the branch in
// its emit is uniform): the kernel carries the network once.
// Costs a long list ~3x what k_sort_tiles_merge<2048, 4096, 1024> spends on it with 1024 threads and 64 KiB -- worth it only
// while such lists are few (kInlineLongTiles, below) and their workgroups start first (longest-list-first launch order).
constexpr uint32_t kSortInlineMax = 4096u;
__device__ __forceinline__ void sort_tile_inline(const Binning& b, uint32_t start, uint32_t n, uint64_t* skey) {
    if (n <= 256u) sort_tile_regs<256, 1>(b, start, n, skey);
    else if (n <= 512u) sort_tile_regs<512, 2>(b, start, n, skey);
    else if (n <= 1024u) sort_tile_regs<1024, 4>(b, start, n, skey);
    else {
        const bool halves = n > kSortSmallMax;   // uniform
        uint64_t* k0 = b.keys + start;
#pragma unroll 1
        for (uint32_t off = 0; off < n; off += kSortSmallMax) {
            // (opaque per iteration: hoisted out of this loop, the eight output addresses of every thread cost the kernel
            // sixteen registers across the whole network, and it spills)
            uint32_t* ids = b.sorted_id + start;
            asm volatile("" : "+s"(ids));
            sort_block_lds<2048, 256>(b, start + off, min(kSortSmallMax, n - off), skey, [&](uint32_t rank, uint64_t key) {
                if (halves) k0[off + rank] = key; else ids[rank] = (uint32_t)key;
            });
        }
        if (halves) {
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
            __syncthreads();
            __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
            // (in two rounds of 8 outputs per thread: 16 at once cost the kernel its register budget)
#pragma unroll 1
            for (uint32_t o = threadIdx.x * 8u; o < n; o += 256u * 8u)
                merge_run_pairs_at<8>(k0, n, kSortSmallMax, o, [&](uint32_t pos, uint64_t key) { b.sorted_id[start + pos] = (uint32_t)key; });
        }
    }
}

// Lists of 2049..4096 entries are sorted by the forward blend (sort_tile_inline) instead of k_sort_tiles_merge<2048, 4096, 1024>
// when the view has at most this many tiles that can hold one (Geom::total[4], k_scan_small) and no longer list at all
// (Geom::total[1] <= 4096): the headline views have one to eight.  Dense scenes, where hundreds of tiles are long, keep the
// merge launch.  Both kernels evaluate this on the device from the same two words, so they always take the same branch.
constexpr uint32_t kInlineLongTiles = 8u;
__device__ __forceinline__ bool few_long_tiles(uint32_t long_slots, uint32_t longest) { return long_slots <= kInlineLongTiles && longest <= kSortInlineMax; }

}  // namespace sr
