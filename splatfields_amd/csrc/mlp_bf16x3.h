// The fused MLP chains with split-bf16 matrix operands ("bf16x3", opt-in: sr_mlp_chain_bf16x3, sr_mlp_chain_group_bf16x3,
// sr_mlp_pack_bf16x3).  Included by mlp.hip inside its namespace, behind the fp32 and bf16 chains whose op interpreter, epilogue
// (mlp_epilogue_plain), argument structs (MlpK, MlpGroupK, MlpPackK) and vector types it uses; it is no translation unit of its own.
#pragma once

// ---- the same chains with split-bf16 matrix operands ("bf16x3", opt-in: sr_mlp_chain_bf16x3) -------------------------------
// Every operand v is split into two bfloat16 values, hi(v) = bf(v) and lo(v) = bf(v - hi(v)) (the fp32 subtraction is exact), and a
// product spends three bf16 MFMAs:
//     acc = bias + hi(W) . hi(x) + hi(W) . lo(x) + lo(W) . hi(x)            (backward ops: W^T and dZ, no bias)
// lo . lo is dropped (at most 2^-18 of the product; hi + lo itself keeps v to 2^-17, 2^-16 at a tie): 16 significant bits where
// plain bf16 carries 8.  The three MFMAs of one (chunk, output tile, point tile) go into the SAME accumulator, in this order:
// hi . hi, then hi . lo (low part of the state / memory channel), then lo . hi (low part of the weight); chunks in K order as in
// k_mlp_chain_bf16.  Products and sums are fp32 inside v_mfma_f32_16x16x32_bf16; everything outside the MFMA is the bf16 kernel's,
// that is the fp32 kernel's: fp32 bias as the accumulator's initial value, fp32 running state split once per op and state tile
// where it becomes an operand, memory channels split as they are loaded, epilogues, sign bits and all stores from the unrounded
// accumulators.  A non-finite operand has lo = inf - inf = NaN, a finite one that bf16 rounds to +-inf (|v| >= 2^127 (2 - 2^-8))
// has lo = -+inf: the accumulators such an operand reaches are not finite (NaN as soon as both parts meet non-zero factors).
//
// Packed matrix (k_mlp_pack_bf16x3), MT output tiles: per chunk c the hi block, then the lo block, each in the bf16 layout
//   bf16 index ((((2 c + part) * MT + mt) * 64 + lane) * 8 + j)  =  part(A[16 mt + (lane & 15)][32 c + 16 (j >> 2) + 4 (lane >> 4) + (j & 3)])
// part 0 = hi, 1 = lo: a chunk is 2 MT KiB, contiguous, and one double-buffered LDS-direct stage still fetches a whole chunk.
#ifndef SR_MLP_BF16X3_WAVES8
#define SR_MLP_BF16X3_WAVES8 2   // wavefronts per SIMD the 128-wide bf16x3 kernel is compiled for
#endif

__device__ __forceinline__ void mlp_split_bf16(const f32x4 a, const f32x4 b, bf16x8& hi, bf16x8& lo) {
#pragma unroll
    for (int e = 0; e < 8; ++e) {
        const float v = e < 4 ? a[e & 3] : b[e & 3];
        const __bf16 h = (__bf16)v;
        hi[e] = h;
        lo[e] = (__bf16)(v - (float)h);
    }
}

// One 32-channel chunk against all output tiles: three MFMAs per output tile and point tile.  `w` points at this lane's 16 bytes
// of output tile 0 of the hi block; the lo block starts `lo_off` vectors behind it (64 x the op's output tiles).
template <int HT, bool FULL>
__device__ __forceinline__ void mlp_chunk_bf16x3(f32x4 (&acc)[2][HT], const bf16x8* w, int out_tiles, int lo_off, const bf16x8 b0h,
                                                 const bf16x8 b0l, const bf16x8 b1h, const bf16x8 b1l) {
#pragma unroll
    for (int mt = 0; mt < HT; ++mt) {
        if (FULL || mt < out_tiles) {
            const bf16x8 ah = w[mt * 64], al = w[(FULL ? HT * 64 : lo_off) + mt * 64];
            acc[0][mt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(ah, b0h, acc[0][mt], 0, 0, 0);
            acc[1][mt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(ah, b1h, acc[1][mt], 0, 0, 0);
            acc[0][mt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(ah, b0l, acc[0][mt], 0, 0, 0);
            acc[1][mt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(ah, b1l, acc[1][mt], 0, 0, 0);
            acc[0][mt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(al, b0h, acc[0][mt], 0, 0, 0);
            acc[1][mt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(al, b1h, acc[1][mt], 0, 0, 0);
        }
    }
}

// body of k_mlp_chain_bf16x3 and k_mlp_chain_group_bf16x3: the op interpreter of mlp_chain_body_bf16 (its own copy: as a
// policy of one shared body the 64-wide kernels compile to other code and measured 1 % slower);
// s_w: two chunks of a packed matrix, [part][mt][lane]
template <int HT>
__device__ __forceinline__ void mlp_chain_body_bf16x3(const SrMlpOp* ops, const int n_ops, bf16x8 (&s_w)[2][HT * 128], int n_points, float slope) {
    const int wave = wave_id(), lane = lane_id();
    const int k = lane >> 4, n = lane & 15;
    const int p0 = (blockIdx.x * 4 + wave) * 32;              // first point of this wavefront
    int prow[2];                                              // this lane's point of each of the two point tiles (clamped)
    bool pvalid[2];
#pragma unroll
    for (int nt = 0; nt < 2; ++nt) { prow[nt] = min(p0 + 16 * nt + n, n_points - 1); pvalid[nt] = p0 + 16 * nt + n < n_points; }

    f32x4 prev[2][HT], acc[2][HT];
#pragma unroll
    for (int nt = 0; nt < 2; ++nt)
#pragma unroll
        for (int t = 0; t < HT; ++t) prev[nt][t] = (f32x4){0.f, 0.f, 0.f, 0.f};

    int buf = 0;
    for (int l = 0; l < n_ops; ++l) {
        const SrMlpOp L = ops[l];
        const bf16x8* w8 = reinterpret_cast<const bf16x8*>(L.w_packed);
        const int lo_off = L.out_tiles * 64;                   // 16-byte vectors of a chunk's hi block: mt x 64
        const int chunk_v = 2 * lo_off;                        // ... of a chunk: hi block + lo block, <= HT * 128
        const int n_chunks = (L.mem_tiles + L.reg_tiles) / 2;
        // LDS-direct staging as in k_mlp_chain: chunk c + 1 is requested under the MFMAs of chunk c and waited for at the top of
        // the next chunk; a wavefront copies whole 64-lane pieces
        auto stage = [&](int c, int into) {
            const bf16x8* src = w8 + (size_t)c * chunk_v;
            for (int j0 = 0; j0 < chunk_v; j0 += kBlock) {
                if (j0 + 64 * wave < chunk_v)
                    lds_copy16_async(src + j0 + (int)threadIdx.x, (uint32_t)__builtin_amdgcn_readfirstlane((int)lds_address(&s_w[into][j0 + 64 * wave])));
            }
        };
#pragma unroll
        for (int mt = 0; mt < HT; ++mt) {                      // the bias stays fp32: the accumulators' initial value
            f32x4 b4 = {0.f, 0.f, 0.f, 0.f};
            if (L.bias && mt < L.out_tiles) { const float4 t4 = reinterpret_cast<const float4*>(L.bias)[4 * mt + k]; b4 = (f32x4){t4.x, t4.y, t4.z, t4.w}; }
            acc[0][mt] = b4; acc[1][mt] = b4;
        }
        uint32_t mbits[2] = {0u, 0u};
        if (L.mask_bits) { mbits[0] = L.mask_bits[(size_t)prow[0] * 4 + k]; mbits[1] = L.mask_bits[(size_t)prow[1] * 4 + k]; }
        __syncthreads();          // everyone has left the previous op's last chunk
        stage(0, buf);
        int c = 0;
        const bool full = L.out_tiles == HT;                   // wave-uniform
        const bool store_vec = (L.store_row & 3) == 0 && (reinterpret_cast<uintptr_t>(L.store) & 15u) == 0;
        // ---- input channels that come from memory: split as they are loaded ----
        for (; c < L.mem_tiles / 2; ++c) {
            bf16x8 bh[2], bl[2];
#pragma unroll
            for (int nt = 0; nt < 2; ++nt) {
                const float* row = L.src + (size_t)prow[nt] * L.src_row + 32 * c + 4 * k;
                const float4 lo = *reinterpret_cast<const float4*>(row), hi = *reinterpret_cast<const float4*>(row + 16);
                mlp_split_bf16((f32x4){lo.x, lo.y, lo.z, lo.w}, (f32x4){hi.x, hi.y, hi.z, hi.w}, bh[nt], bl[nt]);
            }
            lds_copy_wait();      // this wavefront's pieces of chunk c have landed ...
            __syncthreads();      // ... and everybody's; the other buffer is free
            if (c + 1 < n_chunks) stage(c + 1, buf ^ 1);
            if (full) mlp_chunk_bf16x3<HT, true>(acc, &s_w[buf][lane], L.out_tiles, lo_off, bh[0], bl[0], bh[1], bl[1]);
            else mlp_chunk_bf16x3<HT, false>(acc, &s_w[buf][lane], L.out_tiles, lo_off, bh[0], bl[0], bh[1], bl[1]);
            buf ^= 1;
        }
        // ---- input channels that are the register state: each state tile is split once per op, here ----
#pragma unroll
        for (int cr = 0; cr < HT / 2; ++cr) {
            if (cr < L.reg_tiles / 2) {
                bf16x8 bh[2], bl[2];
                mlp_split_bf16(prev[0][2 * cr], prev[0][2 * cr + 1], bh[0], bl[0]);
                mlp_split_bf16(prev[1][2 * cr], prev[1][2 * cr + 1], bh[1], bl[1]);
                lds_copy_wait();
                __syncthreads();
                if (c + 1 < n_chunks) stage(c + 1, buf ^ 1);
                if (full) mlp_chunk_bf16x3<HT, true>(acc, &s_w[buf][lane], L.out_tiles, lo_off, bh[0], bl[0], bh[1], bl[1]);
                else mlp_chunk_bf16x3<HT, false>(acc, &s_w[buf][lane], L.out_tiles, lo_off, bh[0], bl[0], bh[1], bl[1]);
                buf ^= 1;
                ++c;
            }
        }
        // ---- epilogue: the fp32 kernel's, on unrounded fp32 accumulators ----
        const bool plain = full && p0 + 32 <= n_points && !L.keep_state &&
                           (L.epilogue == SR_MLP_LEAKY || (L.epilogue == SR_MLP_MASK && L.mask_bits)) &&
                           (!L.store || (store_vec && L.store_channels == 16 * HT && !L.store_accumulate));   // wave-uniform
        if (plain) { mlp_epilogue_plain<HT>(acc, prev, L, slope, mbits, p0, n, k); continue; }
        // (k_mlp_chain's generic epilogue, repeated as in mlp_chain_body_bf16: a shared function spills)
#pragma unroll
        for (int nt = 0; nt < 2; ++nt) {
            uint32_t signs = 0u;                                // bit 4 mt + i: channel 16 mt + 4 k + i of this point is > 0
#pragma unroll
            for (int mt = 0; mt < HT; ++mt) {
                f32x4 r = {0.f, 0.f, 0.f, 0.f};
                if (mt < L.out_tiles) {
                    r = acc[nt][mt];
                    if (L.epilogue == SR_MLP_LEAKY) {            // activation of a forward layer (leaky ReLU, 0 <= slope < 1)
#pragma unroll
                        for (int i = 0; i < 4; ++i) r[i] = fmaxf(r[i], slope * r[i]);
                    } else if (L.epilogue == SR_MLP_MASK) {      // backward: times leaky'(x), read off the saved activation's sign
                        if (L.mask_bits) {
#pragma unroll
                            for (int i = 0; i < 4; ++i) r[i] *= (mbits[nt] >> (4 * mt + i)) & 1u ? 1.0f : slope;
                        } else {
                            const float4 m4 = *reinterpret_cast<const float4*>(L.mask + (size_t)prow[nt] * L.mask_row + 16 * mt + 4 * k);
                            r[0] *= m4.x > 0.f ? 1.0f : slope; r[1] *= m4.y > 0.f ? 1.0f : slope;
                            r[2] *= m4.z > 0.f ? 1.0f : slope; r[3] *= m4.w > 0.f ? 1.0f : slope;
                        }
                    }
                    if (L.sign_store) {
#pragma unroll
                        for (int i = 0; i < 4; ++i) signs |= (r[i] > 0.f ? 1u : 0u) << (4 * mt + i);
                    }
                    if (L.store && pvalid[nt]) {
                        float* dst = L.store + (size_t)(p0 + 16 * nt + n) * L.store_row + 16 * mt + 4 * k;
                        if (store_vec && 16 * mt + 4 * k + 3 < L.store_channels) {       // whole float4 inside the row: one 16-byte access
                            float4 v = make_float4(r[0], r[1], r[2], r[3]);
                            if (L.store_accumulate) { const float4 o = *reinterpret_cast<const float4*>(dst); v.x += o.x; v.y += o.y; v.z += o.z; v.w += o.w; }
                            *reinterpret_cast<float4*>(dst) = v;
                        } else {
#pragma unroll
                            for (int i = 0; i < 4; ++i)
                                if (16 * mt + 4 * k + i < L.store_channels) dst[i] = L.store_accumulate ? dst[i] + r[i] : r[i];
                        }
                    }
                }
                if (!L.keep_state) prev[nt][mt] = r;
            }
            if (L.sign_store && pvalid[nt]) L.sign_store[(size_t)(p0 + 16 * nt + n) * 4 + k] = signs;
        }
    }
}

template <int HT>
__global__ void __launch_bounds__(kBlock) __attribute__((amdgpu_waves_per_eu(HT == 8 ? SR_MLP_BF16X3_WAVES8 : 3, HT == 8 ? SR_MLP_BF16X3_WAVES8 : 3))) k_mlp_chain_bf16x3(const MlpK net, int n_points, float slope) {
    __shared__ bf16x8 s_w[2][HT * 128];
    mlp_chain_body_bf16x3<HT>(net.op, net.n_ops, s_w, n_points, slope);
}

template <int HT>
__global__ void __launch_bounds__(kBlock) __attribute__((amdgpu_waves_per_eu(HT == 8 ? SR_MLP_BF16X3_WAVES8 : 3, HT == 8 ? SR_MLP_BF16X3_WAVES8 : 3))) k_mlp_chain_group_bf16x3(const MlpGroupK grp, int n_points, float slope) {
    __shared__ bf16x8 s_w[2][HT * 128];
    const int f0 = grp.first[blockIdx.y];
    mlp_chain_body_bf16x3<HT>(grp.op + f0, grp.first[blockIdx.y + 1] - f0, s_w, n_points, slope);
}

// The matrix of a job split into hi = bf(v) and lo = bf(v - hi) in the layout above: the lane -> K permutation of k_mlp_pack_bf16,
// per chunk the hi block and then the lo block (mlp_pack_bf16_parts<2>, mlp.hip).  The destination holds
// 2 x 16 out_tiles (mem_pad + reg_width) bfloat16.  The bias is copied as fp32.
__global__ void __launch_bounds__(kBlock) k_mlp_pack_bf16x3(const MlpPackK jobs) { mlp_pack_bf16_parts<2>(jobs); }
