// Fused MLP kernels of the SplatFields deform network for gfx950: the layer chain (forward, and the
// activation-gradient chain of the backward), the weight packer, and the weight-gradient kernel.  The chain and the packer exist
// three times: exact fp32 (the default, described here) and, opt-in, with bf16 matrix operands (k_mlp_chain_bf16 below) or with
// operands split into two bf16 values, three MFMAs per product (k_mlp_chain_bf16x3, mlp_bf16x3.h).  Each chain has its own copy
// of the op interpreter: as policies of one shared body the fp32 and bf16x3 kernels compile to other code and measured slower
// (DESIGN.md section 22); the packers share what they have in common (mlp_pack_source, mlp_pack_bias, mlp_pack_bf16_parts).
//
// What it replaces: reference utils/time_utils.py:123-191 (`GeneralMLP`: Linear -> activation for every layer, the
// input concatenated back in front of the hidden state after the `skips` layers), which PyTorch-ROCm runs as one GEMM +
// several elementwise kernels per layer with every activation round-tripping through HBM (the
// network is 98 % of a 4-D step).  Here a workgroup carries 128 points through ALL layers: activations never leave the
// registers, weights stream through LDS once per 128 points.
//
// MI355X mapping: Y^T[out x points] = W[out x in] . X^T[in x points] on `v_mfma_f32_16x16x4_f32` (exact fp32 fma chains),
// points in the N dimension (lanes n = lane & 15), so the accumulator of one layer -- lane (k, n), tile t, register i =
// output channel 16 t + 4 k + i of point n -- is EXACTLY the B operand of the next layer once the weights are packed with
// their input index permuted to (t, i, k): step (t, i) of the K loop takes channel 16 t + 4 k + i from lane group k.
// Bias is the accumulator's initial value, the activation a per-register operation.  A wavefront holds 2 x 16 points;
// a workgroup's 4 wavefronts share the weight chunks (2 channel tiles = 32 input channels at a time, double-buffered).
//
// The kernel executes a list of OPS; an op is one matrix applied to [memory channels | the register state]:
//   forward layer     acc = b + W [x0 | h];  h <- leaky(acc);  optionally stored (the backward's saved activations, the output)
//   backward, hidden  acc = W_h^T dZ;        dZ <- acc * leaky'(saved activation of the layer below);  stored for dW = dZ^T X
//   backward, input   acc = W_x^T dZ;        added to dL/dx0 in memory, the register state is kept
// so the same code walks the network in both directions (the backward's matrices are the transposed blocks, packed the same
// way); the weight gradients are a second kernel over the stored dZ and activations (k_mlp_weight_grad below).
//
// Packed matrix with MT output tiles and KT input tiles (host side: splatfields_amd/fused_mlp.py):
//   float index ((((c * MT + mt) * 2 + tl) * 64 + lane) * 4 + i)  =  A[16 mt + (lane & 15)][16 (2 c + tl) + 4 (lane >> 4) + i]
// (zero beyond the matrix's true sizes), bias padded to 16 MT floats.
#include "host_api.h"

namespace sr {

namespace {

typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));

constexpr int kMlpMaxOps = SR_MLP_MAX_OPS;
struct MlpK { int n_ops; SrMlpOp op[kMlpMaxOps]; };

// One 16-channel input tile (4 MFMA K steps) against all output tiles.  `w` points at this lane's float4 of output tile 0
// (consecutive output tiles are 128 float4 apart).  FULL (every one of the HT output tiles is live, the common case): the LDS
// reads of SR_MLP_GROUP output tiles are issued together and the MFMAs rotate over twice as many accumulators, so neither the LDS latency
// nor the dependent accumulate chains stall the matrix pipe; otherwise tile by tile under a wave-uniform test.
#ifndef SR_MLP_GROUP
#define SR_MLP_GROUP 2      // output tiles whose LDS reads are issued together (the MFMAs rotate over 2 x this many accumulators);
                            // 4 costs 8 more registers at the 256-register ceiling of the 128-wide kernel: measured 3-5 % slower
#endif
#ifndef SR_MLP_WAVES8
#define SR_MLP_WAVES8 2     // wavefronts per SIMD the 128-wide kernel is compiled for (256 / 168 VGPRs)
#endif
template <int HT, bool FULL>
__device__ __forceinline__ void mlp_tile(f32x4 (&acc)[2][HT], const float4* w, int out_tiles, const f32x4 b0, const f32x4 b1) {
    if constexpr (FULL) {
#pragma unroll
        for (int h = 0; h < HT; h += SR_MLP_GROUP) {
            float4 a[SR_MLP_GROUP];
#pragma unroll
            for (int m = 0; m < SR_MLP_GROUP; ++m) a[m] = w[(h + m) * 128];
#pragma unroll
            for (int i = 0; i < 4; ++i)
#pragma unroll
                for (int m = 0; m < SR_MLP_GROUP; ++m) {
                    const float av = i == 0 ? a[m].x : i == 1 ? a[m].y : i == 2 ? a[m].z : a[m].w;
                    acc[0][h + m] = __builtin_amdgcn_mfma_f32_16x16x4f32(av, b0[i], acc[0][h + m], 0, 0, 0);
                    acc[1][h + m] = __builtin_amdgcn_mfma_f32_16x16x4f32(av, b1[i], acc[1][h + m], 0, 0, 0);
                }
        }
    } else {
#pragma unroll
        for (int mt = 0; mt < HT; ++mt) {
            if (mt < out_tiles) {
                const float4 a4 = w[mt * 128];
                acc[0][mt] = __builtin_amdgcn_mfma_f32_16x16x4f32(a4.x, b0[0], acc[0][mt], 0, 0, 0);
                acc[1][mt] = __builtin_amdgcn_mfma_f32_16x16x4f32(a4.x, b1[0], acc[1][mt], 0, 0, 0);
                acc[0][mt] = __builtin_amdgcn_mfma_f32_16x16x4f32(a4.y, b0[1], acc[0][mt], 0, 0, 0);
                acc[1][mt] = __builtin_amdgcn_mfma_f32_16x16x4f32(a4.y, b1[1], acc[1][mt], 0, 0, 0);
                acc[0][mt] = __builtin_amdgcn_mfma_f32_16x16x4f32(a4.z, b0[2], acc[0][mt], 0, 0, 0);
                acc[1][mt] = __builtin_amdgcn_mfma_f32_16x16x4f32(a4.z, b1[2], acc[1][mt], 0, 0, 0);
                acc[0][mt] = __builtin_amdgcn_mfma_f32_16x16x4f32(a4.w, b0[3], acc[0][mt], 0, 0, 0);
                acc[1][mt] = __builtin_amdgcn_mfma_f32_16x16x4f32(a4.w, b1[3], acc[1][mt], 0, 0, 0);
            }
        }
    }
}

// Epilogue of the common ops -- every output tile live, all 32 points of the wavefront valid, the store (if any) covering whole
// aligned float4 rows and not accumulating, the result replacing the state: per tile 4 activations + one 16-byte store, the
// only branches wave-uniform (scalar) ones on the op's kind.  (The generic epilogue below decides validity, vector or scalar
// store, accumulation and the channel bound per tile and per channel at run time; the compiler turned that into ~20 branches
// and exec-mask sequences per tile, a quarter of the kernel's time with stores.)
template <int HT>
__device__ __forceinline__ void mlp_epilogue_plain(const f32x4 (&acc)[2][HT], f32x4 (&prev)[2][HT], const SrMlpOp& L, float slope,
                                                   const uint32_t (&mbits)[2], int p0, int n, int k) {
    const bool leaky = L.epilogue == SR_MLP_LEAKY, has_store = L.store != nullptr, has_signs = L.sign_store != nullptr;
#pragma unroll
    for (int nt = 0; nt < 2; ++nt) {
        float* dst = L.store + (size_t)(p0 + 16 * nt + n) * L.store_row + 4 * k;
        uint32_t signs = 0u;                                // bit 4 mt + i: channel 16 mt + 4 k + i of this point is > 0
#pragma unroll
        for (int mt = 0; mt < HT; ++mt) {
            f32x4 r = acc[nt][mt];
            if (leaky) {
#pragma unroll
                for (int i = 0; i < 4; ++i) r[i] = fmaxf(r[i], slope * r[i]);
            } else {
#pragma unroll
                for (int i = 0; i < 4; ++i) r[i] *= (mbits[nt] >> (4 * mt + i)) & 1u ? 1.0f : slope;
            }
            if (has_signs) {
#pragma unroll
                for (int i = 0; i < 4; ++i) signs |= (r[i] > 0.f ? 1u : 0u) << (4 * mt + i);
            }
            if (has_store) *reinterpret_cast<float4*>(dst + 16 * mt) = make_float4(r[0], r[1], r[2], r[3]);
            prev[nt][mt] = r;
        }
        if (has_signs) L.sign_store[(size_t)(p0 + 16 * nt + n) * 4 + k] = signs;
    }
}

// The chain itself, for one workgroup of 128 points and one op table: the body of k_mlp_chain (one network per launch) and of
// k_mlp_chain_group (blockIdx.y picks the network).  `ops` points into the kernel argument; s_w: two chunks of a packed matrix,
// [mt][tl][lane].  Every barrier below is reached by the whole workgroup: the op table is the workgroup's own.
template <int HT>
__device__ __forceinline__ void mlp_chain_body(const SrMlpOp* ops, const int n_ops, float4 (&s_w)[2][HT * 2 * 64], int n_points, float slope) {
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
        const float4* w4 = reinterpret_cast<const float4*>(L.w_packed);
        const int chunk_f4 = L.out_tiles * 128;                // float4 per chunk: mt x 2 x 64
        const int n_chunks = (L.mem_tiles + L.reg_tiles) / 2;
        // A chunk travels memory -> LDS by LDS-direct loads (global_load_lds_dwordx4: 16 bytes per lane land at consecutive LDS
        // addresses, no staging registers, no ds_write) that are REQUESTED here and waited for at the top of the next chunk
        // (lds_copy_wait + barrier): the copy of chunk c + 1 runs under the 128 MFMAs of chunk c.  (Rounds 2-5 loaded the chunk into
        // registers and stored it: an in-order wavefront sat through the L2 round trip in front of every chunk's MFMAs -- it was
        // in its MFMA phases 55 % of its life.)
        auto stage = [&](int c, int into) {
            const float4* src = w4 + (size_t)c * chunk_f4;
            for (int j0 = 0; j0 < chunk_f4; j0 += kBlock) {           // chunk_f4 is a multiple of 128: whole wavefronts
                if (j0 + 64 * wave < chunk_f4)   // (the LDS base is a scalar operand: wave-uniform by construction, told to the compiler)
                    lds_copy16_async(src + j0 + (int)threadIdx.x, (uint32_t)__builtin_amdgcn_readfirstlane((int)lds_address(&s_w[into][j0 + 64 * wave])));
            }
        };
        // accumulators start at the bias: rows 4k..4k+3 of output tile mt
#pragma unroll
        for (int mt = 0; mt < HT; ++mt) {
            f32x4 b4 = {0.f, 0.f, 0.f, 0.f};
            if (L.bias && mt < L.out_tiles) { const float4 t4 = reinterpret_cast<const float4*>(L.bias)[4 * mt + k]; b4 = (f32x4){t4.x, t4.y, t4.z, t4.w}; }
            acc[0][mt] = b4; acc[1][mt] = b4;
        }
        // backward: leaky'(.) of the layer below as one bit per channel (written by the forward's sign_store): one dword per
        // point tile, requested here and used in the epilogue, instead of the 16 float4 of the saved activations themselves
        uint32_t mbits[2] = {0u, 0u};
        if (L.mask_bits) { mbits[0] = L.mask_bits[(size_t)prow[0] * 4 + k]; mbits[1] = L.mask_bits[(size_t)prow[1] * 4 + k]; }
        __syncthreads();          // everyone has left the previous op's last chunk
        stage(0, buf);
        int c = 0;
        // ---- input channels that come from memory (the network input / skip connection; the top gradient) ----
        const bool full = L.out_tiles == HT;                   // wave-uniform
        const bool store_vec = (L.store_row & 3) == 0 && (reinterpret_cast<uintptr_t>(L.store) & 15u) == 0;
        for (; c < L.mem_tiles / 2; ++c) {
            // this chunk's input channels: both tiles' loads go out before the barrier and the staging of the next chunk
            f32x4 bm[2][2];
#pragma unroll
            for (int tl = 0; tl < 2; ++tl)
#pragma unroll
                for (int nt = 0; nt < 2; ++nt) {
                    const float4 t4 = *reinterpret_cast<const float4*>(L.src + (size_t)prow[nt] * L.src_row + 16 * (2 * c + tl) + 4 * k);
                    bm[tl][nt] = (f32x4){t4.x, t4.y, t4.z, t4.w};
                }
            lds_copy_wait();      // this wavefront's pieces of chunk c have landed ...
            __syncthreads();      // ... and everybody's; the other buffer is free
            if (c + 1 < n_chunks) stage(c + 1, buf ^ 1);
#pragma unroll
            for (int tl = 0; tl < 2; ++tl) {
                if (full) mlp_tile<HT, true>(acc, &s_w[buf][tl * 64 + lane], L.out_tiles, bm[tl][0], bm[tl][1]);
                else mlp_tile<HT, false>(acc, &s_w[buf][tl * 64 + lane], L.out_tiles, bm[tl][0], bm[tl][1]);
            }
            buf ^= 1;
        }
        // ---- input channels that are the register state (compile-time register indices) ----
#pragma unroll
        for (int cr = 0; cr < HT / 2; ++cr) {
            if (cr < L.reg_tiles / 2) {
                lds_copy_wait();
                __syncthreads();
                if (c + 1 < n_chunks) stage(c + 1, buf ^ 1);
#pragma unroll
                for (int tl = 0; tl < 2; ++tl) {
                    const int t = 2 * cr + tl;
                    if (full) mlp_tile<HT, true>(acc, &s_w[buf][tl * 64 + lane], L.out_tiles, prev[0][t], prev[1][t]);
                    else mlp_tile<HT, false>(acc, &s_w[buf][tl * 64 + lane], L.out_tiles, prev[0][t], prev[1][t]);
                }
                buf ^= 1;
                ++c;
            }
        }
        // ---- epilogue: channel 16 mt + 4 k + i of point (nt, n) ----
        const bool plain = full && p0 + 32 <= n_points && !L.keep_state &&
                           (L.epilogue == SR_MLP_LEAKY || (L.epilogue == SR_MLP_MASK && L.mask_bits)) &&
                           (!L.store || (store_vec && L.store_channels == 16 * HT && !L.store_accumulate));   // wave-uniform
        if (plain) { mlp_epilogue_plain<HT>(acc, prev, L, slope, mbits, p0, n, k); continue; }
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
__global__ void __launch_bounds__(kBlock) __attribute__((amdgpu_waves_per_eu(HT == 8 ? SR_MLP_WAVES8 : 3, HT == 8 ? SR_MLP_WAVES8 : 3))) k_mlp_chain(const MlpK net, int n_points, float slope) {
    __shared__ float4 s_w[2][HT * 2 * 64];
    mlp_chain_body<HT>(net.op, net.n_ops, s_w, n_points, slope);
}

// The networks of one group in one grid: workgroup (x, y) carries points 128 x .. 128 x + 127 through net y's ops
// (op[first[y]] .. op[first[y + 1]] - 1).  The nets differ in depth, skips and output tiles; a workgroup belongs to one net, so
// its barriers stay uniform, and the workgroups of net y + 1 fill the tail of net y's last round of resident workgroups.
struct MlpGroupK { int n_nets; int first[SR_MLP_GROUP_MAX_NETS + 1]; SrMlpOp op[SR_MLP_GROUP_MAX_OPS]; };
static_assert(sizeof(MlpGroupK) + 2 * sizeof(int) < 4096, "the op table of a group travels as a kernel argument: 4 KB");

template <int HT>
__global__ void __launch_bounds__(kBlock) __attribute__((amdgpu_waves_per_eu(HT == 8 ? SR_MLP_WAVES8 : 3, HT == 8 ? SR_MLP_WAVES8 : 3))) k_mlp_chain_group(const MlpGroupK grp, int n_points, float slope) {
    __shared__ float4 s_w[2][HT * 2 * 64];
    const int f0 = grp.first[blockIdx.y];
    mlp_chain_body<HT>(grp.op + f0, grp.first[blockIdx.y + 1] - f0, s_w, n_points, slope);
}

// ---- the same chains with bf16 matrix operands (opt-in: sr_mlp_chain_bf16) ------------------------------------------------
// acc = bias + bf(W) . bf(x): both MFMA operands are rounded to bfloat16 (round to nearest even, v_cvt_pk_bf16_f32), products and
// accumulation stay fp32 inside `v_mfma_f32_16x16x32_bf16`, and everything outside the MFMA is the fp32 kernel's: the bias as
// the accumulator's initial value, the running state in fp32 registers (rounded only where it becomes an operand, once per op and
// state tile), the epilogues, the sign bits and every store.  The fp32 MFMA issues at the vector rate on gfx950, 1/16 of the bf16
// rate: a 32-channel chunk at HT = 8 is 16 MFMAs here instead of 128.
//
// Operand map of the 16x16x32 MFMA: lane (k = lane >> 4, m or n = lane & 15) holds K indices 8 k + j, j = 0..7, of row m of A and
// of column n of B; the accumulator is the fp32 one (register i of lane (k, n) = row 4 k + i of column n).  A and B share the
// lane -> K map, so WHICH channel sits at K index 8 k + j is free as long as packer and operand agree: element j stands for
// channel 32 c + 16 (j >> 2) + 4 k + (j & 3) of chunk c, which makes the B operand of lane (k, n) the eight values
// [prev[nt][2 c][0..3], prev[nt][2 c + 1][0..3]] it already holds -- the accumulator of one layer is still the operand of the next.
// Packed matrix (k_mlp_pack_bf16), MT output tiles:
//   bf16 index (((c * MT + mt) * 64 + lane) * 8 + j)  =  A[16 mt + (lane & 15)][32 c + 16 (j >> 2) + 4 (lane >> 4) + (j & 3)]
// one ds_read_b128 per lane, output tile and chunk; a chunk is MT KiB in LDS.
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
#ifndef SR_MLP_BF16_WAVES8
#define SR_MLP_BF16_WAVES8 2     // wavefronts per SIMD the 128-wide bf16 kernel is compiled for
#endif

__device__ __forceinline__ bf16x8 mlp_operand_bf16(const f32x4 lo, const f32x4 hi) {
    return (bf16x8){(__bf16)lo[0], (__bf16)lo[1], (__bf16)lo[2], (__bf16)lo[3], (__bf16)hi[0], (__bf16)hi[1], (__bf16)hi[2], (__bf16)hi[3]};
}

// One 32-channel chunk against all output tiles: one MFMA per output tile and point tile.  `w` points at this lane's 16 bytes of
// output tile 0 (consecutive output tiles are 64 x 16 bytes apart).  The 2 HT accumulators are independent: no dependent chains.
template <int HT, bool FULL>
__device__ __forceinline__ void mlp_chunk_bf16(f32x4 (&acc)[2][HT], const bf16x8* w, int out_tiles, const bf16x8 b0, const bf16x8 b1) {
#pragma unroll
    for (int mt = 0; mt < HT; ++mt) {
        if (FULL || mt < out_tiles) {
            const bf16x8 a = w[mt * 64];
            acc[0][mt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, b0, acc[0][mt], 0, 0, 0);
            acc[1][mt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, b1, acc[1][mt], 0, 0, 0);
        }
    }
}

// body of k_mlp_chain_bf16 and k_mlp_chain_group_bf16 (see mlp_chain_body); s_w: two chunks of a packed matrix, [mt][lane]
template <int HT>
__device__ __forceinline__ void mlp_chain_body_bf16(const SrMlpOp* ops, const int n_ops, bf16x8 (&s_w)[2][HT * 64], int n_points, float slope) {
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
        const int chunk_v = L.out_tiles * 64;                  // 16-byte vectors per chunk: mt x 64
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
        // ---- input channels that come from memory: rounded as they are loaded ----
        for (; c < L.mem_tiles / 2; ++c) {
            bf16x8 bm[2];
#pragma unroll
            for (int nt = 0; nt < 2; ++nt) {
                const float* row = L.src + (size_t)prow[nt] * L.src_row + 32 * c + 4 * k;
                const float4 lo = *reinterpret_cast<const float4*>(row), hi = *reinterpret_cast<const float4*>(row + 16);
                bm[nt] = mlp_operand_bf16((f32x4){lo.x, lo.y, lo.z, lo.w}, (f32x4){hi.x, hi.y, hi.z, hi.w});
            }
            lds_copy_wait();      // this wavefront's pieces of chunk c have landed ...
            __syncthreads();      // ... and everybody's; the other buffer is free
            if (c + 1 < n_chunks) stage(c + 1, buf ^ 1);
            if (full) mlp_chunk_bf16<HT, true>(acc, &s_w[buf][lane], L.out_tiles, bm[0], bm[1]);
            else mlp_chunk_bf16<HT, false>(acc, &s_w[buf][lane], L.out_tiles, bm[0], bm[1]);
            buf ^= 1;
        }
        // ---- input channels that are the register state: each state tile is rounded once per op, here ----
#pragma unroll
        for (int cr = 0; cr < HT / 2; ++cr) {
            if (cr < L.reg_tiles / 2) {
                const bf16x8 b0 = mlp_operand_bf16(prev[0][2 * cr], prev[0][2 * cr + 1]), b1 = mlp_operand_bf16(prev[1][2 * cr], prev[1][2 * cr + 1]);
                lds_copy_wait();
                __syncthreads();
                if (c + 1 < n_chunks) stage(c + 1, buf ^ 1);
                if (full) mlp_chunk_bf16<HT, true>(acc, &s_w[buf][lane], L.out_tiles, b0, b1);
                else mlp_chunk_bf16<HT, false>(acc, &s_w[buf][lane], L.out_tiles, b0, b1);
                buf ^= 1;
                ++c;
            }
        }
        // ---- epilogue: the fp32 kernel's, on unrounded fp32 accumulators ----
        const bool plain = full && p0 + 32 <= n_points && !L.keep_state &&
                           (L.epilogue == SR_MLP_LEAKY || (L.epilogue == SR_MLP_MASK && L.mask_bits)) &&
                           (!L.store || (store_vec && L.store_channels == 16 * HT && !L.store_accumulate));   // wave-uniform
        if (plain) { mlp_epilogue_plain<HT>(acc, prev, L, slope, mbits, p0, n, k); continue; }
        // (k_mlp_chain's generic epilogue, repeated: as a function shared by the two kernels it costs ~600 spilled registers at HT = 4)
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
__global__ void __launch_bounds__(kBlock) __attribute__((amdgpu_waves_per_eu(HT == 8 ? SR_MLP_BF16_WAVES8 : 3, HT == 8 ? SR_MLP_BF16_WAVES8 : 3))) k_mlp_chain_bf16(const MlpK net, int n_points, float slope) {
    __shared__ bf16x8 s_w[2][HT * 64];
    mlp_chain_body_bf16<HT>(net.op, net.n_ops, s_w, n_points, slope);
}

template <int HT>
__global__ void __launch_bounds__(kBlock) __attribute__((amdgpu_waves_per_eu(HT == 8 ? SR_MLP_BF16_WAVES8 : 3, HT == 8 ? SR_MLP_BF16_WAVES8 : 3))) k_mlp_chain_group_bf16(const MlpGroupK grp, int n_points, float slope) {
    __shared__ bf16x8 s_w[2][HT * 64];
    const int f0 = grp.first[blockIdx.y];
    mlp_chain_body_bf16<HT>(grp.op + f0, grp.first[blockIdx.y + 1] - f0, s_w, n_points, slope);
}

struct MlpPackK { SrMlpPackJob job[SR_MLP_MAX_PACK_JOBS]; };

// Element (r, cp) of a job's padded matrix: padded column cp is a memory column, then a column of the register state; the padding
// of either and the rows past n_rows are zero.
__device__ __forceinline__ float mlp_pack_source(const SrMlpPackJob& J, int r, int cp) {
    int col = -1;
    if (cp < J.mem_pad) { if (cp < J.n_mem) col = J.mem_col0 + cp; }
    else if (cp - J.mem_pad < J.n_reg) col = J.reg_col0 + cp - J.mem_pad;
    if (r >= J.n_rows || col < 0) return 0.0f;
    return J.transposed ? J.w[(size_t)col * J.ld + J.row0 + r] : J.w[(size_t)(J.row0 + r) * J.ld + col];
}

// the bias of a job, padded with zeros to its output tiles: fp32 in every precision
__device__ __forceinline__ void mlp_pack_bias(const SrMlpPackJob& J) {
    if (J.bias_dst && blockIdx.x == 0)
        for (int j = (int)threadIdx.x; j < 16 * J.out_tiles; j += kBlock) J.bias_dst[j] = j < J.n_bias ? J.bias_src[j] : 0.0f;
}

// One packed float per thread step: thread index = the destination index, decoded to (c, mt, tl, lane, i) -> (row, column).
__global__ void __launch_bounds__(kBlock) k_mlp_pack(const MlpPackK jobs) {
    const SrMlpPackJob J = jobs.job[blockIdx.y];
    const int kt = (J.mem_pad + J.reg_width) / 16;
    const int total = 16 * J.out_tiles * 16 * kt;
    for (int d = blockIdx.x * kBlock + (int)threadIdx.x; d < total; d += gridDim.x * kBlock) {
        const int i = d & 3, lane = (d >> 2) & 63, tl = (d >> 8) & 1;
        const int rest = d >> 9;                       // c * MT + mt
        const int mt = rest % J.out_tiles, c = rest / J.out_tiles;
        J.dst[d] = mlp_pack_source(J, 16 * mt + (lane & 15), 16 * (2 * c + tl) + 4 * (lane >> 4) + i);
    }
    mlp_pack_bias(J);
}

// The matrix of a job as bf16 in the layout the bf16 chunks read (above): two adjacent packed elements (j, j + 1 = two adjacent
// columns of the same 4-column group) per thread step, one 4-byte store.  PARTS = 1: the values rounded to bf16 (k_mlp_pack_bf16);
// PARTS = 2: per chunk the block of the rounded values and then the block of their remainders (k_mlp_pack_bf16x3, mlp_bf16x3.h).
template <int PARTS>
__device__ __forceinline__ void mlp_pack_bf16_parts(const MlpPackK& jobs) {
    const SrMlpPackJob J = jobs.job[blockIdx.y];
    const int pairs = PARTS * 8 * J.out_tiles * (J.mem_pad + J.reg_width);
    uint32_t* dst = reinterpret_cast<uint32_t*>(J.dst);
    for (int d = blockIdx.x * kBlock + (int)threadIdx.x; d < pairs; d += gridDim.x * kBlock) {
        const int j = 2 * (d & 3), lane = (d >> 2) & 63;
        const int rest = d >> 8;                       // (PARTS c + part) * MT + mt
        const int mt = rest % J.out_tiles, cpart = rest / J.out_tiles;
        const int part = PARTS == 2 ? cpart & 1 : 0, c = PARTS == 2 ? cpart >> 1 : cpart;
        const int r = 16 * mt + (lane & 15);
        const int cp = 32 * c + 16 * (j >> 2) + 4 * (lane >> 4) + (j & 3);
        __bf16 p[2];
#pragma unroll
        for (int e = 0; e < 2; ++e) {
            const float v = mlp_pack_source(J, r, cp + e);
            const __bf16 h = (__bf16)v;
            p[e] = part ? (__bf16)(v - (float)h) : h;
        }
        dst[d] = (uint32_t)__builtin_bit_cast(unsigned short, p[0]) | ((uint32_t)__builtin_bit_cast(unsigned short, p[1]) << 16);
    }
    mlp_pack_bias(J);
}

__global__ void __launch_bounds__(kBlock) k_mlp_pack_bf16(const MlpPackK jobs) { mlp_pack_bf16_parts<1>(jobs); }

// the split-bf16 ("bf16x3") chains and their packer: k_mlp_chain_bf16x3, k_mlp_chain_group_bf16x3, k_mlp_pack_bf16x3
#include "mlp_bf16x3.h"

// ---- weight gradients: dW[m][c] = sum over points of dZ[p][m] X[p][c], db[m] = sum over points of dZ[p][m] -------------------------
// The contraction runs over the POINTS (10^5), the result is tiny (128 x 222): library GEMMs serialise it (0.27 ms for one
// 128 x 128 x 100k product on MI355X, 12 TFLOP/s; eight of them were 2.7 of the 3.9 ms of a GeneralMLP training step).  Here
// the points are cut into slabs, one workgroup column per slab; a wavefront owns one 64 x 64 block of one layer's dW and walks its
// slab four points per MFMA step.  Operands come straight from memory with NO transpose: lane (kk, n) loads float4 = channels
// 4n..4n+3 of point s + kk from dZ and from X (256 contiguous bytes per point row), and register i of the dZ load with
// register j of the X load feed tile (i, j), whose MFMA row m' stands for dZ channel 4 m' + i and column n' for X channel
// 4 n' + j: 2 loads per 16 MFMAs.  Partial blocks go to a workspace and a second kernel adds them over the slabs in a fixed
// order (deterministic, no float atomics).
constexpr int kGradMaxSlabs = 256;
struct GradTask { unsigned char job, bm, bk, bias; };
struct MlpGradK {
    int n_tasks, n_points, slab, n_slabs;
    float* part;          // [task][slab][64][64]
    float* bias_part;     // [task][slab][64]
    SrMlpGradJob job[SR_MLP_MAX_GRAD_JOBS];
    GradTask task[SR_MLP_MAX_GRAD_TASKS];
};

__global__ void __launch_bounds__(kBlock) k_mlp_weight_grad(const MlpGradK P) {
    const int t = __builtin_amdgcn_readfirstlane(blockIdx.y * 4 + wave_id());   // wave-uniform: the job's fields stay in SGPRs
    if (t >= P.n_tasks) return;                       // no barriers below
    const GradTask T = P.task[t];
    const SrMlpGradJob J = P.job[T.job];
    const int lane = lane_id(), kk = lane >> 4, n = lane & 15;
    const int s_begin = blockIdx.x * P.slab, s_end = min(P.n_points, s_begin + P.slab);
    // Buffer loads: a byte offset beyond the buffer reads as 0, so rows past the slab's end and channel groups past the row
    // width need no branch (the compiler turns "load, then zero if invalid" back into a branch around the load, which
    // serialises the four steps kept in flight below).
    const bool zok = 64 * T.bm + 4 * n + 3 < J.dz_row, xok = 64 * T.bk + 4 * n + 3 < J.x_row;
    const unsigned zcol = 4u * (64 * T.bm + 4 * n), xcol = 4u * (64 * T.bk + 4 * n);
    const unsigned zbytes = 4u * (unsigned)J.dz_row, xbytes = 4u * (unsigned)J.x_row;
    const __amdgpu_buffer_rsrc_t zsrc = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(J.dz), 0, (int)(zbytes * (unsigned)P.n_points), 0x00020000);
    const __amdgpu_buffer_rsrc_t xsrc = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(J.x), 0, (int)(xbytes * (unsigned)P.n_points), 0x00020000);
    auto ldz = [&](int p) -> float4 {
        const u32x4 v = __builtin_amdgcn_raw_buffer_load_b128(zsrc, (zok && p < s_end) ? (unsigned)p * zbytes + zcol : 0xfffffff0u, 0, 0);
        return make_float4(__uint_as_float(v.x), __uint_as_float(v.y), __uint_as_float(v.z), __uint_as_float(v.w));
    };
    auto ldx = [&](int p) -> float4 {
        const u32x4 v = __builtin_amdgcn_raw_buffer_load_b128(xsrc, (xok && p < s_end) ? (unsigned)p * xbytes + xcol : 0xfffffff0u, 0, 0);
        return make_float4(__uint_as_float(v.x), __uint_as_float(v.y), __uint_as_float(v.z), __uint_as_float(v.w));
    };
    f32x4 acc[4][4];
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[i][j] = (f32x4){0.f, 0.f, 0.f, 0.f};
    float4 colsum = make_float4(0.f, 0.f, 0.f, 0.f);
#define SR_GRAD_ROW(i, ai, b)                                                                \
        acc[i][0] = __builtin_amdgcn_mfma_f32_16x16x4f32(ai, b.x, acc[i][0], 0, 0, 0);        \
        acc[i][1] = __builtin_amdgcn_mfma_f32_16x16x4f32(ai, b.y, acc[i][1], 0, 0, 0);        \
        acc[i][2] = __builtin_amdgcn_mfma_f32_16x16x4f32(ai, b.z, acc[i][2], 0, 0, 0);        \
        acc[i][3] = __builtin_amdgcn_mfma_f32_16x16x4f32(ai, b.w, acc[i][3], 0, 0, 0);
#define SR_GRAD_STEP(a, b, next)                                                              \
        colsum.x += a.x; colsum.y += a.y; colsum.z += a.z; colsum.w += a.w;                    \
        SR_GRAD_ROW(0, a.x, b) SR_GRAD_ROW(1, a.y, b) SR_GRAD_ROW(2, a.z, b) SR_GRAD_ROW(3, a.w, b) \
        a = ldz(next); b = ldx(next);
    float4 a0 = ldz(s_begin + kk), b0 = ldx(s_begin + kk);
    float4 a1 = ldz(s_begin + 4 + kk), b1 = ldx(s_begin + 4 + kk);
    float4 a2 = ldz(s_begin + 8 + kk), b2 = ldx(s_begin + 8 + kk);
    float4 a3 = ldz(s_begin + 12 + kk), b3 = ldx(s_begin + 12 + kk);
    for (int s = s_begin; s < s_end; s += 16) {       // four steps of four points; steps past the slab's end add zeros
        SR_GRAD_STEP(a0, b0, s + 16 + kk)
        SR_GRAD_STEP(a1, b1, s + 20 + kk)
        SR_GRAD_STEP(a2, b2, s + 24 + kk)
        SR_GRAD_STEP(a3, b3, s + 28 + kk)
    }
#undef SR_GRAD_STEP
#undef SR_GRAD_ROW
    // lane (kk, n), tile (i, j), register r  =  block row 16 kk + 4 r + i, block column 4 n + j
    float* out = P.part + ((size_t)t * P.n_slabs + blockIdx.x) * 4096;
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int r = 0; r < 4; ++r)
            *reinterpret_cast<float4*>(out + (16 * kk + 4 * r + i) * 64 + 4 * n) = make_float4(acc[i][0][r], acc[i][1][r], acc[i][2][r], acc[i][3][r]);
    if (T.bias) {                                     // column sums of dZ: add the four point phases kk
        colsum.x += __shfl_xor(colsum.x, 16); colsum.y += __shfl_xor(colsum.y, 16); colsum.z += __shfl_xor(colsum.z, 16); colsum.w += __shfl_xor(colsum.w, 16);
        colsum.x += __shfl_xor(colsum.x, 32); colsum.y += __shfl_xor(colsum.y, 32); colsum.z += __shfl_xor(colsum.z, 32); colsum.w += __shfl_xor(colsum.w, 32);
        if (kk == 0) *reinterpret_cast<float4*>(P.bias_part + ((size_t)t * P.n_slabs + blockIdx.x) * 64 + 4 * n) = colsum;
    }
}

// Adds the partial blocks over the slabs in a FIXED order: a workgroup owns 64 consecutive entries of a task's block (or its
// 64 bias entries); wavefront q adds slabs q, q + 4, q + 8, ... (eight loads in flight), the four partial sums are added in
// order q = 0..3.  (One thread per entry walking all 256 slabs kept a 48 x 48 gradient waiting 65 us on 17 workgroups.)
__global__ void __launch_bounds__(kBlock) k_mlp_weight_grad_reduce(const MlpGradK P) {
    __shared__ float s_part[4][64];
    const int t = blockIdx.y;
    const GradTask T = P.task[t];
    const SrMlpGradJob J = P.job[T.job];
    const int q = wave_id(), e = blockIdx.x * 64 + lane_id();
    const bool bias_row = e >= 4096;
    if (bias_row && !T.bias) return;                  // block-uniform
    const float* src = bias_row ? P.bias_part + (size_t)t * P.n_slabs * 64 + (e - 4096) : P.part + (size_t)t * P.n_slabs * 4096 + e;
    const size_t stride = bias_row ? 64 : 4096;
    float sum = 0.0f;
    int sl = q;
    for (; sl + 28 < P.n_slabs; sl += 32) {
        float v[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) v[u] = src[(size_t)(sl + 4 * u) * stride];
#pragma unroll
        for (int u = 0; u < 8; ++u) sum += v[u];
    }
    for (; sl < P.n_slabs; sl += 4) sum += src[(size_t)sl * stride];
    s_part[q][lane_id()] = sum;
    __syncthreads();
    if (q != 0) return;
    sum = ((s_part[0][lane_id()] + s_part[1][lane_id()]) + s_part[2][lane_id()]) + s_part[3][lane_id()];
    if (bias_row) {
        const int m = 64 * T.bm + (e - 4096);
        if (m < J.m) J.db[m] = sum;
    } else {
        const int m = 64 * T.bm + (e >> 6), c = 64 * T.bk + (e & 63);
        if (m < J.m && c < J.k) J.dw[(size_t)m * J.dw_row + J.dw_col0 + c] = sum;
    }
}

// Fills the task table; returns the number of tasks or -1.
static int grad_tasks(int n_points, int n_jobs, const SrMlpGradJob* jobs, MlpGradK* k) {
    if (n_jobs < 1 || n_jobs > SR_MLP_MAX_GRAD_JOBS) return -1;
    int nt = 0;
    for (int j = 0; j < n_jobs; ++j) {
        const SrMlpGradJob& s = jobs[j];
        if (!s.dz || !s.x || !s.dw || s.m < 1 || s.k < 1 || s.m > s.dz_row || s.k > s.x_row || (s.dz_row & 3) || (s.x_row & 3) ||
            (reinterpret_cast<uintptr_t>(s.dz) & 15u) || (reinterpret_cast<uintptr_t>(s.x) & 15u) || s.dw_col0 < 0 || s.dw_col0 + s.k > s.dw_row ||
            s.m > 64 * 255 || s.k > 64 * 255) return -1;
        if (n_points > 0 && ((size_t)n_points * s.dz_row * 4 >= (1ull << 31) || (size_t)n_points * s.x_row * 4 >= (1ull << 31))) return -1;   // 32-bit buffer offsets
        if (k) k->job[j] = s;
        for (int bm = 0; bm < (s.m + 63) / 64; ++bm)
            for (int bk = 0; bk < (s.k + 63) / 64; ++bk) {
                if (nt >= SR_MLP_MAX_GRAD_TASKS) return -1;
                if (k) k->task[nt] = GradTask{(unsigned char)j, (unsigned char)bm, (unsigned char)bk, (unsigned char)(s.db && bk == 0)};
                ++nt;
            }
    }
    return nt;
}

static void grad_slabs(int n_points, int* slab, int* n_slabs) {
    const int per = (n_points + kGradMaxSlabs - 1) / kGradMaxSlabs;
    *slab = max(64, (per + 3) / 4 * 4);
    *n_slabs = max(1, (n_points + *slab - 1) / *slab);
}

size_t mlp_weight_grad_workspace(int n_points, int n_jobs, const SrMlpGradJob* jobs) {
    const int nt = grad_tasks(n_points, n_jobs, jobs, nullptr);
    if (nt < 0 || n_points < 0) return 0;
    int slab, n_slabs;
    grad_slabs(n_points, &slab, &n_slabs);
    return (size_t)nt * n_slabs * (4096 + 64) * sizeof(float);
}

int launch_mlp_weight_grad(int n_points, int n_jobs, const SrMlpGradJob* jobs, void* workspace, size_t workspace_bytes, hipStream_t st) {
    MlpGradK k;
    const int nt = grad_tasks(n_points, n_jobs, jobs, &k);
    if (nt < 0 || n_points < 1) return 1;
    grad_slabs(n_points, &k.slab, &k.n_slabs);
    if (!workspace || workspace_bytes < (size_t)nt * k.n_slabs * (4096 + 64) * sizeof(float) || (reinterpret_cast<uintptr_t>(workspace) & 15u)) return 1;
    k.n_tasks = nt; k.n_points = n_points;
    k.part = static_cast<float*>(workspace);
    k.bias_part = k.part + (size_t)nt * k.n_slabs * 4096;
    hipLaunchKernelGGL(k_mlp_weight_grad, dim3(k.n_slabs, (nt + 3) / 4), dim3(kBlock), 0, st, k);
    hipLaunchKernelGGL(k_mlp_weight_grad_reduce, dim3((4096 + 64) / 64, nt), dim3(kBlock), 0, st, k);
    return 0;
}

// chain precision of a launch: which packer / chain kernel runs (validation is the same for all three)
enum MlpMode { kMlpFp32 = 0, kMlpBf16 = 1, kMlpBf16x3 = 2, kMlpModes };      // kMlpModes: the size of the kernel tables below

int launch_mlp_pack(int n_jobs, const SrMlpPackJob* jobs, MlpMode mode, hipStream_t st) {
    if (n_jobs < 0 || n_jobs > SR_MLP_MAX_PACK_JOBS) return 1;
    if (n_jobs == 0) return 0;
    MlpPackK k;
    int most = 0;
    for (int j = 0; j < n_jobs; ++j) {
        const SrMlpPackJob& s = jobs[j];
        if (!s.w || !s.dst || s.out_tiles < 1 || s.ld < 1 || s.row0 < 0 || s.n_rows < 0 || s.n_rows > 16 * s.out_tiles ||
            s.n_mem < 0 || s.n_mem > s.mem_pad || s.n_reg < 0 || s.n_reg > s.reg_width || (s.mem_pad & 31) || (s.reg_width & 15) ||
            (((s.mem_pad + s.reg_width) / 16) & 1) || s.mem_pad + s.reg_width < 32 || (reinterpret_cast<uintptr_t>(s.dst) & 15u) ||
            (s.bias_dst && (!s.bias_src || s.n_bias < 0 || s.n_bias > 16 * s.out_tiles))) return 1;
        k.job[j] = s;
        most = max(most, 16 * s.out_tiles * (s.mem_pad + s.reg_width));
    }
    static void (*const kernel[])(const MlpPackK) = {k_mlp_pack, k_mlp_pack_bf16, k_mlp_pack_bf16x3};
    static_assert(sizeof(kernel) / sizeof(kernel[0]) == kMlpModes, "one packer per precision");
    const int steps = mode == kMlpBf16 ? most / 2 : most;     // thread steps, two elements each for the bf16 kinds: bf16 most / 2 pairs, bf16x3 two parts of most / 2 pairs
    hipLaunchKernelGGL(kernel[mode], dim3(min(64, (steps + kBlock * 4 - 1) / (kBlock * 4)), n_jobs), dim3(kBlock), 0, st, k);
    return 0;
}

// what sr_mlp_chain requires of one op (shared by the single-net and the group launch)
static bool mlp_op_ok(const SrMlpOp& s, int hidden_tiles) {
    if (s.out_tiles < 1 || s.out_tiles > hidden_tiles || s.mem_tiles < 0 || s.reg_tiles < 0 || s.reg_tiles > hidden_tiles ||
        (s.mem_tiles & 1) || (s.reg_tiles & 1) || s.mem_tiles + s.reg_tiles < 2 || !s.w_packed ||
        (reinterpret_cast<uintptr_t>(s.w_packed) & 15u) || (reinterpret_cast<uintptr_t>(s.bias) & 15u)) return false;
    if (s.mem_tiles > 0 && (!s.src || s.mem_tiles * 16 > s.src_row || (s.src_row & 3) || (reinterpret_cast<uintptr_t>(s.src) & 15u))) return false;
    if (s.epilogue != SR_MLP_NONE && s.epilogue != SR_MLP_LEAKY && s.epilogue != SR_MLP_MASK) return false;
    if (s.epilogue == SR_MLP_MASK && !s.mask_bits && (!s.mask || s.out_tiles * 16 > s.mask_row || (s.mask_row & 3) || (reinterpret_cast<uintptr_t>(s.mask) & 15u))) return false;
    if ((reinterpret_cast<uintptr_t>(s.mask_bits) & 3u) || (reinterpret_cast<uintptr_t>(s.sign_store) & 3u)) return false;
    if (s.store && (s.store_channels < 1 || s.store_channels > s.store_row || s.store_channels > 16 * s.out_tiles)) return false;
    return true;
}

int launch_mlp_chain(int n_points, int hidden_tiles, int n_ops, const SrMlpOp* ops, float slope, MlpMode mode, hipStream_t st) {
    if (n_ops < 1 || n_ops > kMlpMaxOps) return 1;
    MlpK net;
    net.n_ops = n_ops;
    for (int l = 0; l < n_ops; ++l) {
        if (!mlp_op_ok(ops[l], hidden_tiles)) return 1;
        net.op[l] = ops[l];
    }
    if (n_points <= 0) return 0;
    if (hidden_tiles != 4 && hidden_tiles != 8) return 1;
    static void (*const kernel[kMlpModes][2])(const MlpK, int, float) = {
        {k_mlp_chain<4>, k_mlp_chain<8>}, {k_mlp_chain_bf16<4>, k_mlp_chain_bf16<8>}, {k_mlp_chain_bf16x3<4>, k_mlp_chain_bf16x3<8>}};
    hipLaunchKernelGGL(kernel[mode][hidden_tiles == 8], dim3((n_points + 127) / 128), dim3(kBlock), 0, st, net, n_points, slope);
    return 0;
}

// -> nullptr, or why the group is refused (nothing is launched then)
const char* launch_mlp_chain_group(int n_points, int hidden_tiles, int n_nets, const SrMlpNet* nets, float slope, MlpMode mode, hipStream_t st) {
    if (n_points < 0) return "n_points must not be negative";
    if (hidden_tiles != 4 && hidden_tiles != 8) return "hidden_tiles must be 4 or 8, the same for all nets of a group";
    if (n_nets < 0 || n_nets > SR_MLP_GROUP_MAX_NETS) return "between 0 and SR_MLP_GROUP_MAX_NETS nets per group";
    if (n_nets > 0 && !nets) return "null net table";
    MlpGroupK grp;
    grp.n_nets = n_nets;
    int total = 0;
    for (int y = 0; y < n_nets; ++y) {
        if (!nets[y].ops || nets[y].n_ops < 1) return "every net needs at least one op";
        if (nets[y].n_ops > SR_MLP_GROUP_MAX_OPS - total) return "more than SR_MLP_GROUP_MAX_OPS ops in one group";
        grp.first[y] = total;
        for (int l = 0; l < nets[y].n_ops; ++l) {
            if (!mlp_op_ok(nets[y].ops[l], hidden_tiles))
                return "unsupported op (tile counts within hidden_tiles, even input tile counts, 16-byte aligned rows wide enough for the tiles read)";
            grp.op[total++] = nets[y].ops[l];
        }
    }
    for (int y = n_nets; y <= SR_MLP_GROUP_MAX_NETS; ++y) grp.first[y] = total;
    if (n_points == 0 || n_nets == 0) return nullptr;
    const dim3 grid((n_points + 127) / 128, n_nets);
    static void (*const kernel[kMlpModes][2])(const MlpGroupK, int, float) = {
        {k_mlp_chain_group<4>, k_mlp_chain_group<8>}, {k_mlp_chain_group_bf16<4>, k_mlp_chain_group_bf16<8>},
        {k_mlp_chain_group_bf16x3<4>, k_mlp_chain_group_bf16x3<8>}};
    hipLaunchKernelGGL(kernel[mode][hidden_tiles == 8], grid, dim3(kBlock), 0, st, grp, n_points, slope);
    return nullptr;
}

}  // namespace

}  // namespace sr

// ------------------------------------------------------------------------------------------------------------------------
// ResField weights of ONE frame for all layers of a network (reference utils/resfields.py:185,229,294-300,378-405 in the
// configuration GeneralMLP builds: compression 'vm', mode 'lookup', fuse 'add'):
//     W_eff[j] = W[j] + sum_k weights_t[frame][k] * matrix_t[k][j],      j < out * in
// The reference materialises the [capacity, out * in] matrix of EVERY frame per call and indexes it; composing only the
// current frame with PyTorch ops costs an index, a [1 x rank] x [rank x out in] product and an add per layer, and twice that
// backward -- about 240 small launches per step of the six-network deform field.  Here: one launch per network forward,
// two backward (d matrix_t = coeff (x) dW_eff written in place of an outer-product kernel per layer; d weights_t[frame] =
// matrix_t . dW_eff by a fixed-order two-stage reduction; d W = dW_eff needs no kernel at all).  Memory-bound: matrix_t is
// rank x out x in floats (4.5 MB for a 128 x 222 layer at the reference's rank 40).
// ------------------------------------------------------------------------------------------------------------------------
namespace sr {

struct ResFieldK { SrResFieldJob job[SR_RESFIELD_MAX_JOBS]; const long long* frame; float* part; int blocks_per_job; };

constexpr int kRfPerBlock = kBlock * 4;   // elements of W per workgroup

// frame index as the reference's `mat[frame_id]` reads it: indices in [-capacity, 0) wrap (Python indexing; general_mlp.py's
// host-side check wraps the same way), everything else outside [0, capacity) is an error
__device__ __forceinline__ long long resfield_frame(long long f, int capacity) {
    return (f < 0 && f >= -(long long)capacity) ? f + (long long)capacity : f;
}

__global__ void __launch_bounds__(kBlock) k_resfield_compose(const ResFieldK P) {
    const SrResFieldJob J = P.job[blockIdx.y];
    const int j4 = blockIdx.x * kBlock + (int)threadIdx.x;
    if (4 * j4 >= J.count) return;
    const long long f = resfield_frame(*P.frame, J.capacity);
    if (f < 0 || f >= (long long)J.capacity) {
        // the reference's `mat[frame_id]` raises IndexError here; a kernel cannot, and reading weights_t out of bounds would
        // compose garbage silently: poison the weights instead, so that the network's outputs are NaN from this step on
        const float nan = __builtin_nanf("");
        reinterpret_cast<float4*>(J.out)[j4] = make_float4(nan, nan, nan, nan);
        return;
    }
    const float* coeff = J.weights_t + (size_t)f * J.rank;
    const int q = J.count >> 2;
    const float4* M = reinterpret_cast<const float4*>(J.matrix_t) + j4;
    float4 acc = reinterpret_cast<const float4*>(J.w)[j4];
    int k = 0;
    for (; k + 4 <= J.rank; k += 4) {      // four independent loads in flight
        const float4 m0 = M[(size_t)k * q], m1 = M[(size_t)(k + 1) * q], m2 = M[(size_t)(k + 2) * q], m3 = M[(size_t)(k + 3) * q];
        const float c0 = coeff[k], c1 = coeff[k + 1], c2 = coeff[k + 2], c3 = coeff[k + 3];
        acc.x += c0 * m0.x + c1 * m1.x + c2 * m2.x + c3 * m3.x; acc.y += c0 * m0.y + c1 * m1.y + c2 * m2.y + c3 * m3.y;
        acc.z += c0 * m0.z + c1 * m1.z + c2 * m2.z + c3 * m3.z; acc.w += c0 * m0.w + c1 * m1.w + c2 * m2.w + c3 * m3.w;
    }
    for (; k < J.rank; ++k) {
        const float4 m = M[(size_t)k * q];
        const float c = coeff[k];
        acc.x += c * m.x; acc.y += c * m.y; acc.z += c * m.z; acc.w += c * m.w;
    }
    reinterpret_cast<float4*>(J.out)[j4] = acc;
}

// d_matrix_t[k][j] = coeff[k] * g[j]; partial sums of matrix_t[k][.] . g over this workgroup's 1024 elements -> part
__global__ void __launch_bounds__(kBlock) k_resfield_backward(const ResFieldK P) {
    __shared__ float s_part[4][SR_RESFIELD_MAX_RANK];
    const SrResFieldJob J = P.job[blockIdx.y];
    if (blockIdx.x * kRfPerBlock >= J.count) return;   // whole workgroup
    const int j4 = blockIdx.x * kBlock + (int)threadIdx.x;
    const bool in = 4 * j4 < J.count;
    const long long f_raw = resfield_frame(*P.frame, J.capacity);
    const bool f_ok = f_raw >= 0 && f_raw < (long long)J.capacity;   // out of range: the forward poisoned W_eff with NaN (above);
    const long long f = f_ok ? f_raw : 0;                             //   here: no out-of-bounds read, NaN gradients
    const float* coeff = J.weights_t + (size_t)f * J.rank;
    const int q = J.count >> 2;
    float4 g = in ? reinterpret_cast<const float4*>(J.d_out)[j4] : make_float4(0.f, 0.f, 0.f, 0.f);
    if (!f_ok) g.x = g.y = g.z = g.w = __builtin_nanf("");
    for (int k = 0; k < J.rank; ++k) {
        float dot = 0.0f;
        if (in) {
            const float4 m = reinterpret_cast<const float4*>(J.matrix_t)[(size_t)k * q + j4];
            const float c = coeff[k];
            if (J.d_matrix_t) reinterpret_cast<float4*>(J.d_matrix_t)[(size_t)k * q + j4] = make_float4(c * g.x, c * g.y, c * g.z, c * g.w);
            dot = (m.x * g.x + m.y * g.y) + (m.z * g.z + m.w * g.w);
        }
        const float tot = wave_sum_to_lane63(dot);
        if (lane_id() == 63) s_part[wave_id()][k] = tot;
    }
    __syncthreads();
    if ((int)threadIdx.x < J.rank)
        P.part[((size_t)blockIdx.y * P.blocks_per_job + blockIdx.x) * SR_RESFIELD_MAX_RANK + threadIdx.x] =
            (s_part[0][threadIdx.x] + s_part[1][threadIdx.x]) + (s_part[2][threadIdx.x] + s_part[3][threadIdx.x]);
}

// d_weights_t [capacity, rank]: zero except row `frame` = sum of the workgroups' partial sums in launch order
__global__ void __launch_bounds__(kBlock) k_resfield_finish(const ResFieldK P) {
    const SrResFieldJob J = P.job[blockIdx.x];
    if (!J.d_weights_t) return;
    const long long f = resfield_frame(*P.frame, J.capacity);
    const int nb = (J.count + kRfPerBlock - 1) / kRfPerBlock;
    for (int i = threadIdx.x; i < J.capacity * J.rank; i += kBlock) {
        float v = 0.0f;
        if (i / J.rank == (int)f) {
            const int k = i - (int)f * J.rank;
            for (int b = 0; b < nb; ++b) v += P.part[((size_t)blockIdx.x * P.blocks_per_job + b) * SR_RESFIELD_MAX_RANK + k];
        }
        J.d_weights_t[i] = v;
    }
}

static int resfield_check(int n_jobs, const SrResFieldJob* jobs, bool backward, int* max_count) {
    if (n_jobs < 1 || n_jobs > SR_RESFIELD_MAX_JOBS || !jobs) return 1;
    int mc = 0;
    for (int j = 0; j < n_jobs; ++j) {
        const SrResFieldJob& s = jobs[j];
        if (s.count < 4 || (s.count & 3) || s.rank < 1 || s.rank > SR_RESFIELD_MAX_RANK || s.capacity < 1 || !s.weights_t || !s.matrix_t) return 1;
        if ((reinterpret_cast<uintptr_t>(s.matrix_t) & 15u)) return 1;
        if (!backward && (!s.w || !s.out || ((reinterpret_cast<uintptr_t>(s.w) | reinterpret_cast<uintptr_t>(s.out)) & 15u))) return 1;
        if (backward && (!s.d_out || (reinterpret_cast<uintptr_t>(s.d_out) & 15u) || (reinterpret_cast<uintptr_t>(s.d_matrix_t) & 15u))) return 1;
        mc = s.count > mc ? s.count : mc;
    }
    *max_count = mc;
    return 0;
}

static int launch_resfield_compose(int n_jobs, const SrResFieldJob* jobs, const long long* frame, hipStream_t st) {
    int mc;
    if (!frame || resfield_check(n_jobs, jobs, false, &mc)) return 1;
    ResFieldK P;
    for (int j = 0; j < n_jobs; ++j) P.job[j] = jobs[j];
    P.frame = frame; P.part = nullptr; P.blocks_per_job = (mc + kRfPerBlock - 1) / kRfPerBlock;
    hipLaunchKernelGGL(k_resfield_compose, dim3(P.blocks_per_job, n_jobs), dim3(kBlock), 0, st, P);
    return 0;
}

static size_t resfield_backward_workspace(int n_jobs, const SrResFieldJob* jobs) {
    int mc;
    if (resfield_check(n_jobs, jobs, true, &mc)) return 0;
    return (size_t)n_jobs * ((mc + kRfPerBlock - 1) / kRfPerBlock) * SR_RESFIELD_MAX_RANK * sizeof(float);
}

static int launch_resfield_backward(int n_jobs, const SrResFieldJob* jobs, const long long* frame, void* workspace, size_t workspace_bytes, hipStream_t st) {
    int mc;
    if (!frame || !workspace || resfield_check(n_jobs, jobs, true, &mc)) return 1;
    if (workspace_bytes < resfield_backward_workspace(n_jobs, jobs)) return 1;
    ResFieldK P;
    for (int j = 0; j < n_jobs; ++j) P.job[j] = jobs[j];
    P.frame = frame; P.part = static_cast<float*>(workspace); P.blocks_per_job = (mc + kRfPerBlock - 1) / kRfPerBlock;
    hipLaunchKernelGGL(k_resfield_backward, dim3(P.blocks_per_job, n_jobs), dim3(kBlock), 0, st, P);
    hipLaunchKernelGGL(k_resfield_finish, dim3(n_jobs), dim3(kBlock), 0, st, P);
    return 0;
}

}  // namespace sr

// ------------------------------------------------------------------------------------------------------------------------
// Network input of a GeneralMLP (reference utils/time_utils.py:9-57 `get_embedder` + :178-181): row p of the padded input
// matrix = [ x (3) | sin(2^0 x) (3) | cos(2^0 x) (3) | ... | sin(2^(L-1) x) | cos(2^(L-1) x) | features (F) | time encoding | 0 ... ],
// time encoding = [ t | sin(2^0 t) | cos(2^0 t) | ... | sin(2^(TL-1) t) | cos(2^(TL-1) t) ] when a time per point is given
// (reference utils/time_utils.py:455-456: the time embedding is the tail of the feature vector every network receives).
// One launch instead of the reference's 2 L multiplies, 2 L sin / cos, two concatenations and the padding copy (and as many
// again backward): ~60 small kernels per network and step.
// ------------------------------------------------------------------------------------------------------------------------
namespace sr {

__global__ void __launch_bounds__(kBlock) k_mlp_input_forward(int N, int L, int F, int TL, int row, const float* __restrict__ xyz,
                                                              const float* __restrict__ feat, const float* __restrict__ time,
                                                              float* __restrict__ x0) {
    const int q = row >> 2;
    const long long t = (long long)blockIdx.x * kBlock + threadIdx.x;
    if (t >= (long long)N * q) return;
    const int p = (int)(t / q), c0 = 4 * (int)(t % q);
    const float x[3] = {xyz[3 * (size_t)p], xyz[3 * (size_t)p + 1], xyz[3 * (size_t)p + 2]};
    float v[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int c = c0 + i;
        float o = 0.0f;
        if (c < 3) o = x[c];
        else if (c < 3 + 6 * L) {
            const int k = c - 3, j = k / 6, r = k - 6 * j;
            const float a = x[r < 3 ? r : r - 3] * (float)(1 << j);
            o = r < 3 ? sinf(a) : cosf(a);
        } else if (c < 3 + 6 * L + F) o = feat[(size_t)p * F + (c - 3 - 6 * L)];
        else if (time && c < 3 + 6 * L + F + 1 + 2 * TL) {
            const int m = c - (3 + 6 * L + F);
            const float tv = time[p];
            if (m == 0) o = tv;
            else { const float a = tv * (float)(1 << ((m - 1) >> 1)); o = ((m - 1) & 1) ? cosf(a) : sinf(a); }
        }
        v[i] = o;
    }
    reinterpret_cast<float4*>(x0)[t] = make_float4(v[0], v[1], v[2], v[3]);
}

// d_xyz[p] = g[0:3] + sum_j 2^j (cos(2^j x) g_sin_j - sin(2^j x) g_cos_j);  d_feat[p] = g[3 + 6 L : 3 + 6 L + F]
__global__ void __launch_bounds__(kBlock) k_mlp_input_backward(int N, int L, int F, int row, const float* __restrict__ xyz,
                                                               const float* __restrict__ g, float* __restrict__ d_xyz, float* __restrict__ d_feat) {
    const int per = 1 + (F + 3) / 4;   // thread 0 of a point: the position gradient; the others: 4 feature columns each
    const long long t = (long long)blockIdx.x * kBlock + threadIdx.x;
    if (t >= (long long)N * per) return;
    const int p = (int)(t / per), part = (int)(t % per);
    const float* gp = g + (size_t)p * row;
    if (part == 0) {
        if (!d_xyz) return;
        float d[3] = {gp[0], gp[1], gp[2]};
        const float x[3] = {xyz[3 * (size_t)p], xyz[3 * (size_t)p + 1], xyz[3 * (size_t)p + 2]};
        for (int j = 0; j < L; ++j) {
            const float f = (float)(1 << j);
#pragma unroll
            for (int r = 0; r < 3; ++r) {
                float sn, cs;
                sincosf(x[r] * f, &sn, &cs);
                d[r] += f * (cs * gp[3 + 6 * j + r] - sn * gp[3 + 6 * j + 3 + r]);
            }
        }
        d_xyz[3 * (size_t)p] = d[0]; d_xyz[3 * (size_t)p + 1] = d[1]; d_xyz[3 * (size_t)p + 2] = d[2];
    } else if (d_feat) {
        const int f0 = 4 * (part - 1);
        for (int i = f0; i < min(f0 + 4, F); ++i) d_feat[(size_t)p * F + i] = gp[3 + 6 * L + i];
    }
}

static int launch_mlp_input_forward(int N, int L, int F, int TL, int row, const float* xyz, const float* feat, const float* time, float* x0,
                                    hipStream_t st) {
    if (N < 0 || L < 0 || L > 16 || F < 0 || TL < 0 || TL > 16 || (row & 3) || row < 3 + 6 * L + F + (time ? 1 + 2 * TL : 0) ||
        (F > 0 && !feat) || !xyz || !x0) return 1;
    if (N == 0) return 0;
    const long long threads = (long long)N * (row >> 2);
    hipLaunchKernelGGL(k_mlp_input_forward, dim3((unsigned)((threads + kBlock - 1) / kBlock)), dim3(kBlock), 0, st, N, L, F, TL, row, xyz, feat, time, x0);
    return 0;
}

// Top of a network's backward: G[p][c] = dL/dy[p][c] * leaky'(y[p][c]) for c < out, 0 up to the padded row (the memory input of
// the backward chain's first op and the dZ operand of the last layer's weight gradient).
__global__ void __launch_bounds__(kBlock) k_mlp_top_gradient(int N, int out, int row, const float* __restrict__ y, const float* __restrict__ dy,
                                                             float slope, float* __restrict__ G) {
    const int q = row >> 2;
    const long long t = (long long)blockIdx.x * kBlock + threadIdx.x;
    if (t >= (long long)N * q) return;
    const int p = (int)(t / q), c0 = 4 * (int)(t % q);
    float v[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int c = c0 + i;
        v[i] = c < out ? dy[(size_t)p * out + c] * (y[(size_t)p * out + c] > 0.f ? 1.0f : slope) : 0.0f;
    }
    reinterpret_cast<float4*>(G)[t] = make_float4(v[0], v[1], v[2], v[3]);
}

static int launch_mlp_top_gradient(int N, int out, int row, const float* y, const float* dy, float slope, float* G, hipStream_t st) {
    if (N < 0 || out < 1 || (row & 3) || row < out || !y || !dy || !G) return 1;
    if (N == 0) return 0;
    const long long threads = (long long)N * (row >> 2);
    hipLaunchKernelGGL(k_mlp_top_gradient, dim3((unsigned)((threads + kBlock - 1) / kBlock)), dim3(kBlock), 0, st, N, out, row, y, dy, slope, G);
    return 0;
}

static int launch_mlp_input_backward(int N, int L, int F, int row, const float* xyz, const float* g, float* d_xyz, float* d_feat, hipStream_t st) {
    if (N < 0 || L < 0 || L > 16 || F < 0 || row < 3 + 6 * L + F || !xyz || !g) return 1;
    if (N == 0) return 0;
    const long long threads = (long long)N * (1 + (F + 3) / 4);
    hipLaunchKernelGGL(k_mlp_input_backward, dim3((unsigned)((threads + kBlock - 1) / kBlock)), dim3(kBlock), 0, st, N, L, F, row, xyz, g, d_xyz, d_feat);
    return 0;
}

// ---- the same steps for all heads of a step (sr_mlp_group_*): one launch each, job tables as kernel arguments -----------------------
// The five head networks of a SplatFields step read the same (xyz, features, time): their input matrices, output activations, top
// gradients and the sum of their input gradients are one launch each instead of one (or, for the activations and the sum,
// several PyTorch kernels) per head.  Arithmetic in double, one rounding per stored value; a thread owns what it stores.
struct GroupInK {
    int n_heads, N, F, TL, q_total, l_max;
    int qfirst[SR_MLP_GROUP_MAX_HEADS + 1];      // first float4 column of head h in a point's run of q_total columns
    SrMlpHeadInput head[SR_MLP_GROUP_MAX_HEADS];
    const float* xyz; const float* feat; const float* time;
    float* d_xyz; float* d_feat;
};
struct GroupOutK {
    int n_heads, N, q_total;
    float slope;
    int qfirst[SR_MLP_GROUP_MAX_HEADS + 1];
    SrMlpHeadOutput head[SR_MLP_GROUP_MAX_HEADS];
};

__global__ void __launch_bounds__(kBlock) k_mlp_group_input_forward(const GroupInK P) {
    const long long t = (long long)blockIdx.x * kBlock + threadIdx.x;
    if (t >= (long long)P.N * P.q_total) return;
    const long long p = t / P.q_total;
    const int q = (int)(t - p * P.q_total);
    int h = 0;
    while (h + 1 < P.n_heads && q >= P.qfirst[h + 1]) ++h;
    const SrMlpHeadInput H = P.head[h];
    const int L = H.multires, F = P.F, c0 = 4 * (q - P.qfirst[h]);
    const double x[3] = {(double)P.xyz[3 * (size_t)p], (double)P.xyz[3 * (size_t)p + 1], (double)P.xyz[3 * (size_t)p + 2]};
    // sin / cos of 2^j a come from ONE sincos per axis and j angle doublings in double (s <- 2 s c, c <- 1 - 2 s^2): a doubling
    // costs three operations where a sin or cos of doubles costs a hundred, and its error, about 2^j ulps of double, stays ten
    // binades below float32's rounding for j < 8; from octave 8 on the chain is restarted with a sincos of its own.
    const int t0 = 3 + 6 * L + F;                       // first column of the time encoding
    double sx[3] = {0.0, 0.0, 0.0}, cx[3] = {1.0, 1.0, 1.0}, st = 0.0, ct = 1.0;
    if (c0 < 3 + 6 * L && c0 + 3 >= 3) {
#pragma unroll
        for (int r = 0; r < 3; ++r) sincos(x[r], &sx[r], &cx[r]);
    }
    const double tv = P.time ? (double)P.time[p] : 0.0;
    if (P.time && c0 < t0 + 1 + 2 * P.TL && c0 + 3 > t0) sincos(tv, &st, &ct);
    auto octave = [](double a, double s, double c, int j, double* so, double* co) {
        if (j >= 8) { sincos(a * (double)(1 << (j & ~7)), &s, &c); j &= 7; }
        for (int d = 0; d < j; ++d) { const double s2 = 2.0 * s * c; c = 1.0 - 2.0 * s * s; s = s2; }
        *so = s; *co = c;
    };
    float v[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int c = c0 + i;
        float o = 0.0f;
        if (c < 3) o = (float)x[c];
        else if (c < 3 + 6 * L) {
            const int k = c - 3, j = k / 6, r6 = k - 6 * j, r = r6 < 3 ? r6 : r6 - 3;
            double s, cs;
            octave(r == 0 ? x[0] : r == 1 ? x[1] : x[2], r == 0 ? sx[0] : r == 1 ? sx[1] : sx[2], r == 0 ? cx[0] : r == 1 ? cx[1] : cx[2], j, &s, &cs);
            o = (float)(r6 < 3 ? s : cs);
        } else if (c < t0) o = P.feat[(size_t)p * F + (c - 3 - 6 * L)];
        else if (P.time && c < t0 + 1 + 2 * P.TL) {
            const int m = c - t0;
            if (m == 0) o = (float)tv;
            else { double s, cs; octave(tv, st, ct, (m - 1) >> 1, &s, &cs); o = (float)(((m - 1) & 1) ? cs : s); }
        }
        v[i] = o;
    }
    *reinterpret_cast<float4*>(H.x0 + (size_t)p * H.row + c0) = make_float4(v[0], v[1], v[2], v[3]);
}

// d_xyz[p] = sum over heads h (table order) of g_h[0:3], then for every frequency j the heads' 2^j (cos(2^j x) g_h,sin_j - sin(2^j x) g_h,cos_j)
// in table order (one sincos per frequency and axis for all heads); d_feat[p][i] = sum over heads of g_h[3 + 6 L_h + i]
__global__ void __launch_bounds__(kBlock) k_mlp_group_input_backward(const GroupInK P) {
    const int F = P.F, per = 1 + (F + 3) / 4;
    const long long t = (long long)blockIdx.x * kBlock + threadIdx.x;
    if (t >= (long long)P.N * per) return;
    const long long p = t / per;
    const int part = (int)(t - p * per);
    if (part == 0) {
        if (!P.d_xyz) return;
        double d[3] = {0.0, 0.0, 0.0};
        for (int h = 0; h < P.n_heads; ++h) {
            const float* gp = P.head[h].dL_dx0 + (size_t)p * P.head[h].row;
            d[0] += (double)gp[0]; d[1] += (double)gp[1]; d[2] += (double)gp[2];
        }
        const double x[3] = {(double)P.xyz[3 * (size_t)p], (double)P.xyz[3 * (size_t)p + 1], (double)P.xyz[3 * (size_t)p + 2]};
        double sn3[3], cs3[3];
        for (int j = 0; j < P.l_max; ++j) {
            const double f = (double)(1 << j);
#pragma unroll
            for (int r = 0; r < 3; ++r) {
                // one sincos per axis and eight octaves, angle doublings between (see k_mlp_group_input_forward)
                if ((j & 7) == 0) sincos(x[r] * f, &sn3[r], &cs3[r]);
                else { const double s2 = 2.0 * sn3[r] * cs3[r]; cs3[r] = 1.0 - 2.0 * sn3[r] * sn3[r]; sn3[r] = s2; }
                const double sn = sn3[r], cs = cs3[r];
                for (int h = 0; h < P.n_heads; ++h) {
                    if (j >= P.head[h].multires) continue;
                    const float* gp = P.head[h].dL_dx0 + (size_t)p * P.head[h].row;
                    d[r] += f * (cs * (double)gp[3 + 6 * j + r] - sn * (double)gp[3 + 6 * j + 3 + r]);
                }
            }
        }
        P.d_xyz[3 * (size_t)p] = (float)d[0]; P.d_xyz[3 * (size_t)p + 1] = (float)d[1]; P.d_xyz[3 * (size_t)p + 2] = (float)d[2];
    } else if (P.d_feat) {
        const int f0 = 4 * (part - 1);
        for (int i = f0; i < min(f0 + 4, F); ++i) {
            double s = 0.0;
            for (int h = 0; h < P.n_heads; ++h) s += (double)P.head[h].dL_dx0[(size_t)p * P.head[h].row + 3 + 6 * P.head[h].multires + i];
            P.d_feat[(size_t)p * F + i] = (float)s;
        }
    }
}

// one thread per (point, head): the head's whole output row
__global__ void __launch_bounds__(kBlock) k_mlp_group_output(const GroupOutK P) {
    const long long t = (long long)blockIdx.x * kBlock + threadIdx.x;
    if (t >= (long long)P.N * P.n_heads) return;
    const long long p = t / P.n_heads;
    const SrMlpHeadOutput H = P.head[(int)(t - p * P.n_heads)];
    const float* y = H.y + (size_t)p * H.out_features;
    float* out = H.out + (size_t)p * H.out_features;
    if (H.activation == SR_MLP_OUT_SIGMOID) {
        for (int c = 0; c < H.out_features; ++c) out[c] = (float)(1.0 / (1.0 + exp(-(double)y[c])));
    } else if (H.activation == SR_MLP_OUT_NORMALIZE) {
        double n2 = 0.0;
        for (int c = 0; c < H.out_features; ++c) n2 += (double)y[c] * (double)y[c];
        const double n = fmax(sqrt(n2), 1e-12);
        for (int c = 0; c < H.out_features; ++c) out[c] = (float)((double)y[c] / n);
    } else {
        for (int c = 0; c < H.out_features; ++c) out[c] = y[c];
    }
}

// one thread per (point, float4 of a head's padded row)
__global__ void __launch_bounds__(kBlock) k_mlp_group_top_gradient(const GroupOutK P) {
    const long long t = (long long)blockIdx.x * kBlock + threadIdx.x;
    if (t >= (long long)P.N * P.q_total) return;
    const long long p = t / P.q_total;
    const int q = (int)(t - p * P.q_total);
    int h = 0;
    while (h + 1 < P.n_heads && q >= P.qfirst[h + 1]) ++h;
    const SrMlpHeadOutput H = P.head[h];
    const int out = H.out_features, c0 = 4 * (q - P.qfirst[h]);
    float v[4] = {0.0f, 0.0f, 0.0f, 0.0f};
    if (H.dL_dout && c0 < out) {
        const float* y = H.y + (size_t)p * out;
        const float* d = H.dL_dout + (size_t)p * out;
        double n = 1.0, dot = 0.0;
        bool above = true;
        if (H.activation == SR_MLP_OUT_NORMALIZE) {
            double n2 = 0.0;
            for (int c = 0; c < out; ++c) n2 += (double)y[c] * (double)y[c];
            const double raw = sqrt(n2);
            above = raw > 1e-12;                  // below the clamp the norm is a constant: d (y / eps) = d / eps
            n = fmax(raw, 1e-12);
            for (int c = 0; c < out; ++c) dot += (double)d[c] * ((double)y[c] / n);
        }
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int c = c0 + i;
            if (c >= out) continue;
            const double yc = (double)y[c];
            double g = (double)d[c];
            if (H.activation == SR_MLP_OUT_SIGMOID) { const double s = 1.0 / (1.0 + exp(-yc)); g *= s * (1.0 - s); }
            else if (H.activation == SR_MLP_OUT_NORMALIZE) g = (above ? g - (yc / n) * dot : g) / n;
            v[i] = (float)(g * (y[c] > 0.f ? 1.0 : (double)P.slope));
        }
    }
    *reinterpret_cast<float4*>(H.g + (size_t)p * H.row + c0) = make_float4(v[0], v[1], v[2], v[3]);
}

static const char* group_input_check(int N, int n_heads, const SrMlpHeadInput* heads, int F, int TL, bool time, bool backward) {
    if (N < 0) return "n_points must not be negative";
    if (n_heads < 0 || n_heads > SR_MLP_GROUP_MAX_HEADS) return "between 0 and SR_MLP_GROUP_MAX_HEADS heads";
    if (n_heads > 0 && !heads) return "null head table";
    if (F < 0) return "n_features must not be negative";
    if (TL < 0 || TL > 16) return "time_multires must be in 0..16";
    for (int h = 0; h < n_heads; ++h) {
        const SrMlpHeadInput& s = heads[h];
        if (s.multires < 0 || s.multires > 16) return "multires must be in 0..16";
        if (s.row < 4 || (s.row & 3) || s.row < 3 + 6 * s.multires + F + (time ? 1 + 2 * TL : 0)) return "row must be a multiple of 4 that holds the head's input";
        const float* ptr = backward ? s.dL_dx0 : s.x0;
        if (!ptr) return "null pointer in the head table";
        if (reinterpret_cast<uintptr_t>(ptr) & 15u) return "the heads' matrices must be 16-byte aligned";
    }
    return nullptr;
}

static const char* launch_mlp_group_input_forward(int N, int n_heads, const SrMlpHeadInput* heads, int F, int TL, const float* xyz, const float* feat,
                                                  const float* time, hipStream_t st) {
    if (const char* why = group_input_check(N, n_heads, heads, F, TL, time != nullptr, false)) return why;
    if (N == 0 || n_heads == 0) return nullptr;
    if (!xyz || (F > 0 && !feat)) return "null pointer (xyz, or features with n_features > 0)";
    GroupInK P;
    P.n_heads = n_heads; P.N = N; P.F = F; P.TL = TL; P.l_max = 0;
    P.xyz = xyz; P.feat = feat; P.time = time; P.d_xyz = nullptr; P.d_feat = nullptr;
    int q = 0;
    for (int h = 0; h < n_heads; ++h) { P.head[h] = heads[h]; P.qfirst[h] = q; q += heads[h].row >> 2; }
    for (int h = n_heads; h <= SR_MLP_GROUP_MAX_HEADS; ++h) P.qfirst[h] = q;
    P.q_total = q;
    const long long blocks = ((long long)N * q + kBlock - 1) / kBlock;
    if (blocks > 0x7fffffffLL) return "too many points for one launch";
    hipLaunchKernelGGL(k_mlp_group_input_forward, dim3((unsigned)blocks), dim3(kBlock), 0, st, P);
    return nullptr;
}

static const char* launch_mlp_group_input_backward(int N, int n_heads, const SrMlpHeadInput* heads, int F, const float* xyz, float* d_xyz, float* d_feat,
                                                   hipStream_t st) {
    if (const char* why = group_input_check(N, n_heads, heads, F, 0, false, true)) return why;
    if (N == 0 || n_heads == 0 || (!d_xyz && !d_feat)) return nullptr;
    if (!xyz) return "null pointer (xyz)";
    GroupInK P;
    P.n_heads = n_heads; P.N = N; P.F = F; P.TL = 0; P.l_max = 0; P.q_total = 0;
    P.xyz = xyz; P.feat = nullptr; P.time = nullptr; P.d_xyz = d_xyz; P.d_feat = F > 0 ? d_feat : nullptr;
    for (int h = 0; h < n_heads; ++h) { P.head[h] = heads[h]; P.qfirst[h] = 0; P.l_max = max(P.l_max, heads[h].multires); }
    for (int h = n_heads; h <= SR_MLP_GROUP_MAX_HEADS; ++h) P.qfirst[h] = 0;
    const long long blocks = ((long long)N * (1 + (F + 3) / 4) + kBlock - 1) / kBlock;
    if (blocks > 0x7fffffffLL) return "too many points for one launch";
    hipLaunchKernelGGL(k_mlp_group_input_backward, dim3((unsigned)blocks), dim3(kBlock), 0, st, P);
    return nullptr;
}

static const char* group_output_check(int N, int n_heads, const SrMlpHeadOutput* heads, bool top) {
    if (N < 0) return "n_points must not be negative";
    if (n_heads < 0 || n_heads > SR_MLP_GROUP_MAX_HEADS) return "between 0 and SR_MLP_GROUP_MAX_HEADS heads";
    if (n_heads > 0 && !heads) return "null head table";
    for (int h = 0; h < n_heads; ++h) {
        const SrMlpHeadOutput& s = heads[h];
        if (s.out_features < 1 || s.out_features > 128) return "out_features must be in 1..128";
        if (s.activation != SR_MLP_OUT_NONE && s.activation != SR_MLP_OUT_SIGMOID && s.activation != SR_MLP_OUT_NORMALIZE) return "unknown output activation";
        if (!s.y) return "null pointer in the head table";
        if (top) {
            if (s.row < 4 || (s.row & 3) || s.row < s.out_features) return "row must be a multiple of 4 and >= out_features";
            if (!s.g) return "null pointer in the head table";
            if (reinterpret_cast<uintptr_t>(s.g) & 15u) return "g must be 16-byte aligned";
        } else if (!s.out) return "null pointer in the head table";
        if ((reinterpret_cast<uintptr_t>(s.y) | reinterpret_cast<uintptr_t>(s.out) | reinterpret_cast<uintptr_t>(s.dL_dout)) & 3u) return "float arrays must be 4-byte aligned";
    }
    return nullptr;
}

static const char* launch_mlp_group_output(int N, int n_heads, const SrMlpHeadOutput* heads, hipStream_t st) {
    if (const char* why = group_output_check(N, n_heads, heads, false)) return why;
    if (N == 0 || n_heads == 0) return nullptr;
    GroupOutK P;
    P.n_heads = n_heads; P.N = N; P.q_total = 0; P.slope = 0.0f;
    for (int h = 0; h < n_heads; ++h) { P.head[h] = heads[h]; P.qfirst[h] = 0; }
    for (int h = n_heads; h <= SR_MLP_GROUP_MAX_HEADS; ++h) P.qfirst[h] = 0;
    const long long blocks = ((long long)N * n_heads + kBlock - 1) / kBlock;
    hipLaunchKernelGGL(k_mlp_group_output, dim3((unsigned)blocks), dim3(kBlock), 0, st, P);
    return nullptr;
}

static const char* launch_mlp_group_top_gradient(int N, int n_heads, const SrMlpHeadOutput* heads, float slope, hipStream_t st) {
    if (const char* why = group_output_check(N, n_heads, heads, true)) return why;
    if (N == 0 || n_heads == 0) return nullptr;
    GroupOutK P;
    P.n_heads = n_heads; P.N = N; P.slope = slope;
    int q = 0;
    for (int h = 0; h < n_heads; ++h) { P.head[h] = heads[h]; P.qfirst[h] = q; q += heads[h].row >> 2; }
    for (int h = n_heads; h <= SR_MLP_GROUP_MAX_HEADS; ++h) P.qfirst[h] = q;
    P.q_total = q;
    const long long blocks = ((long long)N * q + kBlock - 1) / kBlock;
    if (blocks > 0x7fffffffLL) return "too many points for one launch";
    hipLaunchKernelGGL(k_mlp_group_top_gradient, dim3((unsigned)blocks), dim3(kBlock), 0, st, P);
    return nullptr;
}

}  // namespace sr

// ---- C entry points (include/splatraster.h): what is refused on the host, then the launchers above --------------------
using sr::fail; using sr::check_hip;

extern "C" {

static int mlp_chain_entry(const char* name, sr::MlpMode mode, int n_points, int hidden_tiles, int n_ops, const SrMlpOp* ops, float negative_slope, void* hip_stream) {
    if (n_points < 0 || !ops) return fail(std::string("bad arguments to ") + name);
    if (!(negative_slope >= 0.0f && negative_slope < 1.0f)) return fail(std::string(name) + ": negative_slope must be in [0, 1)");
    if (sr::launch_mlp_chain(n_points, hidden_tiles, n_ops, ops, negative_slope, mode, static_cast<hipStream_t>(hip_stream)))
        return fail(std::string(name) + ": unsupported op list (hidden_tiles 4 or 8, <= SR_MLP_MAX_OPS ops, even input tile counts, "
                    "16-byte aligned rows wide enough for the tiles read)");
    return check_hip(hipGetLastError(), name + 3);      // the kernel's label: the entry's name without "sr_"
}

static int mlp_pack_entry(const char* name, sr::MlpMode mode, int n_jobs, const SrMlpPackJob* jobs, void* hip_stream) {
    if (n_jobs < 0 || (n_jobs > 0 && !jobs)) return fail(std::string("bad arguments to ") + name);
    if (sr::launch_mlp_pack(n_jobs, jobs, mode, static_cast<hipStream_t>(hip_stream)))
        return fail(std::string(name) + ": unsupported job (<= SR_MLP_MAX_PACK_JOBS jobs; mem_pad multiple of 32, reg_width of 16, even tile "
                    "count; counts within their padded sizes; 16-byte aligned destination)");
    return check_hip(hipGetLastError(), name + 3);      // the kernel's label: the entry's name without "sr_"
}

int sr_mlp_chain(int n_points, int hidden_tiles, int n_ops, const SrMlpOp* ops, float negative_slope, void* hip_stream) {
    return mlp_chain_entry("sr_mlp_chain", sr::kMlpFp32, n_points, hidden_tiles, n_ops, ops, negative_slope, hip_stream);
}

int sr_mlp_chain_bf16(int n_points, int hidden_tiles, int n_ops, const SrMlpOp* ops, float negative_slope, void* hip_stream) {
    return mlp_chain_entry("sr_mlp_chain_bf16", sr::kMlpBf16, n_points, hidden_tiles, n_ops, ops, negative_slope, hip_stream);
}

int sr_mlp_chain_bf16x3(int n_points, int hidden_tiles, int n_ops, const SrMlpOp* ops, float negative_slope, void* hip_stream) {
    return mlp_chain_entry("sr_mlp_chain_bf16x3", sr::kMlpBf16x3, n_points, hidden_tiles, n_ops, ops, negative_slope, hip_stream);
}

// `empty`: the call was valid and launched nothing (no device is needed for that)
static int mlp_group_entry(const char* name, const char* why, const char* kernel, bool empty) {
    if (why) return fail(std::string(name) + ": " + why);
    if (empty) return 0;
    return check_hip(hipGetLastError(), kernel);
}

static int mlp_chain_group_entry(const char* name, const char* kernel, sr::MlpMode mode, int n_points, int hidden_tiles, int n_nets, const SrMlpNet* nets, float negative_slope, void* hip_stream) {
    if (!(negative_slope >= 0.0f && negative_slope < 1.0f)) return fail(std::string(name) + ": negative_slope must be in [0, 1)");
    return mlp_group_entry(name, sr::launch_mlp_chain_group(n_points, hidden_tiles, n_nets, nets, negative_slope, mode, static_cast<hipStream_t>(hip_stream)),
                           kernel, n_points == 0 || n_nets == 0);
}

int sr_mlp_chain_group(int n_points, int hidden_tiles, int n_nets, const SrMlpNet* nets, float negative_slope, void* hip_stream) {
    return mlp_chain_group_entry("sr_mlp_chain_group", "mlp_chain_group", sr::kMlpFp32, n_points, hidden_tiles, n_nets, nets, negative_slope, hip_stream);
}

int sr_mlp_chain_group_bf16(int n_points, int hidden_tiles, int n_nets, const SrMlpNet* nets, float negative_slope, void* hip_stream) {
    return mlp_chain_group_entry("sr_mlp_chain_group_bf16", "mlp_chain_group_bf16", sr::kMlpBf16, n_points, hidden_tiles, n_nets, nets, negative_slope, hip_stream);
}

int sr_mlp_chain_group_bf16x3(int n_points, int hidden_tiles, int n_nets, const SrMlpNet* nets, float negative_slope, void* hip_stream) {
    return mlp_chain_group_entry("sr_mlp_chain_group_bf16x3", "mlp_chain_group_bf16x3", sr::kMlpBf16x3, n_points, hidden_tiles, n_nets, nets, negative_slope, hip_stream);
}

int sr_mlp_group_input_forward(int n_points, int n_heads, const SrMlpHeadInput* heads, int n_features, int time_multires, const float* xyz,
                               const float* features, const float* time, void* hip_stream) {
    return mlp_group_entry("sr_mlp_group_input_forward", sr::launch_mlp_group_input_forward(n_points, n_heads, heads, n_features, time_multires, xyz,
                           features, time, static_cast<hipStream_t>(hip_stream)), "mlp_group_input_forward", n_points == 0 || n_heads == 0);
}

int sr_mlp_group_input_backward(int n_points, int n_heads, const SrMlpHeadInput* heads, int n_features, const float* xyz, float* dL_dxyz,
                                float* dL_dfeatures, void* hip_stream) {
    return mlp_group_entry("sr_mlp_group_input_backward", sr::launch_mlp_group_input_backward(n_points, n_heads, heads, n_features, xyz, dL_dxyz,
                           dL_dfeatures, static_cast<hipStream_t>(hip_stream)), "mlp_group_input_backward", n_points == 0 || n_heads == 0 || (!dL_dxyz && !dL_dfeatures));
}

int sr_mlp_group_output(int n_points, int n_heads, const SrMlpHeadOutput* heads, void* hip_stream) {
    return mlp_group_entry("sr_mlp_group_output", sr::launch_mlp_group_output(n_points, n_heads, heads, static_cast<hipStream_t>(hip_stream)),
                           "mlp_group_output", n_points == 0 || n_heads == 0);
}

int sr_mlp_group_top_gradient(int n_points, int n_heads, const SrMlpHeadOutput* heads, float negative_slope, void* hip_stream) {
    if (!(negative_slope >= 0.0f && negative_slope < 1.0f)) return fail("sr_mlp_group_top_gradient: negative_slope must be in [0, 1)");
    return mlp_group_entry("sr_mlp_group_top_gradient", sr::launch_mlp_group_top_gradient(n_points, n_heads, heads, negative_slope,
                           static_cast<hipStream_t>(hip_stream)), "mlp_group_top_gradient", n_points == 0 || n_heads == 0);
}

int sr_mlp_pack(int n_jobs, const SrMlpPackJob* jobs, void* hip_stream) {
    return mlp_pack_entry("sr_mlp_pack", sr::kMlpFp32, n_jobs, jobs, hip_stream);
}

int sr_mlp_pack_bf16(int n_jobs, const SrMlpPackJob* jobs, void* hip_stream) {
    return mlp_pack_entry("sr_mlp_pack_bf16", sr::kMlpBf16, n_jobs, jobs, hip_stream);
}

int sr_mlp_pack_bf16x3(int n_jobs, const SrMlpPackJob* jobs, void* hip_stream) {
    return mlp_pack_entry("sr_mlp_pack_bf16x3", sr::kMlpBf16x3, n_jobs, jobs, hip_stream);
}

size_t sr_mlp_weight_grad_workspace(int n_points, int n_jobs, const SrMlpGradJob* jobs) {
    if (!jobs) return 0;
    return sr::mlp_weight_grad_workspace(n_points, n_jobs, jobs);
}

int sr_mlp_weight_grad(int n_points, int n_jobs, const SrMlpGradJob* jobs, void* workspace, size_t workspace_bytes, void* hip_stream) {
    if (!jobs || n_points < 1) return fail("bad arguments to sr_mlp_weight_grad");
    if (sr::launch_mlp_weight_grad(n_points, n_jobs, jobs, workspace, workspace_bytes, static_cast<hipStream_t>(hip_stream)))
        return fail("sr_mlp_weight_grad: unsupported job list (<= SR_MLP_MAX_GRAD_JOBS jobs, <= SR_MLP_MAX_GRAD_TASKS 64x64 blocks, "
                    "16-byte aligned rows with strides that are multiples of 4) or workspace too small");
    return check_hip(hipGetLastError(), "mlp_weight_grad");
}

int sr_mlp_input_forward(int n_points, int multires, int n_features, int time_multires, int row, const float* xyz, const float* features,
                         const float* time, float* x0, void* hip_stream) {
    if (sr::launch_mlp_input_forward(n_points, multires, n_features, time_multires, row, xyz, features, time, x0, static_cast<hipStream_t>(hip_stream)))
        return fail("bad arguments to sr_mlp_input_forward (row a multiple of 4 and >= 3 + 6 multires + n_features [+ 1 + 2 time_multires "
                    "with a time], both multires <= 16)");
    return check_hip(hipGetLastError(), "mlp_input_forward");
}

int sr_mlp_top_gradient(int n_points, int out_features, int row, const float* y, const float* dL_dy, float negative_slope, float* g,
                        void* hip_stream) {
    if (!(negative_slope >= 0.0f && negative_slope < 1.0f)) return fail("sr_mlp_top_gradient: negative_slope must be in [0, 1)");
    if (sr::launch_mlp_top_gradient(n_points, out_features, row, y, dL_dy, negative_slope, g, static_cast<hipStream_t>(hip_stream)))
        return fail("bad arguments to sr_mlp_top_gradient (row a multiple of 4 and >= out_features)");
    return check_hip(hipGetLastError(), "mlp_top_gradient");
}

int sr_mlp_input_backward(int n_points, int multires, int n_features, int row, const float* xyz, const float* dL_dx0, float* dL_dxyz,
                          float* dL_dfeatures, void* hip_stream) {
    if (sr::launch_mlp_input_backward(n_points, multires, n_features, row, xyz, dL_dx0, dL_dxyz, dL_dfeatures, static_cast<hipStream_t>(hip_stream)))
        return fail("bad arguments to sr_mlp_input_backward");
    return check_hip(hipGetLastError(), "mlp_input_backward");
}

int sr_resfield_compose(int n_jobs, const SrResFieldJob* jobs, const long long* frame, void* hip_stream) {
    if (sr::launch_resfield_compose(n_jobs, jobs, frame, static_cast<hipStream_t>(hip_stream)))
        return fail("sr_resfield_compose: unsupported job list (<= SR_RESFIELD_MAX_JOBS jobs, count a multiple of 4, 16-byte aligned "
                    "arrays, 1 <= rank <= SR_RESFIELD_MAX_RANK) or null frame pointer");
    return check_hip(hipGetLastError(), "resfield_compose");
}

size_t sr_resfield_backward_workspace(int n_jobs, const SrResFieldJob* jobs) { return sr::resfield_backward_workspace(n_jobs, jobs); }

int sr_resfield_backward(int n_jobs, const SrResFieldJob* jobs, const long long* frame, void* workspace, size_t workspace_bytes,
                         void* hip_stream) {
    if (sr::launch_resfield_backward(n_jobs, jobs, frame, workspace, workspace_bytes, static_cast<hipStream_t>(hip_stream)))
        return fail("sr_resfield_backward: unsupported job list, null frame pointer or workspace too small");
    return check_hip(hipGetLastError(), "resfield_backward");
}

}  // extern "C"
