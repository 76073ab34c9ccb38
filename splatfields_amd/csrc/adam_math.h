// The arithmetic and the 16-byte memory accesses of an Adam step, shared by adam.hip (the splat tensors: the job table is the
// kernel argument) and network_adam.hip (the network's tensors: the job table lives on the device).  Both kernels include this
// header so that one element's update is the same instruction sequence, and therefore the same bits, in either.
//
//   m = beta1 m + (1 - beta1) g;   v = beta2 v + (1 - beta2) g^2;   p = p - step_size * m / (sqrt(v) / sqrt(1 - beta2^t) + eps)
//
// Both moments are evaluated in torch's `lerp` form, m + (1 - beta1) (g - m): the two weights then add up to 1 exactly.  With a
// float32 beta beside a float32 1 - beta they do not (0.9f + 0.1f is off by 1e-8, 0.999f + 0.001f by 1.3e-8), and that error
// enters the moment once per step and adds up over 1 / (1 - beta) steps -- 1.3e-5 of v for beta2 = 0.999.  `/` and sqrtf are the
// correctly rounded ones (no fast-math flag in build.py); every product that could be contracted with a neighbour is written
// as an explicit fmaf or stands alone, so the element-wise and the vector path give the same bits.
#pragma once
#include <cstdint>
#include "common.h"

namespace sr {

#ifndef SR_ADAM_NONTEMPORAL
// A/B switch (tools/adam_bench.py --variants, profiles/adam_bench.json): bit 0 = the gradients are read with non-temporal loads,
// bit 1 = parameter and moments are written with non-temporal stores.  Measured: bit 0 takes the step at 1 M splats from 0.325 to
// 0.279 ms and costs 1 % at 300 k, bit 1 alone gives 0.287, both 0.279.  0 is shipped: the build with bit 0 as the default has
// only been timed on the device, not run through tests/test_gpu_adam.py ("Next").
#define SR_ADAM_NONTEMPORAL 0
#endif

#ifndef SR_ADAM_UNROLL
#define SR_ADAM_UNROLL 2        // A/B switch: 2 keeps the dense kernel at 56 registers (8 waves per SIMD), 4 needs 88 (5 waves)
#endif
constexpr int kAdamUnroll = SR_ADAM_UNROLL;              // slots a thread has in flight in a full chunk
constexpr int kAdamChunkSlots = kBlock * kAdamUnroll;   // 512 slots = 8 KB of each of the four streams
constexpr int kAdamBlocksPerCu = 8;                      // 32 waves per CU

struct AdamScalars { float step_size, bias2_sqrt, om_beta1, om_beta2, eps; };

__device__ __forceinline__ void adam_element(float& p, float g, float& m, float& v, const AdamScalars& k) {
    m = fmaf(k.om_beta1, g - m, m);
    v = fmaf(k.om_beta2, fmaf(g, g, -v), v);
    const float denom = sqrtf(v) / k.bias2_sqrt + k.eps;
    const float ratio = m / denom;
    p = fmaf(-k.step_size, ratio, p);
}

// `bits`: bit i clear = element i keeps the bits that were loaded (adam.hip's row mask); 15 = all four are stepped
__device__ __forceinline__ void adam_vector(float4& p, const float4& g, float4& m, float4& v, unsigned bits, const AdamScalars& k) {
    float pn[4] = {p.x, p.y, p.z, p.w}, mn[4] = {m.x, m.y, m.z, m.w}, vn[4] = {v.x, v.y, v.z, v.w};
    const float gn[4] = {g.x, g.y, g.z, g.w};
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        float pi = pn[i], mi = mn[i], vi = vn[i];
        adam_element(pi, gn[i], mi, vi, k);
        const bool on = (bits >> i) & 1u;      // a hidden element keeps the bits that were loaded
        pn[i] = on ? pi : pn[i]; mn[i] = on ? mi : mn[i]; vn[i] = on ? vi : vn[i];
    }
    p = make_float4(pn[0], pn[1], pn[2], pn[3]);
    m = make_float4(mn[0], mn[1], mn[2], mn[3]);
    v = make_float4(vn[0], vn[1], vn[2], vn[3]);
}

typedef float NativeFloat4 __attribute__((ext_vector_type(4)));   // what the non-temporal builtins take

__device__ __forceinline__ float4 load_grad4(const float* g) {
#if SR_ADAM_NONTEMPORAL & 1
    const NativeFloat4 v = __builtin_nontemporal_load(reinterpret_cast<const NativeFloat4*>(g));
    return make_float4(v.x, v.y, v.z, v.w);
#else
    return *reinterpret_cast<const float4*>(g);
#endif
}

__device__ __forceinline__ float4 load4(const float* src) { return *reinterpret_cast<const float4*>(src); }

__device__ __forceinline__ void store4(float* dst, const float4& value) {
#if SR_ADAM_NONTEMPORAL & 2
    const NativeFloat4 v = {value.x, value.y, value.z, value.w};
    __builtin_nontemporal_store(v, reinterpret_cast<NativeFloat4*>(dst));
#else
    *reinterpret_cast<float4*>(dst) = value;
#endif
}

// floats between the 16-byte boundary at or below an address and that address: 0 .. 3
__host__ __device__ __forceinline__ unsigned adam_lead_of(const void* p) { return ((unsigned)(uintptr_t)p >> 2) & 3u; }

// the alignment test: the four streams of a job can move as 16-byte vectors where their addresses agree modulo 16
__host__ __device__ __forceinline__ bool adam_same_lead(const void* param, const void* grad, const void* exp_avg, const void* exp_avg_sq) {
    const unsigned lp = adam_lead_of(param);
    return lp == adam_lead_of(grad) && lp == adam_lead_of(exp_avg) && lp == adam_lead_of(exp_avg_sq);
}

// compute units of the current device (the grid is capped at kAdamBlocksPerCu workgroups on each); one query per device and process
inline int adam_cu_count() {
    static int cached[64] = {};
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 64) return 256;
    if (cached[dev] == 0) {
        int n = 0;
        cached[dev] = (hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, dev) == hipSuccess && n > 0) ? n : 256;
    }
    return cached[dev];
}

}  // namespace sr
