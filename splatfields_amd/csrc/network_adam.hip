// The Adam step of the deform network: hundreds of small tensors whose addresses do not change, one launch per
// SR_NET_ADAM_MAX_GRADS of them (DESIGN.md "Network optimizer step").
//
// Replaces reference train.py:318 (`deform.optimizer.step()`), the `torch.optim.Adam(l, lr=0.0, eps=1e-15)` that
// scene/deform_model.py:23-34 builds over every parameter of the network.  The arithmetic is adam.hip's (adam_math.h: the lerp
// form, correctly rounded `/` and sqrtf, explicit fmaf), so a tensor stepped here and a tensor stepped by k_adam get the same bits.
//
// What travels.  The job table -- per tensor the parameter, both moments, the element count and the running sum of chunk
// counts -- lives in device memory, written once by the caller.  A step's kernel argument holds, by value, the table pointer, the
// range of the table the launch covers, one set of scalars and the range's gradient pointers: nothing is copied, nothing is
// staged, nothing can be reused too early and nothing waits.
//
// Work split.  A tensor's elements are laid over slots of four floats that start at the 16-byte boundary at or below its
// PARAMETER's first element (the gradient's address changes every step and must not move the chunking): slot s holds the virtual
// elements 4 s .. 4 s + 3, element e of the tensor is virtual element lead + e.  A chunk is kAdamChunkSlots slots of one tensor;
// chunks are numbered across the table and a workgroup walks the range's chunks with a grid stride, finding the tensor of a
// chunk by a binary search over `chunk_end` -- uniform, through the constant address space, so it runs on scalar loads.  Where the
// four addresses of a tensor agree modulo 16 every slot inside the tensor moves as one 16-byte access per stream and only the
// first and last slot go element by element; where they disagree the whole tensor goes element by element.  Same bits either way.
//
// No LDS, no atomics, no scratch; every store is a vector store.
#include "host_api.h"
#include "adam_math.h"

namespace sr {

namespace {

struct NetAdamArgs {
    const SrNetAdamSlot* table;                       // device memory: entry `first` of the caller's table
    int n;                                            // entries of the range
    int total_chunks;                                 // of the range: < 2^31 (480 tensors of at most 2^20 chunks)
    long long chunk0;                                 // chunk_end of the entry before the range
    AdamScalars k;
    const float* grad[SR_NET_ADAM_MAX_GRADS];         // NULL: the tensor is skipped in this launch
};
static_assert(sizeof(NetAdamArgs) < 4096, "the step's data travels as the kernel argument");
static_assert(sizeof(SrNetAdamSlot) == 40, "three pointers and two long long, no padding");

// the table does not change while a kernel runs: read through the constant address space, a uniform index is a scalar load
typedef const SrNetAdamSlot __attribute__((address_space(4))) ConstSlot;

// slots and chunks of a tensor of `count` elements whose parameter starts `lead` floats past a 16-byte boundary
__host__ __device__ __forceinline__ long long net_adam_chunks(unsigned lead, long long count) {
    if (count == 0) return 0;
    const long long slots = ((long long)lead + count + 3) / 4;
    return (slots + kAdamChunkSlots - 1) / kAdamChunkSlots;
}

__global__ __launch_bounds__(kBlock) void k_net_adam(const NetAdamArgs a) {
    ConstSlot* const table = reinterpret_cast<ConstSlot*>(reinterpret_cast<uintptr_t>(a.table));
    const AdamScalars k = a.k;
    for (int c = blockIdx.x; c < a.total_chunks; c += gridDim.x) {
        const long long chunk = a.chunk0 + c;
        int lo = 0, hi = a.n - 1;                       // the first entry whose chunk_end lies above `chunk`: uniform
        while (lo < hi) {
            const int mid = (lo + hi) >> 1;
            if (table[mid].chunk_end > chunk) hi = mid; else lo = mid + 1;
        }
        const float* const grad = a.grad[lo];
        if (!grad) continue;
        float* const param = table[lo].param; float* const exp_avg = table[lo].exp_avg; float* const exp_avg_sq = table[lo].exp_avg_sq;
        const unsigned count = (unsigned)table[lo].count;
        const long long before = lo ? table[lo - 1].chunk_end : a.chunk0;
        const bool vec = adam_same_lead(param, grad, exp_avg, exp_avg_sq);
        const unsigned lead = adam_lead_of(param);
        // virtual element 0 is the boundary below the parameter: the bases are only dereferenced at virtual elements
        // lead .. lead + count - 1
        float* const P = param - lead; const float* const G = grad - lead;
        float* const M = exp_avg - lead; float* const V = exp_avg_sq - lead;
        const unsigned end = lead + count;              // <= 2^31 + 2
        const unsigned slot0 = (unsigned)(chunk - before) * kAdamChunkSlots;

        if (vec && slot0 * 4u >= lead && (slot0 + kAdamChunkSlots) * 4u <= end) {
            // a chunk of whole vectors: every load of the chunk is issued before the first use
            float4 p[kAdamUnroll], g[kAdamUnroll], m[kAdamUnroll], v[kAdamUnroll];
#pragma unroll
            for (int u = 0; u < kAdamUnroll; ++u) {
                const size_t e = (size_t)(slot0 + u * kBlock + threadIdx.x) * 4u;
                p[u] = load4(P + e); g[u] = load_grad4(G + e); m[u] = load4(M + e); v[u] = load4(V + e);
            }
#pragma unroll
            for (int u = 0; u < kAdamUnroll; ++u) {
                const size_t e = (size_t)(slot0 + u * kBlock + threadIdx.x) * 4u;
                adam_vector(p[u], g[u], m[u], v[u], 15u, k);
                store4(P + e, p[u]); store4(M + e, m[u]); store4(V + e, v[u]);
            }
            continue;
        }
        // the first and the last chunk of a tensor, and tensors whose four addresses disagree modulo 16
        const unsigned slots = (end + 3u) / 4u;
#pragma unroll 1
        for (int u = 0; u < kAdamUnroll; ++u) {
            const unsigned s = slot0 + u * kBlock + threadIdx.x;
            if (s >= slots) break;
            const size_t e = (size_t)s * 4u;
            if (vec && e >= lead && e + 4u <= end) {
                float4 p = load4(P + e), g = load_grad4(G + e), m = load4(M + e), v = load4(V + e);
                adam_vector(p, g, m, v, 15u, k);
                store4(P + e, p); store4(M + e, m); store4(V + e, v);
                continue;
            }
#pragma unroll 1
            for (unsigned i = 0; i < 4u; ++i) {
                const size_t x = e + i;
                if (x < lead || x >= end) continue;
                float p = P[x], m = M[x], v = V[x];
                adam_element(p, G[x], m, v, k);
                P[x] = p; M[x] = m; V[x] = v;
            }
        }
    }
}

}  // namespace

}  // namespace sr

// ---- C entry points (include/splatraster.h): what is refused on the host, then the launch ------------------------------
using sr::fail; using sr::check_hip; using sr::any_unaligned4;

extern "C" {

int sr_net_adam_plan(SrNetAdamSlot* table, int table_len) {
    if (table_len < 0) return fail("bad arguments to sr_net_adam_plan: negative table length");
    if (table_len > 0 && !table) return fail("null pointer in sr_net_adam_plan: table_host");
    long long chunks = 0;
    for (int i = 0; i < table_len; ++i) {
        const std::string at = " (entry " + std::to_string(i) + ")";
        if (table[i].count < 0) return fail("bad arguments to sr_net_adam_plan: negative element count" + at);
        if (table[i].count > 0x7fffffffll) return fail("too many elements for sr_net_adam_plan: at most 2^31 - 1 in one tensor" + at);
        if (any_unaligned4(table[i].param)) return fail("sr_net_adam_plan: tensors must be 4-byte aligned" + at);
        chunks += sr::net_adam_chunks(sr::adam_lead_of(table[i].param), table[i].count);
        table[i].chunk_end = chunks;
    }
    return 0;
}

int sr_net_adam_step(const SrNetAdamSlot* table_host, const SrNetAdamSlot* table_dev, int table_len, int first, int n,
                     const float* const* grads_host, const SrNetAdamScalars* scalars, void* hip_stream) {
    if (table_len < 0 || first < 0 || n < 0 || (long long)first + n > table_len)
        return fail("bad arguments to sr_net_adam_step: first .. first + n - 1 must lie inside the table of table_len entries");
    if (n > SR_NET_ADAM_MAX_GRADS) return fail("bad arguments to sr_net_adam_step: n must be 0 .. SR_NET_ADAM_MAX_GRADS (480)");
    if (n == 0) return 0;
    if (!table_host) return fail("null pointer in sr_net_adam_step: table_host");
    if (!table_dev) return fail("null pointer in sr_net_adam_step: table_dev");
    if (!grads_host) return fail("null pointer in sr_net_adam_step: grads_host");
    if (!scalars) return fail("null pointer in sr_net_adam_step: scalars");
    const long long chunk0 = first ? table_host[first - 1].chunk_end : 0;
    if (chunk0 < 0) return fail("sr_net_adam_step: chunk_end is not what sr_net_adam_plan fills (entry " + std::to_string(first - 1) + ")");
    long long chunks = chunk0;
    bool work = false;
    for (int i = 0; i < n; ++i) {
        const SrNetAdamSlot& s = table_host[first + i];
        const float* g = grads_host[i];
        if (s.count < 0) return fail("bad arguments to sr_net_adam_step: negative element count (entry " + std::to_string(first + i) + ")");
        if (s.count > 0x7fffffffll)
            return fail("too many elements for sr_net_adam_step: at most 2^31 - 1 in one tensor (entry " + std::to_string(first + i) + ")");
        if (any_unaligned4(s.param, g, s.exp_avg, s.exp_avg_sq))
            return fail("sr_net_adam_step: tensors must be 4-byte aligned (entry " + std::to_string(first + i) + ")");
        chunks += sr::net_adam_chunks(sr::adam_lead_of(s.param), s.count);
        if (s.chunk_end != chunks)
            return fail("sr_net_adam_step: chunk_end is not what sr_net_adam_plan fills (entry " + std::to_string(first + i) + ")");
        if (s.count == 0 || !g) continue;
        if (!s.param || !s.exp_avg || !s.exp_avg_sq) return fail("null pointer in sr_net_adam_step (entry " + std::to_string(first + i) + ")");
        work = true;
    }
    if (!work) return 0;
    sr::NetAdamArgs a = {};
    a.table = table_dev + first;
    a.n = n;
    a.total_chunks = (int)(chunks - chunk0);
    a.chunk0 = chunk0;
    a.k = sr::AdamScalars{scalars->step_size, scalars->bias_correction2_sqrt, scalars->one_minus_beta1, scalars->one_minus_beta2, scalars->eps};
    for (int i = 0; i < n; ++i) a.grad[i] = grads_host[i];
    const long long cap = (long long)sr::adam_cu_count() * sr::kAdamBlocksPerCu;
    const dim3 grid((unsigned)(a.total_chunks < cap ? a.total_chunks : cap));
    hipLaunchKernelGGL(sr::k_net_adam, grid, dim3(sr::kBlock), 0, static_cast<hipStream_t>(hip_stream), a);
    return check_hip(hipGetLastError(), "net_adam_step");
}

}  // extern "C"
