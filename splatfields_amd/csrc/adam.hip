// The Adam step of a training iteration: every tensor of the step in one launch (DESIGN.md "Optimizer step").
//
// Restates torch.optim.Adam (capturable=False, no weight decay, no amsgrad), which is what reference train.py:314-322 steps
// (scene/gaussian_model.py:130-139 builds it over six tensors), per element in float32:
//
//   m = beta1 m + (1 - beta1) g;   v = beta2 v + (1 - beta2) g^2;   p = p - step_size * m / (sqrt(v) / sqrt(1 - beta2^t) + eps)
//
// with step_size = lr / (1 - beta1^t) and the other scalars computed by the caller in double.  The element's arithmetic and the
// 16-byte accesses are adam_math.h's, shared with network_adam.hip.  Both moments are evaluated in
// torch's `lerp` form, m + (1 - beta1) (g - m): the two weights then add up to 1 exactly.  With a float32 beta beside a
// float32 1 - beta they do not (0.9f + 0.1f is off by 1e-8, 0.999f + 0.001f by 1.3e-8), and that error enters the moment once
// per step and adds up over 1 / (1 - beta) steps -- 1.3e-5 of v for beta2 = 0.999.  `/` and sqrtf are the correctly
// rounded ones (no fast-math flag in build.py); every product that could be contracted with a neighbour is written as an
// explicit fmaf or stands alone, so the element-wise and the vector path give the same bits.
//
// Work split.  The kernel argument is the job table itself (no copy, no wait).  A job's elements are laid over "slots" of four
// floats that start at the 16-byte boundary at or below its first element: slot s holds the virtual elements 4 s .. 4 s + 3,
// element e of the tensor is virtual element lead + e.  Where the four addresses of a job agree modulo 16 every slot that lies
// inside the tensor moves as one 16-byte load or store per stream; the first and last slot (and every slot of a job whose
// addresses disagree) go element by element.  A chunk is kAdamChunkSlots slots of ONE job; chunks are numbered across the jobs
// and a workgroup walks them with a grid stride, finding the job of a chunk by a scan of at most SR_ADAM_MAX_TENSORS sums.
//
// Row mask.  The same kernel with a predicate on (element / row): a slot none of whose rows is visible issues no load and no
// store; a slot with some visible rows stores the loaded bits back for the others.
//
// No LDS, no atomics, no scratch; every store is a vector store.
#include "host_api.h"
#include "adam_math.h"

namespace sr {

namespace {

struct AdamTable {
    SrAdamJob job[SR_ADAM_MAX_TENSORS];
    int chunk_end[SR_ADAM_MAX_TENSORS];   // running sum of the jobs' chunk counts
    int total_chunks;
    const unsigned char* visible;
};

// floats between the 16-byte boundary below a job's first element and that element; -1 when its four addresses disagree
// modulo 16 (no vector path: the job goes element by element from slot 0)
__host__ __device__ __forceinline__ int adam_lead(const SrAdamJob& job) {
    return adam_same_lead(job.param, job.grad, job.exp_avg, job.exp_avg_sq) ? (int)adam_lead_of(job.param) : -1;
}

// bit i set: virtual element 4 slot + i belongs to a visible row (the slot lies inside the tensor)
__device__ __forceinline__ unsigned visible_bits(const unsigned char* __restrict__ visible, unsigned first_element, unsigned row) {
    unsigned r = first_element / row, c = first_element - r * row, bits = 0;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        bits |= (visible[r] != 0 ? 1u : 0u) << i;
        if (++c == row) { c = 0; ++r; }
    }
    return bits;
}

template <bool MASKED>
__global__ __launch_bounds__(kBlock) void k_adam(const AdamTable t) {
    for (int chunk = blockIdx.x; chunk < t.total_chunks; chunk += gridDim.x) {
        int j = 0;
        while (chunk >= t.chunk_end[j]) ++j;            // uniform: scalar compares against the kernel argument
        const SrAdamJob& job = t.job[j];
        const AdamScalars k{job.step_size, job.bias_correction2_sqrt, job.one_minus_beta1, job.one_minus_beta2, job.eps};
        const unsigned count = (unsigned)job.count, row = (unsigned)job.row;
        const int aligned = adam_lead(job);
        const bool vec = aligned >= 0;
        const unsigned lead = vec ? (unsigned)aligned : 0u;
        // virtual element 0 is that boundary: the bases are only dereferenced at virtual elements lead .. lead + count - 1
        float* const P = job.param - lead; const float* const G = job.grad - lead;
        float* const M = job.exp_avg - lead; float* const V = job.exp_avg_sq - lead;
        const unsigned end = lead + count;              // <= 2^31 + 2
        const unsigned slot0 = (unsigned)(chunk - (j ? t.chunk_end[j - 1] : 0)) * kAdamChunkSlots;

        if (vec && slot0 * 4u >= lead && (slot0 + kAdamChunkSlots) * 4u <= end) {
            // a chunk of whole vectors: every load of the chunk is issued before the first use
            float4 p[kAdamUnroll], g[kAdamUnroll], m[kAdamUnroll], v[kAdamUnroll];
            unsigned bits[kAdamUnroll];
#pragma unroll
            for (int u = 0; u < kAdamUnroll; ++u) {
                const size_t e = (size_t)(slot0 + u * kBlock + threadIdx.x) * 4u;
                bits[u] = MASKED ? visible_bits(t.visible, (unsigned)e - lead, row) : 15u;
                if (bits[u]) {
                    p[u] = *reinterpret_cast<const float4*>(P + e); g[u] = load_grad4(G + e);
                    m[u] = *reinterpret_cast<const float4*>(M + e); v[u] = *reinterpret_cast<const float4*>(V + e);
                }
            }
#pragma unroll
            for (int u = 0; u < kAdamUnroll; ++u) {
                if (bits[u]) {
                    const size_t e = (size_t)(slot0 + u * kBlock + threadIdx.x) * 4u;
                    adam_vector(p[u], g[u], m[u], v[u], bits[u], k);
                    store4(P + e, p[u]); store4(M + e, m[u]); store4(V + e, v[u]);
                }
            }
            continue;
        }
        // the first and the last chunk of a job, and jobs whose four addresses disagree modulo 16
        const unsigned slots = (end + 3u) / 4u;
#pragma unroll 1
        for (int u = 0; u < kAdamUnroll; ++u) {
            const unsigned s = slot0 + u * kBlock + threadIdx.x;
            if (s >= slots) break;
            const size_t e = (size_t)s * 4u;
            const bool whole = e >= lead && e + 4u <= end;
            if (vec && whole) {
                const unsigned bits = MASKED ? visible_bits(t.visible, (unsigned)e - lead, row) : 15u;
                if (!bits) continue;
                float4 p = *reinterpret_cast<const float4*>(P + e), g = load_grad4(G + e);
                float4 m = *reinterpret_cast<const float4*>(M + e), v = *reinterpret_cast<const float4*>(V + e);
                adam_vector(p, g, m, v, bits, k);
                store4(P + e, p); store4(M + e, m); store4(V + e, v);
                continue;
            }
#pragma unroll 1
            for (unsigned i = 0; i < 4u; ++i) {
                const size_t x = e + i;
                if (x < lead || x >= end) continue;
                if (MASKED && !t.visible[((unsigned)x - lead) / row]) continue;
                float p = P[x], m = M[x], v = V[x];
                adam_element(p, G[x], m, v, k);
                P[x] = p; M[x] = m; V[x] = v;
            }
        }
    }
}

void launch_adam(int n_jobs, const SrAdamJob* jobs, const unsigned char* visible, hipStream_t st) {
    AdamTable t = {};
    int n = 0;
    long long chunks = 0;
    for (int i = 0; i < n_jobs; ++i) {
        if (jobs[i].count == 0) continue;
        const long long lead = adam_lead(jobs[i]) > 0 ? adam_lead(jobs[i]) : 0;
        const long long slots = (lead + jobs[i].count + 3) / 4;
        chunks += (slots + kAdamChunkSlots - 1) / kAdamChunkSlots;
        t.job[n] = jobs[i];
        t.chunk_end[n] = (int)chunks;                                  // <= 32 * 2^19
        ++n;
    }
    if (n == 0) return;
    t.total_chunks = (int)chunks;
    t.visible = visible;
    const long long cap = (long long)adam_cu_count() * kAdamBlocksPerCu;
    const dim3 grid((unsigned)(chunks < cap ? chunks : cap));
    if (visible) hipLaunchKernelGGL(k_adam<true>, grid, dim3(kBlock), 0, st, t);
    else hipLaunchKernelGGL(k_adam<false>, grid, dim3(kBlock), 0, st, t);
}

}  // namespace

}  // namespace sr

// ---- C entry points (include/splatraster.h): what is refused on the host, then the launchers above --------------------
using sr::fail; using sr::check_hip; using sr::any_unaligned4;

extern "C" {

int sr_adam_step(int n_jobs, const SrAdamJob* jobs, const unsigned char* visible, long long rows, void* hip_stream) {
    if (n_jobs < 0 || n_jobs > SR_ADAM_MAX_TENSORS) return fail("bad arguments to sr_adam_step: n_jobs must be 0 .. SR_ADAM_MAX_TENSORS (32)");
    if (n_jobs > 0 && !jobs) return fail("null pointer in sr_adam_step: jobs");
    if (visible && rows < 0) return fail("bad arguments to sr_adam_step: negative row count");
    bool work = false;
    for (int i = 0; i < n_jobs; ++i) {
        const SrAdamJob& j = jobs[i];
        const std::string at = " (job " + std::to_string(i) + ")";
        if (j.count < 0) return fail("bad arguments to sr_adam_step: negative element count" + at);
        if (j.count > 0x7fffffffll) return fail("too many elements for sr_adam_step: at most 2^31 - 1 in one job" + at);
        if (visible && (j.row <= 0 || j.count != rows * (long long)j.row))
            return fail("sr_adam_step: with a row mask every job needs count == rows * row" + at);
        if (j.count == 0) continue;
        if (!j.param || !j.grad || !j.exp_avg || !j.exp_avg_sq) return fail("null pointer in sr_adam_step" + at);
        if (any_unaligned4(j.param, j.grad, j.exp_avg, j.exp_avg_sq)) return fail("sr_adam_step: tensors must be 4-byte aligned" + at);
        work = true;
    }
    if (!work) return 0;
    sr::launch_adam(n_jobs, jobs, visible, static_cast<hipStream_t>(hip_stream));
    return check_hip(hipGetLastError(), "adam_step");
}

}  // extern "C"
