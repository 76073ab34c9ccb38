// The sum over the views of a training step of the gradients of the inputs those views share: every tensor in one launch
// (DESIGN.md "Views of a step").
//
// rasterizer.rasterize_views runs sr_backward once per view into view-major buffers [V, N, c]; what the per-view loop leaves to
// autograd -- a pairwise add kernel per shared input and view -- is this one streaming pass:
//
//   dst[i] = ((src[V-1][i] + src[V-2][i]) + ...) + src[0][i]
//
// The fold runs from the LAST view to the first because that is the order in which autograd accumulates the gradients of V nodes
// that share an input (the node created last runs first), and float32 addition is not associative: with this order the sum
// has the loop's bits.  Plain additions, nothing a compiler may contract.
//
// Work split, as in adam.hip.  The kernel argument is the job table itself (no copy, no wait).  A job's elements are laid over
// "slots" of four floats that start at the 16-byte boundary at or below dst: slot s holds the virtual elements 4 s .. 4 s + 3,
// element e of the tensor is virtual element lead + e.  Where dst, src and the view stride agree modulo 16 bytes every slot
// that lies inside the tensor moves as one 16-byte load per view and one 16-byte store; the first and last slot (and every slot
// of a job whose addresses disagree) go element by element.  A chunk is kSumChunkSlots slots of ONE job; chunks are numbered
// across the jobs and a workgroup walks them with a grid stride.  All loads of a slot are issued before the first addition.
//
// More than SR_SUM_MAX_VIEWS views: launches of at most that many each, from the last views down; every launch but the first
// starts its fold from what dst holds.  The association is the same as in one pass.
//
// No LDS, no atomics, no scratch; every store is a vector store.
#include "host_api.h"
#include "adam_math.h"

namespace sr {

namespace {

constexpr int kSumChunkSlots = kBlock;   // 256 slots = 4 KB of every view's stream
constexpr int kSumBlocksPerCu = 8;

struct SumTable {
    SrSumJob job[SR_SUM_MAX_JOBS];      // src already points at the FIRST view of this launch
    int chunk_end[SR_SUM_MAX_JOBS];     // running sum of the jobs' chunk counts
    int total_chunks;
    int n_views;                        // 1 .. SR_SUM_MAX_VIEWS views of this launch
    int from_dst;                       // the fold starts from dst (a chained launch) instead of from the last view
};

// floats between the 16-byte boundary below dst and dst; -1 when dst, src and the stride disagree modulo 16 bytes
__host__ __device__ __forceinline__ int sum_lead(const SrSumJob& job, int n_views) {
    const bool same = adam_lead_of(job.dst) == adam_lead_of(job.src) && (n_views == 1 || (job.view_stride & 3ll) == 0);
    return same ? (int)adam_lead_of(job.dst) : -1;
}

__global__ __launch_bounds__(kBlock) void k_sum_views(const SumTable t) {
    const int V = t.n_views;
    for (int chunk = blockIdx.x; chunk < t.total_chunks; chunk += gridDim.x) {
        int j = 0;
        while (chunk >= t.chunk_end[j]) ++j;            // uniform: scalar compares against the kernel argument
        const SrSumJob& job = t.job[j];
        const int aligned = sum_lead(job, V);
        const bool vec = aligned >= 0;
        const unsigned lead = vec ? (unsigned)aligned : 0u;
        // virtual element 0 is that boundary: the bases are only dereferenced at virtual elements lead .. lead + elems - 1
        float* const D = job.dst - lead;
        const float* const S = job.src - lead;
        const size_t stride = (size_t)job.view_stride;
        const unsigned end = lead + (unsigned)job.elems;    // <= 2^31 + 2
        const unsigned slots = (end + 3u) / 4u;
        const unsigned s = (unsigned)(chunk - (j ? t.chunk_end[j - 1] : 0)) * kSumChunkSlots + threadIdx.x;
        if (s >= slots) continue;
        const size_t e = (size_t)s * 4u;
        if (vec && e >= lead && e + 4u <= end) {
            float4 x[SR_SUM_MAX_VIEWS];
#pragma unroll
            for (int v = 0; v < SR_SUM_MAX_VIEWS; ++v)
                if (v < V) x[v] = load4(S + (size_t)v * stride + e);
            float4 acc = t.from_dst ? load4(D + e) : make_float4(0.f, 0.f, 0.f, 0.f);
            bool first = !t.from_dst;
#pragma unroll
            for (int v = SR_SUM_MAX_VIEWS - 1; v >= 0; --v) {
                if (v >= V) continue;
                if (first) { acc = x[v]; first = false; }
                else { acc.x = acc.x + x[v].x; acc.y = acc.y + x[v].y; acc.z = acc.z + x[v].z; acc.w = acc.w + x[v].w; }
            }
            store4(D + e, acc);
            continue;
        }
        // the first and the last slot of a job, and jobs whose addresses disagree modulo 16
#pragma unroll 1
        for (unsigned i = 0; i < 4u; ++i) {
            const size_t x = e + i;
            if (x < lead || x >= end) continue;
            float acc = t.from_dst ? D[x] : S[(size_t)(V - 1) * stride + x];
#pragma unroll 1
            for (int v = t.from_dst ? V - 1 : V - 2; v >= 0; --v) acc = acc + S[(size_t)v * stride + x];
            D[x] = acc;
        }
    }
}

// one launch: views [first, first + n) of every job
void launch_sum_views(int n_jobs, const SrSumJob* jobs, int first, int n, bool from_dst, hipStream_t st) {
    SumTable t = {};
    int m = 0;
    long long chunks = 0;
    for (int i = 0; i < n_jobs; ++i) {
        if (jobs[i].elems == 0) continue;
        SrSumJob job = jobs[i];
        job.src += (long long)first * job.view_stride;
        const long long lead = sum_lead(job, n) > 0 ? sum_lead(job, n) : 0;
        const long long slots = (lead + job.elems + 3) / 4;
        chunks += (slots + kSumChunkSlots - 1) / kSumChunkSlots;
        t.job[m] = job;
        t.chunk_end[m] = (int)chunks;                                  // <= 16 * 2^21
        ++m;
    }
    if (m == 0) return;
    t.total_chunks = (int)chunks;
    t.n_views = n;
    t.from_dst = from_dst ? 1 : 0;
    const long long cap = (long long)adam_cu_count() * kSumBlocksPerCu;
    hipLaunchKernelGGL(k_sum_views, dim3((unsigned)(chunks < cap ? chunks : cap)), dim3(kBlock), 0, st, t);
}

}  // namespace

}  // namespace sr

// ---- C entry point (include/splatraster.h): what is refused on the host, then the launcher above --------------------------
using sr::fail; using sr::check_hip; using sr::any_unaligned4;

extern "C" {

int sr_sum_views(int n_jobs, const SrSumJob* jobs, int n_views, void* hip_stream) {
    if (n_jobs < 0 || n_jobs > SR_SUM_MAX_JOBS) return fail("bad arguments to sr_sum_views: n_jobs must be 0 .. SR_SUM_MAX_JOBS (16)");
    if (n_views < 1) return fail("bad arguments to sr_sum_views: n_views must be at least 1");
    if (n_jobs > 0 && !jobs) return fail("null pointer in sr_sum_views: jobs");
    bool work = false;
    for (int i = 0; i < n_jobs; ++i) {
        const SrSumJob& j = jobs[i];
        const std::string at = " (job " + std::to_string(i) + ")";
        if (j.elems < 0) return fail("bad arguments to sr_sum_views: negative element count" + at);
        if (j.elems > 0x7fffffffll) return fail("too many elements for sr_sum_views: at most 2^31 - 1 in one job" + at);
        if (j.elems == 0) continue;
        if (!j.dst || !j.src) return fail("null pointer in sr_sum_views" + at);
        if (any_unaligned4(j.dst, j.src)) return fail("sr_sum_views: tensors must be 4-byte aligned" + at);
        if (n_views > 1 && j.view_stride < j.elems) return fail("sr_sum_views: view_stride must be at least elems (the views of a job do not overlap)" + at);
        work = true;
    }
    if (!work) return 0;
    const hipStream_t st = static_cast<hipStream_t>(hip_stream);
    // from the last views down; a chained launch folds the next SR_SUM_MAX_VIEWS views onto the partial sum in dst
    for (int hi = n_views; hi > 0; hi -= SR_SUM_MAX_VIEWS) {
        const int lo = hi > SR_SUM_MAX_VIEWS ? hi - SR_SUM_MAX_VIEWS : 0;
        sr::launch_sum_views(n_jobs, jobs, lo, hi - lo, hi != n_views, st);
        SR_TRY(check_hip(hipGetLastError(), "sum_views"));
    }
    return 0;
}

}  // extern "C"
