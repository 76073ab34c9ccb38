// Subset steps on the device (reference train.py:56-60, :68, :281-286 and scene/gaussian_model.py:431-438: `--n_splats`).
//
//   draw      idx[j] = P(j): a keyed bijection of [0, n_rows) evaluated per output -- an alternating Feistel network over the
//             smallest power-of-two domain that holds n_rows, walked until it lands below n_rows (include/splatraster.h has the
//             construction and why it ends).  Integer arithmetic, O(1) state per lane, no permutation of n_rows in memory.
//   ascending the same subset sorted: one lane per ROW asks whether P^-1(row) < n_pick (the same walk through the inverse network),
//             and the ballot words, the fixed-order scan and the ordered gather of ordered_scan.h number the members.
//   gather    all tensors of a step through idx in one launch (copy, exp, exp of one column into three), and its backward;
//   stats     sr_densification_stats with row -> idx[row] on the full-size outputs, through the same device function.
//
// All of it is streaming: no LDS beyond the scan's, no atomics, no floating-point sums across lanes.  The same inputs give the
// same bytes from call to call.
#include "host_api.h"
#include "ordered_scan.h"
#include "densify_stats.h"

namespace sr {

namespace {

constexpr long long kRowsMax = 2147483647LL;

// ---- the keyed bijection ------------------------------------------------------------------------------------------------
struct DrawMap {
    unsigned long long key[SR_DRAW_MAX_KEYS];
    int rounds;
    int lo_bits;                 // the low half's width; the high half has bits - lo_bits
    uint32_t lo_mask, hi_mask;
    uint32_t n_rows;             // 1 .. 2^31 - 1
};

DrawMap make_draw_map(long long n_rows, const unsigned long long* keys, int n_keys) {
    DrawMap m;
    for (int k = 0; k < SR_DRAW_MAX_KEYS; ++k) m.key[k] = k < n_keys ? keys[k] : 0ull;
    m.rounds = n_keys;
    int bits = 0;
    while ((1LL << bits) < n_rows) ++bits;                 // 0 .. 31
    m.lo_bits = bits / 2;
    m.lo_mask = (1u << m.lo_bits) - 1u;
    m.hi_mask = (1u << (bits - m.lo_bits)) - 1u;           // at most 16 bits
    m.n_rows = (uint32_t)n_rows;
    return m;
}

__device__ __forceinline__ uint32_t draw_mix(uint32_t v, unsigned long long key) {
    uint32_t h = (v + (uint32_t)key) * 0x9E3779B1u;
    h ^= h >> 15;
    h = (h ^ (uint32_t)(key >> 32)) * 0x85EBCA6Bu;
    h ^= h >> 13;
    h *= 0xC2B2AE35u;
    h ^= h >> 16;
    return h;
}

// F (or, the rounds in reverse order, F^-1) of x < 2^bits: every round is its own inverse
template <bool INVERSE>
__device__ __forceinline__ uint32_t draw_network(uint32_t x, const DrawMap& m) {
    uint32_t lo = x & m.lo_mask, hi = x >> m.lo_bits;
    for (int k = 0; k < m.rounds; ++k) {
        const int r = INVERSE ? m.rounds - 1 - k : k;        // the same in every lane: the keys are read as scalars
        if (r & 1) hi ^= draw_mix(lo, m.key[r]) & m.hi_mask;
        else lo ^= draw_mix(hi, m.key[r]) & m.lo_mask;
    }
    return (hi << m.lo_bits) | lo;
}

// P(x) (P^-1(x) with INVERSE) for x < n_rows, or -1 after SR_DRAW_MAX_WALK steps outside [0, n_rows): a bounded loop, whatever the map
template <bool INVERSE>
__device__ __forceinline__ long long draw_walk(uint32_t x, const DrawMap& m) {
    for (int step = 0; step < SR_DRAW_MAX_WALK; ++step) {
        x = draw_network<INVERSE>(x, m);
        if (x < m.n_rows) return (long long)x;
    }
    return -1;
}

__global__ void __launch_bounds__(kBlock) k_draw_rows(const DrawMap m, long long n_pick, long long* __restrict__ idx_out,
                                                      int* __restrict__ flag) {
    const long long j = (long long)blockIdx.x * kBlock + threadIdx.x;
    if (j >= n_pick) return;                                 // n_pick <= n_rows: j is a row number
    const long long row = draw_walk<false>((uint32_t)j, m);
    idx_out[j] = row;
    if (row < 0 && flag) *flag = 1;
}

// one lane per row: a member iff its preimage is one of the first n_pick
__global__ void __launch_bounds__(kBlock) k_draw_members(const DrawMap m, long long n_pick, unsigned long long* __restrict__ words,
                                                         uint32_t* __restrict__ block_counts, int* __restrict__ flag) {
    const long long i = (long long)blockIdx.x * kBlock + threadIdx.x;
    bool member = false;
    if (i < (long long)m.n_rows) {
        const long long j = draw_walk<true>((uint32_t)i, m);
        if (j < 0 && flag) *flag = 1;
        member = j >= 0 && j < n_pick;
    }
    compaction_mark(member, i, words, block_counts);         // every lane of the workgroup arrives here: lanes past n_rows vote 0
}

__global__ void __launch_bounds__(kScanBlock) k_draw_scan(long long blocks, uint32_t* __restrict__ block_counts, long long n_pick,
                                                          int* __restrict__ flag) {
    const uint32_t total = ordered_scan(blocks, [&](long long b) { return block_counts[b]; },
                                        [&](long long b, uint32_t offset) { block_counts[b] = offset; });
    if (threadIdx.x == 0 && flag && (long long)total != n_pick) *flag = 1;
}

__global__ void __launch_bounds__(kBlock) k_draw_number(long long n_rows, const unsigned long long* __restrict__ words,
                                                        const uint32_t* __restrict__ block_offsets, long long n_pick,
                                                        long long* __restrict__ idx_out) {
    const long long i = (long long)blockIdx.x * kBlock + threadIdx.x;
    if (i >= n_rows) return;
    long long rank;
    if (!compaction_rank(words, block_offsets, rank) || rank >= n_pick) return;   // rank < n_pick for a bijection: the bound of idx_out all the same
    idx_out[rank] = i;
}

struct DrawCarve { unsigned long long* words; uint32_t* counts; };

// member words [4 per workgroup of 256 rows] | workgroup counts / offsets
size_t carve_draw(void* base, long long n_rows, DrawCarve* out) {
    Carver c{static_cast<char*>(base), 0};
    const size_t blocks = (size_t)(((n_rows > 0 ? n_rows : 1) + kBlock - 1) / kBlock);
    DrawCarve t;
    t.words = c.take<unsigned long long>(blocks * (kBlock / kWave));
    t.counts = c.take<uint32_t>(blocks);
    if (out) *out = t;
    return align_up(c.off, 256);
}

// ---- gather / scatter of a step's tensors ---------------------------------------------------------------------------------
struct RowsTable {
    SrRowsJob job[SR_ROWS_MAX_JOBS];
    const float* dL_ddst[SR_ROWS_MAX_JOBS];
    float* dL_dsrc[SR_ROWS_MAX_JOBS];
    int col_end[SR_ROWS_MAX_JOBS];       // columns of one row of the launch, all jobs side by side: job k owns [col_end[k-1], col_end[k])
    int n_jobs, columns;
};

// item t of a launch -> (row j of the subset, job k, column c inside the job's row); false past the end
__device__ __forceinline__ bool rows_item(const RowsTable& tb, long long n_pick, long long& j, int& k, int& c) {
    const unsigned long long t = (unsigned long long)blockIdx.x * kBlock + threadIdx.x;
    j = (long long)(t / (unsigned)tb.columns);
    if (j >= n_pick) return false;
    c = (int)(t - (unsigned long long)j * (unsigned)tb.columns);
    k = 0;
    int first = 0;
    while (c >= tb.col_end[k]) first = tb.col_end[k++];      // ends inside the table: c < columns = col_end[n_jobs - 1]
    c -= first;
    return true;
}

// one lane per written float: consecutive lanes read consecutive floats of a source row and write consecutive floats of dst
__global__ void __launch_bounds__(kBlock) k_rows_gather(const RowsTable tb, long long n_pick, const long long* __restrict__ idx,
                                                        long long n_rows, int* __restrict__ flag) {
    long long j; int k, c;
    if (!rows_item(tb, n_pick, j, k, c)) return;
    const SrRowsJob& job = tb.job[k];
    float* out = job.dst + (size_t)j * (size_t)job.dst_row_stride + (size_t)(job.dst_col_offset + c);
    const long long row = idx[j];
    if (row < 0 || row >= n_rows) {
        *out = __int_as_float(0x7fc00000);
        if (flag) *flag = 1;
        return;
    }
    const float v = job.src[(size_t)row * (size_t)job.row_floats + (size_t)(job.op == SR_ROWS_EXP_TO3 ? 0 : c)];
    *out = job.op == SR_ROWS_COPY ? v : expf(v);
}

// one lane per float of a drawn SOURCE row
__global__ void __launch_bounds__(kBlock) k_rows_scatter(const RowsTable tb, long long n_pick, const long long* __restrict__ idx,
                                                         long long n_rows, int* __restrict__ flag) {
    long long j; int k, c;
    if (!rows_item(tb, n_pick, j, k, c)) return;
    const SrRowsJob& job = tb.job[k];
    const long long row = idx[j];
    if (row < 0 || row >= n_rows) {
        if (flag) *flag = 1;
        return;
    }
    const size_t at = (size_t)j * (size_t)job.dst_row_stride + (size_t)job.dst_col_offset;
    const float* g = tb.dL_ddst[k] + at;
    float d;
    if (job.op == SR_ROWS_COPY) d = g[c];
    else if (job.op == SR_ROWS_EXP) d = g[c] * job.dst[at + c];
    else d = ((g[0] + g[1]) + g[2]) * job.dst[at];
    tb.dL_dsrc[k][(size_t)row * (size_t)job.row_floats + (size_t)c] = d;
}

__global__ void __launch_bounds__(kBlock) k_densification_stats_rows(long long n_pick, const long long* __restrict__ idx, long long n_rows,
                                                                     const float* __restrict__ dL_dmeans2D, const int* __restrict__ radii,
                                                                     float* __restrict__ grad_accum, float* __restrict__ denom,
                                                                     float* __restrict__ max_radii2D, int* __restrict__ flag) {
    const long long i = (long long)blockIdx.x * kBlock + threadIdx.x;
    if (i >= n_pick) return;
    const int r = radii[i];
    if (r <= 0) return;  // visibility_filter = radii > 0
    const long long row = idx[i];
    if (row < 0 || row >= n_rows) {
        if (flag) *flag = 1;
        return;
    }
    const float gx = dL_dmeans2D[3 * (size_t)i], gy = dL_dmeans2D[3 * (size_t)i + 1];
    densification_stats_row((size_t)row, r, gx, gy, grad_accum, denom, max_radii2D);
}

}  // namespace

}  // namespace sr

// ---- C entry points (include/splatraster.h): what is refused on the host, then the launches ------------------------------------
using sr::fail; using sr::check_hip; using sr::kBlock;

extern "C" {

static int draw_arguments(const char* name, long long n_rows, long long n_pick, const unsigned long long* keys, int n_keys,
                          const long long* idx_out, const int* flag) {
    const std::string who(name);
    if (n_rows < 0 || n_rows > sr::kRowsMax) return fail(who + ": n_rows must be in 0 .. 2^31 - 1");
    if (n_pick < 0 || n_pick > n_rows) return fail(who + ": n_pick must be in 0 .. n_rows");
    if (n_keys < 1 || n_keys > SR_DRAW_MAX_KEYS) return fail(who + ": n_keys must be in 1 .. SR_DRAW_MAX_KEYS");
    if (!keys || (n_pick > 0 && !idx_out)) return fail("null pointer in " + who);
    if ((reinterpret_cast<uintptr_t>(idx_out) & 7u) || sr::any_unaligned4(flag)) return fail(who + ": idx_out must be 8-byte and flag 4-byte aligned");
    return 0;
}

int sr_draw_rows(long long n_rows, long long n_pick, const unsigned long long* keys, int n_keys, long long* idx_out, int* flag_or_null,
                 void* hip_stream) {
    SR_TRY(draw_arguments("sr_draw_rows", n_rows, n_pick, keys, n_keys, idx_out, flag_or_null));
    if (n_pick == 0) return 0;
    const sr::DrawMap m = sr::make_draw_map(n_rows, keys, n_keys);
    hipLaunchKernelGGL(sr::k_draw_rows, dim3((unsigned)((n_pick + kBlock - 1) / kBlock)), dim3(kBlock), 0, static_cast<hipStream_t>(hip_stream),
                       m, n_pick, idx_out, flag_or_null);
    return check_hip(hipGetLastError(), "draw_rows");
}

size_t sr_draw_rows_ascending_workspace_bytes(long long n_rows) {
    return n_rows < 0 || n_rows > sr::kRowsMax ? 0 : sr::carve_draw(nullptr, n_rows, nullptr);
}

int sr_draw_rows_ascending(long long n_rows, long long n_pick, const unsigned long long* keys, int n_keys, void* workspace,
                           long long* idx_out, int* flag_or_null, void* hip_stream) {
    SR_TRY(draw_arguments("sr_draw_rows_ascending", n_rows, n_pick, keys, n_keys, idx_out, flag_or_null));
    if (n_pick == 0) return 0;
    if (!workspace || (reinterpret_cast<uintptr_t>(workspace) & 7u)) return fail("null or misaligned workspace in sr_draw_rows_ascending");
    const sr::DrawMap m = sr::make_draw_map(n_rows, keys, n_keys);
    sr::DrawCarve c;
    sr::carve_draw(workspace, n_rows, &c);
    const long long blocks = (n_rows + kBlock - 1) / kBlock;
    hipStream_t st = static_cast<hipStream_t>(hip_stream);
    hipLaunchKernelGGL(sr::k_draw_members, dim3((unsigned)blocks), dim3(kBlock), 0, st, m, n_pick, c.words, c.counts, flag_or_null);
    hipLaunchKernelGGL(sr::k_draw_scan, dim3(1), dim3(sr::kScanBlock), 0, st, blocks, c.counts, n_pick, flag_or_null);
    hipLaunchKernelGGL(sr::k_draw_number, dim3((unsigned)blocks), dim3(kBlock), 0, st, n_rows, c.words, c.counts, n_pick, idx_out);
    return check_hip(hipGetLastError(), "draw_rows_ascending");
}

// the job table of a gather (scatter: with the two gradient lists) by value; `columns` counts what one subset row of the launch writes
static int rows_table(const char* name, int n_jobs, const SrRowsJob* jobs, const float* const* dL_ddst, float* const* dL_dsrc, bool scatter,
                      long long n_pick, const long long* idx, long long n_rows, const int* flag, sr::RowsTable* out) {
    const std::string who(name);
    if (n_jobs < 0 || n_jobs > SR_ROWS_MAX_JOBS) return fail(who + ": n_jobs must be in 0 .. SR_ROWS_MAX_JOBS");
    if (n_pick < 0 || n_pick > sr::kRowsMax) return fail(who + ": n_pick must be in 0 .. 2^31 - 1");
    if (n_rows < 0 || n_rows > sr::kRowsMax) return fail(who + ": n_rows must be in 0 .. 2^31 - 1");
    if ((n_jobs > 0 && !jobs) || (scatter && n_jobs > 0 && (!dL_ddst || !dL_dsrc)) || (n_pick > 0 && n_jobs > 0 && !idx))
        return fail("null pointer in " + who);
    if ((reinterpret_cast<uintptr_t>(idx) & 7u) || sr::any_unaligned4(flag)) return fail(who + ": idx must be 8-byte and flag 4-byte aligned");
    sr::RowsTable tb{};
    long long columns = 0;
    for (int k = 0; k < n_jobs; ++k) {
        const SrRowsJob& job = jobs[k];
        const std::string at = who + ", job " + std::to_string(k);
        if (job.op != SR_ROWS_COPY && job.op != SR_ROWS_EXP && job.op != SR_ROWS_EXP_TO3) return fail(at + ": unknown op");
        if (job.row_floats < 0) return fail(at + ": row_floats must not be negative");
        if (job.op == SR_ROWS_EXP_TO3 && job.row_floats > 1) return fail(at + ": SR_ROWS_EXP_TO3 reads rows of 1 float");
        const int written = job.op == SR_ROWS_EXP_TO3 ? 3 * job.row_floats : job.row_floats;
        if (job.dst_col_offset < 0 || (long long)job.dst_col_offset + written > (long long)job.dst_row_stride)
            return fail(at + ": the row does not fit into dst_row_stride");
        const bool skipped = job.row_floats == 0 || (scatter && !dL_dsrc[k]);
        if (!skipped) {
            if ((!scatter && !job.src) || !job.dst || (scatter && !dL_ddst[k])) return fail("null pointer in " + at);
            if (sr::any_unaligned4(job.src, job.dst) || (scatter && sr::any_unaligned4(dL_ddst[k], dL_dsrc[k]))) return fail(at + ": misaligned pointer");
            columns += scatter ? job.row_floats : written;
        }
        tb.job[k] = job;
        if (skipped) tb.job[k].row_floats = 0;
        tb.dL_ddst[k] = scatter ? dL_ddst[k] : nullptr;
        tb.dL_dsrc[k] = scatter ? dL_dsrc[k] : nullptr;
        tb.col_end[k] = (int)columns;
        if (columns > (1LL << 20)) return fail(who + ": more than 2^20 floats per row");
    }
    for (int k = n_jobs; k < SR_ROWS_MAX_JOBS; ++k) tb.col_end[k] = (int)columns;
    tb.n_jobs = n_jobs;
    tb.columns = (int)columns;
    if ((n_pick * columns + kBlock - 1) / kBlock > sr::kRowsMax) return fail(who + ": n_pick times the floats of a row exceeds 2^39");
    *out = tb;
    return 0;
}

int sr_rows_gather(int n_jobs, const SrRowsJob* jobs, long long n_pick, const long long* idx, long long n_rows, int* flag_or_null,
                   void* hip_stream) {
    sr::RowsTable tb;
    SR_TRY(rows_table("sr_rows_gather", n_jobs, jobs, nullptr, nullptr, false, n_pick, idx, n_rows, flag_or_null, &tb));
    if (n_pick == 0 || tb.columns == 0) return 0;
    hipLaunchKernelGGL(sr::k_rows_gather, dim3((unsigned)((n_pick * tb.columns + kBlock - 1) / kBlock)), dim3(kBlock), 0,
                       static_cast<hipStream_t>(hip_stream), tb, n_pick, idx, n_rows, flag_or_null);
    return check_hip(hipGetLastError(), "rows_gather");
}

int sr_rows_scatter(int n_jobs, const SrRowsJob* jobs, const float* const* dL_ddst, float* const* dL_dsrc, long long n_pick,
                    const long long* idx, long long n_rows, int* flag_or_null, void* hip_stream) {
    sr::RowsTable tb;
    SR_TRY(rows_table("sr_rows_scatter", n_jobs, jobs, dL_ddst, dL_dsrc, true, n_pick, idx, n_rows, flag_or_null, &tb));
    if (n_pick == 0 || tb.columns == 0) return 0;
    hipLaunchKernelGGL(sr::k_rows_scatter, dim3((unsigned)((n_pick * tb.columns + kBlock - 1) / kBlock)), dim3(kBlock), 0,
                       static_cast<hipStream_t>(hip_stream), tb, n_pick, idx, n_rows, flag_or_null);
    return check_hip(hipGetLastError(), "rows_scatter");
}

int sr_densification_stats_rows(long long n_pick, const long long* idx, long long n_rows, const float* dL_dmeans2D, const int* radii,
                                float* grad_accum, float* denom, float* max_radii2D, int* flag_or_null, void* hip_stream) {
    if (n_pick < 0 || n_pick > sr::kRowsMax) return fail("sr_densification_stats_rows: n_pick must be in 0 .. 2^31 - 1");
    if (n_rows < 0 || n_rows > sr::kRowsMax) return fail("sr_densification_stats_rows: n_rows must be in 0 .. 2^31 - 1");
    if (n_pick > 0 && (!idx || !dL_dmeans2D || !radii)) return fail("null pointer in sr_densification_stats_rows");
    if ((reinterpret_cast<uintptr_t>(idx) & 7u) || sr::any_unaligned4(dL_dmeans2D, radii, grad_accum, denom, max_radii2D, flag_or_null))
        return fail("sr_densification_stats_rows: idx must be 8-byte aligned, everything else 4-byte");
    if (n_pick == 0 || (!grad_accum && !denom && !max_radii2D)) return 0;
    hipLaunchKernelGGL(sr::k_densification_stats_rows, dim3((unsigned)((n_pick + kBlock - 1) / kBlock)), dim3(kBlock), 0,
                       static_cast<hipStream_t>(hip_stream), n_pick, idx, n_rows, dL_dmeans2D, radii, grad_accum, denom, max_radii2D,
                       flag_or_null);
    return check_hip(hipGetLastError(), "densification_stats_rows");
}

}  // extern "C"
