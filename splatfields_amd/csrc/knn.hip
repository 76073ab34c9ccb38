// Mean squared distance to the 3 nearest neighbours of every point -- the MI355X counterpart of
// [EXT] simple_knn._C.distCUDA2 (gitlab.inria.fr/bkerbl/simple-knn@44f7642, reference README.md:29), which the
// reference calls once at initialisation to size the splats (scene/gaussian_model.py:25, :105).
// SURVEY.md §8f row 3 ("next" row; not on the measured fwd+bwd path).
//
// Exact k-NN (k = 3, self excluded by index) on a uniform grid: points are counting-sorted into ~N/2 cells, and each
// point searches growing cubes of cells until its 3rd-best squared distance is <= (ring * cell_size)^2, which
// no point outside the cube can beat.  The published CUDA code does the same job with a Morton sort + box pruning.
//
// Second half of the file: the K-nearest-neighbour GRAPH (2 <= K <= 8, self included) of the Moran's I regulariser on the same
// grid -- the counterpart of [EXT] pytorch3d.ops.knn.knn_points at reference extract_geo.py:101-103.
#include "host_api.h"
#include "ordered_scan.h"

namespace sr {

struct KnnGrid { float3 lo; float inv_cell, cell; int gx, gy, gz; };

__device__ __forceinline__ int3 cell_of(const KnnGrid& g, float x, float y, float z) {
    // clamped as floats, before the conversion: a NaN coordinate lands in cell 0 and an infinite one in an end cell (fmaxf and
    // fminf return their other argument for a NaN), and no out-of-range value ever meets the float -> int conversion
    const float fx = fminf(fmaxf((x - g.lo.x) * g.inv_cell, 0.f), (float)(g.gx - 1));
    const float fy = fminf(fmaxf((y - g.lo.y) * g.inv_cell, 0.f), (float)(g.gy - 1));
    const float fz = fminf(fmaxf((z - g.lo.z) * g.inv_cell, 0.f), (float)(g.gz - 1));
    return make_int3((int)fx, (int)fy, (int)fz);
}

// one workgroup: bounding box of all finite points -> bounds[0..5]
__global__ void __launch_bounds__(1024) k_knn_bounds(int n, const float* __restrict__ pts, float* __restrict__ bounds) {
    __shared__ float s_lo[3][16], s_hi[3][16];
    float lo[3] = {3.0e38f, 3.0e38f, 3.0e38f}, hi[3] = {-3.0e38f, -3.0e38f, -3.0e38f};
    for (int i = threadIdx.x; i < n; i += 1024)
        for (int c = 0; c < 3; ++c) {  // NaN and +-inf stay out: one infinite coordinate would collapse the grid to a single cell
            const float v = pts[3 * (size_t)i + c];
            if (fabsf(v) <= 3.0e38f) { lo[c] = fminf(lo[c], v); hi[c] = fmaxf(hi[c], v); }
        }
    for (int c = 0; c < 3; ++c) {
        for (int d = 32; d > 0; d >>= 1) { lo[c] = fminf(lo[c], __shfl_xor(lo[c], d, 64)); hi[c] = fmaxf(hi[c], __shfl_xor(hi[c], d, 64)); }
        if ((threadIdx.x & 63) == 0) { s_lo[c][threadIdx.x >> 6] = lo[c]; s_hi[c][threadIdx.x >> 6] = hi[c]; }
    }
    __syncthreads();
    if (threadIdx.x < 3) {
        float l = 3.0e38f, h = -3.0e38f;
        for (int w = 0; w < 16; ++w) { l = fminf(l, s_lo[threadIdx.x][w]); h = fmaxf(h, s_hi[threadIdx.x][w]); }
        bounds[threadIdx.x] = l; bounds[3 + threadIdx.x] = h;
    }
}

__device__ __forceinline__ KnnGrid make_grid(const float* bounds, int n, int max_cells) {
    KnnGrid g;
    g.lo = make_float3(bounds[0], bounds[1], bounds[2]);
    float ex = bounds[3] - bounds[0], ey = bounds[4] - bounds[1], ez = bounds[5] - bounds[2];
    const float emax = fmaxf(ex, fmaxf(ey, ez));
    g.gx = g.gy = g.gz = 1; g.cell = 1.0f; g.inv_cell = 0.0f;  // degenerate cloud (all points equal / one point): one cell
    if (!(emax > 0.0f) || !(emax < 3.0e38f)) return g;
    // flat or linear clouds: give the thin axes a floor so that the cell size follows the populated extent
    ex = fmaxf(ex, 1e-3f * emax); ey = fmaxf(ey, 1e-3f * emax); ez = fmaxf(ez, 1e-3f * emax);
    // ~2 points per cell on average, never more cells than the workspace holds
    const float target = fminf(fmaxf(0.5f * n, 1.0f), (float)max_cells);
    float cell = fmaxf(cbrtf(ex) * cbrtf(ey) * cbrtf(ez) / cbrtf(target), emax / 1024.0f);
    bool ok = false;
    for (int it = 0; it < 64 && !ok; ++it) {
        g.gx = (int)(ex / cell) + 1; g.gy = (int)(ey / cell) + 1; g.gz = (int)(ez / cell) + 1;
        ok = (long long)g.gx * g.gy * g.gz <= (long long)max_cells;
        if (!ok) cell *= 1.3f;
    }
    if (!ok) { g.gx = g.gy = g.gz = 1; cell = 2.0f * emax; }
    g.cell = cell; g.inv_cell = 1.0f / cell;
    return g;
}

__global__ void k_knn_count(int n, const float* __restrict__ pts, const float* __restrict__ bounds, int max_cells, uint32_t* __restrict__ count) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const KnnGrid g = make_grid(bounds, n, max_cells);
    const int3 c = cell_of(g, pts[3 * (size_t)i], pts[3 * (size_t)i + 1], pts[3 * (size_t)i + 2]);
    atomicAdd(&count[(c.z * g.gy + c.y) * g.gx + c.x], 1u);
}

// exclusive scan of count[0..cells) by one workgroup (ordered_scan.h) -> start[0..cells]; cursor := 0
__device__ __forceinline__ void scan_counts(int cells, const uint32_t* __restrict__ count, uint32_t* __restrict__ start,
                                            uint32_t* __restrict__ cursor) {
    const uint32_t total = ordered_scan(cells, [&](long long i) { return count[i]; },
                                        [&](long long i, uint32_t offset) { start[i] = offset; cursor[i] = 0u; });
    if (threadIdx.x == 0) start[cells] = total;
}

__global__ void __launch_bounds__(kScanBlock) k_knn_scan(const float* __restrict__ bounds, int n, int max_cells, const uint32_t* __restrict__ count,
                                                         uint32_t* __restrict__ start, uint32_t* __restrict__ cursor) {
    const KnnGrid g = make_grid(bounds, n, max_cells);
    scan_counts(g.gx * g.gy * g.gz, count, start, cursor);
}

__global__ void k_knn_fill(int n, const float* __restrict__ pts, const float* __restrict__ bounds, int max_cells, const uint32_t* __restrict__ start,
                           uint32_t* __restrict__ cursor, uint32_t* __restrict__ order) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const KnnGrid g = make_grid(bounds, n, max_cells);
    const int3 c = cell_of(g, pts[3 * (size_t)i], pts[3 * (size_t)i + 1], pts[3 * (size_t)i + 2]);
    const int cell = (c.z * g.gy + c.y) * g.gx + c.x;
    order[start[cell] + atomicAdd(&cursor[cell], 1u)] = (uint32_t)i;
}

__device__ __forceinline__ void knn_insert(float d, float best[3]) {
    if (d < best[2]) {
        if (d < best[1]) { best[2] = best[1]; if (d < best[0]) { best[1] = best[0]; best[0] = d; } else best[1] = d; }
        else best[2] = d;
    }
}

__global__ void k_knn_search(int n, const float* __restrict__ pts, const float* __restrict__ bounds, int max_cells, const uint32_t* __restrict__ start,
                             const uint32_t* __restrict__ order, float* __restrict__ out) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const KnnGrid g = make_grid(bounds, n, max_cells);
    const float px = pts[3 * (size_t)i], py = pts[3 * (size_t)i + 1], pz = pts[3 * (size_t)i + 2];
    const int3 c = cell_of(g, px, py, pz);
    float best[3] = {3.0e38f, 3.0e38f, 3.0e38f};
    const int rmax = max(g.gx, max(g.gy, g.gz));
    for (int r = 0; r <= rmax; ++r) {
        // visit the shell of cells at Chebyshev distance r from the point's cell
        for (int dz = -r; dz <= r; ++dz) {
            const int z = c.z + dz; if (z < 0 || z >= g.gz) continue;
            for (int dy = -r; dy <= r; ++dy) {
                const int y = c.y + dy; if (y < 0 || y >= g.gy) continue;
                const bool face = (dz == -r || dz == r || dy == -r || dy == r);
                const int step = face ? 1 : max(2 * r, 1);  // interior rows of the shell only have the two x ends
                for (int dx = -r; dx <= r; dx += step) {
                    const int x = c.x + dx; if (x < 0 || x >= g.gx) continue;
                    const int cell = (z * g.gy + y) * g.gx + x;
                    for (uint32_t k = start[cell]; k < start[cell + 1]; ++k) {
                        const uint32_t j = order[k];
                        if ((int)j == i) continue;
                        const float ddx = pts[3 * (size_t)j] - px, ddy = pts[3 * (size_t)j + 1] - py, ddz = pts[3 * (size_t)j + 2] - pz;
                        knn_insert(ddx * ddx + ddy * ddy + ddz * ddz, best);
                    }
                }
            }
        }
        const float safe = r * g.cell;  // every unvisited point is farther than this
        if (best[2] <= safe * safe) break;
    }
    // always a third of the sum: with fewer than 4 points the missing neighbours contribute 0.  A neighbour that exists but
    // whose squared distance is no finite float32 (a point beyond ~1.8e19, a NaN or infinite row) counts as +inf, which is what
    // the published code's sum of FLT_MAX entries overflows to
    const int have = min(n - 1, 3);
    float sum = 0.f;
    for (int k = 0; k < have; ++k) sum += best[k] < 3.0e38f ? best[k] : __builtin_inff();
    out[i] = sum / 3.0f;
}

struct KnnCarve { int max_cells; float* bounds; uint32_t* count; uint32_t* start; uint32_t* cursor; uint32_t* unordered; uint32_t* unordered_edges; };

// bounds [8] | cell counts | cell starts | cell cursors [max_cells + 1 each] | the points, cell after cell, as the cursors left them [n]
// | the graph's reverse edges, target after target, likewise [n k] (k = 0, sr_knn3_mean_dist2: none)
static size_t carve_knn(void* base, int n, int k, KnnCarve* out) {
    Carver c{static_cast<char*>(base), 0};
    KnnCarve t;
    t.max_cells = n > 2 ? n : 2;
    t.bounds = c.take<float>(8);
    t.count = c.take<uint32_t>((size_t)t.max_cells + 1);
    t.start = c.take<uint32_t>((size_t)t.max_cells + 1);
    t.cursor = c.take<uint32_t>((size_t)t.max_cells + 1);
    t.unordered = c.take<uint32_t>((size_t)(n > 0 ? n : 1));
    t.unordered_edges = k > 0 ? c.take<uint32_t>((size_t)n * k) : nullptr;
    if (out) *out = t;
    return align_up(c.off, 256);
}

static void launch_knn3(int n, const float* pts, float* out, void* workspace, hipStream_t st) {
    if (n <= 0) return;
    KnnCarve c;
    carve_knn(workspace, n, 0, &c);
    const int nb = (n + 255) / 256;
    hipMemsetAsync(c.count, 0, sizeof(uint32_t) * ((size_t)c.max_cells + 1), st);
    hipLaunchKernelGGL(k_knn_bounds, dim3(1), dim3(1024), 0, st, n, pts, c.bounds);
    hipLaunchKernelGGL(k_knn_count, dim3(nb), dim3(256), 0, st, n, pts, c.bounds, c.max_cells, c.count);
    hipLaunchKernelGGL(k_knn_scan, dim3(1), dim3(kScanBlock), 0, st, c.bounds, n, c.max_cells, c.count, c.start, c.cursor);
    hipLaunchKernelGGL(k_knn_fill, dim3(nb), dim3(256), 0, st, n, pts, c.bounds, c.max_cells, c.start, c.cursor, c.unordered);
    hipLaunchKernelGGL(k_knn_search, dim3(nb), dim3(256), 0, st, n, pts, c.bounds, c.max_cells, c.start, c.unordered, out);
}

// ---- k-nearest-neighbour graph (self included) and its reverse adjacency: the Moran regulariser's neighbourhoods ----
//
// The same grid and the same growing-cube stop rule as above.  Everything that the unordered integer cursor of k_knn_fill
// touches is put into a fixed order before it is used: a cell's points by index (k_rank_segments), the K-best list by
// (squared distance, index), a target's incoming edges by edge id = source * K + slot (k_rank_segments again).

// slot s of a segmented list filled through a cursor -> its place by value inside its segment.  key[] names the segment
// of a value (NULL: the value's grid cell).  Work is the sum of the squared segment lengths, spread over all slots.
__global__ void k_rank_segments(int slots, const uint32_t* __restrict__ unordered, const int* __restrict__ key, int n, const float* __restrict__ pts,
                                const float* __restrict__ bounds, int max_cells, const uint32_t* __restrict__ start, uint32_t* __restrict__ ordered) {
    const int s = blockIdx.x * blockDim.x + threadIdx.x;
    if (s >= slots) return;
    const uint32_t v = unordered[s];
    int seg;
    if (key) seg = key[v];
    else {
        const KnnGrid g = make_grid(bounds, n, max_cells);
        const int3 c = cell_of(g, pts[3 * (size_t)v], pts[3 * (size_t)v + 1], pts[3 * (size_t)v + 2]);
        seg = (c.z * g.gy + c.y) * g.gx + c.x;
    }
    const uint32_t lo = start[seg], hi = start[seg + 1];
    uint32_t rank = 0;
    for (uint32_t k = lo; k < hi; ++k) rank += unordered[k] < v ? 1u : 0u;
    ordered[lo + rank] = v;
}

template <int K>
__device__ __forceinline__ void knn_insert_k(float d, uint32_t j, float (&bd)[K], uint32_t (&bj)[K]) {
    if (!(d < bd[K - 1] || (d == bd[K - 1] && j < bj[K - 1]))) return;
    bd[K - 1] = d; bj[K - 1] = j;
#pragma unroll
    for (int s = K - 1; s > 0; --s) {
        const bool up = bd[s] < bd[s - 1] || (bd[s] == bd[s - 1] && bj[s] < bj[s - 1]);
        const float td = bd[s - 1]; const uint32_t tj = bj[s - 1];
        bd[s - 1] = up ? bd[s] : td; bj[s - 1] = up ? bj[s] : tj;
        bd[s] = up ? td : bd[s]; bj[s] = up ? tj : bj[s];
    }
}

// thread t serves point order[t]: neighbouring threads search the same cells
template <int K>
__global__ void __launch_bounds__(256) k_knn_search_k(int n, const float* __restrict__ pts, const float* __restrict__ bounds, int max_cells,
                                                      const uint32_t* __restrict__ start, const uint32_t* __restrict__ order, int* __restrict__ nn_ix) {
    const int t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= n) return;
    const uint32_t i = order[t];
    const KnnGrid g = make_grid(bounds, n, max_cells);
    const float px = pts[3 * (size_t)i], py = pts[3 * (size_t)i + 1], pz = pts[3 * (size_t)i + 2];
    const int3 c = cell_of(g, px, py, pz);
    float bd[K]; uint32_t bj[K];
#pragma unroll
    for (int k = 0; k < K; ++k) { bd[k] = 3.0e38f; bj[k] = 0xffffffffu; }
    const int rmax = max(g.gx, max(g.gy, g.gz));
    for (int r = 0; r <= rmax; ++r) {
        for (int dz = -r; dz <= r; ++dz) {
            const int z = c.z + dz; if (z < 0 || z >= g.gz) continue;
            for (int dy = -r; dy <= r; ++dy) {
                const int y = c.y + dy; if (y < 0 || y >= g.gy) continue;
                const bool face = (dz == -r || dz == r || dy == -r || dy == r);
                const int step = face ? 1 : max(2 * r, 1);
                for (int dx = -r; dx <= r; dx += step) {
                    const int x = c.x + dx; if (x < 0 || x >= g.gx) continue;
                    const int cell = (z * g.gy + y) * g.gx + x;
                    for (uint32_t k = start[cell]; k < start[cell + 1]; ++k) {
                        const uint32_t j = order[k];
                        const float ddx = pts[3 * (size_t)j] - px, ddy = pts[3 * (size_t)j + 1] - py, ddz = pts[3 * (size_t)j + 2] - pz;
                        knn_insert_k<K>(ddx * ddx + ddy * ddy + ddz * ddz, j, bd, bj);
                    }
                }
            }
        }
        const float safe = r * g.cell;   // an unvisited point is at least this far: strictly below, so that one at exactly the
        if (bd[K - 1] < safe * safe) break;   // K-th distance with a lower index is still met
    }
    // fewer than K comparable points (non-finite coordinates): the point stands in for the missing ones, so that every
    // index can be gathered
#pragma unroll
    for (int k = 0; k < K; ++k) nn_ix[(size_t)i * K + k] = bj[k] < (uint32_t)n ? (int)bj[k] : (int)i;
}

__global__ void k_rev_count(int edges, const int* __restrict__ nn_ix, uint32_t* __restrict__ count) {
    const int e = blockIdx.x * blockDim.x + threadIdx.x;
    if (e < edges) atomicAdd(&count[nn_ix[e]], 1u);
}

__global__ void __launch_bounds__(kScanBlock) k_rev_scan(int n, const uint32_t* __restrict__ count, uint32_t* __restrict__ start, uint32_t* __restrict__ cursor) {
    scan_counts(n, count, start, cursor);
}

__global__ void k_rev_fill(int edges, const int* __restrict__ nn_ix, const uint32_t* __restrict__ start, uint32_t* __restrict__ cursor,
                           uint32_t* __restrict__ unordered) {
    const int e = blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= edges) return;
    const int t = nn_ix[e];
    unordered[start[t] + atomicAdd(&cursor[t], 1u)] = (uint32_t)e;
}

static size_t knn_graph_workspace_bytes(int n, int k) {
    return n <= 0 || k < kKnnMinK || k > kKnnMaxK ? 0 : carve_knn(nullptr, n, k, nullptr);
}

template <int K>
static void launch_search_k(int nb, int n, const float* pts, const float* bounds, int max_cells, const uint32_t* start, const uint32_t* order,
                            int* nn_ix, hipStream_t st) {
    hipLaunchKernelGGL(k_knn_search_k<K>, dim3(nb), dim3(256), 0, st, n, pts, bounds, max_cells, start, order, nn_ix);
}

static void launch_knn_graph(int n, int k, const float* pts, int* nn_ix, uint32_t* order, uint32_t* rev_start, uint32_t* rev_edges, void* workspace,
                             hipStream_t st) {
    KnnCarve c;
    carve_knn(workspace, n, k, &c);
    const int nb = (n + 255) / 256, edges = n * k, eb = (edges + 255) / 256;
    hipMemsetAsync(c.count, 0, sizeof(uint32_t) * ((size_t)c.max_cells + 1), st);
    hipLaunchKernelGGL(k_knn_bounds, dim3(1), dim3(1024), 0, st, n, pts, c.bounds);
    hipLaunchKernelGGL(k_knn_count, dim3(nb), dim3(256), 0, st, n, pts, c.bounds, c.max_cells, c.count);
    hipLaunchKernelGGL(k_knn_scan, dim3(1), dim3(kScanBlock), 0, st, c.bounds, n, c.max_cells, c.count, c.start, c.cursor);
    hipLaunchKernelGGL(k_knn_fill, dim3(nb), dim3(256), 0, st, n, pts, c.bounds, c.max_cells, c.start, c.cursor, c.unordered);
    hipLaunchKernelGGL(k_rank_segments, dim3(nb), dim3(256), 0, st, n, c.unordered, (const int*)nullptr, n, pts, c.bounds, c.max_cells, c.start, order);
    switch (k) {
        case 2: launch_search_k<2>(nb, n, pts, c.bounds, c.max_cells, c.start, order, nn_ix, st); break;
        case 3: launch_search_k<3>(nb, n, pts, c.bounds, c.max_cells, c.start, order, nn_ix, st); break;
        case 4: launch_search_k<4>(nb, n, pts, c.bounds, c.max_cells, c.start, order, nn_ix, st); break;
        case 5: launch_search_k<5>(nb, n, pts, c.bounds, c.max_cells, c.start, order, nn_ix, st); break;
        case 6: launch_search_k<6>(nb, n, pts, c.bounds, c.max_cells, c.start, order, nn_ix, st); break;
        case 7: launch_search_k<7>(nb, n, pts, c.bounds, c.max_cells, c.start, order, nn_ix, st); break;
        default: launch_search_k<8>(nb, n, pts, c.bounds, c.max_cells, c.start, order, nn_ix, st); break;
    }
    // reverse adjacency: per target, the edges that end there, by edge id
    hipMemsetAsync(c.count, 0, sizeof(uint32_t) * ((size_t)n + 1), st);
    hipLaunchKernelGGL(k_rev_count, dim3(eb), dim3(256), 0, st, edges, nn_ix, c.count);
    hipLaunchKernelGGL(k_rev_scan, dim3(1), dim3(kScanBlock), 0, st, n, c.count, rev_start, c.cursor);
    hipLaunchKernelGGL(k_rev_fill, dim3(eb), dim3(256), 0, st, edges, nn_ix, rev_start, c.cursor, c.unordered_edges);
    hipLaunchKernelGGL(k_rank_segments, dim3(eb), dim3(256), 0, st, edges, c.unordered_edges, nn_ix, n, pts, c.bounds, c.max_cells, rev_start, rev_edges);
}

}  // namespace sr

// ---- C entry points (include/splatraster.h): what is refused on the host, then the launchers above --------------------
using sr::fail; using sr::check_hip;

extern "C" {

size_t sr_knn_workspace_bytes(int n) { return sr::carve_knn(nullptr, n, 0, nullptr); }

int sr_knn3_mean_dist2(int n, const float* points, float* mean_dist2, void* workspace, void* hip_stream) {
    if (n < 0 || (n > 0 && (!points || !mean_dist2 || !workspace))) return fail("bad arguments to sr_knn3_mean_dist2");
    sr::launch_knn3(n, points, mean_dist2, workspace, static_cast<hipStream_t>(hip_stream));
    return check_hip(hipGetLastError(), "knn3");
}

size_t sr_knn_graph_workspace_bytes(int n, int k) { return sr::knn_graph_workspace_bytes(n, k); }

int sr_knn_graph(int n, int k, const float* points, int* nn_ix, unsigned* order, unsigned* rev_start, unsigned* rev_edges, void* workspace,
                 void* hip_stream) {
    if (n <= 0) return fail("bad arguments to sr_knn_graph: sizes must be positive");
    if (k < sr::kKnnMinK || k > sr::kKnnMaxK) return fail("bad arguments to sr_knn_graph: k must be 2 .. 8");
    if (n < k) return fail("bad arguments to sr_knn_graph: fewer points than neighbours (n < k)");
    if (n > 0x7fffffff / (3 * sr::kKnnMaxK)) return fail("too many points for sr_knn_graph");
    if (!points || !nn_ix || !order || !rev_start || !rev_edges || !workspace) return fail("null pointer in sr_knn_graph");
    sr::launch_knn_graph(n, k, points, nn_ix, order, rev_start, rev_edges, workspace, static_cast<hipStream_t>(hip_stream));
    return check_hip(hipGetLastError(), "knn_graph");
}

}  // extern "C"
