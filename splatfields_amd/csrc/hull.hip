// Visual-hull initialisation on the device (the one piece of the dataset readers that is arithmetic).
//
// Restates the hull test of reference scene/dataset_readers.py: :1385-1417 (`visual_hull_samples`), :1419-1458
// (`visual_hull_samples_list`), :605-644 (the Blender `hull` branch of `readNerfSyntheticInfo`) and :544-588 (its `load`
// branch).  The reference projects a G^3 grid into every training view on the host (a [V, G^3, 4] float64 temporary for
// the first two, a per-camera loop over a float32 [G^3, 4] matrix for the Blender branches) and keeps the voxels whose nearest
// pixel lies in the mask of every view.  Here:
//
//   carve    one lane per voxel (or per explicit point): the lane walks the V views and leaves the loop once it is carved;
//            the wavefront's survivors become one 64-bit word (__ballot), the workgroup's count one uint32;
//   scan     one workgroup turns the workgroup counts into exclusive offsets, in index order, and writes the total;
//   gather   every survivor's rank = its workgroup's offset + the bits in front of it: indices and float32 coordinates are
//            written in grid order, up to a caller-supplied capacity.
//
// No atomics anywhere: the same inputs give the same bytes from call to call.
//
// Arithmetic: double throughout, in the reference's order of operations, with floating-point contraction switched off in the
// functions below (a fused multiply-add rounds once where numpy rounds twice).  The result then equals a float64 evaluation on
// the host except for voxels whose pixel coordinate lies within ~1e-13 px of a rounding boundary (k + 1/2), where the order of
// the four-term dot product inside the host's BLAS can decide.  About 20 fp64 operations per voxel and view: the pass is
// bound by its byte gathers, not by the fp64 rate.
#include "host_api.h"
#include "ordered_scan.h"

namespace sr {

namespace {

// does view `w` keep the point (x, y, z)?
__device__ __forceinline__ bool hull_view_keeps(const SrHullView& w, const uint8_t* __restrict__ masks, double x, double y, double z) {
#pragma clang fp contract(off)
    const double h0 = w.m[0] * x + w.m[1] * y + w.m[2] * z + w.m[3];
    const double h1 = w.m[4] * x + w.m[5] * y + w.m[6] * z + w.m[7];
    const double h2 = w.m[8] * x + w.m[9] * y + w.m[10] * z + w.m[11];
    const double u = h0 / h2, v = h1 / h2;            // no sign test on h2: the reference has none
    const double Wd = (double)w.width, Hd = (double)w.height;
    double px, py, un, vn;
    if (w.convention == SR_HULL_KRT) {
        // the reference normalises for grid_sample, which un-normalises again (align_corners=True): the round trip is kept
        un = 2.0 * (u / (Wd - 1.0)) - 1.0;
        vn = 2.0 * (v / (Hd - 1.0)) - 1.0;
        px = ((un + 1.0) / 2.0) * (Wd - 1.0);
        py = ((vn + 1.0) / 2.0) * (Hd - 1.0);
    } else {
        un = u; vn = v;                                // already normalised device coordinates
        px = ((u + 1.0) * Wd - 1.0) * 0.5;             // ndc2Pix
        py = ((v + 1.0) * Hd - 1.0) * 0.5;
    }
    // non-finite: carved under both policies (NaN fails every comparison below anyway; infinities are named here)
    if (!(fabs(px) <= 1.7976931348623157e308) || !(fabs(py) <= 1.7976931348623157e308)) return false;
    if (w.outside == SR_HULL_OUTSIDE_KEEP && (un < -1.0 || un > 1.0 || vn < -1.0 || vn > 1.0)) return true;
    const double rx = rint(px), ry = rint(py);         // nearest pixel, halves to even
    if (!(rx >= 0.0 && rx <= Wd - 1.0 && ry >= 0.0 && ry <= Hd - 1.0)) return false;
    const long long at = w.mask_offset + (long long)ry * (long long)w.width + (long long)rx;
    return masks[at] != 0;
}

// item -> its position: the voxel with linear index i = (iy G + ix) G + iz sits at (gx[ix], gy[iy], gz[iz]) -- the order of
// np.meshgrid(g, g, g) (default indexing) flattened --, or row i of the point list widened to double
struct HullItems {
    const double* grid;      // [3][G] (x, y, z tables) or NULL
    int G;
    const void* points;      // [n, 3] float32 / float64 or NULL
    int point_is_double;
    long long n;
};

__device__ __forceinline__ void hull_position(const HullItems& it, long long i, double& x, double& y, double& z) {
    if (it.grid) {
        const long long G = it.G;
        const int iz = (int)(i % G), ix = (int)((i / G) % G), iy = (int)(i / (G * G));
        x = it.grid[ix]; y = it.grid[G + iy]; z = it.grid[2 * G + iz];
    } else if (it.point_is_double) {
        const double* p = static_cast<const double*>(it.points) + 3 * i;
        x = p[0]; y = p[1]; z = p[2];
    } else {
        const float* p = static_cast<const float*>(it.points) + 3 * i;
        x = (double)p[0]; y = (double)p[1]; z = (double)p[2];
    }
}

__global__ void __launch_bounds__(kBlock) k_hull_carve(const HullItems it, int n_views, const SrHullView* __restrict__ views,
                                                       const uint8_t* __restrict__ masks, unsigned long long* __restrict__ words,
                                                       uint32_t* __restrict__ block_counts) {
    const long long i = (long long)blockIdx.x * kBlock + threadIdx.x;
    bool alive = i < it.n;
    if (alive) {
        double x, y, z;
        hull_position(it, i, x, y, z);
        for (int v = 0; v < n_views && alive; ++v) alive = hull_view_keeps(views[v], masks, x, y, z);   // views[v]: the same record for every lane
    }
    compaction_mark(alive, i, words, block_counts);      // every lane of the workgroup arrives here: lanes past n vote 0
}

// exclusive prefix over the workgroup counts, in index order, in place; the total goes to `total` (workspace) and `count_out`
__global__ void __launch_bounds__(kScanBlock) k_hull_scan(long long blocks, uint32_t* __restrict__ block_counts,
                                                          uint32_t* __restrict__ total, int* __restrict__ count_out) {
    const uint32_t carry = ordered_scan(blocks, [&](long long j) { return block_counts[j]; },
                                        [&](long long j, uint32_t offset) { block_counts[j] = offset; });
    if (threadIdx.x == 0) { *total = carry; if (count_out) *count_out = (int)carry; }
}

__global__ void __launch_bounds__(kBlock) k_hull_gather(const HullItems it, const unsigned long long* __restrict__ words,
                                                        const uint32_t* __restrict__ block_offsets, long long capacity,
                                                        int* __restrict__ indices_out, float* __restrict__ points_out) {
    const long long i = (long long)blockIdx.x * kBlock + threadIdx.x;
    if (i >= it.n) return;
    long long rank;
    if (!compaction_rank(words, block_offsets, rank) || rank >= capacity) return;            // carved, or past an ordered prefix when the caller's buffers are short
    if (indices_out) indices_out[rank] = (int)i;
    if (points_out) {
        double x, y, z;
        hull_position(it, i, x, y, z);
        points_out[3 * rank + 0] = (float)x; points_out[3 * rank + 1] = (float)y; points_out[3 * rank + 2] = (float)z;
    }
}

struct HullCarve { SrHullView* views; unsigned long long* words; uint32_t* counts; uint32_t* total; };

// view table [kHullMaxViews] | survivor words [4 per workgroup] | workgroup counts / offsets | total
size_t carve_hull(void* base, long long n, HullCarve* out) {
    Carver c{static_cast<char*>(base), 0};
    const size_t blocks = (size_t)(((n > 0 ? n : 1) + kBlock - 1) / kBlock);
    HullCarve t;
    t.views = c.take<SrHullView>(SR_HULL_MAX_VIEWS);
    t.words = c.take<unsigned long long>(blocks * (kBlock / kWave));
    t.counts = c.take<uint32_t>(blocks);
    t.total = c.take<uint32_t>(1);
    if (out) *out = t;
    return align_up(c.off, 256);
}

size_t hull_workspace_bytes(long long n) { return carve_hull(nullptr, n, nullptr); }

hipError_t launch_hull_carve(int n_views, const SrHullView* host_views, const uint8_t* masks, const double* grid, int G, const void* points,
                             long long n, int point_is_double, void* workspace, int* count_out, hipStream_t st) {
    HullCarve c;
    carve_hull(workspace, n, &c);
    // the table travels through the stream in front of the kernel that reads it (pageable source: staged before the call returns)
    const hipError_t e = hipMemcpyAsync(c.views, host_views, sizeof(SrHullView) * (size_t)n_views, hipMemcpyHostToDevice, st);
    if (e != hipSuccess) return e;
    const HullItems it{grid, G, points, point_is_double, n};
    const long long blocks = (n + kBlock - 1) / kBlock;
    if (blocks > 0)
        hipLaunchKernelGGL(k_hull_carve, dim3((unsigned)blocks), dim3(kBlock), 0, st, it, n_views, c.views, masks, c.words, c.counts);
    hipLaunchKernelGGL(k_hull_scan, dim3(1), dim3(kScanBlock), 0, st, blocks, c.counts, c.total, count_out);
    return hipSuccess;
}

void launch_hull_gather(const double* grid, int G, const void* points, long long n, int point_is_double, const void* workspace,
                        long long capacity, int* indices_out, float* points_out, hipStream_t st) {
    HullCarve c;
    carve_hull(const_cast<void*>(workspace), n, &c);
    const HullItems it{grid, G, points, point_is_double, n};
    const long long blocks = (n + kBlock - 1) / kBlock;
    if (blocks > 0 && capacity > 0)
        hipLaunchKernelGGL(k_hull_gather, dim3((unsigned)blocks), dim3(kBlock), 0, st, it, c.words, c.counts, capacity, indices_out, points_out);
}

}  // namespace

}  // namespace sr

// ---- C entry points (include/splatraster.h): what is refused on the host, then the launchers above --------------------
using sr::fail; using sr::check_hip;

extern "C" {

// items of a hull call: G^3 or n_points; -1 with the message set when the pair is not acceptable
static long long hull_items(const char* name, const double* grid, int G, const void* points, long long n_points) {
    if ((grid != nullptr) == (points != nullptr)) {
        fail(std::string(name) + ": exactly one of grid and points must be given");
        return -1;
    }
    if (grid) {
        if (G < 1) { fail(std::string(name) + ": G must be at least 1"); return -1; }
        if (G > 1290) { fail(std::string(name) + ": G^3 must not exceed 2^31 - 1 (G <= 1290)"); return -1; }
        return (long long)G * G * G;
    }
    if (n_points < 0 || n_points > 2147483647LL) { fail(std::string(name) + ": n_points must be in 0 .. 2^31 - 1"); return -1; }
    return n_points;
}

size_t sr_hull_workspace_bytes(long long n_items) { return n_items < 0 || n_items > 2147483647LL ? 0 : sr::hull_workspace_bytes(n_items); }

int sr_hull_carve(int n_views, const SrHullView* views, const unsigned char* masks, long long mask_bytes, const double* grid, int G,
                  const void* points, long long n_points, int point_is_double, void* workspace, int* count_out, void* hip_stream) {
    if (n_views <= 0 || n_views > SR_HULL_MAX_VIEWS) return fail("sr_hull_carve: n_views must be in 1 .. SR_HULL_MAX_VIEWS");
    if (!views || !masks || !workspace || !count_out) return fail("null pointer in sr_hull_carve");
    const long long n = hull_items("sr_hull_carve", grid, G, points, n_points);
    if (n < 0) return 1;
    for (int k = 0; k < n_views; ++k) {
        const SrHullView& w = views[k];
        const std::string at = "sr_hull_carve: view " + std::to_string(k);
        if (w.height < 1 || w.width < 1) return fail(at + ": H and W must be at least 1");
        if (w.convention != SR_HULL_KRT && w.convention != SR_HULL_NDC) return fail(at + ": unknown pixel-mapping convention");
        if (w.outside != SR_HULL_OUTSIDE_CARVE && w.outside != SR_HULL_OUTSIDE_KEEP) return fail(at + ": unknown outside policy");
        if (w.convention == SR_HULL_KRT && (w.height == 1 || w.width == 1))
            return fail(at + ": H or W of 1 divides by zero in the krt normalisation (W - 1)");
        if (w.mask_offset < 0 || w.mask_offset + (long long)w.height * w.width > mask_bytes)
            return fail(at + ": the mask does not fit into mask_bytes");
    }
    SR_TRY(check_hip(sr::launch_hull_carve(n_views, views, masks, grid, G, points, n, point_is_double != 0, workspace, count_out,
                                           static_cast<hipStream_t>(hip_stream)), "upload of the hull view table"));
    return check_hip(hipGetLastError(), "hull_carve");
}

int sr_hull_gather(const double* grid, int G, const void* points, long long n_points, int point_is_double, const void* workspace,
                   long long capacity, int* indices_out, float* points_out, void* hip_stream) {
    const long long n = hull_items("sr_hull_gather", grid, G, points, n_points);
    if (n < 0) return 1;
    if (capacity < 0) return fail("sr_hull_gather: capacity must not be negative");
    if (!workspace) return fail("null pointer in sr_hull_gather");
    if (n == 0 || capacity == 0 || (!indices_out && !points_out)) return 0;
    sr::launch_hull_gather(grid, G, points, n, point_is_double != 0, workspace, capacity, indices_out, points_out,
                           static_cast<hipStream_t>(hip_stream));
    return check_hip(hipGetLastError(), "hull_gather");
}

}  // extern "C"
