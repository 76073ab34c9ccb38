// The view-dependent colour head (include/splatraster.h: sr_view_color_*): for every view v of a step,
//   colour[v, n] = sigmoid( W [feature[n] | r_v[n]] + b ),  r_v[n] = normalize(means3D[n] - campos[v])  or  dirs[v, n],
// all views in one launch, and the whole backward in one more.
//
// Mapping.  A workgroup owns 256 consecutive points, one per thread, on every device: no sum depends on the grid.  W [3][F + 3]
// and b sit in LDS (at most 3 x 259 floats, every read a broadcast), the camera centres beside them.  The feature rows (512 bytes
// at the reference's width) are read ONCE for all views, 16 columns of the workgroup's 256 rows at a time through the LDS tile of
// point_tile.h: four lanes load the four 16-byte vectors of one row's 64-byte piece, so a wavefront's load instruction covers 16
// whole 64-byte pieces instead of 64 strided rows, and each thread reads its own row's piece back.  dL/dfeature leaves the same
// way in the other direction, written once for all views.
//
// Arithmetic.  A thread owns its point's whole sum, so there are no partial sums between lanes to combine:
//   a[c] = b[c] + sum over f = 0, 1, ... of feature[f] W[c][f]                        (the view-independent part)
//   z[v, c] = ((a[c] + W[c][F] r_v[0]) + W[c][F + 1] r_v[1]) + W[c][F + 2] r_v[2]
// one chain of double FMAs in exactly that order (the product of two floats is exact in double).  The direction, the sigmoid and
// their backward are doubles with IEEE sqrt and division; every stored value is rounded to fp32 once.  `saved` holds a as doubles,
// [3][N] (24 bytes per point whatever the number of views; a wavefront's accesses to one component are contiguous): the backward
// re-derives r_v and z[v] from it with the same three FMAs instead of a second pass over W feature.  The only sums over points
// are the nine entries of dW[:, F:] and the three of db, one block_sum (reduce.h) each per workgroup, left in `workspace` as
// doubles for the caller to add in workgroup order (dW[:, :F] is sr_mlp_weight_grad's).  No atomics, no host wait.
#include "host_api.h"
#include "point_tile.h"
#include "reduce.h"

namespace sr {

namespace {

struct ViewColorK {
    int mode, width, n_views;
    long long n;
    const float* feature; const float* means; const float* cam_or_dirs; const float* weight; const float* bias;
    float* colours; double* saved;
    const float* g_colours;
    float* d_feature; float* d_pos; float* d_zsum; double* partial;
};

struct Dir { double x, y, z, inv_len; };

constexpr int kViewPartials = 12;        // doubles per workgroup in `workspace`: dW[:, F:] row-major (9), then db (3)

// W [3][width + 3] as it lies in memory, then the camera centres as doubles
__device__ __forceinline__ void stage_head(const ViewColorK& P, float* s_w, double* s_cam) {
    const int row = P.width + 3;
    for (int i = (int)threadIdx.x; i < 3 * row; i += kBlock) s_w[i] = P.weight[i];
    if (P.mode == SR_VIEW_FROM_CAMERAS && (int)threadIdx.x < 3 * P.n_views) s_cam[threadIdx.x] = (double)P.cam_or_dirs[threadIdx.x];
}

// the unit direction of view v at this point (inv_len = 1 / |p - c_v|, used by the backward of the normalisation; 1 for given dirs)
__device__ __forceinline__ Dir view_dir(const ViewColorK& P, const double* s_cam, int v, long long point, double px, double py, double pz) {
    Dir r;
    if (P.mode == SR_VIEW_FROM_CAMERAS) {
        const double dx = px - s_cam[3 * v], dy = py - s_cam[3 * v + 1], dz = pz - s_cam[3 * v + 2];
        const double len = sqrt(fma(dz, dz, fma(dy, dy, dx * dx)));
        r.x = dx / len; r.y = dy / len; r.z = dz / len; r.inv_len = 1.0 / len;
    } else {
        const float* d = P.cam_or_dirs + 3 * ((size_t)v * (size_t)P.n + (size_t)point);
        r.x = (double)d[0]; r.y = (double)d[1]; r.z = (double)d[2]; r.inv_len = 1.0;
    }
    return r;
}

// z[c] of one view from the view-independent part: the three direction columns close the chain, in column order
__device__ __forceinline__ double view_z(const float* s_w, int width, int c, double a, const Dir& r) {
    const float* w = s_w + c * (width + 3) + width;
    return fma((double)w[2], r.z, fma((double)w[1], r.y, fma((double)w[0], r.x, a)));
}

__device__ __forceinline__ double sigmoid(double z) { return 1.0 / (1.0 + exp(-z)); }

__global__ void __launch_bounds__(kBlock) k_view_color_forward(const ViewColorK P) {
    extern __shared__ __align__(16) float s_dyn[];
    __shared__ double s_cam[3 * SR_VIEW_MAX_VIEWS];
    float* s_tile = s_dyn;                                // [256][20]
    float* s_w = s_dyn + kBlock * kTileRow;               // [3][width + 3]
    const int tid = (int)threadIdx.x, row = P.width + 3;
    const long long first = (long long)blockIdx.x * kBlock, point = first + tid;
    stage_head(P, s_w, s_cam);
    __syncthreads();

    double a0 = (double)P.bias[0], a1 = (double)P.bias[1], a2 = (double)P.bias[2];
    for (int c0 = 0; c0 < P.width; c0 += kTileCols) {
        tile_load(P.feature, first, P.n, P.width, c0, s_tile);
        __syncthreads();
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            if (c0 + 4 * q < P.width) {                   // the same in every thread
                const float4 h = *reinterpret_cast<const float4*>(s_tile + tid * kTileRow + 4 * q);
                const double hv[4] = {h.x, h.y, h.z, h.w};
                const float* w = s_w + c0 + 4 * q;
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    a0 = fma(hv[j], (double)w[j], a0);
                    a1 = fma(hv[j], (double)w[row + j], a1);
                    a2 = fma(hv[j], (double)w[2 * row + j], a2);
                }
            }
        }
        __syncthreads();
    }
    if (point >= P.n) return;
    if (P.saved) {
        P.saved[point] = a0;
        P.saved[(size_t)P.n + point] = a1;
        P.saved[2 * (size_t)P.n + point] = a2;
    }
    double px = 0.0, py = 0.0, pz = 0.0;
    if (P.mode == SR_VIEW_FROM_CAMERAS) { px = (double)P.means[3 * point]; py = (double)P.means[3 * point + 1]; pz = (double)P.means[3 * point + 2]; }
    for (int v = 0; v < P.n_views; ++v) {
        const Dir r = view_dir(P, s_cam, v, point, px, py, pz);
        float* out = P.colours + 3 * ((size_t)v * (size_t)P.n + (size_t)point);
        out[0] = (float)sigmoid(view_z(s_w, P.width, 0, a0, r));
        out[1] = (float)sigmoid(view_z(s_w, P.width, 1, a1, r));
        out[2] = (float)sigmoid(view_z(s_w, P.width, 2, a2, r));
    }
}

__global__ void __launch_bounds__(kBlock) k_view_color_backward(const ViewColorK P) {
    extern __shared__ __align__(16) float s_dyn[];
    __shared__ double s_cam[3 * SR_VIEW_MAX_VIEWS];
    __shared__ double s_red[kBlock / kWave];
    float* s_tile = s_dyn;
    float* s_w = s_dyn + kBlock * kTileRow;
    const int tid = (int)threadIdx.x, row = P.width + 3;
    const long long first = (long long)blockIdx.x * kBlock, point = first + tid;
    stage_head(P, s_w, s_cam);
    __syncthreads();

    double gsum[3] = {0.0, 0.0, 0.0};                      // sum over the views of dL/dz, in view order
    double dwd[9] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};      // this point's share of dW[:, F:], [c][k]
    if (point < P.n) {
        const double a[3] = {P.saved[point], P.saved[(size_t)P.n + point], P.saved[2 * (size_t)P.n + point]};
        double px = 0.0, py = 0.0, pz = 0.0;
        if (P.mode == SR_VIEW_FROM_CAMERAS) { px = (double)P.means[3 * point]; py = (double)P.means[3 * point + 1]; pz = (double)P.means[3 * point + 2]; }
        double dp[3] = {0.0, 0.0, 0.0};
        for (int v = 0; v < P.n_views; ++v) {
            const Dir r = view_dir(P, s_cam, v, point, px, py, pz);
            const size_t at = 3 * ((size_t)v * (size_t)P.n + (size_t)point);
            const double rv[3] = {r.x, r.y, r.z};
            double g[3];
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                const double s = sigmoid(view_z(s_w, P.width, c, a[c], r));
                g[c] = (double)P.g_colours[at + c] * (s * (1.0 - s));
                gsum[c] += g[c];
#pragma unroll
                for (int k = 0; k < 3; ++k) dwd[3 * c + k] = fma(g[c], rv[k], dwd[3 * c + k]);
            }
            if (P.d_pos) {
                double t[3];                               // W[:, F:]^T g: the gradient at the direction
#pragma unroll
                for (int k = 0; k < 3; ++k)
                    t[k] = fma((double)s_w[2 * row + P.width + k], g[2], fma((double)s_w[row + P.width + k], g[1], (double)s_w[P.width + k] * g[0]));
                if (P.mode == SR_VIEW_FROM_CAMERAS) {      // through r = d / |d|: (I - r r^T) t / |d|
                    const double rt = fma(r.z, t[2], fma(r.y, t[1], r.x * t[0]));
#pragma unroll
                    for (int k = 0; k < 3; ++k) dp[k] += (t[k] - rv[k] * rt) * r.inv_len;
                } else {
                    P.d_pos[at] = (float)t[0]; P.d_pos[at + 1] = (float)t[1]; P.d_pos[at + 2] = (float)t[2];
                }
            }
        }
        if (P.d_pos && P.mode == SR_VIEW_FROM_CAMERAS) {
            P.d_pos[3 * point] = (float)dp[0]; P.d_pos[3 * point + 1] = (float)dp[1]; P.d_pos[3 * point + 2] = (float)dp[2];
        }
        *reinterpret_cast<float4*>(P.d_zsum + 4 * (size_t)point) = make_float4((float)gsum[0], (float)gsum[1], (float)gsum[2], 0.f);
    }
    // the workgroup's share of dW[:, F:] (nine sums) and of db (three): [kViewPartials] doubles per workgroup
#pragma unroll
    for (int i = 0; i < kViewPartials; ++i) {
        const double sum = block_sum(i < 9 ? dwd[i] : gsum[i - 9], s_red);
        if (tid == 0) P.partial[(size_t)blockIdx.x * kViewPartials + i] = sum;
    }
    if (!P.d_feature) return;
    for (int c0 = 0; c0 < P.width; c0 += kTileCols) {
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            if (c0 + 4 * q < P.width) {
                const float* w = s_w + c0 + 4 * q;
                float o[4];
#pragma unroll
                for (int j = 0; j < 4; ++j)
                    o[j] = (float)fma(gsum[2], (double)w[2 * row + j], fma(gsum[1], (double)w[row + j], gsum[0] * (double)w[j]));
                *reinterpret_cast<float4*>(s_tile + tid * kTileRow + 4 * q) = make_float4(o[0], o[1], o[2], o[3]);
            }
        }
        __syncthreads();
        tile_store(P.d_feature, first, P.n, P.width, c0, s_tile);
        __syncthreads();
    }
}

template <bool kBackward>
void view_launch(const ViewColorK& k, hipStream_t st) {
    const size_t lds = ((size_t)kBlock * kTileRow + 3 * (size_t)(k.width + 3)) * sizeof(float);      // 20 KiB + at most 3108 bytes
    const unsigned blocks = (unsigned)((k.n + kBlock - 1) / kBlock);
    if (kBackward) hipLaunchKernelGGL(k_view_color_backward, dim3(blocks), dim3(kBlock), lds, st, k);
    else hipLaunchKernelGGL(k_view_color_forward, dim3(blocks), dim3(kBlock), lds, st, k);
}

const char* view_color_shape_error(int mode, long long n_points, int width, int n_views) {
    if (mode != SR_VIEW_FROM_CAMERAS && mode != SR_VIEW_DIRS_GIVEN) return "unknown mode";
    if (width < 4 || (width & 3) || width > SR_VIEW_MAX_WIDTH) return "width must be a multiple of 4 in 4 .. SR_VIEW_MAX_WIDTH";
    if (n_views < 1 || n_views > SR_VIEW_MAX_VIEWS) return "n_views must be in 1 .. SR_VIEW_MAX_VIEWS";
    if (n_points < 0 || n_points >= (1ll << 31)) return "n_points must be in 0 .. 2^31 - 1";
    return nullptr;
}

size_t view_color_saved_bytes(long long n) { return (3 * (size_t)n * sizeof(double) + 255) / 256 * 256 + 256; }

size_t view_color_workspace_bytes(long long n) {
    return ((size_t)((n + kBlock - 1) / kBlock) * kViewPartials * sizeof(double) + 255) / 256 * 256 + 256;
}

void launch_view_color_forward(int mode, long long n, int width, int n_views, const float* feature, const float* means, const float* cam_or_dirs,
                               const float* weight, const float* bias, float* colours, void* saved, hipStream_t st) {
    ViewColorK k{};
    k.mode = mode; k.n = n; k.width = width; k.n_views = n_views;
    k.feature = feature; k.means = means; k.cam_or_dirs = cam_or_dirs; k.weight = weight; k.bias = bias;
    k.colours = colours; k.saved = static_cast<double*>(saved);
    view_launch<false>(k, st);
}

void launch_view_color_backward(int mode, long long n, int width, int n_views, const float* means, const float* cam_or_dirs, const float* weight,
                                const void* saved, const float* g_colours, float* d_feature, float* d_pos, float* d_zsum, void* workspace,
                                hipStream_t st) {
    ViewColorK k{};
    k.mode = mode; k.n = n; k.width = width; k.n_views = n_views;
    k.means = means; k.cam_or_dirs = cam_or_dirs; k.weight = weight; k.saved = const_cast<double*>(static_cast<const double*>(saved));
    k.g_colours = g_colours; k.d_feature = d_feature; k.d_pos = d_pos; k.d_zsum = d_zsum; k.partial = static_cast<double*>(workspace);
    view_launch<true>(k, st);
}

}  // namespace

}  // namespace sr

// ---- C entry points (include/splatraster.h): what is refused on the host, then the launchers above --------------------
using sr::fail; using sr::check_hip; using sr::any_unaligned4; using sr::StageTimer;

extern "C" {

size_t sr_view_color_saved_bytes(long long n_points, int width, int n_views) {
    return sr::view_color_shape_error(SR_VIEW_FROM_CAMERAS, n_points, width, n_views) ? 0 : sr::view_color_saved_bytes(n_points);
}

size_t sr_view_color_workspace_bytes(long long n_points, int width, int n_views) {
    return sr::view_color_shape_error(SR_VIEW_FROM_CAMERAS, n_points, width, n_views) ? 0 : sr::view_color_workspace_bytes(n_points);
}

int sr_view_color_forward(int mode, long long n_points, int width, int n_views, const float* feature, const float* means3D,
                          const float* campos_or_dirs, const float* weight, const float* bias, float* colours, void* saved,
                          void* hip_stream) {
    if (const char* why = sr::view_color_shape_error(mode, n_points, width, n_views)) return fail(std::string("sr_view_color_forward: ") + why);
    if (n_points == 0) return 0;
    if (!feature || !campos_or_dirs || !weight || !bias || !colours) return fail("null pointer in sr_view_color_forward");
    if (mode == SR_VIEW_FROM_CAMERAS && !means3D) return fail("null pointer in sr_view_color_forward: the camera mode reads means3D");
    if (((reinterpret_cast<uintptr_t>(feature) | reinterpret_cast<uintptr_t>(weight)) & 15u) || (reinterpret_cast<uintptr_t>(saved) & 7u) ||
        any_unaligned4(means3D, campos_or_dirs, bias, colours))
        return fail("sr_view_color_forward: feature and weight must be 16-byte aligned, saved 8-byte, the others 4-byte");
    hipStream_t st = static_cast<hipStream_t>(hip_stream);
    { StageTimer t_(0, st); sr::launch_view_color_forward(mode, n_points, width, n_views, feature, means3D, campos_or_dirs, weight, bias, colours, saved, st); }
    return check_hip(hipGetLastError(), "view_color_forward");
}

int sr_view_color_backward(int mode, long long n_points, int width, int n_views, const float* means3D, const float* campos_or_dirs,
                           const float* weight, const void* saved, const float* dL_dcolours, float* dL_dfeature, float* dL_dpos,
                           float* dL_dzsum, void* workspace, void* hip_stream) {
    if (const char* why = sr::view_color_shape_error(mode, n_points, width, n_views)) return fail(std::string("sr_view_color_backward: ") + why);
    if (n_points == 0) return 0;
    if (!campos_or_dirs || !weight || !saved || !dL_dcolours || !dL_dzsum || !workspace) return fail("null pointer in sr_view_color_backward");
    if (mode == SR_VIEW_FROM_CAMERAS && !means3D) return fail("null pointer in sr_view_color_backward: the camera mode reads means3D");
    if (((reinterpret_cast<uintptr_t>(weight) | reinterpret_cast<uintptr_t>(dL_dfeature) | reinterpret_cast<uintptr_t>(dL_dzsum)) & 15u) ||
        ((reinterpret_cast<uintptr_t>(saved) | reinterpret_cast<uintptr_t>(workspace)) & 7u) || any_unaligned4(means3D, campos_or_dirs, dL_dcolours, dL_dpos))
        return fail("sr_view_color_backward: weight, dL_dfeature and dL_dzsum must be 16-byte aligned, saved and workspace 8-byte, the others 4-byte");
    hipStream_t st = static_cast<hipStream_t>(hip_stream);
    { StageTimer t_(6, st); sr::launch_view_color_backward(mode, n_points, width, n_views, means3D, campos_or_dirs, weight, saved, dL_dcolours, dL_dfeature,
                                                           dL_dpos, dL_dzsum, workspace, st); }
    return check_hip(hipGetLastError(), "view_color_backward");
}

}  // extern "C"
