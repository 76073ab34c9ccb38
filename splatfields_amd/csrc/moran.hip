// Moran's I regulariser (DESIGN.md "Moran's I regulariser").
//
// Restates reference extract_geo.py:100-109 (`query_nn`), :111-138 (`morans_measure`) and :140-143 (`morans_loss`) as they
// are called by train.py:203-215.  For item p with K rows r_0 .. r_{K-1} (its K nearest points, itself included) and the
// K x K spatial weights
//
//   c_ab = 1 / |q_a - q_b|  where the distance exceeds eps, eps elsewhere and on the diagonal      (q_a = points[r_a])
//   S    = sum_ab c_ab
//
// a feature tensor X [rows, F] has, with x_a = X[r_a, f],
//
//   A_f = sum_ab c_ab x_a x_b,   D_f = sum_a x_a^2 + 1e-4,   m[p, f] = K A_f / (S D_f)
//   term = 1 - clamp(mean_{p, f} m, 0, 1)
//
// (the reference normalises c by S, sums the result to W = 1 and scales by K / W: the same value.)  The drop-in form is the
// same arithmetic with c read from a given weight [n, K, K] and the rows p K .. p K + K - 1.
//
// forward   16 lanes per item: every lane forms c and S, the lanes share the channels of each tensor (a row's channels are
//           neighbours in memory, so a row is read in 64-byte pieces).  One partial sum per workgroup and term.
// reduce    one workgroup adds the partial sums in a fixed order (double accumulators): total | terms | means.
// backward  k_moran_edges, the same walk: per edge (p, a) one row of d m / d x_a and one d / d q_a, stored, not added;
//           k_moran_collect, 16 lanes per target row: the sum over the edges that end there, in edge order, through the
//           reverse adjacency of the graph, times the upstream gradient read from device memory.  The clamp gate is read
//           from the means of the forward on the device.
//
// No floating-point atomics anywhere: values and gradients are bit-identical from call to call.
#include "host_api.h"
#include "reduce.h"
#include <type_traits>

namespace sr {

constexpr int kMoranMaxTensors = SR_MORAN_MAX_TENSORS;
// the feature tensors of one call: x[t] is [rows, width[t]]; dx[t] (backward) may be NULL; offset[] are the running widths,
// edge_offset[] the running widths of the tensors with a dx: only those have columns in the per-edge buffer
struct MoranTensors {
    int count, channels, edge_channels;
    const float* x[kMoranMaxTensors]; float* dx[kMoranMaxTensors];
    int width[kMoranMaxTensors], offset[kMoranMaxTensors], edge_offset[kMoranMaxTensors];
};
// where the K x K spatial weights of item p come from: `points` (c_ab from the distances of the K gathered positions) or
// `weight` [n, K, K] given; nn_ix NULL: item p's rows are p K .. p K + K - 1; order NULL: items in index order
struct MoranSource { int n, k; float eps; const float* points; const float* weight; const int* nn_ix; const uint32_t* order; };

namespace {

constexpr int kMoranLanes = 16;                       // lanes per item
constexpr int kMoranItems = kBlock / kMoranLanes;     // items per workgroup
constexpr float kMoranDenomEps = 1e-4f;               // extract_geo.py:136
constexpr int kMoranReduceBlock = 1024;

struct MoranCoef { float v[kMoranMaxTensors]; };      // -1 / (n F_t): d term_t / d m[p, f] inside the clamp (+: d mean_t)

// rows of item p, its weights c (full matrix), their sum; with WantGrad also the positions and 1/d^3 of the pairs whose
// weight depends on them
template <int K, bool WantGrad>
struct MoranItem {
    int row[K];
    float c[K][K];
    float S;
    float q[K][3];
    float w3[K][K];

    __device__ __forceinline__ void load(const MoranSource& s, int p) {
#pragma unroll
        for (int a = 0; a < K; ++a) row[a] = s.nn_ix ? s.nn_ix[(size_t)p * K + a] : p * K + a;
        if (s.points) {
#pragma unroll
            for (int a = 0; a < K; ++a)
#pragma unroll
                for (int d = 0; d < 3; ++d) q[a][d] = s.points[3 * (size_t)row[a] + d];
#pragma unroll
            for (int a = 0; a < K; ++a) {
                c[a][a] = s.eps;
                if (WantGrad) w3[a][a] = 0.0f;
#pragma unroll
                for (int b = a + 1; b < K; ++b) {
                    const float dx = q[a][0] - q[b][0], dy = q[a][1] - q[b][1], dz = q[a][2] - q[b][2];
                    const float dist = sqrtf(dx * dx + dy * dy + dz * dz);
                    const bool far = dist > s.eps;
                    const float w = far ? 1.0f / dist : s.eps;
                    c[a][b] = c[b][a] = w;
                    if (WantGrad) w3[a][b] = w3[b][a] = far ? w * w * w : 0.0f;
                }
            }
        } else {
#pragma unroll
            for (int a = 0; a < K; ++a)
#pragma unroll
                for (int b = 0; b < K; ++b) c[a][b] = s.weight[((size_t)p * K + a) * K + b];
        }
        S = 0.0f;
#pragma unroll
        for (int a = 0; a < K; ++a)
#pragma unroll
            for (int b = 0; b < K; ++b) S += c[a][b];
    }
};

// the K values of one channel; r_a = sum_b c_ab x_b
template <int K>
__device__ __forceinline__ void moran_channel(const float (&c)[K][K], const float (&x)[K], float (&r)[K], float& A, float& D) {
    A = 0.0f; D = kMoranDenomEps;
#pragma unroll
    for (int a = 0; a < K; ++a) {
        float t = 0.0f;
#pragma unroll
        for (int b = 0; b < K; ++b) t = fmaf(c[a][b], x[b], t);
        r[a] = t;
        A = fmaf(t, x[a], A);
        D = fmaf(x[a], x[a], D);
    }
}

__device__ __forceinline__ int moran_item_of_slot(const MoranSource& s, int slot) { return s.order ? (int)s.order[slot] : slot; }

// partial: [tensors][blocks]
template <int K>
__global__ void __launch_bounds__(kBlock) k_moran_forward(const MoranSource s, const MoranTensors T, float* __restrict__ partial) {
    __shared__ float s_red[kBlock / kWave];
    const int slot = blockIdx.x * kMoranItems + threadIdx.x / kMoranLanes, lane = threadIdx.x % kMoranLanes;
    float acc[kMoranMaxTensors];
#pragma unroll
    for (int t = 0; t < kMoranMaxTensors; ++t) acc[t] = 0.0f;
    if (slot < s.n) {
        MoranItem<K, false> it;
        it.load(s, moran_item_of_slot(s, slot));
        const float scale = (float)K / it.S;
#pragma unroll
        for (int t = 0; t < kMoranMaxTensors; ++t) {
            if (t >= T.count) break;
            const int F = T.width[t];
            const float* __restrict__ X = T.x[t];
            for (int f = lane; f < F; f += kMoranLanes) {
                float x[K], r[K], A, D;
#pragma unroll
                for (int a = 0; a < K; ++a) x[a] = X[(size_t)it.row[a] * F + f];
                moran_channel<K>(it.c, x, r, A, D);
                acc[t] += scale * A / D;
            }
        }
    }
#pragma unroll
    for (int t = 0; t < kMoranMaxTensors; ++t) {
        if (t >= T.count) break;
        const float v = block_sum(acc[t], s_red);
        if (threadIdx.x == 0) partial[(size_t)t * gridDim.x + blockIdx.x] = v;
    }
}

// out: total | term [T] | mean [T]
__global__ void __launch_bounds__(kMoranReduceBlock) k_moran_reduce(size_t blocks, int n, const MoranTensors T, const float* __restrict__ partial,
                                                                    float* __restrict__ out) {
    __shared__ double sh[kMoranReduceBlock];
    double total = 0.0;
    for (int t = 0; t < T.count; ++t) {
        double acc = 0.0;
        for (size_t i = threadIdx.x; i < blocks; i += kMoranReduceBlock) acc += (double)partial[(size_t)t * blocks + i];
        // block_tree_sum (reduce.h) written out: the division sits in front of the last barrier, where the helper would put it behind
        sh[threadIdx.x] = acc;
        __syncthreads();
        for (int d = kMoranReduceBlock / 2; d > 0; d >>= 1) {
            if ((int)threadIdx.x < d) sh[threadIdx.x] += sh[threadIdx.x + d];
            __syncthreads();
        }
        const double mean = sh[0] / ((double)n * (double)T.width[t]);
        __syncthreads();
        const double clamped = mean < 0.0 ? 0.0 : (mean > 1.0 ? 1.0 : mean);   // keeps NaN, as torch.clamp
        const double term = 1.0 - clamped;
        total += term;
        if (threadIdx.x == 0) { out[1 + t] = (float)term; out[1 + T.count + t] = (float)mean; }
    }
    if (threadIdx.x == 0) out[0] = (float)total;
}

// torch.clamp passes the gradient for 0 <= mean <= 1 and blocks it outside
__device__ __forceinline__ bool moran_gate(const float* __restrict__ out, int count, int t) {
    const float mean = out[1 + count + t];
    return mean >= 0.0f && mean <= 1.0f;
}

// sum over the 16 lanes of an item, in every lane
__device__ __forceinline__ float moran_item_sum(float v) {
#pragma unroll
    for (int d = kMoranLanes / 2; d > 0; d >>= 1) v += __shfl_xor(v, d, kMoranLanes);
    return v;
}

// d L / d q_a of item `it` from P_ab = dL/dc_ab + dL/dc_ba (a < b), with d c_ab / d q_a = -(q_a - q_b) / d^3
template <int K>
__device__ __forceinline__ void moran_store_point_edges(const MoranItem<K, true>& it, const float (&P)[K][K], float* __restrict__ edge_q, int p) {
#pragma unroll
    for (int a = 0; a < K; ++a) {
        float g[3] = {0.0f, 0.0f, 0.0f};
#pragma unroll
        for (int b = 0; b < K; ++b) {
            if (b == a) continue;
            const float w = -(a < b ? P[a][b] : P[b][a]) * it.w3[a][b];
#pragma unroll
            for (int d = 0; d < 3; ++d) g[d] = fmaf(w, it.q[a][d] - it.q[b][d], g[d]);
        }
#pragma unroll
        for (int d = 0; d < 3; ++d) edge_q[3 * ((size_t)p * K + a) + d] = g[d];
    }
}

// edge_x: [n K][edge_channels] (the tensors with a dx only) = d (sum of the open terms) / d x of edge (p, a);  edge_q: [n K][3] likewise for q_a (points
// given, d_points wanted);  d_weight: [n][K][K] (weights given), already times the upstream gradient
template <int K>
__global__ void __launch_bounds__(kBlock) k_moran_edges(const MoranSource s, const MoranTensors T, const MoranCoef coef,
                                                        const float* __restrict__ out, const float* __restrict__ upstream,
                                                        float* __restrict__ edge_x, float* __restrict__ edge_q, float* __restrict__ d_weight) {
    const int slot = blockIdx.x * kMoranItems + threadIdx.x / kMoranLanes, lane = threadIdx.x % kMoranLanes;
    if (slot >= s.n) return;     // whole items leave together: the shuffles below stay inside an item's 16 lanes
    const int p = moran_item_of_slot(s, slot);
    const bool want_c = edge_q != nullptr || d_weight != nullptr;
    MoranItem<K, true> it;
    it.load(s, p);
    const float scale = (float)K / it.S, inv_s = 1.0f / it.S;
    float G[K][K];               // upper triangle: dL/dc_ab, which is symmetric in (a, b) whatever c is
#pragma unroll
    for (int a = 0; a < K; ++a)
#pragma unroll
        for (int b = 0; b < K; ++b) G[a][b] = 0.0f;
#pragma unroll
    for (int t = 0; t < kMoranMaxTensors; ++t) {
        if (t >= T.count) break;
        if ((out && !moran_gate(out, T.count, t)) || (!T.dx[t] && !want_c)) continue;
        const int F = T.width[t];
        const float* __restrict__ X = T.x[t];
        const float w = coef.v[t];
        for (int f = lane; f < F; f += kMoranLanes) {
            float x[K], r[K], rt[K], A, D;
#pragma unroll
            for (int a = 0; a < K; ++a) x[a] = X[(size_t)it.row[a] * F + f];
            moran_channel<K>(it.c, x, r, A, D);
            const float inv_d = 1.0f / D;
            const float h = w * scale * inv_d;
            const float m2 = 2.0f * w * scale * A * inv_d * inv_d;      // 2 w m / D
            if (T.dx[t]) {
                // d A / d x_a = sum_b (c_ab + c_ba) x_b
#pragma unroll
                for (int a = 0; a < K; ++a) {
                    float tr = 0.0f;
#pragma unroll
                    for (int b = 0; b < K; ++b) tr = fmaf(it.c[b][a], x[b], tr);
                    rt[a] = tr;
                }
#pragma unroll
                for (int a = 0; a < K; ++a)
                    edge_x[((size_t)p * K + a) * T.edge_channels + T.edge_offset[t] + f] = h * (r[a] + rt[a]) - m2 * x[a];
            }
            if (want_c) {
                const float u = A * inv_s;
#pragma unroll
                for (int a = 0; a < K; ++a)
#pragma unroll
                    for (int b = a; b < K; ++b) G[a][b] = fmaf(h, x[a] * x[b] - u, G[a][b]);
            }
        }
    }
    if (!want_c) return;
#pragma unroll
    for (int a = 0; a < K; ++a)
#pragma unroll
        for (int b = a; b < K; ++b) G[a][b] = moran_item_sum(G[a][b]);
    if (lane != 0) return;
    if (d_weight) {
        const float g = *upstream;
#pragma unroll
        for (int a = 0; a < K; ++a)
#pragma unroll
            for (int b = 0; b < K; ++b) d_weight[((size_t)p * K + a) * K + b] = g * (a <= b ? G[a][b] : G[b][a]);
    } else {
#pragma unroll
        for (int a = 0; a < K; ++a)
#pragma unroll
            for (int b = a + 1; b < K; ++b) G[a][b] *= 2.0f;     // c_ab and c_ba are one function of the positions
        moran_store_point_edges<K>(it, G, edge_q, p);
    }
}

// row j of every gradient: the sum of its incoming edges in edge order (rev_start NULL: edge j alone), times the upstream
// gradient (NULL: 1); exact zeros where the clamp is shut (out NULL: no clamp)
__global__ void __launch_bounds__(kBlock) k_moran_collect(int rows, const MoranTensors T, const uint32_t* __restrict__ rev_start,
                                                          const uint32_t* __restrict__ rev_edges, const float* __restrict__ out,
                                                          const float* __restrict__ upstream, const float* __restrict__ edge_x,
                                                          const float* __restrict__ edge_q, float* __restrict__ d_points) {
    const int j = blockIdx.x * kMoranItems + threadIdx.x / kMoranLanes, lane = threadIdx.x % kMoranLanes;
    if (j >= rows) return;
    const uint32_t lo = rev_start ? rev_start[j] : (uint32_t)j, hi = rev_start ? rev_start[j + 1] : (uint32_t)j + 1u;
    const float g = upstream ? *upstream : 1.0f;
#pragma unroll
    for (int t = 0; t < kMoranMaxTensors; ++t) {
        if (t >= T.count) break;
        if (!T.dx[t]) continue;
        const int F = T.width[t];
        const bool open = out ? moran_gate(out, T.count, t) : true;
        for (int f = lane; f < F; f += kMoranLanes) {
            float sum = 0.0f;
            if (open)
                for (uint32_t k = lo; k < hi; ++k) {
                    const size_t e = rev_edges ? rev_edges[k] : k;
                    sum += edge_x[e * T.edge_channels + T.edge_offset[t] + f];
                }
            T.dx[t][(size_t)j * F + f] = open ? g * sum : 0.0f;     // the upstream gradient multiplies last
        }
    }
    if (d_points && lane < 3) {
        float sum = 0.0f;
        for (uint32_t k = lo; k < hi; ++k) {
            const size_t e = rev_edges ? rev_edges[k] : k;
            sum += edge_q[3 * e + lane];
        }
        d_points[3 * (size_t)j + lane] = g * sum;
    }
}

// query_nn's weights: c / max(S, 1e-5), one thread per point
template <int K>
__global__ void __launch_bounds__(kBlock) k_moran_weights(const MoranSource s, float* __restrict__ weights) {
    const int p = blockIdx.x * kBlock + threadIdx.x;
    if (p >= s.n) return;
    MoranItem<K, false> it;
    it.load(s, p);
    const float inv = 1.0f / fmaxf(it.S, 1e-5f);
#pragma unroll
    for (int a = 0; a < K; ++a)
#pragma unroll
        for (int b = 0; b < K; ++b) weights[((size_t)p * K + a) * K + b] = it.c[a][b] * inv;
}

// d / d q of sum_ab d_weights_ab c_ab / max(S, 1e-5), per edge
template <int K>
__global__ void __launch_bounds__(kBlock) k_moran_weights_edges(const MoranSource s, const float* __restrict__ d_weights, float* __restrict__ edge_q) {
    const int p = blockIdx.x * kBlock + threadIdx.x;
    if (p >= s.n) return;
    MoranItem<K, true> it;
    it.load(s, p);
    float dw[K][K], H = 0.0f;
#pragma unroll
    for (int a = 0; a < K; ++a)
#pragma unroll
        for (int b = 0; b < K; ++b) { dw[a][b] = d_weights[((size_t)p * K + a) * K + b]; H = fmaf(dw[a][b], it.c[a][b], H); }
    const bool clamped = !(it.S > 1e-5f);             // clamp_min(1e-5): S >= K eps, so this binds for tiny eps only
    const float inv = 1.0f / fmaxf(it.S, 1e-5f), shift = clamped ? 0.0f : H * inv * inv;
    float P[K][K];
#pragma unroll
    for (int a = 0; a < K; ++a)
#pragma unroll
        for (int b = a + 1; b < K; ++b) P[a][b] = (dw[a][b] + dw[b][a]) * inv - 2.0f * shift;
    moran_store_point_edges<K>(it, P, edge_q, p);
}

template <typename F>
void for_k(int k, F&& f) {
    switch (k) {
        case 1: f(std::integral_constant<int, 1>()); break;
        case 2: f(std::integral_constant<int, 2>()); break;
        case 3: f(std::integral_constant<int, 3>()); break;
        case 4: f(std::integral_constant<int, 4>()); break;
        case 5: f(std::integral_constant<int, 5>()); break;
        case 6: f(std::integral_constant<int, 6>()); break;
        case 7: f(std::integral_constant<int, 7>()); break;
        default: f(std::integral_constant<int, 8>()); break;
    }
}

size_t moran_blocks(int n) { return ((size_t)n + kMoranItems - 1) / kMoranItems; }

float* edge_q_of(void* edges, int n, int k, int channels) {
    return reinterpret_cast<float*>(static_cast<char*>(edges) + align_up((size_t)n * k * channels * sizeof(float), 256));
}

size_t moran_workspace_bytes(int n, int n_tensors) {
    if (n <= 0 || n_tensors <= 0 || n_tensors > kMoranMaxTensors) return 0;
    return align_up(moran_blocks(n) * n_tensors * sizeof(float), 256);
}

size_t moran_edges_bytes(int n, int k, int channels) {
    if (n <= 0 || k < 1 || k > kKnnMaxK || channels < 0) return 0;
    return align_up((size_t)n * k * channels * sizeof(float), 256) + align_up((size_t)n * k * 3 * sizeof(float), 256);
}

void launch_moran_forward(const MoranSource& s, const MoranTensors& t, void* workspace, float* out, hipStream_t st) {
    const size_t nb = moran_blocks(s.n);
    float* partial = static_cast<float*>(workspace);
    for_k(s.k, [&](auto kc) {
        hipLaunchKernelGGL(k_moran_forward<decltype(kc)::value>, dim3((unsigned)nb), dim3(kBlock), 0, st, s, t, partial);
    });
    hipLaunchKernelGGL(k_moran_reduce, dim3(1), dim3(kMoranReduceBlock), 0, st, nb, s.n, t, partial, out);
}

void launch_moran_backward(const MoranSource& s, const MoranTensors& t, const uint32_t* rev_start, const uint32_t* rev_edges, const float* out,
                           const float* upstream, void* edges, float* d_points, float* d_weight, hipStream_t st) {
    MoranCoef coef;
    for (int i = 0; i < kMoranMaxTensors; ++i) coef.v[i] = i < t.count ? (float)((out ? -1.0 : 1.0) / ((double)s.n * (double)t.width[i])) : 0.0f;
    float* edge_x = static_cast<float*>(edges);
    float* edge_q = d_points ? edge_q_of(edges, s.n, s.k, t.edge_channels) : nullptr;
    for_k(s.k, [&](auto kc) {
        hipLaunchKernelGGL(k_moran_edges<decltype(kc)::value>, dim3((unsigned)moran_blocks(s.n)), dim3(kBlock), 0, st, s, t, coef, out, upstream,
                           edge_x, edge_q, d_weight);
    });
    bool any = d_points != nullptr;
    for (int i = 0; i < t.count; ++i) any = any || t.dx[i];
    if (!any) return;
    const int rows = rev_start ? s.n : s.n * s.k;
    hipLaunchKernelGGL(k_moran_collect, dim3((unsigned)moran_blocks(rows)), dim3(kBlock), 0, st, rows, t, rev_start, rev_edges, out, upstream,
                       edge_x, edge_q, d_points);
}

void launch_moran_weights(const MoranSource& s, float* weights, hipStream_t st) {
    for_k(s.k, [&](auto kc) {
        hipLaunchKernelGGL(k_moran_weights<decltype(kc)::value>, dim3((unsigned)((s.n + kBlock - 1) / kBlock)), dim3(kBlock), 0, st, s, weights);
    });
}

void launch_moran_weights_backward(const MoranSource& s, const uint32_t* rev_start, const uint32_t* rev_edges, const float* d_weights,
                                   void* edges, float* d_points, hipStream_t st) {
    float* edge_q = edge_q_of(edges, s.n, s.k, 0);
    for_k(s.k, [&](auto kc) {
        hipLaunchKernelGGL(k_moran_weights_edges<decltype(kc)::value>, dim3((unsigned)((s.n + kBlock - 1) / kBlock)), dim3(kBlock), 0, st, s,
                           d_weights, edge_q);
    });
    MoranTensors none = {};
    hipLaunchKernelGGL(k_moran_collect, dim3((unsigned)moran_blocks(s.n)), dim3(kBlock), 0, st, s.n, none, rev_start, rev_edges,
                       (const float*)nullptr, (const float*)nullptr, (const float*)nullptr, edge_q, d_points);
}

}  // namespace

}  // namespace sr

// ---- C entry points (include/splatraster.h): what is refused on the host, then the launchers above --------------------
using sr::fail; using sr::check_hip;

namespace {

// the checks that sr_moran_forward and sr_moran_backward share; fills the kernel-side descriptions
int open_moran(const char* who, int n, int k, float eps, const float* points, const float* weight, const int* nn_ix, const unsigned* order,
               int n_tensors, const float* const* features, const int* widths, sr::MoranSource* s, sr::MoranTensors* t) {
    const std::string name(who);
    if (n <= 0) return fail("bad arguments to " + name + ": sizes must be positive");
    if ((points == nullptr) == (weight == nullptr)) return fail(name + ": points or weight (exactly one of them)");
    if (k < (points ? sr::kKnnMinK : 1) || k > sr::kKnnMaxK) return fail("bad arguments to " + name + ": k must be 2 .. 8 (1 .. 8 with weight)");
    if (points && n < k) return fail("bad arguments to " + name + ": fewer points than neighbours (n < k)");
    if (points && !nn_ix) return fail("null pointer in " + name + ": points need nn_ix");
    if (n_tensors < 1) return fail(name + ": at least one feature tensor");
    if (n_tensors > sr::kMoranMaxTensors) return fail(name + ": at most 8 feature tensors in one call");
    if (!features || !widths) return fail("null pointer in " + name);
    *s = sr::MoranSource{n, k, eps, points, weight, nn_ix, order};
    *t = sr::MoranTensors{};
    t->count = n_tensors;
    long long channels = 0;
    for (int i = 0; i < n_tensors; ++i) {
        if (widths[i] <= 0) return fail("bad arguments to " + name + ": sizes must be positive");
        if (!features[i]) return fail("null pointer in " + name);
        t->x[i] = features[i]; t->width[i] = widths[i]; t->offset[i] = (int)channels;
        channels += widths[i];
        if (channels > 0x7fffffff / sr::kKnnMaxK) return fail("too many channels for " + name);
    }
    if ((long long)n > 0x7fffffff / (3 * sr::kKnnMaxK)) return fail("too many items for " + name);
    t->channels = (int)channels;
    return 0;
}

}  // namespace

extern "C" {

size_t sr_moran_workspace_bytes(int n, int n_tensors) { return sr::moran_workspace_bytes(n, n_tensors); }

size_t sr_moran_edges_bytes(int n, int k, int channels) { return sr::moran_edges_bytes(n, k, channels); }

int sr_moran_forward(int n, int k, float eps, const float* points, const float* weight, const int* nn_ix, const unsigned* order, int n_tensors,
                     const float* const* features, const int* widths, void* workspace, float* out, void* hip_stream) {
    sr::MoranSource s; sr::MoranTensors t;
    SR_TRY(open_moran("sr_moran_forward", n, k, eps, points, weight, nn_ix, order, n_tensors, features, widths, &s, &t));
    if (!workspace || !out) return fail("null pointer in sr_moran_forward");
    sr::launch_moran_forward(s, t, workspace, out, static_cast<hipStream_t>(hip_stream));
    return check_hip(hipGetLastError(), "moran_forward");
}

int sr_moran_backward(int n, int k, float eps, const float* points, const float* weight, const int* nn_ix, const unsigned* order,
                      const unsigned* rev_start, const unsigned* rev_edges, int n_tensors, const float* const* features, const int* widths,
                      const float* out, const float* upstream, void* edges, float* const* dL_dfeatures, float* dL_dpoints, float* dL_dweight,
                      void* hip_stream) {
    sr::MoranSource s; sr::MoranTensors t;
    SR_TRY(open_moran("sr_moran_backward", n, k, eps, points, weight, nn_ix, order, n_tensors, features, widths, &s, &t));
    if (!upstream || !edges || !dL_dfeatures) return fail("null pointer in sr_moran_backward");
    if (dL_dpoints && !points) return fail("sr_moran_backward: dL_dpoints without points");
    if (dL_dweight && !weight) return fail("sr_moran_backward: dL_dweight without weight");
    if ((rev_start == nullptr) != (rev_edges == nullptr)) return fail("sr_moran_backward: rev_start and rev_edges go together (both or neither)");
    if (nn_ix && !rev_start) return fail("null pointer in sr_moran_backward: nn_ix needs the reverse adjacency");
    if (!nn_ix && rev_start) return fail("sr_moran_backward: a reverse adjacency without nn_ix");
    for (int i = 0; i < n_tensors; ++i) {
        t.dx[i] = dL_dfeatures[i];
        t.edge_offset[i] = t.edge_channels;
        if (t.dx[i]) t.edge_channels += t.width[i];
    }
    sr::launch_moran_backward(s, t, rev_start, rev_edges, out, upstream, edges, dL_dpoints, dL_dweight, static_cast<hipStream_t>(hip_stream));
    return check_hip(hipGetLastError(), "moran_backward");
}

int sr_moran_weights(int n, int k, float eps, const float* points, const int* nn_ix, float* weights, void* hip_stream) {
    if (n <= 0) return fail("bad arguments to sr_moran_weights: sizes must be positive");
    if (k < sr::kKnnMinK || k > sr::kKnnMaxK) return fail("bad arguments to sr_moran_weights: k must be 2 .. 8");
    if (n < k) return fail("bad arguments to sr_moran_weights: fewer points than neighbours (n < k)");
    if (n > 0x7fffffff / (3 * sr::kKnnMaxK)) return fail("too many points for sr_moran_weights");
    if (!points || !nn_ix || !weights) return fail("null pointer in sr_moran_weights");
    sr::launch_moran_weights(sr::MoranSource{n, k, eps, points, nullptr, nn_ix, nullptr}, weights, static_cast<hipStream_t>(hip_stream));
    return check_hip(hipGetLastError(), "moran_weights");
}

int sr_moran_weights_backward(int n, int k, float eps, const float* points, const int* nn_ix, const unsigned* rev_start, const unsigned* rev_edges,
                              const float* dL_dweights, void* edges, float* dL_dpoints, void* hip_stream) {
    if (n <= 0) return fail("bad arguments to sr_moran_weights_backward: sizes must be positive");
    if (k < sr::kKnnMinK || k > sr::kKnnMaxK) return fail("bad arguments to sr_moran_weights_backward: k must be 2 .. 8");
    if (n < k) return fail("bad arguments to sr_moran_weights_backward: fewer points than neighbours (n < k)");
    if (n > 0x7fffffff / (3 * sr::kKnnMaxK)) return fail("too many points for sr_moran_weights_backward");
    if (!points || !nn_ix || !rev_start || !rev_edges || !dL_dweights || !edges || !dL_dpoints) return fail("null pointer in sr_moran_weights_backward");
    sr::launch_moran_weights_backward(sr::MoranSource{n, k, eps, points, nullptr, nn_ix, nullptr}, rev_start, rev_edges, dL_dweights, edges,
                                      dL_dpoints, static_cast<hipStream_t>(hip_stream));
    return check_hip(hipGetLastError(), "moran_weights_backward");
}

}  // extern "C"
