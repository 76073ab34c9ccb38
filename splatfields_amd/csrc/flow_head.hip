// The flow head of the deform network (include/splatraster.h: sr_flow_head_*): the branch linears
// z = hidden W^T + b of one reference `FlowHead`, the per-point epilogue of its flow model, and the whole backward, one kernel
// each.
//
// Mapping.  A workgroup owns 256 consecutive points, one per thread, on every device: no sum depends on the grid.  The branch
// weights are staged once per workgroup into LDS as one [M][width] fp32 matrix (M = all branch rows, <= 32).  `hidden` rows are
// 512 bytes at the reference's width: the workgroup moves 16 columns of its 256 rows at a time through an LDS tile (point_tile.h),
// coalesced in, and each thread then reads its own row's piece back.  The weights of a column group are the same LDS address in every lane
// (a broadcast read).  dL/dhidden goes the same way in the other direction: 16 columns per thread into the tile, coalesced out.
//
// Arithmetic.  z[m] = bias[m] + sum over columns c = 0, 1, ... of h[c] W[m][c], a chain of double FMAs (the product of two
// floats is exact in double); the epilogue -- normalisation, sin / cos, 1 - cos t and t - sin t, softplus, the transform -- and
// its backward are doubles with IEEE sqrt and division; every stored value is rounded to fp32 once.  The backward starts from
// the forward's z, saved as doubles ([M][N], so that a wavefront's loads and stores of one z are contiguous), and multiplies the
// unrounded dz with W for dL/dhidden.  No atomics, no host wait.
#include "host_api.h"
#include "point_tile.h"
#include "reduce.h"

namespace sr {

namespace {

struct FlowK {
    int model, width, n_basis, n_branches, dz_row;
    long long n;
    SrFlowBranch branch[SR_FLOW_MAX_BRANCHES];
    const float* hidden; const float* pts; const float* bases;
    float* means; float* flow; double* saved;
    const float* g_means; const float* g_flow;
    float* d_pts; float* d_z; float* d_hidden; double* partial;
};

struct Vec3 { double x, y, z; };
__device__ __forceinline__ Vec3 v3(double x, double y, double z) { return Vec3{x, y, z}; }
__device__ __forceinline__ Vec3 operator+(Vec3 a, Vec3 b) { return v3(a.x + b.x, a.y + b.y, a.z + b.z); }
__device__ __forceinline__ Vec3 operator-(Vec3 a, Vec3 b) { return v3(a.x - b.x, a.y - b.y, a.z - b.z); }
__device__ __forceinline__ Vec3 operator*(double s, Vec3 a) { return v3(s * a.x, s * a.y, s * a.z); }
__device__ __forceinline__ double dot(Vec3 a, Vec3 b) { return a.x * b.x + a.y * b.y + a.z * b.z; }
__device__ __forceinline__ Vec3 cross(Vec3 a, Vec3 b) { return v3(a.y * b.z - a.z * b.y, a.z * b.x - a.x * b.z, a.x * b.y - a.y * b.x); }

// what the SE(3) models make of (w_raw, v_raw): the reference's convention w = w_raw / |w_raw| + 1e-5 (not a unit vector)
struct Se3 {
    double theta, s, c, omc, tms, ww;
    Vec3 w, v, wv, wwv, t;
    double R[3][3];
};

__device__ __forceinline__ Se3 se3_eval(Vec3 wr, Vec3 vr) {
    Se3 e;
    e.theta = sqrt(dot(wr, wr));
    e.w = v3(wr.x / e.theta + 1e-5, wr.y / e.theta + 1e-5, wr.z / e.theta + 1e-5);
    e.v = v3(vr.x / e.theta + 1e-5, vr.y / e.theta + 1e-5, vr.z / e.theta + 1e-5);
    e.s = sin(e.theta); e.c = cos(e.theta);
    e.omc = 1.0 - e.c; e.tms = e.theta - e.s;
    e.ww = dot(e.w, e.w);
    const Vec3 w = e.w;
    // R = I + s [w] + (1 - c) (w w^T - |w|^2 I)
    e.R[0][0] = 1.0 + e.omc * (w.x * w.x - e.ww); e.R[0][1] = -e.s * w.z + e.omc * w.x * w.y;   e.R[0][2] = e.s * w.y + e.omc * w.x * w.z;
    e.R[1][0] = e.s * w.z + e.omc * w.y * w.x;    e.R[1][1] = 1.0 + e.omc * (w.y * w.y - e.ww); e.R[1][2] = -e.s * w.x + e.omc * w.y * w.z;
    e.R[2][0] = -e.s * w.y + e.omc * w.z * w.x;   e.R[2][1] = e.s * w.x + e.omc * w.z * w.y;    e.R[2][2] = 1.0 + e.omc * (w.z * w.z - e.ww);
    e.wv = cross(w, e.v);
    e.wwv = cross(w, e.wv);
    e.t = e.theta * e.v + e.omc * e.wv + e.tms * e.wwv;
    return e;
}

__device__ __forceinline__ Vec3 mat_vec(const double (&R)[3][3], Vec3 p) {
    return v3(R[0][0] * p.x + R[0][1] * p.y + R[0][2] * p.z, R[1][0] * p.x + R[1][1] * p.y + R[1][2] * p.z,
              R[2][0] * p.x + R[2][1] * p.y + R[2][2] * p.z);
}
__device__ __forceinline__ Vec3 mat_t_vec(const double (&R)[3][3], Vec3 g) {
    return v3(R[0][0] * g.x + R[1][0] * g.y + R[2][0] * g.z, R[0][1] * g.x + R[1][1] * g.y + R[2][1] * g.z,
              R[0][2] * g.x + R[1][2] * g.y + R[2][2] * g.z);
}

// gradients at (w_raw, v_raw) from the gradients GR at R and Gt at t
__device__ __forceinline__ void se3_backward(const Se3& e, Vec3 wr, Vec3 vr, const double (&GR)[3][3], Vec3 Gt, Vec3* d_wr, Vec3* d_vr) {
    const Vec3 w = e.w;
    // R: the s [w] term sees the antisymmetric part of GR, the (1 - c) term the symmetric one
    const Vec3 a = v3(GR[2][1] - GR[1][2], GR[0][2] - GR[2][0], GR[1][0] - GR[0][1]);
    const double tr = GR[0][0] + GR[1][1] + GR[2][2];
    const Vec3 gw_sym = v3((GR[0][0] + GR[0][0]) * w.x + (GR[0][1] + GR[1][0]) * w.y + (GR[0][2] + GR[2][0]) * w.z,
                           (GR[1][0] + GR[0][1]) * w.x + (GR[1][1] + GR[1][1]) * w.y + (GR[1][2] + GR[2][1]) * w.z,
                           (GR[2][0] + GR[0][2]) * w.x + (GR[2][1] + GR[1][2]) * w.y + (GR[2][2] + GR[2][2]) * w.z);
    const double wGw = w.x * (GR[0][0] * w.x + GR[0][1] * w.y + GR[0][2] * w.z) + w.y * (GR[1][0] * w.x + GR[1][1] * w.y + GR[1][2] * w.z) +
                       w.z * (GR[2][0] * w.x + GR[2][1] * w.y + GR[2][2] * w.z);
    double g_s = dot(w, a);
    double g_omc = wGw - e.ww * tr;
    Vec3 g_w = e.s * a + e.omc * (gw_sym - (2.0 * tr) * w);
    // t = theta v + (1 - c) wv + (theta - s) wwv,  wv = w x v,  wwv = w x wv
    g_omc += dot(Gt, e.wv);
    const double g_tms = dot(Gt, e.wwv);
    Vec3 g_v = e.theta * Gt;
    const Vec3 g_wwv = e.tms * Gt;
    g_w = g_w + cross(e.wv, g_wwv);
    const Vec3 g_wv = e.omc * Gt + cross(g_wwv, w);
    g_w = g_w + cross(e.v, g_wv);
    g_v = g_v + cross(g_wv, w);
    // s = sin, 1 - c, theta - s as functions of theta
    double g_theta = dot(Gt, e.v) + g_s * e.c + g_omc * e.s + g_tms * e.omc;
    // w = w_raw / theta + eps, v = v_raw / theta + eps, theta = |w_raw|
    g_theta -= (dot(g_w, wr) + dot(g_v, vr)) / (e.theta * e.theta);
    *d_wr = v3(g_w.x / e.theta + g_theta * (wr.x / e.theta), g_w.y / e.theta + g_theta * (wr.y / e.theta), g_w.z / e.theta + g_theta * (wr.z / e.theta));
    *d_vr = v3(g_v.x / e.theta, g_v.y / e.theta, g_v.z / e.theta);
}

__device__ __forceinline__ double softplus(double x) { return x > 20.0 ? x : log1p(exp(x)); }
__device__ __forceinline__ double softplus_grad(double x) { return x > 20.0 ? 1.0 : 1.0 / (1.0 + exp(-x)); }

// the branch weights as one [kM][width] fp32 matrix in LDS
template <int kM>
__device__ __forceinline__ void stage_weights(const FlowK& P, float* s_w) {
    const int wq = P.width >> 2;                 // float4s per row
    for (int i = (int)threadIdx.x; i < kM * wq; i += kBlock) {
        int m = i / wq;
        const int q = i - m * wq;
        const int row = m;
        const float* src = nullptr;
#pragma unroll
        for (int b = 0; b < SR_FLOW_MAX_BRANCHES; ++b)
            if (b < P.n_branches && src == nullptr) {
                if (m < P.branch[b].rows) src = P.branch[b].weight + (size_t)m * P.width + 4 * q;
                else m -= P.branch[b].rows;
            }
        reinterpret_cast<float4*>(s_w)[row * wq + q] = *reinterpret_cast<const float4*>(src);
    }
}

__device__ __forceinline__ Vec3 load3(const float* __restrict__ p, long long i) { return v3((double)p[3 * i], (double)p[3 * i + 1], (double)p[3 * i + 2]); }
__device__ __forceinline__ void store3(float* __restrict__ p, long long i, Vec3 v) { p[3 * i] = (float)v.x; p[3 * i + 1] = (float)v.y; p[3 * i + 2] = (float)v.z; }

template <int kM>
__global__ void __launch_bounds__(kBlock) k_flow_head_forward(const FlowK P) {
    extern __shared__ __align__(16) float s_dyn[];
    __shared__ double s_bias[SR_FLOW_MAX_OUT];
    __shared__ double s_bases[SR_FLOW_MAX_BASIS];
    float* s_w = s_dyn;                                   // [kM][width]
    float* s_tile = s_dyn + kM * P.width;                 // [256][20]
    const int tid = (int)threadIdx.x;
    const long long first = (long long)blockIdx.x * kBlock, point = first + tid;
    stage_weights<kM>(P, s_w);
    if (tid < kM) {
        int m = tid;
        float b = 0.f;
        bool found = false;
        for (int k = 0; k < P.n_branches; ++k)
            if (!found) {
                if (m < P.branch[k].rows) { b = P.branch[k].bias[m]; found = true; }
                else m -= P.branch[k].rows;
            }
        s_bias[tid] = (double)b;
    }
    if (P.model == SR_FLOW_DCT && tid < P.n_basis) s_bases[tid] = (double)P.bases[tid];
    __syncthreads();

    double z[kM];
#pragma unroll
    for (int m = 0; m < kM; ++m) z[m] = s_bias[m];
    for (int c0 = 0; c0 < P.width; c0 += kTileCols) {
        tile_load(P.hidden, first, P.n, P.width, c0, s_tile);
        __syncthreads();
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            if (c0 + 4 * q < P.width) {                   // the same in every thread
                const float4 h = *reinterpret_cast<const float4*>(s_tile + tid * kTileRow + 4 * q);
                const double h0 = h.x, h1 = h.y, h2 = h.z, h3 = h.w;
#pragma unroll
                for (int m = 0; m < kM; ++m) {
                    const float4 w = *reinterpret_cast<const float4*>(s_w + m * P.width + c0 + 4 * q);
                    z[m] = fma(h0, (double)w.x, z[m]);
                    z[m] = fma(h1, (double)w.y, z[m]);
                    z[m] = fma(h2, (double)w.z, z[m]);
                    z[m] = fma(h3, (double)w.w, z[m]);
                }
            }
        }
        __syncthreads();
    }
    if (point >= P.n) return;
    if (P.saved) {
#pragma unroll
        for (int m = 0; m < kM; ++m) P.saved[(size_t)m * P.n + point] = z[m];
    }
    const Vec3 p = load3(P.pts, point);
    if (P.model == SR_FLOW_OFFSET) {
        if constexpr (kM == 3) {
            const Vec3 f = v3(z[0], z[1], z[2]);
            store3(P.flow, point, f);
            store3(P.means, point, p + f);
        }
    } else if (P.model == SR_FLOW_DCT) {
        if constexpr (kM % 3 == 0) {
            constexpr int K = kM / 3;
            double f[3];
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                double acc = 0.0;
#pragma unroll
                for (int k = 0; k < K; ++k) acc = fma(z[c * K + k], s_bases[k], acc);
                f[c] = acc;
            }
            const Vec3 fl = v3(f[0], f[1], f[2]);
            store3(P.flow, point, fl);
            store3(P.means, point, p + fl);
        }
    } else if (P.model == SR_FLOW_AFFINE) {
        if constexpr (kM == 12) {
            const Vec3 mean = v3(z[0] * p.x + z[1] * p.y + z[2] * p.z + z[9], z[3] * p.x + z[4] * p.y + z[5] * p.z + z[10],
                                 z[6] * p.x + z[7] * p.y + z[8] * p.z + z[11]);
            store3(P.means, point, mean);
            store3(P.flow, point, mean - p);
        }
    } else {
        if constexpr (kM == 6 || kM == 9 || kM == 10) {
            const Se3 e = se3_eval(v3(z[0], z[1], z[2]), v3(z[3], z[4], z[5]));
            Vec3 mean = mat_vec(e.R, p);
            if constexpr (kM == 10) mean = softplus(z[6]) * mean;
            mean = mean + e.t;
            if constexpr (kM == 9) mean = mean + v3(z[6], z[7], z[8]);
            if constexpr (kM == 10) mean = mean + v3(z[7], z[8], z[9]);
            store3(P.means, point, mean);
            if constexpr (kM == 6) {
                float4* out = reinterpret_cast<float4*>(P.flow + 16 * (size_t)point);
                out[0] = make_float4((float)e.R[0][0], (float)e.R[0][1], (float)e.R[0][2], (float)e.t.x);
                out[1] = make_float4((float)e.R[1][0], (float)e.R[1][1], (float)e.R[1][2], (float)e.t.y);
                out[2] = make_float4((float)e.R[2][0], (float)e.R[2][1], (float)e.R[2][2], (float)e.t.z);
                out[3] = make_float4(0.f, 0.f, 0.f, 1.f);
            } else {
                store3(P.flow, point, mean - p);
            }
        }
    }
}

template <int kM>
__global__ void __launch_bounds__(kBlock) k_flow_head_backward(const FlowK P) {
    extern __shared__ __align__(16) float s_dyn[];
    __shared__ double s_bases[SR_FLOW_MAX_BASIS];
    __shared__ double s_red[kBlock / kWave];
    float* s_w = s_dyn;
    float* s_tile = s_dyn + kM * P.width;
    const int tid = (int)threadIdx.x;
    const long long first = (long long)blockIdx.x * kBlock, point = first + tid;
    const bool live = point < P.n;
    if (P.d_hidden) stage_weights<kM>(P, s_w);
    if (P.model == SR_FLOW_DCT && tid < P.n_basis) s_bases[tid] = (double)P.bases[tid];
    __syncthreads();

    double dz[kM];
#pragma unroll
    for (int m = 0; m < kM; ++m) dz[m] = 0.0;
    [[maybe_unused]] double d_bases[kM % 3 == 0 ? kM / 3 : 1];
#pragma unroll
    for (int k = 0; k < (kM % 3 == 0 ? kM / 3 : 1); ++k) d_bases[k] = 0.0;
    if (live) {
        double z[kM];
#pragma unroll
        for (int m = 0; m < kM; ++m) z[m] = P.saved[(size_t)m * P.n + point];
        const Vec3 p = load3(P.pts, point);
        const Vec3 gm = load3(P.g_means, point);
        Vec3 gf = v3(0.0, 0.0, 0.0);
        if (P.g_flow && P.model != SR_FLOW_SE3) gf = load3(P.g_flow, point);
        const Vec3 G = gm + gf;                            // gradient at means3D of the models whose flow is means3D - p (or p + flow)
        Vec3 d_p = gm;
        if (P.model == SR_FLOW_OFFSET) {
            if constexpr (kM == 3) { dz[0] = G.x; dz[1] = G.y; dz[2] = G.z; }
        } else if (P.model == SR_FLOW_DCT) {
            if constexpr (kM % 3 == 0) {
                constexpr int K = kM / 3;
                const double g[3] = {G.x, G.y, G.z};
#pragma unroll
                for (int c = 0; c < 3; ++c)
#pragma unroll
                    for (int k = 0; k < K; ++k) dz[c * K + k] = g[c] * s_bases[k];
#pragma unroll
                for (int k = 0; k < K; ++k) d_bases[k] = g[0] * z[k] + g[1] * z[K + k] + g[2] * z[2 * K + k];
            }
        } else if (P.model == SR_FLOW_AFFINE) {
            if constexpr (kM == 12) {
                const double g[3] = {G.x, G.y, G.z}, pp[3] = {p.x, p.y, p.z};
#pragma unroll
                for (int i = 0; i < 3; ++i)
#pragma unroll
                    for (int j = 0; j < 3; ++j) dz[3 * i + j] = g[i] * pp[j];
                dz[9] = G.x; dz[10] = G.y; dz[11] = G.z;
                d_p = v3(z[0] * G.x + z[3] * G.y + z[6] * G.z, z[1] * G.x + z[4] * G.y + z[7] * G.z, z[2] * G.x + z[5] * G.y + z[8] * G.z) - gf;
            }
        } else {
            if constexpr (kM == 6 || kM == 9 || kM == 10) {
                const Vec3 wr = v3(z[0], z[1], z[2]), vr = v3(z[3], z[4], z[5]);
                const Se3 e = se3_eval(wr, vr);
                double scale = 1.0;
                if constexpr (kM == 10) scale = softplus(z[6]);
                const double g[3] = {G.x, G.y, G.z}, pp[3] = {p.x, p.y, p.z};
                double GR[3][3];
#pragma unroll
                for (int i = 0; i < 3; ++i)
#pragma unroll
                    for (int j = 0; j < 3; ++j) GR[i][j] = scale * g[i] * pp[j];
                Vec3 Gt = G;
                if constexpr (kM == 6) {
                    if (P.g_flow) {                        // the 4x4 itself is an output: its rotation block and its last column
                        const float* gfl = P.g_flow + 16 * (size_t)point;
#pragma unroll
                        for (int i = 0; i < 3; ++i)
#pragma unroll
                            for (int j = 0; j < 3; ++j) GR[i][j] += (double)gfl[4 * i + j];
                        Gt = Gt + v3((double)gfl[3], (double)gfl[7], (double)gfl[11]);
                    }
                    d_p = mat_t_vec(e.R, gm);
                } else {
                    d_p = scale * mat_t_vec(e.R, G) - gf;
                }
                Vec3 d_wr, d_vr;
                se3_backward(e, wr, vr, GR, Gt, &d_wr, &d_vr);
                dz[0] = d_wr.x; dz[1] = d_wr.y; dz[2] = d_wr.z; dz[3] = d_vr.x; dz[4] = d_vr.y; dz[5] = d_vr.z;
                if constexpr (kM == 9) { dz[6] = G.x; dz[7] = G.y; dz[8] = G.z; }
                if constexpr (kM == 10) {
                    dz[6] = dot(G, mat_vec(e.R, p)) * softplus_grad(z[6]);
                    dz[7] = G.x; dz[8] = G.y; dz[9] = G.z;
                }
            }
        }
        if (P.d_pts) store3(P.d_pts, point, d_p);
        // dL/dz, every branch from a multiple of 4 columns on, zeros between
        float* out = P.d_z + (size_t)point * P.dz_row;
        for (int c = 0; c < P.dz_row; c += 4) *reinterpret_cast<float4*>(out + c) = make_float4(0.f, 0.f, 0.f, 0.f);
        int b = 0, m_end = P.branch[0].rows, shift = 0;
#pragma unroll
        for (int k = 0; k < kM; ++k) {                     // dz stays in registers: k is a constant, its column is not
            if (k == m_end) { shift += (-P.branch[b].rows) & 3; ++b; m_end += P.branch[b].rows; }
            out[k + shift] = (float)dz[k];
        }
    }
    if (P.model == SR_FLOW_DCT) {
        if constexpr (kM % 3 == 0) {
#pragma unroll
            for (int k = 0; k < kM / 3; ++k) {
                const double sum = block_sum(d_bases[k], s_red);
                if (tid == 0) P.partial[(size_t)blockIdx.x * (kM / 3) + k] = sum;
            }
        }
    }
    if (!P.d_hidden) return;
    for (int c0 = 0; c0 < P.width; c0 += kTileCols) {
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            if (c0 + 4 * q < P.width) {
                double o0 = 0.0, o1 = 0.0, o2 = 0.0, o3 = 0.0;
#pragma unroll
                for (int m = 0; m < kM; ++m) {
                    const float4 w = *reinterpret_cast<const float4*>(s_w + m * P.width + c0 + 4 * q);
                    o0 = fma(dz[m], (double)w.x, o0);
                    o1 = fma(dz[m], (double)w.y, o1);
                    o2 = fma(dz[m], (double)w.z, o2);
                    o3 = fma(dz[m], (double)w.w, o3);
                }
                *reinterpret_cast<float4*>(s_tile + tid * kTileRow + 4 * q) = make_float4((float)o0, (float)o1, (float)o2, (float)o3);
            }
        }
        __syncthreads();
        tile_store(P.d_hidden, first, P.n, P.width, c0, s_tile);
        __syncthreads();
    }
}

int flow_rows(int model, int n_basis, int* rows) {
    switch (model) {
        case SR_FLOW_OFFSET: rows[0] = 3; return 1;
        case SR_FLOW_SE3: rows[0] = 3; rows[1] = 3; return 2;
        case SR_FLOW_SE3_AFFINE: rows[0] = 3; rows[1] = 3; rows[2] = 3; return 3;
        case SR_FLOW_SE3_SCALED: rows[0] = 3; rows[1] = 3; rows[2] = 1; rows[3] = 3; return 4;
        case SR_FLOW_AFFINE: rows[0] = 9; rows[1] = 3; return 2;
        case SR_FLOW_DCT: if (n_basis < 1 || n_basis > SR_FLOW_MAX_BASIS) return 0; rows[0] = 3 * n_basis; return 1;
        default: return 0;
    }
}

template <bool kBackward, int kM>
void flow_launch_m(const FlowK& k, hipStream_t st) {
    const size_t lds = ((size_t)kM * k.width + (size_t)kBlock * kTileRow) * sizeof(float);      // <= 32 KiB + 20 KiB
    const unsigned blocks = (unsigned)((k.n + kBlock - 1) / kBlock);
    if (kBackward) hipLaunchKernelGGL(k_flow_head_backward<kM>, dim3(blocks), dim3(kBlock), lds, st, k);
    else hipLaunchKernelGGL(k_flow_head_forward<kM>, dim3(blocks), dim3(kBlock), lds, st, k);
}

template <bool kBackward>
void flow_launch(const FlowK& k, int m, hipStream_t st) {
    switch (m) {
        case 3: flow_launch_m<kBackward, 3>(k, st); break;
        case 6: flow_launch_m<kBackward, 6>(k, st); break;
        case 9: flow_launch_m<kBackward, 9>(k, st); break;
        case 10: flow_launch_m<kBackward, 10>(k, st); break;
        case 12: flow_launch_m<kBackward, 12>(k, st); break;
        case 15: flow_launch_m<kBackward, 15>(k, st); break;
        case 18: flow_launch_m<kBackward, 18>(k, st); break;
        case 21: flow_launch_m<kBackward, 21>(k, st); break;
        case 24: flow_launch_m<kBackward, 24>(k, st); break;
        case 27: flow_launch_m<kBackward, 27>(k, st); break;
        case 30: flow_launch_m<kBackward, 30>(k, st); break;
        default: break;      // flow_head_shape_error has refused it
    }
}

int flow_head_dz_row(int model, int n_basis) {
    int rows[SR_FLOW_MAX_BRANCHES], m = 0;
    const int nb = flow_rows(model, n_basis, rows);
    for (int b = 0; b < nb; ++b) m += (rows[b] + 3) & ~3;
    return m;
}

FlowK flow_params(int model, long long n, int width, int n_basis, int n_branches, const SrFlowBranch* branches) {
    FlowK k{};
    k.model = model; k.n = n; k.width = width; k.n_basis = n_basis; k.n_branches = n_branches;
    k.dz_row = flow_head_dz_row(model, n_basis);
    for (int b = 0; b < n_branches; ++b) k.branch[b] = branches[b];
    return k;
}

const char* flow_head_shape_error(int model, long long n_points, int width, int n_basis) {
    int rows[SR_FLOW_MAX_BRANCHES];
    if (model < SR_FLOW_OFFSET || model > SR_FLOW_DCT) return "unknown flow model";
    if (flow_rows(model, n_basis, rows) == 0) return "n_basis must be in 1 .. SR_FLOW_MAX_BASIS";
    if (width < 4 || (width & 3) || width > SR_FLOW_MAX_WIDTH) return "width must be a multiple of 4 in 4 .. SR_FLOW_MAX_WIDTH";
    if (n_points < 0 || n_points >= (1ll << 31)) return "n_points must be in 0 .. 2^31 - 1";
    return nullptr;
}

int flow_head_outputs(int model, int n_basis) {
    int rows[SR_FLOW_MAX_BRANCHES], m = 0;
    const int nb = flow_rows(model, n_basis, rows);
    for (int b = 0; b < nb; ++b) m += rows[b];
    return m;
}

const char* flow_head_branch_error(int model, int n_basis, int n_branches, const SrFlowBranch* branches) {
    int rows[SR_FLOW_MAX_BRANCHES];
    const int nb = flow_rows(model, n_basis, rows);
    if (!branches || n_branches != nb) return "wrong number of branches for this flow model";
    for (int b = 0; b < nb; ++b)
        if (branches[b].rows != rows[b]) return "wrong branch rows for this flow model";
    return nullptr;
}

size_t flow_head_saved_bytes(int model, long long n, int n_basis) {
    return ((size_t)flow_head_outputs(model, n_basis) * (size_t)n * sizeof(double) + 255) / 256 * 256 + 256;
}

size_t flow_head_workspace_bytes(int model, long long n, int n_basis) {
    const size_t blocks = (size_t)((n + kBlock - 1) / kBlock);
    return ((model == SR_FLOW_DCT ? blocks * n_basis * sizeof(double) : 0) + 255) / 256 * 256 + 256;
}

void launch_flow_head_forward(int model, long long n, int width, int n_basis, int n_branches, const SrFlowBranch* branches, const float* hidden,
                              const float* pts, const float* bases, float* means, float* flow, void* saved, hipStream_t st) {
    FlowK k = flow_params(model, n, width, n_basis, n_branches, branches);
    k.hidden = hidden; k.pts = pts; k.bases = bases; k.means = means; k.flow = flow; k.saved = static_cast<double*>(saved);
    flow_launch<false>(k, flow_head_outputs(model, n_basis), st);
}

void launch_flow_head_backward(int model, long long n, int width, int n_basis, int n_branches, const SrFlowBranch* branches, const float* pts,
                               const float* bases, const void* saved, const float* g_means, const float* g_flow, float* d_pts, float* d_z,
                               float* d_hidden, void* workspace, hipStream_t st) {
    FlowK k = flow_params(model, n, width, n_basis, n_branches, branches);
    k.pts = pts; k.bases = bases; k.saved = const_cast<double*>(static_cast<const double*>(saved));
    k.g_means = g_means; k.g_flow = g_flow; k.d_pts = d_pts; k.d_z = d_z; k.d_hidden = d_hidden; k.partial = static_cast<double*>(workspace);
    flow_launch<true>(k, flow_head_outputs(model, n_basis), st);
}

}  // namespace

}  // namespace sr

// ---- C entry points (include/splatraster.h): what is refused on the host, then the launchers above --------------------
using sr::fail; using sr::check_hip; using sr::any_unaligned4; using sr::StageTimer;

extern "C" {

static int flow_head_check(const char* who, int model, long long n_points, int width, int n_basis, int n_branches, const SrFlowBranch* branches,
                           bool need_bias) {
    if (const char* why = sr::flow_head_shape_error(model, n_points, width, n_basis)) return fail(std::string(who) + ": " + why);
    if (const char* why = sr::flow_head_branch_error(model, n_basis, n_branches, branches)) return fail(std::string(who) + ": " + why);
    for (int b = 0; b < n_branches; ++b) {
        if (!branches[b].weight || (need_bias && !branches[b].bias)) return fail(std::string("null pointer in ") + who + ": a branch's weight or bias");
        if ((reinterpret_cast<uintptr_t>(branches[b].weight) & 15u) || (reinterpret_cast<uintptr_t>(branches[b].bias) & 3u))
            return fail(std::string(who) + ": branch weights must be 16-byte aligned, biases 4-byte");
    }
    return 0;
}

size_t sr_flow_head_saved_bytes(int model, long long n_points, int width, int n_basis) {
    return sr::flow_head_shape_error(model, n_points, width, n_basis) ? 0 : sr::flow_head_saved_bytes(model, n_points, n_basis);
}

size_t sr_flow_head_workspace_bytes(int model, long long n_points, int width, int n_basis) {
    return sr::flow_head_shape_error(model, n_points, width, n_basis) ? 0 : sr::flow_head_workspace_bytes(model, n_points, n_basis);
}

int sr_flow_head_dz_row(int model, int n_basis) { return sr::flow_head_dz_row(model, n_basis); }

int sr_flow_head_forward(int model, long long n_points, int width, int n_basis, int n_branches, const SrFlowBranch* branches,
                         const float* hidden, const float* pts, const float* bases, float* means3D, float* flow, void* saved,
                         void* hip_stream) {
    SR_TRY(flow_head_check("sr_flow_head_forward", model, n_points, width, n_basis, n_branches, branches, true));
    if (n_points == 0) return 0;
    if (!hidden || !pts || !means3D || !flow) return fail("null pointer in sr_flow_head_forward");
    if (model == SR_FLOW_DCT && !bases) return fail("null pointer in sr_flow_head_forward: the DCT model reads bases");
    if ((reinterpret_cast<uintptr_t>(hidden) & 15u) || (model == SR_FLOW_SE3 && (reinterpret_cast<uintptr_t>(flow) & 15u)) ||
        (reinterpret_cast<uintptr_t>(saved) & 7u) || any_unaligned4(pts, bases, means3D, flow))
        return fail("sr_flow_head_forward: hidden (and the 4x4 flow) must be 16-byte aligned, saved 8-byte, the others 4-byte");
    hipStream_t st = static_cast<hipStream_t>(hip_stream);
    { StageTimer t_(0, st); sr::launch_flow_head_forward(model, n_points, width, n_basis, n_branches, branches, hidden, pts, bases, means3D, flow, saved, st); }
    return check_hip(hipGetLastError(), "flow_head_forward");
}

int sr_flow_head_backward(int model, long long n_points, int width, int n_basis, int n_branches, const SrFlowBranch* branches,
                          const float* pts, const float* bases, const void* saved, const float* dL_dmeans3D, const float* dL_dflow,
                          float* dL_dpts, float* dL_dz, float* dL_dhidden, void* workspace, void* hip_stream) {
    SR_TRY(flow_head_check("sr_flow_head_backward", model, n_points, width, n_basis, n_branches, branches, false));
    if (n_points == 0) return 0;
    if (!pts || !saved || !dL_dmeans3D || !dL_dz || !workspace) return fail("null pointer in sr_flow_head_backward");
    if (model == SR_FLOW_DCT && !bases) return fail("null pointer in sr_flow_head_backward: the DCT model reads bases");
    if ((reinterpret_cast<uintptr_t>(dL_dz) & 15u) || (reinterpret_cast<uintptr_t>(dL_dhidden) & 15u) || (reinterpret_cast<uintptr_t>(saved) & 7u) ||
        (reinterpret_cast<uintptr_t>(workspace) & 7u) || any_unaligned4(pts, bases, dL_dmeans3D, dL_dflow, dL_dpts))
        return fail("sr_flow_head_backward: dL_dz and dL_dhidden must be 16-byte aligned, saved and workspace 8-byte, the others 4-byte");
    hipStream_t st = static_cast<hipStream_t>(hip_stream);
    { StageTimer t_(6, st); sr::launch_flow_head_backward(model, n_points, width, n_basis, n_branches, branches, pts, bases, saved, dL_dmeans3D, dL_dflow,
                                                          dL_dpts, dL_dz, dL_dhidden, workspace, st); }
    return check_hip(hipGetLastError(), "flow_head_backward");
}

}  // extern "C"
