// The attention layer of the plane generator's mid block: per plane, with T = h w tokens of width C,
//   t = gamma GroupNorm(x) + beta,  q, k, v = t W^T + b,  P = softmax(q k^T / sqrt(C)),  y = x + (P v) Wo^T + bo.
// The planes of one call share every launch: the kernels take the job table (one SrAttentionJob per plane) as their argument and
// find their plane in blockIdx.y / blockIdx.z, as the convolution kernels do.
//
// Arithmetic.  Inputs, parameters and results are float32 in memory; every product and every sum is a double on the VALU, and a
// result is rounded to float32 once, where it is stored.  What one kernel hands to the next (the group statistics, q, k, v,
// o = P v, the rows' log-sum-exp; in the backward dO, D = dO . o, dq, dk, dv, dt) stays double, in the caller's `saved` buffer
// and workspace.  The layer is tiny (400 x 32 per plane in the reference's configuration): its cost is launches, not FLOPs.
//
// MI355X mapping.  A block is 32 rows (queries, keys or tokens) of <= 64 doubles, staged in LDS with a row of C + 1 doubles (C is
// even, so the 8-byte reads of lanes on different rows fall on different banks).  Eight lanes share a row: in a 32 x 32 score tile
// lane `sub` of row r owns the columns sub + 8 jj, in a 32 x C result the channels sub + 8 cc.  The forward is the streaming
// softmax: a workgroup owns 32 query rows, walks the key / value tiles and keeps (running maximum, running sum, unnormalised
// result) per row; the score tile goes through LDS between the two products.  The backward has one owner for everything it
// writes: query blocks own dq, key blocks own dk and dv, token blocks own dt; the parameter gradients are sums over tokens,
// written as one partial per chunk of token blocks and added in chunk order by a last kernel.  No floating-point atomics.
// The kernels that walk channels are compiled per channel count (C / 8 = 1 .. 8): with constant bounds their loops unroll and
// the LDS reads of a tile are in flight together; with a run-time bound every predicated multiply-add waited for its own read.
// d to_k.bias is written as zeros: the softmax does not see a shift of a whole score row, so the sum over a row of dS is zero.
#include "host_api.h"
#include "reduce.h"

namespace sr {

constexpr int kAttentionBackwardSteps = 6;     // launch_attention_backward(step = 0 .. 5), in this order

namespace {

struct AttnTable { SrAttentionJob job[SR_PLANE_MAX_JOBS]; };

constexpr int kAR = 32;               // rows of a block: queries, keys, tokens
constexpr int kAMaxC = 64;
constexpr int kASl = kAR + 1;         // row of a staged score tile
constexpr int kAMaxChunks = 16;       // partials per plane of the parameter gradients
constexpr int kAStat = 4;             // floats per group in `stats`, as sr_groupnorm_stats writes them

struct AttnArgs {
    int C, groups, T;
    int nblocks;     // ceil(T / 32)
    int bpc;         // token blocks per chunk of the parameter-gradient partials
    int nchunks;     // ceil(nblocks / bpc) <= kAMaxChunks
    double scale;    // 1 / sqrt(C)
    double eps;
};

// `saved` of one plane, in doubles: (mean, rstd) per group, then q, k, v, o as [T, C] and the log-sum-exp [T]
__host__ __device__ inline size_t saved_doubles(int C, int groups, int T) { return 2 * (size_t)groups + 4 * (size_t)T * C + T; }
// the backward's workspace of one plane, in doubles: dO, dq, dk, dv, dt as [T, C], D [T], then `nchunks` partials of
// dWo, dWq, dWk, dWv [C, C] and dbo, dbq, dbv, sum dt, sum dt xhat [C]
__host__ __device__ inline size_t part_doubles(int C) { return 4 * (size_t)C * C + 5 * (size_t)C; }
__host__ __device__ inline size_t ws_doubles(int C, int T, int nchunks) { return 5 * (size_t)T * C + T + nchunks * part_doubles(C); }

struct Saved { const double *gs, *q, *k, *v; double *o, *lse; };
__device__ __forceinline__ Saved saved_of(const SrAttentionJob& J, const AttnArgs& a) {
    double* s = static_cast<double*>(J.saved);
    const size_t tc = (size_t)a.T * a.C;
    Saved r;
    r.gs = s; r.q = s + 2 * a.groups; r.k = r.q + tc; r.v = r.k + tc; r.o = s + 2 * a.groups + 3 * tc; r.lse = r.o + tc;
    return r;
}
struct Work { double *d_o, *dq, *dk, *dv, *dt, *D, *part; };
__device__ __forceinline__ Work work_of(double* ws, int plane, const AttnArgs& a) {
    double* s = ws + (size_t)plane * ws_doubles(a.C, a.T, a.nchunks);
    const size_t tc = (size_t)a.T * a.C;
    Work r;
    r.d_o = s; r.dq = s + tc; r.dk = s + 2 * tc; r.dv = s + 3 * tc; r.dt = s + 4 * tc; r.D = s + 5 * tc; r.part = r.D + a.T;
    return r;
}

// rows row0 .. row0 + 31 of a [T, C] array of doubles into LDS (row C + 1); rows past T are zero
__device__ __forceinline__ void stage_rows(double* dst, const double* __restrict__ src, int row0, const AttnArgs& a) {
    const int ld = a.C + 1, nc = a.C >> 3, r = threadIdx.x >> 3, sub = threadIdx.x & 7;
    const bool inside = row0 + r < a.T;
    const double* __restrict__ p = src + (size_t)(inside ? row0 + r : 0) * a.C + sub;
    double v[8];
#pragma unroll
    for (int cc = 0; cc < 8; ++cc) v[cc] = (inside && cc < nc) ? p[8 * cc] : 0.0;
#pragma unroll
    for (int cc = 0; cc < 8; ++cc)
        if (cc < nc) dst[r * ld + sub + 8 * cc] = v[cc];
}
// tokens tok0 .. tok0 + 31 of a [C, T] array of floats, transposed into LDS rows; tokens past T are zero
__device__ __forceinline__ void stage_cols(double* dst, const float* __restrict__ src, int tok0, const AttnArgs& a) {
    const int ld = a.C + 1, nc = a.C >> 3, r = threadIdx.x & (kAR - 1), c0 = threadIdx.x >> 5;
    const bool inside = tok0 + r < a.T;
    float v[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) v[i] = (inside && i < nc) ? src[(size_t)(c0 + 8 * i) * a.T + tok0 + r] : 0.f;
#pragma unroll
    for (int i = 0; i < 8; ++i)
        if (i < nc) dst[r * ld + c0 + 8 * i] = (double)v[i];
}
// the normalised tokens t = gamma xhat + beta of tok0 .. tok0 + 31 into LDS rows; tokens past T are zero
__device__ __forceinline__ void stage_tokens(double* dst, const SrAttentionJob& J, const double* __restrict__ gs, int tok0, const AttnArgs& a) {
    const int ld = a.C + 1, nc = a.C >> 3, cg = a.C / a.groups, r = threadIdx.x & (kAR - 1), c0 = threadIdx.x >> 5;
    const bool inside = tok0 + r < a.T;
    float v[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) v[i] = (inside && i < nc) ? J.x[(size_t)(c0 + 8 * i) * a.T + tok0 + r] : 0.f;
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        if (i < nc) {
            const int c = c0 + 8 * i, g = c / cg;
            dst[r * ld + c] = inside ? ((double)v[i] - gs[2 * g]) * gs[2 * g + 1] * (double)J.gamma[c] + (double)J.beta[c] : 0.0;
        }
    }
}
// a [C, C] matrix of floats into LDS rows of C + 1 floats
__device__ __forceinline__ void stage_matrix(float* dst, const float* __restrict__ src, int C) {
    const int nc = C >> 3, r = threadIdx.x >> 3, sub = threadIdx.x & 7;
#pragma unroll
    for (int half = 0; half < 2; ++half) {
        const int o = r + 32 * half;
        if (o < C) {
#pragma unroll
            for (int cc = 0; cc < 8; ++cc)
                if (cc < nc) dst[o * (C + 1) + sub + 8 * cc] = src[o * C + sub + 8 * cc];
        }
    }
}
// sum over the eight lanes of a row; the same bits in each of them
__device__ __forceinline__ double row_sum(double v) {
    v += __shfl_xor(v, 1); v += __shfl_xor(v, 2); v += __shfl_xor(v, 4);
    return v;
}
__device__ __forceinline__ double row_max(double v) {
    v = fmax(v, __shfl_xor(v, 1)); v = fmax(v, __shfl_xor(v, 2)); v = fmax(v, __shfl_xor(v, 4));
    return v;
}
// acc[cc] += sum over the 32 staged rows of A[r][o] B[r][c],  o = tid / 4,  c = tid % 4 + 4 cc
__device__ __forceinline__ void outer_acc(const double* A, const double* B, int C, double (&acc)[16]) {
    const int o = threadIdx.x >> 2, c0 = threadIdx.x & 3, ld = C + 1;
    if (o >= C) return;
#pragma unroll 4
    for (int r = 0; r < kAR; ++r) {
        const double av = A[r * ld + o];
#pragma unroll
        for (int cc = 0; cc < 16; ++cc)
            if (c0 + 4 * cc < C) acc[cc] += av * B[r * ld + c0 + 4 * cc];
    }
}
__device__ __forceinline__ void outer_store(double* __restrict__ dst, int C, const double (&acc)[16]) {
    const int o = threadIdx.x >> 2, c0 = threadIdx.x & 3;
    if (o >= C) return;
#pragma unroll
    for (int cc = 0; cc < 16; ++cc)
        if (c0 + 4 * cc < C) dst[o * C + c0 + 4 * cc] = acc[cc];
}

// ---- forward ----------------------------------------------------------------------------------------------------------------
// grid (groups, planes): mean and 1 / sqrt(var + eps) of a group's (C / groups) T contiguous values, two passes in double
__global__ __launch_bounds__(kBlock) void k_attn_stats(const AttnTable t, const AttnArgs a) {
    __shared__ double red[kBlock];
    const SrAttentionJob& J = t.job[blockIdx.y];
    const int g = blockIdx.x, n = (a.C / a.groups) * a.T;
    const float* __restrict__ xg = J.x + (size_t)g * n;
    double s = 0.0;
    for (int i = threadIdx.x; i < n; i += kBlock) s += (double)xg[i];
    const double mean = block_tree_sum<double, kBlock>(s, red) / (double)n;
    double q = 0.0;
    for (int i = threadIdx.x; i < n; i += kBlock) { const double d = (double)xg[i] - mean; q += d * d; }
    const double rstd = 1.0 / sqrt(block_tree_sum<double, kBlock>(q, red) / (double)n + a.eps);
    if (threadIdx.x == 0) {
        double* gs = static_cast<double*>(J.saved);
        gs[2 * g] = mean; gs[2 * g + 1] = rstd;
        float* o = J.stats + kAStat * g;
        const float mean_hi = (float)mean;
        o[0] = mean_hi; o[1] = (float)rstd; o[2] = (float)(mean - (double)mean_hi); o[3] = 0.f;
    }
}

// grid (token blocks, planes): q, k, v of 32 tokens.  Thread (r = tid % 32, og = tid / 32) owns the outputs og + 8 i of token r.
template <int NC>
__global__ __launch_bounds__(kBlock) void k_attn_qkv(const AttnTable t, const AttnArgs a_in) {
    constexpr int C = 8 * NC, ld = C + 1, nc = NC;
    AttnArgs a = a_in;
    a.C = C;
    __shared__ double tl[kAR * ld];
    __shared__ float wl[C * ld];
    const SrAttentionJob& J = t.job[blockIdx.y];
    const Saved S = saved_of(J, a);
    const int r = threadIdx.x & (kAR - 1), og = threadIdx.x >> 5, tok = blockIdx.x * kAR + r;
    stage_tokens(tl, J, S.gs, blockIdx.x * kAR, a);
    double* const dst[3] = {const_cast<double*>(S.q), const_cast<double*>(S.k), const_cast<double*>(S.v)};
    const float* const wsrc[3] = {J.wq, J.wk, J.wv};
    const float* const bsrc[3] = {J.bq, J.bk, J.bv};
#pragma unroll
    for (int m = 0; m < 3; ++m) {
        __syncthreads();
        stage_matrix(wl, wsrc[m], C);
        __syncthreads();
        if (tok < a.T) {
            for (int o = og; o < C; o += 8) {
                double acc = 0.0;
#pragma unroll 8
                for (int c = 0; c < C; ++c) acc += tl[r * ld + c] * (double)wl[o * ld + c];
                dst[m][(size_t)tok * C + o] = acc + (double)bsrc[m][o];
            }
        }
    }
}

// grid (query blocks, planes): the streaming softmax, o and the log-sum-exp, then y = x + o Wo^T + bo
template <int NC>
__global__ __launch_bounds__(kBlock) void k_attn_fwd(const AttnTable t, const AttnArgs a_in) {
    constexpr int C = 8 * NC, ld = C + 1, nc = NC;
    AttnArgs a = a_in;
    a.C = C;
    __shared__ double Ql[kAR * ld], Kl[kAR * ld], Vl[kAR * ld], Sl[kAR * kASl];
    const SrAttentionJob& J = t.job[blockIdx.y];
    const Saved S = saved_of(J, a);
    const int T = a.T, r = threadIdx.x >> 3, sub = threadIdx.x & 7;
    const int q0 = blockIdx.x * kAR, row = q0 + r;
    stage_rows(Ql, S.q, q0, a);
    double m = -INFINITY, l = 0.0, acc[8];
#pragma unroll
    for (int cc = 0; cc < 8; ++cc) acc[cc] = 0.0;
    for (int k0 = 0; k0 < T; k0 += kAR) {
        __syncthreads();
        stage_rows(Kl, S.k, k0, a);
        stage_rows(Vl, S.v, k0, a);
        __syncthreads();
        double s[4] = {0.0, 0.0, 0.0, 0.0};
#pragma unroll 8
        for (int c = 0; c < C; ++c) {
            const double qv = Ql[r * ld + c];
#pragma unroll
            for (int jj = 0; jj < 4; ++jj) s[jj] += qv * Kl[(sub + 8 * jj) * ld + c];
        }
        double tmax = -INFINITY;
#pragma unroll
        for (int jj = 0; jj < 4; ++jj) {
            s[jj] = k0 + sub + 8 * jj < T ? s[jj] * a.scale : -INFINITY;
            tmax = fmax(tmax, s[jj]);
        }
        const double mn = fmax(m, row_max(tmax));      // finite: key k0 is inside
        const double corr = exp(m - mn);
        double ps = 0.0;
#pragma unroll
        for (int jj = 0; jj < 4; ++jj) {
            const double p = exp(s[jj] - mn);
            Sl[r * kASl + sub + 8 * jj] = p;
            ps += p;
        }
        l = l * corr + row_sum(ps);
        m = mn;
#pragma unroll
        for (int cc = 0; cc < 8; ++cc) acc[cc] *= corr;
        __syncthreads();
#pragma unroll 8
        for (int j = 0; j < kAR; ++j) {
            const double p = Sl[r * kASl + j];
#pragma unroll
            for (int cc = 0; cc < 8; ++cc)
                if (cc < nc) acc[cc] += p * Vl[j * ld + sub + 8 * cc];
        }
    }
    __syncthreads();
    float* wl = reinterpret_cast<float*>(Kl);          // 32 rows of doubles hold the C <= 64 rows of floats
    static_assert(kAR * sizeof(double) >= C * sizeof(float), "Wo is staged over the key tile");
    stage_matrix(wl, J.wo, C);
#pragma unroll
    for (int cc = 0; cc < 8; ++cc) {
        if (cc < nc) {
            const double ov = acc[cc] / l;
            Ql[r * ld + sub + 8 * cc] = ov;
            if (row < T) S.o[(size_t)row * C + sub + 8 * cc] = ov;
        }
    }
    if (sub == 0 && row < T) S.lse[row] = m + log(l);
    __syncthreads();
    if (row < T) {
#pragma unroll
        for (int cc = 0; cc < 8; ++cc) {
            if (cc < nc) {
                const int c = sub + 8 * cc;
                double y = 0.0;
#pragma unroll 8
                for (int c2 = 0; c2 < C; ++c2) y += Ql[r * ld + c2] * (double)wl[c * ld + c2];
                const size_t i = (size_t)c * T + row;
                J.out[i] = (float)(y + (double)J.bo[c] + (double)J.x[i]);
            }
        }
    }
}

// ---- backward ---------------------------------------------------------------------------------------------------------------
// grid (chunks, planes): dO = dy Wo and D = dO . o per token; this chunk's partial of dWo = dy^T o and dbo = sum dy
template <int NC>
__global__ __launch_bounds__(kBlock) void k_attn_bwd_out(const AttnTable t, const AttnArgs a_in, double* __restrict__ ws) {
    constexpr int C = 8 * NC, ld = C + 1, nc = NC;
    AttnArgs a = a_in;
    a.C = C;
    __shared__ double dyl[kAR * ld], ol[kAR * ld];
    __shared__ float wl[C * ld];
    const SrAttentionJob& J = t.job[blockIdx.y];
    const Saved S = saved_of(J, a);
    const Work W = work_of(ws, blockIdx.y, a);
    const int T = a.T, r = threadIdx.x >> 3, sub = threadIdx.x & 7;
    double wacc[16], bacc = 0.0;
#pragma unroll
    for (int i = 0; i < 16; ++i) wacc[i] = 0.0;
    stage_matrix(wl, J.wo, C);
    for (int b = blockIdx.x * a.bpc; b < min((int)(blockIdx.x + 1) * a.bpc, a.nblocks); ++b) {
        const int tok0 = b * kAR, row = tok0 + r;
        __syncthreads();
        stage_cols(dyl, J.dy, tok0, a);
        stage_rows(ol, S.o, tok0, a);
        __syncthreads();
        double d = 0.0;
#pragma unroll
        for (int cc = 0; cc < 8; ++cc) {
            if (cc < nc) {
                const int c2 = sub + 8 * cc;
                double v = 0.0;
#pragma unroll 8
                for (int c = 0; c < C; ++c) v += dyl[r * ld + c] * (double)wl[c * ld + c2];
                if (row < T) W.d_o[(size_t)row * C + c2] = v;
                d += v * ol[r * ld + c2];
            }
        }
        d = row_sum(d);
        if (sub == 0 && row < T) W.D[row] = d;
        outer_acc(dyl, ol, C, wacc);
        if (threadIdx.x < C)
            for (int i = 0; i < kAR; ++i) bacc += dyl[i * ld + threadIdx.x];
    }
    double* part = W.part + (size_t)blockIdx.x * part_doubles(C);
    outer_store(part, C, wacc);
    if (threadIdx.x < C) part[4 * C * C + threadIdx.x] = bacc;
}

// grid (query blocks, planes): dq of 32 query rows over every key tile.  P = exp(s - lse), dS = P (dO . v - D).
template <int NC>
__global__ __launch_bounds__(kBlock) void k_attn_bwd_dq(const AttnTable t, const AttnArgs a_in, double* __restrict__ ws) {
    constexpr int C = 8 * NC, ld = C + 1, nc = NC;
    AttnArgs a = a_in;
    a.C = C;
    __shared__ double Ql[kAR * ld], Gl[kAR * ld], Kl[kAR * ld], Vl[kAR * ld], Sl[kAR * kASl];
    const SrAttentionJob& J = t.job[blockIdx.y];
    const Saved S = saved_of(J, a);
    const Work W = work_of(ws, blockIdx.y, a);
    const int T = a.T, r = threadIdx.x >> 3, sub = threadIdx.x & 7;
    const int q0 = blockIdx.x * kAR, row = q0 + r;
    stage_rows(Ql, S.q, q0, a);
    stage_rows(Gl, W.d_o, q0, a);
    const double lse = row < T ? S.lse[row] : 0.0, D = row < T ? W.D[row] : 0.0;
    double acc[8];
#pragma unroll
    for (int cc = 0; cc < 8; ++cc) acc[cc] = 0.0;
    for (int k0 = 0; k0 < T; k0 += kAR) {
        __syncthreads();
        stage_rows(Kl, S.k, k0, a);
        stage_rows(Vl, S.v, k0, a);
        __syncthreads();
        double s[4] = {0.0, 0.0, 0.0, 0.0}, dp[4] = {0.0, 0.0, 0.0, 0.0};
#pragma unroll 8
        for (int c = 0; c < C; ++c) {
            const double qv = Ql[r * ld + c], gv = Gl[r * ld + c];
#pragma unroll
            for (int jj = 0; jj < 4; ++jj) {
                s[jj] += qv * Kl[(sub + 8 * jj) * ld + c];
                dp[jj] += gv * Vl[(sub + 8 * jj) * ld + c];
            }
        }
#pragma unroll
        for (int jj = 0; jj < 4; ++jj) {
            const double p = (row < T && k0 + sub + 8 * jj < T) ? exp(s[jj] * a.scale - lse) : 0.0;
            Sl[r * kASl + sub + 8 * jj] = p * (dp[jj] - D);
        }
        __syncthreads();
#pragma unroll 8
        for (int j = 0; j < kAR; ++j) {
            const double ds = Sl[r * kASl + j];
#pragma unroll
            for (int cc = 0; cc < 8; ++cc)
                if (cc < nc) acc[cc] += ds * Kl[j * ld + sub + 8 * cc];
        }
    }
    if (row < T) {
#pragma unroll
        for (int cc = 0; cc < 8; ++cc)
            if (cc < nc) W.dq[(size_t)row * C + sub + 8 * cc] = acc[cc] * a.scale;
    }
}

// grid (key blocks, planes): dk and dv of 32 key rows over every query tile.  Thread (jr = tid / 8, sub) owns the queries
// sub + 8 ii of a tile in the score products and the channels sub + 8 cc of key jr in the results.
template <int NC>
__global__ __launch_bounds__(kBlock) void k_attn_bwd_dkv(const AttnTable t, const AttnArgs a_in, double* __restrict__ ws) {
    constexpr int C = 8 * NC, ld = C + 1, nc = NC;
    AttnArgs a = a_in;
    a.C = C;
    __shared__ double Kl[kAR * ld], Vl[kAR * ld], Ql[kAR * ld], Gl[kAR * ld], Pl[kAR * kASl], Dl[kAR * kASl];
    __shared__ double lsel[kAR], dl[kAR];
    const SrAttentionJob& J = t.job[blockIdx.y];
    const Saved S = saved_of(J, a);
    const Work W = work_of(ws, blockIdx.y, a);
    const int T = a.T, jr = threadIdx.x >> 3, sub = threadIdx.x & 7;
    const int j0 = blockIdx.x * kAR, key = j0 + jr;
    stage_rows(Kl, S.k, j0, a);
    stage_rows(Vl, S.v, j0, a);
    double ak[8], av[8];
#pragma unroll
    for (int cc = 0; cc < 8; ++cc) { ak[cc] = 0.0; av[cc] = 0.0; }
    for (int i0 = 0; i0 < T; i0 += kAR) {
        __syncthreads();
        stage_rows(Ql, S.q, i0, a);
        stage_rows(Gl, W.d_o, i0, a);
        if (threadIdx.x < kAR) {
            const int i = i0 + threadIdx.x;
            lsel[threadIdx.x] = i < T ? S.lse[i] : 0.0;
            dl[threadIdx.x] = i < T ? W.D[i] : 0.0;
        }
        __syncthreads();
        double s[4] = {0.0, 0.0, 0.0, 0.0}, dp[4] = {0.0, 0.0, 0.0, 0.0};
#pragma unroll 8
        for (int c = 0; c < C; ++c) {
            const double kv = Kl[jr * ld + c], vv = Vl[jr * ld + c];
#pragma unroll
            for (int ii = 0; ii < 4; ++ii) {
                s[ii] += kv * Ql[(sub + 8 * ii) * ld + c];
                dp[ii] += vv * Gl[(sub + 8 * ii) * ld + c];
            }
        }
#pragma unroll
        for (int ii = 0; ii < 4; ++ii) {
            const int i = sub + 8 * ii;
            const double p = (key < T && i0 + i < T) ? exp(s[ii] * a.scale - lsel[i]) : 0.0;
            Pl[jr * kASl + i] = p;
            Dl[jr * kASl + i] = p * (dp[ii] - dl[i]);
        }
        __syncthreads();
#pragma unroll 8
        for (int i = 0; i < kAR; ++i) {
            const double p = Pl[jr * kASl + i], ds = Dl[jr * kASl + i];
#pragma unroll
            for (int cc = 0; cc < 8; ++cc) {
                if (cc < nc) {
                    av[cc] += p * Gl[i * ld + sub + 8 * cc];
                    ak[cc] += ds * Ql[i * ld + sub + 8 * cc];
                }
            }
        }
    }
    if (key < T) {
#pragma unroll
        for (int cc = 0; cc < 8; ++cc) {
            if (cc < nc) {
                W.dk[(size_t)key * C + sub + 8 * cc] = ak[cc] * a.scale;
                W.dv[(size_t)key * C + sub + 8 * cc] = av[cc];
            }
        }
    }
}

// grid (chunks, planes): dt = dq Wq + dk Wk + dv Wv per token; this chunk's partials of dW = d^T t and db = sum d for the
// three projections (none for the key bias), and of sum dt and sum dt xhat per channel
template <int NC>
__global__ __launch_bounds__(kBlock) void k_attn_bwd_proj(const AttnTable t, const AttnArgs a_in, double* __restrict__ ws) {
    constexpr int C = 8 * NC, ld = C + 1, nc = NC;
    AttnArgs a = a_in;
    a.C = C;
    __shared__ double tl[kAR * ld], gl[kAR * ld];
    __shared__ float wl[C * ld];
    const SrAttentionJob& J = t.job[blockIdx.y];
    const Saved S = saved_of(J, a);
    const Work W = work_of(ws, blockIdx.y, a);
    const int T = a.T, cg = C / a.groups, r = threadIdx.x >> 3, sub = threadIdx.x & 7;
    double wacc[3][16], bacc[3] = {0.0, 0.0, 0.0}, s1 = 0.0, s2 = 0.0;
#pragma unroll
    for (int m = 0; m < 3; ++m)
#pragma unroll
        for (int i = 0; i < 16; ++i) wacc[m][i] = 0.0;
    const double* const gsrc[3] = {W.dq, W.dk, W.dv};
    const float* const wsrc[3] = {J.wq, J.wk, J.wv};
    for (int b = blockIdx.x * a.bpc; b < min((int)(blockIdx.x + 1) * a.bpc, a.nblocks); ++b) {
        const int tok0 = b * kAR, row = tok0 + r;
        double dt[8];
#pragma unroll
        for (int cc = 0; cc < 8; ++cc) dt[cc] = 0.0;
        __syncthreads();
        stage_tokens(tl, J, S.gs, tok0, a);
#pragma unroll
        for (int m = 0; m < 3; ++m) {
            __syncthreads();
            stage_rows(gl, gsrc[m], tok0, a);
            stage_matrix(wl, wsrc[m], C);
            __syncthreads();
#pragma unroll 8
            for (int o = 0; o < C; ++o) {
                const double gv = gl[r * ld + o];
#pragma unroll
                for (int cc = 0; cc < 8; ++cc)
                    if (cc < nc) dt[cc] += gv * (double)wl[o * ld + sub + 8 * cc];
            }
            outer_acc(gl, tl, C, wacc[m]);
            if (m != 1 && threadIdx.x < C)
                for (int i = 0; i < kAR; ++i) bacc[m] += gl[i * ld + threadIdx.x];
        }
        __syncthreads();
#pragma unroll
        for (int cc = 0; cc < 8; ++cc) {
            if (cc < nc) {
                gl[r * ld + sub + 8 * cc] = dt[cc];            // rows past T: their d rows are zero, so is dt
                if (row < T) W.dt[(size_t)row * C + sub + 8 * cc] = dt[cc];
            }
        }
        __syncthreads();
        if (threadIdx.x < C) {
            const int c = threadIdx.x, g = c / cg;
            const double mean = S.gs[2 * g], rstd = S.gs[2 * g + 1];
            for (int i = 0; i < kAR && tok0 + i < T; ++i) {
                const double v = gl[i * ld + c], xh = ((double)J.x[(size_t)c * T + tok0 + i] - mean) * rstd;
                s1 += v; s2 += v * xh;
            }
        }
    }
    double* part = W.part + (size_t)blockIdx.x * part_doubles(C);
    const int cc2 = C * C;
#pragma unroll
    for (int m = 0; m < 3; ++m) outer_store(part + (m + 1) * cc2, C, wacc[m]);
    if (threadIdx.x < C) {
        part[4 * cc2 + C + threadIdx.x] = bacc[0];
        part[4 * cc2 + 2 * C + threadIdx.x] = bacc[2];
        part[4 * cc2 + 3 * C + threadIdx.x] = s1;
        part[4 * cc2 + 4 * C + threadIdx.x] = s2;
    }
}

// grid (ceil((4 C C + 6 C) / 256), planes): the chunks' partials added in chunk order; the key bias gets its zeros
__global__ __launch_bounds__(kBlock) void k_attn_bwd_reduce(const AttnTable t, const AttnArgs a, const double* __restrict__ ws) {
    const SrAttentionJob& J = t.job[blockIdx.y];
    const int C = a.C, cc2 = C * C, len = (int)part_doubles(C);
    const int idx = blockIdx.x * kBlock + threadIdx.x;
    if (idx >= len + C) return;
    if (idx >= len) { J.dbk[idx - len] = 0.f; return; }
    const double* p = ws + (size_t)blockIdx.y * ws_doubles(C, a.T, a.nchunks) + 5 * (size_t)a.T * C + a.T + idx;
    double s = 0.0;
    for (int c = 0; c < a.nchunks; ++c) s += p[(size_t)c * len];
    const float v = (float)s;
    if (idx < cc2) J.dwo[idx] = v;
    else if (idx < 2 * cc2) J.dwq[idx - cc2] = v;
    else if (idx < 3 * cc2) J.dwk[idx - 2 * cc2] = v;
    else if (idx < 4 * cc2) J.dwv[idx - 3 * cc2] = v;
    else if (idx < 4 * cc2 + C) J.dbo[idx - 4 * cc2] = v;
    else if (idx < 4 * cc2 + 2 * C) J.dbq[idx - 4 * cc2 - C] = v;
    else if (idx < 4 * cc2 + 3 * C) J.dbv[idx - 4 * cc2 - 2 * C] = v;
    else if (idx < 4 * cc2 + 4 * C) J.dbeta[idx - 4 * cc2 - 3 * C] = v;
    else J.dgamma[idx - 4 * cc2 - 4 * C] = v;
}

// grid (ceil(T / 256), channels, planes): dx = dy + rstd (gamma dt - (S1 + xhat S2) / n), S1 = sum gamma dt and S2 = sum gamma dt
// xhat over the channel's group, from the partials in channel, then chunk order
__global__ __launch_bounds__(kBlock) void k_attn_bwd_dx(const AttnTable t, const AttnArgs a, const double* __restrict__ ws) {
    __shared__ double cs1[kAMaxC], cs2[kAMaxC], tot[2];
    const SrAttentionJob& J = t.job[blockIdx.z];
    const Saved S = saved_of(J, a);
    const int C = a.C, T = a.T, cg = C / a.groups, c = blockIdx.y, g = c / cg, tid = threadIdx.x, len = (int)part_doubles(C);
    const double* base = ws + (size_t)blockIdx.z * ws_doubles(C, T, a.nchunks);
    const double* dt = base + 4 * (size_t)T * C;
    const double* part = base + 5 * (size_t)T * C + T;
    if (tid < cg) {
        const double* p = part + 4 * C * C + 3 * C + g * cg + tid;
        double u = 0.0, v = 0.0;
        for (int k = 0; k < a.nchunks; ++k) { u += p[(size_t)k * len]; v += p[(size_t)k * len + C]; }
        cs1[tid] = u; cs2[tid] = v;
    }
    __syncthreads();
    if (tid == 0) {
        double u = 0.0, v = 0.0;
        for (int k = 0; k < cg; ++k) { const double gm = J.gamma[g * cg + k]; u += gm * cs1[k]; v += gm * cs2[k]; }
        tot[0] = u; tot[1] = v;
    }
    __syncthreads();
    const int tok = blockIdx.x * kBlock + tid;
    if (tok >= T) return;
    const double mean = S.gs[2 * g], rstd = S.gs[2 * g + 1], inv_n = 1.0 / ((double)cg * (double)T), gam = J.gamma[c];
    const size_t i = (size_t)c * T + tok;
    const double xh = ((double)J.x[i] - mean) * rstd;
    J.dx[i] = (float)((double)J.dy[i] + rstd * (dt[(size_t)tok * C + c] * gam - (tot[0] + xh * tot[1]) * inv_n));
}

AttnTable make_table(int n, const SrAttentionJob* jobs) {
    AttnTable t = {};
    for (int i = 0; i < n; ++i) t.job[i] = jobs[i];
    return t;
}

// the kernels that walk channels are compiled per channel count (C / 8 = 1 .. 8): their loops have constant bounds
#define SR_ATTN_LAUNCH(kernel, nc, grid, st, ...)                                                           \
    switch (nc) {                                                                                           \
    case 1: hipLaunchKernelGGL(kernel<1>, grid, dim3(kBlock), 0, st, __VA_ARGS__); break;                   \
    case 2: hipLaunchKernelGGL(kernel<2>, grid, dim3(kBlock), 0, st, __VA_ARGS__); break;                   \
    case 3: hipLaunchKernelGGL(kernel<3>, grid, dim3(kBlock), 0, st, __VA_ARGS__); break;                   \
    case 4: hipLaunchKernelGGL(kernel<4>, grid, dim3(kBlock), 0, st, __VA_ARGS__); break;                   \
    case 5: hipLaunchKernelGGL(kernel<5>, grid, dim3(kBlock), 0, st, __VA_ARGS__); break;                   \
    case 6: hipLaunchKernelGGL(kernel<6>, grid, dim3(kBlock), 0, st, __VA_ARGS__); break;                   \
    case 7: hipLaunchKernelGGL(kernel<7>, grid, dim3(kBlock), 0, st, __VA_ARGS__); break;                   \
    default: hipLaunchKernelGGL(kernel<8>, grid, dim3(kBlock), 0, st, __VA_ARGS__); break;                  \
    }

AttnArgs make_args(int channels, int groups, int h, int w, float eps) {
    AttnArgs a = {};
    a.C = channels; a.groups = groups; a.T = h * w;
    a.nblocks = (a.T + kAR - 1) / kAR;
    a.bpc = (a.nblocks + kAMaxChunks - 1) / kAMaxChunks;
    a.nchunks = (a.nblocks + a.bpc - 1) / a.bpc;
    a.scale = 1.0 / sqrt((double)channels);
    a.eps = (double)eps;
    return a;
}

const char* attention_shape_error(int channels, int groups, int h, int w) {
    if (channels < 8 || channels > kAMaxC || channels % 8 != 0) return "channels must be a multiple of 8 in 8..64";
    if (groups < 1 || channels % groups != 0) return "groups must divide channels";
    if (h < 1 || w < 1 || (long long)h * w > 4096) return "height * width must be 1..4096 tokens";
    if ((long long)(channels / groups) * h * w < 2) return "a group needs at least two values (channels / groups * height * width >= 2)";
    return nullptr;
}
size_t attention_saved_bytes(int n_planes, int channels, int groups, int h, int w) {
    return (size_t)n_planes * saved_doubles(channels, groups, h * w) * sizeof(double);
}
size_t attention_backward_workspace(int n_planes, int channels, int h, int w) {
    // room for min(token blocks, kAMaxChunks) partials: never less than the split uses, and monotone in the token count
    const int nblocks = (h * w + kAR - 1) / kAR;
    return (size_t)n_planes * ws_doubles(channels, h * w, nblocks < kAMaxChunks ? nblocks : kAMaxChunks) * sizeof(double);
}

void launch_attention_stats(int n, const SrAttentionJob* jobs, int channels, int groups, int h, int w, float eps, hipStream_t st) {
    hipLaunchKernelGGL(k_attn_stats, dim3(groups, n), dim3(kBlock), 0, st, make_table(n, jobs), make_args(channels, groups, h, w, eps));
}
void launch_attention_qkv(int n, const SrAttentionJob* jobs, int channels, int groups, int h, int w, float eps, hipStream_t st) {
    const AttnArgs a = make_args(channels, groups, h, w, eps);
    SR_ATTN_LAUNCH(k_attn_qkv, channels >> 3, dim3(a.nblocks, n), st, make_table(n, jobs), a);
}
void launch_attention_softmax(int n, const SrAttentionJob* jobs, int channels, int groups, int h, int w, float eps, hipStream_t st) {
    const AttnArgs a = make_args(channels, groups, h, w, eps);
    SR_ATTN_LAUNCH(k_attn_fwd, channels >> 3, dim3(a.nblocks, n), st, make_table(n, jobs), a);
}
void launch_attention_backward(int step, int n, const SrAttentionJob* jobs, int channels, int groups, int h, int w, float eps, void* ws,
                               hipStream_t st) {
    const AttnArgs a = make_args(channels, groups, h, w, eps);
    const AttnTable t = make_table(n, jobs);
    double* d = static_cast<double*>(ws);
    switch (step) {
    case 0: SR_ATTN_LAUNCH(k_attn_bwd_out, channels >> 3, dim3(a.nchunks, n), st, t, a, d); break;
    case 1: SR_ATTN_LAUNCH(k_attn_bwd_dq, channels >> 3, dim3(a.nblocks, n), st, t, a, d); break;
    case 2: SR_ATTN_LAUNCH(k_attn_bwd_dkv, channels >> 3, dim3(a.nblocks, n), st, t, a, d); break;
    case 3: SR_ATTN_LAUNCH(k_attn_bwd_proj, channels >> 3, dim3(a.nchunks, n), st, t, a, d); break;
    case 4: hipLaunchKernelGGL(k_attn_bwd_reduce, dim3(((int)part_doubles(channels) + channels + kBlock - 1) / kBlock, n), dim3(kBlock), 0, st, t, a, d);
            break;
    default: hipLaunchKernelGGL(k_attn_bwd_dx, dim3((a.T + kBlock - 1) / kBlock, channels, n), dim3(kBlock), 0, st, t, a, d); break;
    }
}

}  // namespace

}  // namespace sr

// ---- C entry points (include/splatraster.h): what is refused on the host, then the launchers above --------------------
using sr::fail; using sr::check_hip; using sr::StageTimer;

extern "C" {

static int attention_check(const char* who, int n_planes, const SrAttentionJob* jobs, int channels, int groups, int height, int width) {
    if (!jobs) return fail(std::string("null pointer in ") + who + ": jobs");
    if (n_planes < 1 || n_planes > SR_PLANE_MAX_JOBS) return fail(std::string("bad arguments to ") + who + ": n_planes must be 1 .. SR_PLANE_MAX_JOBS (8)");
    if (const char* why = sr::attention_shape_error(channels, groups, height, width)) return fail(std::string(who) + ": " + why);
    return 0;
}

size_t sr_attention_saved_bytes(int n_planes, int channels, int groups, int height, int width) {
    if (n_planes < 1 || n_planes > SR_PLANE_MAX_JOBS || sr::attention_shape_error(channels, groups, height, width)) return 0;
    return sr::attention_saved_bytes(n_planes, channels, groups, height, width);
}

size_t sr_attention_backward_workspace(int n_planes, int channels, int groups, int height, int width) {
    if (n_planes < 1 || n_planes > SR_PLANE_MAX_JOBS || sr::attention_shape_error(channels, groups, height, width)) return 0;
    return sr::attention_backward_workspace(n_planes, channels, height, width);
}

int sr_attention_forward(int n_planes, const SrAttentionJob* jobs, int channels, int groups, int height, int width, float eps,
                         void* hip_stream) {
    SR_TRY(attention_check("sr_attention_forward", n_planes, jobs, channels, groups, height, width));
    for (int i_ = 0; i_ < n_planes; ++i_) {
        const SrAttentionJob& j = jobs[i_];
        SR_PLANE_NEED("sr_attention_forward", j.x && j.gamma && j.beta && j.stats && j.wq && j.bq && j.wk && j.bk && j.wv && j.bv && j.wo && j.bo &&
                      j.out && j.saved);
    }
    hipStream_t st = static_cast<hipStream_t>(hip_stream);
    { StageTimer t_(0, st); sr::launch_attention_stats(n_planes, jobs, channels, groups, height, width, eps, st); }
    { StageTimer t_(0, st); sr::launch_attention_qkv(n_planes, jobs, channels, groups, height, width, eps, st); }
    { StageTimer t_(0, st); sr::launch_attention_softmax(n_planes, jobs, channels, groups, height, width, eps, st); }
    return check_hip(hipGetLastError(), "attention_forward");
}

int sr_attention_backward(int n_planes, const SrAttentionJob* jobs, int channels, int groups, int height, int width, float eps,
                          void* workspace, void* hip_stream) {
    SR_TRY(attention_check("sr_attention_backward", n_planes, jobs, channels, groups, height, width));
    if (!workspace) return fail("null pointer in sr_attention_backward: workspace");
    for (int i_ = 0; i_ < n_planes; ++i_) {
        const SrAttentionJob& j = jobs[i_];
        SR_PLANE_NEED("sr_attention_backward", j.x && j.gamma && j.beta && j.wq && j.wk && j.wv && j.wo && j.saved && j.dy && j.dx);
        SR_PLANE_NEED("sr_attention_backward", j.dgamma && j.dbeta && j.dwq && j.dbq && j.dwk && j.dbk && j.dwv && j.dbv && j.dwo && j.dbo);
    }
    hipStream_t st = static_cast<hipStream_t>(hip_stream);
    for (int step = 0; step < sr::kAttentionBackwardSteps; ++step) {
        StageTimer t_(6, st);
        sr::launch_attention_backward(step, n_planes, jobs, channels, groups, height, width, eps, workspace, st);
    }
    return check_hip(hipGetLastError(), "attention_backward");
}

}  // extern "C"
