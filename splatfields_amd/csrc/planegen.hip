// The plane generator's convolution stack: the reference's `TimeVAEDecoder` (scene/time_decoders.py) is a
// chain of  GroupNorm -> SiLU -> [nearest x2] -> conv 3x3 -> [+ residual]  layers at 32 channels.  One layer is one launch here,
// and the three planes of the encoder share it: every kernel takes the job table (one SrPlaneJob per plane) as its argument and
// finds its plane in blockIdx.y / blockIdx.z.
//
// MI355X mapping.  The convolution is an implicit GEMM  Z[channel x pixel] = W[channel x (tap, source channel)] . S[(tap, source
// channel) x pixel]  on `v_mfma_f32_16x16x4_f32`: result channels are the rows (A operand = weights, from LDS), pixels are the
// columns (B operand = the gathered, activated input; lane & 15 = pixel, so the accumulator stores and the residual loads are 64-byte
// runs per channel).  A workgroup owns 128 consecutive output pixels, a wavefront 32 of them (two column tiles) for every result
// channel.  The K loop runs tap by tap: the weights of one tap (<= 64 x 64) are staged in LDS, a tap's chain of <= 64 products is
// accumulated on its own and then added to the running sum -- nine short chains instead of one of 576 products.
// The backward-data kernel is the same loop with the roles of the channel counts swapped, the taps mirrored and, behind an
// upsample, the four positions of a 2 x 2 block walked in a fixed order inside the K loop.
// The weight gradient is  dW[cout x cin] (per tap) = dZ[cout x pixel] . S[cin x pixel]^T  with pixels as K: a workgroup stages
// 128 pixels of both operands in LDS (rows padded to 129 words: a 16-lane column read hits 16 banks), walks a run of such pieces
// and writes its partial per tap; a second kernel adds the partials in chunk order.
// Activations are never stored: SiLU(gamma (x - mean) rstd + beta) is recomputed where it is an operand.  Out-of-range taps are
// zero AFTER the activation (the padding belongs to the activated, upsampled tensor).
// No floating-point atomics; reductions are LDS trees and fixed-order loops over partials.
#include "host_api.h"
#include "reduce.h"

namespace sr {

namespace {

typedef float f32x4 __attribute__((ext_vector_type(4)));

struct PlaneTable { SrPlaneJob job[SR_PLANE_MAX_JOBS]; };

constexpr int kGnChunk = 4096;        // values per workgroup of the statistics / GroupNorm-backward partial kernels (16 per thread)
constexpr int kConvPixels = 128;      // output pixels per workgroup of the convolution
constexpr int kWgPiece = 128;         // pixels staged at a time by the weight gradient
constexpr int kWgRow = kWgPiece + 1;  // LDS row of a staged channel
constexpr int kWgMaxChunks = 64;      // partials per plane the weight gradient aims for at most
constexpr int kMaxCh = 64;
constexpr int kWRowMax = 80;          // LDS row of the staged weights: 16 / 48 / 48 / 80 words for 16 / 32 / 48 / 64 columns

__device__ __forceinline__ float silu(float y) { return y / (1.f + expf(-y)); }
__device__ __forceinline__ float dsilu(float y) {
    const float s = 1.f / (1.f + expf(-y));
    return s * (1.f + y * (1.f - s));
}

// ---- GroupNorm statistics ---------------------------------------------------------------------------------------------------
// The sums are doubles, and the mean is handed on as a float pair (mean, mean_lo): where a group holds few, nearly equal values
// rstd is large and the rounding of a float mean (half an ulp of |x|) would come out of (x - mean) rstd amplified.
constexpr int kStat = 4;      // floats per group in `stats`: mean, rstd, mean_lo, unused

// grid (chunks, groups, planes): (mean, M2) of one chunk of a group's contiguous values
__global__ __launch_bounds__(kBlock) void k_gn_stats_partial(const PlaneTable t, int group_elems, int nchunks, double* __restrict__ ws) {
    __shared__ double red[kBlock];
    const float* __restrict__ x = t.job[blockIdx.z].x + (size_t)blockIdx.y * group_elems;
    const int lo = blockIdx.x * kGnChunk, hi = min(lo + kGnChunk, group_elems);
    float v[kGnChunk / kBlock];
    double s = 0.0;
#pragma unroll
    for (int i = 0; i < kGnChunk / kBlock; ++i) {
        const int idx = lo + i * kBlock + threadIdx.x;
        v[i] = idx < hi ? x[idx] : 0.f;
        s += (double)v[i];
    }
    const double mean = block_tree_sum<double, kBlock>(s, red) / (double)(hi - lo);
    double q = 0.0;
#pragma unroll
    for (int i = 0; i < kGnChunk / kBlock; ++i) {
        const int idx = lo + i * kBlock + threadIdx.x;
        const double d = (double)v[i] - mean;
        q += idx < hi ? d * d : 0.0;
    }
    const double m2 = block_tree_sum<double, kBlock>(q, red);
    if (threadIdx.x == 0) {
        double* o = ws + (((size_t)blockIdx.z * gridDim.y + blockIdx.y) * nchunks + blockIdx.x) * 2;
        o[0] = mean; o[1] = m2;
    }
}

// one thread per (plane, group): the chunks combined in order (Chan et al.)
__global__ __launch_bounds__(kBlock) void k_gn_stats_final(const PlaneTable t, int n_planes, int groups, int group_elems, int nchunks, float eps,
                                                           const double* __restrict__ ws) {
    const int i = blockIdx.x * kBlock + threadIdx.x;
    if (i >= n_planes * groups) return;
    const int plane = i / groups, g = i - plane * groups;
    const double* p = ws + (size_t)i * nchunks * 2;
    double n = 0.0, mean = 0.0, m2 = 0.0;
    for (int c = 0; c < nchunks; ++c) {
        const double nc = (double)(min((c + 1) * kGnChunk, group_elems) - c * kGnChunk);
        const double d = p[2 * c] - mean, nn = n + nc;
        mean += d * (nc / nn);
        m2 += p[2 * c + 1] + d * d * (n * nc / nn);
        n = nn;
    }
    float* o = t.job[plane].stats + kStat * g;
    const float mean_hi = (float)mean;
    o[0] = mean_hi;
    o[1] = (float)(1.0 / sqrt(m2 / n + (double)eps));
    o[2] = (float)(mean - (double)mean_hi);
    o[3] = 0.f;
}

// ---- convolution: forward (MODE 0) and gradient at the activated input (MODE 1) -----------------------------------------------
struct ConvArgs {
    int cin, cout, hin, win, ho, wo, up, flags, groups;
    int kc;        // source channels of the GEMM: cin forward, cout backward
    int nc;        // result channels: cout forward, cin backward
    int ntiles;    // ceil(nc / 16)
    int wrow;      // LDS row of the staged weights (words)
};

template <int MODE>
__global__ __launch_bounds__(kBlock) void k_conv(const PlaneTable t, const ConvArgs a) {
    __shared__ float Wl[kMaxCh * kWRowMax];
    __shared__ float pm[kMaxCh], pml[kMaxCh], pa[kMaxCh], pb[kMaxCh];
    const SrPlaneJob& J = t.job[blockIdx.y];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, lr = lane & 15, lk = lane >> 4;
    const int out_w = MODE == 0 ? a.wo : a.win;
    const int out_px = MODE == 0 ? a.ho * a.wo : a.hin * a.win;
    const bool prologue = MODE == 0 && (a.flags & SR_CONV_PROLOGUE);
    const bool dsilu_in = MODE == 1 && (a.flags & SR_CONV_SILU_OUT);
    if (prologue && tid < a.cin) {
        const int g = tid / (a.cin / a.groups);
        pm[tid] = J.stats[kStat * g];
        pml[tid] = J.stats[kStat * g + 2];
        pa[tid] = J.stats[kStat * g + 1] * J.gamma[tid];
        pb[tid] = J.beta[tid];
    }
    const float* __restrict__ src = MODE == 0 ? J.x : J.dy;
    const float* __restrict__ wsrc = J.weight;
    const size_t src_plane = MODE == 0 ? (size_t)a.hin * a.win : (size_t)a.ho * a.wo;
    int p[2], py[2], px[2];
    bool pv[2];
#pragma unroll
    for (int m = 0; m < 2; ++m) {
        p[m] = blockIdx.x * kConvPixels + wave * 32 + m * 16 + lr;
        pv[m] = p[m] < out_px;
        const int pc = pv[m] ? p[m] : 0;
        py[m] = pc / out_w; px[m] = pc - py[m] * out_w;
    }
    f32x4 acc[2][4];
#pragma unroll
    for (int m = 0; m < 2; ++m)
#pragma unroll
        for (int n = 0; n < 4; ++n) acc[m][n] = (f32x4){0.f, 0.f, 0.f, 0.f};
    const int ncp = a.ntiles * 16;
    const int nsub = (MODE == 1 && a.up) ? 4 : 1;
    for (int sub = 0; sub < nsub; ++sub) {
        for (int tap = 0; tap < 9; ++tap) {
            const int dy = tap / 3 - 1, dx = tap - (tap / 3) * 3 - 1;
            __syncthreads();
            for (int idx = tid; idx < a.kc * ncp; idx += kBlock) {
                int k, n;
                if (MODE == 0) { n = idx / a.kc; k = idx - n * a.kc; } else { k = idx / ncp; n = idx - k * ncp; }
                float w = 0.f;
                if (n < a.nc) w = MODE == 0 ? wsrc[((size_t)n * a.cin + k) * 9 + tap] : wsrc[((size_t)k * a.cin + n) * 9 + tap];
                Wl[k * a.wrow + n] = w;
            }
            __syncthreads();
            bool valid[2];
            size_t off[2];
#pragma unroll
            for (int m = 0; m < 2; ++m) {
                int Y, X;
                if (MODE == 0) { Y = py[m] + dy; X = px[m] + dx; }
                else { Y = (a.up ? 2 * py[m] + (sub >> 1) : py[m]) - dy; X = (a.up ? 2 * px[m] + (sub & 1) : px[m]) - dx; }
                valid[m] = pv[m] && Y >= 0 && Y < a.ho && X >= 0 && X < a.wo;
                if (!valid[m]) { Y = 0; X = 0; }
                off[m] = MODE == 0 ? (size_t)(Y >> a.up) * a.win + (X >> a.up) : (size_t)Y * a.wo + X;
            }
            f32x4 part[2][4];
#pragma unroll
            for (int m = 0; m < 2; ++m)
#pragma unroll
                for (int n = 0; n < 4; ++n) part[m][n] = (f32x4){0.f, 0.f, 0.f, 0.f};
            for (int k0 = 0; k0 < a.kc; k0 += 4) {
                const int k = k0 + lk;
                float b[2];
#pragma unroll
                for (int m = 0; m < 2; ++m) {
                    float v = 0.f;
                    if (valid[m]) {
                        v = src[k * src_plane + off[m]];
                        if (prologue) v = silu(fmaf((v - pm[k]) - pml[k], pa[k], pb[k]));
                        if (dsilu_in) v *= dsilu(J.pre[k * src_plane + off[m]]);
                    }
                    b[m] = v;
                }
#pragma unroll
                for (int n = 0; n < 4; ++n) {
                    if (n < a.ntiles) {
                        const float w = Wl[k * a.wrow + n * 16 + lr];
                        part[0][n] = __builtin_amdgcn_mfma_f32_16x16x4f32(w, b[0], part[0][n], 0, 0, 0);
                        part[1][n] = __builtin_amdgcn_mfma_f32_16x16x4f32(w, b[1], part[1][n], 0, 0, 0);
                    }
                }
            }
#pragma unroll
            for (int m = 0; m < 2; ++m)
#pragma unroll
                for (int n = 0; n < 4; ++n) acc[m][n] += part[m][n];
        }
    }
    // lane (lk, lr) of tile n holds channels 16 n + 4 lk + i of pixel lr
#pragma unroll
    for (int m = 0; m < 2; ++m) {
        if (!pv[m]) continue;
#pragma unroll
        for (int n = 0; n < 4; ++n) {
            if (n >= a.ntiles) continue;
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const int ch = n * 16 + 4 * lk + i;
                if (ch >= a.nc) continue;
                float v = acc[m][n][i];
                const size_t o = (size_t)ch * out_px + p[m];
                if (MODE == 0) {
                    if (J.bias) v += J.bias[ch];
                    if (a.flags & SR_CONV_RESIDUAL) v += J.residual[o];
                    if (a.flags & SR_CONV_SILU_OUT) { J.pre[o] = v; v = silu(v); }
                    J.out[o] = v;
                } else {
                    J.dx[o] = v;
                }
            }
        }
    }
}

// ---- weight gradient --------------------------------------------------------------------------------------------------------
// grid (chunks, planes); a chunk is `pieces` runs of 128 output pixels.  Partial layout per (plane, chunk): dW [cout, cin, 9], db [cout]
__global__ __launch_bounds__(kBlock) void k_conv_wgrad(const PlaneTable t, const ConvArgs a, int pieces, int nchunks, float* __restrict__ ws) {
    __shared__ float Dl[kMaxCh * kWgRow];
    __shared__ float Al[kMaxCh * kWgRow];
    __shared__ float pm[kMaxCh], pml[kMaxCh], pa[kMaxCh], pb[kMaxCh];
    const SrPlaneJob& J = t.job[blockIdx.y];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, lr = lane & 15, lk = lane >> 4;
    const int P = a.ho * a.wo;
    const bool prologue = a.flags & SR_CONV_PROLOGUE, silu_out = a.flags & SR_CONV_SILU_OUT;
    if (prologue && tid < a.cin) {
        const int g = tid / (a.cin / a.groups);
        pm[tid] = J.stats[kStat * g];
        pml[tid] = J.stats[kStat * g + 2];
        pa[tid] = J.stats[kStat * g + 1] * J.gamma[tid];
        pb[tid] = J.beta[tid];
    }
    const int mt_n = (a.cout + 15) / 16, nt_n = (a.cin + 15) / 16, tiles = mt_n * nt_n;
    const size_t part_len = (size_t)a.cout * a.cin * 9 + a.cout;
    float* __restrict__ part = ws + ((size_t)blockIdx.y * nchunks + blockIdx.x) * part_len;
    const int j = tid & (kWgPiece - 1), half = tid >> 7;
    const size_t in_plane = (size_t)a.hin * a.win;
    float bsum[16];
#pragma unroll
    for (int q = 0; q < 16; ++q) bsum[q] = 0.f;
    for (int tap = 0; tap < 9; ++tap) {
        const int dy = tap / 3 - 1, dx = tap - (tap / 3) * 3 - 1;
        f32x4 acc[4];
#pragma unroll
        for (int q = 0; q < 4; ++q) acc[q] = (f32x4){0.f, 0.f, 0.f, 0.f};
        for (int s = 0; s < pieces; ++s) {
            const long long pl = ((long long)blockIdx.x * pieces + s) * kWgPiece + j;
            const bool pv = pl < P;
            const int p = pv ? (int)pl : 0;
            const int oy = p / a.wo, ox = p - oy * a.wo;
            int Y = oy + dy, X = ox + dx;
            const bool av = pv && Y >= 0 && Y < a.ho && X >= 0 && X < a.wo;
            if (!av) { Y = 0; X = 0; }
            const size_t aoff = (size_t)(Y >> a.up) * a.win + (X >> a.up);
            __syncthreads();
            for (int co = half; co < mt_n * 16; co += 2) {
                float v = 0.f;
                if (pv && co < a.cout) {
                    const size_t o = (size_t)co * P + p;
                    v = J.dy[o];
                    if (silu_out) {
                        v *= dsilu(J.pre[o]);
                        if (tap == 0 && J.d_residual) J.d_residual[o] = v;
                    }
                }
                Dl[co * kWgRow + j] = v;
            }
            for (int ci = half; ci < nt_n * 16; ci += 2) {
                float v = 0.f;
                if (av && ci < a.cin) {
                    v = J.x[ci * in_plane + aoff];
                    if (prologue) v = silu(fmaf((v - pm[ci]) - pml[ci], pa[ci], pb[ci]));
                }
                Al[ci * kWgRow + j] = v;
            }
            __syncthreads();
            if (tap == 0) {
#pragma unroll
                for (int q = 0; q < 16; ++q) {
                    const int co = wave + 4 * q;
                    if (co < a.cout) {
                        float v = Dl[co * kWgRow + lane] + Dl[co * kWgRow + lane + 64];
#pragma unroll
                        for (int sh = 32; sh > 0; sh >>= 1) v += __shfl_xor(v, sh);
                        bsum[q] += v;
                    }
                }
            }
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const int tile = wave + 4 * q;
                if (tile < tiles) {
                    const int mt = tile / nt_n, nt = tile - mt * nt_n;
                    const float* dr = Dl + (mt * 16 + lr) * kWgRow + lk;
                    const float* ar = Al + (nt * 16 + lr) * kWgRow + lk;
                    f32x4 u = (f32x4){0.f, 0.f, 0.f, 0.f};
#pragma unroll 8
                    for (int k0 = 0; k0 < kWgPiece; k0 += 4) u = __builtin_amdgcn_mfma_f32_16x16x4f32(dr[k0], ar[k0], u, 0, 0, 0);
                    acc[q] += u;
                }
            }
        }
        // rows = cout (4 lk + i), columns = cin (lr)
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int tile = wave + 4 * q;
            if (tile < tiles) {
                const int mt = tile / nt_n, nt = tile - mt * nt_n, ci = nt * 16 + lr;
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    const int co = mt * 16 + 4 * lk + i;
                    if (co < a.cout && ci < a.cin) part[((size_t)co * a.cin + ci) * 9 + tap] = acc[q][i];
                }
            }
        }
    }
    if (lane == 0) {
#pragma unroll
        for (int q = 0; q < 16; ++q) {
            const int co = wave + 4 * q;
            if (co < a.cout) part[(size_t)a.cout * a.cin * 9 + co] = bsum[q];
        }
    }
}

// grid (ceil(part_len / 256), planes): the chunks' partials added in chunk order
__global__ __launch_bounds__(kBlock) void k_conv_wgrad_reduce(const PlaneTable t, int cin, int cout, int nchunks, const float* __restrict__ ws) {
    const size_t wlen = (size_t)cout * cin * 9, part_len = wlen + cout;
    const size_t idx = (size_t)blockIdx.x * kBlock + threadIdx.x;
    if (idx >= part_len) return;
    const float* p = ws + (size_t)blockIdx.y * nchunks * part_len + idx;
    float s = 0.f;
    for (int c = 0; c < nchunks; ++c) s += p[(size_t)c * part_len];
    const SrPlaneJob& J = t.job[blockIdx.y];
    if (idx < wlen) J.dweight[idx] = s;
    else if (J.dbias) J.dbias[idx - wlen] = s;
}

// ---- backward through SiLU and GroupNorm ------------------------------------------------------------------------------------
struct GnArgs { int channels, groups, hw, nchunks, small; float eps; };

// A group of few values (<= kGnSmall) goes through double arithmetic from the raw x on: with n values in a group the backward
// subtracts the projection of dy onto (1, xhat), and what is left is of relative size eps rstd^2 when n is tiny (n = 2: xhat =
// +-a, 1 - a^2 = eps rstd^2) -- float statistics cannot resolve that.  Large groups keep the float path and the stored statistics.
constexpr int kGnSmall = 1024;

// mean and 1 / sqrt(var + eps) of the n <= kGnSmall contiguous values of a group, by the whole workgroup
__device__ __forceinline__ void group_stats_d(const float* __restrict__ xg, int n, double eps, double* red, double* mean, double* rstd) {
    double s = 0.0;
    for (int i = threadIdx.x; i < n; i += kBlock) s += (double)xg[i];
    const double m = block_tree_sum<double, kBlock>(s, red) / (double)n;
    double q = 0.0;
    for (int i = threadIdx.x; i < n; i += kBlock) { const double d = (double)xg[i] - m; q += d * d; }
    const double var = block_tree_sum<double, kBlock>(q, red) / (double)n;
    *mean = m;
    *rstd = 1.0 / sqrt(var + eps);
}

__device__ __forceinline__ double gn_dy_d(double x, double g, double mean, double rstd, double gam, double bet, double* xh) {
    *xh = (x - mean) * rstd;
    const double y = *xh * gam + bet, sg = 1.0 / (1.0 + exp(-y));
    return g * sg * (1.0 + y * (1.0 - sg));
}

__device__ __forceinline__ float gn_dy(float x, float g, float mean, float mean_lo, float rstd, float gam, float bet, float* xh) {
    const float xc = (x - mean) - mean_lo;
    *xh = xc * rstd;
    return g * dsilu(fmaf(xc, rstd * gam, bet));
}

// grid (chunks, channels, planes): sum dy and sum dy xhat of one chunk of a channel.  Partials are pairs of doubles.
__global__ __launch_bounds__(kBlock) void k_gn_bwd_partial(const PlaneTable t, const GnArgs a, double* __restrict__ ws) {
    __shared__ double red[kBlock];
    const SrPlaneJob& J = t.job[blockIdx.z];
    const int cg = a.channels / a.groups, c = blockIdx.y, g = c / cg;
    const float* __restrict__ x = J.x + (size_t)c * a.hw;
    const float* __restrict__ ga = J.dx + (size_t)c * a.hw;
    const int lo = blockIdx.x * kGnChunk, hi = min(lo + kGnChunk, a.hw);
    double s1 = 0.0, s2 = 0.0;
    if (a.small) {
        double mean, rstd;
        group_stats_d(J.x + (size_t)g * cg * a.hw, cg * a.hw, (double)a.eps, red, &mean, &rstd);
        const double gam = J.gamma[c], bet = J.beta[c];
        for (int idx = lo + threadIdx.x; idx < hi; idx += kBlock) {
            double xh;
            const double d = gn_dy_d(x[idx], ga[idx], mean, rstd, gam, bet, &xh);
            s1 += d; s2 += d * xh;
        }
    } else {
        const float mean = J.stats[kStat * g], rstd = J.stats[kStat * g + 1], mean_lo = J.stats[kStat * g + 2], gam = J.gamma[c], bet = J.beta[c];
        float f1 = 0.f, f2 = 0.f;
#pragma unroll
        for (int i = 0; i < kGnChunk / kBlock; ++i) {
            const int idx = lo + i * kBlock + threadIdx.x;
            if (idx < hi) {
                float xh;
                const float d = gn_dy(x[idx], ga[idx], mean, mean_lo, rstd, gam, bet, &xh);
                f1 += d; f2 += d * xh;
            }
        }
        s1 = f1; s2 = f2;
    }
    s1 = block_tree_sum<double, kBlock>(s1, red);
    s2 = block_tree_sum<double, kBlock>(s2, red);
    if (threadIdx.x == 0) {
        double* o = ws + (((size_t)blockIdx.z * a.channels + c) * a.nchunks + blockIdx.x) * 2;
        o[0] = s1; o[1] = s2;
    }
}

// grid (ceil(hw / 1024), channels, planes)
__global__ __launch_bounds__(kBlock) void k_gn_bwd_apply(const PlaneTable t, const GnArgs a, const double* __restrict__ ws) {
    __shared__ double red[kBlock];
    __shared__ double cs1[kMaxCh], cs2[kMaxCh], tot[2];
    const SrPlaneJob& J = t.job[blockIdx.z];
    const int cg = a.channels / a.groups, c = blockIdx.y, g = c / cg, tid = threadIdx.x;
    if (tid < cg) {
        const double* p = ws + ((size_t)blockIdx.z * a.channels + g * cg + tid) * a.nchunks * 2;
        double u = 0.0, v = 0.0;
        for (int k = 0; k < a.nchunks; ++k) { u += p[2 * k]; v += p[2 * k + 1]; }
        cs1[tid] = u; cs2[tid] = v;
    }
    __syncthreads();
    if (tid == 0) {
        double u = 0.0, v = 0.0;
        for (int k = 0; k < cg; ++k) { const double gm = J.gamma[g * cg + k]; u += gm * cs1[k]; v += gm * cs2[k]; }
        tot[0] = u; tot[1] = v;
        if (blockIdx.x == 0) { J.dbeta[c] = (float)cs1[c - g * cg]; J.dgamma[c] = (float)cs2[c - g * cg]; }
    }
    __syncthreads();
    const size_t base = (size_t)c * a.hw;
    if (a.small) {
        double mean, rstd;
        group_stats_d(J.x + (size_t)g * cg * a.hw, cg * a.hw, (double)a.eps, red, &mean, &rstd);
        const double S1 = tot[0], S2 = tot[1], inv_n = 1.0 / ((double)cg * (double)a.hw), gam = J.gamma[c], bet = J.beta[c];
        for (int i = 0; i < 4; ++i) {
            const int idx = blockIdx.x * (4 * kBlock) + i * kBlock + tid;
            if (idx < a.hw) {
                double xh;
                const double d = gn_dy_d(J.x[base + idx], J.dx[base + idx], mean, rstd, gam, bet, &xh);
                double r = rstd * (d * gam - (S1 + xh * S2) * inv_n);
                if (J.add) r += (double)J.add[base + idx];
                J.dx_out[base + idx] = (float)r;
            }
        }
        return;
    }
    const float S1 = (float)tot[0], S2 = (float)tot[1], inv_n = 1.f / ((float)cg * (float)a.hw);
    const float mean = J.stats[kStat * g], rstd = J.stats[kStat * g + 1], mean_lo = J.stats[kStat * g + 2], gam = J.gamma[c], bet = J.beta[c];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int idx = blockIdx.x * (4 * kBlock) + i * kBlock + tid;
        if (idx < a.hw) {
            float xh;
            const float d = gn_dy(J.x[base + idx], J.dx[base + idx], mean, mean_lo, rstd, gam, bet, &xh);
            float r = rstd * (d * gam - (S1 + xh * S2) * inv_n);
            if (J.add) r += J.add[base + idx];
            J.dx_out[base + idx] = r;
        }
    }
}

PlaneTable make_table(int n, const SrPlaneJob* jobs) {
    PlaneTable t = {};
    for (int i = 0; i < n; ++i) t.job[i] = jobs[i];
    return t;
}

ConvArgs make_conv_args(int cin, int cout, int hin, int win, int groups, int flags, bool backward) {
    ConvArgs a = {};
    a.cin = cin; a.cout = cout; a.hin = hin; a.win = win; a.up = (flags & SR_CONV_UPSAMPLE) ? 1 : 0;
    a.ho = hin << a.up; a.wo = win << a.up; a.flags = flags; a.groups = groups > 0 ? groups : 1;
    a.kc = backward ? cout : cin; a.nc = backward ? cin : cout;
    a.ntiles = (a.nc + 15) / 16;
    a.wrow = a.ntiles == 1 ? 16 : a.ntiles <= 3 ? 48 : 80;
    return a;
}

int gn_chunks(long long elems) { return (int)((elems + kGnChunk - 1) / kGnChunk); }

bool plane_channels_ok(int c) { return c >= 8 && c <= kMaxCh && c % 8 == 0; }
bool plane_conv_shape_ok(int cin, int cout, int hin, int win, int flags) {
    if (!plane_channels_ok(cin) || !plane_channels_ok(cout) || hin <= 0 || win <= 0 || hin > 4096 || win > 4096) return false;
    const long long up = (flags & SR_CONV_UPSAMPLE) ? 2 : 1;
    return (long long)hin * up * win * up < (1ll << 24) && (flags & ~15) == 0;
}
bool plane_gn_shape_ok(int channels, int groups, int h, int w) {
    return channels >= 1 && channels <= kMaxCh && groups >= 1 && channels % groups == 0 && h > 0 && w > 0 && h <= 8192 && w <= 8192 &&
           (long long)h * w < (1ll << 24);
}

size_t gn_stats_workspace(int n_planes, int channels, int groups, int h, int w) {
    return (size_t)n_planes * groups * gn_chunks((long long)(channels / groups) * h * w) * 2 * sizeof(double);
}
void launch_gn_stats_partial(int n, const SrPlaneJob* jobs, int channels, int groups, int h, int w, void* ws, hipStream_t st) {
    const int ge = (channels / groups) * h * w, nch = gn_chunks(ge);
    hipLaunchKernelGGL(k_gn_stats_partial, dim3(nch, groups, n), dim3(kBlock), 0, st, make_table(n, jobs), ge, nch, static_cast<double*>(ws));
}
void launch_gn_stats_final(int n, const SrPlaneJob* jobs, int channels, int groups, int h, int w, float eps, const void* ws, hipStream_t st) {
    const int ge = (channels / groups) * h * w, nch = gn_chunks(ge);
    hipLaunchKernelGGL(k_gn_stats_final, dim3((n * groups + kBlock - 1) / kBlock), dim3(kBlock), 0, st, make_table(n, jobs), n, groups, ge, nch, eps,
                       static_cast<const double*>(ws));
}

void launch_conv3x3_forward(int n, const SrPlaneJob* jobs, int cin, int cout, int hin, int win, int groups, int flags, hipStream_t st) {
    const ConvArgs a = make_conv_args(cin, cout, hin, win, groups, flags, false);
    const int px = a.ho * a.wo;
    hipLaunchKernelGGL(k_conv<0>, dim3((px + kConvPixels - 1) / kConvPixels, n), dim3(kBlock), 0, st, make_table(n, jobs), a);
}
void launch_conv3x3_backward_data(int n, const SrPlaneJob* jobs, int cin, int cout, int hin, int win, int flags, hipStream_t st) {
    const ConvArgs a = make_conv_args(cin, cout, hin, win, 1, flags, true);
    const int px = hin * win;
    hipLaunchKernelGGL(k_conv<1>, dim3((px + kConvPixels - 1) / kConvPixels, n), dim3(kBlock), 0, st, make_table(n, jobs), a);
}

static void wgrad_split(int hin, int win, int flags, int* pieces, int* nchunks) {
    const int up = (flags & SR_CONV_UPSAMPLE) ? 1 : 0;
    const long long px = (long long)(hin << up) * (win << up);
    const long long npieces = (px + kWgPiece - 1) / kWgPiece;
    *pieces = (int)((npieces + kWgMaxChunks - 1) / kWgMaxChunks);
    *nchunks = (int)((npieces + *pieces - 1) / *pieces);
}
size_t conv3x3_weight_grad_workspace(int n_planes, int cin, int cout, int hin, int win, int flags) {
    // room for min(pieces of the image, kWgMaxChunks) partials: never less than the split uses, and monotone in the image size
    const int up = (flags & SR_CONV_UPSAMPLE) ? 1 : 0;
    const long long npieces = ((long long)(hin << up) * (win << up) + kWgPiece - 1) / kWgPiece;
    const long long nchunks = npieces < kWgMaxChunks ? npieces : kWgMaxChunks;
    return (size_t)n_planes * nchunks * ((size_t)cout * cin * 9 + cout) * sizeof(float);
}
void launch_conv3x3_wgrad_partial(int n, const SrPlaneJob* jobs, int cin, int cout, int hin, int win, int groups, int flags, void* ws, hipStream_t st) {
    int pieces, nchunks;
    wgrad_split(hin, win, flags, &pieces, &nchunks);
    const ConvArgs a = make_conv_args(cin, cout, hin, win, groups, flags, false);
    hipLaunchKernelGGL(k_conv_wgrad, dim3(nchunks, n), dim3(kBlock), 0, st, make_table(n, jobs), a, pieces, nchunks, static_cast<float*>(ws));
}
void launch_conv3x3_wgrad_reduce(int n, const SrPlaneJob* jobs, int cin, int cout, int hin, int win, int flags, const void* ws, hipStream_t st) {
    int pieces, nchunks;
    wgrad_split(hin, win, flags, &pieces, &nchunks);
    const int len = cout * cin * 9 + cout;
    hipLaunchKernelGGL(k_conv_wgrad_reduce, dim3((len + kBlock - 1) / kBlock, n), dim3(kBlock), 0, st, make_table(n, jobs), cin, cout, nchunks,
                       static_cast<const float*>(ws));
}

size_t gn_silu_backward_workspace(int n_planes, int channels, int h, int w) {
    return (size_t)n_planes * channels * gn_chunks((long long)h * w) * 2 * sizeof(double);
}
static GnArgs make_gn_args(int channels, int groups, int h, int w, float eps) {
    GnArgs a = {};
    a.channels = channels; a.groups = groups; a.hw = h * w; a.nchunks = gn_chunks((long long)h * w);
    a.small = (long long)(channels / groups) * h * w <= kGnSmall ? 1 : 0;
    a.eps = eps;
    return a;
}
void launch_gn_silu_backward_partial(int n, const SrPlaneJob* jobs, int channels, int groups, int h, int w, float eps, void* ws, hipStream_t st) {
    const GnArgs a = make_gn_args(channels, groups, h, w, eps);
    hipLaunchKernelGGL(k_gn_bwd_partial, dim3(a.nchunks, channels, n), dim3(kBlock), 0, st, make_table(n, jobs), a, static_cast<double*>(ws));
}
void launch_gn_silu_backward_apply(int n, const SrPlaneJob* jobs, int channels, int groups, int h, int w, float eps, const void* ws, hipStream_t st) {
    const GnArgs a = make_gn_args(channels, groups, h, w, eps);
    hipLaunchKernelGGL(k_gn_bwd_apply, dim3((a.hw + 4 * kBlock - 1) / (4 * kBlock), channels, n), dim3(kBlock), 0, st, make_table(n, jobs), a,
                       static_cast<const double*>(ws));
}

}  // namespace

}  // namespace sr

// ---- C entry points (include/splatraster.h): what is refused on the host, then the launchers above --------------------
using sr::fail; using sr::check_hip; using sr::StageTimer;

extern "C" {

static int plane_jobs_ok(const char* who, int n_planes, const SrPlaneJob* jobs) {
    if (!jobs) return fail(std::string("null pointer in ") + who + ": jobs");
    if (n_planes < 1 || n_planes > SR_PLANE_MAX_JOBS) return fail(std::string("bad arguments to ") + who + ": n_planes must be 1 .. SR_PLANE_MAX_JOBS (8)");
    return 0;
}

size_t sr_groupnorm_stats_workspace(int n_planes, int channels, int groups, int height, int width) {
    if (n_planes < 1 || n_planes > SR_PLANE_MAX_JOBS || !sr::plane_gn_shape_ok(channels, groups, height, width)) return 0;
    return sr::gn_stats_workspace(n_planes, channels, groups, height, width);
}

int sr_groupnorm_stats(int n_planes, const SrPlaneJob* jobs, int channels, int groups, int height, int width, float eps, void* workspace,
                       void* hip_stream) {
    SR_TRY(plane_jobs_ok("sr_groupnorm_stats", n_planes, jobs));
    if (!sr::plane_gn_shape_ok(channels, groups, height, width))
        return fail("sr_groupnorm_stats: channels in 1..64, groups must divide channels, height * width < 2^24");
    if (!workspace) return fail("null pointer in sr_groupnorm_stats: workspace");
    for (int i_ = 0; i_ < n_planes; ++i_) { const SrPlaneJob& j = jobs[i_]; SR_PLANE_NEED("sr_groupnorm_stats", j.x && j.stats); }
    hipStream_t st = static_cast<hipStream_t>(hip_stream);
    { StageTimer t_(0, st); sr::launch_gn_stats_partial(n_planes, jobs, channels, groups, height, width, workspace, st); }
    { StageTimer t_(0, st); sr::launch_gn_stats_final(n_planes, jobs, channels, groups, height, width, eps, workspace, st); }
    return check_hip(hipGetLastError(), "groupnorm_stats");
}

static int conv_shape_check(const char* who, int cin, int cout, int h_in, int w_in, int groups, int flags) {
    if (!sr::plane_conv_shape_ok(cin, cout, h_in, w_in, flags))
        return fail(std::string(who) + ": cin and cout must be multiples of 8 in 8..64, the output below 2^24 pixels, flags SR_CONV_* bits");
    if ((flags & SR_CONV_PROLOGUE) && (groups < 1 || cin % groups != 0)) return fail(std::string(who) + ": groups must divide cin");
    return 0;
}

int sr_conv3x3_forward(int n_planes, const SrPlaneJob* jobs, int cin, int cout, int h_in, int w_in, int groups, int flags, void* hip_stream) {
    SR_TRY(plane_jobs_ok("sr_conv3x3_forward", n_planes, jobs));
    SR_TRY(conv_shape_check("sr_conv3x3_forward", cin, cout, h_in, w_in, groups, flags));
    for (int i_ = 0; i_ < n_planes; ++i_) {
        const SrPlaneJob& j = jobs[i_];
        SR_PLANE_NEED("sr_conv3x3_forward", j.x && j.weight && j.out);
        if (flags & SR_CONV_PROLOGUE) SR_PLANE_NEED("sr_conv3x3_forward", j.gamma && j.beta && j.stats);
        if (flags & SR_CONV_RESIDUAL) SR_PLANE_NEED("sr_conv3x3_forward", j.residual);
        if (flags & SR_CONV_SILU_OUT) SR_PLANE_NEED("sr_conv3x3_forward", j.pre);
    }
    hipStream_t st = static_cast<hipStream_t>(hip_stream);
    { StageTimer t_(0, st); sr::launch_conv3x3_forward(n_planes, jobs, cin, cout, h_in, w_in, groups, flags, st); }
    return check_hip(hipGetLastError(), "conv3x3_forward");
}

int sr_conv3x3_backward_data(int n_planes, const SrPlaneJob* jobs, int cin, int cout, int h_in, int w_in, int flags, void* hip_stream) {
    SR_TRY(plane_jobs_ok("sr_conv3x3_backward_data", n_planes, jobs));
    SR_TRY(conv_shape_check("sr_conv3x3_backward_data", cin, cout, h_in, w_in, 1, flags & ~SR_CONV_PROLOGUE));
    for (int i_ = 0; i_ < n_planes; ++i_) {
        const SrPlaneJob& j = jobs[i_];
        SR_PLANE_NEED("sr_conv3x3_backward_data", j.dy && j.weight && j.dx);
        if (flags & SR_CONV_SILU_OUT) SR_PLANE_NEED("sr_conv3x3_backward_data", j.pre);
    }
    hipStream_t st = static_cast<hipStream_t>(hip_stream);
    { StageTimer t_(6, st); sr::launch_conv3x3_backward_data(n_planes, jobs, cin, cout, h_in, w_in, flags, st); }
    return check_hip(hipGetLastError(), "conv3x3_backward_data");
}

size_t sr_groupnorm_silu_backward_workspace(int n_planes, int channels, int height, int width) {
    if (n_planes < 1 || n_planes > SR_PLANE_MAX_JOBS || !sr::plane_gn_shape_ok(channels, 1, height, width)) return 0;
    return sr::gn_silu_backward_workspace(n_planes, channels, height, width);
}

int sr_groupnorm_silu_backward(int n_planes, const SrPlaneJob* jobs, int channels, int groups, int height, int width, float eps,
                               void* workspace, void* hip_stream) {
    SR_TRY(plane_jobs_ok("sr_groupnorm_silu_backward", n_planes, jobs));
    if (!sr::plane_gn_shape_ok(channels, groups, height, width))
        return fail("sr_groupnorm_silu_backward: channels in 1..64, groups must divide channels, height * width < 2^24");
    if (!workspace) return fail("null pointer in sr_groupnorm_silu_backward: workspace");
    for (int i_ = 0; i_ < n_planes; ++i_) {
        const SrPlaneJob& j = jobs[i_];
        SR_PLANE_NEED("sr_groupnorm_silu_backward", j.dx && j.x && j.gamma && j.beta && j.stats && j.dx_out && j.dgamma && j.dbeta);
    }
    hipStream_t st = static_cast<hipStream_t>(hip_stream);
    { StageTimer t_(6, st); sr::launch_gn_silu_backward_partial(n_planes, jobs, channels, groups, height, width, eps, workspace, st); }
    { StageTimer t_(6, st); sr::launch_gn_silu_backward_apply(n_planes, jobs, channels, groups, height, width, eps, workspace, st); }
    return check_hip(hipGetLastError(), "groupnorm_silu_backward");
}

size_t sr_conv3x3_weight_grad_workspace(int n_planes, int cin, int cout, int h_in, int w_in, int flags) {
    if (n_planes < 1 || n_planes > SR_PLANE_MAX_JOBS || !sr::plane_conv_shape_ok(cin, cout, h_in, w_in, flags)) return 0;
    return sr::conv3x3_weight_grad_workspace(n_planes, cin, cout, h_in, w_in, flags);
}

int sr_conv3x3_weight_grad(int n_planes, const SrPlaneJob* jobs, int cin, int cout, int h_in, int w_in, int groups, int flags, void* workspace,
                           void* hip_stream) {
    SR_TRY(plane_jobs_ok("sr_conv3x3_weight_grad", n_planes, jobs));
    SR_TRY(conv_shape_check("sr_conv3x3_weight_grad", cin, cout, h_in, w_in, groups, flags));
    if (!workspace) return fail("null pointer in sr_conv3x3_weight_grad: workspace");
    for (int i_ = 0; i_ < n_planes; ++i_) {
        const SrPlaneJob& j = jobs[i_];
        SR_PLANE_NEED("sr_conv3x3_weight_grad", j.dy && j.x && j.dweight);
        if (flags & SR_CONV_PROLOGUE) SR_PLANE_NEED("sr_conv3x3_weight_grad", j.gamma && j.beta && j.stats);
        if (flags & SR_CONV_SILU_OUT) SR_PLANE_NEED("sr_conv3x3_weight_grad", j.pre);
    }
    hipStream_t st = static_cast<hipStream_t>(hip_stream);
    { StageTimer t_(6, st); sr::launch_conv3x3_wgrad_partial(n_planes, jobs, cin, cout, h_in, w_in, groups, flags, workspace, st); }
    { StageTimer t_(6, st); sr::launch_conv3x3_wgrad_reduce(n_planes, jobs, cin, cout, h_in, w_in, flags, workspace, st); }
    return check_hip(hipGetLastError(), "conv3x3_weight_grad");
}

}  // extern "C"
