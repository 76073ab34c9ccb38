// LPIPS (VGG) of a batch of image pairs (DESIGN.md "LPIPS"): forward only, float32 throughout.
//
// Restates the published `lpips` package, v0.1, net='vgg', spatial=False, eval mode, with weights the caller supplies:
//
//   input    both images quantised (SR_QUANT_*), mapped [0,1] -> [-1,1] as 2 x - 1, then (x - shift_c) / scale_c;
//   trunk    13 convolutions 3x3, padding 1 (zeros in the scaled domain), bias, ReLU; widths 64,64 | 128,128 | 256,256,256 |
//            512,512,512 | 512,512,512; a 2x2 / stride-2 max-pool (floor) between the groups;
//   taps     the ReLU output of the last convolution of each group;
//   per tap  both features divided by (sqrt(sum_c x^2) + 1e-10), the squared difference weighted with lin_l[c], summed over
//            the channels, averaged over the tap's pixels;
//   value    the sum of the five taps.
//
// Activations are channels-last: [image][row][pixel][channel], image = 2 item + (0: pred, 1: gt), so that pred and gt of every
// item of the call go through the same launches and the K dimension of the implicit GEMM is contiguous.
//
// k_lpips_conv0   the first layer (cin 3, K = 27) on the VALU: a workgroup per 16x16 pixels, the 18x18x3 region goes to LDS
//                 quantised, mapped and scaled, addressed by the caller's strides; a thread per pixel, 64 results.
// k_lpips_conv    cin in {64, 128, 256, 512}: an implicit GEMM on v_mfma_f32_32x32x2_f32.  A workgroup computes 8x16 pixels x 64
//                 result channels; per 16 input channels the 10x18 region and the 9 x 64 x 16 weights go to LDS (the next
//                 piece is fetched into registers while the current one is multiplied); a wavefront owns 4x16 pixels x 32
//                 channels = two accumulators of 32x32.  A lane's four consecutive channels are one 16-byte LDS read and feed
//                 four MFMAs: MFMA c of an 8-channel group takes channels {c, 4 + c} -- the same assignment on both operands,
//                 and a sum does not care which K index a term carries.  Each piece is summed from zero and added to the
//                 running total (a blocked sum: a third of the rounding error of one chain over 9 cin terms).  Epilogue: bias, ReLU, the full-resolution store,
//                 and for the last layer of a group the 2x2 maximum, which lies inside one lane's accumulator.
// k_lpips_head    a tap: a wavefront per pixel holds both features in registers, two shuffle-tree sums for the norms, one for
//                 the weighted squared difference; 64 pixels per workgroup, one partial sum (double) per workgroup.
// k_lpips_reduce  one workgroup; a wavefront per item adds the item's partial sums of each tap in a fixed order.
//
// 13 + 5 + 1 = 19 launches per call (kLpLaunches).  No atomics, no host wait: results are bit-identical from call to call, and
// an item's partial sums are its own, so its value does not depend on the rest of the batch.
#include "host_api.h"
#include "quantise.h"
#include "reduce.h"

namespace sr {

namespace {

constexpr int kLpLayers = SR_LPIPS_CONVS, kLpTaps = SR_LPIPS_TAPS;
constexpr int kLpLaunches = 19;
constexpr int kLpCin[kLpLayers] = {3, 64, 64, 128, 128, 256, 256, 256, 512, 512, 512, 512, 512};
constexpr int kLpCout[kLpLayers] = {64, 64, 128, 128, 256, 256, 256, 512, 512, 512, 512, 512, 512};
constexpr int kLpGroup[kLpLayers] = {0, 0, 1, 1, 2, 2, 2, 3, 3, 3, 4, 4, 4};
constexpr int kLpTapC[kLpTaps] = {64, 128, 256, 512, 512};
constexpr int kLpMaxSide = 32768;

// ---- the packed weights: one blob of floats ----
//   layer 0        [27][64]: k = 9 ci + 3 ky + kx, then the result channel
//   layers 1..12   [cout / 64][cin / 16][9 taps][64 result channels][16 input channels]: what one workgroup of k_lpips_conv
//                  stages per piece is one contiguous run of 9216 floats
//   then the 13 biases, the 5 lin vectors, shift[3], scale[3]; every part starts on a 256-byte boundary
struct LpLayout { size_t w[kLpLayers], b[kLpLayers], lin[kLpTaps], shift, scale, total; };
LpLayout lp_layout() {
    LpLayout L;
    size_t off = 0;
    auto take = [&](size_t n) { const size_t at = off; off = align_up(off + n, 64); return at; };
    for (int l = 0; l < kLpLayers; ++l) L.w[l] = take((size_t)9 * kLpCin[l] * kLpCout[l]);
    for (int l = 0; l < kLpLayers; ++l) L.b[l] = take((size_t)kLpCout[l]);
    for (int t = 0; t < kLpTaps; ++t) L.lin[t] = take((size_t)kLpTapC[t]);
    L.shift = take(3); L.scale = take(3);
    L.total = off;
    return L;
}

constexpr int kCvTileH = 8, kCvTileW = 16, kCvN = 64, kCvK = 16;
constexpr int kCvHaloH = kCvTileH + 2, kCvHaloW = kCvTileW + 2, kCvHalo = kCvHaloH * kCvHaloW;   // 10 x 18 = 180 pixels
constexpr int kCvStride = kCvK + 4;          // floats per LDS row: 5 x 16 bytes, an odd count, so 16-byte reads of 8 rows spread
constexpr int kCvWRows = 9 * kCvN;           // 576 (tap, result channel) rows of 16 input channels
constexpr int kCvPiece = kCvWRows * kCvK;    // 9216 floats of weights per piece
constexpr int kCvInLoads = (kCvHalo * (kCvK / 4) + kBlock - 1) / kBlock;   // 720 float4 -> 3 per thread
constexpr int kCvWLoads = kCvPiece / 4 / kBlock;                           // 2304 float4 -> 9 per thread
static_assert(kCvPiece % (4 * kBlock) == 0, "whole float4 per thread");

typedef float f32x16 __attribute__((ext_vector_type(16)));

// dst index -> source element of a torch [cout, cin, 3, 3] weight
__global__ void __launch_bounds__(kBlock) k_lpips_pack_conv(int cin, int cout, const float* __restrict__ src, float* __restrict__ dst) {
    const size_t n = (size_t)9 * cin * cout;
    const size_t i = (size_t)blockIdx.x * kBlock + threadIdx.x;
    if (i >= n) return;
    if (cin == 3) {
        const int co = (int)(i % 64), k = (int)(i / 64);
        dst[i] = src[(size_t)co * 27 + k];
        return;
    }
    const int k = (int)(i % kCvK), nn = (int)((i / kCvK) % kCvN), tap = (int)((i / (kCvK * kCvN)) % 9);
    const size_t piece = i / kCvPiece;
    const int pieces = cin / kCvK;
    const int chunk = (int)(piece % pieces), blk = (int)(piece / pieces);
    dst[i] = src[((size_t)(blk * kCvN + nn) * cin + (chunk * kCvK + k)) * 9 + tap];
}

__global__ void __launch_bounds__(kBlock) k_lpips_copy(int n, const float* __restrict__ src, float* __restrict__ dst) {
    const int i = blockIdx.x * kBlock + threadIdx.x;
    if (i < n) dst[i] = src[i];
}

struct Conv0Dims {
    int H, W, tiles_x, tiles_y;
    long long ps[4], gs[4];      // element strides of pred and gt: item, channel, row, pixel
};

// out: [n_img][H][W][64]
template <int kQuant>
__global__ void __launch_bounds__(kBlock) k_lpips_conv0(const Conv0Dims d, const float* __restrict__ pred, const float* __restrict__ gt,
                                                        const float* __restrict__ w, const float* __restrict__ bias,
                                                        const float* __restrict__ shift, const float* __restrict__ scale,
                                                        float* __restrict__ out) {
    __shared__ float s_x[3][18 * 18];
    __shared__ __attribute__((aligned(16))) float s_w[27 * 64];
    __shared__ __attribute__((aligned(16))) float s_b[64];
    const unsigned per_img = (unsigned)d.tiles_x * (unsigned)d.tiles_y;
    const unsigned img = blockIdx.x / per_img, t_in = blockIdx.x - img * per_img;
    const int ty = (int)(t_in / (unsigned)d.tiles_x), tx = (int)(t_in - (unsigned)ty * (unsigned)d.tiles_x);
    const int y0 = ty * 16, x0 = tx * 16;
    const int item = (int)(img >> 1);
    const bool is_gt = (img & 1u) != 0u;
    const long long* st = is_gt ? d.gs : d.ps;
    const float* base = (is_gt ? gt : pred) + (long long)item * st[0];
    for (int i = threadIdx.x; i < 27 * 64; i += kBlock) s_w[i] = w[i];
    if (threadIdx.x < 64) s_b[threadIdx.x] = bias[threadIdx.x];
    for (int i = threadIdx.x; i < 3 * 18 * 18; i += kBlock) {
        const int c = i / (18 * 18), p = i - c * (18 * 18);
        const int hy = p / 18, hx = p - hy * 18;
        const int y = y0 - 1 + hy, x = x0 - 1 + hx;
        float v = 0.0f;          // the padding is zero in the scaled domain
        if (y >= 0 && y < d.H && x >= 0 && x < d.W) {
            float level;
            const float q = quantise<kQuant>(base[(long long)c * st[1] + (long long)y * st[2] + (long long)x * st[3]], level);
            v = __fdiv_rn(__fsub_rn(__fsub_rn(__fmul_rn(2.0f, q), 1.0f), shift[c]), scale[c]);
        }
        s_x[c][p] = v;
    }
    __syncthreads();
    const int py = threadIdx.x >> 4, px = threadIdx.x & 15;
    const int y = y0 + py, x = x0 + px;
    if (y >= d.H || x >= d.W) return;
    float xin[27];
#pragma unroll
    for (int c = 0; c < 3; ++c)
#pragma unroll
        for (int t = 0; t < 9; ++t) xin[9 * c + t] = s_x[c][(py + t / 3) * 18 + px + t % 3];
    float4* o = reinterpret_cast<float4*>(out + (((size_t)img * d.H + y) * d.W + x) * 64);
#pragma unroll 1
    for (int cb = 0; cb < 16; ++cb) {
        float4 acc = *reinterpret_cast<const float4*>(&s_b[4 * cb]);
#pragma unroll
        for (int k = 0; k < 27; ++k) {
            const float4 wk = *reinterpret_cast<const float4*>(&s_w[k * 64 + 4 * cb]);
            acc.x = fmaf(xin[k], wk.x, acc.x); acc.y = fmaf(xin[k], wk.y, acc.y);
            acc.z = fmaf(xin[k], wk.z, acc.z); acc.w = fmaf(xin[k], wk.w, acc.w);
        }
        o[cb] = make_float4(fmaxf(acc.x, 0.0f), fmaxf(acc.y, 0.0f), fmaxf(acc.z, 0.0f), fmaxf(acc.w, 0.0f));
    }
}

struct ConvDims {
    int H, W, cin, cout, tiles_x, tiles_y;
    int Hp, Wp;                  // H / 2, W / 2: the pooled output (written when `pooled` is given)
};

// The staging registers of k_lpips_conv are named one by one: as arrays they stay in scratch memory across the multiply loop.
#define SR_LP_IN3(F) F(0) F(1) F(2)
#define SR_LP_W9(F) F(0) F(1) F(2) F(3) F(4) F(5) F(6) F(7) F(8)
static_assert(kCvInLoads == 3 && kCvWLoads == 9, "SR_LP_IN3 / SR_LP_W9");

// in: [n_img][H][W][cin], out: [n_img][H][W][cout], pooled (may be NULL): [n_img][Hp][Wp][cout]
// (two workgroups of 60 KB of LDS fit a compute unit: two wavefronts per SIMD, and the registers that go with them)
__global__ void __launch_bounds__(kBlock) __attribute__((amdgpu_waves_per_eu(2, 2)))
k_lpips_conv(const ConvDims d, const float* __restrict__ in, const float* __restrict__ wpk, const float* __restrict__ bias,
             float* __restrict__ out, float* __restrict__ pooled) {
    __shared__ __attribute__((aligned(16))) float s_in[kCvHalo * kCvStride];
    __shared__ __attribute__((aligned(16))) float s_w[kCvWRows * kCvStride];

    const unsigned per_img = (unsigned)d.tiles_x * (unsigned)d.tiles_y;
    const unsigned img = blockIdx.x / per_img, t_in = blockIdx.x - img * per_img;
    const int ty = (int)(t_in / (unsigned)d.tiles_x), tx = (int)(t_in - (unsigned)ty * (unsigned)d.tiles_x);
    const int y0 = ty * kCvTileH, x0 = tx * kCvTileW;
    const int H = d.H, W = d.W, cin = d.cin, cout = d.cout;
    const int pieces = cin / kCvK;
    const int n0 = blockIdx.y * kCvN;
    const float* in_img = in + (size_t)img * H * W * cin;
    const float* w_blk = wpk + (size_t)blockIdx.y * pieces * kCvPiece;

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int half = lane >> 5, l32 = lane & 31;
    const int mrow0 = (wave & 1) * 4;            // the wavefront's first row of the tile: 4 rows x 16 pixels
    const int nb = (wave >> 1) * 32;             // and its first result channel of the 64

    // where this thread's parts of the region come from (the piece adds its channel offset) and go to; then per piece:
    // global memory -> registers (SR_LP_FETCH), registers -> LDS (SR_LP_STAGE)
#define SR_LP_DECL_IN(i)                                                                                  \
    const float* in_src##i; int in_dst##i; float4 rin##i;                                                 \
    {                                                                                                     \
        const int idx = tid + kBlock * i, pix = idx >> 2, q = idx & 3;                                    \
        const int hy = pix / kCvHaloW, hx = pix - hy * kCvHaloW;                                          \
        const int y = y0 - 1 + hy, x = x0 - 1 + hx;                                                       \
        const bool ok = idx < kCvHalo * 4 && y >= 0 && y < H && x >= 0 && x < W;                          \
        in_src##i = ok ? in_img + ((size_t)y * W + x) * cin + 4 * q : nullptr;                            \
        in_dst##i = idx < kCvHalo * 4 ? pix * kCvStride + 4 * q : -1;                                     \
    }
#define SR_LP_DECL_W(i) float4 rw##i;
#define SR_LP_FETCH_IN(i) rin##i = in_src##i ? *reinterpret_cast<const float4*>(in_src##i + c0_) : make_float4(0.0f, 0.0f, 0.0f, 0.0f);
#define SR_LP_FETCH_W(i) rw##i = wsrc_[tid + kBlock * i];
#define SR_LP_FETCH(piece)                                                                                \
    {                                                                                                     \
        const int c0_ = (piece) * kCvK;                                                                   \
        const float4* wsrc_ = reinterpret_cast<const float4*>(w_blk + (size_t)(piece) * kCvPiece);        \
        SR_LP_IN3(SR_LP_FETCH_IN) SR_LP_W9(SR_LP_FETCH_W)                                                 \
    }
#define SR_LP_STAGE_IN(i) if (in_dst##i >= 0) *reinterpret_cast<float4*>(&s_in[in_dst##i]) = rin##i;
#define SR_LP_STAGE_W(i) *reinterpret_cast<float4*>(&s_w[((tid + kBlock * i) >> 2) * kCvStride + 4 * ((tid + kBlock * i) & 3)]) = rw##i;
    SR_LP_IN3(SR_LP_DECL_IN)
    SR_LP_W9(SR_LP_DECL_W)

    // a piece (16 channels x 9 taps = 144 terms) is summed inside the MFMAs from zero, the pieces are added one after another:
    // one chain over all 9 cin terms (4608 at cin 512) would cost three times the rounding error of such a blocked sum
    f32x16 total[2];
#pragma unroll
    for (int m = 0; m < 2; ++m)
#pragma unroll
        for (int v = 0; v < 16; ++v) total[m][v] = 0.0f;

    // operand A: pixel l32 of the 2 x 16 pixels of accumulator m; operand B: result channel l32; both: channels 4 half .. + 3
    const int a_base = ((mrow0 + (l32 >> 4)) * kCvHaloW + (l32 & 15)) * kCvStride + 4 * half;
    const int b_base = (nb + l32) * kCvStride + 4 * half;

    SR_LP_FETCH(0)
    for (int piece = 0; piece < pieces; ++piece) {
        if (piece) __syncthreads();              // the previous piece has been read by every wavefront
        SR_LP_IN3(SR_LP_STAGE_IN) SR_LP_W9(SR_LP_STAGE_W)
        __syncthreads();
        if (piece + 1 < pieces) SR_LP_FETCH(piece + 1)
        f32x16 acc[2];
#pragma unroll
        for (int m = 0; m < 2; ++m)
#pragma unroll
            for (int v = 0; v < 16; ++v) acc[m][v] = 0.0f;
#pragma unroll
        for (int tap = 0; tap < 9; ++tap) {
            const int dy = tap / 3, dx = tap % 3;
#pragma unroll
            for (int g = 0; g < 2; ++g) {
                const float4 b = *reinterpret_cast<const float4*>(&s_w[b_base + tap * kCvN * kCvStride + 8 * g]);
#pragma unroll
                for (int m = 0; m < 2; ++m) {
                    const float4 a = *reinterpret_cast<const float4*>(&s_in[a_base + ((2 * m + dy) * kCvHaloW + dx) * kCvStride + 8 * g]);
                    acc[m] = __builtin_amdgcn_mfma_f32_32x32x2f32(a.x, b.x, acc[m], 0, 0, 0);
                    acc[m] = __builtin_amdgcn_mfma_f32_32x32x2f32(a.y, b.y, acc[m], 0, 0, 0);
                    acc[m] = __builtin_amdgcn_mfma_f32_32x32x2f32(a.z, b.z, acc[m], 0, 0, 0);
                    acc[m] = __builtin_amdgcn_mfma_f32_32x32x2f32(a.w, b.w, acc[m], 0, 0, 0);
                }
            }
        }
#pragma unroll
        for (int m = 0; m < 2; ++m) total[m] += acc[m];
    }

    // accumulator element v of lane: result channel l32, pixel (v & 3) + 8 (v >> 2) + 4 half of the 2 x 16
    const int co = n0 + nb + l32;
    const float bv = bias[co];
#pragma unroll
    for (int m = 0; m < 2; ++m) {
        const int yr = y0 + mrow0 + 2 * m;
        float r[16];
#pragma unroll
        for (int v = 0; v < 16; ++v) {
            r[v] = fmaxf(total[m][v] + bv, 0.0f);
            const int i = (v & 3) + 8 * (v >> 2) + 4 * half;
            const int y = yr + (i >> 4), x = x0 + (i & 15);
            if (y < H && x < W) out[(((size_t)img * H + y) * W + x) * cout + co] = r[v];
        }
        if (pooled) {
            // pixels i, i + 1 (elements v, v + 1) and i + 16, i + 17 (elements v + 8, v + 9) are one 2x2 window
            const int py = yr >> 1;
#pragma unroll
            for (int blk = 0; blk < 2; ++blk)
#pragma unroll
                for (int vb = 0; vb < 4; vb += 2) {
                    const int v = 4 * blk + vb;
                    const float mx = fmaxf(fmaxf(r[v], r[v + 1]), fmaxf(r[v + 8], r[v + 9]));
                    const int px = (x0 + 8 * blk + 4 * half + vb) >> 1;
                    if (py < d.Hp && px < d.Wp) pooled[(((size_t)img * d.Hp + py) * d.Wp + px) * cout + co] = mx;
                }
        }
    }
}

#undef SR_LP_DECL_IN
#undef SR_LP_DECL_W
#undef SR_LP_FETCH_IN
#undef SR_LP_FETCH_W
#undef SR_LP_FETCH
#undef SR_LP_STAGE_IN
#undef SR_LP_STAGE_W
#undef SR_LP_IN3
#undef SR_LP_W9

constexpr int kHeadPixels = 64, kHeadPerWave = kHeadPixels / (kBlock / kWave);   // 16 pixels per wavefront, one after another

// feat: [2 batch][px][C]; lin [C]; map (may be NULL): [batch][px]; partial: [batch][blocks_per_item] doubles
__global__ void __launch_bounds__(kBlock) k_lpips_head(int C, unsigned px, unsigned blocks_per_item, const float* __restrict__ feat,
                                                       const float* __restrict__ lin, float* __restrict__ map,
                                                       double* __restrict__ partial) {
    __shared__ double s_red[kBlock / kWave];
    const unsigned item = blockIdx.x / blocks_per_item, blk = blockIdx.x - item * blocks_per_item;
    const int lane = threadIdx.x & (kWave - 1), wave = threadIdx.x / kWave;
    const int per_lane = C / kWave;              // 1, 2, 4 or 8 channels
    float wl[8];
#pragma unroll
    for (int k = 0; k < 8; ++k) wl[k] = k < per_lane ? lin[lane + kWave * k] : 0.0f;
    const float* f0 = feat + (size_t)(2u * item) * px * C;
    const float* f1 = f0 + (size_t)px * C;
    double sum = 0.0;
    for (int j = 0; j < kHeadPerWave; ++j) {
        const unsigned p = blk * kHeadPixels + (unsigned)(wave * kHeadPerWave + j);
        if (p >= px) break;                      // the same for the whole wavefront
        const float* a_p = f0 + (size_t)p * C;
        const float* b_p = f1 + (size_t)p * C;
        float a[8], b[8], s0 = 0.0f, s1 = 0.0f;
#pragma unroll
        for (int k = 0; k < 8; ++k) {
            a[k] = k < per_lane ? a_p[lane + kWave * k] : 0.0f;
            b[k] = k < per_lane ? b_p[lane + kWave * k] : 0.0f;
            s0 = fmaf(a[k], a[k], s0);
            s1 = fmaf(b[k], b[k], s1);
        }
        const float n0 = sqrtf(__shfl(wave_sum(s0), 0, kWave)) + 1e-10f, n1 = sqrtf(__shfl(wave_sum(s1), 0, kWave)) + 1e-10f;
        float t = 0.0f;
#pragma unroll
        for (int k = 0; k < 8; ++k) {
            const float dk = __fdiv_rn(a[k], n0) - __fdiv_rn(b[k], n1);
            t = fmaf(wl[k], dk * dk, t);
        }
        t = wave_sum(t);
        if (lane == 0) {
            if (map) map[(size_t)item * px + p] = t;
            sum += (double)t;
        }
    }
    const double bs = block_sum(lane == 0 ? sum : 0.0, s_red);
    if (threadIdx.x == 0) partial[(size_t)item * blocks_per_item + blk] = bs;
}

constexpr int kLpReduceBlock = 1024;

struct ReduceDims { unsigned blocks[kLpTaps]; size_t off[kLpTaps]; double px[kLpTaps]; };

// One workgroup; wavefront w takes items w, w + 16, ...; tap by tap its lanes stride over the item's partial sums and a
// shuffle tree adds the lanes.  The order of every sum is fixed by the shape alone.
__global__ void __launch_bounds__(kLpReduceBlock) k_lpips_reduce(int batch, const ReduceDims r, const double* __restrict__ partial,
                                                                 float* __restrict__ out, float* __restrict__ out_taps) {
    const int lane = threadIdx.x & (kWave - 1), wave = threadIdx.x / kWave;
    for (int b = wave; b < batch; b += kLpReduceBlock / kWave) {
        double total = 0.0;
#pragma unroll
        for (int t = 0; t < kLpTaps; ++t) {
            const double* p = partial + r.off[t] + (size_t)b * r.blocks[t];
            double acc = 0.0;
            for (unsigned i = lane; i < r.blocks[t]; i += kWave) acc += p[i];
            acc = wave_sum(acc) / r.px[t];
            total += acc;
            if (lane == 0 && out_taps) out_taps[(size_t)b * kLpTaps + t] = (float)acc;
        }
        if (lane == 0) out[b] = (float)total;
    }
}

// ---- host side: the shape's limits, the workspace, the launches ----

struct LpShape {
    int H[kLpTaps], W[kLpTaps];
    unsigned head_blocks[kLpTaps];     // per item
    size_t partial_off[kLpTaps], partials;
    size_t act, pool;                  // floats of one full-resolution buffer and of the pooled buffer
};

// false: the shape is out of range.  Limits: 16 <= height, width <= 32768; 2 batch x the 8x16-pixel tiles of one image, and
// batch x ceil(height width / 64), each fit a grid of 2^31 - 1 workgroups
bool lp_shape(int batch, int H, int W, LpShape* s) {
    if (batch <= 0 || H < 16 || W < 16 || H > kLpMaxSide || W > kLpMaxSide) return false;
    const size_t tiles = (size_t)((H + kCvTileH - 1) / kCvTileH) * (size_t)((W + kCvTileW - 1) / kCvTileW);
    const size_t px = (size_t)H * W, limit = 0x7fffffffull;
    if (2 * (size_t)batch * tiles > limit || (size_t)batch * ((px + kHeadPixels - 1) / kHeadPixels) > limit) return false;
    LpShape t;
    size_t off = 0;
    for (int g = 0; g < kLpTaps; ++g) {
        t.H[g] = H >> g; t.W[g] = W >> g;
        t.head_blocks[g] = (unsigned)(((size_t)t.H[g] * t.W[g] + kHeadPixels - 1) / kHeadPixels);
        t.partial_off[g] = off;
        off += (size_t)batch * t.head_blocks[g];
    }
    t.partials = off;
    t.act = 2 * (size_t)batch * px * 64;
    t.pool = 2 * (size_t)batch * (size_t)(H / 2) * (size_t)(W / 2) * 64;
    if (s) *s = t;
    return true;
}

struct LpWork { float *a, *b, *pool; double* partial; };
size_t carve_lpips(void* base, const LpShape& s, LpWork* w) {
    Carver c{static_cast<char*>(base), 0};
    LpWork t;
    t.a = c.take<float>(s.act); t.b = c.take<float>(s.act); t.pool = c.take<float>(s.pool);
    t.partial = c.take<double>(s.partials);
    if (w) *w = t;
    return align_up(c.off, 256);
}

void launch_lpips(int batch, int H, int W, const float* pred, const long long* ps, const float* gt, const long long* gs, int quantize,
                  const float* packed, void* workspace, float* out, float* out_taps, float* maps, hipStream_t st) {
    LpShape s;
    lp_shape(batch, H, W, &s);
    LpWork wk;
    carve_lpips(workspace, s, &wk);
    const LpLayout L = lp_layout();
    const unsigned n_img = 2u * (unsigned)batch;

    Conv0Dims d0;
    d0.H = H; d0.W = W; d0.tiles_x = (W + 15) / 16; d0.tiles_y = (H + 15) / 16;
    for (int k = 0; k < 4; ++k) { d0.ps[k] = ps[k]; d0.gs[k] = gs[k]; }
    const dim3 g0(n_img * (unsigned)(d0.tiles_x * d0.tiles_y));
    const float *w0 = packed + L.w[0], *b0 = packed + L.b[0], *sh = packed + L.shift, *sc = packed + L.scale;
    if (quantize == SR_QUANT_PNG)
        hipLaunchKernelGGL((k_lpips_conv0<SR_QUANT_PNG>), g0, dim3(kBlock), 0, st, d0, pred, gt, w0, b0, sh, sc, wk.a);
    else if (quantize == SR_QUANT_TO8B)
        hipLaunchKernelGGL((k_lpips_conv0<SR_QUANT_TO8B>), g0, dim3(kBlock), 0, st, d0, pred, gt, w0, b0, sh, sc, wk.a);
    else
        hipLaunchKernelGGL((k_lpips_conv0<SR_QUANT_NONE>), g0, dim3(kBlock), 0, st, d0, pred, gt, w0, b0, sh, sc, wk.a);

    // the activations alternate between the two buffers; the last layer of a group also writes the pooled buffer, which the
    // first layer of the next group reads; a tap is consumed by its head launch before its buffer is written again
    float* cur = wk.a;
    float* other = wk.b;
    size_t map_off = 0;
    for (int l = 1; l < kLpLayers; ++l) {
        const int g = kLpGroup[l];
        const bool first = kLpGroup[l - 1] != g, last = l + 1 == kLpLayers || kLpGroup[l + 1] != g;
        ConvDims d;
        d.H = s.H[g]; d.W = s.W[g]; d.cin = kLpCin[l]; d.cout = kLpCout[l];
        d.tiles_x = (d.W + kCvTileW - 1) / kCvTileW; d.tiles_y = (d.H + kCvTileH - 1) / kCvTileH;
        d.Hp = d.H / 2; d.Wp = d.W / 2;
        const float* src = first ? wk.pool : cur;
        float* dst = first ? cur : other;     // after a pooled read both buffers are free
        const bool pool_out = last && g + 1 < kLpTaps;
        hipLaunchKernelGGL(k_lpips_conv, dim3(n_img * (unsigned)(d.tiles_x * d.tiles_y), (unsigned)(d.cout / kCvN)), dim3(kBlock), 0, st, d,
                           src, packed + L.w[l], packed + L.b[l], dst, pool_out ? wk.pool : nullptr);
        if (!first) { float* t = cur; cur = other; other = t; }
        if (last) {
            const unsigned px = (unsigned)(d.H * d.W);
            hipLaunchKernelGGL(k_lpips_head, dim3((unsigned)batch * s.head_blocks[g]), dim3(kBlock), 0, st, kLpTapC[g], px, s.head_blocks[g],
                               cur, packed + L.lin[g], maps ? maps + map_off : nullptr, wk.partial + s.partial_off[g]);
            map_off += (size_t)batch * px;
        }
    }
    ReduceDims r;
    for (int t = 0; t < kLpTaps; ++t) { r.blocks[t] = s.head_blocks[t]; r.off[t] = s.partial_off[t]; r.px[t] = (double)s.H[t] * s.W[t]; }
    hipLaunchKernelGGL(k_lpips_reduce, dim3(1), dim3(kLpReduceBlock), 0, st, batch, r, wk.partial, out, out_taps);
}

}  // namespace

}  // namespace sr

// ---- C entry points (include/splatraster.h): what is refused on the host, then the launchers above --------------------
using sr::fail; using sr::check_hip;

extern "C" {

size_t sr_lpips_packed_bytes(void) { return sr::lp_layout().total * sizeof(float); }

int sr_lpips_pack_weights(const float* const* conv_weights, const float* const* conv_biases, const float* const* lins,
                          const float* shift, const float* scale, void* packed, void* hip_stream) {
    if (!conv_weights || !conv_biases || !lins || !shift || !scale || !packed) return fail("null pointer in sr_lpips_pack_weights");
    for (int l = 0; l < sr::kLpLayers; ++l)
        if (!conv_weights[l] || !conv_biases[l]) return fail("null pointer in sr_lpips_pack_weights: convolution " + std::to_string(l));
    for (int t = 0; t < sr::kLpTaps; ++t)
        if (!lins[t]) return fail("null pointer in sr_lpips_pack_weights: lin " + std::to_string(t));
    if (reinterpret_cast<uintptr_t>(packed) & 255u) return fail("misaligned blob in sr_lpips_pack_weights: 256 bytes");
    const sr::LpLayout L = sr::lp_layout();
    float* dst = static_cast<float*>(packed);
    hipStream_t st = static_cast<hipStream_t>(hip_stream);
    auto copy = [&](const float* src, size_t at, int n) {
        hipLaunchKernelGGL(sr::k_lpips_copy, dim3((n + sr::kBlock - 1) / sr::kBlock), dim3(sr::kBlock), 0, st, n, src, dst + at);
    };
    for (int l = 0; l < sr::kLpLayers; ++l) {
        const size_t n = (size_t)9 * sr::kLpCin[l] * sr::kLpCout[l];
        hipLaunchKernelGGL(sr::k_lpips_pack_conv, dim3((unsigned)((n + sr::kBlock - 1) / sr::kBlock)), dim3(sr::kBlock), 0, st, sr::kLpCin[l],
                           sr::kLpCout[l], conv_weights[l], dst + L.w[l]);
        copy(conv_biases[l], L.b[l], sr::kLpCout[l]);
    }
    for (int t = 0; t < sr::kLpTaps; ++t) copy(lins[t], L.lin[t], sr::kLpTapC[t]);
    copy(shift, L.shift, 3);
    copy(scale, L.scale, 3);
    return check_hip(hipGetLastError(), "lpips_pack_weights");
}

size_t sr_lpips_workspace_bytes(int batch, int height, int width) {
    sr::LpShape s;
    return sr::lp_shape(batch, height, width, &s) ? sr::carve_lpips(nullptr, s, nullptr) : 0;
}

size_t sr_lpips_maps_floats(int batch, int height, int width) {
    sr::LpShape s;
    if (!sr::lp_shape(batch, height, width, &s)) return 0;
    size_t n = 0;
    for (int t = 0; t < sr::kLpTaps; ++t) n += (size_t)batch * s.H[t] * s.W[t];
    return n;
}

int sr_lpips_forward(int batch, int height, int width, const float* pred, const long long* pred_strides4, const float* gt,
                     const long long* gt_strides4, int quantize, const void* packed, void* workspace, float* out, float* out_taps,
                     float* maps, void* hip_stream) {
    if (batch <= 0 || height <= 0 || width <= 0) return fail("bad arguments to sr_lpips_forward: sizes must be positive");
    if (height < 16 || width < 16) return fail("bad arguments to sr_lpips_forward: relu5_3 has no pixel below height and width 16");
    if (!sr::lp_shape(batch, height, width, nullptr)) return fail("image or batch too large for sr_lpips_forward");
    if (!pred || !gt || !pred_strides4 || !gt_strides4 || !packed || !out) return fail("null pointer in sr_lpips_forward");
    if (!workspace || (reinterpret_cast<uintptr_t>(workspace) & 255u)) return fail("null or misaligned workspace in sr_lpips_forward");
    if (reinterpret_cast<uintptr_t>(packed) & 255u) return fail("misaligned blob in sr_lpips_forward: 256 bytes");
    if (sr::any_unaligned4(pred, gt, out, out_taps, maps)) return fail("misaligned pointer in sr_lpips_forward: 4 bytes");
    if (quantize != SR_QUANT_NONE && quantize != SR_QUANT_PNG && quantize != SR_QUANT_TO8B)
        return fail("bad arguments to sr_lpips_forward: unknown quantisation mode (SR_QUANT_NONE, SR_QUANT_PNG, SR_QUANT_TO8B)");
    for (int k = 0; k < 4; ++k)
        if (pred_strides4[k] < 0 || gt_strides4[k] < 0) return fail("bad arguments to sr_lpips_forward: negative stride");
    sr::launch_lpips(batch, height, width, pred, pred_strides4, gt, gt_strides4, quantize, static_cast<const float*>(packed), workspace, out,
                     out_taps, maps, static_cast<hipStream_t>(hip_stream));
    return check_hip(hipGetLastError(), "lpips_forward");
}

}  // extern "C"
