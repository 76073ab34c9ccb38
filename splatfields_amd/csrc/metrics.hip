// Evaluation metrics of a batch of views, fused (DESIGN.md "Evaluation metrics"): forward only.
//
// Restates reference render.py:33-43 (`compute_psnr`), :45-160 (`compute_ssim`, the multinerf / tf.image.ssim form with its
// defaults filter_size 11, filter_sigma 1.5, k1 0.01, k2 0.03, max_val 1), utils/image_utils.py `psnr`, and the 8-bit
// quantisation of the image files the reference reads its metrics from, per item of a [batch, 3, H, W] pair:
//
//   quantise  png:  q = trunc(clamp(x 255 + 0.5, 0, 255)),  to8b:  q = trunc(255 clamp(x, 0, 1));  both images become q / 255
//             (multiply and add rounded separately: a contracted FMA flips pixels at the half-way points);
//   window    f_i = exp(-0.5 ((i - 5) / 1.5)^2) / sum, float32; "valid": the map is (H-10) x (W-10), no padding;
//   filter    first along W, then along H.  Under a mask m (read as m != 0) each pass is the reference's partial convolution
//               r = filter(q m),  n = number of mask pixels in the 11-window,  q' = n != 0 ? (r 11) / n : 0,  m' = (n != 0)
//             and the second pass filters q' m' with the counts of m';
//   ssim      mu0, mu1, s00 = max(0, E[xx] - mu0^2), s11 likewise, s01 = sign(s01) min(sqrt(s00 s11), |s01|),
//             mean over ALL (H-10)(W-10) 3 entries of (2 mu0 mu1 + c1)(2 s01 + c2) / ((mu0^2 + mu1^2 + c1)(s00 + s11 + c2));
//             a position whose windows hold no mask pixel evaluates to exactly 1 and is counted;
//   psnr      -10 / ln 10 ln(mean squared error over the item),  psnr_channels[c] = 20 log10(1 / sqrt(mse_c)): over the full
//             H x W, never masked.
//
// k_metrics  one workgroup per 32x32 tile of the map of one (item, channel) plane: the 42x42 input region goes to LDS once,
//            quantised (and masked), the five filtered quantities go through LDS separably and never to global memory.  Each
//            input pixel is owned by exactly one tile, which adds its squared error (the product and the sum in double) and
//            stores its quantised byte when frames are asked for.  Per workgroup two partial sums in double.
// k_metrics_reduce  one workgroup; a wavefront per item adds that item's partial sums in a fixed order and writes the results.
//
// No floating-point atomics and no host wait: results are bit-identical from call to call.
#include "host_api.h"
#include "quantise.h"
#include "reduce.h"
#include "window11.h"

namespace sr {

namespace {

constexpr int kMetGroups = kWinRawStride / 4;      // a row of the region is staged as 11 groups of 4 columns
constexpr float kMetC1 = (float)(0.01 * 0.01), kMetC2 = (float)(0.03 * 0.03);   // Python doubles, rounded where they meet float32

// float32(exp(-0.5 ((i-5)/1.5)^2)) / float32 sum, as torch evaluates the filter of the reference's compute_ssim
// (tests/test_metric_reference.py compares these literals with that evaluation bit by bit)
#define SR_METRIC_TAPS { 0x1.0d9570p-10f, 0x1.f1fdf8p-8f, 0x1.26eb18p-5f, 0x1.bff0fcp-4f, 0x1.b43c3ep-3f, 0x1.106560p-2f, \
                         0x1.b43c3ep-3f, 0x1.bff0fcp-4f, 0x1.26eb18p-5f, 0x1.f1fdf8p-8f, 0x1.0d9570p-10f }

struct MetricDims {
    int batch, H, W;
    int out_h, out_w;            // H - 10, W - 10
    int tiles_x, tiles_y;
    long long ps[4], gs[4];      // element strides of pred and gt: item, channel, row, pixel
    long long mask_item;         // element stride between the masks of two items (0: one mask for all)
    int vec;                     // pixel stride 1 and everything 16-byte aligned: the region is loaded as float4
};

// the partial convolution's normalisation: n of the 11 window pixels are inside the mask
__device__ __forceinline__ float met_normalise(float r, int n) { return n != 0 ? __fdiv_rn(r * 11.0f, (float)n) : 0.0f; }

// partial: [2][blocks] doubles = the sum of the tile's similarity map | the squared error of the pixels the tile owns.
// frames (may be NULL): uint8 [batch, H, W, 3], the quantised prediction.
template <bool kMasked, int kQuant>
__global__ void __launch_bounds__(kBlock) k_metrics(const MetricDims d, const float* __restrict__ pred, const float* __restrict__ gt,
                                                    const float* __restrict__ mask, unsigned char* __restrict__ frames,
                                                    double* __restrict__ partial) {
    __shared__ __attribute__((aligned(16))) float s_raw[2][kWinRaw * kWinRawStride];
    __shared__ __attribute__((aligned(16))) float s_row[5][kWinRaw * kWinTile];
    // the mask and the first pass's mask as bytes (0 / 1): the masked kernel keeps three workgroups on a compute unit
    __shared__ __attribute__((aligned(16))) unsigned char s_mask[kMasked ? kWinRaw * kWinRawStride : 16];
    __shared__ __attribute__((aligned(16))) unsigned char s_m1[kMasked ? kWinRaw * kWinTile : 16];
    __shared__ double s_red[kBlock / kWave];

    const unsigned per_plane = (unsigned)d.tiles_x * (unsigned)d.tiles_y;
    const unsigned plane = blockIdx.x / per_plane, t_in = blockIdx.x - plane * per_plane;
    const int ty = (int)(t_in / (unsigned)d.tiles_x), tx = (int)(t_in - (unsigned)ty * (unsigned)d.tiles_x);
    const int item = (int)(plane / 3u), ch = (int)(plane - 3u * (unsigned)item);
    const int x0 = tx * kWinTile, y0 = ty * kWinTile;
    const int H = d.H, W = d.W;
    const bool last_x = tx == d.tiles_x - 1, last_y = ty == d.tiles_y - 1;
    const float* pp = pred + (long long)item * d.ps[0] + (long long)ch * d.ps[1];
    const float* pg = gt + (long long)item * d.gs[0] + (long long)ch * d.gs[1];
    const float* pm = kMasked ? mask + (long long)item * d.mask_item : nullptr;

    // ---- stage the 42 x 42 region: quantise, add up the squared error of the owned pixels, mask ----
    double sum_se = 0.0;
    for (int i = threadIdx.x; i < kWinRaw * kMetGroups; i += kBlock) {
        const int r = i / kMetGroups, g = i - r * kMetGroups;
        const int gy = y0 + r, gx0 = x0 + 4 * g;
        float xv[4] = {0.0f, 0.0f, 0.0f, 0.0f}, yv[4] = {0.0f, 0.0f, 0.0f, 0.0f};
        unsigned mbytes = 0u;
        if (gy < H && gx0 < W) {
            const int n = min(4, W - gx0);
            float mv[4] = {0.0f, 0.0f, 0.0f, 0.0f};
            if (d.vec) {   // W % 4 == 0: n == 4
                const float4 a = *reinterpret_cast<const float4*>(pp + (long long)gy * d.ps[2] + gx0);
                const float4 b = *reinterpret_cast<const float4*>(pg + (long long)gy * d.gs[2] + gx0);
                xv[0] = a.x; xv[1] = a.y; xv[2] = a.z; xv[3] = a.w;
                yv[0] = b.x; yv[1] = b.y; yv[2] = b.z; yv[3] = b.w;
                if (kMasked) {
                    const float4 m = *reinterpret_cast<const float4*>(pm + (size_t)gy * W + gx0);
                    mv[0] = m.x; mv[1] = m.y; mv[2] = m.z; mv[3] = m.w;
                }
            } else {
                const float* qx = pp + (long long)gy * d.ps[2] + (long long)gx0 * d.ps[3];
                const float* qy = pg + (long long)gy * d.gs[2] + (long long)gx0 * d.gs[3];
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    if (j < n) {
                        xv[j] = qx[j * d.ps[3]];
                        yv[j] = qy[j * d.gs[3]];
                        if (kMasked) mv[j] = pm[(size_t)gy * W + gx0 + j];
                    }
                }
            }
            const bool own_row = r < kWinTile || last_y;
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                if (j < n) {
                    const int c = 4 * g + j;
                    float level;
                    xv[j] = quantise<kQuant>(xv[j], level);
                    float unused;
                    yv[j] = quantise<kQuant>(yv[j], unused);
                    if (own_row && (c < kWinTile || (last_x && c < kWinRaw))) {
                        const double diff = (double)(xv[j] - yv[j]);
                        sum_se += diff * diff;
                        if (kQuant != SR_QUANT_NONE && frames)
                            frames[(((size_t)item * H + gy) * W + (gx0 + j)) * 3 + ch] = (unsigned char)(int)level;
                    }
                    if (kMasked) {
                        const bool in = mv[j] != 0.0f;
                        mbytes |= (in ? 1u : 0u) << (8 * j);
                        xv[j] = in ? xv[j] : 0.0f;
                        yv[j] = in ? yv[j] : 0.0f;
                    }
                }
            }
        }
        *reinterpret_cast<float4*>(&s_raw[0][r * kWinRawStride + 4 * g]) = make_float4(xv[0], xv[1], xv[2], xv[3]);
        *reinterpret_cast<float4*>(&s_raw[1][r * kWinRawStride + 4 * g]) = make_float4(yv[0], yv[1], yv[2], yv[3]);
        if (kMasked) *reinterpret_cast<unsigned*>(&s_mask[r * kWinRawStride + 4 * g]) = mbytes;
    }
    __syncthreads();

    const float taps[kWinTaps] = SR_METRIC_TAPS;

    // ---- rows: five quantities along W ----
    for (int it = threadIdx.x; it < kWinRaw * kWinQuads; it += kBlock) {
        const int r = it / kWinQuads, q = it % kWinQuads;
        float x[16], y[16], p[16], o[5][4];
        win_read_span(s_raw[0], r, q, x);
        win_read_span(s_raw[1], r, q, y);
        win_filter_span(taps, x, o[0]);
        win_filter_span(taps, y, o[1]);
#pragma unroll
        for (int j = 0; j < 14; ++j) p[j] = x[j] * x[j];
        win_filter_span(taps, p, o[2]);
#pragma unroll
        for (int j = 0; j < 14; ++j) p[j] = y[j] * y[j];
        win_filter_span(taps, p, o[3]);
#pragma unroll
        for (int j = 0; j < 14; ++j) p[j] = x[j] * y[j];
        win_filter_span(taps, p, o[4]);
        if (kMasked) {
            const unsigned* mw = reinterpret_cast<const unsigned*>(&s_mask[r * kWinRawStride + 4 * q]);
            int b[16];
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const unsigned w = mw[k];
#pragma unroll
                for (int j = 0; j < 4; ++j) b[4 * k + j] = (int)((w >> (8 * j)) & 1u);
            }
            int n[4];
            n[0] = 0;
#pragma unroll
            for (int t = 0; t < kWinTaps; ++t) n[0] += b[t];
#pragma unroll
            for (int j = 1; j < 4; ++j) n[j] = n[j - 1] - b[j - 1] + b[j + kWinTaps - 1];
            unsigned m1 = 0u;
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                m1 |= (n[j] != 0 ? 1u : 0u) << (8 * j);
#pragma unroll
                for (int k = 0; k < 5; ++k) o[k][j] = met_normalise(o[k][j], n[j]);
            }
            *reinterpret_cast<unsigned*>(&s_m1[r * kWinTile + 4 * q]) = m1;
        }
#pragma unroll
        for (int k = 0; k < 5; ++k)
            *reinterpret_cast<float4*>(&s_row[k][r * kWinTile + 4 * q]) = make_float4(o[k][0], o[k][1], o[k][2], o[k][3]);
    }
    __syncthreads();

    // ---- columns: the same along H, then the similarity of this thread's 4 outputs ----
    const int row = threadIdx.x / kWinQuads, quad = threadIdx.x % kWinQuads;
    float o[5][4];
#pragma unroll
    for (int k = 0; k < 5; ++k) win_filter_column(taps, s_row[k], row, quad, o[k]);
    if (kMasked) {
        unsigned packed = 0u;   // four byte counters, at most 11 each
#pragma unroll
        for (int t = 0; t < kWinTaps; ++t) packed += *reinterpret_cast<const unsigned*>(&s_m1[(row + t) * kWinTile + 4 * quad]);
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int n = (int)((packed >> (8 * j)) & 0xffu);
#pragma unroll
            for (int k = 0; k < 5; ++k) o[k][j] = met_normalise(o[k][j], n);
        }
    }
    const int oy = y0 + row, ox = x0 + 4 * quad;
    const int n_valid = oy < d.out_h ? min(4, d.out_w - ox) : 0;   // <= 0: none
    float sum_s = 0.0f;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const float mu0 = o[0][j], mu1 = o[1][j];
        const float mu00 = mu0 * mu0, mu11 = mu1 * mu1, mu01 = mu0 * mu1;
        const float s00 = fmaxf(0.0f, o[2][j] - mu00), s11 = fmaxf(0.0f, o[3][j] - mu11);
        const float raw01 = o[4][j] - mu01;
        const float s01 = copysignf(fminf(sqrtf(s00 * s11), fabsf(raw01)), raw01);
        const float numer = (2.0f * mu01 + kMetC1) * (2.0f * s01 + kMetC2);
        const float denom = (mu00 + mu11 + kMetC1) * (s00 + s11 + kMetC2);
        const float v = __fdiv_rn(numer, denom);
        if (j < n_valid) sum_s += v;
    }
    const double bs = block_sum((double)sum_s, s_red), be = block_sum(sum_se, s_red);
    if (threadIdx.x == 0) {
        partial[blockIdx.x] = bs;
        partial[(size_t)gridDim.x + blockIdx.x] = be;
    }
}

constexpr int kMetReduceBlock = 1024;

// One workgroup; wavefront w takes items w, w + 16, ...: its lanes stride over the item's tiles, a shuffle tree adds the
// lanes.  The order of every sum is fixed by the shape alone.
__global__ void __launch_bounds__(kMetReduceBlock) k_metrics_reduce(int batch, unsigned tiles_per_plane, double px_per_plane,
                                                                    double out_per_item, const double* __restrict__ partial,
                                                                    float* __restrict__ psnr, float* __restrict__ ssim,
                                                                    float* __restrict__ psnr_channels) {
    const int lane = threadIdx.x & (kWave - 1), wave = threadIdx.x / kWave;
    const size_t blocks = (size_t)batch * 3u * tiles_per_plane;
    for (int b = wave; b < batch; b += kMetReduceBlock / kWave) {
        double acc_s = 0.0, acc_e[3] = {0.0, 0.0, 0.0};
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const size_t first = ((size_t)b * 3u + c) * tiles_per_plane;
            for (unsigned t = lane; t < tiles_per_plane; t += kWave) {
                acc_s += partial[first + t];
                acc_e[c] += partial[blocks + first + t];
            }
        }
        acc_s = wave_sum(acc_s);
#pragma unroll
        for (int c = 0; c < 3; ++c) acc_e[c] = wave_sum(acc_e[c]);
        if (lane == 0) {
            ssim[b] = (float)(acc_s / out_per_item);
            const double mse = ((acc_e[0] + acc_e[1]) + acc_e[2]) / (3.0 * px_per_plane);
            psnr[b] = (float)(-10.0 / log(10.0) * log(mse));
#pragma unroll
            for (int c = 0; c < 3; ++c) psnr_channels[3 * b + c] = (float)(20.0 * log10(1.0 / sqrt(acc_e[c] / px_per_plane)));
        }
    }
}

// tiles of the (H-10) x (W-10) map of every plane; 0 when the shape is out of range or the grid would not fit: a launch
// takes fewer than 2^32 threads, so at most (2^32 - 1) / 256 workgroups
constexpr size_t kMetMaxBlocks = 0xffffffffull / kBlock;
size_t metric_blocks(int batch, int H, int W) {
    if (batch <= 0 || H < kWinTaps || W < kWinTaps) return 0;
    const size_t ty = (size_t)(H - kWinTaps + 1 + kWinTile - 1) / kWinTile, tx = (size_t)(W - kWinTaps + 1 + kWinTile - 1) / kWinTile;
    const size_t per_plane = ty * tx;   // < 2^52
    if (per_plane > kMetMaxBlocks || (size_t)batch > kMetMaxBlocks / 3u) return 0;
    const size_t n = (size_t)batch * 3u * per_plane;
    return n <= kMetMaxBlocks ? n : 0;
}

template <bool kMasked>
void launch_metrics_quant(int quantize, unsigned nb, hipStream_t st, const MetricDims& d, const float* pred, const float* gt,
                          const float* mask, unsigned char* frames, double* partial) {
    if (quantize == SR_QUANT_PNG)
        hipLaunchKernelGGL((k_metrics<kMasked, SR_QUANT_PNG>), dim3(nb), dim3(kBlock), 0, st, d, pred, gt, mask, frames, partial);
    else if (quantize == SR_QUANT_TO8B)
        hipLaunchKernelGGL((k_metrics<kMasked, SR_QUANT_TO8B>), dim3(nb), dim3(kBlock), 0, st, d, pred, gt, mask, frames, partial);
    else
        hipLaunchKernelGGL((k_metrics<kMasked, SR_QUANT_NONE>), dim3(nb), dim3(kBlock), 0, st, d, pred, gt, mask, frames, partial);
}

bool metrics_shape_ok(int batch, int H, int W) { return metric_blocks(batch, H, W) > 0; }

size_t metrics_workspace_bytes(int batch, int H, int W) {
    const size_t nb = metric_blocks(batch, H, W);
    return nb ? align_up(2 * sizeof(double) * nb, 256) : 0;
}

void launch_image_metrics(int batch, int H, int W, const float* pred, const long long* pred_strides, const float* gt,
                          const long long* gt_strides, const float* mask, long long mask_item_stride, int quantize, void* workspace,
                          float* psnr, float* ssim, float* psnr_channels, unsigned char* frames, hipStream_t st) {
    MetricDims d;
    d.batch = batch; d.H = H; d.W = W;
    d.out_h = H - kWinTaps + 1; d.out_w = W - kWinTaps + 1;
    d.tiles_x = (d.out_w + kWinTile - 1) / kWinTile; d.tiles_y = (d.out_h + kWinTile - 1) / kWinTile;
    d.mask_item = mask_item_stride;
    bool vec = (W % 4) == 0 && aligned16(pred) && aligned16(gt) && aligned16(mask) && (mask_item_stride % 4) == 0;
    for (int k = 0; k < 4; ++k) {
        d.ps[k] = pred_strides[k]; d.gs[k] = gt_strides[k];
        if (k < 3) vec = vec && (pred_strides[k] % 4) == 0 && (gt_strides[k] % 4) == 0;
    }
    d.vec = vec && pred_strides[3] == 1 && gt_strides[3] == 1;
    const size_t nb = metric_blocks(batch, H, W);
    double* partial = static_cast<double*>(workspace);
    if (mask) launch_metrics_quant<true>(quantize, (unsigned)nb, st, d, pred, gt, mask, frames, partial);
    else launch_metrics_quant<false>(quantize, (unsigned)nb, st, d, pred, gt, mask, frames, partial);
    hipLaunchKernelGGL(k_metrics_reduce, dim3(1), dim3(kMetReduceBlock), 0, st, batch, (unsigned)(d.tiles_x * d.tiles_y), (double)H * W,
                       3.0 * (double)d.out_h * (double)d.out_w, partial, psnr, ssim, psnr_channels);
}

}  // namespace

}  // namespace sr

// ---- C entry points (include/splatraster.h): what is refused on the host, then the launchers above --------------------
using sr::fail; using sr::check_hip;

extern "C" {

size_t sr_metrics_workspace_bytes(int batch, int height, int width) { return sr::metrics_workspace_bytes(batch, height, width); }

int sr_image_metrics(int batch, int height, int width, const float* pred, const long long* pred_strides4, const float* gt,
                     const long long* gt_strides4, const float* mask, long long mask_item_stride, int quantize, void* workspace,
                     float* psnr, float* ssim, float* psnr_channels, unsigned char* frames, void* hip_stream) {
    if (batch <= 0 || height <= 0 || width <= 0) return fail("bad arguments to sr_image_metrics: sizes must be positive");
    if (height < 11 || width < 11) return fail("bad arguments to sr_image_metrics: the 11-tap valid window needs height and width >= 11");
    if (!sr::metrics_shape_ok(batch, height, width)) return fail("image too large for sr_image_metrics");
    if (!pred || !gt || !pred_strides4 || !gt_strides4 || !workspace || !psnr || !ssim || !psnr_channels) return fail("null pointer in sr_image_metrics");
    if (quantize != SR_QUANT_NONE && quantize != SR_QUANT_PNG && quantize != SR_QUANT_TO8B)
        return fail("bad arguments to sr_image_metrics: unknown quantisation mode (SR_QUANT_NONE, SR_QUANT_PNG, SR_QUANT_TO8B)");
    if (frames && quantize == SR_QUANT_NONE) return fail("sr_image_metrics: frames are the quantised prediction and need a quantisation mode");
    for (int k = 0; k < 4; ++k)
        if (pred_strides4[k] < 0 || gt_strides4[k] < 0) return fail("bad arguments to sr_image_metrics: negative stride");
    if (mask && mask_item_stride != 0 && mask_item_stride < (long long)height * width)
        return fail("bad arguments to sr_image_metrics: mask_item_stride must be 0 or at least height * width");
    sr::launch_image_metrics(batch, height, width, pred, pred_strides4, gt, gt_strides4, mask, mask_item_stride, quantize, workspace, psnr,
                             ssim, psnr_channels, frames, static_cast<hipStream_t>(hip_stream));
    return check_hip(hipGetLastError(), "image_metrics");
}

}  // extern "C"
