// The photometric loss of a training step, fused (DESIGN.md "Photometric loss").
//
// Restates reference utils/loss_utils.py:18 (`l1_loss`), :33-76 (`ssim`) and train.py:183-193 (their blend with the opacity
// mask term) per plane of a [planes, H, W] image:
//
//   window   11 taps, sigma 1.5, rounded to float32 and normalised in float32 as the reference's `gaussian()` does;
//            zero padding of 5 (conv2d(padding=5): the window is NOT renormalised at the border);
//   mu = w*x,  s11 = w*(x x) - mu1^2,  s22 = w*(y y) - mu2^2,  s12 = w*(x y) - mu1 mu2,
//   A = 2 mu1 mu2 + C1,  B = 2 s12 + C2,  D = mu1^2 + mu2^2 + C1,  E = s11 + s22 + C2,  S = A B / (D E),  ssim = mean(S);
//   l1 = mean|x - y|;   mask_l1 = mean|clamp(a, 0, 1) - m|.
//
// forward   one workgroup per 32x32 tile of one plane: the tile and its halo of 5 go to LDS once, the five filtered
//           quantities go through LDS separably (rows, then columns) and never to global memory.  Per workgroup one partial
//           sum each of S, |x - y| and |clamp(a) - m|; when a backward will follow, the three per-pixel derivative maps
//             P_mu = dS/dmu1 = 2 mu2 (B - A)/(D E) - 2 mu1 S/D + 2 mu1 S/E,   P_a = dS/d(w*xx) = -S/E,   P_c = dS/d(w*xy) = 2A/(D E)
//           are stored (see DESIGN.md for the store-or-recompute arithmetic).
// reduce    one workgroup adds the partial sums in a fixed order (double accumulators) and writes the four values.
// backward  the same tile walk over the three maps:
//             dL/dx = g [ w_l1 sign(x - y)/n + w_ssim/n (w*P_mu + 2x (w*P_a) + y (w*P_c)) ]
//             dL/da = g w_mask sign(clamp(a) - m) [0 <= a <= 1] / n_mask
//           with the upstream gradient g read from device memory.
//
// No floating-point atomics anywhere: values and gradients are bit-identical from call to call.
#include "host_api.h"
#include "reduce.h"
#include "window11.h"

namespace sr {

namespace {

constexpr float kC1 = 0.01f * 0.01f, kC2 = 0.03f * 0.03f;

// float32(exp(-(i-5)^2 / 4.5)) / float32 sum, as torch evaluates the reference's gaussian(11, 1.5)
// (tests/test_loss_reference.py compares these literals with that evaluation bit by bit)
#define SR_LOSS_TAPS { 0x1.0d956cp-10f, 0x1.f1fe02p-8f, 0x1.26eb18p-5f, 0x1.bff0fep-4f, 0x1.b43c3ep-3f, 0x1.106560p-2f, \
                       0x1.b43c3ep-3f, 0x1.bff0fep-4f, 0x1.26eb18p-5f, 0x1.f1fe02p-8f, 0x1.0d956cp-10f }

struct LossDims {
    int planes, channels, H, W;
    int tiles_x, tiles_y;
    int vec;   // W % 4 == 0 and every base pointer 16-byte aligned: centre loads and stores are float4
};

// the haloed tile of one plane -> LDS, zero outside the image (the reference's zero padding)
__device__ __forceinline__ void load_haloed(const float* __restrict__ plane, int H, int W, int x0, int y0, float* __restrict__ s) {
    for (int i = threadIdx.x; i < kWinRaw * kWinRaw; i += kBlock) {
        const int r = i / kWinRaw, c = i - r * kWinRaw;
        const int gy = y0 + r - kWinHalo, gx = x0 + c - kWinHalo;
        const bool in = gy >= 0 && gy < H && gx >= 0 && gx < W;
        s[r * kWinRawStride + c] = in ? plane[(size_t)gy * W + gx] : 0.0f;
    }
}

// row pass: the 4 filtered outputs of a span -> their 16-byte slot of a row-filtered plane (`dst` without __restrict__: with it
// the backward filters its three maps one after another instead of interleaved)
__device__ __forceinline__ void filter_span_to(const float (&w)[kWinTaps], const float (&v)[16], float* dst) {
    float o[4];
    win_filter_span(w, v, o);
    *reinterpret_cast<float4*>(dst) = make_float4(o[0], o[1], o[2], o[3]);
}

__device__ __forceinline__ void load4(const float* __restrict__ p, int n_valid, int vec, float (&v)[4]) {
    if (vec) {
        const float4 q = *reinterpret_cast<const float4*>(p);
        v[0] = q.x; v[1] = q.y; v[2] = q.z; v[3] = q.w;
    } else {
#pragma unroll
        for (int j = 0; j < 4; ++j) v[j] = j < n_valid ? p[j] : 0.0f;
    }
}

__device__ __forceinline__ void store4(float* __restrict__ p, int n_valid, int vec, const float (&v)[4]) {
    if (vec) {
        *reinterpret_cast<float4*>(p) = make_float4(v[0], v[1], v[2], v[3]);
    } else {
#pragma unroll
        for (int j = 0; j < 4; ++j) if (j < n_valid) p[j] = v[j];
    }
}

__device__ __forceinline__ float clamp01(float a) { return a < 0.0f ? 0.0f : (a > 1.0f ? 1.0f : a); }   // keeps NaN, as torch.clamp

struct TilePos { int plane, x0, y0; };

__device__ __forceinline__ TilePos tile_of_block(const LossDims& d) {
    const unsigned b = blockIdx.x;
    const unsigned per_plane = (unsigned)d.tiles_x * (unsigned)d.tiles_y;
    const unsigned plane = b / per_plane, t = b - plane * per_plane;
    const unsigned ty = t / (unsigned)d.tiles_x, tx = t - ty * (unsigned)d.tiles_x;
    return {(int)plane, (int)tx * kWinTile, (int)ty * kWinTile};
}

// partial: [3][blocks] = sum S | sum |x - y| | sum |clamp(a) - m| of each workgroup's tile.  maps (may be NULL):
// [3][planes][H][W] = P_mu | P_a | P_c.
__global__ void __launch_bounds__(kBlock) k_loss_forward(const LossDims d, const float* __restrict__ image, const float* __restrict__ gt,
                                                         const float* __restrict__ alpha, const float* __restrict__ gt_mask, int do_ssim,
                                                         float* __restrict__ maps, float* __restrict__ partial) {
    __shared__ __attribute__((aligned(16))) float s_raw[2][kWinRaw * kWinRawStride];
    __shared__ __attribute__((aligned(16))) float s_row[5][kWinRaw * kWinTile];
    __shared__ float s_red[kBlock / kWave];
    const TilePos tp = tile_of_block(d);
    const int H = d.H, W = d.W;
    const size_t plane_px = (size_t)H * W;
    const float* px = image + (size_t)tp.plane * plane_px;
    const float* py = gt + (size_t)tp.plane * plane_px;
    const int row = threadIdx.x / kWinQuads, quad = threadIdx.x % kWinQuads;   // this thread's 4 pixels in the column pass
    const int gy = tp.y0 + row, gx = tp.x0 + 4 * quad;
    const int n_valid = gy < H ? min(4, W - gx) : 0;                              // <= 0: none

    float sum_s = 0.0f, sum_l1 = 0.0f, sum_mask = 0.0f;
    if (do_ssim) {
        const float taps[kWinTaps] = SR_LOSS_TAPS;
        load_haloed(px, H, W, tp.x0, tp.y0, s_raw[0]);
        load_haloed(py, H, W, tp.x0, tp.y0, s_raw[1]);
        __syncthreads();
        for (int item = threadIdx.x; item < kWinRaw * kWinQuads; item += kBlock) {   // rows
            const int r = item / kWinQuads, q = item % kWinQuads;
            float x[16], y[16], p[16];
            win_read_span(s_raw[0], r, q, x);
            win_read_span(s_raw[1], r, q, y);
            float* out = &s_row[0][r * kWinTile + 4 * q];
            constexpr int kPlane = kWinRaw * kWinTile;
            filter_span_to(taps, x, out);
            filter_span_to(taps, y, out + kPlane);
#pragma unroll
            for (int j = 0; j < 14; ++j) p[j] = x[j] * x[j];
            filter_span_to(taps, p, out + 2 * kPlane);
#pragma unroll
            for (int j = 0; j < 14; ++j) p[j] = y[j] * y[j];
            filter_span_to(taps, p, out + 3 * kPlane);
#pragma unroll
            for (int j = 0; j < 14; ++j) p[j] = x[j] * y[j];
            filter_span_to(taps, p, out + 4 * kPlane);
        }
        __syncthreads();
        float mu1[4], mu2[4], xx[4], yy[4], xy[4];   // columns
        win_filter_column(taps, s_row[0], row, quad, mu1);
        win_filter_column(taps, s_row[1], row, quad, mu2);
        win_filter_column(taps, s_row[2], row, quad, xx);
        win_filter_column(taps, s_row[3], row, quad, yy);
        win_filter_column(taps, s_row[4], row, quad, xy);
        float p_mu[4], p_a[4], p_c[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const float mu1_sq = mu1[j] * mu1[j], mu2_sq = mu2[j] * mu2[j], mu12 = mu1[j] * mu2[j];
            const float s11 = xx[j] - mu1_sq, s22 = yy[j] - mu2_sq, s12 = xy[j] - mu12;
            const float A = 2.0f * mu12 + kC1, B = 2.0f * s12 + kC2, D = mu1_sq + mu2_sq + kC1, E = s11 + s22 + kC2;
            const float inv_d = 1.0f / D, inv_e = 1.0f / E;
            const float S = (A * B) * (inv_d * inv_e);
            if (j < n_valid) sum_s += S;
            p_a[j] = -S * inv_e;
            p_c[j] = 2.0f * A * (inv_d * inv_e);
            p_mu[j] = 2.0f * mu2[j] * (B - A) * (inv_d * inv_e) + 2.0f * mu1[j] * S * (inv_e - inv_d);
        }
        if (maps && n_valid > 0) {
            const size_t off = (size_t)tp.plane * plane_px + (size_t)gy * W + gx, all = (size_t)d.planes * plane_px;
            store4(maps + off, n_valid, d.vec, p_mu);
            store4(maps + all + off, n_valid, d.vec, p_a);
            store4(maps + 2 * all + off, n_valid, d.vec, p_c);
        }
        if (n_valid > 0) {   // |x - y| of the same pixels, from the tile in LDS
            const float* cx = &s_raw[0][(row + kWinHalo) * kWinRawStride + 4 * quad + kWinHalo];
            const float* cy = &s_raw[1][(row + kWinHalo) * kWinRawStride + 4 * quad + kWinHalo];
#pragma unroll
            for (int j = 0; j < 4; ++j) if (j < n_valid) sum_l1 += fabsf(cx[j] - cy[j]);
        }
    } else if (n_valid > 0) {
        const size_t off = (size_t)gy * W + gx;
        float x[4], y[4];
        load4(px + off, n_valid, d.vec, x);
        load4(py + off, n_valid, d.vec, y);
#pragma unroll
        for (int j = 0; j < 4; ++j) if (j < n_valid) sum_l1 += fabsf(x[j] - y[j]);
    }
    if (alpha && tp.plane % d.channels == 0 && n_valid > 0) {   // the first channel's workgroups also cover the opacity plane
        const size_t off = (size_t)(tp.plane / d.channels) * plane_px + (size_t)gy * W + gx;
        float a[4], m[4];
        load4(alpha + off, n_valid, d.vec, a);
        load4(gt_mask + off, n_valid, d.vec, m);
#pragma unroll
        for (int j = 0; j < 4; ++j) if (j < n_valid) sum_mask += fabsf(clamp01(a[j]) - m[j]);
    }
    const float bs = block_sum(sum_s, s_red), bl = block_sum(sum_l1, s_red), bm = block_sum(sum_mask, s_red);
    if (threadIdx.x == 0) {
        const size_t nb = gridDim.x;
        partial[blockIdx.x] = bs;
        partial[nb + blockIdx.x] = bl;
        partial[2 * nb + blockIdx.x] = bm;
    }
}

constexpr int kReduceBlock = 1024;

// sum of v[0 .. n) in a fixed order, in every thread
__device__ __forceinline__ double reduce_range(const float* __restrict__ v, size_t n, double* s) {
    double acc = 0.0;
    for (size_t i = threadIdx.x; i < n; i += kReduceBlock) acc += (double)v[i];
    return block_tree_sum<double, kReduceBlock>(acc, s);
}

__global__ void __launch_bounds__(kReduceBlock) k_loss_reduce(size_t blocks, int batch, size_t blocks_per_item, double px_per_item,
                                                              double px_per_alpha, const float* __restrict__ partial, int do_ssim,
                                                              int has_mask, float lambda_dssim, float lambda_mask, float* __restrict__ loss,
                                                              float* __restrict__ l1, float* __restrict__ ssim, float* __restrict__ mask_l1) {
    __shared__ double s[kReduceBlock];
    const double v_l1 = reduce_range(partial + blocks, blocks, s) / (px_per_item * batch);
    const double v_mask = has_mask ? reduce_range(partial + 2 * blocks, blocks, s) / (px_per_alpha * batch) : 0.0;
    double all_s = 0.0;
    if (do_ssim) {
        for (int b = 0; b < batch; ++b) {
            const double item = reduce_range(partial + (size_t)b * blocks_per_item, blocks_per_item, s);
            all_s += item;
            if (threadIdx.x == 0) ssim[b] = (float)(item / px_per_item);
        }
    }
    if (threadIdx.x == 0) {
        const double v_ssim = all_s / (px_per_item * batch);
        double v = (1.0 - (double)lambda_dssim) * v_l1;
        if (do_ssim) v += (double)lambda_dssim * (1.0 - v_ssim);
        if (has_mask) v += (double)lambda_mask * v_mask;
        *loss = (float)v;
        *l1 = (float)v_l1;
        if (has_mask) *mask_l1 = (float)v_mask;
    }
}

__global__ void __launch_bounds__(kBlock) k_loss_backward(const LossDims d, const float* __restrict__ image, const float* __restrict__ gt,
                                                          const float* __restrict__ alpha, const float* __restrict__ gt_mask,
                                                          const float* __restrict__ maps, float c_l1, float c_ssim, float c_mask,
                                                          const float* __restrict__ g, int g_per_item, float* __restrict__ dL_dimage,
                                                          float* __restrict__ dL_dalpha) {
    __shared__ __attribute__((aligned(16))) float s_raw[3][kWinRaw * kWinRawStride];
    __shared__ __attribute__((aligned(16))) float s_row[3][kWinRaw * kWinTile];
    const TilePos tp = tile_of_block(d);
    const int H = d.H, W = d.W;
    const size_t plane_px = (size_t)H * W, all = (size_t)d.planes * plane_px;
    const int item_idx = tp.plane / d.channels;
    const float gv = g[g_per_item ? item_idx : 0];
    const int row = threadIdx.x / kWinQuads, quad = threadIdx.x % kWinQuads;
    const int gy = tp.y0 + row, gx = tp.x0 + 4 * quad;
    const int n_valid = gy < H ? min(4, W - gx) : 0;

    float conv_mu[4] = {0.0f, 0.0f, 0.0f, 0.0f}, conv_a[4] = {0.0f, 0.0f, 0.0f, 0.0f}, conv_c[4] = {0.0f, 0.0f, 0.0f, 0.0f};
    if (maps) {
        const float taps[kWinTaps] = SR_LOSS_TAPS;
#pragma unroll
        for (int m = 0; m < 3; ++m) load_haloed(maps + m * all + (size_t)tp.plane * plane_px, H, W, tp.x0, tp.y0, s_raw[m]);
        __syncthreads();
        for (int item = threadIdx.x; item < kWinRaw * kWinQuads; item += kBlock) {
            const int r = item / kWinQuads, q = item % kWinQuads;
#pragma unroll
            for (int m = 0; m < 3; ++m) {
                float v[16];
                win_read_span(s_raw[m], r, q, v);
                filter_span_to(taps, v, &s_row[m][r * kWinTile + 4 * q]);
            }
        }
        __syncthreads();
        win_filter_column(taps, s_row[0], row, quad, conv_mu);
        win_filter_column(taps, s_row[1], row, quad, conv_a);
        win_filter_column(taps, s_row[2], row, quad, conv_c);
    }
    if (n_valid <= 0) return;
    const size_t px_off = (size_t)gy * W + gx;
    {
        const size_t off = (size_t)tp.plane * plane_px + px_off;
        float x[4], y[4], out[4];
        load4(image + off, n_valid, d.vec, x);
        load4(gt + off, n_valid, d.vec, y);
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const float diff = x[j] - y[j];
            const float sgn = (float)((diff > 0.0f) - (diff < 0.0f));
            const float ds = conv_mu[j] + 2.0f * x[j] * conv_a[j] + y[j] * conv_c[j];
            const float t = c_l1 * sgn + c_ssim * ds;
            out[j] = gv * t;    // the upstream gradient multiplies last: a power-of-two g scales the result exactly
        }
        store4(dL_dimage + off, n_valid, d.vec, out);
    }
    if (dL_dalpha && tp.plane % d.channels == 0) {
        const size_t off = (size_t)item_idx * plane_px + px_off;
        float a[4], m[4], out[4];
        load4(alpha + off, n_valid, d.vec, a);
        load4(gt_mask + off, n_valid, d.vec, m);
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const float diff = clamp01(a[j]) - m[j];
            const float sgn = (float)((diff > 0.0f) - (diff < 0.0f));
            const float t = (a[j] >= 0.0f && a[j] <= 1.0f) ? c_mask * sgn : 0.0f;
            out[j] = gv * t;
        }
        store4(dL_dalpha + off, n_valid, d.vec, out);
    }
}

// 0 when the tile count does not fit a grid
size_t loss_blocks(int planes, int H, int W) {
    if (planes <= 0 || H <= 0 || W <= 0) return 0;
    const size_t n = (size_t)planes * (size_t)((H + kWinTile - 1) / kWinTile) * (size_t)((W + kWinTile - 1) / kWinTile);
    return n <= 0x7fffffffull ? n : 0;
}

LossDims loss_dims(int batch, int channels, int H, int W) {
    LossDims d;
    d.planes = batch * channels; d.channels = channels; d.H = H; d.W = W;
    d.tiles_x = (W + kWinTile - 1) / kWinTile; d.tiles_y = (H + kWinTile - 1) / kWinTile;
    d.vec = (W % 4) == 0;
    return d;
}

bool loss_shape_ok(int batch, int channels, int H, int W) {
    return batch > 0 && channels > 0 && (long long)batch * channels <= 0x7fffffffll && loss_blocks(batch * channels, H, W) > 0;
}

size_t loss_workspace_bytes(int planes, int H, int W) {
    const size_t nb = loss_blocks(planes, H, W);
    return nb ? align_up(3 * sizeof(float) * nb, 256) : 0;
}

size_t loss_maps_bytes(int planes, int H, int W) {
    return loss_blocks(planes, H, W) ? align_up(3 * sizeof(float) * (size_t)planes * H * W, 256) : 0;
}

void launch_loss_forward(int batch, int channels, int H, int W, const float* image, const float* gt, const float* alpha,
                         const float* gt_mask, float lambda_dssim, float lambda_mask, void* workspace, float* maps, float* loss,
                         float* l1, float* ssim, float* mask_l1, hipStream_t st) {
    LossDims d = loss_dims(batch, channels, H, W);
    d.vec = d.vec && aligned16(image) && aligned16(gt) && aligned16(alpha) && aligned16(gt_mask) && aligned16(maps);
    const size_t nb = loss_blocks(d.planes, H, W);
    float* partial = static_cast<float*>(workspace);
    const int do_ssim = ssim != nullptr;
    hipLaunchKernelGGL(k_loss_forward, dim3((unsigned)nb), dim3(kBlock), 0, st, d, image, gt, alpha, gt_mask, do_ssim, maps, partial);
    hipLaunchKernelGGL(k_loss_reduce, dim3(1), dim3(kReduceBlock), 0, st, nb, batch, nb / (size_t)batch, (double)channels * H * W,
                       (double)H * W, partial, do_ssim, alpha != nullptr, lambda_dssim, lambda_mask, loss, l1, ssim, mask_l1);
}

void launch_loss_backward(int batch, int channels, int H, int W, const float* image, const float* gt, const float* alpha,
                          const float* gt_mask, const float* maps, float w_l1, float w_ssim, float w_mask, const float* g, int g_per_item,
                          float* dL_dimage, float* dL_dalpha, hipStream_t st) {
    LossDims d = loss_dims(batch, channels, H, W);
    d.vec = d.vec && aligned16(image) && aligned16(gt) && aligned16(alpha) && aligned16(gt_mask) && aligned16(dL_dimage) && aligned16(dL_dalpha);
    const size_t nb = loss_blocks(d.planes, H, W);
    const double n_item = (double)channels * H * W, n_all = n_item * batch;
    // every mean is over all items except the structural similarity of a per-item upstream gradient (size_average=False)
    const float c_l1 = (float)((double)w_l1 / n_all), c_ssim = (float)((double)w_ssim / (g_per_item ? n_item : n_all));
    const float c_mask = (float)((double)w_mask / ((double)H * W * batch));
    hipLaunchKernelGGL(k_loss_backward, dim3((unsigned)nb), dim3(kBlock), 0, st, d, image, gt, alpha, gt_mask, maps, c_l1, c_ssim, c_mask, g,
                       g_per_item, dL_dimage, dL_dalpha);
}

}  // namespace

}  // namespace sr

// ---- C entry points (include/splatraster.h): what is refused on the host, then the launchers above --------------------
using sr::fail; using sr::check_hip;

extern "C" {

size_t sr_loss_workspace_bytes(int planes, int height, int width) { return sr::loss_workspace_bytes(planes, height, width); }

size_t sr_loss_maps_bytes(int planes, int height, int width) { return sr::loss_maps_bytes(planes, height, width); }

int sr_photometric_forward(int batch, int channels, int height, int width, const float* image, const float* gt, const float* alpha,
                           const float* gt_mask, float lambda_dssim, float lambda_mask, void* workspace, float* maps, float* loss,
                           float* l1, float* ssim, float* mask_l1, void* hip_stream) {
    if (batch <= 0 || channels <= 0 || height <= 0 || width <= 0) return fail("bad arguments to sr_photometric_forward: sizes must be positive");
    if (!sr::loss_shape_ok(batch, channels, height, width)) return fail("image too large for sr_photometric_forward");
    if (!image || !gt || !workspace || !loss || !l1) return fail("null pointer in sr_photometric_forward");
    if ((alpha == nullptr) != (gt_mask == nullptr)) return fail("sr_photometric_forward: alpha and gt_mask go together (both or neither)");
    if (alpha && !mask_l1) return fail("null pointer in sr_photometric_forward: mask_l1 is written when alpha is given");
    if (!alpha && lambda_mask != 0.0f) return fail("sr_photometric_forward: lambda_mask without alpha and gt_mask");
    if (!ssim && (lambda_dssim != 0.0f || maps)) return fail("sr_photometric_forward: the ssim output may be omitted only with lambda_dssim = 0 and no maps");
    sr::launch_loss_forward(batch, channels, height, width, image, gt, alpha, gt_mask, lambda_dssim, lambda_mask, workspace, maps, loss, l1,
                            ssim, mask_l1, static_cast<hipStream_t>(hip_stream));
    return check_hip(hipGetLastError(), "photometric_forward");
}

int sr_photometric_backward(int batch, int channels, int height, int width, const float* image, const float* gt, const float* alpha,
                            const float* gt_mask, const float* maps, float w_l1, float w_ssim, float w_mask, const float* upstream,
                            int upstream_per_item, float* dL_dimage, float* dL_dalpha, void* hip_stream) {
    if (batch <= 0 || channels <= 0 || height <= 0 || width <= 0) return fail("bad arguments to sr_photometric_backward: sizes must be positive");
    if (!sr::loss_shape_ok(batch, channels, height, width)) return fail("image too large for sr_photometric_backward");
    if (!image || !gt || !upstream || !dL_dimage) return fail("null pointer in sr_photometric_backward");
    if ((alpha == nullptr) != (gt_mask == nullptr)) return fail("sr_photometric_backward: alpha and gt_mask go together (both or neither)");
    if (dL_dalpha && !alpha) return fail("sr_photometric_backward: dL_dalpha without alpha and gt_mask");
    if (w_ssim != 0.0f && !maps) return fail("sr_photometric_backward: a structural-similarity weight needs the maps of the forward");
    sr::launch_loss_backward(batch, channels, height, width, image, gt, alpha, gt_mask, w_ssim != 0.0f ? maps : nullptr, w_l1, w_ssim, w_mask,
                             upstream, upstream_per_item != 0, dL_dimage, dL_dalpha, static_cast<hipStream_t>(hip_stream));
    return check_hip(hipGetLastError(), "photometric_backward");
}

}  // extern "C"
