// The tail of the training objective: the splat regularisers and the depth L1 (DESIGN.md "Training objective").
//
// Restates reference train.py, per step, for means3D x [N,3] and the opacities o [N] (the [N,1] tensor):
//
//   :195-197  norm        = mean_i |x_i|
//   :198-201  norm_mean   = mean_i |x_i - m|,  m = mean_i x_i, detached and rounded to float32 as the reference's float32 mean is
//   :244-246  opacity_reg = mean_i (o_i - 1)^2
//   :224-229  depth_l1    = mean over ALL B H W elements of |d v - g v|,  v = (g > 0): F.l1_loss divides by every element
//
// and their gradients: x / |x| (exactly 0 for a row of length 0: torch's norm backward), 2 (o - 1) / N, sign(d - g) v / (B H W)
// with sign(0) = 0.
//
// Arithmetic.  The inputs are float32; every expression of a row or pixel is evaluated in double from them (products and
// differences of two floats are exact there), with the IEEE sqrt and `/` (no fast-math flag in build.py, no rsqrt), summed in
// double and rounded to float32 ONCE where it is stored.  The kernels stream 12-byte rows from memory; what the double
// arithmetic of a row costs beside its loads: DESIGN.md.
//
// Access.  means3D is walked as a flat array in 16-byte vectors: four rows are three vectors.  Row i starts on a 16-byte
// boundary when i = lead (mod 4), lead = ((address >> 2) & 3) of the base pointer, so the first `lead` rows and the last
// (N - lead) % 4 go element by element (workgroup 0) and a 4-byte-aligned base (a slice with a storage offset) takes the
// vector path all the same.  The opacities of a group of four rows and both gradient tensors move as one vector where their
// own address allows it and element by element where not.  The depth images are walked per item in Adam's slots (adam.hip).
//
// Sums.  Every workgroup writes its partial sums in double; one workgroup adds them in an order that the shape alone fixes.
// The centred norm needs the mean before its pass: every workgroup of that pass adds the coordinate partials itself, in the
// same order, which saves the launch a separate mean kernel would take.  Forward: 2 launches, 3 with the centred norm; depth
// L1: 2.  Backward: 1 each.  No floating-point atomics, no host wait: identical bits from call to call.
#include "host_api.h"
#include "reduce.h"

namespace sr {

namespace {

constexpr int kObjMaxBlocks = 512;       // partial sums per quantity: the second stage and the mean are sums over at most these
constexpr int kObjDepthItemBlocks = 256; // workgroups (= partial sums) per depth item at most

// float lanes between the 16-byte boundary at or below p and p
inline int obj_lead(const void* p) { return (int)((reinterpret_cast<uintptr_t>(p) >> 2) & 3u); }

// ---------------------------------------------------------------- splat regularisers ----------------------------------

enum { kSumNorm = 0, kSumX = 1, kSumY = 2, kSumZ = 3, kSumOpacity = 4, kSumCentred = 5, kSumCount = 6 };

struct RegDims {
    long long n;          // rows
    long long groups;     // groups of four rows on the vector path: rows lead .. lead + 4 groups - 1
    int lead;             // rows in front of the first group
    int tail;             // rows behind the last group: lead + tail <= 6
    int blocks;           // workgroups of a pass = partial sums per quantity
    int want_norm, want_mean, want_opacity;
    int o_vec;            // the four opacities of a group are one 16-byte vector
    int dx_vec, do_vec;   // backward: the same for the two gradient tensors
};

struct RegRow { double x, y, z; };

__device__ __forceinline__ double reg_length(const RegRow& r) { return sqrt(r.x * r.x + r.y * r.y + r.z * r.z); }

// row k (0 .. 3) of a group held as three vectors
__device__ __forceinline__ RegRow reg_row(const float (&v)[12], int k) {
    return RegRow{(double)v[3 * k], (double)v[3 * k + 1], (double)v[3 * k + 2]};
}

__device__ __forceinline__ void reg_load_group(const float* __restrict__ x, long long first_row, float (&v)[12]) {
    const float4* p = reinterpret_cast<const float4*>(x + 3 * first_row);      // 16-byte aligned: first_row = lead (mod 4)
#pragma unroll
    for (int j = 0; j < 3; ++j) {
        const float4 q = p[j];
        v[4 * j] = q.x; v[4 * j + 1] = q.y; v[4 * j + 2] = q.z; v[4 * j + 3] = q.w;
    }
}

__device__ __forceinline__ void reg_load_opacity(const float* __restrict__ o, long long first_row, bool vec, float (&v)[4]) {
    if (vec) {
        const float4 q = *reinterpret_cast<const float4*>(o + first_row);
        v[0] = q.x; v[1] = q.y; v[2] = q.z; v[3] = q.w;
    } else {
#pragma unroll
        for (int k = 0; k < 4; ++k) v[k] = o[first_row + k];
    }
}

// the row a thread of workgroup 0 takes element by element, or -1: the `lead` rows in front and the `tail` rows behind
__device__ __forceinline__ long long reg_edge_row(const RegDims& d) {
    if (blockIdx.x != 0 || (int)threadIdx.x >= d.lead + d.tail) return -1;
    const int t = (int)threadIdx.x;
    return t < d.lead ? (long long)t : (long long)d.lead + 4 * d.groups + (t - d.lead);
}

// every workgroup adds the coordinate sums of the first pass in the same order: wavefront c takes coordinate c
__device__ __forceinline__ void reg_mean(const RegDims& d, const double* __restrict__ partial, double* s_mean) {
    const int lane = threadIdx.x & (kWave - 1), wave = threadIdx.x / kWave;
    if (wave < 3) {
        double acc = 0.0;
        for (int b = lane; b < d.blocks; b += kWave) acc += partial[(size_t)(kSumX + wave) * kObjMaxBlocks + b];
        acc = wave_sum(acc);
        if (lane == 0) s_mean[wave] = (double)(float)(acc / (double)d.n);     // the reference's mean is a float32 tensor
    }
    __syncthreads();
}

// partial: [kSumCount][kObjMaxBlocks] doubles.  kCentred = false: sum |x|, sum x (three), sum (o - 1)^2, whichever are asked
// for; kCentred = true (after the first): sum |x - m|.
template <bool kCentred>
__global__ void __launch_bounds__(kBlock) k_splat_reg_partial(const RegDims d, const float* __restrict__ x, const float* __restrict__ o,
                                                              double* __restrict__ partial) {
    __shared__ double s_red[kBlock / kWave];
    __shared__ double s_mean[3];
    double m[3] = {0.0, 0.0, 0.0};
    if (kCentred) {
        reg_mean(d, partial, s_mean);
        m[0] = s_mean[0]; m[1] = s_mean[1]; m[2] = s_mean[2];
    }
    double a_len = 0.0, a_x = 0.0, a_y = 0.0, a_z = 0.0, a_o = 0.0;
    const bool rows = kCentred || d.want_norm || d.want_mean;
    const bool opacity = !kCentred && d.want_opacity;
    for (long long g = (long long)blockIdx.x * kBlock + threadIdx.x; g < d.groups; g += (long long)d.blocks * kBlock) {
        const long long first = d.lead + 4 * g;
        if (rows) {
            float v[12];
            reg_load_group(x, first, v);
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                RegRow r = reg_row(v, k);
                if (kCentred) { r.x -= m[0]; r.y -= m[1]; r.z -= m[2]; }
                if (kCentred || d.want_norm) a_len += reg_length(r);
                if (!kCentred) { a_x += r.x; a_y += r.y; a_z += r.z; }
            }
        }
        if (opacity) {
            float v[4];
            reg_load_opacity(o, first, d.o_vec != 0, v);
#pragma unroll
            for (int k = 0; k < 4; ++k) { const double e = (double)v[k] - 1.0; a_o += e * e; }
        }
    }
    const long long edge = reg_edge_row(d);
    if (edge >= 0) {
        if (rows) {
            RegRow r{(double)x[3 * edge], (double)x[3 * edge + 1], (double)x[3 * edge + 2]};
            if (kCentred) { r.x -= m[0]; r.y -= m[1]; r.z -= m[2]; }
            if (kCentred || d.want_norm) a_len += reg_length(r);
            if (!kCentred) { a_x += r.x; a_y += r.y; a_z += r.z; }
        }
        if (opacity) { const double e = (double)o[edge] - 1.0; a_o += e * e; }
    }
    if (kCentred) {
        const double s = block_sum(a_len, s_red);
        if (threadIdx.x == 0) partial[(size_t)kSumCentred * kObjMaxBlocks + blockIdx.x] = s;
        return;
    }
    const double s_len = block_sum(a_len, s_red), s_x = block_sum(a_x, s_red), s_y = block_sum(a_y, s_red);
    const double s_z = block_sum(a_z, s_red), s_o = block_sum(a_o, s_red);
    if (threadIdx.x == 0) {
        partial[(size_t)kSumNorm * kObjMaxBlocks + blockIdx.x] = s_len;
        partial[(size_t)kSumX * kObjMaxBlocks + blockIdx.x] = s_x;
        partial[(size_t)kSumY * kObjMaxBlocks + blockIdx.x] = s_y;
        partial[(size_t)kSumZ * kObjMaxBlocks + blockIdx.x] = s_z;
        partial[(size_t)kSumOpacity * kObjMaxBlocks + blockIdx.x] = s_o;
    }
}

// One workgroup: out[8] = loss | norm | norm_mean | opacity_reg | m (three) | 0.  A term that was not asked for is written as 0.
__global__ void __launch_bounds__(kBlock) k_splat_reg_final(const RegDims d, double lambda_norm, double lambda_norm_mean, double lambda_opacity,
                                                            const double* __restrict__ partial, float* __restrict__ out) {
    __shared__ double s_red[kBlock / kWave];
    __shared__ double s_mean[3];
    if (d.want_mean) reg_mean(d, partial, s_mean);        // the very sums of the centred pass: the backward gets the same mean
    double total[kSumCount] = {};
#pragma unroll
    for (int q = 0; q < kSumCount; ++q) {
        if (q >= kSumX && q <= kSumZ) continue;
        double acc = 0.0;
        const bool used = q == kSumNorm ? d.want_norm != 0 : (q == kSumOpacity ? d.want_opacity != 0 : d.want_mean != 0);
        if (used)
            for (int b = threadIdx.x; b < d.blocks; b += kBlock) acc += partial[(size_t)q * kObjMaxBlocks + b];
        total[q] = block_sum(acc, s_red);
    }
    if (threadIdx.x == 0) {
        const double n = (double)d.n;
        const double norm = total[kSumNorm] / n, centred = total[kSumCentred] / n, opacity = total[kSumOpacity] / n;
        double loss = 0.0;                      // a term that is off is not in the sum at all: 0 * NaN never appears
        if (d.want_norm) loss += lambda_norm * norm;
        if (d.want_mean) loss += lambda_norm_mean * centred;
        if (d.want_opacity) loss += lambda_opacity * opacity;
        out[0] = (float)loss;
        out[1] = d.want_norm ? (float)norm : 0.0f;
        out[2] = d.want_mean ? (float)centred : 0.0f;
        out[3] = d.want_opacity ? (float)opacity : 0.0f;
        out[4] = d.want_mean ? (float)s_mean[0] : 0.0f;
        out[5] = d.want_mean ? (float)s_mean[1] : 0.0f;
        out[6] = d.want_mean ? (float)s_mean[2] : 0.0f;
        out[7] = 0.0f;
    }
}

struct RegScale { double norm, centred, opacity; double m[3]; };   // the weights times g / N; opacity: times 2 g / N

__device__ __forceinline__ void reg_row_gradient(const RegRow& r, const RegScale& k, bool want_norm, bool want_mean, float* dst) {
    double gx = 0.0, gy = 0.0, gz = 0.0;
    if (want_norm) {
        const double len = reg_length(r);
        const double c = len > 0.0 ? k.norm / len : 0.0;                  // a row of length 0 contributes exactly 0
        gx = c * r.x; gy = c * r.y; gz = c * r.z;
    }
    if (want_mean) {
        const RegRow e{r.x - k.m[0], r.y - k.m[1], r.z - k.m[2]};
        const double len = reg_length(e);
        const double c = len > 0.0 ? k.centred / len : 0.0;
        gx += c * e.x; gy += c * e.y; gz += c * e.z;
    }
    dst[0] = (float)gx; dst[1] = (float)gy; dst[2] = (float)gz;
}

// dx [N,3] (may be NULL) and d_o [N] (may be NULL), with g = *upstream and the mean of the forward in out[4..6]
__global__ void __launch_bounds__(kBlock) k_splat_reg_backward(const RegDims d, double lambda_norm, double lambda_norm_mean,
                                                               double lambda_opacity, const float* __restrict__ x,
                                                               const float* __restrict__ o, const float* __restrict__ out,
                                                               const float* __restrict__ upstream, float* __restrict__ dx,
                                                               float* __restrict__ d_o) {
    const double g_n = (double)upstream[0] / (double)d.n;
    RegScale k;
    k.norm = g_n * lambda_norm; k.centred = g_n * lambda_norm_mean; k.opacity = 2.0 * g_n * lambda_opacity;
    k.m[0] = d.want_mean ? (double)out[4] : 0.0; k.m[1] = d.want_mean ? (double)out[5] : 0.0; k.m[2] = d.want_mean ? (double)out[6] : 0.0;
    const bool want_norm = d.want_norm != 0, want_mean = d.want_mean != 0;
    for (long long g = (long long)blockIdx.x * kBlock + threadIdx.x; g < d.groups; g += (long long)d.blocks * kBlock) {
        const long long first = d.lead + 4 * g;
        if (dx) {
            float v[12], r[12];
            reg_load_group(x, first, v);
#pragma unroll
            for (int j = 0; j < 4; ++j) reg_row_gradient(reg_row(v, j), k, want_norm, want_mean, r + 3 * j);
            if (d.dx_vec) {
                float4* p = reinterpret_cast<float4*>(dx + 3 * first);
#pragma unroll
                for (int j = 0; j < 3; ++j) p[j] = make_float4(r[4 * j], r[4 * j + 1], r[4 * j + 2], r[4 * j + 3]);
            } else {
#pragma unroll
                for (int j = 0; j < 12; ++j) dx[3 * first + j] = r[j];
            }
        }
        if (d_o) {
            float v[4], r[4];
            reg_load_opacity(o, first, d.o_vec != 0, v);
#pragma unroll
            for (int j = 0; j < 4; ++j) r[j] = (float)(k.opacity * ((double)v[j] - 1.0));
            if (d.do_vec) {
                *reinterpret_cast<float4*>(d_o + first) = make_float4(r[0], r[1], r[2], r[3]);
            } else {
#pragma unroll
                for (int j = 0; j < 4; ++j) d_o[first + j] = r[j];
            }
        }
    }
    const long long edge = reg_edge_row(d);
    if (edge >= 0) {
        if (dx) {
            const RegRow r{(double)x[3 * edge], (double)x[3 * edge + 1], (double)x[3 * edge + 2]};
            reg_row_gradient(r, k, want_norm, want_mean, dx + 3 * edge);
        }
        if (d_o) d_o[edge] = (float)(k.opacity * ((double)o[edge] - 1.0));
    }
}

// The split of n rows.  `rows`: means3D is walked and sets the 16-byte phase of the groups; else the opacities alone do.
RegDims reg_dims(long long n, bool rows, const float* x, const float* o, bool want_norm, bool want_mean, bool want_opacity) {
    RegDims d = {};
    d.n = n;
    d.want_norm = want_norm; d.want_mean = want_mean; d.want_opacity = want_opacity;
    // row i of x starts at byte 12 i past the base: on a 16-byte boundary when i = lead(x) (mod 4); element i of o when
    // i = -lead(o) (mod 4)
    long long lead = rows ? obj_lead(x) : (4 - obj_lead(o)) & 3;
    if (lead > n) lead = n;
    d.lead = (int)lead;
    d.groups = (n - lead) / 4;
    d.tail = (int)(n - lead - 4 * d.groups);
    d.o_vec = o != nullptr && ((obj_lead(o) + d.lead) & 3) == 0;
    const long long blocks = (d.groups + kBlock - 1) / kBlock;
    d.blocks = (int)(blocks < 1 ? 1 : (blocks > kObjMaxBlocks ? kObjMaxBlocks : blocks));
    return d;
}

// ---------------------------------------------------------------- depth L1 --------------------------------------------

struct DepthDims {
    int batch;
    long long pixels;       // H W of one item
    int item_blocks;        // workgroups (= partial sums) per item
    int in_vec;             // depth and gt agree modulo 16: slots inside an item load as 16-byte vectors
    int out_vec;            // backward: the gradient agrees with them too
};

__device__ __forceinline__ double depth_term(float dv, float gv) { return gv > 0.0f ? fabs((double)dv - (double)gv) : 0.0; }

__device__ __forceinline__ float depth_gradient(float dv, float gv, float scale) {
    if (!(gv > 0.0f)) return 0.0f;
    return dv > gv ? scale : (dv < gv ? -scale : 0.0f);
}

// partial [batch][item_blocks] doubles: sum over the slots of the workgroup of |d v - g v|.  An item's elements are laid over
// slots of four floats from the 16-byte boundary at or below its first element (adam.hip): element e is virtual element lead + e.
__global__ void __launch_bounds__(kBlock) k_depth_l1_partial(const DepthDims d, const float* __restrict__ depth, const float* __restrict__ gt,
                                                             double* __restrict__ partial) {
    __shared__ double s_red[kBlock / kWave];
    const int item = blockIdx.x / d.item_blocks, k = blockIdx.x - item * d.item_blocks;
    const float* pd = depth + (size_t)item * d.pixels;
    const float* pg = gt + (size_t)item * d.pixels;
    const long long lead = d.in_vec ? (long long)((reinterpret_cast<uintptr_t>(pd) >> 2) & 3u) : 0;
    const long long end = lead + d.pixels, slots = (end + 3) / 4;
    pd -= lead; pg -= lead;            // only dereferenced at virtual elements lead .. end - 1
    double acc = 0.0;
    for (long long s = (long long)k * kBlock + threadIdx.x; s < slots; s += (long long)d.item_blocks * kBlock) {
        const long long e = 4 * s;
        if (d.in_vec && e >= lead && e + 4 <= end) {
            const float4 a = *reinterpret_cast<const float4*>(pd + e), b = *reinterpret_cast<const float4*>(pg + e);
            acc += depth_term(a.x, b.x) + depth_term(a.y, b.y) + depth_term(a.z, b.z) + depth_term(a.w, b.w);
        } else {
            for (long long i = e; i < e + 4; ++i)
                if (i >= lead && i < end) acc += depth_term(pd[i], pg[i]);
        }
    }
    const double s = block_sum(acc, s_red);
    if (threadIdx.x == 0) partial[blockIdx.x] = s;
}

// One workgroup: out[0] = the mean over everything, out[1 + b] = the mean over item b.
__global__ void __launch_bounds__(kBlock) k_depth_l1_final(const DepthDims d, const double* __restrict__ partial, float* __restrict__ out) {
    __shared__ double s_red[kBlock / kWave];
    const int lane = threadIdx.x & (kWave - 1), wave = threadIdx.x / kWave;
    for (int b = wave; b < d.batch; b += kBlock / kWave) {
        double acc = 0.0;
        for (int k = lane; k < d.item_blocks; k += kWave) acc += partial[(size_t)b * d.item_blocks + k];
        acc = wave_sum(acc);
        if (lane == 0) out[1 + b] = (float)(acc / (double)d.pixels);
    }
    double acc = 0.0;
    const long long count = (long long)d.batch * d.item_blocks;
    for (long long i = threadIdx.x; i < count; i += kBlock) acc += partial[i];
    const double total = block_sum(acc, s_red);
    if (threadIdx.x == 0) out[0] = (float)(total / ((double)d.batch * (double)d.pixels));
}

__global__ void __launch_bounds__(kBlock) k_depth_l1_backward(const DepthDims d, const float* __restrict__ depth, const float* __restrict__ gt,
                                                              const float* __restrict__ upstream, int per_item, float* __restrict__ grad) {
    const int item = blockIdx.x / d.item_blocks, k = blockIdx.x - item * d.item_blocks;
    const float* pd = depth + (size_t)item * d.pixels;
    const float* pg = gt + (size_t)item * d.pixels;
    float* po = grad + (size_t)item * d.pixels;
    const long long lead = d.in_vec ? (long long)((reinterpret_cast<uintptr_t>(pd) >> 2) & 3u) : 0;
    const long long end = lead + d.pixels, slots = (end + 3) / 4;
    pd -= lead; pg -= lead; po -= lead;
    const double divisor = per_item ? (double)d.pixels : (double)d.batch * (double)d.pixels;
    const float scale = (float)((double)upstream[per_item ? item : 0] / divisor);
    for (long long s = (long long)k * kBlock + threadIdx.x; s < slots; s += (long long)d.item_blocks * kBlock) {
        const long long e = 4 * s;
        if (d.in_vec && e >= lead && e + 4 <= end) {
            const float4 a = *reinterpret_cast<const float4*>(pd + e), b = *reinterpret_cast<const float4*>(pg + e);
            const float4 r = make_float4(depth_gradient(a.x, b.x, scale), depth_gradient(a.y, b.y, scale),
                                         depth_gradient(a.z, b.z, scale), depth_gradient(a.w, b.w, scale));
            if (d.out_vec) {
                *reinterpret_cast<float4*>(po + e) = r;
            } else {
                po[e] = r.x; po[e + 1] = r.y; po[e + 2] = r.z; po[e + 3] = r.w;
            }
        } else {
            for (long long i = e; i < e + 4; ++i)
                if (i >= lead && i < end) po[i] = depth_gradient(pd[i], pg[i], scale);
        }
    }
}

DepthDims depth_dims(int batch, int H, int W, const float* depth, const float* gt, const float* grad) {
    DepthDims d = {};
    d.batch = batch;
    d.pixels = (long long)H * W;
    const long long blocks = (d.pixels / 4 + 1 + kBlock - 1) / kBlock;        // slots of an item, at most
    d.item_blocks = (int)(blocks > kObjDepthItemBlocks ? kObjDepthItemBlocks : blocks);
    // the items of one tensor are `pixels` floats apart: two tensors that agree modulo 16 at item 0 agree at every item
    d.in_vec = obj_lead(depth) == obj_lead(gt);
    d.out_vec = grad != nullptr && d.in_vec && obj_lead(grad) == obj_lead(depth);
    return d;
}

size_t splat_reg_workspace_bytes(long long n) {
    return n > 0 ? align_up(sizeof(double) * kSumCount * kObjMaxBlocks, 256) : 0;
}

void launch_splat_reg_forward(long long n, const float* means3D, const float* opacity, double lambda_norm, double lambda_norm_mean,
                              double lambda_opacity, void* workspace, float* out, hipStream_t st) {
    const RegDims d = reg_dims(n, lambda_norm != 0.0 || lambda_norm_mean != 0.0, means3D, opacity, lambda_norm != 0.0, lambda_norm_mean != 0.0, lambda_opacity != 0.0);
    double* partial = static_cast<double*>(workspace);
    if (d.want_norm || d.want_mean || d.want_opacity)
        hipLaunchKernelGGL(k_splat_reg_partial<false>, dim3(d.blocks), dim3(kBlock), 0, st, d, means3D, opacity, partial);
    if (d.want_mean) hipLaunchKernelGGL(k_splat_reg_partial<true>, dim3(d.blocks), dim3(kBlock), 0, st, d, means3D, opacity, partial);
    hipLaunchKernelGGL(k_splat_reg_final, dim3(1), dim3(kBlock), 0, st, d, lambda_norm, lambda_norm_mean, lambda_opacity, partial, out);
}

void launch_splat_reg_backward(long long n, const float* means3D, const float* opacity, double lambda_norm, double lambda_norm_mean,
                               double lambda_opacity, const float* out, const float* upstream, float* d_means3D, float* d_opacity,
                               hipStream_t st) {
    // the rows set the phase whenever their gradient is written, as in the forward
    const bool rows = d_means3D != nullptr;
    RegDims d = reg_dims(n, rows, means3D, opacity, rows && lambda_norm != 0.0, rows && lambda_norm_mean != 0.0,
                         d_opacity != nullptr);
    d.dx_vec = rows && obj_lead(d_means3D) == obj_lead(means3D);
    d.do_vec = d_opacity != nullptr && ((obj_lead(d_opacity) + d.lead) & 3) == 0;
    hipLaunchKernelGGL(k_splat_reg_backward, dim3(d.blocks), dim3(kBlock), 0, st, d, lambda_norm, lambda_norm_mean, lambda_opacity, means3D,
                       opacity, out, upstream, d_means3D, d_opacity);
}

bool depth_l1_shape_ok(int batch, int H, int W) {
    return batch >= 0 && H > 0 && W > 0 && (long long)batch * kObjDepthItemBlocks <= 0x7fffffffll / kBlock;
}

size_t depth_l1_workspace_bytes(int batch, int H, int W) {
    if (!depth_l1_shape_ok(batch, H, W) || batch == 0) return 0;
    return align_up(sizeof(double) * (size_t)batch * kObjDepthItemBlocks, 256);
}

void launch_depth_l1_forward(int batch, int H, int W, const float* depth, const float* gt, void* workspace, float* out, hipStream_t st) {
    const DepthDims d = depth_dims(batch, H, W, depth, gt, nullptr);
    double* partial = static_cast<double*>(workspace);
    hipLaunchKernelGGL(k_depth_l1_partial, dim3((unsigned)batch * d.item_blocks), dim3(kBlock), 0, st, d, depth, gt, partial);
    hipLaunchKernelGGL(k_depth_l1_final, dim3(1), dim3(kBlock), 0, st, d, partial, out);
}

void launch_depth_l1_backward(int batch, int H, int W, const float* depth, const float* gt, const float* upstream, bool per_item,
                              float* grad, hipStream_t st) {
    const DepthDims d = depth_dims(batch, H, W, depth, gt, grad);
    hipLaunchKernelGGL(k_depth_l1_backward, dim3((unsigned)batch * d.item_blocks), dim3(kBlock), 0, st, d, depth, gt, upstream,
                       per_item ? 1 : 0, grad);
}

}  // namespace

}  // namespace sr

// ---- C entry points (include/splatraster.h): what is refused on the host, then the launchers above --------------------
using sr::fail; using sr::check_hip; using sr::any_unaligned4;

extern "C" {

size_t sr_splat_reg_workspace_bytes(int n_splats) { return sr::splat_reg_workspace_bytes(n_splats); }

int sr_splat_reg_forward(int n_splats, const float* means3D, const float* opacity, double lambda_norm, double lambda_norm_mean,
                         double lambda_opacity, void* workspace, float* out, void* hip_stream) {
    if (n_splats < 0) return fail("bad arguments to sr_splat_reg_forward: negative splat count");
    if (!(lambda_norm == lambda_norm) || !(lambda_norm_mean == lambda_norm_mean) || !(lambda_opacity == lambda_opacity))
        return fail("bad arguments to sr_splat_reg_forward: a weight is NaN");
    if (n_splats == 0) return 0;
    if (!workspace || !out) return fail("null pointer in sr_splat_reg_forward");
    if ((lambda_norm != 0.0 || lambda_norm_mean != 0.0) && !means3D) return fail("null pointer in sr_splat_reg_forward: means3D is read by the norm terms");
    if (lambda_opacity != 0.0 && !opacity) return fail("null pointer in sr_splat_reg_forward: opacity is read by the opacity term");
    if (any_unaligned4(means3D, opacity)) return fail("sr_splat_reg_forward: tensors must be 4-byte aligned");
    sr::launch_splat_reg_forward(n_splats, means3D, opacity, lambda_norm, lambda_norm_mean, lambda_opacity, workspace, out,
                                 static_cast<hipStream_t>(hip_stream));
    return check_hip(hipGetLastError(), "splat_reg_forward");
}

int sr_splat_reg_backward(int n_splats, const float* means3D, const float* opacity, double lambda_norm, double lambda_norm_mean,
                          double lambda_opacity, const float* out, const float* upstream, float* dL_dmeans3D, float* dL_dopacity,
                          void* hip_stream) {
    if (n_splats < 0) return fail("bad arguments to sr_splat_reg_backward: negative splat count");
    if (!(lambda_norm == lambda_norm) || !(lambda_norm_mean == lambda_norm_mean) || !(lambda_opacity == lambda_opacity))
        return fail("bad arguments to sr_splat_reg_backward: a weight is NaN");
    if (n_splats == 0 || (!dL_dmeans3D && !dL_dopacity)) return 0;
    if (!upstream) return fail("null pointer in sr_splat_reg_backward");
    if (dL_dmeans3D && !means3D) return fail("null pointer in sr_splat_reg_backward: dL_dmeans3D without means3D");
    if (dL_dopacity && !opacity) return fail("null pointer in sr_splat_reg_backward: dL_dopacity without opacity");
    if (dL_dmeans3D && lambda_norm_mean != 0.0 && !out) return fail("null pointer in sr_splat_reg_backward: the centred norm needs the mean in `out` of the forward");
    if (any_unaligned4(means3D, opacity, dL_dmeans3D, dL_dopacity)) return fail("sr_splat_reg_backward: tensors must be 4-byte aligned");
    sr::launch_splat_reg_backward(n_splats, means3D, opacity, lambda_norm, lambda_norm_mean, lambda_opacity, out, upstream, dL_dmeans3D,
                                  dL_dopacity, static_cast<hipStream_t>(hip_stream));
    return check_hip(hipGetLastError(), "splat_reg_backward");
}

size_t sr_depth_l1_workspace_bytes(int batch, int height, int width) { return sr::depth_l1_workspace_bytes(batch, height, width); }

int sr_depth_l1_forward(int batch, int height, int width, const float* depth, const float* gt_depth, void* workspace, float* out,
                        void* hip_stream) {
    if (batch < 0 || height <= 0 || width <= 0) return fail("bad arguments to sr_depth_l1_forward: the image size must be positive and the batch not negative");
    if (!sr::depth_l1_shape_ok(batch, height, width)) return fail("too many items for sr_depth_l1_forward");
    if (batch == 0) return 0;
    if (!depth || !gt_depth || !workspace || !out) return fail("null pointer in sr_depth_l1_forward");
    if (any_unaligned4(depth, gt_depth)) return fail("sr_depth_l1_forward: tensors must be 4-byte aligned");
    sr::launch_depth_l1_forward(batch, height, width, depth, gt_depth, workspace, out, static_cast<hipStream_t>(hip_stream));
    return check_hip(hipGetLastError(), "depth_l1_forward");
}

int sr_depth_l1_backward(int batch, int height, int width, const float* depth, const float* gt_depth, const float* upstream,
                         int upstream_per_item, float* dL_ddepth, void* hip_stream) {
    if (batch < 0 || height <= 0 || width <= 0) return fail("bad arguments to sr_depth_l1_backward: the image size must be positive and the batch not negative");
    if (!sr::depth_l1_shape_ok(batch, height, width)) return fail("too many items for sr_depth_l1_backward");
    if (batch == 0) return 0;
    if (!depth || !gt_depth || !upstream || !dL_ddepth) return fail("null pointer in sr_depth_l1_backward");
    if (any_unaligned4(depth, gt_depth, dL_ddepth)) return fail("sr_depth_l1_backward: tensors must be 4-byte aligned");
    sr::launch_depth_l1_backward(batch, height, width, depth, gt_depth, upstream, upstream_per_item != 0, dL_ddepth,
                                 static_cast<hipStream_t>(hip_stream));
    return check_hip(hipGetLastError(), "depth_l1_backward");
}

}  // extern "C"
