// Depth-map initialisation on the device: the back-projection in front of the visual hull (hull.hip's sibling).
//
// Restates `_gen_3dpoints` of reference scene/dataset_readers.py:1476-1491, which `readCamerasFromNeus` (:1376) and
// `readCamerasFromResFields` (:1463) call once per camera and frame, and what `readNeuSceneInfo` takes from the concatenated cloud:
// its two bounds (:1603-1613, the box of the hull) or `num_pts` random rows (:1653-1658, the `depth` branch).  For image b of a
// batch [B,H,W] and the pixel (x, y) -- integer coordinates, no half-pixel offset --
//
//   p = Kinv[b] (x, y, 1),  v = p / |p|,  v' = R[b] v,  point = o[b] + depth[b,y,x] v'          (pose[b] = [R | o], 3x4)
//
// and the pixel is kept iff depth > 0 (0, negatives and NaN are dropped, +inf is kept) and its mask byte, if a mask is given, is
// non-zero.  Rows follow the pixels in row-major (y, x) order, image after image.  Here:
//
//   mark     one lane per pixel: the wavefront's survivors become one 64-bit word (__ballot), the workgroup's count one uint32,
//            the smallest and largest float32 coordinate of its survivors two floats;
//   scan     one workgroup turns the counts into exclusive offsets in index order, writes the total and reduces the bounds;
//   gather   every survivor's rank = its workgroup's offset + the bits in front of it: points, colours and pixel indices are written
//            in that order up to a capacity -- or
//   select   row j = survivor number ranks[j], found by bisection over the offsets, the four words' popcounts and the bit inside
//            the word: a sample of the cloud without the cloud.
//
// Points are recomputed where they are written, never stored by the mark pass.  No atomics anywhere: the same inputs give the same
// bytes from call to call.
//
// Arithmetic: double, in the order written above (every three-term dot product left to right, sqrt of the sum of squares, one
// division per component), with floating-point contraction switched off, rounded to float32 once.
//
// Bounds and NaN: a coordinate can be NaN only when the depth is +inf (inf * 0, or inf - inf against the origin).  Such a row is
// kept and written as it is, but a NaN coordinate takes no part in the bounds (an infinite one does): the bounds are the minimum
// and maximum over the non-NaN coordinates of the survivors, (+inf, -inf) when there are none.
#include "host_api.h"
#include "ordered_scan.h"

namespace sr {

namespace {

struct DepthItems {
    const SrDepthCamera* cams;   // [B], device
    const void* depths;          // [B,H,W] float32 / float64
    int depth_is_double;
    unsigned H, W, HW;
    long long n;                 // B H W <= 2^31 - 1
};

__device__ __forceinline__ double depth_of(const DepthItems& it, long long i) {
    return it.depth_is_double ? static_cast<const double*>(it.depths)[i] : (double)static_cast<const float*>(it.depths)[i];
}

// the point of pixel i with depth d, rounded once
__device__ __forceinline__ void depth_point(const DepthItems& it, long long i, double d, float& X, float& Y, float& Z) {
#pragma clang fp contract(off)
    const unsigned b = (unsigned)i / it.HW, r = (unsigned)i % it.HW;
    const double x = (double)(r % it.W), y = (double)(r / it.W);
    const SrDepthCamera& c = it.cams[b];                 // the same record for (nearly) every lane of a wavefront
    const double p0 = c.kinv[0] * x + c.kinv[1] * y + c.kinv[2] * 1.0;
    const double p1 = c.kinv[3] * x + c.kinv[4] * y + c.kinv[5] * 1.0;
    const double p2 = c.kinv[6] * x + c.kinv[7] * y + c.kinv[8] * 1.0;
    const double len = sqrt(p0 * p0 + p1 * p1 + p2 * p2);
    const double v0 = p0 / len, v1 = p1 / len, v2 = p2 / len;
    const double w0 = c.pose[0] * v0 + c.pose[1] * v1 + c.pose[2] * v2;
    const double w1 = c.pose[4] * v0 + c.pose[5] * v1 + c.pose[6] * v2;
    const double w2 = c.pose[8] * v0 + c.pose[9] * v1 + c.pose[10] * v2;
    X = (float)(c.pose[3] + d * w0);
    Y = (float)(c.pose[7] + d * w1);
    Z = (float)(c.pose[11] + d * w2);
}

__device__ __forceinline__ float wave_min(float v) {
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) { const float o = __shfl_xor(v, d, 64); v = o < v ? o : v; }
    return v;
}
__device__ __forceinline__ float wave_max(float v) {
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) { const float o = __shfl_xor(v, d, 64); v = o > v ? o : v; }
    return v;
}

__global__ void __launch_bounds__(kBlock) k_depth_mark(const DepthItems it, const uint8_t* __restrict__ masks,
                                                       unsigned long long* __restrict__ words, uint32_t* __restrict__ block_counts,
                                                       float* __restrict__ block_lo, float* __restrict__ block_hi) {
    __shared__ float s_lo[kBlock / kWave], s_hi[kBlock / kWave];
    const long long i = (long long)blockIdx.x * kBlock + threadIdx.x;
    bool alive = false;
    float lo = __builtin_inff(), hi = -__builtin_inff();
    if (i < it.n) {
        const double d = depth_of(it, i);
        alive = d > 0.0 && (!masks || masks[i] != 0);     // NaN fails the comparison
        if (alive) {
            float c[3];
            depth_point(it, i, d, c[0], c[1], c[2]);
#pragma unroll
            for (int a = 0; a < 3; ++a)
                if (c[a] == c[a]) { lo = c[a] < lo ? c[a] : lo; hi = c[a] > hi ? c[a] : hi; }   // a NaN coordinate is skipped
        }
    }
    lo = wave_min(lo); hi = wave_max(hi);
    if (lane_id() == 0) { s_lo[wave_id()] = lo; s_hi[wave_id()] = hi; }
    compaction_mark(alive, i, words, block_counts);      // every lane of the workgroup arrives here: lanes past n vote 0
    if (threadIdx.x == 0) {                               // behind the barrier of compaction_mark
        float l = s_lo[0], h = s_hi[0];
#pragma unroll
        for (int w = 1; w < kBlock / kWave; ++w) { l = s_lo[w] < l ? s_lo[w] : l; h = s_hi[w] > h ? s_hi[w] : h; }
        block_lo[blockIdx.x] = l; block_hi[blockIdx.x] = h;
    }
}

// counts -> exclusive offsets and the total (ordered_scan.h), then the workgroups' bounds -> the two bounds
__global__ void __launch_bounds__(kScanBlock) k_depth_scan(long long blocks, uint32_t* __restrict__ block_counts,
                                                           const float* __restrict__ block_lo, const float* __restrict__ block_hi,
                                                           uint32_t* __restrict__ total, int* __restrict__ count_out,
                                                           float* __restrict__ bounds_out) {
    __shared__ float s_lo[kScanBlock / kWave], s_hi[kScanBlock / kWave];
    const uint32_t carry = ordered_scan(blocks, [&](long long j) { return block_counts[j]; },
                                        [&](long long j, uint32_t offset) { block_counts[j] = offset; });
    float lo = __builtin_inff(), hi = -__builtin_inff();
    for (long long j = threadIdx.x; j < blocks; j += kScanBlock) {
        const float l = block_lo[j], h = block_hi[j];
        lo = l < lo ? l : lo; hi = h > hi ? h : hi;
    }
    lo = wave_min(lo); hi = wave_max(hi);
    if (lane_id() == 0) { s_lo[wave_id()] = lo; s_hi[wave_id()] = hi; }
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int w = 1; w < kScanBlock / kWave; ++w) { lo = s_lo[w] < lo ? s_lo[w] : lo; hi = s_hi[w] > hi ? s_hi[w] : hi; }
        *total = carry;
        if (count_out) *count_out = (int)carry;
        if (bounds_out) { bounds_out[0] = lo; bounds_out[1] = hi; }
    }
}

// what a row receives; any of the three may be NULL
struct DepthRows {
    float* points;               // [rows, 3]
    void* colors;                // [rows, 3] elements of color_bytes bytes
    long long* indices;          // [rows] b H W + y W + x
    const void* images;          // [B,H,W,3] elements of color_bytes bytes
    int color_bytes;             // 1, 4 or 8
};

template <typename T>
__device__ __forceinline__ void copy3(void* dst, const void* src, long long row, long long i) {
    T* d = static_cast<T*>(dst) + 3 * row;
    const T* s = static_cast<const T*>(src) + 3 * i;
    d[0] = s[0]; d[1] = s[1]; d[2] = s[2];
}

__device__ __forceinline__ void depth_write_row(const DepthItems& it, const DepthRows& out, long long row, long long i) {
    if (out.points) {
        float X, Y, Z;
        depth_point(it, i, depth_of(it, i), X, Y, Z);
        out.points[3 * row + 0] = X; out.points[3 * row + 1] = Y; out.points[3 * row + 2] = Z;
    }
    if (out.colors) {
        if (out.color_bytes == 1) copy3<uint8_t>(out.colors, out.images, row, i);
        else if (out.color_bytes == 4) copy3<uint32_t>(out.colors, out.images, row, i);
        else copy3<unsigned long long>(out.colors, out.images, row, i);
    }
    if (out.indices) out.indices[row] = i;
}

__global__ void __launch_bounds__(kBlock) k_depth_gather(const DepthItems it, const unsigned long long* __restrict__ words,
                                                         const uint32_t* __restrict__ block_offsets, long long capacity,
                                                         const DepthRows out) {
    const long long i = (long long)blockIdx.x * kBlock + threadIdx.x;
    if (i >= it.n) return;
    long long rank;
    if (!compaction_rank(words, block_offsets, rank) || rank >= capacity) return;            // dropped, or past an ordered prefix when the caller's buffers are short
    depth_write_row(it, out, rank, i);
}

// row j = survivor number ranks[j].  A rank outside [0, total) gives a row of NaN coordinates, zero colour bytes and the index -1,
// and sets *flag to 1 (every offending lane stores the same word: no atomic is needed); nothing else is read for it
__global__ void __launch_bounds__(kBlock) k_depth_select(const DepthItems it, long long blocks, const unsigned long long* __restrict__ words,
                                                         const uint32_t* __restrict__ block_offsets, const uint32_t* __restrict__ total,
                                                         const long long* __restrict__ ranks, long long n_ranks, const DepthRows out,
                                                         int* __restrict__ flag) {
    const long long j = (long long)blockIdx.x * kBlock + threadIdx.x;
    if (j >= n_ranks) return;
    const long long r = ranks[j];
    long long i = -1;
    if (r >= 0 && r < (long long)*total) {
        long long a = 0, b = blocks - 1;                  // the last workgroup whose offset is <= r: empty ones in front of it share it
        while (a < b) {
            const long long mid = (a + b + 1) >> 1;
            if ((long long)block_offsets[mid] <= r) a = mid; else b = mid - 1;
        }
        int k = (int)(r - (long long)block_offsets[a]);   // survivors of workgroup `a` in front of the one we want
        unsigned long long word = 0ull;
        int w = 0;
        for (; w < kBlock / kWave; ++w) {
            word = words[a * (kBlock / kWave) + w];
            const int c = __popcll(word);
            if (k < c) break;
            k -= c;
        }
        if (w < kBlock / kWave) {
            int pos = 0;                                  // the bit with k set bits below it, by halving
#pragma unroll
            for (int s = 32; s > 0; s >>= 1) {
                const int c = __popcll(word & (((1ull << s) - 1ull) << pos));
                if (k >= c) { k -= c; pos += s; }
            }
            i = a * kBlock + w * kWave + pos;
        }
        if (i >= it.n) i = -1;                            // a workspace that no mark pass of these items wrote
    }
    if (i >= 0) { depth_write_row(it, out, j, i); return; }
    *flag = 1;
    if (out.points) { const float q = __builtin_nanf(""); out.points[3 * j + 0] = q; out.points[3 * j + 1] = q; out.points[3 * j + 2] = q; }
    if (out.colors) {
        uint8_t* d = static_cast<uint8_t*>(out.colors) + 3ll * out.color_bytes * j;
        for (int k = 0; k < 3 * out.color_bytes; ++k) d[k] = 0;
    }
    if (out.indices) out.indices[j] = -1;
}

struct DepthCarve { unsigned long long* words; uint32_t* counts; float* lo; float* hi; uint32_t* total; };

// survivor words [4 per workgroup] | workgroup counts / offsets | workgroup minima | workgroup maxima | total
size_t carve_depth(void* base, long long n, DepthCarve* out) {
    Carver c{static_cast<char*>(base), 0};
    const size_t blocks = (size_t)(((n > 0 ? n : 1) + kBlock - 1) / kBlock);
    DepthCarve t;
    t.words = c.take<unsigned long long>(blocks * (kBlock / kWave));
    t.counts = c.take<uint32_t>(blocks);
    t.lo = c.take<float>(blocks);
    t.hi = c.take<float>(blocks);
    t.total = c.take<uint32_t>(1);
    if (out) *out = t;
    return align_up(c.off, 256);
}

DepthItems depth_items(int B, int H, int W, const SrDepthCamera* cams, const void* depths, int depth_is_double) {
    return DepthItems{cams, depths, depth_is_double, (unsigned)H, (unsigned)W, (unsigned)H * (unsigned)W, (long long)B * H * W};
}

void launch_depth_mark(const DepthItems& it, const uint8_t* masks, void* workspace, int* count_out, float* bounds_out, hipStream_t st) {
    DepthCarve c;
    carve_depth(workspace, it.n, &c);
    const long long blocks = (it.n + kBlock - 1) / kBlock;
    { StageTimer t_(0, st); hipLaunchKernelGGL(k_depth_mark, dim3((unsigned)blocks), dim3(kBlock), 0, st, it, masks, c.words, c.counts, c.lo, c.hi); }
    { StageTimer t_(0, st); hipLaunchKernelGGL(k_depth_scan, dim3(1), dim3(kScanBlock), 0, st, blocks, c.counts, c.lo, c.hi, c.total, count_out, bounds_out); }
}

void launch_depth_gather(const DepthItems& it, const void* workspace, long long capacity, const DepthRows& out, hipStream_t st) {
    DepthCarve c;
    carve_depth(const_cast<void*>(workspace), it.n, &c);
    const long long blocks = (it.n + kBlock - 1) / kBlock;
    StageTimer t_(0, st);
    hipLaunchKernelGGL(k_depth_gather, dim3((unsigned)blocks), dim3(kBlock), 0, st, it, c.words, c.counts, capacity, out);
}

void launch_depth_select(const DepthItems& it, const void* workspace, const long long* ranks, long long n_ranks, const DepthRows& out,
                         int* flag, hipStream_t st) {
    DepthCarve c;
    carve_depth(const_cast<void*>(workspace), it.n, &c);
    const long long blocks = (it.n + kBlock - 1) / kBlock;
    StageTimer t_(0, st);
    hipLaunchKernelGGL(k_depth_select, dim3((unsigned)((n_ranks + kBlock - 1) / kBlock)), dim3(kBlock), 0, st, it, blocks, c.words, c.counts,
                       c.total, ranks, n_ranks, out, flag);
}

}  // namespace

}  // namespace sr

// ---- C entry points (include/splatraster.h): what is refused on the host, then the launchers above --------------------
using sr::fail; using sr::check_hip;

extern "C" {

static const long long kDepthMaxItems = 2147483647LL;

// items of a call: B H W; -1 with the message set when the batch is not acceptable
static long long depth_batch(const char* name, int B, int H, int W, const void* cams, const void* depths, int depth_is_double) {
    if (B < 0) { fail(std::string(name) + ": B must not be negative"); return -1; }
    if (H < 1 || W < 1) { fail(std::string(name) + ": H and W must be at least 1"); return -1; }
    if ((long long)H * W > kDepthMaxItems || (long long)B * ((long long)H * W) > kDepthMaxItems) {
        fail(std::string(name) + ": B H W must not exceed 2^31 - 1");
        return -1;
    }
    if (depth_is_double != 0 && depth_is_double != 1) { fail(std::string(name) + ": depth_is_double must be 0 (float32) or 1 (float64)"); return -1; }
    if (B > 0 && (!cams || !depths)) { fail(std::string("null pointer in ") + name); return -1; }
    if ((reinterpret_cast<uintptr_t>(cams) & 7u) || (reinterpret_cast<uintptr_t>(depths) & (depth_is_double ? 7u : 3u))) {
        fail(std::string(name) + ": cameras must be 8-byte aligned and depths aligned to their element");
        return -1;
    }
    return (long long)B * H * W;
}

// the outputs of a gather or select call: 1 with the message set when they are not acceptable
static int depth_rows(const char* name, const void* images, int color_bytes, float* points_out, void* colors_out, long long* indices_out,
                      sr::DepthRows* rows) {
    if (colors_out) {
        if (color_bytes != 1 && color_bytes != 4 && color_bytes != 8) return fail(std::string(name) + ": color_bytes must be 1, 4 or 8");
        if (!images) return fail(std::string("null pointer in ") + name + ": colors_out needs images");
        const uintptr_t m = (uintptr_t)color_bytes - 1u;
        if ((reinterpret_cast<uintptr_t>(images) & m) || (reinterpret_cast<uintptr_t>(colors_out) & m))
            return fail(std::string(name) + ": images and colors_out must be aligned to color_bytes");
    }
    if ((reinterpret_cast<uintptr_t>(points_out) & 3u) || (reinterpret_cast<uintptr_t>(indices_out) & 7u))
        return fail(std::string(name) + ": points_out must be 4-byte and indices_out 8-byte aligned");
    *rows = sr::DepthRows{points_out, colors_out, indices_out, images, color_bytes};
    return 0;
}

size_t sr_depth_points_workspace_bytes(long long n_items) {
    return n_items < 0 || n_items > kDepthMaxItems ? 0 : sr::carve_depth(nullptr, n_items, nullptr);
}

int sr_depth_points_mark(int B, int H, int W, const SrDepthCamera* cameras, const void* depths, int depth_is_double, const unsigned char* masks,
                         void* workspace, int* count_out, float* bounds_out, void* hip_stream) {
    const long long n = depth_batch("sr_depth_points_mark", B, H, W, cameras, depths, depth_is_double);
    if (n < 0) return 1;
    if (!workspace || (!count_out && !bounds_out)) return fail("null pointer in sr_depth_points_mark");
    if ((reinterpret_cast<uintptr_t>(workspace) & 7u) || sr::any_unaligned4(count_out, bounds_out))
        return fail("sr_depth_points_mark: the workspace must be 8-byte, count_out and bounds_out 4-byte aligned");
    if (n == 0) return 0;
    sr::launch_depth_mark(sr::depth_items(B, H, W, cameras, depths, depth_is_double), masks, workspace, count_out, bounds_out,
                          static_cast<hipStream_t>(hip_stream));
    return check_hip(hipGetLastError(), "depth_points_mark");
}

int sr_depth_points_gather(int B, int H, int W, const SrDepthCamera* cameras, const void* depths, int depth_is_double, const void* images,
                           int color_bytes, const void* workspace, long long capacity, float* points_out, void* colors_out,
                           long long* indices_out, void* hip_stream) {
    const long long n = depth_batch("sr_depth_points_gather", B, H, W, cameras, depths, depth_is_double);
    if (n < 0) return 1;
    if (capacity < 0) return fail("sr_depth_points_gather: capacity must not be negative");
    if (!workspace || (reinterpret_cast<uintptr_t>(workspace) & 7u)) return fail("null or misaligned workspace in sr_depth_points_gather");
    sr::DepthRows rows;
    SR_TRY(depth_rows("sr_depth_points_gather", images, color_bytes, points_out, colors_out, indices_out, &rows));
    if (n == 0 || capacity == 0 || (!points_out && !colors_out && !indices_out)) return 0;
    sr::launch_depth_gather(sr::depth_items(B, H, W, cameras, depths, depth_is_double), workspace, capacity, rows,
                            static_cast<hipStream_t>(hip_stream));
    return check_hip(hipGetLastError(), "depth_points_gather");
}

int sr_depth_points_select(int B, int H, int W, const SrDepthCamera* cameras, const void* depths, int depth_is_double, const void* images,
                           int color_bytes, const void* workspace, const long long* ranks, long long n_ranks, float* points_out,
                           void* colors_out, long long* indices_out, int* flag_out, void* hip_stream) {
    const long long n = depth_batch("sr_depth_points_select", B, H, W, cameras, depths, depth_is_double);
    if (n < 0) return 1;
    if (n_ranks < 0 || n_ranks > kDepthMaxItems) return fail("sr_depth_points_select: n_ranks must be in 0 .. 2^31 - 1");
    if (!workspace || (reinterpret_cast<uintptr_t>(workspace) & 7u)) return fail("null or misaligned workspace in sr_depth_points_select");
    if (n_ranks > 0 && (!ranks || !flag_out)) return fail("null pointer in sr_depth_points_select");
    if ((reinterpret_cast<uintptr_t>(ranks) & 7u) || sr::any_unaligned4(flag_out))
        return fail("sr_depth_points_select: ranks must be 8-byte and flag_out 4-byte aligned");
    sr::DepthRows rows;
    SR_TRY(depth_rows("sr_depth_points_select", images, color_bytes, points_out, colors_out, indices_out, &rows));
    if (n_ranks == 0 || (!points_out && !colors_out && !indices_out)) return 0;
    if (n == 0) return fail("sr_depth_points_select: an empty batch has no row to select");
    sr::launch_depth_select(sr::depth_items(B, H, W, cameras, depths, depth_is_double), workspace, ranks, n_ranks, rows, flag_out,
                            static_cast<hipStream_t>(hip_stream));
    return check_hip(hipGetLastError(), "depth_points_select");
}

}  // extern "C"
