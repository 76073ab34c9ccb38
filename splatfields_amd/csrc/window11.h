// The separable 11-tap window over a 32 x 32 tile, as the photometric loss and the evaluation metrics walk it: the tile's
// 42 x 42 input region lies in LDS at a row stride of 44, a row pass writes planes of [42][32], a column pass reads them.
// The taps are the caller's: the two ops restate two different formulas of the reference, whose float32 values differ.
#pragma once
#include <hip/hip_runtime.h>

namespace sr {

constexpr int kWinTile = 32;                       // output tile edge
constexpr int kWinTaps = 11;
constexpr int kWinHalo = kWinTaps / 2;
constexpr int kWinRaw = kWinTile + kWinTaps - 1;   // 42: the input region of a tile
constexpr int kWinRawStride = 44;                  // LDS row stride of the region: 16-byte rows for the ds_read_b128 of the row pass
constexpr int kWinQuads = kWinTile / 4;            // a thread filters 4 neighbouring columns

// 14 neighbouring values of LDS row `row` of the region, from column 4 * quad (two columns more are read and not used)
__device__ __forceinline__ void win_read_span(const float* __restrict__ s, int row, int quad, float (&v)[16]) {
    const float4* p = reinterpret_cast<const float4*>(s + row * kWinRawStride + 4 * quad);
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const float4 q = p[j];
        v[4 * j] = q.x; v[4 * j + 1] = q.y; v[4 * j + 2] = q.z; v[4 * j + 3] = q.w;
    }
}

// row pass: 4 neighbouring outputs of the filter over a span
__device__ __forceinline__ void win_filter_span(const float (&w)[kWinTaps], const float (&v)[16], float (&o)[4]) {
#pragma unroll
    for (int j = 0; j < 4; ++j) o[j] = 0.0f;
#pragma unroll
    for (int t = 0; t < kWinTaps; ++t)
#pragma unroll
        for (int j = 0; j < 4; ++j) o[j] = fmaf(w[t], v[j + t], o[j]);
}

// column pass: 4 neighbouring outputs of row `row` from a row-filtered plane [kWinRaw][kWinTile].  A wavefront reads
// 8 quads x 8 rows = 1 KiB of consecutive LDS per tap: no bank conflict.
__device__ __forceinline__ void win_filter_column(const float (&w)[kWinTaps], const float* __restrict__ s, int row, int quad, float (&o)[4]) {
#pragma unroll
    for (int j = 0; j < 4; ++j) o[j] = 0.0f;
#pragma unroll
    for (int t = 0; t < kWinTaps; ++t) {
        const float4 q = *reinterpret_cast<const float4*>(s + (row + t) * kWinTile + 4 * quad);
        o[0] = fmaf(w[t], q.x, o[0]); o[1] = fmaf(w[t], q.y, o[1]); o[2] = fmaf(w[t], q.z, o[2]); o[3] = fmaf(w[t], q.w, o[3]);
    }
}

}  // namespace sr
