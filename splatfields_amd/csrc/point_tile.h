// How the per-point heads (flow_head.hip, view_color.hip) move a [N, width] fp32 matrix whose rows are up to 1 KiB: a thread
// walking its own row would touch 64 cache lines per wave instruction, so the workgroup moves 16 columns of its 256 rows at a time
// through an LDS tile -- four lanes load (or store) the four 16-byte vectors of one row's 64-byte piece, and each thread reads
// (or has written) its own row's piece in the tile (row stride 20 floats: the 16 lanes of a ds_read_b128 group land on 16
// different 4-bank slots).  The caller places the barriers: one after tile_load before the tile is read, one before the tile is
// written again.
#pragma once
#include "common.h"

namespace sr {

constexpr int kTileCols = 16;            // columns of the matrix per pass through the tile
constexpr int kTileRow = 20;             // floats per tile row: 16 + 4 of padding

// 16 columns [c0, c0 + 16) of this workgroup's 256 rows of `src` into the tile; columns past the width and rows past n read as zeros
__device__ __forceinline__ void tile_load(const float* __restrict__ src, long long first, long long n, int width, int c0, float* s_tile) {
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int idx = (int)threadIdx.x + kBlock * i, row = idx >> 2, q = idx & 3;
        const long long point = first + row;
        float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
        if (point < n && c0 + 4 * q < width) v = *reinterpret_cast<const float4*>(src + (size_t)point * width + c0 + 4 * q);
        *reinterpret_cast<float4*>(s_tile + row * kTileRow + 4 * q) = v;
    }
}

__device__ __forceinline__ void tile_store(float* __restrict__ dst, long long first, long long n, int width, int c0, const float* s_tile) {
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int idx = (int)threadIdx.x + kBlock * i, row = idx >> 2, q = idx & 3;
        const long long point = first + row;
        if (point < n && c0 + 4 * q < width)
            *reinterpret_cast<float4*>(dst + (size_t)point * width + c0 + 4 * q) = *reinterpret_cast<const float4*>(s_tile + row * kTileRow + 4 * q);
    }
}

}  // namespace sr
