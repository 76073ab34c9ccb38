// Host-side launchers of the rasterizer's gfx950 kernels (one translation unit per pipeline stage), called from api.hip.
// Every other op keeps its launchers file-local, above its own entry points.
#pragma once
#include "common.h"

namespace sr {

struct SplatsK {
    int N;
    const float* means3D; const float* opacities; const float* scales; const float* rotations;
    const float* cov3D; const float* shs; const float* colors;
    int raw;  // SR_RAW_* bits: activations applied on load, their derivatives on the way out
    const float* shs_rest;  // non-NULL: shs = dc [N,1,3], shs_rest = [N,15,3]
};

struct GradsK {
    float* means3D; float* means2D; float* opacity; float* scales; float* rotations; float* cov3D;
    float* shs; float* colors; float* shs_rest;
};

// preprocess.hip
void launch_preprocess(const ViewK& v, const SplatsK& s, const Geom& g, int* radii, hipStream_t st);
void launch_mark_visible(int N, const float* means3D, const float* viewmatrix, unsigned char* present, hipStream_t st);
void launch_densification_stats(int N, const float* dL_dmeans2D, const int* radii, float* grad_accum, float* denom, float* max_radii2D,
                                hipStream_t st);
void launch_preprocess_backward(const ViewK& v, const SplatsK& s, const Geom& g, const int* radii,
                                const float* slots, const uint8_t* reached, const GradsK& gr, int first, int count, bool small_footprint,
                                hipStream_t st);
// binning.hip
// true when the image is small enough for the atomic-free count-matrix bucketing
inline bool use_count_matrix(const ViewK& v) { return v.gx * v.gy <= kMaxMatrixTiles; }
void launch_count_tiles(const ViewK& v, int N, const Geom& g, hipStream_t st);
void launch_scan_small(const ViewK& v, int N, const Geom& g, uint32_t* host_out, uint32_t host_seq, hipStream_t st);
void launch_emit(const ViewK& v, int N, const Geom& g, const Binning& b, hipStream_t st);
int launch_sort_tiles(const ViewK& v, const Geom& g, const Binning& b, long long max_len, long long expected_len, long long long_tiles,
                      hipStream_t st);
// render.hip
void launch_render_forward(const ViewK& v, const Geom& g, const Binning& b, const Image& im,
                           float* out_color, float* out_depth, float* out_alpha, hipStream_t st);
void launch_render_backward(const ViewK& v, const Geom& g, const Binning& b, const Image& im,
                            const float* dL_dcolor, const float* dL_ddepth, const float* dL_dalpha,
                            float* slots, hipStream_t st);
// blend_bwd.hip
void launch_render_backward_quads(const ViewK& v, const Geom& g, const Binning& b, const Image& im,
                                 const float* dL_dcolor, const float* dL_ddepth, const float* dL_dalpha,
                                 float* slots, hipStream_t st);

int backward_stats(unsigned long long* out8, int reset);

}  // namespace sr
