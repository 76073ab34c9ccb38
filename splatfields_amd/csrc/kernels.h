// Host-side launchers of the gfx950 kernels (one translation unit per pipeline stage).
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
void launch_sort_tiles(const ViewK& v, const Geom& g, const Binning& b, long long max_len, long long expected_len, hipStream_t st);
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

// densify.hip
struct DensifyArgs { float grad_threshold, min_opacity, extent, percent_dense, max_screen_size; };
size_t densify_workspace_bytes(int n);
void launch_densify_plan(int n, const float* log_scales, int scale_cols, const float* opacity_logit, const float* grad_accum,
                         const float* denom, const float* max_radii2D, const DensifyArgs& a, void* workspace, int32_t* dest,
                         uint32_t** totals_out, hipStream_t st);
void launch_densify_gather(int n, int row, const float* src, float* dst, const int32_t* dest, int mode, const float* log_scales,
                           int scale_cols, const float* rotations, const float* unit, hipStream_t st);

// hull.hip: arguments are checked by the caller (sr_hull_*); exactly one of grid / points, n = G^3 or the number of points
size_t hull_workspace_bytes(long long n);
hipError_t launch_hull_carve(int n_views, const SrHullView* host_views, const uint8_t* masks, const double* grid, int G, const void* points,
                             long long n, int point_is_double, void* workspace, int* count_out, hipStream_t st);
void launch_hull_gather(const double* grid, int G, const void* points, long long n, int point_is_double, const void* workspace,
                        long long capacity, int* indices_out, float* points_out, hipStream_t st);

// mlp.hip
size_t mlp_weight_grad_workspace(int n_points, int n_jobs, const SrMlpGradJob* jobs);
int launch_mlp_weight_grad(int n_points, int n_jobs, const SrMlpGradJob* jobs, void* workspace, size_t workspace_bytes, hipStream_t st);
int launch_mlp_pack(int n_jobs, const SrMlpPackJob* jobs, bool bf16, hipStream_t st);
int launch_mlp_chain(int n_points, int hidden_tiles, int n_ops, const SrMlpOp* ops, float slope, bool bf16, hipStream_t st);

int launch_mlp_input_forward(int N, int L, int F, int TL, int row, const float* xyz, const float* feat, const float* time, float* x0, hipStream_t st);
int launch_mlp_top_gradient(int N, int out, int row, const float* y, const float* dy, float slope, float* G, hipStream_t st);
int launch_mlp_input_backward(int N, int L, int F, int row, const float* xyz, const float* g, float* d_xyz, float* d_feat, hipStream_t st);
// the heads of a step as one group (sr_mlp_chain_group, sr_mlp_group_*): nullptr, or why the call is refused (nothing launched)
const char* launch_mlp_chain_group(int n_points, int hidden_tiles, int n_nets, const SrMlpNet* nets, float slope, bool bf16, hipStream_t st);
const char* launch_mlp_group_input_forward(int N, int n_heads, const SrMlpHeadInput* heads, int F, int TL, const float* xyz, const float* feat,
                                           const float* time, hipStream_t st);
const char* launch_mlp_group_input_backward(int N, int n_heads, const SrMlpHeadInput* heads, int F, const float* xyz, float* d_xyz, float* d_feat,
                                            hipStream_t st);
const char* launch_mlp_group_output(int N, int n_heads, const SrMlpHeadOutput* heads, hipStream_t st);
const char* launch_mlp_group_top_gradient(int N, int n_heads, const SrMlpHeadOutput* heads, float slope, hipStream_t st);
int launch_resfield_compose(int n_jobs, const SrResFieldJob* jobs, const long long* frame, hipStream_t st);
size_t resfield_backward_workspace(int n_jobs, const SrResFieldJob* jobs);
int launch_resfield_backward(int n_jobs, const SrResFieldJob* jobs, const long long* frame, void* workspace, size_t workspace_bytes, hipStream_t st);

// triplane.hip
int launch_triplane_forward(int N, int C, int H, int W, const float* planes_chw, float* planes_hwc, const float* pts, float* out, hipStream_t st);
int launch_triplane_backward(int N, int C, int H, int W, const float* planes_hwc, const float* pts, const float* g, float* d_planes_chw,
                             float* d_pts, void* workspace, hipStream_t st);
size_t triplane_backward_workspace(int N, int C, int H, int W);

// knn.hip
size_t knn_workspace_bytes(int n);
void launch_knn3(int n, const float* pts, float* out, void* workspace, hipStream_t st);
constexpr int kKnnMinK = 2, kKnnMaxK = 8;
size_t knn_graph_workspace_bytes(int n, int k);   // 0 for sizes out of range
void launch_knn_graph(int n, int k, const float* pts, int* nn_ix, uint32_t* order, uint32_t* rev_start, uint32_t* rev_edges, void* workspace,
                      hipStream_t st);

// moran.hip
constexpr int kMoranMaxTensors = SR_MORAN_MAX_TENSORS;
// the feature tensors of one call: x[t] is [rows, width[t]]; dx[t] (backward) may be NULL; offset[] are the running widths,
// edge_offset[] the running widths of the tensors with a dx: only those have columns in the per-edge buffer
struct MoranTensors {
    int count, channels, edge_channels;
    const float* x[kMoranMaxTensors]; float* dx[kMoranMaxTensors];
    int width[kMoranMaxTensors], offset[kMoranMaxTensors], edge_offset[kMoranMaxTensors];
};
// where the K x K spatial weights of item p come from: `points` (c_ab from the distances of the K gathered positions) or
// `weight` [n, K, K] given; nn_ix NULL: item p's rows are p K .. p K + K - 1; order NULL: items in index order
struct MoranSource { int n, k; float eps; const float* points; const float* weight; const int* nn_ix; const uint32_t* order; };
size_t moran_workspace_bytes(int n, int n_tensors);
size_t moran_edges_bytes(int n, int k, int channels);
void launch_moran_forward(const MoranSource& s, const MoranTensors& t, void* workspace, float* out, hipStream_t st);
void launch_moran_backward(const MoranSource& s, const MoranTensors& t, const uint32_t* rev_start, const uint32_t* rev_edges, const float* out,
                           const float* upstream, void* edges, float* d_points, float* d_weight, hipStream_t st);
void launch_moran_weights(const MoranSource& s, float* weights, hipStream_t st);
void launch_moran_weights_backward(const MoranSource& s, const uint32_t* rev_start, const uint32_t* rev_edges, const float* d_weights,
                                   void* edges, float* d_points, hipStream_t st);

// loss.hip
bool loss_shape_ok(int batch, int channels, int H, int W);
size_t loss_workspace_bytes(int planes, int H, int W);
size_t loss_maps_bytes(int planes, int H, int W);
void launch_loss_forward(int batch, int channels, int H, int W, const float* image, const float* gt, const float* alpha,
                         const float* gt_mask, float lambda_dssim, float lambda_mask, void* workspace, float* maps, float* loss,
                         float* l1, float* ssim, float* mask_l1, hipStream_t st);
void launch_loss_backward(int batch, int channels, int H, int W, const float* image, const float* gt, const float* alpha,
                          const float* gt_mask, const float* maps, float w_l1, float w_ssim, float w_mask, const float* g, int g_per_item,
                          float* dL_dimage, float* dL_dalpha, hipStream_t st);

// metrics.hip
bool metrics_shape_ok(int batch, int H, int W);
size_t metrics_workspace_bytes(int batch, int H, int W);   // 0 for a shape out of range
void launch_image_metrics(int batch, int H, int W, const float* pred, const long long* pred_strides, const float* gt,
                          const long long* gt_strides, const float* mask, long long mask_item_stride, int quantize, void* workspace,
                          float* psnr, float* ssim, float* psnr_channels, unsigned char* frames, hipStream_t st);

// objective.hip: arguments are checked by the caller (sr_splat_reg_*, sr_depth_l1_*); n > 0, batch > 0
size_t splat_reg_workspace_bytes(long long n);
void launch_splat_reg_forward(long long n, const float* means3D, const float* opacity, double lambda_norm, double lambda_norm_mean,
                              double lambda_opacity, void* workspace, float* out, hipStream_t st);
void launch_splat_reg_backward(long long n, const float* means3D, const float* opacity, double lambda_norm, double lambda_norm_mean,
                               double lambda_opacity, const float* out, const float* upstream, float* d_means3D, float* d_opacity,
                               hipStream_t st);
bool depth_l1_shape_ok(int batch, int H, int W);
size_t depth_l1_workspace_bytes(int batch, int H, int W);   // 0 for a shape out of range or an empty batch
void launch_depth_l1_forward(int batch, int H, int W, const float* depth, const float* gt, void* workspace, float* out, hipStream_t st);
void launch_depth_l1_backward(int batch, int H, int W, const float* depth, const float* gt, const float* upstream, bool per_item,
                              float* grad, hipStream_t st);

// adam.hip: the jobs are checked by the caller (sr_adam_step); jobs with count 0 are skipped
void launch_adam(int n_jobs, const SrAdamJob* jobs, const unsigned char* visible, hipStream_t st);

// planegen.hip: shapes are checked by the caller (plane_*_ok); every function is exactly one kernel launch
bool plane_channels_ok(int c);
bool plane_conv_shape_ok(int cin, int cout, int hin, int win, int flags);
bool plane_gn_shape_ok(int channels, int groups, int h, int w);
size_t gn_stats_workspace(int n_planes, int channels, int groups, int h, int w);
void launch_gn_stats_partial(int n, const SrPlaneJob* jobs, int channels, int groups, int h, int w, void* ws, hipStream_t st);
void launch_gn_stats_final(int n, const SrPlaneJob* jobs, int channels, int groups, int h, int w, float eps, const void* ws, hipStream_t st);
void launch_conv3x3_forward(int n, const SrPlaneJob* jobs, int cin, int cout, int hin, int win, int groups, int flags, hipStream_t st);
void launch_conv3x3_backward_data(int n, const SrPlaneJob* jobs, int cin, int cout, int hin, int win, int flags, hipStream_t st);
size_t conv3x3_weight_grad_workspace(int n_planes, int cin, int cout, int hin, int win, int flags);
void launch_conv3x3_wgrad_partial(int n, const SrPlaneJob* jobs, int cin, int cout, int hin, int win, int groups, int flags, void* ws, hipStream_t st);
void launch_conv3x3_wgrad_reduce(int n, const SrPlaneJob* jobs, int cin, int cout, int hin, int win, int flags, const void* ws, hipStream_t st);
size_t gn_silu_backward_workspace(int n_planes, int channels, int h, int w);
void launch_gn_silu_backward_partial(int n, const SrPlaneJob* jobs, int channels, int groups, int h, int w, float eps, void* ws, hipStream_t st);
void launch_gn_silu_backward_apply(int n, const SrPlaneJob* jobs, int channels, int groups, int h, int w, float eps, const void* ws, hipStream_t st);

// flow_head.hip: arguments are checked by the caller (sr_flow_head_*: flow_head_shape_error / flow_head_branch_error, null = fine);
// n > 0; every launch_* is one kernel launch
const char* flow_head_shape_error(int model, long long n_points, int width, int n_basis);
const char* flow_head_branch_error(int model, int n_basis, int n_branches, const SrFlowBranch* branches);
int flow_head_outputs(int model, int n_basis);
int flow_head_dz_row(int model, int n_basis);
size_t flow_head_saved_bytes(int model, long long n, int n_basis);
size_t flow_head_workspace_bytes(int model, long long n, int n_basis);
void launch_flow_head_forward(int model, long long n, int width, int n_basis, int n_branches, const SrFlowBranch* branches, const float* hidden,
                              const float* pts, const float* bases, float* means, float* flow, void* saved, hipStream_t st);
void launch_flow_head_backward(int model, long long n, int width, int n_basis, int n_branches, const SrFlowBranch* branches, const float* pts,
                               const float* bases, const void* saved, const float* g_means, const float* g_flow, float* d_pts, float* d_z,
                               float* d_hidden, void* workspace, hipStream_t st);

// view_color.hip: arguments are checked by the caller (sr_view_color_*: view_color_shape_error, null = fine); n > 0; every
// launch_* is one kernel launch
const char* view_color_shape_error(int mode, long long n_points, int width, int n_views);
size_t view_color_saved_bytes(long long n);
size_t view_color_workspace_bytes(long long n);
void launch_view_color_forward(int mode, long long n, int width, int n_views, const float* feature, const float* means, const float* cam_or_dirs,
                               const float* weight, const float* bias, float* colours, void* saved, hipStream_t st);
void launch_view_color_backward(int mode, long long n, int width, int n_views, const float* means, const float* cam_or_dirs, const float* weight,
                                const void* saved, const float* g_colours, float* d_feature, float* d_pos, float* d_zsum, void* workspace,
                                hipStream_t st);

// attention.hip: shapes are checked by the caller (attention_shape_error: null = supported); every launch_* is one kernel launch
constexpr int kAttentionBackwardSteps = 6;     // launch_attention_backward(step = 0 .. 5), in this order
const char* attention_shape_error(int channels, int groups, int h, int w);
size_t attention_saved_bytes(int n_planes, int channels, int groups, int h, int w);
size_t attention_backward_workspace(int n_planes, int channels, int h, int w);
void launch_attention_stats(int n, const SrAttentionJob* jobs, int channels, int groups, int h, int w, float eps, hipStream_t st);
void launch_attention_qkv(int n, const SrAttentionJob* jobs, int channels, int groups, int h, int w, float eps, hipStream_t st);
void launch_attention_softmax(int n, const SrAttentionJob* jobs, int channels, int groups, int h, int w, float eps, hipStream_t st);
void launch_attention_backward(int step, int n, const SrAttentionJob* jobs, int channels, int groups, int h, int w, float eps, void* ws,
                               hipStream_t st);

// sh.hip
void launch_sh_forward(int N, int K, int deg, const float* means3D, const float* shs, const float* campos, float* colors,
                       unsigned char* clamped, hipStream_t st);
void launch_sh_forward_views(int N, int K, int deg, int V, const float* means3D, const float* shs, const float* campos, float* colors,
                             float* keep, hipStream_t st);
void launch_sh_backward(int N, int K, int deg, int V, const float* means3D, const float* shs, const float* campos, const float* dcol,
                        float scale, float* d_shs, float* d_means, int accumulate_means, hipStream_t st);

}  // namespace sr
