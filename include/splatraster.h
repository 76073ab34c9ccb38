/*
 * splatraster.h -- C ABI of libsplatraster.so, the MI355X (gfx950) differentiable
 * Gaussian-splat rasterizer that replaces the `diff_gaussian_rasterization._C` extension
 * SplatFields imports at reference gaussian_renderer/__init__.py:14.
 *
 * Every entry point takes plain pointers and sizes; no torch / C++ types cross this boundary.
 * All device memory (inputs, outputs, gradients, the three opaque state buffers) is owned by
 * the caller (PyTorch-ROCm tensors, `tensor.data_ptr()`); the library owns nothing persistent (its only state: 64-byte
 * status blocks of pinned, coherent host memory -- one per host thread and device for sr_forward, a pool per device for the
 * tickets of sr_forward_async --, the mutex-guarded event list of the optional stage profiling, and per-device "attribute
 * set" flags of three kernels).
 * Every kernel is launched on the caller-supplied HIP stream.  Functions return 0 on success,
 * a non-zero status otherwise; `sr_last_error()` returns a thread-local message.
 *
 * Which upstream interface each entry replaces ([EXT] = the pip dependency
 * ingra14m/depth-diff-gaussian-rasterization@f2d8fa9, reference README.md:28, not vendored):
 *
 *   sr_forward_prepare + sr_forward_render
 *        <- [EXT] `_C.rasterize_gaussians(...)`, reached from `GaussianRasterizer.forward`
 *           called at reference gaussian_renderer/__init__.py:94-102 and :106-114.
 *   sr_backward
 *        <- [EXT] `_C.rasterize_gaussians_backward(...)`, reached from autograd when
 *           reference train.py:252 runs `loss.backward()`.
 *   sr_forward_prepare_views + sr_forward_render_views, sr_sum_views
 *        <- the loop of reference train.py:158-177 around those two (up to `num_views` views per iteration, one backward):
 *           the forward of all views with one host wait, and the sum autograd forms of the views' gradients of a shared input.
 *   sr_mark_visible
 *        <- [EXT] `_C.mark_visible(...)` (`GaussianRasterizer.markVisible`; never called by
 *           SplatFields, exported for completeness).
 *   sr_densification_stats
 *        <- reference train.py:280-286 and scene/gaussian_model.py:427-438 (`add_densification_stats`): the
 *           consumers of `radii` and `viewspace_points.grad`, fused into one kernel.
 *   sr_photometric_forward / sr_photometric_backward
 *        <- reference train.py:183-193 with utils/loss_utils.py:18 (`l1_loss`) and :33-76 (`ssim`): the loss between
 *           `render()` and `loss.backward()`, as one kernel each way plus a fixed-order reduction.
 *   sr_knn_graph + sr_moran_forward / sr_moran_backward, sr_moran_weights / sr_moran_weights_backward
 *        <- reference extract_geo.py:100-143 (`query_nn`, `morans_measure`, `morans_loss`) as train.py:203-215 calls them:
 *           [EXT] pytorch3d.ops.knn.knn_points and the [N,F,K,K] temporaries of the Moran's I regulariser.
 *   sr_image_metrics
 *        <- reference render.py:33-160 (`compute_psnr`, `compute_ssim`: the scipy evaluation `eval_all` runs per image on the
 *           host) and utils/image_utils.py:19-21 (`psnr`, train.py:387-396), with the 8-bit quantisation of the image files
 *           in between (torchvision `save_image`, render.py:282 `to8b`): a batch of views in one kernel plus a fixed-order
 *           reduction.
 *   sr_lpips_pack_weights + sr_lpips_forward
 *        <- reference render.py:174-180 (`eval_lpips`) as `eval_all` (render.py:163-207) calls it: [EXT] the `lpips` package's
 *           VGG-16 trunk, five taps and distance, with weights the caller supplies, for a batch of views: 13 convolution
 *           launches, 5 head launches and a fixed-order reduction.
 *   sr_splat_reg_forward / sr_splat_reg_backward, sr_depth_l1_forward / sr_depth_l1_backward
 *        <- reference train.py:195-201 (`lambda_norm`, `lambda_norm_mean`), :244-246 (`lambda_opacity`) and :224-229
 *           (`lambda_depthl1`): the tail of the objective between `render()` and `loss.backward()`, each a streaming pass and a
 *           fixed-order reduction forward and one kernel backward.
 *   sr_adam_step
 *        <- reference train.py:314-322 (`gaussians.optimizer.step()`), the `torch.optim.Adam` of scene/gaussian_model.py:130-139:
 *           every tensor of the step in one launch.
 *   sr_net_adam_plan, sr_net_adam_step
 *        <- reference train.py:318 (`deform.optimizer.step()`), the `torch.optim.Adam` of scene/deform_model.py:23-34 over the
 *           deform network's 71 to 502 parameter tensors: a job table in device memory, one launch per 480 tensors.
 *   sr_groupnorm_stats, sr_conv3x3_forward / _backward_data / _weight_grad, sr_groupnorm_silu_backward
 *        <- reference scene/time_decoders.py (`TimeVAEDecoder`) behind scene/tripFields.py:176-204 (`Tensorial2D`): the plane
 *           generator's GroupNorm -> SiLU -> [nearest x2] -> conv 3x3 -> [+ residual] layers, all planes per launch.
 *   sr_hull_carve + sr_hull_gather
 *        <- the visual hull every shipped recipe starts from (`--pts_samples hull` / `load`), reference
 *           scene/dataset_readers.py:1385-1417 (`visual_hull_samples`), :1419-1458 (`visual_hull_samples_list`), :605-644 (the
 *           Blender `hull` branch of `readNerfSyntheticInfo`) and :544-588 (its `load` branch, a point cloud filtered by the same
 *           test): the host's projection of a G^3 grid into every training view, as one streaming pass plus an ordered compaction.
 *   sr_depth_points_mark + sr_depth_points_gather / sr_depth_points_select
 *        <- reference scene/dataset_readers.py:1476-1491 (`_gen_3dpoints`, called per camera and frame at :1376 and :1463) and
 *           what `readNeuSceneInfo` takes from the concatenated cloud: its bounds (:1603-1613, the hull's box) or `num_pts`
 *           random rows (:1653-1658, the `depth` initialisation): one streaming pass, an ordered compaction or a sample by rank.
 *   sr_draw_rows / sr_draw_rows_ascending, sr_rows_gather / sr_rows_scatter, sr_densification_stats_rows
 *        <- the `--n_splats` subset step: reference train.py:56-60 (`torch.randperm(N)[:n_splats]` on the host and the indexing of
 *           xyz, scaling and features), :68 (`idx` in gaussian_dict), :281-286 and scene/gaussian_model.py:431-438 (the `_idx`
 *           branch of the densification bookkeeping) -- and the `torch.randperm(M)[:n_pts]` of the two initialisations.
 *   SrView
 *        <- the 12-field `GaussianRasterizationSettings` built at reference
 *           gaussian_renderer/__init__.py:59-72 (and :76-89 for the alpha pass).
 *   SrSplats
 *        <- the keyword arguments of the call at reference gaussian_renderer/__init__.py:94-102.
 *   geom / binning / image buffers
 *        <- [EXT] geomBuffer / binningBuffer / imgBuffer saved by the autograd ctx.
 *
 * Conventions: viewmatrix / projmatrix are the *transposed* matrices of
 * reference scene/cameras.py:68-73 stored contiguously, i.e. element [i][j] at ptr[4*i+j] and
 * p_hom = [x y z 1] @ M; quaternions are (r,x,y,z) used as given; scales and opacities are
 * already activated; SH is [N,K,3] coefficient-major.
 */
#ifndef SPLATRASTER_H
#define SPLATRASTER_H

#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

/* Version of this ABI; sr_version() returns the library's.  A caller built against another version must not use the library
 * (the binding checks at load).  History: 3 = rounds 2-3; 4 = round 4's additions made official (sr_backward's `binning` is
 * written; sr_backward_blend / sr_backward_splats / sr_debug_snapshot; Geom's eight count words; images of at most 4095 tiles a
 * side; record quarter 3 / block_offsets carry the instance index) + round 5: sr_forward_async / sr_ticket_* / sr_debug_counters. */
#define SR_VERSION 4
#define SR_TILE 16 /* binning tile edge in pixels (upstream BLOCK_X = BLOCK_Y) */

typedef struct SrView {
    int image_height;         /* 1..65520: at most 4095 tiles a side (tile coordinates are stored in 12 bits) */
    int image_width;          /* 1..65520 */
    float tanfovx;
    float tanfovy;
    float scale_modifier;
    int sh_degree;            /* active SH degree, 0..3 */
    int sh_coeffs;            /* K = coefficients stored per splat (shs.shape[1]); 0 with precomputed colours */
    int prefiltered;
    int debug;                /* non-zero: synchronise + check after every launch */
    const float* viewmatrix;  /* device, 16 floats */
    const float* projmatrix;  /* device, 16 floats */
    const float* campos;      /* device, 3 floats */
    const float* bg;          /* device, 3 floats */
} SrView;

typedef struct SrSplats {
    int count;                   /* N */
    const float* means3D;        /* device [N,3] */
    const float* opacities;      /* device [N] (the [N,1] tensor, contiguous) */
    const float* scales;         /* device [N,3]; NULL iff cov3D_precomp is given */
    const float* rotations;      /* device [N,4]; NULL iff cov3D_precomp is given */
    const float* cov3D_precomp;  /* device [N,6] (xx,xy,xz,yy,yz,zz) or NULL */
    const float* shs;            /* device [N,K,3] or NULL */
    const float* colors_precomp; /* device [N,3] or NULL (exactly one of shs / colors_precomp) */
    int raw_params;              /* bit mask of SR_RAW_*: inputs that arrive as the optimiser's raw parameters; the activation of
                                  * reference scene/gaussian_model.py:64-86 is applied inside the preprocess kernels and its
                                  * derivative inside sr_backward (the gradients are then w.r.t. the raw parameters) */
    const float* shs_rest;       /* NULL, or device [N,15,3]: the SH coefficients arrive as the reference stores them, `shs` =
                                  * `_features_dc` [N,1,3] and `shs_rest` = `_features_rest` [N,15,3] (scene/gaussian_model.py:40-41),
                                  * instead of their per-iteration concatenation (:79-82); needs sh_coeffs == 16, both 16-byte
                                  * aligned.  The gradients then go to SrGrads.dL_dshs [N,1,3] and dL_dshs_rest [N,15,3]. */
} SrSplats;

#define SR_RAW_SCALES 1    /* scales = log-scales:        get_scaling  = exp(_scaling)          (gaussian_model.py:64-68) */
#define SR_RAW_OPACITY 2   /* opacities = logits:         get_opacity  = sigmoid(_opacity)      (gaussian_model.py:84-86) */
#define SR_RAW_ROTATIONS 4 /* rotations = unnormalised:   get_rotation = normalize(_rotation)   (gaussian_model.py:70-72) */
#define SR_FORWARD_ONLY 8  /* no sr_backward will follow this forward (rendering / evaluation): state only the backward reads is not
                            * written (the 36 B/splat colour-direction Jacobian of the SH path) */

/* Dense per-splat gradient outputs, all written in full by sr_backward (culled splats get zeros). */
typedef struct SrGrads {
    float* dL_dmeans3D;   /* [N,3] */
    float* dL_dmeans2D;   /* [N,3]; [:, :2] in the upstream NDC-scaled convention (x 0.5*W, 0.5*H), [:,2] = 0 */
    float* dL_dopacity;   /* [N]   */
    float* dL_dscales;    /* [N,3] or NULL with cov3D_precomp */
    float* dL_drotations; /* [N,4] or NULL with cov3D_precomp */
    float* dL_dcov3D;     /* [N,6] or NULL unless cov3D_precomp */
    float* dL_dshs;       /* [N,K,3] or NULL */
    float* dL_dcolors;    /* [N,3] or NULL.  With SH input, dL_dshs == NULL and dL_dcolors != NULL selects the colour-gradient
                           * mode: the clamp-masked dL/dcolour is written instead of dL/dsh (view-parallel exchange, sr_sh_backward);
                           * the gradient through the view direction is still added to dL_dmeans3D. */
    float* dL_dshs_rest;  /* [N,15,3] with SrSplats.shs_rest, else NULL */
} SrGrads;

int sr_version(void);
const char* sr_last_error(void);

/* Sizes (bytes) of the caller-allocated opaque buffers.  `instances` is the value
 * sr_forward_prepare returned for this view. */
size_t sr_geom_bytes(int n_splats, int height, int width);
size_t sr_binning_bytes(long long instances, int height, int width);
size_t sr_image_bytes(int height, int width);
size_t sr_backward_scratch_bytes(long long instances);

/* Stage 1: cull, 3D->2D covariance projection (EWA), conic, radius, tile rectangle, SH->RGB,
 * per-tile instance counts and their prefix sums.  Writes `radii` [N] (int32) and the geom buffer.
 * Blocks on the stream once to read back the number of tile-splat instances. */
int sr_forward_prepare(const SrView* view, const SrSplats* splats, void* geom, int* radii,
                       long long* instances_out, void* hip_stream);

/* Stage 2: bucket instances per tile, sort each tile's list front-to-back (depth, then splat
 * index), alpha-composite.  Writes out_color [3,H,W], out_depth [1,H,W], out_alpha [1,H,W]
 * (= 1 - final transmittance; may be NULL) plus the binning and image state buffers. */
int sr_forward_render(const SrView* view, const SrSplats* splats, void* geom, void* binning,
                      long long instances, void* image, float* out_color, float* out_depth,
                      float* out_alpha, void* hip_stream);

/* Both forward stages in one call WITHOUT draining the pipeline: stage 1 is launched -- its last kernel stores the instance
 * count and the longest tile list into a status block (pinned, coherent host memory) and then publishes the block's sequence
 * number; nothing is enqueued in the stream for the read-back, neither a copy nor an event --, stage 2 is launched right behind
 * it for a binning buffer sized for `binning_capacity` instances (every stage-2 kernel exits immediately if the count exceeds
 * it), and only then does the host wait: it polls the block while the GPU keeps running stage 2.  (So the host still blocks
 * once per forward, as upstream's num_rendered read-back does, but only until stage 1 has finished: the GPU never idles.)
 * Returns 0 when the count fits (outputs valid), SR_NEED_CAPACITY when it does not: the caller then allocates
 * sr_binning_bytes(*instances_out) and calls sr_forward_render with instances = *instances_out.
 * The binning buffer is carved for the capacity it was rendered with; pass that same number as `instances`
 * to sr_backward.
 * Threading: the read-back uses one status block per (host thread, device); host threads may call concurrently, each on its
 * own stream and buffers. */
#define SR_NEED_CAPACITY 2
int sr_forward(const SrView* view, const SrSplats* splats, void* geom, int* radii, void* binning,
               long long binning_capacity, void* image, float* out_color, float* out_depth, float* out_alpha,
               long long* instances_out, void* hip_stream);

/* sr_forward WITHOUT any host wait (the capacity-bounded form of SURVEY.md section 8b: "... or is avoided with a capacity-bounded
 * workspace"; [EXT] reads num_rendered back in the middle of every forward).  The caller supplies what sr_forward learns by
 * waiting -- a binning capacity and the longest tile list to expect (`longest_list_hint`: which sort classes to launch: lists up
 * to 2048 / 4096 / 8192 entries, or all) -- typically what an earlier forward of the same view reported, with headroom.  Both
 * stages are launched back to back and the call returns; every stage-2 kernel exits on the device if the instance count
 * exceeds the capacity, and the blend exits if a list is longer than the launched sort classes cover, so a wrong guess never
 * reads or writes out of bounds -- it leaves the OUTPUTS UNDEFINED.  `*ticket_out` receives a ticket (a status block of its
 * own, which stage 1 fills as it does sr_forward's; pooled inside the library); the caller MUST redeem it with sr_ticket_wait before it uses
 * the outputs' gradients (before sr_backward at the latest): it waits for stage 1 of that forward only -- usually long
 * finished -- and returns the instance count and the longest list; the outputs are valid iff
 *     instances <= binning_capacity  and  longest_list <= max(2048, the class bound the hint selected).
 * When they are not, re-run the forward (sr_forward, or sr_forward_async with the reported figures).
 * `longest_list_expected` (<= the hint, or -1): the figure without its headroom.  A sort class that is launched only for the
 * headroom's sake (no list of its length is expected) gets a grid of a few workgroups instead of 512: it finds nothing and
 * leaves, or sorts the one list that did grow into it.
 * sr_ticket_release = sr_ticket_wait without results (a forward whose outputs were dropped).  A ticket is redeemed once. */
int sr_forward_async(const SrView* view, const SrSplats* splats, void* geom, int* radii, void* binning,
                     long long binning_capacity, long long longest_list_hint, long long longest_list_expected, void* image,
                     float* out_color, float* out_depth, float* out_alpha, void** ticket_out, void* hip_stream);
int sr_ticket_wait(void* ticket, long long* instances_out, long long* longest_list_out);
/* the longest tile list of the calling thread's most recent sr_forward (-1 before the first): the hint of a later
 * sr_forward_async of the same view */
long long sr_last_longest_list(void);
/* How many tiles of the view can hold a list of more than 2048 entries (an upper bound from the coarse length classes of the
 * launch order; 0 when the longest list has at most 2048): the figure of the calling thread's most recent sr_forward or
 * sr_ticket_wait (-1 before the first).  Next to the longest list it is what a caller learns about a camera. */
long long sr_last_long_tiles(void);
/* What the caller expects that figure to be for the NEXT sr_forward_async of the calling thread (consumed by that call; < 0 or
 * never called: no expectation).  With at most 8 expected, and a longest_list_expected of at most 4096, the separate sort
 * launch for lists of 2049..4096 entries is left out and the forward blend sorts whatever such lists the view turns out to
 * have: a wrong expectation costs time, never a result.  Returns 0. */
int sr_expect_long_tiles(long long tiles);
int sr_ticket_release(void* ticket);

/* The forward of the n_views views of one training step (reference train.py:158-177 renders up to `num_views` views and
 * back-propagates once) in two calls with ONE host wait between them.  Every table has n_views entries: `views` and `splats`
 * are arrays of the structs themselves, the others arrays of what the one-view entries take.
 *   sr_forward_prepare_views  launches stage 1 of every view back to back, each with a status block of its own from the ticket
 *       pool, then waits once on the host -- for the last view's block first, by which time the others have long arrived -- and
 *       returns per view the instance count, the longest tile list and the number of tiles that can hold a list of more than 2048
 *       entries (what sr_forward learns by waiting, and sr_last_longest_list / sr_last_long_tiles report).  It counts as one
 *       host wait in sr_debug_counters.  The blocks go back to the pool on every path, with sr_forward_async's rule for a failed
 *       launch (the stream is drained first) and sr_ticket_wait's for figures that never arrive (that block is not reused).
 *   sr_forward_render_views   launches stage 2 of every view with those figures: binning buffers of capacities[v] >= the
 *       view's instance count (sr_binning_bytes(capacities[v])), and exactly the sort classes a waiting sr_forward launches
 *       for a longest list of longest[v] on a view with long_tiles[v] such tiles.  It never waits.  out_alpha, or any of its
 *       entries, may be NULL.  Pass capacities[v] as `instances` and the view's count as `instances_rendered` to sr_backward.
 * Outputs, state buffers and gradients of a view are bit for bit those of sr_forward / sr_backward on that view. */
int sr_forward_prepare_views(int n_views, const SrView* views, const SrSplats* splats, void* const* geoms, int* const* radii,
                             long long* instances_out, long long* longest_out, long long* long_tiles_out, void* hip_stream);
int sr_forward_render_views(int n_views, const SrView* views, const SrSplats* splats, void* const* geoms, void* const* binnings,
                            const long long* capacities, const long long* longest, const long long* long_tiles, void* const* images,
                            float* const* out_color, float* const* out_depth, float* const* out_alpha, void* hip_stream);

/* The sum over the views of a step of the gradients of the inputs the views share, ONE launch for every tensor: job j has
 * n_views source tensors of `elems` floats, view v at src + v * view_stride, and writes
 *   dst[i] = ((src[V-1][i] + src[V-2][i]) + ...) + src[0][i]                                      (float32, V = n_views)
 * -- the left fold from the LAST view to the first: the order in which autograd accumulates the gradients of V rasterizer
 * nodes that share an input (it runs the node created last first), so the sum has the bits of the per-view loop's.
 * dst overlaps no source and no other job's dst.  All bases are 4-byte aligned; where dst, src and 4 * view_stride agree modulo 16 the body moves as 16-byte vectors
 * and only the unaligned head and tail go element by element.  elems <= 2^31 - 1.  n_views >= 1; more than SR_SUM_MAX_VIEWS
 * views are folded by chained launches of at most that many each, the partial sum being the first operand of the next: the
 * association does not change.  n_jobs = 0 and jobs of 0 elements are valid and launch nothing.  The job table is the kernel
 * argument (no copy); no LDS, no atomics, nothing waits for the device. */
#define SR_SUM_MAX_JOBS 16
#define SR_SUM_MAX_VIEWS 16
typedef struct SrSumJob {
    float* dst;
    const float* src;
    long long elems;
    long long view_stride;   /* in floats */
} SrSumJob;
int sr_sum_views(int n_jobs, const SrSumJob* jobs, int n_views, void* hip_stream);

/* Backward of both stages.  dL_ddepth / dL_dalpha may be NULL (treated as zero).  `instances` is the capacity the binning
 * buffer was rendered with; `scratch` holds sr_backward_scratch_bytes(instances) bytes.
 * `instances_rendered`: the instance count the forward reported for these buffers (*instances_out), or -1 if the caller did
 * not keep it.  It only selects a variant of the per-splat reduction (fewer than SR_BWD_SLOT_SPEC_BELOW instances per splat on
 * average, or unknown: a splat's first gradient slots are requested together with their `reached` bytes); the results are the
 * same.  (Rounds 2-5 also switched the backward BLEND kernel on it; since round 6 the entry-per-lane kernel -- quad buckets,
 * DPP scans: blend_bwd.hip -- runs at every footprint, and the pixel-per-lane kernel of render.hip is kept as a second
 * implementation of the same gradient slots: sr_set_backward_kernel.)
 * `binning` is NOT const: the backward blend sets, inside it, one `reached` byte per tile-splat instance it wrote a gradient
 * slot for (the forward's scatter cleared them), and the per-splat reduction reads them back.  Consequences for callers:
 * ONE backward at a time per set of forward buffers (two concurrent backwards on the same buffers -- different streams or
 * host threads -- race on those bytes), a backward may be REPEATED on the same buffers (it sets the same bytes again:
 * `retain_graph=True` works), and a copy of the binning buffer taken before a backward is a valid input of another one. */
#define SR_BWD_SLOT_SPEC_BELOW 6
int sr_backward(const SrView* view, const SrSplats* splats, const void* geom, void* binning,
                long long instances, long long instances_rendered, const void* image, const int* radii,
                const float* dL_dcolor, const float* dL_ddepth, const float* dL_dalpha, void* scratch,
                const SrGrads* grads, void* hip_stream);

/* sr_backward in two calls, for callers that overlap an exchange of finished gradients with the rest of the backward (the
 * view-parallel training step, splatfields_amd/view_parallel.py; no counterpart in [EXT], which is single-GPU):
 *   sr_backward_blend   -- the backward blend only: fills `scratch` (one gradient slot per reached tile-splat instance);
 *   sr_backward_splats  -- the per-splat part (slot reduction + chain rule to means3D / scales / rotations / SH / opacity)
 *                          for splats [first_splat, first_splat + n_splats) only; first_splat must be a multiple of 256;
 *                          the SrGrads pointers are the bases of the FULL gradient tensors (rows outside the range are not
 *                          touched).  Any partition of [0, count) into such ranges, in any order, after one
 *                          sr_backward_blend, gives exactly what sr_backward gives (same kernels, same arithmetic per splat).
 * Same buffers and the same `instances` / `instances_rendered` meaning as sr_backward (the per-splat kernel has a variant for
 * small footprints too: it requests a splat's first gradient slots together with their `reached` bytes). */
int sr_backward_blend(const SrView* view, const SrSplats* splats, const void* geom, void* binning,
                      long long instances, long long instances_rendered, const void* image,
                      const float* dL_dcolor, const float* dL_ddepth, const float* dL_dalpha, void* scratch, void* hip_stream);
int sr_backward_splats(const SrView* view, const SrSplats* splats, const void* geom, void* binning,
                       long long instances, long long instances_rendered, const void* image, const int* radii, void* scratch,
                       const SrGrads* grads, int first_splat, int n_splats, void* hip_stream);

/* Pins the backward blend kernel for A/B measurements and for the test that compares the two: 0 = the product choice (default;
 * the entry-per-lane kernel at every footprint, see sr_backward), 1 = pixel-per-lane kernel, 2 = entry-per-lane kernel.  The initial value comes from the environment
 * variable SPLATRASTER_BWD ("wave" = 1, "quads" = 2), read once when the library is loaded.  Process-wide; returns the
 * previous setting, or -1 for an unknown value (nothing changes). */
int sr_set_backward_kernel(int which);

/* Who sorts the tile lists of up to 4096 entries, for A/B measurements and for the tests that compare the paths: 0 = the product
 * choice (default): the workgroup of the forward blend that blends the list sorts it first, inside the same launch -- lists of
 * up to 2048 entries always, lists of 2049..4096 entries on views that have at most 8 tiles that long and nothing longer (other
 * views keep the separate launch of that class); 1 = standalone kernels in launches of their own in front of the forward blend;
 * 2 = the forward blend sorts the lists of up to 2048 entries only.  Lists, images and gradients are bit-identical.
 * The initial value comes from the environment variable SPLATRASTER_SORT ("standalone" = 1, "short" = 2), read once when the
 * library is loaded.  Process-wide; applies to forwards launched afterwards; returns the previous setting, or -1 for an unknown value
 * (nothing changes). */
int sr_set_sort_kernel(int which);

/* present[i] = 1 iff splat i passes the near-plane test (view z > 0.2). */
int sr_mark_visible(int n_splats, const float* means3D, const float* viewmatrix,
                    const float* projmatrix, unsigned char* present, void* hip_stream);

/* The per-view densification bookkeeping that consumes the rasterizer's outputs (reference train.py:280-286 and
 * scene/gaussian_model.py:427-438, `add_densification_stats`), for the splats with radii > 0 (`visibility_filter`), fused:
 *   grad_accum[i] += |dL_dmeans2D[i, :2]|;   denom[i] += 1;   max_radii2D[i] = max(max_radii2D[i], radii[i]).
 * The reference does this with boolean-mask indexing (several kernels and a host synchronisation per iteration).
 * Any of the three outputs may be NULL. */
int sr_densification_stats(int n_splats, const float* dL_dmeans2D, const int* radii, float* grad_accum, float* denom,
                           float* max_radii2D, void* hip_stream);

/* The photometric loss of a training step (reference train.py:183-193, utils/loss_utils.py:18 and :33-76), fused:
 *   l1 = mean|image - gt|;   ssim[b] = mean over item b of the structural similarity map (11-tap Gaussian window, sigma 1.5,
 *   float32 taps, zero padding of 5, C1 = 0.01^2, C2 = 0.03^2);   mask_l1 = mean|clamp(alpha, 0, 1) - gt_mask|;
 *   loss = (1 - lambda_dssim) l1 + lambda_dssim (1 - mean_b ssim[b]) + lambda_mask mask_l1.
 * image, gt: [batch, channels, height, width] float32; alpha, gt_mask: [batch, height, width] (both or neither).  Any size
 * >= 1: a plane smaller than the window is an ordinary case.  All four results are written to device memory (ssim: `batch`
 * floats); nothing is read back and nothing waits: both calls only enqueue on `hip_stream`.
 * `workspace`: sr_loss_workspace_bytes(batch * channels, height, width) bytes, the per-workgroup partial sums, which one
 * workgroup adds in a fixed order (no floating-point atomics: results are bit-identical from call to call).
 * `maps`: NULL, or sr_loss_maps_bytes(batch * channels, height, width) bytes that receive the three per-pixel derivative
 * maps sr_photometric_backward reads.  `ssim` may be NULL when lambda_dssim = 0 and maps = NULL: the window is then skipped.
 *
 * sr_photometric_backward writes, with g = upstream[upstream_per_item ? b : 0] read on the device,
 *   dL_dimage = g (w_l1 d l1/d image + w_ssim d ssim/d image),   dL_dalpha (may be NULL) = g w_mask d mask_l1/d alpha,
 * where `ssim` is the mean over all items, or item b's own with upstream_per_item.  The loss above is w_l1 = 1 - lambda_dssim,
 * w_ssim = -lambda_dssim, w_mask = lambda_mask.  sign(0) = 0; clamp passes the gradient for 0 <= alpha <= 1.
 * `maps` may be NULL when w_ssim = 0. */
size_t sr_loss_workspace_bytes(int planes, int height, int width);
size_t sr_loss_maps_bytes(int planes, int height, int width);
int sr_photometric_forward(int batch, int channels, int height, int width, const float* image, const float* gt,
                           const float* alpha, const float* gt_mask, float lambda_dssim, float lambda_mask, void* workspace,
                           float* maps, float* loss, float* l1, float* ssim, float* mask_l1, void* hip_stream);
int sr_photometric_backward(int batch, int channels, int height, int width, const float* image, const float* gt,
                            const float* alpha, const float* gt_mask, const float* maps, float w_l1, float w_ssim, float w_mask,
                            const float* upstream, int upstream_per_item, float* dL_dimage, float* dL_dalpha, void* hip_stream);

/* Evaluation metrics of a batch of views (reference render.py:33-160 `compute_psnr` / `compute_ssim` with its defaults,
 * utils/image_utils.py `psnr`), forward only.  pred, gt: `batch` RGB images of height x width float32, addressed by ELEMENT
 * strides {item, channel, row, pixel}: [B,3,H,W] renders and [B,H,W,3] images both go in without a copy.  height, width >= 11.
 * `quantize` is applied to both images first:
 *   SR_QUANT_NONE  as given;
 *   SR_QUANT_PNG   trunc(clamp(x 255 + 0.5, 0, 255)) / 255: torchvision `save_image`, then the `/255.` of `eval_imgs`;
 *   SR_QUANT_TO8B  trunc(255 clamp(x, 0, 1)) / 255: `to8b` of render.py:282.
 * `mask`: NULL, or float32 [height, width] per item, rows contiguous, `mask_item_stride` elements apart (0: one mask for
 * every item), read as mask != 0.  It selects the reference's two-stage partial convolution (count-normalised per pass);
 * a window without a mask pixel scores exactly 1 and is counted.  The squared error is never masked.
 * Written, all to device memory:  psnr[b] = -10/ln10 ln(mse_b);  ssim[b] = mean of the (height-10) x (width-10) x 3 similarity
 * map (11-tap "valid" window, sigma 1.5, float32 taps, clipped variances);  psnr_channels[b,c] = 20 log10(1/sqrt(mse_bc));
 * `frames` (may be NULL; needs a quantisation): uint8 [batch, height, width, 3], the quantised prediction.
 * Identical images give psnr = +inf.  `workspace`: sr_metrics_workspace_bytes(batch, height, width) bytes (0 for a shape
 * out of range), the per-workgroup partial sums in double, which one workgroup adds in a fixed order: no floating-point
 * atomics, results bit-identical from call to call.  The call only enqueues on `hip_stream`; nothing waits. */
#define SR_QUANT_NONE 0
#define SR_QUANT_PNG 1
#define SR_QUANT_TO8B 2
size_t sr_metrics_workspace_bytes(int batch, int height, int width);
int sr_image_metrics(int batch, int height, int width, const float* pred, const long long* pred_strides4, const float* gt,
                     const long long* gt_strides4, const float* mask, long long mask_item_stride, int quantize, void* workspace,
                     float* psnr, float* ssim, float* psnr_channels, unsigned char* frames, void* hip_stream);

/* LPIPS (VGG) of a batch of image pairs, forward only, float32 throughout (exact f32-input MFMA): the published `lpips` package
 * v0.1, net='vgg', spatial=False, eval mode, restated from its published behaviour, with weights the caller supplies:
 *   x' = ((2 q(x) - 1) - shift_c) / scale_c, q the quantisation `quantize` (SR_QUANT_*) as in sr_image_metrics;
 *   13 convolutions 3x3, padding 1, bias, ReLU, of widths 64,64 | 128,128 | 256,256,256 | 512,512,512 | 512,512,512, a 2x2 /
 *   stride-2 max-pool (floor) between the groups;  taps = the output of the last convolution of each group;
 *   tap_l = mean over the tap's pixels of sum_c lin_l[c] (f0 / (sqrt(sum_c f0^2) + 1e-10) - f1 / (sqrt(sum_c f1^2) + 1e-10))^2;
 *   out[b] = sum of the five taps of pair b.
 * sr_lpips_pack_weights: `conv_weights` / `conv_biases` are HOST arrays of SR_LPIPS_CONVS device pointers ([cout,cin,3,3] and
 *   [cout], contiguous float32), `lins` a host array of SR_LPIPS_TAPS device pointers ([64], [128], [256], [512], [512]),
 *   `shift`, `scale` device [3].  Writes the kernels' layout into `packed`: sr_lpips_packed_bytes() bytes of device memory,
 *   256-byte aligned.  Once per set of weights, not per call.
 * sr_lpips_forward: pred, gt as for sr_image_metrics (element strides {item, channel, row, pixel}), in [0,1].  Limits:
 *   16 <= height, width <= 32768 (below 16 relu5_3 has no pixel), and 2 batch ceil(height / 8) ceil(width / 16) as well as
 *   batch ceil(height width / 64) at most 2^31 - 1; anything else is refused before any launch.  `workspace`:
 *   sr_lpips_workspace_bytes(batch, height, width) bytes (0 for a shape out of range), 256-byte aligned: two activation
 *   buffers of 2 batch height width 64 floats, the pooled buffer, the per-workgroup partial sums in double.  Written, all to
 *   device memory: out [batch]; out_taps (may be NULL) [batch, 5]; maps (may be NULL) sr_lpips_maps_floats(batch, height,
 *   width) floats: the five per-pixel maps [batch, height >> l, width >> l], l = 0..4, one after another.
 * 19 launches per call on `hip_stream`, no atomics, nothing waits: results are bit-identical from call to call, and an item's
 * value does not depend on the other items of the batch. */
#define SR_LPIPS_CONVS 13
#define SR_LPIPS_TAPS 5
size_t sr_lpips_packed_bytes(void);
int sr_lpips_pack_weights(const float* const* conv_weights, const float* const* conv_biases, const float* const* lins,
                          const float* shift, const float* scale, void* packed, void* hip_stream);
size_t sr_lpips_workspace_bytes(int batch, int height, int width);
size_t sr_lpips_maps_floats(int batch, int height, int width);
int sr_lpips_forward(int batch, int height, int width, const float* pred, const long long* pred_strides4, const float* gt,
                     const long long* gt_strides4, int quantize, const void* packed, void* workspace, float* out, float* out_taps,
                     float* maps, void* hip_stream);

/* SH colour evaluation as a stand-alone stage (the SH part of the forward preprocess; reference utils/sh_utils.py:57-112,
 * extract_geo.py:40-44): colors[N,3] = max(sum_k basis_k(dir) shs[k] + 0.5, 0), clamped[N] bit c set where channel c was
 * clamped.  Feeding `colors` to sr_forward as colors_precomp gives the same image as passing `shs`. */
int sr_sh_forward(int n_splats, int sh_coeffs, int sh_degree, const float* means3D, const float* shs, const float* campos,
                  float* colors, unsigned char* clamped, void* hip_stream);

/* sr_sh_forward for n_views cameras in one pass over the coefficients (SH-sharded view-parallel step):
 * campos [n_views,3]; colors [n_views,N,3]; keep [n_views,N,3] (may be NULL) = 1 where the channel was not clamped, else 0
 * (the factor that channel's colour gradient gets before sr_sh_backward). */
int sr_sh_forward_views(int n_splats, int sh_coeffs, int sh_degree, int n_views, const float* means3D, const float* shs,
                        const float* campos, float* colors, float* keep, void* hip_stream);

/* Backward of sr_sh_forward for n_views cameras at once (view-parallel training).
 * campos [n_views,3]; dL_dcolors [n_views,N,3], zero where the colour was clamped in that view.
 * dL_dshs [N,K,3] (may be NULL) = scale * sum_v basis(dir_v) (x) dL_dcolors[v];
 * dL_dmeans3D [N,3] (may be NULL) = or += scale * the gradient through the view direction. */
int sr_sh_backward(int n_splats, int sh_coeffs, int sh_degree, int n_views, const float* means3D, const float* shs,
                   const float* campos, const float* dL_dcolors, float scale, float* dL_dshs, float* dL_dmeans3D,
                   int accumulate_means, void* hip_stream);

/* mean_dist2[i] = mean squared distance from point i to its 3 nearest other points (exact k-NN).
 * Replaces [EXT] simple_knn._C.distCUDA2 (reference README.md:29), called once at initialisation by reference
 * scene/gaussian_model.py:105.  `workspace` holds sr_knn_workspace_bytes(n) bytes of device memory.
 * With fewer than 4 points the sum over the neighbours that exist is divided by 3.  A row with a NaN or infinite coordinate,
 * or one whose neighbours' squared distances overflow float32, gets +inf and takes no part in any other row's search. */
size_t sr_knn_workspace_bytes(int n_points);
int sr_knn3_mean_dist2(int n_points, const float* points, float* mean_dist2, void* workspace, void* hip_stream);

/* The K nearest points of every point, itself included (exact; 2 <= k <= SR_KNN_MAX_K <= n_points), nearest first, ordered
 * by (squared distance, index): nn_ix [n,k] int32.  Replaces [EXT] pytorch3d.ops.knn.knn_points(pts, pts, K) of reference
 * extract_geo.py:101-103.  Also written, for the kernels below: order [n] (the points in grid-cell order, by index inside a
 * cell), and the reverse adjacency rev_start [n+1] / rev_edges [n k] -- per point the edges p * k + slot that end there, in
 * ascending order.  `workspace`: sr_knn_graph_workspace_bytes(n, k) bytes (0 = sizes out of range). */
#define SR_KNN_MAX_K 8
size_t sr_knn_graph_workspace_bytes(int n_points, int k);
int sr_knn_graph(int n_points, int k, const float* points, int* nn_ix, unsigned* order, unsigned* rev_start, unsigned* rev_edges,
                 void* workspace, void* hip_stream);

/* Moran's I regulariser (reference extract_geo.py:100-143 as called by train.py:203-215).  Item p has k rows r_a and a k x k
 * matrix c: with `points` [rows,3], r_a = nn_ix[p,a] and c_ab = 1 / |q_a - q_b| where that distance exceeds eps, eps elsewhere
 * and on the diagonal; with `weight` [n,k,k] (exactly one of the two is given), c = weight[p] and r_a = nn_ix ? nn_ix[p,a] :
 * p k + a.  For each of the n_tensors (1 .. SR_MORAN_MAX_TENSORS) feature tensors features[t] [rows, widths[t]]:
 *   m[p,f] = k sum_ab c_ab x_a x_b / (sum_ab c_ab (sum_a x_a^2 + 1e-4)),  x_a = features[t][r_a, f],
 *   mean_t = mean_{p,f} m,  term_t = 1 - clamp(mean_t, 0, 1).
 * sr_moran_forward writes out [1 + 2 n_tensors] = sum_t term_t | term_t | mean_t.  `workspace`: sr_moran_workspace_bytes(n,
 * n_tensors), per-workgroup partial sums added in a fixed order.  `order` (may be NULL) is the order the items are walked in.
 * sr_moran_backward reads `out` and the upstream gradient of out[0] on the device and writes, for every non-NULL
 * dL_dfeatures[t], the gradient of features[t] (zeros where the clamp of term t is shut); dL_dpoints [rows,3] (points given,
 * may be NULL) or dL_dweight [n,k,k] (weight given, may be NULL).  Contributions are stored per edge in `edges`
 * (sr_moran_edges_bytes(n, k, sum of the widths whose dL_dfeatures[t] is not NULL)) and added per row in edge order through rev_start / rev_edges (required with
 * nn_ix; without nn_ix every row has one edge): no floating-point atomics, identical bits from call to call.
 * sr_moran_weights writes `query_nn`'s weights [n,k,k] = c / max(sum c, 1e-5); sr_moran_weights_backward its gradient to
 * the points (`edges`: sr_moran_edges_bytes(n, k, 0)).  With out = NULL sr_moran_backward differentiates sum_t mean_t instead
 * (`morans_measure`: no clamp).  No entry point waits for the device. */
#define SR_MORAN_MAX_TENSORS 8
size_t sr_moran_workspace_bytes(int n_items, int n_tensors);
size_t sr_moran_edges_bytes(int n_items, int k, int channels);
int sr_moran_forward(int n_items, int k, float eps, const float* points, const float* weight, const int* nn_ix,
                     const unsigned* order, int n_tensors, const float* const* features, const int* widths, void* workspace,
                     float* out, void* hip_stream);
int sr_moran_backward(int n_items, int k, float eps, const float* points, const float* weight, const int* nn_ix,
                      const unsigned* order, const unsigned* rev_start, const unsigned* rev_edges, int n_tensors,
                      const float* const* features, const int* widths, const float* out, const float* upstream, void* edges,
                      float* const* dL_dfeatures, float* dL_dpoints, float* dL_dweight, void* hip_stream);
int sr_moran_weights(int n_points, int k, float eps, const float* points, const int* nn_ix, float* weights, void* hip_stream);
int sr_moran_weights_backward(int n_points, int k, float eps, const float* points, const int* nn_ix, const unsigned* rev_start,
                              const unsigned* rev_edges, const float* dL_dweights, void* edges, float* dL_dpoints,
                              void* hip_stream);

/* The splat regularisers of the training objective, for means3D [n,3] and the opacities [n] (the reference's [n,1] tensor):
 *   norm        = mean_i |x_i|                                      reference train.py:195-197 (`lambda_norm`)
 *   norm_mean   = mean_i |x_i - m|,  m = mean_i x_i, detached        reference train.py:198-201 (`lambda_norm_mean`); m is rounded
 *                                                                   to float32 before the subtraction, as the float32 `mean` is
 *   opacity_reg = mean_i (o_i - 1)^2                                reference train.py:244-246 (`lambda_opacity`)
 *   loss        = lambda_norm norm + lambda_norm_mean norm_mean + lambda_opacity opacity_reg.
 * A term whose weight is 0 is skipped: it is neither computed nor read (its tensor may be NULL) and is written as 0.
 * sr_splat_reg_forward writes out[8] = loss | norm | norm_mean | opacity_reg | m (three floats) | 0 to device memory.
 * `workspace`: sr_splat_reg_workspace_bytes(n) bytes (0 for n <= 0), the per-workgroup partial sums in double, which one
 * workgroup adds in an order the shape alone fixes.  Launches: 2, or 3 with the centred norm (the mean comes before its pass).
 * sr_splat_reg_backward, one launch, writes with g = *upstream read on the device and m = out[4..6] of the forward
 *   dL_dmeans3D[i] (may be NULL) = g / n (lambda_norm x_i / |x_i| + lambda_norm_mean (x_i - m) / |x_i - m|),
 *   dL_dopacity[i] (may be NULL) = g lambda_opacity 2 (o_i - 1) / n;
 * a vector of length 0 contributes exactly 0 (torch's `norm` backward).  `out` may be NULL when lambda_norm_mean = 0.
 * Every row is evaluated in double from its float32 inputs with the IEEE square root and division and rounded to float32 once
 * where it is stored.  All tensors are contiguous and 4-byte aligned; means3D moves as 16-byte vectors over the flat array for
 * any such base (a slice with a storage offset included), the opacities and a gradient where their address agrees with the
 * rows' modulo 16, element by element where not.  n = 0 is valid and launches nothing.  No floating-point atomics, nothing
 * waits for the device: identical bits from call to call. */
size_t sr_splat_reg_workspace_bytes(int n_splats);
int sr_splat_reg_forward(int n_splats, const float* means3D, const float* opacity, double lambda_norm, double lambda_norm_mean,
                         double lambda_opacity, void* workspace, float* out, void* hip_stream);
int sr_splat_reg_backward(int n_splats, const float* means3D, const float* opacity, double lambda_norm, double lambda_norm_mean,
                          double lambda_opacity, const float* out, const float* upstream, float* dL_dmeans3D, float* dL_dopacity,
                          void* hip_stream);

/* Depth L1 (reference train.py:224-229, `lambda_depthl1`): for depth, gt_depth [batch, height, width] float32, contiguous,
 *   valid = gt_depth > 0,   depth_l1 = mean over ALL batch height width elements of |depth valid - gt_depth valid|
 * (`F.l1_loss` divides by every element, the masked ones included).  Inputs are assumed finite.
 * sr_depth_l1_forward writes out[1 + batch] = the mean over everything | the mean over each item.  `workspace`:
 * sr_depth_l1_workspace_bytes(batch, height, width) bytes (0 for a shape out of range or an empty batch).  2 launches.
 * sr_depth_l1_backward, one launch, writes dL_ddepth = g sign(depth - gt_depth) valid / (batch height width), sign(0) = 0,
 * g = upstream[0]; with upstream_per_item, g = upstream[b] and the divisor is height width: the gradient of sum_b g_b item_b.
 * batch = 0 is valid and launches nothing; a non-positive image size is an error.  4-byte aligned bases; 16-byte vectors
 * wherever the tensors agree modulo 16.  No floating-point atomics, nothing waits for the device. */
size_t sr_depth_l1_workspace_bytes(int batch, int height, int width);
int sr_depth_l1_forward(int batch, int height, int width, const float* depth, const float* gt_depth, void* workspace, float* out,
                        void* hip_stream);
int sr_depth_l1_backward(int batch, int height, int width, const float* depth, const float* gt_depth, const float* upstream,
                         int upstream_per_item, float* dL_ddepth, void* hip_stream);

/* Densification / pruning of the splat set on the device: reference scene/gaussian_model.py:411-425 (`densify_and_prune`) with
 * :394-409 (`densify_and_clone`), :355-380 (`densify_and_split`, N = 2), :306-353 (`densification_postfix`) and :272-304
 * (`prune_points`), planned together.  Inputs are the optimiser's RAW parameters (log-scales [N,1|3], opacity logits [N]) and
 * the densification statistics (`xyz_gradient_accum` [N], `denom` [N], `max_radii2D` [N] or NULL = not tested).
 *
 * sr_densify_plan writes dest [4][N] (int32): the row, in the final tensors, of splat i itself (k = 0), of its clone (k = 1)
 * and of its two split children (k = 2, 3), or -1 -- in the order the reference's cat / mask sequence produces:
 * [surviving originals][clones][first children][second children] -- and returns counts5 = rows of each kind + their sum.
 * It synchronises the stream once (the caller needs the new size to allocate).  `workspace`: sr_densify_workspace_bytes(N).
 *
 * sr_densify_gather builds one final tensor from one source tensor of [N, row_floats]:
 *   mode 0  every surviving row is a copy (features, opacity, rotation);
 *   mode 1  Adam moment: the splat's own row is copied, new rows are zero (cat_tensors_to_optimizer);
 *   mode 2  positions [N,3]: children = xyz + build_rotation(rotation) (unit_normal * exp(log_scale)), unit_normals [2][N][3];
 *   mode 3  log-scales: children = log(exp(log_scale) / (0.8 * 2)). */
size_t sr_densify_workspace_bytes(int n_splats);
int sr_densify_plan(int n_splats, const float* log_scales, int scale_cols, const float* opacity_logits, const float* grad_accum,
                    const float* denom, const float* max_radii2D, float grad_threshold, float min_opacity, float extent,
                    float percent_dense, float max_screen_size, void* workspace, int* dest, long long* counts5, void* hip_stream);
int sr_densify_gather(int n_splats, int row_floats, const float* src, float* dst, const int* dest, int mode,
                      const float* log_scales, int scale_cols, const float* rotations, const float* unit_normals,
                      void* hip_stream);

/* The Adam step of a training iteration (reference train.py:314-322; the optimizer is `torch.optim.Adam(l, lr=0.0, eps=1e-15)`
 * over six tensors, scene/gaussian_model.py:130-139): ONE launch updates every tensor of the call.  Per element, in float32
 * with correctly rounded division and square root,
 *   m = m + one_minus_beta1 (g - m);   v = v + one_minus_beta2 (g^2 - v);        (= beta m + (1 - beta) g, weights summing to 1)
 *   p = p - step_size * m / (sqrt(v) / bias_correction2_sqrt + eps).
 * The scalars of a job are computed by the caller in double, as torch.optim.Adam does with capturable=False, and rounded to
 * float32 once:  step_size = lr / (1 - beta1^t),  bias_correction2_sqrt = sqrt(1 - beta2^t),  one_minus_beta = 1 - beta
 * (rounded from the double difference: 1.0f - 0.999f is off by 1.3e-5 of its value).
 * param / grad / exp_avg / exp_avg_sq: `count` contiguous floats each (count <= 2^31 - 1), 4-byte aligned; where the four
 * addresses agree modulo 16 the body moves as 16-byte vectors and only the unaligned head and tail go element by element.
 * `visible` (may be NULL): one byte per row, `rows` of them; every job must then have count == rows * row, and the elements
 * of a row whose byte is 0 are neither read nor changed: parameter and both moments keep their bits (the semantics of a
 * sparse Adam with the global step count in the bias corrections).  `row` is not read without `visible`.
 * n_jobs = 0 and jobs with count = 0 are valid and launch nothing.  No LDS, no atomics, nothing waits for the device. */
#define SR_ADAM_MAX_TENSORS 32
typedef struct SrAdamJob {
    float* param;
    const float* grad;
    float* exp_avg;
    float* exp_avg_sq;
    long long count;
    int row;
    float step_size, bias_correction2_sqrt, one_minus_beta1, one_minus_beta2, eps;
} SrAdamJob;
int sr_adam_step(int n_jobs, const SrAdamJob* jobs, const unsigned char* visible_or_null, long long rows, void* hip_stream);

/* The Adam step of the deform network (reference train.py:318 `deform.optimizer.step()`; scene/deform_model.py:23-34 builds
 * `torch.optim.Adam(l, lr=0.0, eps=1e-15)` over every parameter of the network: 71 to 502 tensors, most of them under 1024
 * elements).  The arithmetic is sr_adam_step's, bit for bit.  What differs is how the job list travels: the addresses of a
 * network's parameters and moments do not change from step to step, so they live in a TABLE IN DEVICE MEMORY that the caller
 * owns and writes once (one SrNetAdamSlot per tensor), and a step passes only what changes -- the range of the table it covers,
 * one set of scalars and the range's gradient pointers -- by value as the kernel argument: no copy, no staging buffer, nothing
 * to reuse too early and no wait.  One launch covers up to SR_NET_ADAM_MAX_GRADS consecutive table entries.
 *
 * Chunking.  A tensor's elements are laid over slots of four floats from the 16-byte boundary at or below `param`; a chunk is 512
 * slots of one tensor; `chunk_end` is the running sum of the chunk counts over the table (entry i owns the chunks
 * chunk_end[i-1] .. chunk_end[i] - 1, a tensor of 0 elements owns none).  It depends on `param` and `count` alone, never on the
 * gradient's address: sr_net_adam_plan (host only, no device) fills it, and sr_net_adam_step refuses a table it disagrees with.
 * Whether a tensor's interior moves as 16-byte vectors (its four addresses agree modulo 16) or element by element is decided in
 * the kernel per step; both give the same bits.
 *
 * sr_net_adam_step: `table_host` and `table_dev` are the same `table_len` records in host and in device memory; the entries
 * first .. first + n - 1 are stepped with `scalars`, entry first + i with the gradient grads_host[i]; a NULL gradient skips that
 * tensor in this launch: its parameter and moments keep their bits.  Everything is validated on the host from `table_host`
 * before the launch: count in 0 .. 2^31 - 1, no NULL and 4-byte alignment of every pointer of a tensor that is stepped (the
 * gradients included), chunk_end as sr_net_adam_plan fills it.  n = 0, a range whose gradients are all NULL and a range whose
 * counts are all 0 launch nothing and succeed without a device.  No LDS, no atomics, nothing waits for the device, and the
 * library keeps no memory of its own. */
#define SR_NET_ADAM_MAX_GRADS 480
typedef struct SrNetAdamSlot {
    float* param;
    float* exp_avg;
    float* exp_avg_sq;
    long long count;
    long long chunk_end;
} SrNetAdamSlot;
typedef struct SrNetAdamScalars {
    float step_size, bias_correction2_sqrt, one_minus_beta1, one_minus_beta2, eps;
} SrNetAdamScalars;
int sr_net_adam_plan(SrNetAdamSlot* table_host, int table_len);
int sr_net_adam_step(const SrNetAdamSlot* table_host, const SrNetAdamSlot* table_dev, int table_len, int first, int n,
                     const float* const* grads_host, const SrNetAdamScalars* scalars, void* hip_stream);

/* Fused MLP chains of the SplatFields deform network's `GeneralMLP`s (reference utils/time_utils.py:123-191; SURVEY.md
 * section 8f row 4): n_points points are carried through a list of OPS in ONE kernel, the running state (<= 16 * hidden_tiles
 * channels per point) in registers, exact fp32 MFMA.  An op applies one packed matrix to [mem_tiles x 16 channels read from
 * `src` (row stride src_row floats, rows 16-byte aligned) | reg_tiles x 16 channels of the running state], starting from
 * `bias` (or 0), and produces out_tiles x 16 channels, which then go through `epilogue`:
 *   SR_MLP_LEAKY  leaky ReLU with negative_slope         -- a forward layer: y = act(W [x0 | h] + b); the reference
 *                 concatenates the skip input IN FRONT of the hidden state, hence memory channels first;
 *   SR_MLP_MASK   times leaky'(.) read off the sign of `mask` (the saved activation of the layer below, row stride mask_row)
 *                 -- a backward step: dZ_below = (W_hidden^T dZ) * act'(.);
 *   SR_MLP_NONE   nothing.
 * The result becomes the new running state unless keep_state != 0, and, if `store` is set, its first store_channels
 * channels are written to (store_accumulate: added to) store[point * store_row + channel]: the saved activations / output
 * of the forward, the dZ of every layer (for the weight-gradient GEMMs) and dL/dx0 of the backward.  hidden_tiles = 4 or 8
 * bounds out_tiles and reg_tiles; tile counts of the inputs are even.  Matrices arrive packed for the MFMA K order (layout:
 * csrc/mlp.hip header; packer: splatfields_amd/fused_mlp.py), biases padded to 16 * out_tiles floats.  Host side that builds
 * the forward and backward op lists of a GeneralMLP: splatfields_amd/fused_mlp.py. */
#define SR_MLP_MAX_OPS 24
#define SR_MLP_NONE 0
#define SR_MLP_LEAKY 1
#define SR_MLP_MASK 2
typedef struct SrMlpOp {
    const float* w_packed;
    const float* bias;         /* may be null */
    const float* src;          /* memory input channels (mem_tiles > 0) */
    const float* mask;         /* SR_MLP_MASK */
    float* store;              /* may be null */
    unsigned int* sign_store;  /* may be null: word [point * 4 + k], bit 4 t + i = (result channel 16 t + 4 k + i > 0) */
    const unsigned int* mask_bits; /* SR_MLP_MASK: if set, leaky'(.) comes from these bits (the layout sign_store writes) instead of `mask` */
    int out_tiles;
    int mem_tiles;             /* even */
    int reg_tiles;             /* even */
    int src_row;
    int epilogue;
    int mask_row;
    int store_row;
    int store_channels;
    int store_accumulate;
    int keep_state;
} SrMlpOp;
int sr_mlp_chain(int n_points, int hidden_tiles, int n_ops, const SrMlpOp* ops, float negative_slope, void* hip_stream);

/* Packs matrices for sr_mlp_chain on the device (training repacks every step: the weights change, and ResField layers
 * compose W + delta(frame) per step -- reference utils/resfields.py:378-405).  Job j builds the packed form of the matrix
 *   A[r][c'],  r < 16 * out_tiles,  c' < mem_pad + reg_width:
 *     c' <  mem_pad:  column c = c' of the memory block   (zero unless c < n_mem),  source column mem_col0 + c
 *     c' >= mem_pad:  column c = c' - mem_pad of the register block (zero unless c < n_reg), source column reg_col0 + c
 *   A[r][.] = 0 unless r < n_rows;  element = transposed ? W[column][row0 + r] : W[row0 + r][column],  W row stride `ld`
 * (transposed jobs build the backward's W^T blocks straight from the layer's weight), and, when bias_dst is set, copies
 * n_bias floats of bias_src to bias_dst and zero-fills it up to 16 * out_tiles.  mem_pad and reg_width are multiples of 32 / 16
 * with an even total tile count.  dst holds 16 * out_tiles * (mem_pad + reg_width) floats, 16-byte aligned. */
#define SR_MLP_MAX_PACK_JOBS 32
typedef struct SrMlpPackJob {
    const float* w;
    const float* bias_src;     /* may be null */
    float* dst;
    float* bias_dst;           /* may be null */
    int ld;
    int transposed;
    int row0, n_rows;
    int n_mem, mem_pad, mem_col0;
    int n_reg, reg_width, reg_col0;
    int out_tiles;
    int n_bias;
} SrMlpPackJob;
int sr_mlp_pack(int n_jobs, const SrMlpPackJob* jobs, void* hip_stream);

/* The same chains with bfloat16 matrix operands (opt-in; the fp32 pair above stays the default and is not affected).  With
 * bf(.) = round to nearest even to bfloat16:
 *   forward ops   acc = bias + bf(W) . bf(x)        backward ops   acc = bf(W^T) . bf(dZ)
 * Products and accumulation are fp32 (v_mfma_f32_16x16x32_bf16); the bias is fp32 and the accumulator's initial value; the
 * running state stays fp32 in registers and is rounded only where it becomes an MFMA operand; channels read from `src` are
 * rounded as they are loaded.  Everything stored (saved activations, dZ, y, dL/dx0, accumulating stores), the epilogues and the
 * sign bits are computed from the unrounded fp32 accumulators exactly as by sr_mlp_chain, and results are bit-identical from
 * run to run.  Weight gradients come from sr_mlp_weight_grad on those stored fp32 values, unchanged.
 * sr_mlp_pack_bf16 takes the job table of sr_mlp_pack: `dst` receives 16 * out_tiles * (mem_pad + reg_width) bfloat16 values
 * (16-byte aligned; layout: csrc/mlp.hip), `bias_dst` stays fp32.  sr_mlp_chain_bf16 takes the op table of sr_mlp_chain with
 * `w_packed` pointing at what sr_mlp_pack_bf16 wrote.  Arguments are validated as by the fp32 entry points. */
int sr_mlp_pack_bf16(int n_jobs, const SrMlpPackJob* jobs, void* hip_stream);
int sr_mlp_chain_bf16(int n_points, int hidden_tiles, int n_ops, const SrMlpOp* ops, float negative_slope, void* hip_stream);

/* The same chains with split-bfloat16 matrix operands, "bf16x3" (opt-in).  Every operand v is split into hi(v) = bf(v) and
 * lo(v) = bf(v - hi(v)) (the fp32 subtraction is exact) and a product spends three bf16 MFMAs, lo . lo is dropped:
 *   forward ops   acc = bias + hi(W) . hi(x) + hi(W) . lo(x) + lo(W) . hi(x)
 *   backward ops  acc = hi(W^T) . hi(dZ) + hi(W^T) . lo(dZ) + lo(W^T) . hi(dZ)
 * About 16 significant bits per operand instead of 8.  The three MFMAs of one (chunk, output tile, point tile) go into the same
 * fp32 accumulator in that order; everything outside the MFMA is as for sr_mlp_chain_bf16 (fp32 bias, state, epilogues, sign bits
 * and stores; the state is split once per op and state tile, channels read from `src` as they are loaded); results are
 * bit-identical from run to run.  A non-finite operand has lo = NaN, a finite one that bfloat16 rounds to +-inf has lo = -+inf: what
 * such an operand reaches is not finite.
 * sr_mlp_pack_bf16x3 takes the job table of sr_mlp_pack: `dst` receives 2 * 16 * out_tiles * (mem_pad + reg_width) bfloat16 values
 * (4 bytes per weight; 16-byte aligned; per 32-column chunk the hi block, then the lo block, each in the layout of
 * sr_mlp_pack_bf16: csrc/mlp.hip), `bias_dst` stays fp32.  sr_mlp_chain_bf16x3 takes the op table of sr_mlp_chain with `w_packed`
 * pointing at what sr_mlp_pack_bf16x3 wrote.  Arguments are validated as by the fp32 entry points. */
int sr_mlp_pack_bf16x3(int n_jobs, const SrMlpPackJob* jobs, void* hip_stream);
int sr_mlp_chain_bf16x3(int n_points, int hidden_tiles, int n_ops, const SrMlpOp* ops, float negative_slope, void* hip_stream);

/* Several networks of the SAME hidden width over the SAME points in one launch (the heads of a SplatFields step: reference
 * utils/time_utils.py:466-503 evaluates five GeneralMLPs on one input): net y of `nets` is an op list in the format of
 * sr_mlp_chain, the grid is (ceil(n_points / 128), n_nets) and workgroup (x, y) does for its 128 points exactly what
 * sr_mlp_chain(n_points, hidden_tiles, nets[y].n_ops, nets[y].ops, ...) does for them -- per point and op the same arithmetic in
 * the same order, so every stored value is bit-identical to n_nets separate calls.  What changes is the schedule: the
 * workgroups of net y + 1 start in the tail of net y's last round of resident workgroups.  Nets may differ in depth, skips and
 * output tiles.  At most SR_MLP_GROUP_MAX_NETS nets and SR_MLP_GROUP_MAX_OPS ops in total (the table is a kernel argument:
 * < 4 KB); every op is validated as by sr_mlp_chain.  n_points == 0 or n_nets == 0: nothing is launched, success.
 * sr_mlp_chain_group_bf16: the same for sr_mlp_chain_bf16; sr_mlp_chain_group_bf16x3: for sr_mlp_chain_bf16x3. */
#define SR_MLP_GROUP_MAX_NETS 8
#define SR_MLP_GROUP_MAX_OPS 40
typedef struct SrMlpNet {
    const SrMlpOp* ops;
    int n_ops;
} SrMlpNet;
int sr_mlp_chain_group(int n_points, int hidden_tiles, int n_nets, const SrMlpNet* nets, float negative_slope, void* hip_stream);
int sr_mlp_chain_group_bf16(int n_points, int hidden_tiles, int n_nets, const SrMlpNet* nets, float negative_slope, void* hip_stream);
int sr_mlp_chain_group_bf16x3(int n_points, int hidden_tiles, int n_nets, const SrMlpNet* nets, float negative_slope, void* hip_stream);

/* Weight and bias gradients of the layers of a fused MLP: for every job
 *   dw[m * dw_row + dw_col0 + c] = sum over points p of dz[p * dz_row + m] * x[p * x_row + c],   m < job.m, c < job.k
 *   db[m]                        = sum over points p of dz[p * dz_row + m]                       (when db is set)
 * -- dW_l = dZ_l^T [h_in | h_{l-1}] as one job per column block, all layers of the network in ONE launch: the contraction
 * runs over the 10^5 points and the result is tiny, which library GEMMs serialise (csrc/mlp.hip).  dz and x rows are 16-byte
 * aligned with row strides that are multiples of 4 floats; entries of a row beyond m / k up to the row stride may hold
 * anything finite or not (they only reach results that are dropped).  Results are written, not accumulated; the sum over the
 * points has a fixed order (deterministic).  `workspace`: sr_mlp_weight_grad_workspace(...) bytes, 16-byte aligned. */
#define SR_MLP_MAX_GRAD_JOBS 16
#define SR_MLP_MAX_GRAD_TASKS 128      /* 64 x 64 blocks over all jobs */
typedef struct SrMlpGradJob {
    const float* dz;
    const float* x;
    float* dw;
    float* db;                 /* may be null */
    int dz_row, m;
    int x_row, k;
    int dw_row, dw_col0;
} SrMlpGradJob;
size_t sr_mlp_weight_grad_workspace(int n_points, int n_jobs, const SrMlpGradJob* jobs);   /* 0 for an unsupported job list */
int sr_mlp_weight_grad(int n_points, int n_jobs, const SrMlpGradJob* jobs, void* workspace, size_t workspace_bytes, void* hip_stream);

/* Input matrix of a GeneralMLP (reference utils/time_utils.py:9-57 `get_embedder`, :178-181): row p of x0 [N, row] =
 * [ x (3) | sin(2^0 x) | cos(2^0 x) | ... | sin(2^(L-1) x) | cos(2^(L-1) x) | features (n_features) | time encoding | zeros up to `row` ],
 * the layout sr_mlp_chain reads; `row` a multiple of 4 (the fused MLP pads to 32).  `time` (may be NULL): one value per point,
 * encoded as [ t | sin(2^0 t) | cos(2^0 t) | ... | sin(2^(TL-1) t) | cos(2^(TL-1) t) ], TL = time_multires -- the time embedding the
 * reference appends to the features of every network (utils/time_utils.py:455-456); it receives no gradient.  Backward: given
 * dL/dx0, d_xyz = g[0:3] + sum_j 2^j (cos(2^j x) g_sin_j - sin(2^j x) g_cos_j) and d_features = the feature columns of g
 * (either may be NULL). */
int sr_mlp_input_forward(int n_points, int multires, int n_features, int time_multires, int row, const float* xyz, const float* features,
                         const float* time, float* x0, void* hip_stream);
int sr_mlp_input_backward(int n_points, int multires, int n_features, int row, const float* xyz, const float* dL_dx0, float* dL_dxyz,
                          float* dL_dfeatures, void* hip_stream);
/* Top of the backward of a GeneralMLP (the activation follows EVERY layer, the last one included: reference
 * utils/time_utils.py:178-191): g[p][c] = dL_dy[p][c] * (y[p][c] > 0 ? 1 : negative_slope) for c < out_features, 0 for
 * out_features <= c < row -- the padded matrix the backward chain's first op and the last layer's weight gradient read. */
int sr_mlp_top_gradient(int n_points, int out_features, int row, const float* y, const float* dL_dy, float negative_slope, float* g,
                        void* hip_stream);

/* The same three steps for ALL heads of a step in one launch each (job tables; <= SR_MLP_GROUP_MAX_HEADS heads), around
 * sr_mlp_chain_group.  Pointwise arithmetic is in double with one rounding per stored value; no atomics, no host wait, 64-bit
 * row offsets, bit-identical from run to run.  n_points == 0 or n_heads == 0: nothing is launched, success.
 *   sr_mlp_group_input_forward   x0 of every head (its own `multires` and `row`, layout of sr_mlp_input_forward) from one
 *                                xyz / features / time.
 *   sr_mlp_group_input_backward  dL_dxyz [N, 3] and dL_dfeatures [N, n_features] (either may be NULL), WRITTEN once: the sum over
 *                                the heads, in table order, of what sr_mlp_input_backward computes from each head's dL_dx0.
 *   sr_mlp_group_output          out = act(y) per head: SR_MLP_OUT_SIGMOID 1 / (1 + exp(-y)), SR_MLP_OUT_NORMALIZE
 *                                y / max(|y|, 1e-12) over the row (SR_MLP_OUT_NONE is a copy; a caller may leave such a head out).
 *   sr_mlp_group_top_gradient    g [N, row] = dL_dout o act'(.) o leaky'(y), zero-padded to `row` (the matrix sr_mlp_top_gradient
 *                                writes, with the output activation's backward folded in): sigmoid s (1 - s), s = sigmoid(y);
 *                                normalize (n = |y|, u = y / max(n, 1e-12)): (n > 1e-12 ? d - u (d . u) : d) / max(n, 1e-12);
 *                                a head with dL_dout == NULL gets g = 0. */
#define SR_MLP_GROUP_MAX_HEADS 8
#define SR_MLP_OUT_NONE 0
#define SR_MLP_OUT_SIGMOID 1
#define SR_MLP_OUT_NORMALIZE 2
typedef struct SrMlpHeadInput {
    float* x0;                 /* forward: [N, row], 16-byte aligned */
    const float* dL_dx0;       /* backward: [N, row] */
    int multires;              /* 0 .. 16 */
    int row;                   /* multiple of 4, >= the width of the head's input */
} SrMlpHeadInput;
typedef struct SrMlpHeadOutput {
    const float* y;            /* [N, out_features]: the chain's output */
    float* out;                /* sr_mlp_group_output: [N, out_features] */
    const float* dL_dout;      /* sr_mlp_group_top_gradient: [N, out_features] or NULL (no gradient reached this head) */
    float* g;                  /* sr_mlp_group_top_gradient: [N, row], 16-byte aligned */
    int out_features;          /* 1 .. 128 */
    int row;                   /* multiple of 4, >= out_features */
    int activation;            /* SR_MLP_OUT_* */
    int reserved;
} SrMlpHeadOutput;
int sr_mlp_group_input_forward(int n_points, int n_heads, const SrMlpHeadInput* heads, int n_features, int time_multires, const float* xyz,
                               const float* features, const float* time, void* hip_stream);
int sr_mlp_group_input_backward(int n_points, int n_heads, const SrMlpHeadInput* heads, int n_features, const float* xyz, float* dL_dxyz,
                                float* dL_dfeatures, void* hip_stream);
int sr_mlp_group_output(int n_points, int n_heads, const SrMlpHeadOutput* heads, void* hip_stream);
int sr_mlp_group_top_gradient(int n_points, int n_heads, const SrMlpHeadOutput* heads, float negative_slope, void* hip_stream);

/* ResField weights of the current frame for all layers of one network in one launch (reference utils/resfields.py:185,229,
 * 294-300,378-405 in the configuration GeneralMLP builds -- compression 'vm', mode 'lookup', fuse 'add'):
 *   out[j] = w[j] + sum_k weights_t[frame * rank + k] * matrix_t[k * count + j],   j < count = out_features * in_features.
 * `frame` points at an int64 on the device (the reference derives frame_id on the device: no host synchronisation).
 * Backward, given d_out = dL/d out: d_matrix_t[k * count + j] = weights_t[frame * rank + k] * d_out[j];
 * d_weights_t [capacity, rank] = 0 except row `frame` = matrix_t . d_out (summed in a fixed order); dL/dw = d_out itself.
 * count a multiple of 4, 16-byte aligned arrays, rank <= SR_RESFIELD_MAX_RANK. */
#define SR_RESFIELD_MAX_JOBS 16
#define SR_RESFIELD_MAX_RANK 64
typedef struct SrResFieldJob {
    const float* w; const float* weights_t; const float* matrix_t; float* out;    /* forward */
    const float* d_out; float* d_matrix_t; float* d_weights_t;                     /* backward (either output may be NULL) */
    int count, rank, capacity;
} SrResFieldJob;
int sr_resfield_compose(int n_jobs, const SrResFieldJob* jobs, const long long* frame, void* hip_stream);
size_t sr_resfield_backward_workspace(int n_jobs, const SrResFieldJob* jobs);     /* 0 for an unsupported job list */
int sr_resfield_backward(int n_jobs, const SrResFieldJob* jobs, const long long* frame, void* workspace, size_t workspace_bytes,
                         void* hip_stream);

/* Tri-plane feature lookup of the deform network's encoder -- the per-point half of the reference's VarTriPlaneEncoder.forward
 * (scene/tripFields.py:430-436): F.grid_sample (bilinear, zero padding, align_corners = False) of three planes [3, C, H, W] at
 * the (x, y), (y, z), (z, x) projections of the points, features concatenated plane-major: out [N, 3 C].  C a multiple of 4.
 * The plane generator (the reference's diffusers-based decoder, :176-204) is the caller's; it hands over `planes`.
 * `planes_texel_major` [3, H, W, C] is written by the forward (a transposed copy: a corner becomes C contiguous floats) and
 * read again by the backward.
 * Backward: dL_dpoints [N, 3] (gather) and / or dL_dplanes [3, C, H, W] (either may be NULL).  The plane gradient is
 * accumulated in 64-bit fixed point with integer atomics -- bit-reproducible, no floating-point atomics: the (point, plane)
 * pairs are binned by tile of the plane and every tile is summed in LDS by one workgroup; `workspace` holds
 * sr_triplane_backward_workspace(N, C, H, W) bytes (tile counters and the binned lists; needed only with dL_dplanes; 0 for
 * unsupported sizes: C a multiple of 4, <= 128).  The limit of 128 channels is the plane gradient's (its LDS tile): the
 * forward and a backward with dL_dpoints alone take any multiple of 4. */
size_t sr_triplane_backward_workspace(int n_points, int channels, int height, int width);
int sr_triplane_forward(int n_points, int channels, int height, int width, const float* planes, float* planes_texel_major,
                        const float* points, float* out, void* hip_stream);
int sr_triplane_backward(int n_points, int channels, int height, int width, const float* planes_texel_major, const float* points,
                         const float* dL_dout, float* dL_dplanes, float* dL_dpoints, void* workspace, void* hip_stream);

/* Plane generator -- the other half of the reference's VarTriPlaneEncoder: the CNN decoder that turns a fixed noise map into a
 * plane on every step (`Tensorial2D` around `TimeVAEDecoder`, scene/tripFields.py:176-204, scene/time_decoders.py).  Its
 * convolution stack is GroupNorm -> SiLU -> [nearest x2] -> 3x3 convolution -> [+ residual]; every layer of it is one
 * sr_conv3x3_forward, and every plane of the encoder goes through the SAME launch: the entry points take a job table with one
 * row per plane (shapes are shared, pointers are per plane).  All tensors are fp32 NCHW without the batch dimension, contiguous.
 * Matrix products run on v_mfma_f32_16x16x4_f32; there are no floating-point atomics, every sum across workgroups goes
 * through partials in the caller's workspace that are added in a fixed order (bit-identical from call to call); nothing waits
 * on the host.  sr_profile_collect counts the launches of the forward entries under stage 0 and of the backward entries
 * under stage 6 (one record per kernel launch).
 *
 * Channel counts of a convolution: multiples of 8 in 8..64.  GroupNorm: any `groups` dividing the channel count, channels
 * 1..64.  height * width of the convolution's OUTPUT below 2^24.  Anything else returns nonzero before any launch.
 *
 * One row serves all five entry points; each reads the fields named in its description and ignores the others. */
#define SR_PLANE_MAX_JOBS 8
#define SR_CONV_PROLOGUE 1 /* the convolution's input is SiLU(gamma (x - mean) rstd + beta), recomputed from x and `stats`        */
#define SR_CONV_UPSAMPLE 2 /* ... then upsampled nearest x2: the convolution runs at [2 h_in, 2 w_in]                             */
#define SR_CONV_RESIDUAL 4 /* `residual` [cout, h_out, w_out] is added to the result                                               */
#define SR_CONV_SILU_OUT 8 /* out = SiLU(z), z = convolution + bias + residual; the forward also writes z to `pre`                 */
typedef struct SrPlaneJob {
    const float* x;        /* layer input [cin, h_in, w_in] (for sr_groupnorm_*: [channels, h, w])                               */
    const float* weight;   /* [cout, cin, 3, 3]                                                                                   */
    const float* bias;     /* [cout] or NULL                                                                                      */
    const float* gamma;    /* [cin] GroupNorm weight (SR_CONV_PROLOGUE, sr_groupnorm_silu_backward)                               */
    const float* beta;     /* [cin] GroupNorm bias                                                                                */
    float* stats;          /* [groups, 4]: mean, 1 / sqrt(var + eps), mean_lo (the double mean = mean + mean_lo), 0;
                              written by sr_groupnorm_stats, read by the others                                                   */
    const float* residual; /* [cout, h_out, w_out] (SR_CONV_RESIDUAL)                                                              */
    float* out;            /* [cout, h_out, w_out]                                                                                */
    float* pre;            /* [cout, h_out, w_out] (SR_CONV_SILU_OUT): written by the forward, read by the two backward entries   */
    const float* dy;       /* [cout, h_out, w_out] gradient at `out`                                                              */
    float* dx;             /* sr_conv3x3_backward_data: [cin, h_in, w_in], gradient at the ACTIVATED (not yet upsampled) input;
                              sr_groupnorm_silu_backward reads it as the gradient at the activated tensor                         */
    float* dweight;        /* [cout, cin, 3, 3]                                                                                   */
    float* dbias;          /* [cout] or NULL                                                                                      */
    float* dgamma;         /* [channels]                                                                                          */
    float* dbeta;          /* [channels]                                                                                          */
    float* d_residual;     /* sr_conv3x3_weight_grad with SR_CONV_SILU_OUT: [cout, h_out, w_out] gradient at z (which is the
                              residual's gradient), or NULL                                                                       */
    const float* add;      /* sr_groupnorm_silu_backward: [channels, h, w] added to the result (a residual branch), or NULL       */
    float* dx_out;         /* sr_groupnorm_silu_backward: [channels, h, w] gradient at x                                          */
} SrPlaneJob;

/* stats[g] = (mean, 1 / sqrt(biased variance + eps), mean_lo, 0) over channels / groups * h * w values of x, summed in double.
 * Two launches: per-chunk (mean, M2) partials, then their fixed-order combination.  The workspace is 8-byte aligned.
 * Fields: x, stats. */
size_t sr_groupnorm_stats_workspace(int n_planes, int channels, int groups, int height, int width);   /* 0: unsupported */
int sr_groupnorm_stats(int n_planes, const SrPlaneJob* jobs, int channels, int groups, int height, int width, float eps,
                       void* workspace, void* hip_stream);

/* One fused layer, one launch.  `flags`: SR_CONV_* bits.  The zero padding applies to the activated, upsampled tensor (a border
 * tap contributes 0).  Fields: x, weight, bias, residual, out; gamma, beta, stats with SR_CONV_PROLOGUE; pre with
 * SR_CONV_SILU_OUT. */
int sr_conv3x3_forward(int n_planes, const SrPlaneJob* jobs, int cin, int cout, int h_in, int w_in, int groups, int flags,
                       void* hip_stream);

/* dx = gradient at the activated input of the convolution (before the upsample: the 2x2 blocks are summed in a fixed order).
 * With SR_CONV_SILU_OUT dy is first taken through SiLU'(pre).  One launch.  Fields: dy, weight, dx; pre. */
int sr_conv3x3_backward_data(int n_planes, const SrPlaneJob* jobs, int cin, int cout, int h_in, int w_in, int flags, void* hip_stream);

/* dx_out = gradient at x of a = SiLU(gamma (x - mean) rstd + beta) given dx = gradient at a, (+ add); dgamma, dbeta.  Two
 * launches: per-channel partial sums, then their fixed-order combination and the element-wise pass.
 * A group of at most 1024 values is taken through double arithmetic from x on (mean and variance included, hence `eps`): with
 * few values per group the result is a difference of relative size eps rstd^2 that float statistics do not resolve.
 * The workspace is 8-byte aligned.
 * Fields: dx, x, gamma, beta, stats, add, dx_out, dgamma, dbeta. */
size_t sr_groupnorm_silu_backward_workspace(int n_planes, int channels, int height, int width);
int sr_groupnorm_silu_backward(int n_planes, const SrPlaneJob* jobs, int channels, int groups, int height, int width, float eps,
                               void* workspace, void* hip_stream);

/* dweight, dbias of the layer sr_conv3x3_forward ran with the same shapes and flags; the activated input is recomputed.  Two
 * launches: partials per tile of pixels, then their fixed-order sum.
 * Fields: dy, x, dweight, dbias; gamma, beta, stats with SR_CONV_PROLOGUE; pre, d_residual with SR_CONV_SILU_OUT. */
size_t sr_conv3x3_weight_grad_workspace(int n_planes, int cin, int cout, int h_in, int w_in, int flags);
int sr_conv3x3_weight_grad(int n_planes, const SrPlaneJob* jobs, int cin, int cout, int h_in, int w_in, int groups, int flags,
                           void* workspace, void* hip_stream);

/* The attention layer of the generator's mid block (the `Attention` inside `TimeDecoder.mid_block`, scene/time_decoders.py), for
 * every plane of the encoder in the same launches.  Per plane, with T = height * width tokens of width `channels`:
 *   t = gamma GroupNorm(x) + beta  (no SiLU),   q, k, v = t W^T + b,   P = softmax(q k^T / sqrt(channels))  (one head),
 *   out = x + (P v) Wo^T + bo.
 * Tensors are fp32 and contiguous, activations [channels, height, width], weights [out, in] as nn.Linear holds them.  Every
 * product and sum is a double (the group statistics included: two passes over the group); the softmax subtracts the row
 * maximum; each result is rounded to fp32 once, on store.  No floating-point atomics: the parameter gradients are sums over
 * tokens that go through per-chunk partials in the workspace and are added in an order the shape alone fixes, so repeated calls
 * are bit-identical.  Nothing waits on the host.  sr_profile_collect counts the forward's launches under stage 0 and the
 * backward's under stage 6.
 *
 * channels: a multiple of 8 in 8..64; groups divides channels; 1 <= height * width <= 4096; channels / groups * height * width
 * >= 2 (a group of one value has no variance); 1 <= n_planes <= SR_PLANE_MAX_JOBS.  Anything else returns nonzero before any
 * launch, and the size queries return 0.
 *
 * `saved` is the caller's buffer that carries the forward's intermediates (the statistics, q, k, v, P v and the rows'
 * log-sum-exp, as doubles) to the backward: sr_attention_saved_bytes is the size for the whole call, plane i's part is the
 * i-th of n_planes equal pieces (8-byte aligned), or any buffer of that piece's size. */
typedef struct SrAttentionJob {
    const float* x;      /* [channels, h, w] layer input                                                                          */
    const float* gamma;  /* [channels] GroupNorm weight                                                                           */
    const float* beta;   /* [channels] GroupNorm bias                                                                             */
    float* stats;        /* [groups, 4], written by the forward in sr_groupnorm_stats' format (mean, rstd, mean_lo, 0)            */
    const float* wq;     /* [channels, channels] to_q.weight                                                                      */
    const float* bq;     /* [channels]                                                                                            */
    const float* wk;     /* to_k                                                                                                  */
    const float* bk;
    const float* wv;     /* to_v                                                                                                  */
    const float* bv;
    const float* wo;     /* to_out.0                                                                                              */
    const float* bo;
    float* out;          /* [channels, h, w]                                                                                      */
    void* saved;         /* this plane's piece of the saved buffer: written by the forward, read by the backward                  */
    const float* dy;     /* [channels, h, w] gradient at `out`                                                                    */
    float* dx;           /* [channels, h, w] gradient at x, the residual branch included                                          */
    float* dgamma;       /* [channels]                                                                                            */
    float* dbeta;        /* [channels]                                                                                            */
    float* dwq;          /* [channels, channels]                                                                                  */
    float* dbq;          /* [channels]                                                                                            */
    float* dwk;
    float* dbk;          /* written as zeros: a key bias shifts every score of a row alike, and the softmax does not see it      */
    float* dwv;
    float* dbv;
    float* dwo;
    float* dbo;
} SrAttentionJob;

size_t sr_attention_saved_bytes(int n_planes, int channels, int groups, int height, int width);          /* 0: unsupported */
size_t sr_attention_backward_workspace(int n_planes, int channels, int groups, int height, int width);   /* 0: unsupported */

/* Three launches: the group statistics, the three projections, the streaming softmax with the output projection and the
 * residual.  No workspace.  Fields: x, gamma, beta, stats, wq .. bo, out, saved. */
int sr_attention_forward(int n_planes, const SrAttentionJob* jobs, int channels, int groups, int height, int width, float eps,
                         void* hip_stream);

/* Every gradient of the layer the forward ran on the same fields and `saved`.  Six launches: dO and D per token with the
 * partials of dwo / dbo; dq per block of query rows; dk and dv per block of key rows; the gradient at t with the partials of
 * the other parameter gradients; the partials' fixed-order sums; dx.  The workspace is 8-byte aligned.
 * Fields: x, gamma, beta, wq, wk, wv, wo, saved, dy, dx and the ten parameter gradients. */
int sr_attention_backward(int n_planes, const SrAttentionJob* jobs, int channels, int groups, int height, int width, float eps,
                          void* workspace, void* hip_stream);

/* Visual-hull initialisation (reference scene/dataset_readers.py:1385-1417, :1419-1458, :605-644, :544-588): which voxels of a
 * G^3 grid -- or which points of a list -- fall, in every view, on a pixel of that view's mask.
 *
 * Per view (SrHullView), all in double, in this order of operations, without fused multiply-adds:
 *   h = m [x y z 1]^T (m: 3x4, row-major; each row summed left to right),  u = h0 / h2,  v = h1 / h2   (no test on the sign of h2)
 *   SR_HULL_KRT   un = 2 (u / (W - 1)) - 1,  px = ((un + 1) / 2) (W - 1)   -- grid_sample's round trip with align_corners=True;
 *                 the same for y with H; m is the reference's KRT (:1389)
 *   SR_HULL_NDC   un = u,  px = ((u + 1) W - 1) 0.5 (`ndc2Pix` :515),  py likewise with H; m holds columns 0, 1, 2 of the
 *                 reference's transposed full_proj_transform as rows, so h2 is clip z, not w (:625).  The reference swaps H and W
 *                 in both the scale and the bounds test: this equals it for square images, the only ones it is defined for
 *   the nearest pixel is (rint(px), rint(py)), halves to even; the view keeps the item iff that pixel is inside the image and its
 *   mask byte is non-zero.  SR_HULL_OUTSIDE_CARVE: an item outside the image is carved.  SR_HULL_OUTSIDE_KEEP (:1443,1450): an
 *   item with un or vn outside [-1, 1] is kept by this view.  A non-finite px or py is carved under both.
 * An item survives iff every view keeps it.
 *
 * Items: with `grid` (device, double [3][G]: the coordinate tables of x, y, z, made on the host -- np.linspace -- and uploaded)
 * item i = (iy G + ix) G + iz is the voxel (grid[0][ix], grid[1][iy], grid[2][iz]), the order of np.meshgrid(g, g, g) flattened;
 * with `points` (device, [n_points, 3] float32, or float64 with point_is_double) item i is row i.  Exactly one of the two.
 * `masks`: device, one flat byte buffer of `mask_bytes` bytes (non-zero = inside the silhouette); view k's H x W image starts at
 * its mask_offset, so ragged sizes are fine.  `views`: HOST array of n_views records; it is checked on the host and copied into
 * the workspace through the stream.
 *
 * sr_hull_carve: 2 launches (one lane per item, then one workgroup that orders the workgroup counts); writes the number of
 * survivors to `count_out` (device, int32) and one survivor bit per item into the workspace.  Nothing waits for the device.
 * sr_hull_gather (same items, same workspace, after sr_hull_carve): 1 launch; writes the first `capacity` survivors in item
 * order: indices_out [capacity] int32 (item index) and points_out [capacity, 3] float32 (the coordinates rounded from double);
 * either may be NULL.  A capacity below the count gives an ordered prefix.  No atomics: the same inputs give the same bytes.
 * `workspace`: sr_hull_workspace_bytes(items) bytes, items = G^3 or n_points.
 * Refused on the host, before any launch: n_views outside 1 .. SR_HULL_MAX_VIEWS, G < 1, G^3 or n_points > 2^31 - 1, both or
 * neither of grid and points, H or W < 1, H or W == 1 under SR_HULL_KRT (the normalisation divides by W - 1), an unknown
 * convention or policy, a mask that does not fit into mask_bytes.  n_points = 0 is valid (count 0). */
#define SR_HULL_KRT 0
#define SR_HULL_NDC 1
#define SR_HULL_OUTSIDE_CARVE 0
#define SR_HULL_OUTSIDE_KEEP 1
#define SR_HULL_MAX_VIEWS 1024
typedef struct SrHullView {
    double m[12];              /* 3x4 projection, row-major */
    long long mask_offset;     /* first byte of this view's mask in `masks` */
    int height, width;
    int convention;            /* SR_HULL_KRT / SR_HULL_NDC */
    int outside;               /* SR_HULL_OUTSIDE_CARVE / SR_HULL_OUTSIDE_KEEP */
} SrHullView;
size_t sr_hull_workspace_bytes(long long n_items);
int sr_hull_carve(int n_views, const SrHullView* views, const unsigned char* masks, long long mask_bytes, const double* grid, int G,
                  const void* points, long long n_points, int point_is_double, void* workspace, int* count_out, void* hip_stream);
int sr_hull_gather(const double* grid, int G, const void* points, long long n_points, int point_is_double, const void* workspace,
                   long long capacity, int* indices_out, float* points_out, void* hip_stream);

/* Depth-map initialisation (reference scene/dataset_readers.py:1476-1491 `_gen_3dpoints`, called at :1376 and :1463; its cloud is
 * used at :1603-1613 for the hull's box and at :1653-1658 as the `depth` initialisation): every pixel with a positive depth of a
 * batch of depth maps [B,H,W], back-projected.  For image b and the pixel (x, y) -- integers, no half-pixel offset --, all in
 * double, in this order of operations (every three-term sum left to right), without fused multiply-adds:
 *   p = kinv (x, y, 1),  v = p / sqrt(p0 p0 + p1 p1 + p2 p2),  v' = R v,  point = o + depth v'     (pose = [R | o], 3x4 row-major)
 * rounded to float32 once.  A pixel survives iff depth > 0 (0, -0, negatives and NaN are dropped; +inf survives and gives
 * non-finite coordinates) and, when `masks` is given, its mask byte is non-zero.  Survivors are numbered in pixel order
 * i = b H W + y W + x.
 *
 * `cameras`: DEVICE array of B records, 8-byte aligned.  `depths`: device, [B,H,W] float32, or float64 with depth_is_double = 1.
 * `masks`: device, [B,H,W] bytes, or NULL.  `images`: device, [B,H,W,3] elements of color_bytes (1, 4 or 8) bytes each, read only
 * when colors_out is given.  `workspace`: sr_depth_points_workspace_bytes(B H W) bytes, 8-byte aligned.
 *
 * sr_depth_points_mark: 2 launches (one lane per pixel, then one workgroup that orders the workgroup counts and reduces the
 *   bounds).  Writes the number of survivors to count_out (device int32) and to bounds_out (device float[2]) the smallest and the
 *   largest float32 coordinate of the survivors, the three components together; either may be NULL, not both.  A NaN coordinate
 *   (possible only for depth = +inf) takes no part in the bounds, an infinite one does; without any, the bounds are (+inf, -inf).
 * sr_depth_points_gather (same batch and workspace, after the mark call): 1 launch; writes the first `capacity` survivors in pixel
 *   order: points_out [capacity,3] float32 (recomputed, not stored by the mark call), colors_out [capacity,3] elements copied
 *   from `images`, indices_out [capacity] int64 pixel indices; any of them may be NULL.  A capacity below the count gives an
 *   ordered prefix.
 * sr_depth_points_select (instead of the gather): 1 launch; row j of the outputs [n_ranks, ...] is survivor number ranks[j]
 *   (device int64; any order, repeats allowed).  A rank outside [0, count) reads nothing and writes a row of NaN coordinates,
 *   zero colour bytes and the index -1, and stores 1 to *flag_out (device int32), which the call otherwise leaves alone: zero it
 *   before the call.
 * No atomics: the same inputs give the same bytes.  Nothing waits for the device; every launch goes to hip_stream.
 * Refused on the host, before any launch: B < 0, H or W < 1, B H W > 2^31 - 1, a depth_is_double other than 0 and 1, a
 * color_bytes other than 1, 4 and 8 (when colors_out is given), a negative capacity or n_ranks, a null pointer where one is read
 * or written, and a misaligned one.  B = 0 (an empty batch; mark and gather), capacity = 0, n_ranks = 0 and a call without any
 * output launch nothing and succeed; the mark call then leaves count_out and bounds_out alone. */
typedef struct SrDepthCamera {
    double kinv[9];            /* rows of the inverse intrinsics' upper-left 3x3 */
    double pose[12];           /* rows of the camera-to-world pose's upper 3x4: [R | o] */
} SrDepthCamera;
size_t sr_depth_points_workspace_bytes(long long n_items);
int sr_depth_points_mark(int B, int H, int W, const SrDepthCamera* cameras, const void* depths, int depth_is_double,
                         const unsigned char* masks, void* workspace, int* count_out, float* bounds_out, void* hip_stream);
int sr_depth_points_gather(int B, int H, int W, const SrDepthCamera* cameras, const void* depths, int depth_is_double,
                           const void* images, int color_bytes, const void* workspace, long long capacity, float* points_out,
                           void* colors_out, long long* indices_out, void* hip_stream);
int sr_depth_points_select(int B, int H, int W, const SrDepthCamera* cameras, const void* depths, int depth_is_double,
                           const void* images, int color_bytes, const void* workspace, const long long* ranks, long long n_ranks,
                           float* points_out, void* colors_out, long long* indices_out, int* flag_out, void* hip_stream);

/* Subset steps (reference train.py:56-60, :68, :281-286, scene/gaussian_model.py:431-438: `--n_splats`): draw n_pick of n_rows
 * rows on the device, gather the step's tensors through them, scatter gradients and the densification bookkeeping back.
 *
 * The draw.  idx_out[j] = P(j), j < n_pick, where P is a keyed bijection of [0, n_rows): n_pick distinct rows, a uniform subset in
 * random order, without a permutation of n_rows in memory.  With b = the smallest number of bits with 2^b >= n_rows, lo = b / 2
 * (rounded down) and hi = b - lo, a value x < 2^b is split into L = its low lo bits and H = its high hi bits, and round r = 0 ..
 * n_keys - 1 of an alternating Feistel network maps
 *   r even:  L ^= mix(H, keys[r]) mod 2^lo          r odd:  H ^= mix(L, keys[r]) mod 2^hi
 *   mix(v, k): h = (v + k_lo) * 0x9E3779B1;  h ^= h >> 15;  h = (h ^ k_hi) * 0x85EBCA6B;  h ^= h >> 13;  h *= 0xC2B2AE35;  h ^= h >> 16
 * in unsigned 32-bit arithmetic (k_lo / k_hi: the halves of the 64-bit key).  Every round is an involution of [0, 2^b), so the
 * network F is a bijection of it for any keys, and 2^b < 2 n_rows.  P(j) = the first of F(j), F(F(j)), ... that is < n_rows (cycle
 * walking): the walk from j < n_rows stays on j's cycle of F and meets a value < n_rows at j itself at the latest, and the first
 * such values of different j differ -- P is a bijection of [0, n_rows) because F is one of [0, 2^b).  Each step lands below n_rows
 * with probability > 1/2; a lane gives up after SR_DRAW_MAX_WALK steps, writes -1 and stores 1 to *flag (a correct F gets there
 * with probability < 2^-256: the bound is there so that no lane can spin).  Integer arithmetic only; `keys` is HOST memory, passed
 * to the kernel by value (the facade derives them from one 64-bit seed with splitmix64).
 *
 * sr_draw_rows: 1 launch, one lane per output, no workspace.
 * sr_draw_rows_ascending: the same subset in ascending order (coalescing gathers, a result that does not depend on the draw
 *   order): 3 launches and no fill.  Row i belongs to the subset iff P^-1(i) < n_pick, and P^-1 is the same walk with F^-1 (the
 *   rounds in reverse order): one lane per ROW decides that with O(1) memory, the wavefront's members become one 64-bit word, and the
 *   fixed-order scan and the ordered gather the hull and the depth op use write the members' numbers.  No flag byte per row, no
 *   fill, no atomics.  `workspace`: sr_draw_rows_ascending_workspace_bytes(n_rows) bytes (one bit per row and one count per 256
 *   rows), 8-byte aligned.  *flag also becomes 1 when the members counted differ from n_pick (impossible for a bijection).
 *
 * sr_rows_gather: 1 launch for up to SR_ROWS_MAX_JOBS tensors.  Job k writes, for every j < n_pick and every column c of its row,
 *   dst[j dst_row_stride + dst_col_offset + c] = op(src[idx[j] row_floats + c]):  SR_ROWS_COPY the value, SR_ROWS_EXP its expf
 *   (`scaling_activation`), SR_ROWS_EXP_TO3 (row_floats must be 1) expf of the one source float into three columns
 *   (`use_isotropic`, scene/gaussian_model.py:66-67).  Stride and offset count floats: `_features_dc` [N,1,3] at offset 0 and
 *   `_features_rest` [N,15,3] at offset 3 of stride 48 give `get_features` (:79-82) without the cat.  A job with row_floats = 0 is
 *   skipped.  An idx[j] outside [0, n_rows) reads nothing, writes NaN to the row of every job and stores 1 to *flag.
 * sr_rows_scatter: its backward, 1 launch, the same job table (job.src is not read; job.dst is the forward's output, read by the
 *   two EXP ops as the saved value of expf).  dL_ddst[k] has job k's dst layout, dL_dsrc[k] its src layout [n_rows, row_floats]
 *   (NULL: job k has no gradient to write).  dL_dsrc[k][idx[j], c] = dL_ddst[k][j, c] (times dst[j, c] for SR_ROWS_EXP;
 *   SR_ROWS_EXP_TO3: the three columns of dL_ddst added in column order, times dst[j, 0]).  Rows that were not drawn are not
 *   written: zero dL_dsrc first.  PRECONDITION: the idx are distinct (what the draw gives) -- every element then has one writer,
 *   there are no atomics and repeated calls give the same bytes; with a repeated index one of its writers wins.  An idx[j] outside
 *   [0, n_rows) writes nothing and stores 1 to *flag.
 * sr_densification_stats_rows: sr_densification_stats with i -> idx[i] on the three full-size outputs, 1 launch: for i < n_pick
 *   with radii[i] > 0,  grad_accum[idx[i]] += |dL_dmeans2D[i, :2]|;  denom[idx[i]] += 1;  max_radii2D[idx[i]] = max(.., radii[i]);
 *   every other row keeps its bits.  (Reference train.py:284-286 builds the drawn rows of max_radii2D with torch.empty_like, so a
 *   drawn row that is not visible receives uninitialised memory there; here it is unchanged, as in the `_idx is None` branch.)
 *   Same precondition: distinct idx.  An idx[i] outside [0, n_rows) updates nothing and stores 1 to *flag.
 *
 * `flag` (device int32, may be NULL) is only ever set, never cleared: zero it before the call.  Rows are addressed with 64-bit
 * offsets.  Nothing waits for the device; every launch goes to hip_stream.  Refused on the host, before any launch: n_rows outside
 * 0 .. 2^31 - 1, n_pick outside 0 .. n_rows (the two draws) or 0 .. 2^31 - 1, n_keys outside 1 .. SR_DRAW_MAX_KEYS, n_jobs outside
 * 0 .. SR_ROWS_MAX_JOBS, an unknown op, a negative row_floats, SR_ROWS_EXP_TO3 with another row_floats than 1, a row that does not
 * fit into dst_row_stride, a null pointer where one is read or written, and a misaligned one.  n_pick = 0 launches nothing. */
#define SR_DRAW_MAX_KEYS 16
#define SR_DRAW_MAX_WALK 256
#define SR_ROWS_MAX_JOBS 8
#define SR_ROWS_COPY 0
#define SR_ROWS_EXP 1
#define SR_ROWS_EXP_TO3 2
typedef struct SrRowsJob {
    const float* src;          /* [n_rows, row_floats] */
    float* dst;                /* [n_pick, dst_row_stride], written from column dst_col_offset on */
    int row_floats;            /* floats of a source row; 0: the job is skipped */
    int dst_row_stride;        /* floats between two rows of dst */
    int dst_col_offset;        /* first column of dst this job writes */
    int op;                    /* SR_ROWS_* */
} SrRowsJob;
int sr_draw_rows(long long n_rows, long long n_pick, const unsigned long long* keys, int n_keys, long long* idx_out,
                 int* flag_or_null, void* hip_stream);
size_t sr_draw_rows_ascending_workspace_bytes(long long n_rows);
int sr_draw_rows_ascending(long long n_rows, long long n_pick, const unsigned long long* keys, int n_keys, void* workspace,
                           long long* idx_out, int* flag_or_null, void* hip_stream);
int sr_rows_gather(int n_jobs, const SrRowsJob* jobs, long long n_pick, const long long* idx, long long n_rows, int* flag_or_null,
                   void* hip_stream);
int sr_rows_scatter(int n_jobs, const SrRowsJob* jobs, const float* const* dL_ddst, float* const* dL_dsrc, long long n_pick,
                    const long long* idx, long long n_rows, int* flag_or_null, void* hip_stream);
int sr_densification_stats_rows(long long n_pick, const long long* idx, long long n_rows, const float* dL_dmeans2D, const int* radii,
                                float* grad_accum, float* denom, float* max_radii2D, int* flag_or_null, void* hip_stream);

/* The flow head of the deform network (reference utils/time_utils.py:194-304 `FlowHead`, the last stage of a dynamic step; replaces
 * two to four nn.Linear calls, ~25 small per-point kernels and their autograd backward): per point n, with the row h = hidden[n]
 * (`width` floats) and the point p = pts[n],
 *   z = [ branch_0(h) | branch_1(h) | ... ],  branch_i(h) = weight_i h + bias_i  (weight_i [rows_i, width] as nn.Linear holds it)
 * and an epilogue by `model` (eps = 1e-5; I + sin(t) [w] + (1 - cos t) [w]^2 = R(w, t), [w]^2 = w w^T - |w|^2 I;
 * T(w, v, t) = t v + (1 - cos t) w x v + (t - sin t) w x (w x v)):
 *   SR_FLOW_OFFSET      branches warp(3)                    flow = z,  means3D = p + flow
 *   SR_FLOW_SE3         w(3), v(3)                          t = |w|, w' = w / t + eps, v' = v / t + eps, R = R(w', t), T = T(w', v', t):
 *                                                           means3D = R p + T,  flow = [R T; 0 0 0 1]  ([N, 4, 4], row-major)
 *   SR_FLOW_SE3_AFFINE  w(3), v(3), offset(3)               means3D = R p + T + offset,  flow = means3D - p
 *   SR_FLOW_SE3_SCALED  w(3), v(3), scale(1), offset(3)     means3D = softplus(scale) R p + T + offset  (softplus: log1p(exp x), x itself
 *                                                           above 20),  flow = means3D - p
 *   SR_FLOW_AFFINE      w(9), v(3)                          means3D = A p + v, A = the nine outputs row-major,  flow = means3D - p
 *   SR_FLOW_DCT         coeff(3 n_basis)                    flow[c] = sum_k coeff[c n_basis + k] bases[k],  means3D = p + flow
 * `flow` is [N, 3] except for SR_FLOW_SE3.  A point with |w| = 0 gives non-finite results (as in the reference).
 *
 * Tensors are fp32, contiguous and 16-byte aligned (pts, means3D, flow [N, 3] and bases: 4-byte).  z is a sum of doubles in a fixed order
 * (bias, then the columns of h in order), the epilogue runs in double, and every stored value is rounded once; a workgroup is 256
 * consecutive points whatever the device, nothing is added atomically and nothing waits on the host: repeated calls are
 * bit-identical.  Rows are addressed with 64-bit offsets.  One launch each.
 *
 * Limits: width a multiple of 4 in 4 .. SR_FLOW_MAX_WIDTH; 1 <= n_basis <= SR_FLOW_MAX_BASIS for SR_FLOW_DCT (ignored otherwise);
 * the branch count and rows of the model as listed; 0 <= n_points < 2^31.  Anything else, a null pointer where one is read or
 * written, or a misaligned one, returns nonzero with sr_last_error set before any launch, and the three size queries return 0.
 * n_points = 0 is valid and launches nothing.
 *
 * forward:  `saved` (may be null: no backward will follow) receives z as doubles, sr_flow_head_saved_bytes bytes, 8-byte aligned.
 * backward: reads pts, bases, `saved`, the branch weights (bias is not read), dL_dmeans3D and dL_dflow (may be null = zeros);
 *   writes dL_dz [n_points, dz_row] fp32 with dz_row = sr_flow_head_dz_row: every branch's columns start at the next multiple of 4
 *   (the padding is written as zeros), so that one SrMlpGradJob per branch -- dz = dL_dz + first column, m = rows -- gives all
 *   weight and bias gradients in one sr_mlp_weight_grad call (allocate one row more than n_points: such a job reads whole rows
 *   from its first column on); dL_dpts [N, 3] and dL_dhidden [N, width] = dz W (either may be null); and, for SR_FLOW_DCT, one
 *   partial sum of dL_dbases per workgroup into `workspace`: doubles [ceil(n_points / 256)][n_basis], to be added in this order.
 *   `workspace`: sr_flow_head_workspace_bytes bytes (never 0 for a supported shape), 8-byte aligned. */
#define SR_FLOW_OFFSET 0
#define SR_FLOW_SE3 1
#define SR_FLOW_SE3_AFFINE 2
#define SR_FLOW_SE3_SCALED 3
#define SR_FLOW_AFFINE 4
#define SR_FLOW_DCT 5
#define SR_FLOW_MAX_BRANCHES 4
#define SR_FLOW_MAX_WIDTH 256
#define SR_FLOW_MAX_OUT 32
#define SR_FLOW_MAX_BASIS 10
typedef struct SrFlowBranch {
    const float* weight;       /* [rows, width] */
    const float* bias;         /* [rows]; not read by the backward */
    int rows;
} SrFlowBranch;
size_t sr_flow_head_saved_bytes(int model, long long n_points, int width, int n_basis);
size_t sr_flow_head_workspace_bytes(int model, long long n_points, int width, int n_basis);
int sr_flow_head_dz_row(int model, int n_basis);
int sr_flow_head_forward(int model, long long n_points, int width, int n_basis, int n_branches, const SrFlowBranch* branches,
                         const float* hidden, const float* pts, const float* bases, float* means3D, float* flow, void* saved,
                         void* hip_stream);
int sr_flow_head_backward(int model, long long n_points, int width, int n_basis, int n_branches, const SrFlowBranch* branches,
                          const float* pts, const float* bases, const void* saved, const float* dL_dmeans3D, const float* dL_dflow,
                          float* dL_dpts, float* dL_dz, float* dL_dhidden, void* workspace, void* hip_stream);

/* The view-dependent colour head (reference utils/time_utils.py:360-376, 494-498 `mlp_rgb_viewdep` with use_view_dep_rgb, evaluated per
 * view by gaussian_renderer/__init__.py:43-46; replaces, per view, a subtract, a norm, a divide, a cat that materialises
 * [N, width + 3], an addmm, a sigmoid and their autograd backward): for every point n and every view v of a step, in one launch,
 *   z[v, c]   = bias[c] + sum_f weight[c, f] feature[n, f] + sum_k weight[c, width + k] r_v[k],   colours[v, n, c] = 1 / (1 + exp(-z[v, c]))
 *   r_v = (p - c_v) / |p - c_v|, p = means3D[n], c_v = campos[v]   (SR_VIEW_FROM_CAMERAS: `campos_or_dirs` is campos [V, 3])
 *   r_v = dirs[v, n]                                                (SR_VIEW_DIRS_GIVEN:   `campos_or_dirs` is dirs [V, N, 3]; means3D is not read)
 * `weight` [3, width + 3] and `bias` [3] as nn.Linear holds them over cat([feature, viewdir]).  The one limit: a point that
 * coincides with a camera centre gives non-finite values in that view (as in the reference).
 *
 * Tensors are fp32 and contiguous; feature, weight, dL_dfeature and dL_dzsum 16-byte aligned, saved and workspace 8-byte, the
 * [., 3] tensors and bias 4-byte.  z is a sum of doubles in a fixed order (bias, then the feature columns in order, then the three
 * direction columns); the direction, the sigmoid and the backward run in double and every stored value is rounded once; a workgroup
 * is 256 consecutive points whatever the device, nothing is added atomically and nothing waits on the host: repeated calls are
 * bit-identical.  Rows are addressed with 64-bit offsets.  One launch each; the feature rows are read once for all views.
 *
 * Limits: mode one of the two; width a multiple of 4 in 4 .. SR_VIEW_MAX_WIDTH; 1 <= n_views <= SR_VIEW_MAX_VIEWS (more views:
 * several calls); 0 <= n_points < 2^31.  Anything else, a null pointer where one is read or written, or a misaligned one, returns
 * nonzero with sr_last_error set before any launch, and the two size queries return 0.  n_points = 0 is valid and launches nothing.
 *
 * forward:  `saved` (may be null: no backward will follow) receives the view-independent part bias + weight[:, :width] feature as
 *   doubles [3][n_points], sr_view_color_saved_bytes bytes: the backward re-derives every z[v] from it with the same three FMAs.
 * backward: reads means3D / campos or dirs, weight, `saved` and dL_dcolours [V, N, 3] (feature and bias are not read).  With
 *   g[v] = dL_dcolours[v, n] s (1 - s) it writes
 *     dL_dzsum [n_points + 1, 4]: row n = [ sum_v g[v] in view order | 0 ] (the last row is not written), so that ONE SrMlpGradJob --
 *       dz = dL_dzsum, dz_row = 4, m = 3, x = feature, k = width, dw_row = width + 3, dw_col0 = 0, db = null -- gives dweight[:, :width];
 *     dL_dfeature [N, width] = that sum times weight[:, :width], written once (may be null);
 *     dL_dpos (may be null): SR_VIEW_FROM_CAMERAS dL_dmeans3D [N, 3] = sum_v (I - r_v r_v^T) / |p - c_v| weight[:, width:]^T g[v] in view
 *       order; SR_VIEW_DIRS_GIVEN dL_ddirs [V, N, 3], [v, n] = weight[:, width:]^T g[v];
 *     one partial sum per workgroup of dweight[:, width:] = sum_n sum_v g[v] (x) r_v (row-major 3 x 3) and of dbias = sum_n sum_v g[v]
 *       into `workspace`: doubles [ceil(n_points / 256)][12], nine and three, to be added in this order.  (dbias is summed here, in
 *       double: its terms span the whole range of the upstream gradients, which a float32 sum over 10^5 points does not hold.)
 *   `workspace`: sr_view_color_workspace_bytes bytes (never 0 for a supported shape). */
#define SR_VIEW_FROM_CAMERAS 0
#define SR_VIEW_DIRS_GIVEN 1
#define SR_VIEW_MAX_WIDTH 256
#define SR_VIEW_MAX_VIEWS 16
size_t sr_view_color_saved_bytes(long long n_points, int width, int n_views);
size_t sr_view_color_workspace_bytes(long long n_points, int width, int n_views);
int sr_view_color_forward(int mode, long long n_points, int width, int n_views, const float* feature, const float* means3D,
                          const float* campos_or_dirs, const float* weight, const float* bias, float* colours, void* saved,
                          void* hip_stream);
int sr_view_color_backward(int mode, long long n_points, int width, int n_views, const float* means3D, const float* campos_or_dirs,
                           const float* weight, const void* saved, const float* dL_dcolours, float* dL_dfeature, float* dL_dpos,
                           float* dL_dzsum, void* workspace, void* hip_stream);

/* Diagnostics for the parity tests: byte offsets of four arrays inside the opaque buffers of a view with these sizes
 * (`instances` = the capacity the binning buffer was carved for):
 *   out[0]  geom:    tile_start  uint32[tiles + 1]   first list entry of every 16x16 tile (row-major tiles)
 *   out[1]  binning: sorted_id   uint32[instances]   splat index of every list entry, per tile front to back
 *   out[2]  geom:    total       uint32[4]           [0] = tile-splat instances
 *   out[3]  geom:    offsets     uint32[N]           first gradient slot of every splat
 * The per-tile lists are the counterpart of [EXT]'s sorted point_list + ranges (binningBuffer / imgBuffer). */
int sr_debug_layout(int n_splats, int height, int width, long long instances, size_t* out4);

/* Work counters of the backward blend, accumulated over the sr_backward calls of a library built with -DSR_BWD_STATS
 * (bench.py's pairs_evaluated / pairs_blended; the product build leaves them out and returns zeros):
 * out16 = { list entries replayed, (4x4 quad, entry) pairs, 16-entry buckets, (pixel, entry) pairs evaluated,
 *           pairs blended, list chunks, 0, 0,  then 8 shader-clock totals (summed over wavefronts) of the kernel's phases:
 *           preamble, test, barrier, slot assignment + scatter, barrier, replay, barrier, combine }.
 * Synchronises the device; reset != 0 clears the counters afterwards. */
int sr_debug_backward_stats(unsigned long long* out16, int reset);

/* Host-synchronisation counters of the forward (process-wide, since load or the last reset):
 *   out4 = { host waits inside sr_forward (one per call: the instance-count read-back),  sr_forward_async calls (none waits),
 *            tickets that were redeemed while stage 1 of their forward was still running (the host waited in sr_ticket_wait),
 *            tickets ever created (the pool's size) }. */
int sr_debug_counters(long long* out4, int reset);

/* Launch counters of the separate per-tile sort kernels in front of the forward blend (process-wide, since load or the last
 * reset; one count per forward that launched the class):
 *   out4 = { the kernel for lists of up to 2048 entries (never under the product setting, where the forward blend sorts those
 *            lists itself: sr_set_sort_kernel),  the class of 2049..4096 entries,  4097..8192,  longer lists }. */
int sr_debug_sort_counters(long long* out4, int reset);

/* debug = true (SrView.debug): every stage is followed by a stream synchronisation + error check, and a FAILED stage writes
 * the call's arguments to snapshot_fw.dump / snapshot_bw.dump in the working directory before the error is returned -- what
 * [EXT] does with `debug` set (its snapshot_fw.dump / snapshot_bw.dump; reference gaussian_renderer/__init__.py:71 passes
 * pipe.debug).  Format: "SRSNAP1\0", failing stage [32], then records {name[16], uint64 bytes, payload}: view scalars,
 * count, camera arrays, every per-splat input that was passed, for the backward the upstream gradients (a record whose
 * device-to-host copy fails has 0 bytes).  sr_debug_snapshot runs that path for given arguments without a failure (tests). */
int sr_debug_snapshot(const SrView* view, const SrSplats* splats, const float* dL_dcolor, const float* dL_ddepth,
                      const float* dL_dalpha, int backward);

/* Optional per-kernel timing with HIP events recorded on the launch stream (used by bench.py for the
 * live roofline figure; off by default, adds two event records per launch when on).
 * sr_profile_collect synchronises the recorded events, ADDS the elapsed milliseconds and launch counts
 * per stage into the caller's arrays of SR_PROFILE_STAGES entries, and clears the recording. */
#define SR_PROFILE_STAGES 7 /* preprocess, scan, emit, sort_tiles, render_forward, render_backward, preprocess_backward */
int sr_profile_enable(int on);
int sr_profile_collect(double* ms_sum, long long* launches);
const char* sr_profile_stage_name(int stage);

#ifdef __cplusplus
}
#endif
#endif /* SPLATRASTER_H */
