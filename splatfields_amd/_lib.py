"""ctypes binding of the C ABI declared in include/splatraster.h.

The product path has no CPU fallback: if libsplatraster.so is missing this module raises."""
from __future__ import annotations

import ctypes as C
from pathlib import Path

import os

import torch

# SPLATRASTER_LIB selects an alternative build of the same ABI (A/B experiments); default: the in-tree library.
LIB_PATH = Path(os.environ.get("SPLATRASTER_LIB") or (Path(__file__).resolve().parent / "libsplatraster.so"))

c_float_p = C.c_void_p  # raw device pointers travel as integers


class SrView(C.Structure):
    _fields_ = [("image_height", C.c_int), ("image_width", C.c_int), ("tanfovx", C.c_float), ("tanfovy", C.c_float),
                ("scale_modifier", C.c_float), ("sh_degree", C.c_int), ("sh_coeffs", C.c_int), ("prefiltered", C.c_int),
                ("debug", C.c_int), ("viewmatrix", C.c_void_p), ("projmatrix", C.c_void_p), ("campos", C.c_void_p),
                ("bg", C.c_void_p)]


class SrSplats(C.Structure):
    _fields_ = [("count", C.c_int), ("means3D", C.c_void_p), ("opacities", C.c_void_p), ("scales", C.c_void_p),
                ("rotations", C.c_void_p), ("cov3D_precomp", C.c_void_p), ("shs", C.c_void_p),
                ("colors_precomp", C.c_void_p), ("raw_params", C.c_int), ("shs_rest", C.c_void_p)]


class SrGrads(C.Structure):
    _fields_ = [("dL_dmeans3D", C.c_void_p), ("dL_dmeans2D", C.c_void_p), ("dL_dopacity", C.c_void_p),
                ("dL_dscales", C.c_void_p), ("dL_drotations", C.c_void_p), ("dL_dcov3D", C.c_void_p),
                ("dL_dshs", C.c_void_p), ("dL_dcolors", C.c_void_p), ("dL_dshs_rest", C.c_void_p)]


class SrMlpOp(C.Structure):
    _fields_ = [("w_packed", C.c_void_p), ("bias", C.c_void_p), ("src", C.c_void_p), ("mask", C.c_void_p), ("store", C.c_void_p),
                ("sign_store", C.c_void_p), ("mask_bits", C.c_void_p),
                ("out_tiles", C.c_int), ("mem_tiles", C.c_int), ("reg_tiles", C.c_int), ("src_row", C.c_int), ("epilogue", C.c_int),
                ("mask_row", C.c_int), ("store_row", C.c_int), ("store_channels", C.c_int), ("store_accumulate", C.c_int),
                ("keep_state", C.c_int)]


class SrMlpNet(C.Structure):
    _fields_ = [("ops", C.POINTER(SrMlpOp)), ("n_ops", C.c_int)]


class SrMlpHeadInput(C.Structure):
    _fields_ = [("x0", C.c_void_p), ("dL_dx0", C.c_void_p), ("multires", C.c_int), ("row", C.c_int)]


class SrMlpHeadOutput(C.Structure):
    _fields_ = [("y", C.c_void_p), ("out", C.c_void_p), ("dL_dout", C.c_void_p), ("g", C.c_void_p), ("out_features", C.c_int),
                ("row", C.c_int), ("activation", C.c_int), ("reserved", C.c_int)]


class SrMlpPackJob(C.Structure):
    _fields_ = [("w", C.c_void_p), ("bias_src", C.c_void_p), ("dst", C.c_void_p), ("bias_dst", C.c_void_p), ("ld", C.c_int),
                ("transposed", C.c_int), ("row0", C.c_int), ("n_rows", C.c_int), ("n_mem", C.c_int), ("mem_pad", C.c_int),
                ("mem_col0", C.c_int), ("n_reg", C.c_int), ("reg_width", C.c_int), ("reg_col0", C.c_int), ("out_tiles", C.c_int),
                ("n_bias", C.c_int)]


class SrMlpGradJob(C.Structure):
    _fields_ = [("dz", C.c_void_p), ("x", C.c_void_p), ("dw", C.c_void_p), ("db", C.c_void_p), ("dz_row", C.c_int), ("m", C.c_int),
                ("x_row", C.c_int), ("k", C.c_int), ("dw_row", C.c_int), ("dw_col0", C.c_int)]


class SrResFieldJob(C.Structure):
    _fields_ = [("w", C.c_void_p), ("weights_t", C.c_void_p), ("matrix_t", C.c_void_p), ("out", C.c_void_p), ("d_out", C.c_void_p),
                ("d_matrix_t", C.c_void_p), ("d_weights_t", C.c_void_p), ("count", C.c_int), ("rank", C.c_int), ("capacity", C.c_int)]


class SrAdamJob(C.Structure):
    _fields_ = [("param", C.c_void_p), ("grad", C.c_void_p), ("exp_avg", C.c_void_p), ("exp_avg_sq", C.c_void_p),
                ("count", C.c_longlong), ("row", C.c_int), ("step_size", C.c_float), ("bias_correction2_sqrt", C.c_float),
                ("one_minus_beta1", C.c_float), ("one_minus_beta2", C.c_float), ("eps", C.c_float)]


class SrSumJob(C.Structure):
    _fields_ = [("dst", C.c_void_p), ("src", C.c_void_p), ("elems", C.c_longlong), ("view_stride", C.c_longlong)]


class SrNetAdamSlot(C.Structure):
    _fields_ = [("param", C.c_void_p), ("exp_avg", C.c_void_p), ("exp_avg_sq", C.c_void_p), ("count", C.c_longlong),
                ("chunk_end", C.c_longlong)]


class SrNetAdamScalars(C.Structure):
    _fields_ = [("step_size", C.c_float), ("bias_correction2_sqrt", C.c_float), ("one_minus_beta1", C.c_float),
                ("one_minus_beta2", C.c_float), ("eps", C.c_float)]


class SrPlaneJob(C.Structure):
    _fields_ = [(name, C.c_void_p) for name in (
        "x", "weight", "bias", "gamma", "beta", "stats", "residual", "out", "pre", "dy", "dx", "dweight", "dbias", "dgamma", "dbeta",
        "d_residual", "add", "dx_out")]


class SrAttentionJob(C.Structure):
    _fields_ = [(name, C.c_void_p) for name in (
        "x", "gamma", "beta", "stats", "wq", "bq", "wk", "bk", "wv", "bv", "wo", "bo", "out", "saved", "dy", "dx", "dgamma", "dbeta",
        "dwq", "dbq", "dwk", "dbk", "dwv", "dbv", "dwo", "dbo")]


class SrHullView(C.Structure):
    _fields_ = [("m", C.c_double * 12), ("mask_offset", C.c_longlong), ("height", C.c_int), ("width", C.c_int),
                ("convention", C.c_int), ("outside", C.c_int)]


class SrDepthCamera(C.Structure):
    _fields_ = [("kinv", C.c_double * 9), ("pose", C.c_double * 12)]


class SrRowsJob(C.Structure):
    _fields_ = [("src", C.c_void_p), ("dst", C.c_void_p), ("row_floats", C.c_int), ("dst_row_stride", C.c_int),
                ("dst_col_offset", C.c_int), ("op", C.c_int)]


class SrFlowBranch(C.Structure):
    _fields_ = [("weight", C.c_void_p), ("bias", C.c_void_p), ("rows", C.c_int)]


# include/splatraster.h: SR_FLOW_*
FLOW_OFFSET, FLOW_SE3, FLOW_SE3_AFFINE, FLOW_SE3_SCALED, FLOW_AFFINE, FLOW_DCT = 0, 1, 2, 3, 4, 5
FLOW_MAX_BRANCHES, FLOW_MAX_WIDTH, FLOW_MAX_OUT, FLOW_MAX_BASIS = 4, 256, 32, 10
VIEW_FROM_CAMERAS, VIEW_DIRS_GIVEN, VIEW_MAX_WIDTH, VIEW_MAX_VIEWS = 0, 1, 256, 16   # include/splatraster.h: SR_VIEW_*
HULL_KRT, HULL_NDC, HULL_OUTSIDE_CARVE, HULL_OUTSIDE_KEEP, HULL_MAX_VIEWS = 0, 1, 0, 1, 1024   # include/splatraster.h: SR_HULL_*
DRAW_MAX_KEYS, DRAW_MAX_WALK = 16, 256                       # include/splatraster.h: SR_DRAW_*
ROWS_MAX_JOBS, ROWS_COPY, ROWS_EXP, ROWS_EXP_TO3 = 8, 0, 1, 2   # include/splatraster.h: SR_ROWS_*
RESFIELD_MAX_JOBS, RESFIELD_MAX_RANK = 16, 64
PLANE_MAX_JOBS = 8                                           # include/splatraster.h: SR_PLANE_MAX_JOBS
CONV_PROLOGUE, CONV_UPSAMPLE, CONV_RESIDUAL, CONV_SILU_OUT = 1, 2, 4, 8   # include/splatraster.h: SR_CONV_*
MLP_MAX_GRAD_JOBS, MLP_MAX_GRAD_TASKS = 16, 128
MLP_MAX_PACK_JOBS = 32
MORAN_MAX_TENSORS, KNN_MAX_K = 8, 8                          # include/splatraster.h: SR_MORAN_MAX_TENSORS, SR_KNN_MAX_K
ADAM_MAX_TENSORS = 32                                        # include/splatraster.h: SR_ADAM_MAX_TENSORS
SUM_MAX_JOBS, SUM_MAX_VIEWS = 16, 16                          # include/splatraster.h: SR_SUM_MAX_JOBS, SR_SUM_MAX_VIEWS
NET_ADAM_MAX_GRADS = 480                                     # include/splatraster.h: SR_NET_ADAM_MAX_GRADS
QUANT_NONE, QUANT_PNG, QUANT_TO8B = 0, 1, 2                     # include/splatraster.h: SR_QUANT_*
LPIPS_CONVS, LPIPS_TAPS = 13, 5                                # include/splatraster.h: SR_LPIPS_*
MLP_MAX_OPS, MLP_NONE, MLP_LEAKY, MLP_MASK = 24, 0, 1, 2      # include/splatraster.h: SR_MLP_*
MLP_GROUP_MAX_NETS, MLP_GROUP_MAX_OPS, MLP_GROUP_MAX_HEADS = 8, 40, 8      # include/splatraster.h: SR_MLP_GROUP_*
MLP_OUT_NONE, MLP_OUT_SIGMOID, MLP_OUT_NORMALIZE = 0, 1, 2                 # include/splatraster.h: SR_MLP_OUT_*


# every symbol include/splatraster.h declares: name -> (restype, argtypes)
SYMBOLS = {
    "sr_version": (C.c_int, []),
    "sr_last_error": (C.c_char_p, []),
    "sr_geom_bytes": (C.c_size_t, [C.c_int, C.c_int, C.c_int]),
    "sr_binning_bytes": (C.c_size_t, [C.c_longlong, C.c_int, C.c_int]),
    "sr_image_bytes": (C.c_size_t, [C.c_int, C.c_int]),
    "sr_backward_scratch_bytes": (C.c_size_t, [C.c_longlong]),
    "sr_forward_prepare": (C.c_int, [C.POINTER(SrView), C.POINTER(SrSplats), C.c_void_p, C.c_void_p,
                                     C.POINTER(C.c_longlong), C.c_void_p]),
    "sr_forward_render": (C.c_int, [C.POINTER(SrView), C.POINTER(SrSplats), C.c_void_p, C.c_void_p, C.c_longlong,
                                    C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "sr_forward": (C.c_int, [C.POINTER(SrView), C.POINTER(SrSplats), C.c_void_p, C.c_void_p, C.c_void_p, C.c_longlong,
                             C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(C.c_longlong), C.c_void_p]),
    "sr_forward_async": (C.c_int, [C.POINTER(SrView), C.POINTER(SrSplats), C.c_void_p, C.c_void_p, C.c_void_p, C.c_longlong,
                                   C.c_longlong, C.c_longlong, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(C.c_void_p),
                                   C.c_void_p]),
    "sr_ticket_wait": (C.c_int, [C.c_void_p, C.POINTER(C.c_longlong), C.POINTER(C.c_longlong)]),
    "sr_ticket_release": (C.c_int, [C.c_void_p]),
    "sr_forward_prepare_views": (C.c_int, [C.c_int, C.POINTER(SrView), C.POINTER(SrSplats), C.POINTER(C.c_void_p), C.POINTER(C.c_void_p),
                                           C.POINTER(C.c_longlong), C.POINTER(C.c_longlong), C.POINTER(C.c_longlong), C.c_void_p]),
    "sr_forward_render_views": (C.c_int, [C.c_int, C.POINTER(SrView), C.POINTER(SrSplats), C.POINTER(C.c_void_p), C.POINTER(C.c_void_p),
                                          C.POINTER(C.c_longlong), C.POINTER(C.c_longlong), C.POINTER(C.c_longlong), C.POINTER(C.c_void_p),
                                          C.POINTER(C.c_void_p), C.POINTER(C.c_void_p), C.POINTER(C.c_void_p), C.c_void_p]),
    "sr_sum_views": (C.c_int, [C.c_int, C.POINTER(SrSumJob), C.c_int, C.c_void_p]),
    "sr_last_longest_list": (C.c_longlong, []),
    "sr_last_long_tiles": (C.c_longlong, []),
    "sr_expect_long_tiles": (C.c_int, [C.c_longlong]),
    "sr_debug_counters": (C.c_int, [C.POINTER(C.c_longlong), C.c_int]),
    "sr_debug_sort_counters": (C.c_int, [C.POINTER(C.c_longlong), C.c_int]),
    "sr_backward": (C.c_int, [C.POINTER(SrView), C.POINTER(SrSplats), C.c_void_p, C.c_void_p, C.c_longlong, C.c_longlong, C.c_void_p,
                              C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(SrGrads),
                              C.c_void_p]),
    "sr_backward_blend": (C.c_int, [C.POINTER(SrView), C.POINTER(SrSplats), C.c_void_p, C.c_void_p, C.c_longlong, C.c_longlong, C.c_void_p,
                                    C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "sr_backward_splats": (C.c_int, [C.POINTER(SrView), C.POINTER(SrSplats), C.c_void_p, C.c_void_p, C.c_longlong, C.c_longlong, C.c_void_p, C.c_void_p,
                                     C.c_void_p, C.POINTER(SrGrads), C.c_int, C.c_int, C.c_void_p]),
    "sr_debug_snapshot": (C.c_int, [C.POINTER(SrView), C.POINTER(SrSplats), C.c_void_p, C.c_void_p, C.c_void_p, C.c_int]),
    "sr_set_backward_kernel": (C.c_int, [C.c_int]),
    "sr_set_sort_kernel": (C.c_int, [C.c_int]),
    "sr_sh_forward": (C.c_int, [C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "sr_sh_forward_views": (C.c_int, [C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "sr_sh_backward": (C.c_int, [C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_float,
                                 C.c_void_p, C.c_void_p, C.c_int, C.c_void_p]),
    "sr_knn_workspace_bytes": (C.c_size_t, [C.c_int]),
    "sr_knn3_mean_dist2": (C.c_int, [C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "sr_knn_graph_workspace_bytes": (C.c_size_t, [C.c_int, C.c_int]),
    "sr_knn_graph": (C.c_int, [C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "sr_moran_workspace_bytes": (C.c_size_t, [C.c_int, C.c_int]),
    "sr_moran_edges_bytes": (C.c_size_t, [C.c_int, C.c_int, C.c_int]),
    "sr_moran_forward": (C.c_int, [C.c_int, C.c_int, C.c_float, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int,
                                   C.POINTER(C.c_void_p), C.POINTER(C.c_int), C.c_void_p, C.c_void_p, C.c_void_p]),
    "sr_moran_backward": (C.c_int, [C.c_int, C.c_int, C.c_float, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                    C.c_int, C.POINTER(C.c_void_p), C.POINTER(C.c_int), C.c_void_p, C.c_void_p, C.c_void_p,
                                    C.POINTER(C.c_void_p), C.c_void_p, C.c_void_p, C.c_void_p]),
    "sr_moran_weights": (C.c_int, [C.c_int, C.c_int, C.c_float, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "sr_moran_weights_backward": (C.c_int, [C.c_int, C.c_int, C.c_float, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                            C.c_void_p, C.c_void_p, C.c_void_p]),
    "sr_loss_workspace_bytes": (C.c_size_t, [C.c_int, C.c_int, C.c_int]),
    "sr_loss_maps_bytes": (C.c_size_t, [C.c_int, C.c_int, C.c_int]),
    "sr_photometric_forward": (C.c_int, [C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_float,
                                         C.c_float, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "sr_photometric_backward": (C.c_int, [C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                          C.c_float, C.c_float, C.c_float, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]),
    "sr_metrics_workspace_bytes": (C.c_size_t, [C.c_int, C.c_int, C.c_int]),
    "sr_image_metrics": (C.c_int, [C.c_int, C.c_int, C.c_int, C.c_void_p, C.POINTER(C.c_longlong), C.c_void_p, C.POINTER(C.c_longlong),
                                   C.c_void_p, C.c_longlong, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                   C.c_void_p]),
    "sr_lpips_packed_bytes": (C.c_size_t, []),
    # the three pointer tables are HOST arrays of device pointers
    "sr_lpips_pack_weights": (C.c_int, [C.POINTER(C.c_void_p), C.POINTER(C.c_void_p), C.POINTER(C.c_void_p), C.c_void_p, C.c_void_p,
                                        C.c_void_p, C.c_void_p]),
    "sr_lpips_workspace_bytes": (C.c_size_t, [C.c_int, C.c_int, C.c_int]),
    "sr_lpips_maps_floats": (C.c_size_t, [C.c_int, C.c_int, C.c_int]),
    "sr_lpips_forward": (C.c_int, [C.c_int, C.c_int, C.c_int, C.c_void_p, C.POINTER(C.c_longlong), C.c_void_p, C.POINTER(C.c_longlong),
                                   C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "sr_adam_step": (C.c_int, [C.c_int, C.POINTER(SrAdamJob), C.c_void_p, C.c_longlong, C.c_void_p]),
    "sr_net_adam_plan": (C.c_int, [C.POINTER(SrNetAdamSlot), C.c_int]),
    "sr_net_adam_step": (C.c_int, [C.POINTER(SrNetAdamSlot), C.POINTER(SrNetAdamSlot), C.c_int, C.c_int, C.c_int, C.POINTER(C.c_void_p),
                                   C.POINTER(SrNetAdamScalars), C.c_void_p]),
    "sr_splat_reg_workspace_bytes": (C.c_size_t, [C.c_int]),
    "sr_splat_reg_forward": (C.c_int, [C.c_int, C.c_void_p, C.c_void_p, C.c_double, C.c_double, C.c_double, C.c_void_p, C.c_void_p, C.c_void_p]),
    "sr_splat_reg_backward": (C.c_int, [C.c_int, C.c_void_p, C.c_void_p, C.c_double, C.c_double, C.c_double, C.c_void_p, C.c_void_p, C.c_void_p,
                                        C.c_void_p, C.c_void_p]),
    "sr_depth_l1_workspace_bytes": (C.c_size_t, [C.c_int, C.c_int, C.c_int]),
    "sr_depth_l1_forward": (C.c_int, [C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "sr_depth_l1_backward": (C.c_int, [C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]),
    "sr_densify_workspace_bytes": (C.c_size_t, [C.c_int]),
    "sr_densify_plan": (C.c_int, [C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_float, C.c_float,
                                  C.c_float, C.c_float, C.c_float, C.c_void_p, C.c_void_p, C.POINTER(C.c_longlong), C.c_void_p]),
    "sr_densify_gather": (C.c_int, [C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p,
                                    C.c_void_p, C.c_void_p]),
    "sr_hull_workspace_bytes": (C.c_size_t, [C.c_longlong]),
    "sr_hull_carve": (C.c_int, [C.c_int, C.POINTER(SrHullView), C.c_void_p, C.c_longlong, C.c_void_p, C.c_int, C.c_void_p, C.c_longlong,
                                C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]),
    "sr_hull_gather": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_longlong, C.c_int, C.c_void_p, C.c_longlong, C.c_void_p, C.c_void_p,
                                 C.c_void_p]),
    # `cameras` is a DEVICE array of SrDepthCamera records: never dereferenced on the host (depth_cameras_arg casts the address)
    "sr_depth_points_workspace_bytes": (C.c_size_t, [C.c_longlong]),
    "sr_depth_points_mark": (C.c_int, [C.c_int, C.c_int, C.c_int, C.POINTER(SrDepthCamera), C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p,
                                       C.c_void_p, C.c_void_p]),
    "sr_depth_points_gather": (C.c_int, [C.c_int, C.c_int, C.c_int, C.POINTER(SrDepthCamera), C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p,
                                         C.c_longlong, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "sr_depth_points_select": (C.c_int, [C.c_int, C.c_int, C.c_int, C.POINTER(SrDepthCamera), C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p,
                                         C.c_void_p, C.c_longlong, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    # `keys` is HOST memory: an array of c_ulonglong
    "sr_draw_rows": (C.c_int, [C.c_longlong, C.c_longlong, C.POINTER(C.c_ulonglong), C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]),
    "sr_draw_rows_ascending_workspace_bytes": (C.c_size_t, [C.c_longlong]),
    "sr_draw_rows_ascending": (C.c_int, [C.c_longlong, C.c_longlong, C.POINTER(C.c_ulonglong), C.c_int, C.c_void_p, C.c_void_p, C.c_void_p,
                                         C.c_void_p]),
    "sr_rows_gather": (C.c_int, [C.c_int, C.POINTER(SrRowsJob), C.c_longlong, C.c_void_p, C.c_longlong, C.c_void_p, C.c_void_p]),
    "sr_rows_scatter": (C.c_int, [C.c_int, C.POINTER(SrRowsJob), C.POINTER(C.c_void_p), C.POINTER(C.c_void_p), C.c_longlong, C.c_void_p,
                                  C.c_longlong, C.c_void_p, C.c_void_p]),
    "sr_densification_stats_rows": (C.c_int, [C.c_longlong, C.c_void_p, C.c_longlong, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                              C.c_void_p, C.c_void_p, C.c_void_p]),
    "sr_mlp_pack": (C.c_int, [C.c_int, C.POINTER(SrMlpPackJob), C.c_void_p]),
    "sr_mlp_weight_grad_workspace": (C.c_size_t, [C.c_int, C.c_int, C.POINTER(SrMlpGradJob)]),
    "sr_mlp_weight_grad": (C.c_int, [C.c_int, C.c_int, C.POINTER(SrMlpGradJob), C.c_void_p, C.c_size_t, C.c_void_p]),
    "sr_mlp_chain": (C.c_int, [C.c_int, C.c_int, C.c_int, C.POINTER(SrMlpOp), C.c_float, C.c_void_p]),
    "sr_mlp_pack_bf16": (C.c_int, [C.c_int, C.POINTER(SrMlpPackJob), C.c_void_p]),
    "sr_mlp_chain_bf16": (C.c_int, [C.c_int, C.c_int, C.c_int, C.POINTER(SrMlpOp), C.c_float, C.c_void_p]),
    "sr_mlp_pack_bf16x3": (C.c_int, [C.c_int, C.POINTER(SrMlpPackJob), C.c_void_p]),
    "sr_mlp_chain_bf16x3": (C.c_int, [C.c_int, C.c_int, C.c_int, C.POINTER(SrMlpOp), C.c_float, C.c_void_p]),
    "sr_mlp_chain_group": (C.c_int, [C.c_int, C.c_int, C.c_int, C.POINTER(SrMlpNet), C.c_float, C.c_void_p]),
    "sr_mlp_chain_group_bf16": (C.c_int, [C.c_int, C.c_int, C.c_int, C.POINTER(SrMlpNet), C.c_float, C.c_void_p]),
    "sr_mlp_chain_group_bf16x3": (C.c_int, [C.c_int, C.c_int, C.c_int, C.POINTER(SrMlpNet), C.c_float, C.c_void_p]),
    "sr_mlp_group_input_forward": (C.c_int, [C.c_int, C.c_int, C.POINTER(SrMlpHeadInput), C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p,
                                             C.c_void_p]),
    "sr_mlp_group_input_backward": (C.c_int, [C.c_int, C.c_int, C.POINTER(SrMlpHeadInput), C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "sr_mlp_group_output": (C.c_int, [C.c_int, C.c_int, C.POINTER(SrMlpHeadOutput), C.c_void_p]),
    "sr_mlp_group_top_gradient": (C.c_int, [C.c_int, C.c_int, C.POINTER(SrMlpHeadOutput), C.c_float, C.c_void_p]),
    "sr_mlp_input_forward": (C.c_int, [C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "sr_mlp_top_gradient": (C.c_int, [C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_float, C.c_void_p, C.c_void_p]),
    "sr_mlp_input_backward": (C.c_int, [C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "sr_resfield_compose": (C.c_int, [C.c_int, C.POINTER(SrResFieldJob), C.c_void_p, C.c_void_p]),
    "sr_resfield_backward_workspace": (C.c_size_t, [C.c_int, C.POINTER(SrResFieldJob)]),
    "sr_resfield_backward": (C.c_int, [C.c_int, C.POINTER(SrResFieldJob), C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]),
    "sr_triplane_backward_workspace": (C.c_size_t, [C.c_int, C.c_int, C.c_int, C.c_int]),
    "sr_triplane_forward": (C.c_int, [C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "sr_triplane_backward": (C.c_int, [C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                       C.c_void_p, C.c_void_p]),
    "sr_groupnorm_stats_workspace": (C.c_size_t, [C.c_int, C.c_int, C.c_int, C.c_int, C.c_int]),
    "sr_groupnorm_stats": (C.c_int, [C.c_int, C.POINTER(SrPlaneJob), C.c_int, C.c_int, C.c_int, C.c_int, C.c_float, C.c_void_p, C.c_void_p]),
    "sr_conv3x3_forward": (C.c_int, [C.c_int, C.POINTER(SrPlaneJob), C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p]),
    "sr_conv3x3_backward_data": (C.c_int, [C.c_int, C.POINTER(SrPlaneJob), C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p]),
    "sr_groupnorm_silu_backward_workspace": (C.c_size_t, [C.c_int, C.c_int, C.c_int, C.c_int]),
    "sr_groupnorm_silu_backward": (C.c_int, [C.c_int, C.POINTER(SrPlaneJob), C.c_int, C.c_int, C.c_int, C.c_int, C.c_float, C.c_void_p,
                                             C.c_void_p]),
    "sr_conv3x3_weight_grad_workspace": (C.c_size_t, [C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int]),
    "sr_conv3x3_weight_grad": (C.c_int, [C.c_int, C.POINTER(SrPlaneJob), C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p,
                                         C.c_void_p]),
    "sr_attention_saved_bytes": (C.c_size_t, [C.c_int, C.c_int, C.c_int, C.c_int, C.c_int]),
    "sr_attention_backward_workspace": (C.c_size_t, [C.c_int, C.c_int, C.c_int, C.c_int, C.c_int]),
    "sr_attention_forward": (C.c_int, [C.c_int, C.POINTER(SrAttentionJob), C.c_int, C.c_int, C.c_int, C.c_int, C.c_float, C.c_void_p]),
    "sr_attention_backward": (C.c_int, [C.c_int, C.POINTER(SrAttentionJob), C.c_int, C.c_int, C.c_int, C.c_int, C.c_float, C.c_void_p,
                                        C.c_void_p]),
    "sr_flow_head_saved_bytes": (C.c_size_t, [C.c_int, C.c_longlong, C.c_int, C.c_int]),
    "sr_flow_head_workspace_bytes": (C.c_size_t, [C.c_int, C.c_longlong, C.c_int, C.c_int]),
    "sr_flow_head_dz_row": (C.c_int, [C.c_int, C.c_int]),
    "sr_flow_head_forward": (C.c_int, [C.c_int, C.c_longlong, C.c_int, C.c_int, C.c_int, C.POINTER(SrFlowBranch), C.c_void_p, C.c_void_p,
                                       C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "sr_flow_head_backward": (C.c_int, [C.c_int, C.c_longlong, C.c_int, C.c_int, C.c_int, C.POINTER(SrFlowBranch), C.c_void_p, C.c_void_p,
                                        C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "sr_view_color_saved_bytes": (C.c_size_t, [C.c_longlong, C.c_int, C.c_int]),
    "sr_view_color_workspace_bytes": (C.c_size_t, [C.c_longlong, C.c_int, C.c_int]),
    "sr_view_color_forward": (C.c_int, [C.c_int, C.c_longlong, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                        C.c_void_p, C.c_void_p, C.c_void_p]),
    "sr_view_color_backward": (C.c_int, [C.c_int, C.c_longlong, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                         C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "sr_debug_layout": (C.c_int, [C.c_int, C.c_int, C.c_int, C.c_longlong, C.POINTER(C.c_size_t)]),
    "sr_debug_backward_stats": (C.c_int, [C.POINTER(C.c_ulonglong), C.c_int]),
    "sr_profile_enable": (C.c_int, [C.c_int]),
    "sr_profile_collect": (C.c_int, [C.POINTER(C.c_double), C.POINTER(C.c_longlong)]),
    "sr_profile_stage_name": (C.c_char_p, [C.c_int]),
    "sr_mark_visible": (C.c_int, [C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "sr_densification_stats": (C.c_int, [C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
}

PROFILE_STAGES = 7
SR_VERSION = 4          # include/splatraster.h: the ABI this binding was written against
SR_NEED_CAPACITY = 2
SR_RAW_SCALES, SR_RAW_OPACITY, SR_RAW_ROTATIONS, SR_FORWARD_ONLY = 1, 2, 4, 8
_lib = None


def bind(path) -> C.CDLL:
    """dlopen a build of the library and attach the prototypes of every declared symbol."""
    lib = C.CDLL(str(path))
    for name, (res, args) in SYMBOLS.items():
        fn = getattr(lib, name)  # AttributeError if the ABI is incomplete
        fn.restype = res
        fn.argtypes = args
    got = lib.sr_version()
    if got != SR_VERSION:   # struct layouts, workspace sizes and buffer contracts belong to a version: never mix them
        raise RuntimeError(f"{path} implements version {got} of the splatraster ABI, this binding expects {SR_VERSION}: "
                           "rebuild it with `python -m splatfields_amd.build`")
    return lib


def load() -> C.CDLL:
    """Loads libsplatraster.so once; fails loudly when it has not been built."""
    global _lib
    if _lib is None:
        if not LIB_PATH.exists():
            raise RuntimeError(
                f"{LIB_PATH} is missing: build it with `python -m splatfields_amd.build` "
                "(hipcc --offload-arch=gfx950). There is no CPU fallback.")
        _lib = bind(LIB_PATH)
    return _lib


class use_library:
    """Context manager: route the facade through another build of the same ABI (bench.py's counting build)."""

    def __init__(self, path):
        self.handle = bind(path)

    def __enter__(self):
        global _lib
        self.prev, _lib = _lib, self.handle
        return self.handle

    def __exit__(self, *exc):
        global _lib
        _lib = self.prev
        return False


def view_color_shape_error(width: int, n_views: int):
    """why sr_view_color_* refuses this shape, or None (the limits of include/splatraster.h, restated so that a module can be
    refused at construction without the library)"""
    if width < 4 or width % 4 or width > VIEW_MAX_WIDTH:
        return f"the feature width must be a multiple of 4 in 4..{VIEW_MAX_WIDTH}, got {width}"
    if not (1 <= n_views <= VIEW_MAX_VIEWS):
        return f"the number of views of one call must be in 1..{VIEW_MAX_VIEWS}, got {n_views}"
    return None


def check(status: int) -> None:
    if status != 0:
        raise RuntimeError("libsplatraster: " + load().sr_last_error().decode("utf-8", "replace"))


# ---- what every caller of the library hands it: a data pointer, the stream, float32 contiguous memory ----

def ptr(t):
    """the data pointer of a tensor as a void* argument; None (NULL) for None"""
    return None if t is None else C.c_void_p(t.data_ptr())


def depth_cameras_arg(table):
    """a float64 [B, 21] DEVICE tensor as the `const SrDepthCamera*` of sr_depth_points_*: the address only, never read here"""
    return C.cast(C.c_void_p(table.data_ptr()), C.POINTER(SrDepthCamera))


def stream(device):
    """the current stream of `device` as the void* every launch takes last"""
    return C.c_void_p(torch.cuda.current_stream(device).cuda_stream)


def f32c(t):
    """detached, float32, contiguous: the tensor's own memory when it already is both"""
    t = t.detach()
    if t.dtype is not torch.float32 or not t.is_contiguous():
        t = t.to(torch.float32).contiguous()
    return t
