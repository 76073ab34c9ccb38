"""MI355X-native differentiable Gaussian-splat rasterizer behind SplatFields' render() boundary."""
from .rasterizer import GaussianRasterizationSettings, GaussianRasterizer, rasterize_gaussians, rasterize_views  # noqa: F401
from .render import render, render_views  # noqa: F401
from .losses import (centered_position_norm, depth_l1_loss, l1_loss, opacity_regularizer, photometric_loss, position_norm,  # noqa: F401
                     splat_regularizers, ssim, training_objective)
from .metrics import LPIPSWeights, compute_psnr, compute_ssim, eval_lpips, image_metrics, lpips_vgg, psnr  # noqa: F401
from .moran import knn_graph, moran_loss, morans_loss, morans_measure, query_nn  # noqa: F401
from .optim import SplatAdam  # noqa: F401
from .network_optim import NetworkAdam, network_optimizer, set_network_optimizer  # noqa: F401
from .fused_mlp import heads, mlp_precision, set_heads, set_mlp_precision  # noqa: F401
from .flow_head import flow_head_path, fused_flow_head, set_flow_head  # noqa: F401
from .view_color import fused_view_color, set_view_color, view_color_path  # noqa: F401
from .init import (depth_point_cloud, depth_points, depth_points_bounds, gen_3dpoints, hull_filter, hull_matrices,  # noqa: F401
                   splats_from_points, visual_hull, visual_hull_samples, visual_hull_samples_list)
from .subset import draw_rows, gather_rows, get_gaussian_dict  # noqa: F401
from .densify_stats import densification_stats  # noqa: F401
from .plane_generator import Tensorial2D, TimeVAEDecoder, VarTriPlaneEncoder, fused_attention, fused_layer, generate_planes, set_attention  # noqa: F401
