"""Counterpart of the reference's render boundary, gaussian_renderer/__init__.py:30-124.

Same signature, same ``gaussian_dict`` keys in, same result dict out
(``render, viewspace_points, visibility_filter, radii, opacity, depth``).  Two differences, both
inside the boundary: (1) the alpha image comes out of the same rasterization (fused output) instead
of a second full pass with white colours on a black background (:104-115) -- identical values, half
the work; ``two_pass=True`` reproduces the reference's call pattern literally; (2) the device of the
screen-space dummy follows ``means3D`` instead of the literal "cuda" (:49).  Opt-in: a ``gaussian_rgb_fnc`` that is the
network's ``ViewColor`` object on its fused path is asked for the view's colours in one launch instead of :44-46's ops."""
from __future__ import annotations

import torch

from . import rasterizer as _rz
from .rasterizer import GaussianRasterizer, settings_from_camera


def render(viewpoint_camera, gaussian_dict: dict, pipe, bg_color: torch.Tensor, scaling_modifier=1.0,
           return_opacity=True, two_pass=False):
    means3D = gaussian_dict['means3D']
    active_sh_degree = gaussian_dict['active_sh_degree']
    gaussian_opacity = gaussian_dict['gaussian_opacity']
    gaussian_scales = gaussian_dict['gaussian_scales']
    gaussian_rotations = gaussian_dict['gaussian_rotations']
    gaussian_features = gaussian_dict.get('gaussian_features', None)
    gaussian_rgb = gaussian_dict.get('gaussian_rgb', None)
    rgb_fnc = gaussian_dict.get('gaussian_rgb_fnc', None) if gaussian_rgb is None else None
    if rgb_fnc is not None and hasattr(rgb_fnc, "for_cameras") and getattr(rgb_fnc, "path", None) == "fused":
        # the view-dependent head on its kernels (splatfields_amd/view_color.py): directions, linear and sigmoid in one launch
        gaussian_rgb = rgb_fnc.for_cameras(means3D, viewpoint_camera.camera_center[None])[0]
    elif gaussian_rgb is None and 'gaussian_rgb_fnc' in gaussian_dict:
        ray_d = means3D - viewpoint_camera.camera_center[None]
        ray_d = ray_d / torch.norm(ray_d, dim=-1, keepdim=True)
        gaussian_rgb = gaussian_dict['gaussian_rgb_fnc'](ray_d)

    # zero tensor whose gradient is dL/d(screen-space mean); non-leaf + retain_grad as at :49-53
    screenspace_points = torch.zeros_like(means3D, dtype=means3D.dtype, requires_grad=True) + 0
    try:
        screenspace_points.retain_grad()
    except Exception:
        pass

    def settings(bg):
        return settings_from_camera(viewpoint_camera, bg, active_sh_degree, scaling_modifier, getattr(pipe, "debug", False))

    rasterizer = GaussianRasterizer(raster_settings=settings(bg_color))
    kw = dict(means3D=means3D, means2D=screenspace_points, shs=gaussian_features, colors_precomp=gaussian_rgb,
              opacities=gaussian_opacity, scales=gaussian_scales, rotations=gaussian_rotations, cov3D_precomp=None)
    if two_pass:   # the reference's literal calls: the three-output `forward` (:94-102), then the mask rasterizer (:104-115)
        fwd = lambda: rasterizer(**kw) + (None,)
    else:
        fwd = lambda: rasterizer.forward_ex(**kw)
    # pipe.debug: nothing leaves this function unchecked (with SPLATRASTER_ASYNC=1 a forward may have been launched on a promise:
    # rasterizer.redeemed renders one whose promise did not hold again)
    rendered_image, radii, depth, alpha = _rz.redeemed(fwd) if getattr(pipe, "debug", False) else fwd()
    opacity_image = None
    if return_opacity:
        if two_pass:
            rasterizer_mask = GaussianRasterizer(raster_settings=settings(bg_color * 0.0))
            opacity_image = rasterizer_mask(
                means3D=means3D, means2D=screenspace_points, shs=None,
                colors_precomp=torch.ones(gaussian_opacity.shape[0], 3, device=gaussian_opacity.device),
                opacities=gaussian_opacity, scales=gaussian_scales, rotations=gaussian_rotations,
                cov3D_precomp=None)[0][:1]
        else:
            opacity_image = alpha
    return {"render": rendered_image, "viewspace_points": screenspace_points, "visibility_filter": radii > 0,
            "radii": radii, "opacity": opacity_image, "depth": depth}


def render_views(cameras, gaussian_dict: dict, pipe, bg_color: torch.Tensor, scaling_modifier=1.0, return_opacity=True):
    """``render`` for the V views of one training step (reference train.py:158-177 renders them one by one and back-propagates
    once) in one rasterizer call: one host wait for the instance counts of all views instead of one per view, and one launch
    that adds the views' gradients of the shared inputs instead of an autograd add per input and view.  Same ``gaussian_dict``;
    the result dict holds the stacked tensors ``render`` [V,3,H,W], ``depth`` [V,1,H,W], ``opacity`` [V,1,H,W] (or None),
    ``radii`` [V,N] int32, ``visibility_filter`` [V,N] bool and ``viewspace_points`` [V,N,3] with a retained gradient -- row v of
    each is what ``render(cameras[v], ...)`` returns, bit for bit, and so is every gradient (dL/dshs up to rounding: it is summed
    over the views by one SH backward launch).  ``losses.training_objective`` takes the stacked tensors as they are.

    All cameras share one image size (group them by shape otherwise).  ``bg_color``: [3], or [V,3] for a background per view.
    ``gaussian_rgb``: [N,3] for colours the views share, or [V,N,3] for a colour per view (its gradient is written in place);
    a ``gaussian_rgb_fnc`` is evaluated for all views at once when it is the network's ``ViewColor`` on its fused path."""
    cameras = list(cameras)
    if not cameras:
        raise ValueError("render_views needs at least one camera")
    shapes = [(int(c.image_height), int(c.image_width)) for c in cameras]
    if any(s != shapes[0] for s in shapes):
        raise ValueError(f"render_views: all cameras of one call share one image size, got (H, W) = {shapes}: group the cameras by shape")
    V = len(cameras)
    means3D = gaussian_dict['means3D']
    active_sh_degree = gaussian_dict['active_sh_degree']
    gaussian_features = gaussian_dict.get('gaussian_features', None)
    gaussian_rgb = gaussian_dict.get('gaussian_rgb', None)
    if gaussian_rgb is None and gaussian_dict.get('gaussian_rgb_fnc', None) is not None:
        rgb_fnc = gaussian_dict['gaussian_rgb_fnc']
        if hasattr(rgb_fnc, "for_cameras") and getattr(rgb_fnc, "path", None) == "fused":
            gaussian_rgb = rgb_fnc.for_cameras(means3D, torch.stack([c.camera_center for c in cameras]))
        else:   # the reference's expression (gaussian_renderer/__init__.py:44-46), view by view
            per_view = []
            for cam in cameras:
                ray_d = means3D - cam.camera_center[None]
                ray_d = ray_d / torch.norm(ray_d, dim=-1, keepdim=True)
                per_view.append(rgb_fnc(ray_d))
            gaussian_rgb = torch.stack(per_view)
    if bg_color.dim() == 2 and bg_color.shape[0] != V:
        raise ValueError(f"render_views: bg_color must be [3] or [V,3] = {(V, 3)}, got {tuple(bg_color.shape)}")

    screenspace_points = torch.zeros((V,) + tuple(means3D.shape), dtype=means3D.dtype, device=means3D.device, requires_grad=True) + 0
    try:
        screenspace_points.retain_grad()
    except Exception:
        pass
    debug = getattr(pipe, "debug", False)
    settings = [settings_from_camera(cam, bg_color if bg_color.dim() == 1 else bg_color[v], active_sh_degree, scaling_modifier, debug)
                for v, cam in enumerate(cameras)]
    rendered, radii, depth, alpha = _rz.rasterize_views(
        means3D, screenspace_points, gaussian_features, gaussian_rgb, gaussian_dict['gaussian_opacity'],
        gaussian_dict['gaussian_scales'], gaussian_dict['gaussian_rotations'], None, settings)
    return {"render": rendered, "viewspace_points": screenspace_points, "visibility_filter": radii > 0, "radii": radii,
            "opacity": alpha if return_opacity else None, "depth": depth}


def render_model(viewpoint_camera, gaussians, pipe, bg_color: torch.Tensor, scaling_modifier=1.0, return_opacity=True):
    """``render`` for the static / warm-up branch of reference train.py:41-50, taking the ``GaussianModel`` itself instead
    of the dict of its accessors: the raw parameters (``_xyz, _features_dc, _features_rest, _opacity, _scaling, _rotation``,
    scene/gaussian_model.py:38-46) go to the rasterizer as they are stored, and ``exp`` / ``sigmoid`` / ``normalize`` /
    ``cat`` (:64-86) happen inside its preprocess kernels (``GaussianRasterizer.forward_raw``).  Same result dict as
    ``render``; gradients arrive on the raw parameters."""
    means3D = gaussians._xyz
    log_scales = gaussians._scaling
    if log_scales.shape[-1] == 1:  # use_isotropic (gaussian_model.py:64-68): the accessor repeats the single scale
        log_scales = log_scales.expand(-1, 3)
    screenspace_points = torch.zeros_like(means3D, dtype=means3D.dtype, requires_grad=True) + 0
    try:
        screenspace_points.retain_grad()
    except Exception:
        pass
    rs = settings_from_camera(viewpoint_camera, bg_color, int(gaussians.active_sh_degree), scaling_modifier,
                              getattr(pipe, "debug", False))
    dc, rest = gaussians._features_dc, gaussians._features_rest
    if rest.shape[1] == 15:
        kw = dict(shs=dc, shs_rest=rest)
    else:  # other SH widths: the concatenated tensor, as the accessor builds it
        kw = dict(shs=torch.cat((dc, rest), dim=1))
    fwd = lambda: GaussianRasterizer(raster_settings=rs).forward_raw(
        means3D=means3D, means2D=screenspace_points, opacity_logits=gaussians._opacity, log_scales=log_scales,
        quaternions=gaussians._rotation, **kw)
    rendered_image, radii, depth, alpha = _rz.redeemed(fwd) if getattr(pipe, "debug", False) else fwd()
    return {"render": rendered_image, "viewspace_points": screenspace_points, "visibility_filter": radii > 0,
            "radii": radii, "opacity": alpha if return_opacity else None, "depth": depth}
