"""The view-dependent colour head on its HIP kernels (include/splatraster.h: sr_view_color_*; csrc/view_color.hip).

`fused_view_color(feature, weight, bias, means3D=..., camera_centers=...)` evaluates what reference
gaussian_renderer/__init__.py:43-46 evaluates once per view around utils/time_utils.py:496 --

    ray_d = normalize(means3D - camera_center);  colour = sigmoid(Linear(F + 3 -> 3)(cat[feature, ray_d]))

-- for ALL V views of a step in ONE launch that reads the [N, F] feature once, and is differentiable: the backward is one kernel
that writes dL/dfeature once (the sum over the views times W[:, :F]), dL/dmeans3D (summed in view order), the per-point sum of
dL/dz and one partial sum of dW[:, F:] and db per workgroup (doubles, workgroup = 256 consecutive points, whatever the device), plus
one weight_grad.run call (two kernels) for dW[:, :F].  With `dirs=[V, N, 3]` instead of the camera centres the directions
are taken as given and receive the gradient (V = 1: the reference's `rgb_fnc(viewdir)`).  float32 tensors, double arithmetic
inside the kernels, one rounding per stored value, no atomics, no host wait: repeated calls are bit-identical.  No CPU path.
The one limit: a point that coincides with a camera centre gives non-finite values in that view, as in the reference.

More than VIEW_MAX_VIEWS (16) views are evaluated in chunks of 16, one forward and one backward launch per chunk, and the chunks'
gradients are added in chunk order.

Opt-in: `SplatFields(view_color="fused")`, `set_view_color("fused")` or SPLATFIELDS_VIEW_COLOR=fused; the process default is
"torch" (the PyTorch ops of splatfields_amd/deform_field.py and render.py)."""
from __future__ import annotations

import os
from typing import Optional

import torch

from . import _lib, weight_grad

VIEW_COLORS = ("torch", "fused")
VIEW_COLOR_LAUNCHES = (1, 3)     # library kernels of the "fused" head for up to 16 views: (forward, backward: its own + weight_grad.run's two)


def checked_view_color(name) -> str:
    if name not in VIEW_COLORS:
        raise ValueError(f"unknown view-colour path {name!r}: expected one of {VIEW_COLORS}")
    return name


# process default of the view-dependent colour head, read once: SPLATFIELDS_VIEW_COLOR=fused turns the HIP kernels on for every
# network that does not name a path itself
_VIEW_COLOR = checked_view_color(os.environ.get("SPLATFIELDS_VIEW_COLOR") or "torch")


def set_view_color(name: str) -> str:
    """Process default of the view-dependent colour head: "torch" (PyTorch ops) or "fused" (csrc/view_color.hip).  Returns the
    previous setting."""
    global _VIEW_COLOR
    prev, _VIEW_COLOR = _VIEW_COLOR, checked_view_color(name)
    return prev


def view_color_path() -> str:
    return _VIEW_COLOR


def resolve_view_color(name: Optional[str]) -> str:
    """`None` -> the process default, at call time."""
    return _VIEW_COLOR if name is None else checked_view_color(name)


def _chunks(n_views):
    return [(lo, min(lo + _lib.VIEW_MAX_VIEWS, n_views)) for lo in range(0, n_views, _lib.VIEW_MAX_VIEWS)]


class _ViewColorFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, mode, grad_enabled, feature, weight, bias, pos, cams):
        """pos: means3D [N, 3] with cams [V, 3] (VIEW_FROM_CAMERAS), or dirs [V, N, 3] with cams None (VIEW_DIRS_GIVEN)"""
        lib = _lib.load()
        feature, weight, bias, pos = _lib.f32c(feature), _lib.f32c(weight), _lib.f32c(bias), _lib.f32c(pos)
        cams = _lib.f32c(cams) if cams is not None else None
        dev, n, width = feature.device, feature.shape[0], feature.shape[1]
        n_views = cams.shape[0] if mode == _lib.VIEW_FROM_CAMERAS else pos.shape[0]
        colours = torch.empty(n_views, n, 3, dtype=torch.float32, device=dev)
        need = grad_enabled and any(ctx.needs_input_grad)
        saved = None
        if need:
            size = lib.sr_view_color_saved_bytes(n, width, 1)
            if size == 0:
                raise ValueError("fused view colour: unsupported shape: " + (_lib.view_color_shape_error(width, 1) or "too many points"))
            saved = torch.empty(size // 8, dtype=torch.float64, device=dev)
        means = pos if mode == _lib.VIEW_FROM_CAMERAS else None
        per_view = cams if mode == _lib.VIEW_FROM_CAMERAS else pos
        with torch.cuda.device(dev):
            for i, (lo, hi) in enumerate(_chunks(n_views)):      # the view-independent part is the same in every chunk: saved once
                _lib.check(lib.sr_view_color_forward(mode, n, width, hi - lo, _lib.ptr(feature), _lib.ptr(means), _lib.ptr(per_view[lo:hi]),
                                                     _lib.ptr(weight), _lib.ptr(bias), _lib.ptr(colours[lo:hi]),
                                                     _lib.ptr(saved) if i == 0 else None, _lib.stream(dev)))
        if need:
            ctx.mode, ctx.n_views = mode, n_views
            ctx.save_for_backward(feature, weight, pos, cams, saved)
        return colours

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g_colours):
        lib = _lib.load()
        mode, n_views = ctx.mode, ctx.n_views
        feature, weight, pos, cams, saved = ctx.saved_tensors
        dev, n, width = feature.device, feature.shape[0], feature.shape[1]
        need_feature, need_weight, need_bias, need_pos = ctx.needs_input_grad[2:6]
        g_colours = _lib.f32c(g_colours)
        means = pos if mode == _lib.VIEW_FROM_CAMERAS else None
        per_view = cams if mode == _lib.VIEW_FROM_CAMERAS else pos
        d_pos = torch.empty_like(pos) if need_pos else None
        blocks = (n + 255) // 256
        ws_bytes = lib.sr_view_color_workspace_bytes(n, width, 1)
        total = None
        for lo, hi in _chunks(n_views):
            dz = torch.empty(weight_grad.dz_rows(n), 4, dtype=torch.float32, device=dev)      # the kernel's layout: [N + 1, 4]
            d_feature = torch.empty_like(feature) if need_feature else None
            ws = torch.empty(ws_bytes // 8, dtype=torch.float64, device=dev)
            if mode == _lib.VIEW_FROM_CAMERAS:
                d_out = (d_pos if total is None else torch.empty_like(pos)) if need_pos else None
            else:
                d_out = d_pos[lo:hi] if need_pos else None
            with torch.cuda.device(dev):
                _lib.check(lib.sr_view_color_backward(mode, n, width, hi - lo, _lib.ptr(means), _lib.ptr(per_view[lo:hi]), _lib.ptr(weight),
                                                      _lib.ptr(saved), _lib.ptr(g_colours[lo:hi]), _lib.ptr(d_feature), _lib.ptr(d_out),
                                                      _lib.ptr(dz), _lib.ptr(ws), _lib.stream(dev)))
            if total is None:
                total = (dz, d_feature, ws)
            else:      # more than 16 views: the chunks are added in chunk order
                total[0][:n].add_(dz[:n])
                total[2][: blocks * 12].add_(ws[: blocks * 12])
                if need_feature:
                    total[1].add_(d_feature)
                if need_pos and mode == _lib.VIEW_FROM_CAMERAS:
                    d_pos.add_(d_out)
        dz, d_feature, ws = total
        d_weight, d_bias = None, None
        if need_weight or need_bias:
            d_weight = _weight_grads(feature, dz, n)
            # one partial per workgroup of 256 consecutive points: the shape alone fixes the order of this sum
            sums = ws[: blocks * 12].view(blocks, 12).sum(0)
            d_weight[:, width:] = sums[:9].view(3, 3)
            d_bias = sums[9:].float()
        return (None, None, d_feature, d_weight if need_weight else None, d_bias if need_bias else None, d_pos, None)


def _weight_grads(feature, dz, n):
    """dW[:, :F] = dz^T feature written into a [3, F + 3] matrix (the job's dw_row addresses it directly) by one weight_grad.run
    job; the columns behind F are left as allocated, for the caller to fill."""
    width = feature.shape[1]
    dW = torch.empty(3, width + 3, dtype=torch.float32, device=feature.device)
    weight_grad.run(n, feature.device, weight_grad.job_list(((4, 3, width, width, width + 3, 0),)), [dz.data_ptr()], [feature.data_ptr()],
                    [dW], [None])
    return dW


def fused_view_color(feature: torch.Tensor, weight: torch.Tensor, bias: torch.Tensor, *, means3D: Optional[torch.Tensor] = None,
                     camera_centers: Optional[torch.Tensor] = None, dirs: Optional[torch.Tensor] = None) -> torch.Tensor:
    """-> colours [V, N, 3] of the reference's view-dependent head for V views: feature [N, F], weight [3, F + 3] and bias [3] as
    `nn.Linear(F + 3, 3)` holds them over cat([feature, viewdir]); either means3D [N, 3] with camera_centers [V, 3] (the
    directions are normalize(means3D - centre), the gradient goes to means3D) or dirs [V, N, 3] (taken as given, and
    differentiable).  Differentiable in feature, weight, bias and means3D / dirs, not in camera_centers; tensors live on a HIP
    device; float64 / autocast inputs are converted to float32 at the boundary (the results are float32)."""
    if (dirs is None) == (means3D is None and camera_centers is None) or (means3D is None) != (camera_centers is None):
        raise ValueError("fused_view_color takes either means3D [N, 3] with camera_centers [V, 3], or dirs [V, N, 3]")
    if not feature.is_cuda:
        raise RuntimeError("fused_view_color has no CPU path: tensors must be on a HIP ('cuda') device")
    if feature.dim() != 2 or tuple(weight.shape) != (3, feature.shape[1] + 3) or tuple(bias.shape) != (3,):
        raise ValueError("feature must be [N, F], weight [3, F + 3] and bias [3]")
    n = feature.shape[0]
    if dirs is not None:
        if dirs.dim() != 3 or dirs.shape[1] != n or dirs.shape[2] != 3 or dirs.shape[0] < 1:
            raise ValueError("dirs must be [V, N, 3] with V >= 1")
        mode, pos, cams = _lib.VIEW_DIRS_GIVEN, dirs, None
    else:
        if tuple(means3D.shape) != (n, 3) or camera_centers.dim() != 2 or camera_centers.shape[1] != 3 or camera_centers.shape[0] < 1:
            raise ValueError("means3D must be [N, 3] and camera_centers [V, 3] with V >= 1")
        if camera_centers.requires_grad:
            raise ValueError("fused_view_color is not differentiable in camera_centers (the reference never differentiates them): detach them")
        mode, pos, cams = _lib.VIEW_FROM_CAMERAS, means3D, camera_centers
    why = _lib.view_color_shape_error(feature.shape[1], 1)
    if why:
        raise ValueError("fused_view_color: " + why)
    for t in (weight, bias, pos, cams):
        if t is not None and t.device != feature.device:
            raise RuntimeError("fused_view_color has no CPU path: every tensor must be on the device of `feature`")
    n_views = pos.shape[0] if cams is None else cams.shape[0]
    with torch.autocast("cuda", enabled=False):
        f32 = lambda t: t if t.dtype is torch.float32 else t.float()      # differentiable: gradients return in the caller's dtype
        feature, weight, bias, pos = f32(feature), f32(weight), f32(bias), f32(pos)
        if n == 0:      # nothing to launch; keep the graph connected so that parameters still receive (zero) gradients
            zero = 0.0 * (feature.sum() + weight.sum() + bias.sum() + pos.sum())
            return feature.new_zeros(n_views, 0, 3) + zero
        return _ViewColorFn.apply(mode, torch.is_grad_enabled(), feature, weight, bias, pos, cams)
