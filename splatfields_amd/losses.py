"""The photometric loss of a training step on the device: the reference's ``l1_loss`` / ``ssim`` (utils/loss_utils.py:18,
:45-76) as drop-ins, and lines 183-193 of its train.py as one fused call.

The reference writes, per view,

    Ll1  = l1_loss(image, gt_image)
    loss = (1.0 - lambda_dssim) * Ll1 + lambda_dssim * (1.0 - ssim(image, gt_image))
    loss += lambda_mask * F.l1_loss(torch.clamp(opacity, 0, 1).view(-1), gt_mask.view(-1))

which is five depthwise 11x11 convolutions, about thirty element-wise kernels and three reductions, and as many again in the
backward.  ``photometric_loss`` is one kernel and a fixed-order reduction forward (``sr_photometric_forward``) and one kernel
backward (``sr_photometric_backward``): no host synchronisation, no floating-point atomics, bit-identical results from call
to call.  There is no CPU path."""
from __future__ import annotations

from typing import Optional

import torch

from . import _lib
from ._lib import f32c, ptr

WINDOW_SIZE = 11   # the kernels are built for the reference's window: 11 taps, sigma 1.5

_FUSED, _L1, _SSIM = 0, 1, 2


def _run_forward(x, y, a, m, shape, lambda_dssim, lambda_mask, with_ssim, with_maps):
    """Enqueues sr_photometric_forward on the current stream of x's device; float32 contiguous tensors in, (loss, l1, ssim [batch],
    mask_l1, maps or None) out, all on the device."""
    lib = _lib.load()
    batch, channels, h, w = shape
    dev = x.device
    with torch.cuda.device(dev):
        work = torch.empty(lib.sr_loss_workspace_bytes(batch * channels, h, w), dtype=torch.uint8, device=dev)
        out = torch.empty(3 + batch, dtype=torch.float32, device=dev)   # loss | l1 | mask_l1 (written with a mask only) | ssim [batch]
        maps = torch.empty((3,) + tuple(x.shape), dtype=torch.float32, device=dev) if with_maps else None
        ssim_out = out[3:] if with_ssim else None
        _lib.check(lib.sr_photometric_forward(batch, channels, h, w, ptr(x), ptr(y), ptr(a), ptr(m), float(lambda_dssim),
                                              float(lambda_mask), ptr(work), ptr(maps), ptr(out[0:1]), ptr(out[1:2]),
                                              ptr(ssim_out), ptr(out[2:3]) if a is not None else None, _lib.stream(dev)))
    return out[0], out[1], out[3:], out[2], maps


class _Photometric(torch.autograd.Function):
    """One differentiable output per mode -- the blended loss, l1, or the per-item structural similarity -- and the other terms
    as detached tensors.  Gradients flow to `image` and `opacity` only."""

    @staticmethod
    def forward(ctx, image, gt, opacity, gt_mask, mode, shape, lambda_dssim, lambda_mask):
        x, y = f32c(image), f32c(gt)
        a = None if opacity is None else f32c(opacity)
        m = None if gt_mask is None else f32c(gt_mask)
        with_ssim = mode != _L1
        loss, l1, ssim_items, mask_l1, maps = _run_forward(x, y, a, m, shape, lambda_dssim, lambda_mask, with_ssim, with_maps=with_ssim)
        ctx.save_for_backward(x, y, a, m, maps)
        ctx.set_materialize_grads(False)    # no zero tensors for the detached outputs' gradients
        ctx.mode, ctx.shape = mode, shape
        ctx.weights = {_FUSED: (1.0 - lambda_dssim, -lambda_dssim, lambda_mask), _L1: (1.0, 0.0, 0.0), _SSIM: (0.0, 1.0, 0.0)}[mode]
        ctx.image_meta = (image.shape, image.dtype)
        ctx.opacity_meta = None if opacity is None else (opacity.shape, opacity.dtype)
        dt = image.dtype
        outs = [loss.to(dt), l1.to(dt), ssim_items.to(dt), mask_l1.to(dt)]
        ctx.mark_non_differentiable(*[o for k, o in enumerate(outs) if k != {_FUSED: 0, _L1: 1, _SSIM: 2}[mode]])
        return tuple(outs)

    @staticmethod
    def backward(ctx, g_loss, g_l1, g_ssim, g_mask):
        lib = _lib.load()
        x, y, a, m, maps = ctx.saved_tensors
        batch, channels, h, w = ctx.shape
        g = {_FUSED: g_loss, _L1: g_l1, _SSIM: g_ssim}[ctx.mode]
        if g is None:
            return (None,) * 8
        g = f32c(g)
        per_item = ctx.mode == _SSIM
        dev = x.device
        want_alpha = a is not None and ctx.needs_input_grad[2]
        with torch.cuda.device(dev):
            d_image = torch.empty_like(x)
            d_alpha = torch.empty_like(a) if want_alpha else None
            w_l1, w_ssim, w_mask = ctx.weights
            _lib.check(lib.sr_photometric_backward(batch, channels, h, w, ptr(x), ptr(y), ptr(a), ptr(m), ptr(maps), w_l1, w_ssim,
                                                   w_mask, ptr(g), int(per_item), ptr(d_image), ptr(d_alpha), _lib.stream(dev)))
        shape, dt = ctx.image_meta
        d_image = d_image.reshape(shape).to(dt) if ctx.needs_input_grad[0] else None
        if want_alpha:
            shape, dt = ctx.opacity_meta
            d_alpha = d_alpha.reshape(shape).to(dt)
        return d_image, None, d_alpha, None, None, None, None, None


def _check_pair(name, image, gt):
    if not isinstance(image, torch.Tensor) or not isinstance(gt, torch.Tensor):
        raise TypeError(f"{name} takes tensors")
    if not image.is_cuda or not gt.is_cuda:
        raise RuntimeError(f"{name} has no CPU path: tensors must be on a HIP ('cuda') device")
    if gt.device != image.device:
        raise RuntimeError(f"{name}: the two images must be on the same device")
    if image.shape != gt.shape:
        raise RuntimeError(f"{name}: the two images must have the same shape, got {tuple(image.shape)} and {tuple(gt.shape)}")
    if not image.is_floating_point() or image.numel() == 0:
        raise RuntimeError(f"{name}: a non-empty floating-point image is required")
    if gt.requires_grad and torch.is_grad_enabled():
        raise RuntimeError(f"{name}: the target requires grad, and no gradient is computed for it (detach it)")


def _call(image, gt, opacity, gt_mask, mode, shape, lambda_dssim, lambda_mask):
    tracked = torch.is_grad_enabled() and (image.requires_grad or (opacity is not None and opacity.requires_grad))
    if tracked:
        return _Photometric.apply(image, gt, opacity, gt_mask, mode, shape, lambda_dssim, lambda_mask)
    # nothing to differentiate: no derivative maps are written and nothing is kept
    loss, l1, ssim_items, mask_l1, _ = _run_forward(f32c(image), f32c(gt), None if opacity is None else f32c(opacity),
                                                    None if gt_mask is None else f32c(gt_mask), shape, lambda_dssim, lambda_mask,
                                                    with_ssim=mode != _L1, with_maps=False)
    dt = image.dtype
    return loss.to(dt), l1.to(dt), ssim_items.to(dt), mask_l1.to(dt)


def l1_loss(network_output: torch.Tensor, gt: torch.Tensor) -> torch.Tensor:
    """``torch.abs(network_output - gt).mean()`` (reference utils/loss_utils.py:18) for tensors of any shape."""
    _check_pair("l1_loss", network_output, gt)
    h, w = (network_output.shape[-2], network_output.shape[-1]) if network_output.dim() >= 2 else (1, network_output.numel())
    shape = (1, network_output.numel() // (h * w), h, w)
    return _call(network_output, gt, None, None, _L1, shape, 0.0, 0.0)[1]


def _image_shape(name, image):
    if image.dim() not in (3, 4):
        raise RuntimeError(f"{name}: expected a [C,H,W] or [B,C,H,W] image, got {tuple(image.shape)}")
    b = image.shape[0] if image.dim() == 4 else 1
    return b, image.shape[-3], image.shape[-2], image.shape[-1]


def ssim(img1: torch.Tensor, img2: torch.Tensor, window_size: int = 11, size_average: bool = True) -> torch.Tensor:
    """The reference's ``ssim`` (utils/loss_utils.py:45-76): mean structural similarity of [C,H,W] or [B,C,H,W] images, a
    0-dim tensor, or [B] with ``size_average=False``.  Differentiable in ``img1``."""
    if window_size != WINDOW_SIZE:
        raise ValueError(f"ssim: the kernel is built for the reference's window of {WINDOW_SIZE} taps (sigma 1.5), got window_size={window_size}")
    _check_pair("ssim", img1, img2)
    b, c, h, w = _image_shape("ssim", img1)
    if size_average:
        return _call(img1, img2, None, None, _SSIM, (1, b * c, h, w), 0.0, 0.0)[2].reshape(())
    items = _call(img1, img2, None, None, _SSIM, (b, c, h, w), 0.0, 0.0)[2]
    return items if img1.dim() == 4 else items.reshape(())


def photometric_loss(image: torch.Tensor, gt_image: torch.Tensor, lambda_dssim: float = 0.2, opacity: Optional[torch.Tensor] = None,
                     gt_mask: Optional[torch.Tensor] = None, lambda_mask: float = 0.0, return_terms: bool = False):
    """Lines 183-193 of the reference's train.py as one forward and one backward launch:

        loss = (1 - lambda_dssim) * l1_loss(image, gt_image) + lambda_dssim * (1 - ssim(image, gt_image))
               + lambda_mask * F.l1_loss(clamp(opacity, 0, 1).view(-1), gt_mask.view(-1))        # when opacity / gt_mask are given

    Returns ``(loss, Ll1)``, ``Ll1`` detached (the reference only logs it); with ``return_terms`` also a dict of the detached
    ``ssim`` and ``mask`` terms (``mask`` is None without an opacity).  Gradients flow to ``image`` and ``opacity``."""
    _check_pair("photometric_loss", image, gt_image)
    shape = _image_shape("photometric_loss", image)
    if (opacity is None) != (gt_mask is None):
        raise RuntimeError("photometric_loss: opacity and gt_mask go together (both or neither)")
    if opacity is None and lambda_mask != 0.0:
        raise RuntimeError("photometric_loss: lambda_mask without opacity and gt_mask")
    if opacity is not None:
        for name, t in (("opacity", opacity), ("gt_mask", gt_mask)):
            if not t.is_cuda or t.device != image.device:
                raise RuntimeError(f"photometric_loss has no CPU path: {name} must be on the image's HIP ('cuda') device")
            if t.numel() != shape[0] * shape[2] * shape[3]:
                raise RuntimeError(f"photometric_loss: {name} must have one value per pixel, got {tuple(t.shape)} for an image {tuple(image.shape)}")
        if gt_mask.requires_grad and torch.is_grad_enabled():
            raise RuntimeError("photometric_loss: the target requires grad, and no gradient is computed for it (detach it)")
    loss, l1, ssim_items, mask_l1 = _call(image, gt_image, opacity, gt_mask, _FUSED, shape, float(lambda_dssim), float(lambda_mask))
    if return_terms:
        return loss, l1, {"ssim": ssim_items.mean() if shape[0] > 1 else ssim_items.reshape(()),
                          "mask": mask_l1 if opacity is not None else None}
    return loss, l1


# ---------------------------------------------------------------------------------------------------------------------------
# The tail of the objective (reference train.py:195-201, :224-229, :244-246) and the objective of a step (:165-250):
# sr_splat_reg_* and sr_depth_l1_* (csrc/objective.hip).  A streaming pass and a fixed-order reduction forward, one kernel
# backward; no host synchronisation, no floating-point atomics, bit-identical results from call to call.  No CPU path.

def _empty_in_phase(t: torch.Tensor) -> torch.Tensor:
    """An uninitialised float32 tensor of t's shape whose address agrees with t's modulo 16 (t: float32, contiguous): the
    kernels then store a gradient in the same 16-byte vectors they load its input in, whatever t's storage offset."""
    lead = (t.data_ptr() >> 2) & 3
    if lead == 0:
        return torch.empty_like(t)
    return torch.empty(t.numel() + lead, dtype=torch.float32, device=t.device)[lead:].view(t.shape)


def _nan_like_graph(t: torch.Tensor) -> torch.Tensor:
    """The mean of an empty tensor, as the reference's expressions give it: NaN, still a function of t."""
    return t.sum() * float("nan")


def _run_splat_reg(x, o, weights):
    """Enqueues sr_splat_reg_forward on the current stream: float32 contiguous tensors (or None) in, out[8] on the device =
    loss | norm | norm_mean | opacity_reg | mean (3) | 0."""
    lib = _lib.load()
    first = x if x is not None else o
    n, dev = first.shape[0], first.device
    with torch.cuda.device(dev):
        work = torch.empty(lib.sr_splat_reg_workspace_bytes(n), dtype=torch.uint8, device=dev)
        out = torch.empty(8, dtype=torch.float32, device=dev)
        _lib.check(lib.sr_splat_reg_forward(n, ptr(x), ptr(o), *weights, ptr(work), ptr(out), _lib.stream(dev)))
    return out


class _SplatReg(torch.autograd.Function):
    """loss = lambda_norm * norm + lambda_norm_mean * norm_mean + lambda_opacity * opacity_reg, differentiable, and the three
    terms, detached.  Gradients flow to `means3D` and `opacity`."""

    @staticmethod
    def forward(ctx, means3D, opacity, weights):
        x = None if means3D is None else f32c(means3D)
        o = None if opacity is None else f32c(opacity)
        out = _run_splat_reg(x, o, weights)
        n = (x if x is not None else o).shape[0]
        ctx.save_for_backward(x, o, out)
        ctx.set_materialize_grads(False)
        ctx.weights, ctx.n = weights, n
        ctx.x_meta = None if means3D is None else (means3D.shape, means3D.dtype)
        ctx.o_meta = None if opacity is None else (opacity.shape, opacity.dtype)
        dt = (means3D if x is not None else opacity).dtype
        outs = [out[0].to(dt), out[1].to(dt), out[2].to(dt), out[3].to(dt)]
        ctx.mark_non_differentiable(*outs[1:])
        return tuple(outs)

    @staticmethod
    def backward(ctx, g_loss, g_norm, g_norm_mean, g_opacity):
        if g_loss is None:
            return None, None, None
        lib = _lib.load()
        x, o, out = ctx.saved_tensors
        lam_n, lam_nm, lam_o = ctx.weights
        want_x = x is not None and ctx.needs_input_grad[0]
        want_o = o is not None and ctx.needs_input_grad[1]
        if not want_x and not want_o:
            return None, None, None
        g = f32c(g_loss)
        dev = out.device
        with torch.cuda.device(dev):
            d_x = _empty_in_phase(x) if want_x else None
            d_o = _empty_in_phase(o) if want_o else None
            _lib.check(lib.sr_splat_reg_backward(ctx.n, ptr(x), ptr(o), lam_n, lam_nm, lam_o, ptr(out), ptr(g), ptr(d_x), ptr(d_o), _lib.stream(dev)))
        if want_x:
            shape, dt = ctx.x_meta
            d_x = d_x.reshape(shape).to(dt)
        if want_o:
            shape, dt = ctx.o_meta
            d_o = d_o.reshape(shape).to(dt)
        return d_x, d_o, None


def _check_splats(name, means3D, opacity):
    for what, t in (("means3D", means3D), ("opacity", opacity)):
        if t is None:
            continue
        if not isinstance(t, torch.Tensor):
            raise TypeError(f"{name} takes tensors")
        if not t.is_cuda:
            raise RuntimeError(f"{name} has no CPU path: {what} must be on a HIP ('cuda') device")
        if not t.is_floating_point():
            raise RuntimeError(f"{name}: {what} must be a floating-point tensor")
    if means3D is not None and (means3D.dim() != 2 or means3D.shape[1] != 3):
        raise RuntimeError(f"{name}: means3D must be [N,3], got {tuple(means3D.shape)}")
    if opacity is not None and not (opacity.dim() == 1 or (opacity.dim() == 2 and opacity.shape[1] == 1)):
        raise RuntimeError(f"{name}: opacity must be [N] or [N,1], got {tuple(opacity.shape)}")
    if means3D is not None and opacity is not None:
        if opacity.shape[0] != means3D.shape[0]:
            raise RuntimeError(f"{name}: {means3D.shape[0]} rows of means3D and {opacity.shape[0]} opacities")
        if opacity.device != means3D.device:
            raise RuntimeError(f"{name}: means3D and opacity must be on the same device")


def splat_regularizers(means3D: Optional[torch.Tensor], opacity: Optional[torch.Tensor] = None, lambda_norm: float = 0.0,
                       lambda_norm_mean: float = 0.0, lambda_opacity: float = 0.0):
    """The splat terms of the reference's objective in one fused forward and one backward launch:

        loss = lambda_norm * means3D.norm(dim=1).mean()                                               # train.py:195-197
             + lambda_norm_mean * (means3D - means3D.detach().mean(0, keepdim=True)).norm(dim=1).mean()   # train.py:198-201
             + lambda_opacity * ((opacity - 1.0) ** 2).mean()                                          # train.py:244-246

    Returns ``(loss, terms)``: ``terms`` holds the detached device scalars ``norm``, ``norm_mean`` and ``opacity`` of the terms
    that were asked for.  A term with weight 0 is skipped, not computed.  Gradients flow to ``means3D`` and ``opacity``."""
    weights = (float(lambda_norm), float(lambda_norm_mean), float(lambda_opacity))
    need_x, need_o = weights[0] != 0.0 or weights[1] != 0.0, weights[2] != 0.0
    if need_x and means3D is None:
        raise RuntimeError("splat_regularizers: lambda_norm / lambda_norm_mean without means3D")
    if need_o and opacity is None:
        raise RuntimeError("splat_regularizers: lambda_opacity without opacity")
    if not need_x and not need_o:
        raise RuntimeError("splat_regularizers: every weight is 0, there is nothing to compute")
    _check_splats("splat_regularizers", means3D if need_x else None, opacity if need_o else None)
    first = means3D if need_x else opacity
    names = [k for k, on in (("norm", weights[0] != 0.0), ("norm_mean", weights[1] != 0.0), ("opacity", weights[2] != 0.0)) if on]
    if first.shape[0] == 0:      # the mean of nothing
        loss = _nan_like_graph(first)
        return loss, {k: loss.detach() for k in names}
    x, o = (means3D if need_x else None), (opacity if need_o else None)
    if torch.is_grad_enabled() and ((x is not None and x.requires_grad) or (o is not None and o.requires_grad)):
        loss, norm, norm_mean, opacity_reg = _SplatReg.apply(x, o, weights)
    else:       # nothing to differentiate: nothing is kept
        out = _run_splat_reg(None if x is None else f32c(x), None if o is None else f32c(o), weights).to(first.dtype)
        loss, norm, norm_mean, opacity_reg = out[0], out[1], out[2], out[3]
    values = {"norm": norm, "norm_mean": norm_mean, "opacity": opacity_reg}
    return loss, {k: values[k] for k in names}


def position_norm(means3D: torch.Tensor) -> torch.Tensor:
    """``means3D.norm(dim=1).mean()`` (reference train.py:196), differentiable."""
    return splat_regularizers(means3D, lambda_norm=1.0)[0]


def centered_position_norm(means3D: torch.Tensor) -> torch.Tensor:
    """``(means3D - means3D.detach().mean(dim=0, keepdim=True)).norm(dim=1).mean()`` (reference train.py:199-200)."""
    return splat_regularizers(means3D, lambda_norm_mean=1.0)[0]


def opacity_regularizer(opacity: torch.Tensor) -> torch.Tensor:
    """``((opacity - 1.0) ** 2).mean()`` (reference train.py:245) for the [N,1] (or [N]) opacities."""
    return splat_regularizers(None, opacity, lambda_opacity=1.0)[0]


def _run_depth_l1(d, g, shape):
    """Enqueues sr_depth_l1_forward on the current stream: float32 contiguous tensors in, out[1 + batch] on the device = the
    mean over everything | the mean per item."""
    lib = _lib.load()
    batch, h, w = shape
    dev = d.device
    with torch.cuda.device(dev):
        work = torch.empty(lib.sr_depth_l1_workspace_bytes(batch, h, w), dtype=torch.uint8, device=dev)
        out = torch.empty(1 + batch, dtype=torch.float32, device=dev)
        _lib.check(lib.sr_depth_l1_forward(batch, h, w, ptr(d), ptr(g), ptr(work), ptr(out), _lib.stream(dev)))
    return out


class _DepthL1(torch.autograd.Function):
    """(mean over everything, mean per item): `per_item` selects the differentiable one.  Gradients flow to `depth`."""

    @staticmethod
    def forward(ctx, depth, gt, shape, per_item):
        d, g = f32c(depth), f32c(gt)       # each converted to float32 on its own: a half-precision render does not round the target
        out = _run_depth_l1(d, g, shape)
        ctx.save_for_backward(d, g)
        ctx.set_materialize_grads(False)
        ctx.shape, ctx.per_item, ctx.meta = shape, per_item, (depth.shape, depth.dtype)
        outs = (out[0].to(depth.dtype), out[1:].to(depth.dtype))
        ctx.mark_non_differentiable(outs[0 if per_item else 1])
        return outs

    @staticmethod
    def backward(ctx, g_all, g_items):
        up = g_items if ctx.per_item else g_all
        if up is None or not ctx.needs_input_grad[0]:
            return None, None, None, None
        lib = _lib.load()
        d, g = ctx.saved_tensors
        batch, h, w = ctx.shape
        up = f32c(up)
        dev = d.device
        with torch.cuda.device(dev):
            grad = _empty_in_phase(d)
            _lib.check(lib.sr_depth_l1_backward(batch, h, w, ptr(d), ptr(g), ptr(up), int(ctx.per_item), ptr(grad), _lib.stream(dev)))
        shape, dt = ctx.meta
        return grad.reshape(shape).to(dt), None, None, None


def depth_l1_loss(depth: torch.Tensor, gt_depth: torch.Tensor, size_average: bool = True) -> torch.Tensor:
    """Lines 224-229 of the reference's train.py:

        _dmask = gt_depth > 0
        F.l1_loss(depth * _dmask, gt_depth * _dmask)          # the mean over ALL elements, the masked ones included

    for depth maps [H,W], [1,H,W] or [B,H,W] (``gt_depth`` in any of these shapes with as many elements).  A 0-dim tensor, or
    the [B] per-item means with ``size_average=False``.  Differentiable in ``depth``; inputs are assumed finite."""
    if not isinstance(depth, torch.Tensor) or not isinstance(gt_depth, torch.Tensor):
        raise TypeError("depth_l1_loss takes tensors")
    if not depth.is_cuda or not gt_depth.is_cuda:
        raise RuntimeError("depth_l1_loss has no CPU path: tensors must be on a HIP ('cuda') device")
    if gt_depth.device != depth.device:
        raise RuntimeError("depth_l1_loss: the two depth maps must be on the same device")
    if depth.dim() not in (2, 3) or not depth.is_floating_point():
        raise RuntimeError(f"depth_l1_loss: expected a floating-point [H,W], [1,H,W] or [B,H,W] depth map, got {tuple(depth.shape)}")
    if gt_depth.numel() != depth.numel() or gt_depth.shape[-2:] != depth.shape[-2:]:
        raise RuntimeError(f"depth_l1_loss: the two depth maps must have the same size, got {tuple(depth.shape)} and {tuple(gt_depth.shape)}")
    if gt_depth.requires_grad and torch.is_grad_enabled():
        raise RuntimeError("depth_l1_loss: the target requires grad, and no gradient is computed for it (detach it)")
    shape = (depth.shape[0] if depth.dim() == 3 else 1, depth.shape[-2], depth.shape[-1])
    if depth.numel() == 0:       # the mean of nothing
        nan = _nan_like_graph(depth)
        return nan if size_average else nan.expand(shape[0])
    if torch.is_grad_enabled() and depth.requires_grad:
        everything, items = _DepthL1.apply(depth, gt_depth, shape, not size_average)
        return everything if size_average else items
    out = _run_depth_l1(f32c(depth), f32c(gt_depth), shape).to(depth.dtype)      # nothing to differentiate: nothing is kept
    return out[0] if size_average else out[1:]


def _as_views(name, arg, n_views=None):
    """A per-view argument as (list of per-view tensors, the stacked tensor or None): a list / tuple of V tensors, or a tensor
    whose first dimension is V."""
    if arg is None:
        return None, None
    if isinstance(arg, torch.Tensor):
        if arg.dim() < 3:
            raise RuntimeError(f"training_objective: {name} must be a list of per-view tensors or stacked along a first view dimension, got {tuple(arg.shape)}")
        views, stacked = list(arg.unbind(0)), arg
    else:
        views, stacked = list(arg), None
        if not all(isinstance(v, torch.Tensor) for v in views):
            raise TypeError(f"training_objective: {name} takes tensors")
    if n_views is not None and len(views) != n_views:
        raise RuntimeError(f"training_objective: {len(views)} {name} for {n_views} views")
    return views, stacked


def _batch(views, stacked, index, tail_dims):
    """The views `index` as one batch [len(index), *tail]: the stacked tensor itself when it is all of them."""
    if stacked is not None and len(index) == len(views):
        return stacked.reshape((len(index),) + tuple(tail_dims))
    return torch.stack([views[i].reshape(tuple(tail_dims)) for i in index])


def training_objective(images, gt_images, *, opacities=None, gt_masks=None, depths=None, gt_depths=None, means3D=None,
                       gaussian_opacity=None, gradient_error=None, extra=None, lambda_dssim: float, lambda_mask: float = 0.0,
                       lambda_norm: float = 0.0, lambda_norm_mean: float = 0.0, lambda_opacity: float = 0.0,
                       lambda_depthl1: float = 0.0, lambda_gradient: float = 0.0):
    """The objective of the reference's train.py:165-250 for the V views of a step, rendered from one ``gaussian_dict``:

        per view   (1 - lambda_dssim) * Ll1 + lambda_dssim * (1 - ssim)  + lambda_mask * mask  + lambda_depthl1 * depthl1
        once       lambda_norm * norm + lambda_norm_mean * norm_mean + lambda_opacity * opacity
                   + lambda_gradient * gradient_error + extra

    the view terms summed and divided by V.  The reference adds the two norm terms to every view's loss before it divides the
    sum by V, which is the same value; they are evaluated once here.  As in the reference, a term is on when its weight is
    > 0 (and, for ``gradient_error``, when it is given).  ``extra`` is the caller's ``lambda_corr * moran_loss(...)``.

    ``images`` / ``gt_images``: a list of V [3,H,W] tensors or one stacked [V,3,H,W]; ``opacities`` / ``gt_masks`` /
    ``depths`` / ``gt_depths`` likewise, one value per pixel.  Views of equal shape go through ONE batched ``photometric_loss``
    and one batched depth L1; views of differing shapes are grouped by shape and the groups' means combined with the weights
    (views in the group) / V.  Returns ``(loss, log)``; ``log`` carries ``Ll1`` and the reference's ``loss_dict`` entries these
    terms feed -- ``mask``, ``depthl1``, ``opacity``, ``loss_gradient`` -- as detached device tensors (0 for a term that is off).
    Nothing is read back to the host."""
    views, stacked = _as_views("images", images)
    n_views = len(views)
    if n_views == 0:
        raise RuntimeError("training_objective: at least one view is required")
    gts, gts_stacked = _as_views("gt_images", gt_images, n_views)
    use_mask, use_depth = lambda_mask > 0.0, lambda_depthl1 > 0.0
    if use_mask and (opacities is None or gt_masks is None):
        raise RuntimeError("training_objective: lambda_mask needs opacities and gt_masks")
    if use_depth and (depths is None or gt_depths is None):
        raise RuntimeError("training_objective: lambda_depthl1 needs depths and gt_depths")
    alphas, alphas_stacked = _as_views("opacities", opacities, n_views) if use_mask else (None, None)
    masks, masks_stacked = _as_views("gt_masks", gt_masks, n_views) if use_mask else (None, None)
    rendered, rendered_stacked = _as_views("depths", depths, n_views) if use_depth else (None, None)
    targets, targets_stacked = _as_views("gt_depths", gt_depths, n_views) if use_depth else (None, None)

    groups = {}                                    # shape -> view indices, in order of first appearance
    for i, v in enumerate(views):
        if v.dim() != 3:
            raise RuntimeError(f"training_objective: a view is [C,H,W], got {tuple(v.shape)}")
        groups.setdefault(tuple(v.shape), []).append(i)

    def combine(total, term, count):
        term = term if count == n_views else term * (count / n_views)
        return term if total is None else total + term

    loss = l1 = mask_term = depth_term = None
    for shape, index in groups.items():
        c, h, w = shape
        image = _batch(views, stacked, index, shape)
        gt = _batch(gts, gts_stacked, index, shape)
        alpha = _batch(alphas, alphas_stacked, index, (h, w)) if use_mask else None
        mask = _batch(masks, masks_stacked, index, (h, w)) if use_mask else None
        group_loss, group_l1, terms = photometric_loss(image, gt, lambda_dssim, alpha, mask, lambda_mask if use_mask else 0.0,
                                                       return_terms=True)
        loss, l1 = combine(loss, group_loss, len(index)), combine(l1, group_l1, len(index))
        if use_mask:
            mask_term = combine(mask_term, terms["mask"], len(index))
        if use_depth:
            value = depth_l1_loss(_batch(rendered, rendered_stacked, index, (h, w)), _batch(targets, targets_stacked, index, (h, w)))
            depth_term = combine(depth_term, value, len(index))
    if use_depth:
        loss = loss + lambda_depthl1 * depth_term

    lam_n, lam_nm, lam_o = (max(float(v), 0.0) for v in (lambda_norm, lambda_norm_mean, lambda_opacity))
    if (lam_n or lam_nm) and means3D is None:
        raise RuntimeError("training_objective: lambda_norm / lambda_norm_mean need means3D")
    if lam_o and gaussian_opacity is None:
        raise RuntimeError("training_objective: lambda_opacity needs gaussian_opacity")
    opacity_term = None
    if lam_n or lam_nm or lam_o:
        reg, terms = splat_regularizers(means3D if (lam_n or lam_nm) else None, gaussian_opacity if lam_o else None, lam_n, lam_nm, lam_o)
        loss = loss + reg.to(loss.dtype)
        opacity_term = terms.get("opacity")
    gradient_term = None
    if lambda_gradient > 0.0 and gradient_error is not None:
        gradient_term = gradient_error
        loss = loss + lambda_gradient * gradient_term
    if extra is not None:
        loss = loss + extra

    zero = None

    def logged(t):
        nonlocal zero
        if t is not None:
            return t.detach()
        if zero is None:
            zero = torch.zeros((), dtype=loss.dtype, device=loss.device)
        return zero

    log = {"Ll1": l1.detach(), "mask": logged(mask_term), "depthl1": logged(depth_term), "opacity": logged(opacity_term),
           "loss_gradient": logged(gradient_term)}
    return loss, log
