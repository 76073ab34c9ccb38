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

import ctypes as C
from typing import Optional

import torch

from . import _lib

WINDOW_SIZE = 11   # the kernels are built for the reference's window: 11 taps, sigma 1.5

_FUSED, _L1, _SSIM = 0, 1, 2


def _ptr(t: Optional[torch.Tensor]):
    return None if t is None else C.c_void_p(t.data_ptr())


def _f32(t: torch.Tensor) -> torch.Tensor:
    t = t.detach()
    if t.dtype is not torch.float32 or not t.is_contiguous():
        t = t.to(torch.float32).contiguous()
    return t


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
        _lib.check(lib.sr_photometric_forward(batch, channels, h, w, _ptr(x), _ptr(y), _ptr(a), _ptr(m), float(lambda_dssim),
                                              float(lambda_mask), _ptr(work), _ptr(maps), _ptr(out[0:1]), _ptr(out[1:2]),
                                              _ptr(ssim_out), _ptr(out[2:3]) if a is not None else None,
                                              C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)))
    return out[0], out[1], out[3:], out[2], maps


class _Photometric(torch.autograd.Function):
    """One differentiable output per mode -- the blended loss, l1, or the per-item structural similarity -- and the other terms
    as detached tensors.  Gradients flow to `image` and `opacity` only."""

    @staticmethod
    def forward(ctx, image, gt, opacity, gt_mask, mode, shape, lambda_dssim, lambda_mask):
        x, y = _f32(image), _f32(gt)
        a = None if opacity is None else _f32(opacity)
        m = None if gt_mask is None else _f32(gt_mask)
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
        g = _f32(g)
        per_item = ctx.mode == _SSIM
        dev = x.device
        want_alpha = a is not None and ctx.needs_input_grad[2]
        with torch.cuda.device(dev):
            d_image = torch.empty_like(x)
            d_alpha = torch.empty_like(a) if want_alpha else None
            w_l1, w_ssim, w_mask = ctx.weights
            _lib.check(lib.sr_photometric_backward(batch, channels, h, w, _ptr(x), _ptr(y), _ptr(a), _ptr(m), _ptr(maps), w_l1, w_ssim,
                                                   w_mask, _ptr(g), int(per_item), _ptr(d_image), _ptr(d_alpha),
                                                   C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)))
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
    loss, l1, ssim_items, mask_l1, _ = _run_forward(_f32(image), _f32(gt), None if opacity is None else _f32(opacity),
                                                    None if gt_mask is None else _f32(gt_mask), shape, lambda_dssim, lambda_mask,
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
