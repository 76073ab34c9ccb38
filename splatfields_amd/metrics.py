"""The evaluation metrics of a run on the device: the reference's ``compute_psnr`` / ``compute_ssim`` (render.py:33-160) and
``psnr`` (utils/image_utils.py:19-21) as drop-ins, and the metric loop of ``eval_all`` / ``training_report`` as one batched call.

The reference evaluates on the host, one image at a time: ``compute_ssim`` copies both images to the CPU and runs
``scipy.signal.convolve2d`` per channel, per quantity and per pass, and it does so on 8-bit images read back from disk.
``image_metrics`` takes a batch of renders as they leave the rasterizer ([B,3,H,W], or [B,H,W,3] images, by strides and without
a permuting copy), applies the file round trip's quantisation in the kernel (``quantize="png"``: torchvision ``save_image`` then
``/255.``; ``"to8b"``: render.py:282) and writes PSNR, the masked "valid"-window SSIM and the per-channel PSNR of every item
to device memory: one kernel and a fixed-order reduction (``sr_image_metrics``), no host synchronisation, no floating-point
atomics, bit-identical results from call to call.  There is no CPU path and nothing is differentiable."""
from __future__ import annotations

import ctypes as C
from typing import Optional

import torch

from . import _lib
from ._lib import ptr

FILTER_SIZE = 11   # the kernel is built for the reference's defaults: 11 taps, sigma 1.5, k1 0.01, k2 0.03, max_val 1
_DEFAULTS = {"max_val": 1.0, "filter_size": FILTER_SIZE, "filter_sigma": 1.5, "k1": 0.01, "k2": 0.03}
_QUANT = {None: _lib.QUANT_NONE, "png": _lib.QUANT_PNG, "to8b": _lib.QUANT_TO8B}


def _f32(t: torch.Tensor) -> torch.Tensor:
    """float32; any strides are kept (the kernel addresses by strides), only another dtype costs a copy.  Not _lib.f32c, which
    would make it contiguous."""
    t = t.detach()
    return t if t.dtype is torch.float32 else t.to(torch.float32)


def _check_pair(name, pred, gt):
    if not isinstance(pred, torch.Tensor) or not isinstance(gt, torch.Tensor):
        raise TypeError(f"{name} takes tensors")
    if not pred.is_cuda or not gt.is_cuda:
        raise RuntimeError(f"{name} has no CPU path: tensors must be on a HIP ('cuda') device")
    if gt.device != pred.device:
        raise RuntimeError(f"{name}: the two images must be on the same device")
    if pred.shape != gt.shape:
        raise RuntimeError(f"{name}: the two images must have the same shape, got {tuple(pred.shape)} and {tuple(gt.shape)}")
    if not pred.is_floating_point() or not gt.is_floating_point():
        raise RuntimeError(f"{name}: floating-point images are required")


def _strides4(t: torch.Tensor, layout: str):
    """element strides (item, channel, row, pixel) of a 4-dim tensor in `layout`"""
    s = t.stride()
    item, channel, row, pixel = (s[0], s[1], s[2], s[3]) if layout == "chw" else (s[0], s[3], s[1], s[2])
    return (C.c_longlong * 4)(item, channel, row, pixel)


def image_metrics(pred: torch.Tensor, gt: torch.Tensor, mask: Optional[torch.Tensor] = None, *, layout: str = "chw",
                  quantize: Optional[str] = None, return_frames: bool = False, lpips=None) -> dict:
    """PSNR and the reference's SSIM of one image or a batch, on the device.

    pred, gt   [3,H,W] / [B,3,H,W] with ``layout="chw"`` (what ``render()`` returns), [H,W,3] / [B,H,W,3] with ``"hwc"``;
               any strides, H and W at least 11.
    mask       None, or a foreground mask with one value per pixel of one image ([H,W], [H,W,1], [1,H,W]: shared by the
               batch) or of every image ([B,H,W], [B,H,W,1], [B,1,H,W]); read as ``mask != 0``.  It selects the reference's
               partial convolution for the SSIM; the PSNR is never masked.
    quantize   None, ``"png"`` or ``"to8b"``: both images go through the 8-bit round trip first.
    lpips      None, or an ``LPIPSWeights``: adds ``"lpips"`` [B], ``lpips_vgg`` of the same (quantised) images, as ``eval_all``
               evaluates all three metrics on the image files.  Without it the call and its outputs are unchanged.
    -> ``{"psnr": [B], "ssim": [B], "psnr_channels": [B,3]}`` float32 device tensors (0-dim / [3] for one image), and with
    ``return_frames`` also ``"frames"``: the quantised prediction, uint8 [B,H,W,3] ([H,W,3])."""
    _check_pair("image_metrics", pred, gt)
    if layout not in ("chw", "hwc"):
        raise ValueError(f"image_metrics: layout must be 'chw' or 'hwc', got {layout!r}")
    if quantize not in _QUANT:
        raise ValueError(f"image_metrics: quantize must be None, 'png' or 'to8b', got {quantize!r}")
    if return_frames and quantize is None:
        raise ValueError("image_metrics: frames are the quantised prediction: return_frames needs quantize='png' or 'to8b'")
    if pred.dim() not in (3, 4):
        raise RuntimeError(f"image_metrics: expected one image or a batch of images, got {tuple(pred.shape)}")
    single = pred.dim() == 3
    x, y = _f32(pred), _f32(gt)
    if single:
        x, y = x[None], y[None]
    batch = x.shape[0]
    channels, h, w = (x.shape[1], x.shape[2], x.shape[3]) if layout == "chw" else (x.shape[3], x.shape[1], x.shape[2])
    if channels != 3:
        raise RuntimeError(f"image_metrics: RGB images are required, got {channels} channels in layout {layout!r} for {tuple(pred.shape)}")
    if batch == 0:
        raise RuntimeError("image_metrics: an empty batch")
    if h < FILTER_SIZE or w < FILTER_SIZE:
        raise ValueError(f"image_metrics: the {FILTER_SIZE}-tap valid window needs images of at least {FILTER_SIZE} x {FILTER_SIZE}, got {h} x {w}")
    dev = x.device
    m, mask_item = None, 0
    if mask is not None:
        if not isinstance(mask, torch.Tensor) or not mask.is_cuda or mask.device != dev:
            raise RuntimeError("image_metrics has no CPU path: the mask must be on the images' HIP ('cuda') device")
        shape = tuple(mask.shape)
        if shape in ((h, w), (h, w, 1), (1, h, w)):
            mask_item = 0
        elif shape in ((batch, h, w), (batch, h, w, 1), (batch, 1, h, w)):
            mask_item = h * w
        else:
            raise RuntimeError(f"image_metrics: the mask must be [H,W], [H,W,1] or [1,H,W] (shared) or [B,H,W], [B,H,W,1] or [B,1,H,W], "
                               f"got {shape} for images {tuple(pred.shape)}")
        m = mask.detach()
        if m.dtype is not torch.float32 or not m.is_contiguous():
            m = m.to(torch.float32).contiguous()
    lib = _lib.load()
    with torch.cuda.device(dev):
        work = torch.empty(lib.sr_metrics_workspace_bytes(batch, h, w), dtype=torch.uint8, device=dev)
        out = torch.empty(5 * batch, dtype=torch.float32, device=dev)   # psnr [B] | ssim [B] | psnr_channels [B,3]
        frames = torch.empty((batch, h, w, 3), dtype=torch.uint8, device=dev) if return_frames else None
        _lib.check(lib.sr_image_metrics(batch, h, w, ptr(x), _strides4(x, layout), ptr(y), _strides4(y, layout), ptr(m), mask_item,
                                        _QUANT[quantize], ptr(work), ptr(out[:batch]), ptr(out[batch:2 * batch]),
                                        ptr(out[2 * batch:]), ptr(frames), _lib.stream(dev)))
    res = {"psnr": out[:batch], "ssim": out[batch:2 * batch], "psnr_channels": out[2 * batch:].reshape(batch, 3)}
    if return_frames:
        res["frames"] = frames
    if single:
        res = {k: v[0] for k, v in res.items()}
    if lpips is not None:
        res["lpips"] = lpips_vgg(pred, gt, lpips, layout=layout, quantize=quantize)
    return res


def compute_psnr(img0: torch.Tensor, img1: torch.Tensor) -> torch.Tensor:
    """The reference's ``compute_psnr`` (render.py:33-43): [H,W,3] images -> PSNR in dB, a 0-dim tensor."""
    _check_pair("compute_psnr", img0, img1)
    if img0.dim() != 3 or img0.shape[-1] != 3:
        raise RuntimeError(f"compute_psnr: expected [H,W,3] images, got {tuple(img0.shape)}")
    return image_metrics(img0, img1, layout="hwc")["psnr"].to(img0.dtype)


def compute_ssim(img0: torch.Tensor, img1: torch.Tensor, mask: Optional[torch.Tensor] = None, max_val: float = 1.0,
                 filter_size: int = 11, filter_sigma: float = 1.5, k1: float = 0.01, k2: float = 0.03) -> torch.Tensor:
    """The reference's ``compute_ssim`` (render.py:45-160): [H,W,3] images and an optional [H,W,1] foreground mask -> SSIM, a
    0-dim tensor.  The kernel is built for the reference's defaults; other filter parameters raise NotImplementedError."""
    given = {"max_val": max_val, "filter_size": filter_size, "filter_sigma": filter_sigma, "k1": k1, "k2": k2}
    if given != _DEFAULTS:
        raise NotImplementedError(f"compute_ssim: the kernel is built for the reference's defaults {_DEFAULTS}, got {given}")
    _check_pair("compute_ssim", img0, img1)
    if img0.dim() != 3 or img0.shape[-1] != 3:
        raise RuntimeError(f"compute_ssim: expected [H,W,3] images, got {tuple(img0.shape)}")
    if mask is not None and tuple(mask.shape) != (img0.shape[0], img0.shape[1], 1):
        raise RuntimeError(f"compute_ssim: expected an [H,W,1] mask, got {tuple(mask.shape)} for images {tuple(img0.shape)}")
    return image_metrics(img0, img1, mask, layout="hwc")["ssim"].to(img0.dtype)


def psnr(img1: torch.Tensor, img2: torch.Tensor) -> torch.Tensor:
    """The reference's ``psnr`` (utils/image_utils.py:19-21): [3,H,W] images -> [3,1], ``20 * log10(1 / sqrt(mse))`` per channel."""
    _check_pair("psnr", img1, img2)
    if img1.dim() != 3 or img1.shape[0] != 3:
        raise RuntimeError(f"psnr: expected [3,H,W] images, got {tuple(img1.shape)}")
    return image_metrics(img1, img2)["psnr_channels"].reshape(3, 1).to(img1.dtype)


from .lpips import LPIPSWeights, eval_lpips, lpips_vgg  # noqa: E402,F401  (lpips.py builds on the helpers above)
