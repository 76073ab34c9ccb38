"""The photometric loss restated in plain PyTorch (any device, any float dtype): the yardstick of the fused HIP loss on
machines where the reference checkout is absent.  tests/test_loss_reference.py pins it to the reference's own
utils/loss_utils.py through tests/golden/loss_cases.npz (float64, 1e-12 relative).

    l1      = mean |x - y|
    ssim    = mean S,  S = (2 mu1 mu2 + C1)(2 s12 + C2) / ((mu1^2 + mu2^2 + C1)(s11 + s22 + C2)),
              mu = w * x,  s11 = w * x^2 - mu1^2,  s12 = w * (x y) - mu1 mu2,  zero padding of 5
    w       = the 11 x 11 outer product of the float32 taps float32(exp(-(i - 5)^2 / 4.5)) / their float32 sum, itself
              rounded to float32 and only then cast to the images' dtype
    loss    = (1 - lambda_dssim) l1 + lambda_dssim (1 - ssim) + lambda_mask mean |clamp(opacity, 0, 1) - gt_mask|

An image is [..., H, W]; every leading index is a plane of its own (a [H, W, 1] depth tensor is H planes of W x 1)."""
from __future__ import annotations

import math

import torch
import torch.nn.functional as F

TAPS = 11
C1, C2 = 0.01 ** 2, 0.03 ** 2


def window_taps() -> torch.Tensor:
    """The 1-D window in float32, normalised in float32."""
    g = torch.tensor([math.exp(-((i - TAPS // 2) ** 2) / (2.0 * 1.5 ** 2)) for i in range(TAPS)], dtype=torch.float32)
    return g / g.sum()


def window_2d(dtype, device) -> torch.Tensor:
    g = window_taps()
    return (g[:, None] * g[None, :]).to(torch.float32).to(device=device, dtype=dtype)


def ssim_map(x: torch.Tensor, y: torch.Tensor) -> torch.Tensor:
    """S per pixel, in the shape of x."""
    h, w = x.shape[-2], x.shape[-1]
    k = window_2d(x.dtype, x.device)[None, None]
    blur = lambda t: F.conv2d(t.reshape(-1, 1, h, w), k, padding=TAPS // 2).reshape(t.shape)
    mu1, mu2 = blur(x), blur(y)
    s11 = blur(x * x) - mu1 * mu1
    s22 = blur(y * y) - mu2 * mu2
    s12 = blur(x * y) - mu1 * mu2
    return ((2 * mu1 * mu2 + C1) * (2 * s12 + C2)) / ((mu1 * mu1 + mu2 * mu2 + C1) * (s11 + s22 + C2))


def l1(x: torch.Tensor, y: torch.Tensor) -> torch.Tensor:
    return (x - y).abs().mean()


def ssim(x: torch.Tensor, y: torch.Tensor, size_average: bool = True) -> torch.Tensor:
    s = ssim_map(x, y)
    return s.mean() if size_average else s.reshape(s.shape[0], -1).mean(dim=1)


def mask_l1(opacity: torch.Tensor, gt_mask: torch.Tensor) -> torch.Tensor:
    return (opacity.clamp(0.0, 1.0).reshape(-1) - gt_mask.reshape(-1)).abs().mean()


def photometric(image, gt, lambda_dssim=0.2, opacity=None, gt_mask=None, lambda_mask=0.0):
    """-> (loss, l1, ssim, mask term or None)"""
    a, s = l1(image, gt), ssim(image, gt)
    loss = (1.0 - lambda_dssim) * a + lambda_dssim * (1.0 - s)
    m = None
    if opacity is not None:
        m = mask_l1(opacity, gt_mask)
        loss = loss + lambda_mask * m
    return loss, a, s, m


def evaluate(image, gt, opacity=None, gt_mask=None, lambda_dssim=0.2, lambda_mask=0.0, dtype=torch.float64, device="cpu"):
    """Values and gradients of the loss in `dtype`: dict of detached CPU tensors l1, ssim, loss, d_image (and mask, d_opacity)."""
    x = image.detach().to(device=device, dtype=dtype).requires_grad_(True)
    y = gt.detach().to(device=device, dtype=dtype)
    a = m = None
    if opacity is not None:
        a = opacity.detach().to(device=device, dtype=dtype).requires_grad_(True)
        m = gt_mask.detach().to(device=device, dtype=dtype)
    loss, v_l1, v_ssim, v_mask = photometric(x, y, lambda_dssim, a, m, lambda_mask)
    loss.backward()
    out = {"l1": v_l1, "ssim": v_ssim, "loss": loss, "d_image": x.grad}
    if a is not None:
        out["mask"], out["d_opacity"] = v_mask, a.grad
    return {k: v.detach().cpu() for k, v in out.items()}


def blob_scene(height: int, width: int, background: float, seed: int = 0, channels: int = 3):
    """A shaded blob on a flat background: (prediction, target, opacity, mask), float32.  Outside the blob the prediction equals
    the target exactly and the opacity is exactly 0; in its core the opacity is exactly 1."""
    gen = torch.Generator().manual_seed(seed)
    yy, xx = torch.meshgrid(torch.linspace(-1, 1, height), torch.linspace(-1, 1, width), indexing="ij")
    r2 = (xx - 0.1) ** 2 + (yy + 0.05) ** 2
    inside = r2 < 0.45
    shade = (1.0 - r2 / 0.45).clamp_min(0.0).sqrt()
    tint = torch.tensor([0.9, 0.6, 0.3, 0.5, 0.7, 0.2][:channels]).reshape(-1, 1, 1)
    body = tint * (0.25 + 0.75 * shade) * (1.0 + 0.1 * torch.sin(9.0 * xx + 5.0 * yy))
    target = torch.where(inside, body, torch.full_like(body, background)).clamp(0.0, 1.0)
    noise = 0.08 * (torch.rand(target.shape, generator=gen) - 0.5)
    pred = torch.where(inside, (target + noise).clamp(0.0, 1.0), target)
    mask = inside.to(torch.float32)[None]
    opacity = torch.where(r2 < 0.1, torch.ones_like(r2), (1.4 * shade - 0.2) * inside)[None]   # below 0 at the rim, above 1 around the core, 1 in it
    return pred.to(torch.float32), target.to(torch.float32), opacity.to(torch.float32), mask


# ---- the golden cases (tests/golden/loss_cases.npz, written by tests/golden/make_loss_golden.py from the reference itself) ----

METRICS = ("ssim", "loss", "grad_max", "grad_l2")


def load_golden_cases() -> dict:
    """{case: {"image", "gt", "lambdas", ["opacity", "gt_mask", "item_weights"], "f64": {...}, "f32": {...}}} of torch tensors."""
    import os

    import numpy as np
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "loss_cases.npz")
    cases: dict = {}
    with np.load(path) as z:
        for key in z.files:
            parts = key.split("/")
            node = cases.setdefault(parts[0], {})
            for p in parts[1:-1]:
                node = node.setdefault(p, {})
            node[parts[-1]] = torch.from_numpy(z[key])
    return cases


def deviations(got: dict, want: dict) -> dict:
    """The four figures by which one evaluation `got` differs from the float64 evaluation `want` (dicts as `evaluate` returns,
    optionally with ssim_items / d_image_items): |d ssim|, |d loss| (l1 and the mask term count here), and over every gradient
    tensor max|d grad| / max|grad| and the relative L2."""
    f = lambda t: torch.as_tensor(t).to(torch.float64)
    out = {"ssim": 0.0, "loss": 0.0, "grad_max": 0.0, "grad_l2": 0.0}
    for k in ("ssim", "ssim_items"):
        if k in want and k in got:
            out["ssim"] = max(out["ssim"], (f(got[k]) - f(want[k])).abs().max().item())
    for k in ("loss", "l1", "mask"):
        if k in want and k in got:
            out["loss"] = max(out["loss"], (f(got[k]) - f(want[k])).abs().max().item())
    for k in ("d_image", "d_opacity", "d_image_items"):
        if k in want and k in got:
            g, w = f(got[k]).reshape(-1), f(want[k]).reshape(-1)
            out["grad_max"] = max(out["grad_max"], ((g - w).abs().max() / w.abs().max().clamp_min(1e-300)).item())
            out["grad_l2"] = max(out["grad_l2"], ((g - w).norm() / w.norm().clamp_min(1e-300)).item())
    return out


def reference_error(cases: dict) -> dict:
    """r per metric: the largest deviation, over ALL golden cases, of the reference's own float32 evaluation from its float64
    evaluation.  Another float32 evaluation of the same formulas (the HIP kernels) may deviate from float64 by 4 r."""
    r = dict.fromkeys(METRICS, 0.0)
    for c in cases.values():
        d = deviations(c["f32"], c["f64"])
        r = {k: max(r[k], d[k]) for k in METRICS}
    return r
