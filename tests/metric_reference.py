"""The evaluation metrics restated in plain PyTorch (any device, float32 or float64, no scipy): the yardstick of the fused HIP
metrics on machines where the reference checkout is absent.  tests/test_metric_reference.py pins it to the reference's own
render.py (`compute_psnr`, `compute_ssim`) through tests/golden/metric_cases.npz (float64, 1e-12).

    quantise  png:  trunc(clamp(x 255 + 0.5, 0, 255)) / 255      to8b:  trunc(255 clamp(x, 0, 1)) / 255
    taps      f_i = exp(-0.5 ((i - 5) / 1.5)^2) / sum, evaluated in float32 and only then cast to the images' dtype
    pass      r = valid_filter(q m),  n = valid_filter(m, ones),  q' = where(n != 0, r 11 / n, 0),  m' = (n != 0)
              first along W, then along H (with q' and m'); without a mask m = 1, as the reference does it
    ssim      mu0, mu1;  s00 = max(0, E[xx] - mu0^2), s11 likewise;  s01 = sign(s01) min(sqrt(s00 s11), |s01|)
              mean of (2 mu0 mu1 + c1)(2 s01 + c2) / ((mu0^2 + mu1^2 + c1)(s00 + s11 + c2)) over the (H-10) x (W-10) x 3 map
    psnr      -10 / ln 10 ln(mean (x - y)^2);   psnr_channels = 20 log10(1 / sqrt(mean_c (x - y)^2))

Images are [..., 3, H, W] here (channels first); `hwc()` / `chw()` convert."""
from __future__ import annotations

import math
import os

import torch
import torch.nn.functional as F

TAPS = 11
C1, C2 = (0.01 * 1.0) ** 2, (0.03 * 1.0) ** 2
METRICS = ("ssim", "psnr")


def filter_taps() -> torch.Tensor:
    """The 1-D filter as the reference's compute_ssim evaluates it: float32 throughout."""
    hw = TAPS // 2
    shift = (2 * hw - TAPS + 1) / 2
    f_i = ((torch.arange(TAPS) - hw + shift) / 1.5) ** 2
    filt = torch.exp(-0.5 * f_i)
    filt /= torch.sum(filt)
    assert filt.dtype is torch.float32
    return filt


def quantize(x: torch.Tensor, mode) -> torch.Tensor:
    """Both 8-bit round trips, on float32 as the reference applies them; the result is float32 on the grid k / 255."""
    if mode is None:
        return x
    x = x.to(torch.float32)
    if mode == "png":       # torchvision.utils.save_image, then eval_imgs' `.float() / 255.`
        return x.mul(255).add_(0.5).clamp_(0, 255).to(torch.uint8).float() / 255.
    if mode == "to8b":      # render.py:282 on the float32 array
        return (255 * x.clamp(0, 1)).to(torch.uint8).float() / 255.
    raise ValueError(mode)


def frames(x: torch.Tensor, mode) -> torch.Tensor:
    """The bytes themselves: [..., 3, H, W] float -> uint8 [..., H, W, 3]."""
    x = x.to(torch.float32)
    q = x.mul(255).add_(0.5).clamp_(0, 255) if mode == "png" else 255 * x.clamp(0, 1)
    return q.to(torch.uint8).movedim(-3, -1).contiguous()


def _valid(z: torch.Tensor, k: torch.Tensor, along_w: bool) -> torch.Tensor:
    """valid filter of every [H,W] plane of z along one axis (the taps are symmetric: correlation = convolution)"""
    h, w = z.shape[-2], z.shape[-1]
    kernel = k.reshape(1, 1, 1, TAPS) if along_w else k.reshape(1, 1, TAPS, 1)
    out = F.conv2d(z.reshape(-1, 1, h, w), kernel.to(z.dtype))
    return out.reshape(z.shape[:-2] + out.shape[-2:])


def _partial_pass(q, m, taps, along_w):
    ones = torch.ones(TAPS, dtype=q.dtype, device=q.device)
    r = _valid(q * m, taps, along_w)
    n = _valid(m, ones, along_w)             # a count of 0/1 values: exact in any summation order
    out = torch.where(n != 0, r * ones.sum() / n, torch.zeros((), dtype=q.dtype, device=q.device))
    return out, (n != 0).to(q.dtype)


def ssim_map(x: torch.Tensor, y: torch.Tensor, mask: torch.Tensor = None) -> torch.Tensor:
    """[..., 3, H, W] images, mask None or broadcastable to [..., 1, H, W] (read as != 0) -> the map [..., 3, H-10, W-10]."""
    if x.shape[-1] < TAPS or x.shape[-2] < TAPS:
        raise ValueError("the valid window needs at least 11 x 11 pixels")
    taps = filter_taps().to(device=x.device)
    m = torch.ones_like(x[..., :1, :, :]) if mask is None else (mask != 0).to(x.dtype)
    m = m.expand(x.shape[:-3] + (1,) + x.shape[-2:]).expand_as(x).contiguous()

    def filt(q):
        q1, m1 = _partial_pass(q, m, taps, along_w=True)
        return _partial_pass(q1, m1, taps, along_w=False)[0]

    mu0, mu1 = filt(x), filt(y)
    mu00, mu11, mu01 = mu0 * mu0, mu1 * mu1, mu0 * mu1
    s00 = (filt(x * x) - mu00).clamp_min(0.0)
    s11 = (filt(y * y) - mu11).clamp_min(0.0)
    s01 = filt(x * y) - mu01
    s01 = torch.sign(s01) * torch.minimum(torch.sqrt(s00 * s11), s01.abs())
    return ((2 * mu01 + C1) * (2 * s01 + C2)) / ((mu00 + mu11 + C1) * (s00 + s11 + C2))


def evaluate(pred, gt, mask=None, quantize_mode=None, dtype=torch.float64, device="cpu") -> dict:
    """-> {"psnr": [B], "ssim": [B], "psnr_channels": [B,3]} (0-dim / [3] for one image) of detached CPU tensors in `dtype`.
    pred, gt: [3,H,W] or [B,3,H,W]; mask: anything with H*W or B*H*W values."""
    single = pred.dim() == 3
    x = quantize(pred.detach(), quantize_mode).to(device=device, dtype=dtype)
    y = quantize(gt.detach(), quantize_mode).to(device=device, dtype=dtype)
    if single:
        x, y = x[None], y[None]
    b, _, h, w = x.shape
    m = None
    if mask is not None:
        m = mask.detach().to(device=device).reshape(-1, 1, h, w)
    se = ((x - y) ** 2).reshape(b, 3, -1)
    out = {"psnr": -10.0 / math.log(10) * torch.log(se.reshape(b, -1).mean(dim=1)),
           "psnr_channels": 20 * torch.log10(1.0 / torch.sqrt(se.mean(dim=2))),
           "ssim": ssim_map(x, y, m).reshape(b, -1).mean(dim=1)}
    return {k: (v[0] if single else v).detach().cpu() for k, v in out.items()}


def hwc(t: torch.Tensor) -> torch.Tensor:
    return t.movedim(-3, -1)


def chw(t: torch.Tensor) -> torch.Tensor:
    return t.movedim(-1, -3)


# ---- inputs ----

def textured_pair(height: int, width: int, seed: int = 0, noise: float = 0.08):
    """A shaded, textured disc on a white background and a noisy prediction of it: ([3,H,W] prediction, target, [H,W] mask of
    the disc), float32.  Outside the disc the prediction equals the target exactly."""
    gen = torch.Generator().manual_seed(seed)
    yy, xx = torch.meshgrid(torch.linspace(-1, 1, height), torch.linspace(-1, 1, width), indexing="ij")
    r2 = (xx - 0.1) ** 2 + (yy + 0.05) ** 2
    inside = r2 < 0.45
    shade = (1.0 - r2 / 0.45).clamp_min(0.0).sqrt()
    tint = torch.tensor([0.9, 0.6, 0.3]).reshape(3, 1, 1)
    body = tint * (0.25 + 0.75 * shade) * (1.0 + 0.1 * torch.sin(9.0 * xx + 5.0 * yy))
    target = torch.where(inside, body, torch.ones_like(body)).clamp(0.0, 1.0)
    pred = torch.where(inside, (target + noise * (torch.rand(target.shape, generator=gen) - 0.5)).clamp(0.0, 1.0), target)
    return pred.float(), target.float(), inside.float()


def golden_inputs() -> dict:
    """{case: (pred [3,H,W], gt [3,H,W], mask [H,W] or None)}: the smallest shapes at which the tile walk can go wrong."""
    gen = torch.Generator().manual_seed(20240911)
    rand = lambda *s: torch.rand(*s, generator=gen)
    out = {}
    for h, w in ((11, 11), (11, 64), (64, 11), (12, 30), (37, 53), (43, 75)):   # one output; a degenerate axis; ragged tile edges
        out[f"noise_{h}x{w}"] = (rand(3, h, w), rand(3, h, w), None)
    t = 0.2 + 0.6 * rand(3, 37, 53)
    out["near_equal"] = (t + 1e-3 * (2 * rand(3, 37, 53) - 1), t, None)
    out["grid8"] = (quantize(rand(3, 43, 75), "png"), quantize(rand(3, 43, 75), "png"), None)   # already on the 8-bit grid
    p, t, disc = textured_pair(43, 75, seed=5)
    out["disc"] = (p, t, disc)
    x, y = rand(3, 37, 53), rand(3, 37, 53)
    out["mask_random"] = (x, y, (rand(37, 53) < 0.7).float())
    hole = torch.ones(37, 53)
    hole[4:29, 20:45] = 0.0                                                       # 25 x 25 zeros: windows without a mask pixel
    hole[33, :] = 0.0
    hole[:, 3] = 0.0
    out["mask_hole"] = (x, y, hole)
    out["mask_zero"] = (x, y, torch.zeros(37, 53))
    out["mask_one"] = (x, y, torch.ones(37, 53))
    return {k: (p.float().contiguous(), t.float().contiguous(), m) for k, (p, t, m) in out.items()}


# ---- the golden cases (tests/golden/metric_cases.npz, written by tests/golden/make_metric_golden.py from the reference itself) ----

def load_golden_cases() -> dict:
    """{case: {"pred", "gt" [3,H,W], ["mask" [H,W]], "f64": {"psnr", "ssim"}, "f32": {...}}} of torch tensors."""
    import numpy as np
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "metric_cases.npz")
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
    """|d ssim| and |d psnr| in dB (psnr_channels count as psnr) of one evaluation from the float64 one; the largest over the
    items.  Two infinities of the same sign agree."""
    f = lambda t: torch.as_tensor(t).to(torch.float64).reshape(-1)
    out = dict.fromkeys(METRICS, 0.0)
    for k, metric in (("ssim", "ssim"), ("psnr", "psnr"), ("psnr_channels", "psnr")):
        if k in want and k in got:
            g, w = f(got[k]), f(want[k])
            assert g.shape == w.shape, (k, g.shape, w.shape)
            d = torch.where(g == w, torch.zeros_like(g), (g - w).abs())
            d = torch.nan_to_num(d, nan=float("inf"))
            out[metric] = max(out[metric], d.max().item())
    return out


def reference_error(cases: dict) -> dict:
    """r per metric: the largest deviation, over ALL golden cases, of the reference's own float32 evaluation from its float64
    evaluation.  Another float32 evaluation of the same formulas (the HIP kernel) may deviate from float64 by 4 r."""
    r = dict.fromkeys(METRICS, 0.0)
    for c in cases.values():
        d = deviations(c["f32"], c["f64"])
        r = {k: max(r[k], d[k]) for k in METRICS}
    return r
