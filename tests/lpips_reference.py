"""LPIPS (VGG) restated in torch: the published `lpips` package v0.1, net='vgg', spatial=False, eval mode, from its published
behaviour (the package is not available here, so nothing is compared with it).  `dtype` is a parameter: float64 is the reference
of the GPU tests, and float32 has two evaluation orders whose errors against float64 measure what a float32 evaluation may cost:

  "conv2d"   F.conv2d per layer;
  "chunked"  per 16 input channels and per tap of the 3x3 window a partial convolution, added one after another.

Imports torch only (the weights come as plain tensors: `parts(weights)` reads them off an LPIPSWeights)."""
import torch
import torch.nn.functional as F

GROUPS = (2, 2, 3, 3, 3)           # convolutions per group; a 2x2 / stride-2 max-pool (floor) between the groups
EPS = 1e-10
ORDERS = ("conv2d", "chunked")


def parts(weights):
    """(convs, lins, shift, scale) of an LPIPSWeights, on the CPU"""
    return ([(w.cpu(), b.cpu()) for w, b in weights.convs], [v.cpu() for v in weights.lins], weights.shift.cpu(), weights.scale.cpu())


def quantise(x, mode):
    """the 8-bit round trip of image_metrics, in float32 (what the kernel applies on load)"""
    x = x.float()
    if mode == "png":
        return (x * 255.0 + 0.5).clamp(0, 255).trunc() / 255.0
    if mode == "to8b":
        return (255.0 * x.clamp(0, 1)).trunc() / 255.0
    assert mode is None, mode
    return x


def conv3x3(x, w, b, order):
    if order == "conv2d":
        return F.conv2d(x, w, b, padding=1)
    assert order == "chunked", order
    h, wd = x.shape[-2:]
    xp = F.pad(x, (1, 1, 1, 1))
    out = b.reshape(1, -1, 1, 1).expand(x.shape[0], -1, h, wd).clone()
    for c0 in range(0, x.shape[1], 16):
        for ky in range(3):
            for kx in range(3):
                out = out + F.conv2d(xp[:, c0:c0 + 16, ky:ky + h, kx:kx + wd], w[:, c0:c0 + 16, ky:ky + 1, kx:kx + 1])
    return out


def tap_features(x, convs, shift, scale, order="conv2d"):
    """x [N,3,H,W] in [0,1] (already in the working dtype) -> the five taps"""
    dt = x.dtype
    x = (x * 2.0 - 1.0 - shift.to(dt).reshape(1, 3, 1, 1)) / scale.to(dt).reshape(1, 3, 1, 1)
    taps, layer = [], 0
    for g, n in enumerate(GROUPS):
        if g:
            x = F.max_pool2d(x, 2, 2)
        for _ in range(n):
            w, b = convs[layer]
            x = torch.relu(conv3x3(x, w.to(dt), b.to(dt), order))
            layer += 1
        taps.append(x)
    return taps


def evaluate(pred, gt, convs, lins, shift, scale, dtype=torch.float64, order="conv2d", quantize=None):
    """pred, gt [B,3,H,W] in [0,1] -> {"value": [B], "taps": [B,5], "maps": five [B, H >> l, W >> l]} in `dtype`, on the CPU"""
    with torch.no_grad():
        x = torch.cat([quantise(pred.cpu(), quantize), quantise(gt.cpu(), quantize)]).to(dtype)
        feats = tap_features(x, convs, shift, scale, order)
        n = pred.shape[0]
        maps = []
        for f, lin in zip(feats, lins):
            f = f / (f.pow(2).sum(1, keepdim=True).sqrt() + EPS)
            maps.append(((f[:n] - f[n:]).pow(2) * lin.to(dtype).reshape(1, -1, 1, 1)).sum(1))
        taps = torch.stack([m.mean((1, 2)) for m in maps], 1)
        return {"value": taps.sum(1), "taps": taps, "maps": maps}


def images(batch, h, w, seed):
    """the inputs of the tests: gt ~ U(0,1), pred = clamp(gt + 0.1 N(0,1)), [B,3,H,W] float32"""
    g = torch.Generator().manual_seed(seed)
    gt = torch.rand(batch, 3, h, w, generator=g)
    pred = (gt + 0.1 * torch.randn(batch, 3, h, w, generator=g)).clamp(0, 1)
    return pred, gt
