"""Plain-PyTorch restatement of the reference's plane generator -- `Tensorial2D` around `TimeVAEDecoder`
(scene/tripFields.py:176-204, scene/time_decoders.py) -- as a function of a state dict with the reference's names.  The
yardstick of splatfields_amd/plane_generator.py: it runs in float64 and float32 on any device and is differentiated by autograd.

What is pinned by the reference itself (tests/golden/plane_decoder_*.npz are runs of ITS classes, see
tests/golden/make_plane_decoder_golden.py): the layer order, `TimeLoRACompatibleConv.get_weights`, the resnet / mid / up blocks,
`TimeDecoder.forward`.  What is stated from the published behaviour of packages the reference imports but does not ship:
`Upsample2D(use_conv=True)` = nearest x2 then a 3x3 convolution; the mid block's `Attention` = GroupNorm, one head over H W
tokens of width C, q / k / v / out linears with bias, softmax(q k^T / sqrt(C)) v, residual; eps = 1e-6 everywhere.
"""
from __future__ import annotations

import math

import torch
import torch.nn.functional as F

EPS = 1e-6


def conv_weight(sd, prefix, frame_id):
    """TimeLoRACompatibleConv.get_weights (time_decoders.py:38-43): weight + frame_weights[frame_id] when the layer has per-frame
    weights for more than one frame."""
    w = sd[prefix + ".weight"]
    fw = sd.get(prefix + ".frame_weights")
    if fw is None or fw.shape[0] <= 1:
        return w
    if torch.is_tensor(frame_id):
        frame_id = frame_id.long()
    return w + fw[frame_id]


def norm_silu(sd, prefix, x, groups):
    return F.silu(F.group_norm(x, groups, sd[prefix + ".weight"], sd[prefix + ".bias"], EPS))


def resnet(sd, prefix, x, groups, frame_id):
    """TimeResnetBlock2D.forward (time_decoders.py:184-250) without a time embedding, dropout 0, output_scale_factor 1"""
    h = norm_silu(sd, prefix + ".norm1", x, groups)
    h = F.conv2d(h, conv_weight(sd, prefix + ".conv1", frame_id), sd[prefix + ".conv1.bias"], padding=1)
    h = norm_silu(sd, prefix + ".norm2", h, groups)
    h = F.conv2d(h, conv_weight(sd, prefix + ".conv2", frame_id), sd[prefix + ".conv2.bias"], padding=1)
    if prefix + ".conv_shortcut.weight" in sd:    # the block changes width (never in the reference's configuration)
        x = F.conv2d(x, sd[prefix + ".conv_shortcut.weight"], sd.get(prefix + ".conv_shortcut.bias"))
    return x + h


def attention(sd, prefix, x, groups):
    b, c, h, w = x.shape
    t = F.group_norm(x.view(b, c, h * w), groups, sd[prefix + ".group_norm.weight"], sd[prefix + ".group_norm.bias"], EPS).transpose(1, 2)
    q = F.linear(t, sd[prefix + ".to_q.weight"], sd[prefix + ".to_q.bias"])
    k = F.linear(t, sd[prefix + ".to_k.weight"], sd[prefix + ".to_k.bias"])
    v = F.linear(t, sd[prefix + ".to_v.weight"], sd[prefix + ".to_v.bias"])
    probs = (torch.bmm(q, k.transpose(1, 2)) * (1.0 / math.sqrt(c))).softmax(dim=-1)
    o = F.linear(torch.bmm(probs, v), sd[prefix + ".to_out.0.weight"], sd[prefix + ".to_out.0.bias"])
    return o.transpose(1, 2).reshape(b, c, h, w) + x


def upsample_conv(sd, prefix, x):
    return F.conv2d(F.interpolate(x, scale_factor=2.0, mode="nearest"), sd[prefix + ".conv.weight"], sd[prefix + ".conv.bias"], padding=1)


def count(sd, prefix):
    """number of consecutive children prefix0, prefix1, ... in the state dict"""
    n = 0
    while any(k.startswith(f"{prefix}{n}.") for k in sd):
        n += 1
    return n


def decoder(sd, z, groups, frame_id=None, prefix=""):
    """TimeDecoder.forward (time_decoders.py:528-580): z [1, in_ch, h, w] -> [1, out_ch, H, W]"""
    h = F.conv2d(z, sd[prefix + "conv_in.weight"], sd[prefix + "conv_in.bias"], padding=1)
    h = resnet(sd, prefix + "mid_block.resnets.0", h, groups, frame_id)
    for i in range(count(sd, prefix + "mid_block.attentions.")):
        h = attention(sd, f"{prefix}mid_block.attentions.{i}", h, groups)
        h = resnet(sd, f"{prefix}mid_block.resnets.{i + 1}", h, groups, frame_id)
    for i in range(count(sd, prefix + "up_blocks.")):
        for j in range(count(sd, f"{prefix}up_blocks.{i}.resnets.")):
            h = resnet(sd, f"{prefix}up_blocks.{i}.resnets.{j}", h, groups, frame_id)
        if f"{prefix}up_blocks.{i}.upsamplers.0.conv.weight" in sd:
            h = upsample_conv(sd, f"{prefix}up_blocks.{i}.upsamplers.0", h)
    h = norm_silu(sd, prefix + "conv_norm_out", h, groups)
    return F.conv2d(h, sd[prefix + "conv_out.weight"], sd[prefix + "conv_out.bias"], padding=1)


def tensorial2d(sd, groups=32, frame_id=None, prefix=""):
    """Tensorial2D.forward (tripFields.py:202-204): the decoder at the module's own noise buffer"""
    return decoder(sd, sd[prefix + "noise"], groups, frame_id, prefix + "net.")


def planes(sd, groups=32, frame_id=None, prefix="subs."):
    """VarTriPlaneEncoder.get_planes (tripFields.py:401-405): [n_planes, out_ch, H, W]"""
    return torch.cat([tensorial2d(sd, groups, frame_id, f"{prefix}{i}.") for i in range(count(sd, prefix))], dim=0)


def run(fn, sd, probe, dtype, device="cpu", no_grad=("noise",)):
    """out = fn(state dict in `dtype` on `device`); gradients of sum(out * probe) for every tensor of the state dict that is a
    parameter (everything but the `noise` buffers).  -> dict(out=..., grads={name: ...}) as float64 on the CPU."""
    leaf = {}
    for k, v in sd.items():
        t = torch.as_tensor(v).detach().to(device=device, dtype=dtype).clone()
        if t.is_floating_point() and not any(k == n or k.endswith("." + n) for n in no_grad):
            t.requires_grad_(True)
        leaf[k] = t
    out = fn(leaf)
    (out * torch.as_tensor(probe).to(device=device, dtype=dtype)).sum().backward()
    grads = {k: (t.grad if t.grad is not None else torch.zeros_like(t)).detach().double().cpu() for k, t in leaf.items() if t.requires_grad}
    return dict(out=out.detach().double().cpu(), grads=grads)


def layer(x, weight, bias, gamma, beta, residual, groups, prologue, upsample, silu_out):
    """one fused layer as sr_conv3x3_forward defines it (include/splatraster.h): x [1, Cin, h, w]"""
    a = F.silu(F.group_norm(x, groups, gamma, beta, EPS)) if prologue else x
    if upsample:
        a = F.interpolate(a, scale_factor=2.0, mode="nearest")
    z = F.conv2d(a, weight, bias, padding=1)
    if residual is not None:
        z = z + residual
    return F.silu(z) if silu_out else z
