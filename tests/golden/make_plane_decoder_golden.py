"""Writes tests/golden/plane_decoder_*.npz and plane_decoder_keys.json by running the REFERENCE's plane generator classes
(scene/time_decoders.py, scene/tripFields.py).  Run once, by hand, where a checkout of the reference exists:

    python tests/golden/make_plane_decoder_golden.py /path/to/reference

No test imports this file.  The reference imports three packages it does not ship (mmgen, mmcv, diffusers); stand-ins for the
few names it takes from them are installed into sys.modules first:

    mmgen.models.build_module          constructs the reference's own TimeVAEDecoder from the config dict
    mmgen.models.builder.MODULES       register_module() is a no-op decorator
    mmcv.cnn.utils                     kaiming_init (kaiming_normal_, fan_out, relu, bias 0), constant_init (weight = val, bias 0)
    diffusers ... ModelMixin           an empty class
    diffusers ... Upsample2D           use_conv=True: F.interpolate(scale_factor=2, nearest), then Conv2d(c, c, 3, padding=1) as `conv`
    diffusers ... Attention            GroupNorm `group_norm`, Linear `to_q` / `to_k` / `to_v` / `to_out.0` with bias, one head over
                                       the H W tokens, softmax(q k^T / sqrt(dim_head)) v, residual connection
    get_activation('silu' | 'swish')   nn.SiLU();  ResnetBlock2D, LoRAConv2dLayer, logging, is_torch_version: inert

Everything else that runs is the reference's code.  After construction every parameter is overwritten from a seeded generator
(`zero_init_residual` would otherwise leave half the network a no-op), GroupNorm biases of order 1.
Fixtures hold numeric arrays and name lists only.
"""
import json
import math
import os
import sys
import types

import numpy as np
import torch
import torch.nn.functional as F
from torch import nn

HERE = os.path.dirname(os.path.abspath(__file__))


class Upsample2D(nn.Module):
    def __init__(self, channels, use_conv=False, use_conv_transpose=False, out_channels=None, name="conv"):
        super().__init__()
        assert use_conv and not use_conv_transpose and name == "conv"
        self.conv = nn.Conv2d(channels, out_channels or channels, 3, padding=1)

    def forward(self, x, output_size=None, scale=1.0):
        return self.conv(F.interpolate(x, scale_factor=2.0, mode="nearest"))


class Attention(nn.Module):
    def __init__(self, query_dim, heads=8, dim_head=64, rescale_output_factor=1.0, eps=1e-5, norm_num_groups=None, spatial_norm_dim=None,
                 residual_connection=False, bias=False, upcast_softmax=False, _from_deprecated_attn_block=False):
        super().__init__()
        assert heads == 1 and spatial_norm_dim is None and residual_connection and rescale_output_factor == 1
        inner = heads * dim_head
        self.scale = dim_head ** -0.5
        self.group_norm = nn.GroupNorm(norm_num_groups, query_dim, eps=eps, affine=True)
        self.to_q, self.to_k, self.to_v = nn.Linear(query_dim, inner, bias=bias), nn.Linear(query_dim, inner, bias=bias), nn.Linear(query_dim, inner, bias=bias)
        self.to_out = nn.ModuleList([nn.Linear(inner, query_dim), nn.Dropout(0.0)])

    def forward(self, x, temb=None):
        b, c, h, w = x.shape
        t = self.group_norm(x.view(b, c, h * w)).transpose(1, 2)
        q, k, v = self.to_q(t), self.to_k(t), self.to_v(t)
        probs = (torch.bmm(q, k.transpose(1, 2)) * self.scale).softmax(dim=-1)
        o = self.to_out[1](self.to_out[0](torch.bmm(probs, v)))
        return o.transpose(1, 2).reshape(b, c, h, w) + x


def install_stand_ins(ref):
    def module(name, **attrs):
        m = types.ModuleType(name)
        m.__path__ = []
        m.__dict__.update(attrs)
        sys.modules[name] = m
        return m

    def kaiming_init(m, a=0, mode="fan_out", nonlinearity="relu", bias=0, distribution="normal"):
        nn.init.kaiming_normal_(m.weight, a=a, mode=mode, nonlinearity=nonlinearity)
        if getattr(m, "bias", None) is not None:
            nn.init.constant_(m.bias, bias)

    def constant_init(m, val, bias=0):
        nn.init.constant_(m.weight, val)
        if getattr(m, "bias", None) is not None:
            nn.init.constant_(m.bias, bias)

    class Registry:
        def register_module(self, *a, **k):
            return lambda cls: cls

    def build_module(cfg, *a, **k):
        from scene.time_decoders import TimeVAEDecoder
        cfg = dict(cfg)
        assert cfg.pop("type") == "TimeVAEDecoder"
        return TimeVAEDecoder(**cfg)

    def get_activation(name):
        assert name in ("silu", "swish")
        return nn.SiLU()

    inert = type("Inert", (), {})
    log = types.SimpleNamespace(get_logger=lambda name: types.SimpleNamespace(warn=print, warning=print, info=print))
    module("mmgen"); module("mmgen.models", build_module=build_module); module("mmgen.models.builder", MODULES=Registry())
    module("mmcv"); module("mmcv.cnn"); module("mmcv.cnn.utils", kaiming_init=kaiming_init, constant_init=constant_init)
    module("diffusers"); module("diffusers.models")
    module("diffusers.models.modeling_utils", ModelMixin=type("ModelMixin", (), {}))
    module("diffusers.models.resnet", ResnetBlock2D=type("ResnetBlock2D", (inert,), {}), Upsample2D=Upsample2D)
    module("diffusers.models.attention_processor", Attention=Attention)
    module("diffusers.models.vae", is_torch_version=lambda *a: True, get_activation=get_activation)
    module("diffusers.models.lora", LoRAConv2dLayer=type("LoRAConv2dLayer", (inert,), {}))
    module("diffusers.utils", logging=log)
    pkg = types.ModuleType("scene")
    pkg.__path__ = [os.path.join(ref, "scene")]
    sys.modules["scene"] = pkg
    sys.path.insert(0, ref)


def overwrite(mod, gen, half=False):
    """every parameter from the seeded generator: weights ~ N(0, 1) / sqrt(fan_in), biases ~ 0.3 N(0, 1), GroupNorm weight
    1 + 0.3 N(0, 1) and bias N(0, 1), per-frame weights of the size of the weights.  half: on the float16 grid (exact in a float16 file)."""
    norms = {id(p) for m in mod.modules() if isinstance(m, nn.GroupNorm) for p in m.parameters()}
    with torch.no_grad():
        for name, p in mod.named_parameters():
            r = torch.randn(p.shape, generator=gen)
            if id(p) in norms:
                v = 1.0 + 0.3 * r if name.endswith("weight") else r
            elif name.endswith("frame_weights"):
                v = r / math.sqrt(p[0][0].numel())
            elif p.dim() > 1:
                v = r / math.sqrt(p[0].numel())
            else:
                v = 0.3 * r
            p.copy_(v.half().float() if half else v)


def grads_of(mod, out, probe, names=None):
    mod.zero_grad()
    (out * probe).sum().backward()
    return {n: p.grad.detach().clone().numpy() for n, p in mod.named_parameters() if names is None or any(n.startswith(s) for s in names)}


def decoder_cases():
    from scene.time_decoders import TimeVAEDecoder
    kw = dict(in_channels=8, out_channels=16, up_block_types=("TimeUpDecoderBlock2D",) * 4, block_out_channels=(16,) * 4, norm_num_groups=4,
              layers_per_block=1)
    # strategy 'none': everything
    g = torch.Generator().manual_seed(101)
    net = TimeVAEDecoder(**kw, layer_kwargs={"n_frames": 1, "strategy": "none"})
    overwrite(net, g)
    noise = torch.randn(1, 8, 3, 5, generator=g)
    out = net(noise, frame_id=None)
    probe = torch.randn(out.shape, generator=g)
    arrays = {"noise": noise.numpy(), "out": out.detach().numpy(), "probe": probe.numpy(), "groups": np.array(4)}
    arrays.update({"param/" + n: p.detach().numpy() for n, p in net.named_parameters()})
    arrays.update({"grad/" + n: v for n, v in grads_of(net, out, probe).items()})
    np.savez_compressed(os.path.join(HERE, "plane_decoder_small.npz"), **arrays)
    print("plane_decoder_small:", tuple(noise.shape), "->", tuple(out.shape), len(arrays), "arrays")

    # per_frame, three frames, two of them evaluated; float16-exact parameters, gradients of a subset
    g = torch.Generator().manual_seed(102)
    net = TimeVAEDecoder(**kw, layer_kwargs={"n_frames": 3, "strategy": "per_frame"})
    overwrite(net, g, half=True)
    noise = torch.randn(1, 8, 3, 5, generator=g).half().float()
    subset = ("conv_in.", "mid_block.resnets.0.", "up_blocks.2.resnets.1.conv1.", "up_blocks.3.resnets.0.conv2.", "conv_norm_out.", "conv_out.")
    arrays = {"noise": noise.half().numpy(), "groups": np.array(4), "frame_ids": np.array([0, 2])}
    arrays.update({"param/" + n: p.detach().half().numpy() for n, p in net.named_parameters()})
    for fid in (0, 2):
        out = net(noise, frame_id=fid)
        probe = torch.randn(out.shape, generator=g).half().float()
        arrays[f"out/{fid}"], arrays[f"probe/{fid}"] = out.detach().numpy(), probe.half().numpy()
        arrays.update({f"grad/{fid}/" + n: v for n, v in grads_of(net, out, probe, subset).items()})
    np.savez_compressed(os.path.join(HERE, "plane_decoder_per_frame.npz"), **arrays)
    print("plane_decoder_per_frame:", len(arrays), "arrays")


def tensorial2d_case():
    from scene.tripFields import Tensorial2D
    g = torch.Generator().manual_seed(103)
    mod = Tensorial2D(8, 16, 2, layer_kwargs={"n_frames": 0, "strategy": "none"})
    overwrite(mod, g, half=True)
    with torch.no_grad():
        mod.noise.copy_(torch.randn(mod.noise.shape, generator=g).half().float())
    out = mod(frame_id=None)
    probe = torch.randn(out.shape, generator=g).half().float()
    subset = ("net.conv_in.", "net.conv_out.", "net.conv_norm_out.", "net.up_blocks.1.resnets.0.")
    arrays = {"noise": mod.noise.half().numpy(), "out": out.detach().numpy(), "probe": probe.half().numpy(), "groups": np.array(32)}
    arrays.update({"param/" + n: p.detach().half().numpy() for n, p in mod.named_parameters()})
    arrays.update({"grad/" + n: v for n, v in grads_of(mod, out, probe, subset).items()})
    np.savez_compressed(os.path.join(HERE, "plane_decoder_tensorial2d.npz"), **arrays)
    print("plane_decoder_tensorial2d:", tuple(mod.noise.shape), "->", tuple(out.shape), len(arrays), "arrays")


def key_lists():
    from scene.tripFields import VarTriPlaneEncoder
    lists = {}
    for tag, layer_kwargs in (("none", {"n_frames": 0, "strategy": "none"}), ("per_frame", {"n_frames": 4, "strategy": "per_frame"})):
        enc = VarTriPlaneEncoder({"in_ch": 8, "out_ch": 16, "noise_res": 20, "layer_kwargs": layer_kwargs})
        lists[tag] = [[k, list(v.shape)] for k, v in enc.state_dict().items()]
        zero = [k for k, v in enc.state_dict().items() if v.is_floating_point() and not v.any()]
        lists[tag + "_zero"] = zero
        with torch.no_grad():
            lists[tag + "_plane_shape"] = list(enc.get_planes(frame_id=0).shape)
        print("keys", tag, len(lists[tag]), "tensors,", len(zero), "all zero, planes", lists[tag + "_plane_shape"])
    with open(os.path.join(HERE, "plane_decoder_keys.json"), "w") as f:
        json.dump(lists, f, indent=0)


if __name__ == "__main__":
    install_stand_ins(os.path.abspath(sys.argv[1]))
    decoder_cases()
    tensorial2d_case()
    key_lists()
