"""The set-up that the GPU tests of the grouped head networks (tests/test_gpu_heads.py) and of the bf16x3 chains
(tests/test_gpu_mlp_bf16x3.py) share: the op tables and random nets of the chain kernels, the module configurations with their CPU
references (computed once), the bound both hold the module to, and which kernel names count as the library's."""
import functools

import torch

import heads_reference as hr
from tests import accuracy


def bound(ref64, *approximations):
    """accuracy.bound with the ulp floor taken at 1e-30 where the tensor's maximum is smaller"""
    floor = accuracy.FACTOR * accuracy.ulp32(max(ref64.abs().max().item(), 1e-30))
    return max(accuracy.bound(ref64, *approximations, floor=False), floor)


def default_specs(dynamic=True):
    from splatfields_amd.deform_field import SplatFields
    torch.manual_seed(11)
    net = SplatFields(n_frames=5 if dynamic else 0, heads="grouped", encoder=hr.LinearEncoder())
    return net._head_group.specs, net.time_multires


def chain_groups():
    from splatfields_amd import fused_mlp as fm
    specs, _ = default_specs()
    s64, s128 = [s.shape for s in specs[:3]], [s.shape for s in specs[3:]]
    small = fm._Shape([torch.zeros(64, 21), torch.zeros(64, 64), torch.zeros(5, 64)], 21, [])      # 3 ops forward, 3 backward
    return {"three_64": s64, "two_128": s128, "one_net": [s64[2]], "net_limit": [small] * 8}


def make_net(shape, n, gen, dev):
    ws = [(torch.randn(r, c, generator=gen) / c ** 0.5).to(dev) for r, c in shape.layer_dims]
    bs = [(0.1 * torch.randn(r, generator=gen)).to(dev) for r, _ in shape.layer_dims]
    x0 = torch.zeros(n, shape.mem_pad)
    x0[:, :shape.d_in] = torch.randn(n, shape.d_in, generator=gen)
    return ws, bs, x0.to(dev), torch.randn(n, shape.out_features, generator=gen).to(dev)


MODULE_CONFIGS = {
    "static": dict(n_frames=0, kwargs=dict()),
    "dynamic_se3": dict(n_frames=6, kwargs=dict(composition_rank=4, flow_model="se3")),
    "viewdep": dict(n_frames=0, kwargs=dict(use_view_dep_rgb=True)),
}


def build_net(name, with_encoder, **extra):
    from splatfields_amd.deform_field import SplatFields
    cfg = MODULE_CONFIGS[name]
    torch.manual_seed(21)
    enc = dict(encoder=hr.LinearEncoder()) if with_encoder else dict(encoder_type="none")
    return SplatFields(n_frames=cfg["n_frames"], **enc, **cfg["kwargs"], **extra)


def module_inputs(n):
    gen = torch.Generator().manual_seed(40 + n)
    xyz = 0.6 * torch.randn(n, 3, generator=gen)
    t = torch.full((n, 1), 0.4)
    viewdir = torch.nn.functional.normalize(torch.randn(n, 3, generator=gen), dim=-1)
    return xyz, t, viewdir, gen


@functools.lru_cache(maxsize=None)
def cpu_references(name, with_encoder, n):
    """(state dict, probes, float64 outputs and gradients, float32 outputs and gradients) of the CPU formula path: computed once,
    shared by the precisions"""
    from splatfields_amd import general_mlp
    from test_general_mlp import formula
    xyz, t, viewdir, gen = module_inputs(n)
    net = build_net(name, with_encoder)
    state = {k: v.clone() for k, v in net.state_dict().items()}
    real = general_mlp.fused_general_mlp
    general_mlp.fused_general_mlp = formula
    try:
        first, _ = hr.step(net, xyz, t, viewdir, {k: torch.ones(1) for k in ("scales", "opacity", "rotations", "rgb", "flow", "means3D")})
        probes = {k: torch.randn(v.shape, generator=gen) for k, v in first.items()}
        f32 = hr.step(net, xyz, t, viewdir, probes)
        net64 = build_net(name, with_encoder).double()
        net64.load_state_dict({k: v.double() for k, v in state.items()})
        f64 = hr.step(net64, xyz.double(), t.double(), viewdir.double(), probes)
    finally:
        general_mlp.fused_general_mlp = real
    return state, probes, f64, f32


def library(names):
    return [n for n in names if "k_mlp_" in n or "k_resfield_" in n]
