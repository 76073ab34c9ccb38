"""PyTorch statements of what the grouped head kernels compute (include/splatraster.h: sr_mlp_group_*), in the dtype of their
inputs: float64 for the references of tests/test_gpu_heads.py, float32 for the error scale those tests measure against, and
as CPU stand-ins for the kernels in tests/test_heads_grouping.py."""
import contextlib

import torch
import torch.nn.functional as F


def encoding(x, multires):
    """[x, sin(2^0 x), cos(2^0 x), ...]: reference utils/time_utils.py:9-57"""
    parts = [x]
    for j in range(multires):
        parts += [torch.sin(x * float(2 ** j)), torch.cos(x * float(2 ** j))]
    return torch.cat(parts, dim=-1)


def input_matrix(xyz, feat, time, multires, time_multires, row):
    parts = [encoding(xyz, multires)] + ([feat] if feat is not None else []) + \
        ([encoding(time.reshape(-1, 1), time_multires)] if time is not None else [])
    x = torch.cat(parts, dim=-1)
    return F.pad(x, (0, row - x.shape[1]))


def input_backward(xyz, dx0s, multires, n_feat):
    """(d_xyz, d_feat): the sum over the heads of each head's input-kernel backward"""
    d_xyz, d_feat = torch.zeros_like(xyz), xyz.new_zeros(xyz.shape[0], n_feat)
    for g, L in zip(dx0s, multires):
        d = g[:, 0:3].clone()
        for j in range(L):
            f = float(2 ** j)
            d = d + f * (torch.cos(xyz * f) * g[:, 3 + 6 * j:6 + 6 * j] - torch.sin(xyz * f) * g[:, 6 + 6 * j:9 + 6 * j])
        d_xyz = d_xyz + d
        d_feat = d_feat + g[:, 3 + 6 * L:3 + 6 * L + n_feat]
    return d_xyz, d_feat


def output(y, activation):
    if activation == "sigmoid":
        return 1.0 / (1.0 + torch.exp(-y))
    if activation == "normalize":
        return y / y.norm(dim=-1, keepdim=True).clamp_min(1e-12)
    return y.clone()


def top_gradient(y, d, activation, slope, row):
    """dOut o act'(.) o leaky'(y), zero-padded to `row`; d None: zeros"""
    if d is None:
        return y.new_zeros(y.shape[0], row)
    g = d
    if activation == "sigmoid":
        s = 1.0 / (1.0 + torch.exp(-y))
        g = d * s * (1.0 - s)
    elif activation == "normalize":          # general_mlp._Normalize.backward
        raw = y.norm(dim=-1, keepdim=True)
        n = raw.clamp_min(1e-12)
        u = y / n
        g = torch.where(raw > 1e-12, d - u * (d * u).sum(dim=-1, keepdim=True), d) / n
    g = g * torch.where(y > 0, 1.0, slope).to(y.dtype)
    return F.pad(g, (0, row - y.shape[1]))


def weight_grads(shape, x0, acts, G, dz, weights):
    """the contraction sr_mlp_weight_grad performs on the stored buffers"""
    dWs, dbs = [], []
    for j in range(shape.n_layers):
        dZ = G[:, :shape.out_features] if j == shape.n_layers - 1 else dz[j]
        segments = ([x0[:, :shape.d_in]] if shape.reads_input[j] else []) + ([acts[j - 1]] if j > 0 else [])
        dWs.append(dZ.t() @ torch.cat(segments, 1))
        dbs.append(dZ.sum(0))
    return dWs, dbs


def on_cpu(monkeypatch, counts=None):
    """Routes the grouped path through CPU stand-ins: the op-list interpreter of tests/test_fused_mlp_oplist.py for the pack +
    chain launches, the formulas above for the small kernels.  `counts` (a dict) receives how often each stand-in ran."""
    from splatfields_amd import _lib, deform_field, fused_mlp as fm, general_mlp
    from test_fused_mlp_oplist import interpret
    from test_general_mlp import formula
    counts = {} if counts is None else counts

    def hit(name):
        counts[name] = counts.get(name, 0) + 1

    class _Stream:
        cuda_stream = 0

    def run_group(self, lib, ptrs_per_net, device, n, ht, slope, stream):
        hit("chain_group")
        for plan, ptrs in zip(self.plans, ptrs_per_net):
            interpret(plan, lib, ptrs, device, n, ht, slope, stream)

    def input_forward(lib, heads, time_multires, x32, f32, t32, x0s):
        hit("input_forward")
        for h, x0 in zip(heads, x0s):
            x0.copy_(input_matrix(x32, f32, t32, h.multires, time_multires, h.shape.mem_pad))

    def input_back(lib, heads, n_feat, x32, dx0s, d_xyz, d_feat):
        hit("input_backward")
        dx, df = input_backward(x32, dx0s, [h.multires for h in heads], n_feat)
        if d_xyz is not None:
            d_xyz.copy_(dx)
        if d_feat is not None:
            d_feat.copy_(df)

    def group_output(lib, heads, ys):
        hit("output")
        return [y if h.activation == "none" else output(y, h.activation) for h, y in zip(heads, ys)]

    def group_top(lib, heads, ys, dOuts, slope, Gs):
        hit("top_gradient")
        for h, y, d, G in zip(heads, ys, dOuts, Gs):
            G.copy_(top_gradient(y, d, h.activation, slope, h.shape.out_pad))

    def fuse_time(self, xyz_in, t):      # SplatFields._fuse_time without "on the device"
        return self.n_frames > 0 and torch.is_tensor(t) and t.dtype == torch.float32 and not t.requires_grad and \
            t.numel() == xyz_in.shape[0] and not self.geo_model_disable_pts

    monkeypatch.setattr(_lib, "load", lambda: None)
    monkeypatch.setattr(torch.cuda, "device", lambda d: contextlib.nullcontext())
    monkeypatch.setattr(torch.cuda, "current_stream", lambda d=None: _Stream())
    monkeypatch.setattr(fm._GroupPlan, "run", run_group)
    monkeypatch.setattr(fm, "_group_input_forward", input_forward)
    monkeypatch.setattr(fm, "_group_input_backward", input_back)
    monkeypatch.setattr(fm, "_group_output", group_output)
    monkeypatch.setattr(fm, "_group_top_gradient", group_top)
    monkeypatch.setattr(fm, "_weight_grads", weight_grads)
    monkeypatch.setattr(fm, "grouped_inputs_ok", lambda xyz, feat, time: xyz.shape[0] > 0)
    monkeypatch.setattr(deform_field.SplatFields, "_fuse_time", fuse_time)
    monkeypatch.setattr(general_mlp, "fused_general_mlp", formula)      # mlp_deform, and every net of the separate path
    return counts


class LinearEncoder(torch.nn.Module):
    """a small pure-PyTorch encoder with the encoder interface of SplatFields: encoder(x[None]) -> [1, N, out_dim]"""
    out_dim = 16

    def __init__(self):
        super().__init__()
        self.lin = torch.nn.Linear(3, self.out_dim)

    def forward(self, x):
        return torch.tanh(self.lin(x))


def step(net, xyz, t, viewdir, probes):
    """one forward + backward of sum(output * probe): ({name: output}, {name: gradient}) with "xyz" and every parameter"""
    for p in net.parameters():
        p.grad = None
    xyz = xyz.detach().clone().requires_grad_()
    out = net(xyz, t)
    if "rgb_fnc" in out:
        out = dict(out, rgb=out["rgb_fnc"](viewdir))
        del out["rgb_fnc"]
    out = {k: v for k, v in out.items() if v is not None}
    loss = 0.0
    for k in sorted(out):
        loss = loss + (out[k] * probes[k].to(out[k])).sum()
    loss.backward()
    grads = {"xyz": xyz.grad}
    for k, p in net.named_parameters():
        grads[k] = p.grad if p.grad is not None else torch.zeros_like(p)
    return {k: v.detach() for k, v in out.items()}, {k: v.detach().clone() for k, v in grads.items()}
