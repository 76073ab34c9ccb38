"""The bf16 precision of the fused MLP chains restated in plain PyTorch (any device, float32 or float64): the yardstick of
sr_mlp_chain_bf16 on machines where the reference checkout is absent.  tests/test_mlp_bf16_reference.py pins it to the
reference's own GeneralMLP, run with a rounding `F.linear`, through tests/golden/mlp_bf16_cases.npz.

With bf(.) = round to nearest even to bfloat16 (the value is kept in the working dtype):

    forward, every layer      z = b + bf(W) . bf(x),   x = [h_in | h] or h;   h <- leaky(z)        products, sums, b, h: working dtype
    backward, every layer     dx = bf(dz) . bf(W)      (dz = dL/dh * leaky'(z): what autograd hands the linear op)
                              dW = dz^T x,  db = sum dz                        from the UNROUNDED x and dz

so a value is rounded exactly where it enters a matrix product of a layer chain and nowhere else: not the bias, not what the
activation sees, not the operands of the weight gradients.  Everything around the layer loop is the reference's fp arithmetic:
positional encoding, feature concatenation, ResField composition W + (weights_t[frame] @ matrix_t) (the rounding applies to
the composed weight), the output activation.

`exact_case` builds networks on which all of this is EXACT arithmetic in float32 (see there): the HIP kernels must then
reproduce the restatement bit for bit, whatever order they add in."""
from __future__ import annotations

import torch
import torch.nn.functional as F


def bf16_round(x: torch.Tensor) -> torch.Tensor:
    """Round to nearest even to bfloat16, by integer arithmetic on the float32 bit pattern (ties go to the even 7-bit mantissa;
    the carry of a rounded-up mantissa runs into the exponent, up to infinity; NaN stays NaN).  Returned in x's dtype."""
    u = x.detach().to(torch.float32).contiguous().view(torch.int32).to(torch.int64) & 0xFFFFFFFF
    r = ((u + 0x7FFF + ((u >> 16) & 1)) & 0xFFFF0000)
    nan = (u & 0x7FFFFFFF) > 0x7F800000
    r = torch.where(nan, u | 0x00400000, r) & 0xFFFFFFFF
    r = torch.where(r >= 0x80000000, r - 0x100000000, r).to(torch.int32)
    return r.view(torch.float32).to(x.dtype)


class _BfLinear(torch.autograd.Function):
    """y = bf(x) bf(W)^T + b;  dx = bf(dy) bf(W),  dW = dy^T x,  db = sum dy.  `mm(a, b)` = a @ b: the summation order is the
    caller's (tests/test_mlp_bf16_reference.py evaluates the exact networks in two orders)."""

    @staticmethod
    def forward(ctx, x, W, b, mm):
        ctx.save_for_backward(x, W)
        ctx.mm = mm
        return mm(bf16_round(x), bf16_round(W).t()) + b

    @staticmethod
    def backward(ctx, dy):
        x, W = ctx.saved_tensors
        return ctx.mm(bf16_round(dy), bf16_round(W)), dy.t() @ x, dy.sum(0), None


def bf_linear(x, W, b, mm=torch.matmul):
    return _BfLinear.apply(x, W, b, mm)


def sequential_mm(order: str):
    """a @ b with the K terms of every output added one after the other, first to last ("forward") or last to first."""
    def mm(a, b):
        prod = a[:, :, None] * b[None, :, :]                     # [n, K, m]
        if order == "backward":
            prod = prod.flip(1)
        acc = torch.zeros_like(prod[:, 0])
        for k in range(prod.shape[1]):
            acc = acc + prod[:, k]
        return acc
    return mm


def mlp_chain(h_in, weights, biases, skips=(), negative_slope=0.01, mm=torch.matmul):
    """The layer loop (reference utils/time_utils.py:184-188) with the rounding linear op."""
    h = h_in
    for i, (W, b) in enumerate(zip(weights, biases)):
        h = F.leaky_relu(bf_linear(h, W, b, mm), negative_slope)
        if i in set(skips) and i != len(weights) - 1:
            h = torch.cat([h_in, h], dim=-1)
    return h


def positional_encoding(x, multires):
    out = [x]
    for j in range(max(multires, 0)):
        out += [torch.sin(x * float(2 ** j)), torch.cos(x * float(2 ** j))]
    return torch.cat(out, dim=-1) if len(out) > 1 else x


_OUT_ACT = {"none": lambda x: x, "sigmoid": torch.sigmoid, "tanh": torch.tanh, "normalize": lambda x: F.normalize(x, dim=-1)}
_SLOPE = {"leaky_relu": 0.01, "relu": 0.0}


def general_mlp(params: dict, kwargs: dict, xyz, feat=None, frame=None):
    """A whole GeneralMLP (reference utils/time_utils.py:123-191, ResField layers in the 'vm' / 'lookup' / 'add' configuration)
    under the bf16 semantics.  `params`: the module's state dict as leaf tensors ("net.<i>.weight", ".bias", and for ResField
    layers ".weights_t" [capacity, rank], ".matrix_t" [rank, out * in]); `kwargs`: its constructor arguments."""
    n_layers = kwargs["num_hidden_layers"] + 2
    weights, biases = [], []
    for i in range(n_layers):
        W = params[f"net.{i}.weight"]
        if f"net.{i}.matrix_t" in params:
            W = W + (params[f"net.{i}.weights_t"][frame].reshape(1, -1) @ params[f"net.{i}.matrix_t"]).view_as(W)
        weights.append(W)
        biases.append(params[f"net.{i}.bias"])
    h_in = positional_encoding(xyz, kwargs["multires"])
    if feat is not None:
        h_in = torch.cat([h_in, feat], dim=-1)
    h = mlp_chain(h_in, weights, biases, kwargs["skips"], _SLOPE[kwargs["act"]])
    return _OUT_ACT[kwargs["out_activation"]](h)


# ---- networks on which the bf16 semantics are exact arithmetic ---------------------------------------------------------------
EXACT_SLOPE = 0.25
EXACT_SHAPES = {
    # name: (layer widths, d_in, skips)
    "wide": ([128] * 5 + [16], 64, [2]),      # hidden_tiles 8; the input enters layers 0 and 3; 16 of 128 output channels
    "narrow": ([64] * 4 + [3], 32, [1]),      # hidden_tiles 4; one input chunk; an output row of 3 floats
}


def exact_case(name: str, n_points: int, seed: int = 0, dtype=torch.float32):
    """-> (h_in [n, d_in], weights, biases, skips, dY [n, out]).  Inputs and dY lie on the 2^-6 grid in [-1, 1], biases on that
    grid in [-1/8, 1/8], every weight row has 8 non-zeros from {+-1/8, +-1/4}, the slope is 1/4: every product is a power of two
    times an (at most) 8-bit operand, every sum has 8 terms (+ the bias), and all partial sums stay exactly representable in
    float32 -- in any order, which tests/test_mlp_bf16_reference.py checks against float64 for the cases the GPU test uses."""
    widths, d_in, skips = EXACT_SHAPES[name]
    g = torch.Generator().manual_seed(1000 + seed)
    weights, biases = [], []
    for j, out in enumerate(widths):
        cols = d_in if j == 0 else widths[j - 1] + (d_in if (j - 1) in skips else 0)
        W = torch.zeros(out, cols, dtype=dtype)
        for r in range(out):
            idx = torch.randperm(cols, generator=g)[:8]
            mag = torch.tensor([0.125, 0.25], dtype=dtype)[torch.randint(0, 2, (8,), generator=g)]
            W[r, idx] = mag * (2 * torch.randint(0, 2, (8,), generator=g) - 1).to(dtype)
        weights.append(W)
        biases.append(torch.randint(-8, 9, (out,), generator=g).to(dtype) / 64)
    h_in = torch.randint(-64, 65, (n_points, d_in), generator=g).to(dtype) / 64
    dY = torch.randint(-64, 65, (n_points, widths[-1]), generator=g).to(dtype) / 64
    return h_in, weights, biases, skips, dY


def run_chain(h_in, weights, biases, skips, dY, slope=EXACT_SLOPE, mm=torch.matmul, dtype=None):
    """forward + backward of `mlp_chain` -> dict(y, d_in, dW [list], db [list]), evaluated in `dtype` (default: the inputs')."""
    cast = (lambda t: t.detach().to(dtype)) if dtype is not None else (lambda t: t.detach().clone())
    x = cast(h_in).requires_grad_()
    ws, bs = [cast(w).requires_grad_() for w in weights], [cast(b).requires_grad_() for b in biases]
    y = mlp_chain(x, ws, bs, skips, slope, mm)
    y.backward(cast(dY))
    return dict(y=y.detach(), d_in=x.grad, dW=[w.grad for w in ws], db=[b.grad for b in bs])


# ---- the fixture tests/golden/mlp_bf16_cases.npz (tests/golden/make_mlp_bf16_golden.py) ----------------------------------------
def load_fixture_case(golden_dir: str, name: str):
    """-> (constructor kwargs, data of general_mlp_<name>.npz, emul64 {tensor: float64 array}, e_fmt {tensor: float}, rho).  The
    `.matrix_t` gradients of emul64 are not stored: d matrix_t = weights_t[frame] (x) d weight, rebuilt here in float64."""
    import importlib.util
    import os

    import numpy as np
    spec = importlib.util.spec_from_file_location("make_golden", os.path.join(golden_dir, "make_golden.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)                      # definitions only; nothing is generated, no reference checkout is touched
    kwargs = mod.GENERAL_MLP_CASES[name][0]
    data = np.load(os.path.join(golden_dir, f"general_mlp_{name}.npz"))
    fx = np.load(os.path.join(golden_dir, "mlp_bf16_cases.npz"))
    pre = f"{name}/emul64/"
    emul = {k[len(pre):]: fx[k].astype(np.float64) for k in fx.files if k.startswith(pre)}
    frame = int(data["frame_id"])
    for k in [k for k in data.files if k.startswith("param:") and k.endswith(".matrix_t")]:
        layer = k[len("param:"):-len(".matrix_t")]
        coeff = data[f"param:{layer}.weights_t"][frame].astype(np.float64)
        emul[f"grad:{layer}.matrix_t"] = np.outer(coeff, emul[f"grad:{layer}.weight"].reshape(-1))
    e_fmt = {k[len(f"{name}/e_fmt/"):]: float(fx[k]) for k in fx.files if k.startswith(f"{name}/e_fmt/")}
    return kwargs, data, emul, e_fmt, float(fx["rho"])


def run_module(name, device, precision="unset", data=None, kwargs=None):
    """forward + backward of GeneralMLP on a committed case -> {tensor name: float64 CPU tensor}"""
    import os

    from splatfields_amd.general_mlp import GeneralMLP
    if data is None:
        kwargs, data, _, _, _ = load_fixture_case(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"), name)
    net = GeneralMLP(**kwargs) if precision == "unset" else GeneralMLP(**kwargs, precision=precision)
    net.load_state_dict({k[len("param:"):]: torch.from_numpy(data[k]) for k in data.files if k.startswith("param:")}, strict=True)
    net = net.to(device)
    xyz = torch.from_numpy(data["xyz"]).to(device).requires_grad_()
    feat = torch.from_numpy(data["feat"]).to(device).requires_grad_() if "feat" in data.files else None
    frame = int(data["frame_id"])
    out = net(xyz, feat, frame_id=None if frame < 0 else torch.tensor(frame, device=device))
    (out * torch.from_numpy(data["probe"]).to(device)).sum().backward()
    res = {"out": out.detach(), "grad_xyz": xyz.grad}
    if feat is not None:
        res["grad_feat"] = feat.grad
    for k, p in net.named_parameters():
        res["grad:" + k] = p.grad if p.grad is not None else torch.zeros_like(p)
    return {k: v.cpu().double() for k, v in res.items()}
