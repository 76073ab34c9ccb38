"""The split-bf16 ("bf16x3") precision of the fused MLP chains restated in plain PyTorch (any device, float32 or float64): the
yardstick of sr_mlp_chain_bf16x3 on machines where the reference checkout is absent.  tests/test_mlp_bf16x3_reference.py pins it to
the reference's own GeneralMLP, run with a splitting `F.linear`, through tests/golden/mlp_bf16x3_cases.npz.

With bf(.) = round to nearest even to bfloat16 (tests/mlp_bf16_reference.py: bf16_round; the value is kept in the working dtype),
hi(v) = bf(v) and lo(v) = bf(v - hi(v)) (the subtraction is exact in float32):

    forward, every layer      z = b + hi(W) . hi(x) + hi(W) . lo(x) + lo(W) . hi(x),   x = [h_in | h] or h;   h <- leaky(z)
    backward, every layer     dx = hi(dz) . hi(W) + lo(dz) . hi(W) + hi(dz) . lo(W)     (dz = dL/dh * leaky'(z))
                              dW = dz^T x,  db = sum dz                                  from the UNSPLIT x and dz

lo . lo is dropped.  A value is split exactly where it enters a matrix product of a layer chain and nowhere else: not the bias, not
what the activation sees, not the operands of the weight gradients; everything around the layer loop is the reference's arithmetic
(tests/mlp_bf16_reference.py: general_mlp).  A non-finite operand has lo = inf - inf = NaN, a finite one that bf(.) rounds to
+-inf has lo = -+inf: what such an operand reaches is not finite.

`exact_case` builds networks on which all of this is EXACT arithmetic in float32 (see there): the HIP kernels must then reproduce
the restatement bit for bit, whatever order they add in."""
from __future__ import annotations

import torch
import torch.nn.functional as F

import mlp_bf16_reference as B
from mlp_bf16_reference import bf16_round, positional_encoding, sequential_mm  # noqa: F401  (re-exported)

TERMS = ("hh", "hl", "lh")          # (part of W)(part of x or dz); the kernels add them in this order into one accumulator


def split(v: torch.Tensor):
    """-> (hi, lo) in v's dtype; the subtraction is exact in float32 and in float64"""
    v = v.detach()
    hi = bf16_round(v)
    return hi, bf16_round(v - hi)


def split_product(a, b_t, mm, terms=TERMS):
    """a . b_t with both operands split: sum over `terms` of part(b) . part(a), first letter = the part of the WEIGHT operand b_t"""
    (ah, al), (bh, bl) = split(a), split(b_t)
    part = {"hh": (ah, bh), "hl": (al, bh), "lh": (ah, bl), "ll": (al, bl)}
    acc = None
    for t in terms:
        p = mm(*part[t])
        acc = p if acc is None else acc + p
    return acc


class _SplitLinear(torch.autograd.Function):
    """y = b + split product of x and W^T;  dx = split product of dy and W,  dW = dy^T x,  db = sum dy.  `mm(a, b)` = a @ b: the
    summation order is the caller's."""

    @staticmethod
    def forward(ctx, x, W, b, mm, terms):
        ctx.save_for_backward(x, W)
        ctx.mm, ctx.terms = mm, terms
        return split_product(x, W.t(), mm, terms) + b

    @staticmethod
    def backward(ctx, dy):
        x, W = ctx.saved_tensors
        return split_product(dy, W, ctx.mm, ctx.terms), dy.t() @ x, dy.sum(0), None, None


def split_linear(x, W, b, mm=torch.matmul, terms=TERMS):
    return _SplitLinear.apply(x, W, b, mm, terms)


def mlp_chain(h_in, weights, biases, skips=(), negative_slope=0.01, mm=torch.matmul, terms=TERMS):
    """The layer loop (reference utils/time_utils.py:184-188) with the splitting linear op."""
    h = h_in
    for i, (W, b) in enumerate(zip(weights, biases)):
        h = F.leaky_relu(split_linear(h, W, b, mm, terms), negative_slope)
        if i in set(skips) and i != len(weights) - 1:
            h = torch.cat([h_in, h], dim=-1)
    return h


def general_mlp(params: dict, kwargs: dict, xyz, feat=None, frame=None):
    """A whole GeneralMLP under the bf16x3 semantics: tests/mlp_bf16_reference.py's `general_mlp` with this module's layer loop."""
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
    h = mlp_chain(h_in, weights, biases, kwargs["skips"], B._SLOPE[kwargs["act"]])
    return B._OUT_ACT[kwargs["out_activation"]](h)


# ---- networks on which the bf16x3 semantics are exact arithmetic --------------------------------------------------------------
# A weight with a non-zero low part carries >= 9 more bits than its high part, an input with one >= 10 bits: a float32 sum (24 bits)
# holds ONE such product layer and one layer of power-of-two weights behind it, not the five layers of the bf16 networks.
EXACT_SLOPE = 0.5
EXACT_SHAPES = {
    # name: (hidden, d_in, out); two layers, the input concatenated back in front of layer 1 (skips = [0])
    "wide": (128, 64, 16),        # hidden_tiles 8; two input chunks; 16 of 128 output channels
    "narrow": (64, 32, 3),        # hidden_tiles 4; one input chunk; an output row of 3 floats
}


def exact_case(name: str, n_points: int, seed: int = 0, dtype=torch.float32):
    """-> (h_in [n, d_in], weights, biases, skips, dY [n, out]).

    Inputs on the 2^-9 grid in [-1, 1] (10 bits: a non-zero low part from 1/2 on); biases on the 2^-6 grid in [-1/8, 1/8].
    Layer 0: every row has 2 non-zeros +-(1/4 +- 2^-11) (hi = +-1/4, lo = +-2^-11) and every column of the matrix the same number
    of them (d W_0^T is a sum over them): z_0 lies on the 2^-20 grid below 0.63, h_0 = leaky(z_0, 1/2) on the 2^-21 grid -- 20 bits,
    so the register state has low parts.  Layer 1 reads [h_in | h_0] with 4 non-zeros +-1/4 per row, at most one per column: z_1 on
    the 2^-23 grid below 1.13.  Backward: dY on the 2^-9 grid in [-1, 1], G = dY * leaky'(y) on the 2^-10 grid (low parts in the top
    gradient's memory channels); dZ_0 = (W_1^T G) * leaky' has one term per entry, up to 10 bits on the 2^-13 grid below 1/4 (low
    parts in the backward's register state); W_0^T dZ_0 lies on the 2^-24 grid below 1/4, dL/dh_in = W_1[:, input]^T G + W_0^T dZ_0
    below 1/2.  Every product is 8 bits x 8 bits and every partial sum stays representable in float32 -- in any order, which
    tests/test_mlp_bf16x3_reference.py checks against float64 for the cases the GPU test uses."""
    H, d_in, out = EXACT_SHAPES[name]
    g = torch.Generator().manual_seed(3000 + seed)
    sign = lambda n: (2 * torch.randint(0, 2, (n,), generator=g) - 1).to(dtype)
    # layer 0: row r has its non-zeros at columns perm[(2 r) % d_in] and perm[(2 r + 1) % d_in]: 2 H / d_in per column
    perm = torch.randperm(d_in, generator=g)
    W0 = torch.zeros(H, d_in, dtype=dtype)
    for r in range(H):
        cols = perm[[(2 * r) % d_in, (2 * r + 1) % d_in]]
        W0[r, cols] = sign(2) * (0.25 + sign(2) * 2.0 ** -11)
    W1 = torch.zeros(out, d_in + H, dtype=dtype)
    cols1 = torch.randperm(d_in + H, generator=g)             # 4 non-zeros per row, at most one per column
    for r in range(out):
        W1[r, cols1[4 * r:4 * r + 4]] = 0.25 * sign(4)
    weights = [W0, W1]
    biases = [torch.randint(-8, 9, (m,), generator=g).to(dtype) / 64 for m in (H, out)]
    h_in = torch.randint(-512, 513, (n_points, d_in), generator=g).to(dtype) / 512
    dY = torch.randint(-512, 513, (n_points, out), generator=g).to(dtype) / 512
    return h_in, weights, biases, [0], dY


def run_chain(h_in, weights, biases, skips, dY, slope=EXACT_SLOPE, mm=torch.matmul, dtype=None, terms=TERMS):
    """forward + backward of `mlp_chain` -> dict(y, d_in, dW [list], db [list]), evaluated in `dtype` (default: the inputs')."""
    cast = (lambda t: t.detach().to(dtype)) if dtype is not None else (lambda t: t.detach().clone())
    x = cast(h_in).requires_grad_()
    ws, bs = [cast(w).requires_grad_() for w in weights], [cast(b).requires_grad_() for b in biases]
    y = mlp_chain(x, ws, bs, skips, slope, mm, terms)
    y.backward(cast(dY))
    return dict(y=y.detach(), d_in=x.grad, dW=[w.grad for w in ws], db=[b.grad for b in bs])


# ---- the fixture tests/golden/mlp_bf16x3_cases.npz (tests/golden/make_mlp_bf16x3_golden.py) -------------------------------------
def load_fixture_case(golden_dir: str, name: str):
    """-> (constructor kwargs, data of general_mlp_<name>.npz, emul64 {tensor: float64 array}, e_fmt3 {tensor: float},
    e_32 {tensor: float}).  The `.matrix_t` gradients of emul64 are not stored: d matrix_t = weights_t[frame] (x) d weight, rebuilt
    here in float64."""
    import importlib.util
    import os

    import numpy as np
    spec = importlib.util.spec_from_file_location("make_golden", os.path.join(golden_dir, "make_golden.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)                      # definitions only; nothing is generated, no reference checkout is touched
    kwargs = mod.GENERAL_MLP_CASES[name][0]
    data = np.load(os.path.join(golden_dir, f"general_mlp_{name}.npz"))
    fx = np.load(os.path.join(golden_dir, "mlp_bf16x3_cases.npz"))
    pre = f"{name}/emul64/"
    emul = {k[len(pre):]: fx[k].astype(np.float64) for k in fx.files if k.startswith(pre)}
    frame = int(data["frame_id"])
    for k in [k for k in data.files if k.startswith("param:") and k.endswith(".matrix_t")]:
        layer = k[len("param:"):-len(".matrix_t")]
        coeff = data[f"param:{layer}.weights_t"][frame].astype(np.float64)
        emul[f"grad:{layer}.matrix_t"] = np.outer(coeff, emul[f"grad:{layer}.weight"].reshape(-1))
    table = lambda key: {k[len(f"{name}/{key}/"):]: float(fx[k]) for k in fx.files if k.startswith(f"{name}/{key}/")}
    return kwargs, data, emul, table("e_fmt3"), table("e_32")
