"""The flow head of the deform network on its HIP kernels (include/splatraster.h: sr_flow_head_*; csrc/flow_head.hip).

`fused_flow_head(model, hidden, pts, weights, biases, bases)` evaluates one `FlowHead` of reference utils/time_utils.py:194-304
-- the branch linears z = hidden W^T + b of the model, and the per-point epilogue that turns z and the point into `flow` and
`means3D` -- in ONE launch, and is differentiable: the backward is one kernel that re-derives the epilogue from the saved z
(doubles) and writes dL/dpts, dL/dz and dL/dhidden = dz W, plus one weight_grad.run call (two kernels) for the weight and bias
gradients of every branch.  For the two DCT models the same backward kernel leaves one partial sum of dL/dbases per workgroup
(doubles, workgroup = 256 consecutive points, whatever the device), which a `sum(0)` adds.  float32 tensors, double arithmetic
inside the kernels, one rounding per stored value, no atomics, no host wait: repeated calls are bit-identical.  No CPU path.

Opt-in: `FlowHead(path="fused")`, `SplatFields(flow_head="fused")`, `set_flow_head("fused")` or SPLATFIELDS_FLOW_HEAD=fused; the
process default is "torch" (the PyTorch-op path of splatfields_amd/deform_field.py)."""
from __future__ import annotations

import os
from typing import Optional, Sequence

import torch

from . import _lib, weight_grad

FLOW_HEADS = ("torch", "fused")
FLOW_HEAD_LAUNCHES = (1, 3)      # library kernels of the "fused" head: (forward, backward: the epilogue + weight_grad.run's two)
# model -> (SR_FLOW_* code, rows of its branches in the order of the z layout; None = 3 * n_basis)
MODELS = {"offset": (_lib.FLOW_OFFSET, (3,)), "se3": (_lib.FLOW_SE3, (3, 3)), "se3Affine": (_lib.FLOW_SE3_AFFINE, (3, 3, 3)),
          "se3Scaled": (_lib.FLOW_SE3_SCALED, (3, 3, 1, 3)), "affine": (_lib.FLOW_AFFINE, (9, 3)), "dct": (_lib.FLOW_DCT, (None,)),
          "dct_siren": (_lib.FLOW_DCT, (None,))}


def checked_flow_head(name) -> str:
    if name not in FLOW_HEADS:
        raise ValueError(f"unknown flow-head path {name!r}: expected one of {FLOW_HEADS}")
    return name


# process default of the flow head, read once: SPLATFIELDS_FLOW_HEAD=fused turns the HIP kernels on for every head that does not
# name a path itself
_FLOW_HEAD = checked_flow_head(os.environ.get("SPLATFIELDS_FLOW_HEAD") or "torch")


def set_flow_head(name: str) -> str:
    """Process default of the flow head: "torch" (PyTorch ops) or "fused" (csrc/flow_head.hip).  Returns the previous setting."""
    global _FLOW_HEAD
    prev, _FLOW_HEAD = _FLOW_HEAD, checked_flow_head(name)
    return prev


def flow_head_path() -> str:
    return _FLOW_HEAD


def resolve_flow_head(name: Optional[str]) -> str:
    """`None` -> the process default, at call time."""
    return _FLOW_HEAD if name is None else checked_flow_head(name)


def branch_rows(model: str, n_basis: int):
    return tuple(3 * n_basis if r is None else r for r in MODELS[model][1])


def fused_shape_error(model: str, width: int, n_basis: int) -> Optional[str]:
    """why the kernels refuse this head, or None (the limits of include/splatraster.h, restated so that a module can be refused
    at construction without the library)"""
    if model not in MODELS:
        return f"unknown flow model {model!r}"
    if width < 4 or width % 4 or width > _lib.FLOW_MAX_WIDTH:
        return f"the hidden width must be a multiple of 4 in 4..{_lib.FLOW_MAX_WIDTH}, got {width}"
    if model in ("dct", "dct_siren") and not (1 <= n_basis <= _lib.FLOW_MAX_BASIS):
        return f"the number of DCT bases must be in 1..{_lib.FLOW_MAX_BASIS}, got {n_basis}"
    return None


def _branch_table(weights, biases):
    table = (_lib.SrFlowBranch * len(weights))()
    for i, (w, b) in enumerate(zip(weights, biases)):
        table[i].weight, table[i].bias, table[i].rows = w.data_ptr(), b.data_ptr(), w.shape[0]
    return table


class _FlowHeadFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, model, n_basis, grad_enabled, hidden, pts, bases, *params):
        lib = _lib.load()
        code = MODELS[model][0]
        nb = len(params) // 2
        weights = [_lib.f32c(p) for p in params[:nb]]
        biases = [_lib.f32c(p) for p in params[nb:]]
        hidden, pts = _lib.f32c(hidden), _lib.f32c(pts)
        bases32 = _lib.f32c(bases) if bases is not None else None
        dev, n, width = hidden.device, hidden.shape[0], hidden.shape[1]
        means = torch.empty(n, 3, dtype=torch.float32, device=dev)
        flow = torch.empty((n, 4, 4) if model == "se3" else (n, 3), dtype=torch.float32, device=dev)
        need = grad_enabled and any(ctx.needs_input_grad)
        saved = None
        if need:
            size = lib.sr_flow_head_saved_bytes(code, n, width, n_basis)
            if size == 0:
                raise ValueError("fused flow head: unsupported shape: " + (fused_shape_error(model, width, n_basis) or "too many points"))
            saved = torch.empty(size // 8, dtype=torch.float64, device=dev)
        with torch.cuda.device(dev):
            _lib.check(lib.sr_flow_head_forward(code, n, width, n_basis, nb, _branch_table(weights, biases), _lib.ptr(hidden), _lib.ptr(pts),
                                                _lib.ptr(bases32), _lib.ptr(means), _lib.ptr(flow), _lib.ptr(saved), _lib.stream(dev)))
        if need:
            ctx.spec = (model, code, n_basis, nb)
            ctx.bases_dtype = bases.dtype if bases is not None else None      # float64 bases (the SIREN's) get the unrounded sum back
            ctx.save_for_backward(hidden, pts, bases32, saved, *weights)
            ctx.set_materialize_grads(False)
        return flow, means

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g_flow, g_means):
        lib = _lib.load()
        model, code, n_basis, nb = ctx.spec
        hidden, pts, bases32, saved, *weights = ctx.saved_tensors
        dev, n, width = hidden.device, hidden.shape[0], hidden.shape[1]
        need_hidden, need_pts, need_bases = ctx.needs_input_grad[3], ctx.needs_input_grad[4], bases32 is not None and ctx.needs_input_grad[5]
        need_W = any(ctx.needs_input_grad[6:])
        g_means = _lib.f32c(g_means) if g_means is not None else torch.zeros(n, 3, dtype=torch.float32, device=dev)
        g_flow = _lib.f32c(g_flow) if g_flow is not None else None        # null: the training loop's case (nothing reads `flow`)
        rows = [w.shape[0] for w in weights]
        dz_row = lib.sr_flow_head_dz_row(code, n_basis)
        dz = torch.empty(weight_grad.dz_rows(n), dz_row, dtype=torch.float32, device=dev)      # a branch's job starts at its own column
        d_hidden = torch.empty_like(hidden) if need_hidden else None
        d_pts = torch.empty(n, 3, dtype=torch.float32, device=dev) if need_pts else None
        ws = torch.empty(lib.sr_flow_head_workspace_bytes(code, n, width, n_basis) // 8, dtype=torch.float64, device=dev)
        table = (_lib.SrFlowBranch * nb)()
        for i, w in enumerate(weights):
            table[i].weight, table[i].bias, table[i].rows = w.data_ptr(), None, rows[i]
        with torch.cuda.device(dev):
            _lib.check(lib.sr_flow_head_backward(code, n, width, n_basis, nb, table, _lib.ptr(pts), _lib.ptr(bases32), _lib.ptr(saved),
                                                 _lib.ptr(g_means), _lib.ptr(g_flow), _lib.ptr(d_pts), _lib.ptr(dz), _lib.ptr(d_hidden),
                                                 _lib.ptr(ws), _lib.stream(dev)))
        d_bases = None
        if need_bases:       # one partial per workgroup of 256 consecutive points: the shape alone fixes the order of this sum
            d_bases = ws[: (n + 255) // 256 * n_basis].view(-1, n_basis).sum(0).to(ctx.bases_dtype)
        dWs, dbs = [None] * nb, [None] * nb
        if need_W:
            dWs, dbs = _branch_weight_grads(hidden, dz, dz_row, weights, n)
            dWs = [g if ctx.needs_input_grad[6 + j] else None for j, g in enumerate(dWs)]
            dbs = [g if ctx.needs_input_grad[6 + nb + j] else None for j, g in enumerate(dbs)]
        return (None, None, None, d_hidden, d_pts, d_bases, *dWs, *dbs)


def _branch_weight_grads(hidden, dz, dz_row, weights, n):
    """dW_b = dz_b^T hidden, db_b = sum dz_b of every branch in one weight_grad.run call: one job per branch, whose dz address is
    the branch's first column (a multiple of 4 floats) of the shared [N, dz_row] matrix."""
    dev, width = hidden.device, hidden.shape[1]
    fields, dz_at, at = [], [], dz.data_ptr()
    for w in weights:
        fields.append((dz_row, w.shape[0], width, width, width, 0))
        dz_at.append(at)
        at += 4 * ((w.shape[0] + 3) // 4 * 4)
    dWs = [torch.empty_like(w) for w in weights]
    dbs = [torch.empty(w.shape[0], dtype=torch.float32, device=dev) for w in weights]
    weight_grad.run(n, dev, weight_grad.job_list(tuple(fields)), dz_at, [hidden.data_ptr()] * len(weights), dWs, dbs)
    return dWs, dbs


def fused_flow_head(model: str, hidden: torch.Tensor, pts: torch.Tensor, weights: Sequence[torch.Tensor], biases: Sequence[torch.Tensor],
                    bases: Optional[torch.Tensor] = None):
    """-> (flow, means3D) of the reference's `FlowHead(flow_model=model)`: hidden [N, W], pts [N, 3], weights[i] [rows_i, W] and
    biases[i] [rows_i] in the branch order of include/splatraster.h (offset: warp; se3: w, v; se3Affine: w, v, offset; se3Scaled:
    w, v, scale, offset; affine: w (9), v; dct / dct_siren: coeff), bases [K] (float32 or float64) for the two DCT models.  `flow` is [N, 4, 4] for
    'se3' and [N, 3] otherwise.  Differentiable in everything; tensors live on a HIP device; float64 / autocast inputs are
    converted to float32 at the boundary (the results are float32)."""
    if model not in MODELS:
        raise ValueError(f"unknown flow model {model!r}: expected one of {tuple(MODELS)}")
    if not hidden.is_cuda:
        raise RuntimeError("fused_flow_head has no CPU path: tensors must be on a HIP ('cuda') device")
    dct = MODELS[model][0] == _lib.FLOW_DCT
    if hidden.dim() != 2 or pts.dim() != 2 or pts.shape[1] != 3 or pts.shape[0] != hidden.shape[0]:
        raise ValueError("hidden must be [N, W] and pts [N, 3]")
    if dct != (bases is not None) or (dct and bases.dim() != 1):
        raise ValueError("bases [K] goes with the dct models, and only with them")
    n_basis = int(bases.shape[0]) if dct else 0
    why = fused_shape_error(model, hidden.shape[1], n_basis)
    if why:
        raise ValueError("fused_flow_head: " + why)
    want = branch_rows(model, n_basis)
    if len(weights) != len(want) or len(biases) != len(want):
        raise ValueError(f"flow model {model!r} has {len(want)} branches")
    for w, b, r in zip(weights, biases, want):
        if tuple(w.shape) != (r, hidden.shape[1]) or tuple(b.shape) != (r,):
            raise ValueError(f"flow model {model!r}: branch weights must be {[(r_, hidden.shape[1]) for r_ in want]} with matching biases")
    for t in (pts, bases, *weights, *biases):
        if t is not None and t.device != hidden.device:
            raise RuntimeError("fused_flow_head has no CPU path: every tensor must be on the device of `hidden`")
    with torch.autocast("cuda", enabled=False):
        f32 = lambda t: t if t is None or t.dtype is torch.float32 else t.float()      # differentiable: gradients return in the caller's dtype
        hidden, pts = f32(hidden), f32(pts)      # `bases` keeps its dtype: the kernel reads it rounded to float32, its gradient is not rounded
        weights, biases = [f32(w) for w in weights], [f32(b) for b in biases]
        if hidden.shape[0] == 0:      # nothing to launch; keep the graph connected so that parameters still receive (zero) gradients
            zero = 0.0 * (hidden.sum() + pts.sum() + sum(w.sum() for w in weights) + sum(b.sum() for b in biases) +
                          (bases.float().sum() if bases is not None else 0.0))
            return hidden.new_zeros((0, 4, 4) if model == "se3" else (0, 3)) + zero, pts.new_zeros(0, 3) + zero
        return _FlowHeadFn.apply(model, n_basis, torch.is_grad_enabled(), hidden, pts, bases, *weights, *biases)
