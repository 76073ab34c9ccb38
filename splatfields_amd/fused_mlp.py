"""Fused MLPs of the SplatFields deform network, forward and backward (include/splatraster.h: sr_mlp_chain, sr_mlp_pack;
csrc/mlp.hip; the weight gradients through splatfields_amd/weight_grad.py).

`fused_general_mlp` evaluates one `GeneralMLP` of reference utils/time_utils.py:123-191 -- `h = act(layer_i(h))` for every
layer, `h = cat([h_in, h])` after the layers listed in `skips`, act = leaky ReLU -- for all points in one kernel
(activations in registers, exact fp32 MFMA), and is differentiable: the backward runs the activation-gradient chain
dZ_{l-1} = (W_l^T dZ_l) * act'(.) and dL/dh_in in one more kernel of the same shape, and the weight gradients
dW_l = dZ_l^T [h_in | h_{l-1}], db_l = sum dZ_l of ALL layers in one launch of a kernel that splits the points over the
chip (library GEMMs serialise this contraction: 2.7 of the 3.9 ms of a PyTorch-ROCm step of one 128 x 8 network).  It takes the
layers' *effective* weights as ordinary autograd tensors: for ResField layers (reference utils/resfields.py:378-405) the
caller composes `W + delta(frame)` first and autograd carries dW on to W and the delta factors.  `FusedGeneralMLP` is the
module-style wrapper.  No CPU path.

`precision="bf16"` (opt-in; `set_mlp_precision` / SPLATFIELDS_MLP_PRECISION set the process default, "fp32") runs the two layer
chains on the bf16 MFMA: weights and the chains' inputs are rounded to bfloat16 where they enter a matrix product, products and
sums, biases, the running state, the epilogues and everything stored stay fp32, and the weight gradients come from the fp32
kernel on those stored values (include/splatraster.h: sr_mlp_chain_bf16).  `precision="bf16x3"` (opt-in the
same way) splits every such operand into two bfloat16 values, hi = bf(v) and lo = bf(v - hi), and spends three bf16 MFMAs per
product (hi hi + hi lo + lo hi): about 16 significant bits instead of 8, everything else as for "bf16" (sr_mlp_chain_bf16x3; DESIGN.md
section 21).

`fused_grouped_heads` (opt-in; `set_heads` / SPLATFIELDS_HEADS set the process default, "separate") evaluates several such networks
that read the same points, features and time through one autograd function: the networks of one hidden width and precision in one
chain launch per direction, the input matrices, output activations, top gradients and the summed input gradient of all of them in
one launch each (include/splatraster.h: sr_mlp_chain_group, sr_mlp_group_*).
"""
from __future__ import annotations

import ctypes as C
import os
import threading
from operator import itemgetter
from typing import List, Optional, Sequence, Tuple

import torch
import torch.nn.functional as F

from . import _lib, weight_grad


PRECISIONS = ("fp32", "bf16")
SPLIT_PRECISIONS = ("bf16x3",)      # bf16 MFMAs on operands split into two bfloat16 values: accepted wherever a precision name is


def _checked_precision(name) -> str:
    if name not in PRECISIONS and name not in SPLIT_PRECISIONS:
        raise ValueError(f"unknown MLP precision {name!r}: expected one of {PRECISIONS + SPLIT_PRECISIONS}")
    return name


# process default of the fused MLP chains, read once: SPLATFIELDS_MLP_PRECISION=bf16 turns the bf16 MFMA path on for every
# network that does not name a precision itself
_MLP_PRECISION = _checked_precision(os.environ.get("SPLATFIELDS_MLP_PRECISION") or "fp32")


def set_mlp_precision(name: str) -> str:
    """Process default of the fused MLP chains: "fp32" (exact fp32 MFMA), "bf16" (bf16 operands, fp32 accumulation) or "bf16x3"
    (operands split into two bf16 values, three bf16 MFMAs per product).  Returns the previous setting."""
    global _MLP_PRECISION
    prev, _MLP_PRECISION = _MLP_PRECISION, _checked_precision(name)
    return prev


def mlp_precision() -> str:
    return _MLP_PRECISION


def resolve_precision(precision: Optional[str]) -> str:
    """`None` -> the process default, at call time."""
    return _MLP_PRECISION if precision is None else _checked_precision(precision)


def pack_layer_weight(W: torch.Tensor, n_mem: int, mem_pad: int, reg_width: int, out_tiles: int) -> torch.Tensor:
    """PyTorch statement of the packing (the device packer sr_mlp_pack is tested against it).  W [M, n_mem + n_reg] (the
    reference's column order: network input first, hidden state after it) -> the packed K order of csrc/mlp.hip:
    float ((((c MT + mt) 2 + tl) 64 + 16 k + m) 4 + i) = W'[16 mt + m][16 (2 c + tl) + 4 k + i], where W' is W with the input
    block zero-padded to `mem_pad` columns, the hidden block to `reg_width`, and the rows to 16 `out_tiles`."""
    M, K = W.shape
    n_reg = K - n_mem
    Wp = W.new_zeros(16 * out_tiles, mem_pad + reg_width)
    if n_mem:
        Wp[:M, :n_mem] = W[:, :n_mem]
    if n_reg:
        Wp[:M, mem_pad:mem_pad + n_reg] = W[:, n_mem:]
    kt = (mem_pad + reg_width) // 16
    v = Wp.view(out_tiles, 16, kt // 2, 2, 4, 4)            # (mt, m, c, tl, k, i)
    return v.permute(2, 0, 3, 4, 1, 5).contiguous().reshape(-1)   # (c, mt, tl, k, m, i)


def pack_layer_weight_bf16(W: torch.Tensor, n_mem: int, mem_pad: int, reg_width: int, out_tiles: int) -> torch.Tensor:
    """PyTorch statement of the bf16 packing (the device packer sr_mlp_pack_bf16 is tested against it): the same padded matrix W'
    as `pack_layer_weight`, rounded to bfloat16, in the K order of the 16x16x32 MFMA (csrc/mlp.hip):
    bf16 (((c MT + mt) 64 + 16 k + m) 8 + j) = W'[16 mt + m][32 c + 16 (j >> 2) + 4 k + (j & 3)]."""
    M, K = W.shape
    n_reg = K - n_mem
    Wp = W.new_zeros(16 * out_tiles, mem_pad + reg_width)
    if n_mem:
        Wp[:M, :n_mem] = W[:, :n_mem]
    if n_reg:
        Wp[:M, mem_pad:mem_pad + n_reg] = W[:, n_mem:]
    v = Wp.to(torch.bfloat16).view(out_tiles, 16, (mem_pad + reg_width) // 32, 2, 4, 4)     # (mt, m, c, j >> 2, k, j & 3)
    return v.permute(2, 0, 4, 1, 3, 5).contiguous().reshape(-1)                          # (c, mt, k, m, j >> 2, j & 3)


def pack_layer_weight_bf16x3(W: torch.Tensor, n_mem: int, mem_pad: int, reg_width: int, out_tiles: int) -> torch.Tensor:
    """PyTorch statement of the bf16x3 packing (the device packer sr_mlp_pack_bf16x3 is tested against it): the same padded matrix
    W' as `pack_layer_weight`, split into hi = bf(W') and lo = bf(W' - hi), per 32-column chunk the hi block and then the lo block,
    each in the K order of `pack_layer_weight_bf16` (csrc/mlp_bf16x3.h):
    bf16 ((((2 c + part) MT + mt) 64 + 16 k + m) 8 + j) = part(W'[16 mt + m][32 c + 16 (j >> 2) + 4 k + (j & 3)]), part 0 = hi, 1 = lo."""
    M, K = W.shape
    n_reg = K - n_mem
    Wp = W.new_zeros(16 * out_tiles, mem_pad + reg_width, dtype=torch.float32)
    if n_mem:
        Wp[:M, :n_mem] = W[:, :n_mem]
    if n_reg:
        Wp[:M, mem_pad:mem_pad + n_reg] = W[:, n_mem:]
    hi = Wp.to(torch.bfloat16)
    lo = (Wp - hi.to(torch.float32)).to(torch.bfloat16)
    v = torch.stack([hi, lo]).view(2, out_tiles, 16, (mem_pad + reg_width) // 32, 2, 4, 4)     # (part, mt, m, c, j >> 2, k, j & 3)
    return v.permute(3, 0, 1, 5, 2, 4, 6).contiguous().reshape(-1)                          # (c, part, mt, k, m, j >> 2, j & 3)


def _f32c(t: torch.Tensor) -> torch.Tensor:
    """the tensor as contiguous float32 -- itself when it already is (the usual case: one attribute
    test instead of three tensor methods; ~50 of these per network and step are host time the GPU waits for).
    Not _lib.f32c, which detaches first: one tensor method more on that usual case."""
    if t.dtype is torch.float32 and t.is_contiguous():
        return t          # only its data pointer is used; autograd.Function inputs may be saved as they are
    return t.detach().to(torch.float32).contiguous()


class _Shape:
    """Static description of one GeneralMLP: which layers read the network input, tile counts, validity."""

    def __init__(self, weights: Sequence[torch.Tensor], d_in: int, skips: Sequence[int]):
        self.n_layers = len(weights)
        if self.n_layers < 2:
            raise ValueError("a fused MLP has at least two layers")
        self.d_in = int(d_in)
        self.hidden = int(weights[0].shape[0])
        if self.hidden not in (64, 128):
            raise ValueError("fused MLPs support hidden widths 64 and 128")
        self.ht = self.hidden // 16
        self.skips = {int(s) for s in skips if 0 <= int(s) < self.n_layers - 1}
        self.out_features = int(weights[-1].shape[0])
        if self.out_features > self.hidden:
            raise ValueError("the output may not be wider than the hidden layers")
        self.out_tiles_last = (self.out_features + 15) // 16
        self.out_pad = (self.out_features + 31) // 32 * 32      # the top gradient is a memory input: two tiles per chunk
        self.mem_pad = (self.d_in + 31) // 32 * 32
        self.reads_input = [j == 0 or (j - 1) in self.skips for j in range(self.n_layers)]
        for j, W in enumerate(weights):
            want = self.d_in if j == 0 else self.hidden + (self.d_in if self.reads_input[j] else 0)
            rows = self.hidden if j < self.n_layers - 1 else self.out_features
            if tuple(W.shape) != (rows, want):
                raise ValueError(f"layer {j}: expected weight [{rows}, {want}], got {tuple(W.shape)}")
        # input-gradient ops write <= ht tiles each
        self.input_groups = [(g, min(self.ht, self.mem_pad // 16 - g)) for g in range(0, self.mem_pad // 16, self.ht)
                             if self.d_in - 16 * g > 0]
        self.layer_dims = [tuple(W.shape) for W in weights]
        self.plans: dict = {}     # descriptor arrays of the forward / backward / weight-gradient launches, built on first use


_PACK_PTRS, _OP_PTRS = ("w", "bias_src"), ("src", "mask", "store", "sign_store", "mask_bits")


class _Plan:
    """One pack launch + one chain launch of a fixed shape, with the ctypes descriptor arrays built ONCE: everything static
    (tile counts, strides, epilogues) is filled in when the plan is made; pointer fields are symbolic -- ("W", j, byte offset)
    = weights[j].data_ptr() + offset -- and are patched per call (building ~40 descriptor structs per network and step in
    Python cost ~0.6 ms of host time per network; patching ~60 pointers costs a few tens of microseconds)."""

    def __init__(self, precision: str = "fp32"):
        self.mode = _checked_precision(precision)                # which packer / chain kernel runs
        self.bf16 = self.mode == "bf16"                          # packed matrices are plain bfloat16 (biases stay fp32)
        self.wsize = 2 if self.bf16 else 4                       # bytes per packed weight; "bf16x3": two bfloat16, hi and lo
        self.jobs: List[dict] = []
        self.ops: List[dict] = []
        self.sizes: List[Tuple[int, int]] = []
        self._arrays = None
        self._lock = threading.Lock()

    def add(self, job: dict, op: dict, with_bias: bool):
        floats = 16 * job["out_tiles"] * (job["mem_pad"] + job["reg_width"])
        self.jobs.append(job)
        self.sizes.append((floats, 16 * job["out_tiles"] if with_bias else 0))
        self.ops.append(op)

    def _fill(self, jobs, ops, start: int, at: int):
        """writes this plan's static fields into jobs[start:] / ops[start:] (its own arrays, or a group's: _GroupPlan) with its
        packed matrices from byte `at` of the buffer on; -> (binds (struct, field, symbol, index, byte offset), next free byte)"""
        binds = []            # `at`: bytes, every piece a multiple of 16
        wsize = self.wsize
        for j, (job, op, (wf, bf)) in enumerate(zip(self.jobs, self.ops, self.sizes)):
            J, O = jobs[start + j], ops[start + j]
            J.ld, J.transposed, J.row0, J.n_rows = job["ld"], job["transposed"], job["row0"], job["n_rows"]
            J.n_mem, J.mem_pad, J.mem_col0 = job["n_mem"], job["mem_pad"], 0
            J.n_reg, J.reg_width, J.reg_col0 = job["n_reg"], job["reg_width"], job["reg_col0"]
            J.out_tiles, J.n_bias = job["out_tiles"], job.get("n_bias", 0)
            O.out_tiles, O.mem_tiles, O.reg_tiles = job["out_tiles"], job["mem_pad"] // 16, job["reg_width"] // 16
            O.src_row, O.epilogue, O.mask_row = op.get("src_row", 0), op["epilogue"], op.get("mask_row", 0)
            O.store_row, O.store_channels = op.get("store_row", 0), op.get("store_channels", 0)
            O.store_accumulate, O.keep_state = op.get("store_accumulate", 0), op.get("keep_state", 0)
            binds.append((J, "dst", "buf", 0, at)); binds.append((O, "w_packed", "buf", 0, at))
            if bf:
                binds.append((J, "bias_dst", "buf", 0, at + wsize * wf)); binds.append((O, "bias", "buf", 0, at + wsize * wf))
            at += wsize * wf + 4 * bf
            for f, key in (("w", "w"), ("bias_src", "bias")):
                if job.get(key) is not None:
                    binds.append((J, f) + tuple(job[key]))
            for f in _OP_PTRS:
                if op.get(f) is not None:
                    binds.append((O, f) + tuple(op[f]))
        return binds, at

    def _freeze(self):
        if len(self.jobs) > _lib.MLP_MAX_PACK_JOBS or len(self.ops) > _lib.MLP_MAX_OPS:
            raise ValueError("network too deep for one fused chain")
        n = len(self.jobs)
        jobs = (_lib.SrMlpPackJob * n)()
        ops = (_lib.SrMlpOp * n)()
        binds, at = self._fill(jobs, ops, 0, 0)
        self._arrays = (jobs, ops, binds, at)

    def run(self, lib, ptrs: dict, device, n_points: int, ht: int, slope: float, stream) -> torch.Tensor:
        with self._lock:      # the descriptor arrays are shared by every call with this shape
            if self._arrays is None:
                self._freeze()
            jobs, ops, binds, total = self._arrays
            buf = torch.empty(total // 4, dtype=torch.float32, device=device)
            ptrs = dict(ptrs, buf=(buf.data_ptr(),))
            for obj, field, sym, idx, off in binds:
                setattr(obj, field, ptrs[sym][idx] + off)
            pack, chain = _entries(lib, self.mode, group=False)
            _lib.check(pack(len(jobs), jobs, stream))
            _lib.check(chain(n_points, ht, len(ops), ops, slope, stream))
        return buf      # alive until the caller drops it; the stream orders its reuse


def _entries(lib, mode: str, group: bool):
    """(pack entry, chain entry) of a chain precision; a name without kernels is an error, never another precision's kernels"""
    suffix = {"fp32": "", "bf16": "_bf16", "bf16x3": "_bf16x3"}[mode]
    return getattr(lib, "sr_mlp_pack" + suffix), getattr(lib, ("sr_mlp_chain_group" if group else "sr_mlp_chain") + suffix)


def _forward_plan(shape: _Shape, save: bool, precision: str = "fp32") -> _Plan:
    key = ("fwd", save, precision)
    if key not in shape.plans:
        H, L = shape.hidden, shape.n_layers
        b = _Plan(precision)
        for j in range(L):
            last = j == L - 1
            rows, cols = shape.layer_dims[j]
            n_mem = shape.d_in if shape.reads_input[j] else 0
            job = dict(w=("W", j, 0), ld=cols, transposed=0, row0=0, n_rows=rows, n_mem=n_mem,
                       mem_pad=shape.mem_pad if n_mem else 0, n_reg=cols - n_mem, reg_width=0 if j == 0 else H, reg_col0=n_mem,
                       out_tiles=shape.out_tiles_last if last else shape.ht, bias=("B", j, 0), n_bias=rows)
            op = dict(epilogue=_lib.MLP_LEAKY, src=("x0", 0, 0) if n_mem else None, src_row=shape.mem_pad)
            if last:
                op.update(store=("y", 0, 0), store_row=shape.out_features, store_channels=shape.out_features)
            elif save:       # the activation itself (an operand of dW of the layer above) and its signs (leaky' for the backward chain)
                op.update(store=("acts", j, 0), store_row=H, store_channels=H, sign_store=("signs", j, 0))
            b.add(job, op, with_bias=True)
        shape.plans[key] = b
    return shape.plans[key]


def _forward(shape: _Shape, x0: torch.Tensor, weights, biases, slope: float, save: bool, precision: str = "fp32"):
    """x0 [N, mem_pad] -> (y [N, out], acts [L-1, N, hidden] or None, signs [L-1, N, 4] int32 or None: one bit per activation,
    set where it is > 0, in the layout of SrMlpOp.sign_store)."""
    lib = _lib.load()
    dev, n, H, L = x0.device, x0.shape[0], shape.hidden, shape.n_layers
    y = torch.empty(n, shape.out_features, dtype=torch.float32, device=dev)
    acts = torch.empty(L - 1, n, H, dtype=torch.float32, device=dev) if save else None
    signs = torch.empty(L - 1, n, 4, dtype=torch.int32, device=dev) if save else None
    ptrs = {"W": [w.data_ptr() for w in weights], "B": [b_.data_ptr() for b_ in biases], "x0": (x0.data_ptr(),), "y": (y.data_ptr(),),
            "acts": [acts.data_ptr() + 4 * j * n * H for j in range(L - 1)] if save else (),
            "signs": [signs.data_ptr() + 16 * j * n for j in range(L - 1)] if save else ()}
    with torch.cuda.device(dev):
        _forward_plan(shape, save, precision).run(lib, ptrs, dev, n, shape.ht, slope, _lib.stream(dev))
    return y, acts, signs


def _backward_plan(shape: _Shape, need_input: bool, bits: bool, precision: str = "fp32") -> _Plan:
    key = ("bwd", need_input, bits, precision)
    if key not in shape.plans:
        H, L = shape.hidden, shape.n_layers
        b = _Plan(precision)
        wrote_input = False        # dL/dx0 is not cleared beforehand: the first layer that feeds it (the topmost) stores, incl. zero padding
        for j in range(L - 1, -1, -1):
            ld = shape.layer_dims[j][1]
            top = j == L - 1
            n_mem_w = shape.d_in if shape.reads_input[j] else 0        # columns of W_j that multiply the network input
            # this layer's dZ is the op input: memory (G) for the top layer, the register state below it
            cols = dict(n_mem=shape.out_features, mem_pad=shape.out_pad, n_reg=0, reg_width=0, reg_col0=0) if top else \
                dict(n_mem=0, mem_pad=0, n_reg=H, reg_width=H, reg_col0=0)
            src = dict(src=("G", 0, 0), src_row=shape.out_pad) if top else {}
            if need_input and n_mem_w:
                for g0, cnt in shape.input_groups:                      # dL/dx0 (+)= W_j[:, input block]^T dZ_j, <= ht tiles at a time
                    rows = min(16 * cnt, shape.d_in - 16 * g0)
                    job = dict(w=("W", j, 0), ld=ld, transposed=1, row0=16 * g0, n_rows=rows, out_tiles=cnt, **cols)
                    # packed rows beyond `rows` are zero: storing all 16 cnt channels also writes the padding columns' zeros
                    op = dict(epilogue=_lib.MLP_NONE, keep_state=1, store=("dx0", 0, 4 * 16 * g0), store_row=shape.mem_pad,
                              store_channels=rows if wrote_input else 16 * cnt, store_accumulate=1 if wrote_input else 0, **src)
                    b.add(job, op, with_bias=False)
                wrote_input = True
            if j > 0:                                                   # dZ_{j-1} = (W_j[:, hidden block]^T dZ_j) * act'(h_{j-1})
                job = dict(w=("W", j, 0), ld=ld, transposed=1, row0=n_mem_w, n_rows=H, out_tiles=shape.ht, **cols)
                mask = dict(mask_bits=("signs", j - 1, 0)) if bits else dict(mask=("acts", j - 1, 0), mask_row=H)
                op = dict(epilogue=_lib.MLP_MASK, store=("dz", j - 1, 0), store_row=H, store_channels=H, **mask, **src)
                b.add(job, op, with_bias=False)
        shape.plans[key] = b
    return shape.plans[key]


def _top_gradient(lib, shape: _Shape, y, dY, slope: float, G):
    """G[:, :out] = dY * leaky'(y), zero padding behind: one launch (sr_mlp_top_gradient)"""
    dev = y.device
    with torch.cuda.device(dev):
        _lib.check(lib.sr_mlp_top_gradient(y.shape[0], shape.out_features, shape.out_pad, _lib.ptr(y), _lib.ptr(dY),
                                           slope, _lib.ptr(G), _lib.stream(dev)))


def _backward(shape: _Shape, x0, acts, y, dY, weights, slope: float, need_input: bool, signs=None, precision: str = "fp32"):
    """-> (dL/dx0 [N, mem_pad] or None, G [N, out_pad] = dZ of the last layer (zero-padded), dz [L-1, N, hidden] = dZ of the others).
    leaky'(.) of the hidden layers is read off `signs` (16 bytes per point and layer) when given, else off `acts` (4 * hidden)."""
    lib = _lib.load()
    dev, n, H, L = x0.device, x0.shape[0], shape.hidden, shape.n_layers
    G = torch.empty(n, shape.out_pad, dtype=torch.float32, device=dev)
    dz = torch.empty(L - 1, n, H, dtype=torch.float32, device=dev)
    dx0 = torch.empty(n, shape.mem_pad, dtype=torch.float32, device=dev) if need_input else None   # the chain's first input op stores
    _top_gradient(lib, shape, y, dY, slope, G)
    ptrs = {"W": [w.data_ptr() for w in weights], "G": (G.data_ptr(),), "dx0": (dx0.data_ptr() if need_input else 0,),
            "acts": [acts.data_ptr() + 4 * j * n * H for j in range(L - 1)], "dz": [dz.data_ptr() + 4 * j * n * H for j in range(L - 1)],
            "signs": [signs.data_ptr() + 16 * j * n for j in range(L - 1)] if signs is not None else ()}
    with torch.cuda.device(dev):
        _backward_plan(shape, need_input, signs is not None, precision).run(lib, ptrs, dev, n, shape.ht, slope, _lib.stream(dev))
    return dx0, G, dz


def _grad_jobs(shape: _Shape):
    """static part of the weight-gradient job list: (its JobList, then per job as itemgetters: dz and x out of the addresses
    [G, x0, dz_0.., acts_0..], dw out of the layers' dW, db out of [the layers' db.., None]: the first job of a layer carries it)"""
    if "grad" not in shape.plans:
        H, L, fields, picks = shape.hidden, shape.n_layers, [], []
        for j in range(L):
            dz_at, dz_row, m = (0, shape.out_pad, shape.out_features) if j == L - 1 else (2 + j, H, H)
            col0 = 0
            segments = []
            if shape.reads_input[j]:
                segments.append((1, shape.mem_pad, shape.d_in))
            if j > 0:
                segments.append((L + j, H, H))
            for x_at, x_row, k in segments:
                fields.append((dz_row, m, x_row, k, shape.layer_dims[j][1], col0))
                picks.append((dz_at, x_at, j, j if col0 == 0 else L))
                col0 += k
        jobs = weight_grad.JobList(fields)      # raises for a network too deep for one launch
        shape.plans["grad"] = (jobs, *[itemgetter(*column) for column in zip(*picks)])
    return shape.plans["grad"]


def _weight_grads(shape: _Shape, x0, acts, G, dz, weights):
    """dW_j = dZ_j^T [h_in | h_{j-1}], db_j = sum over points of dZ_j, all layers in one launch: one job per column block of a dW
    (the input segment, the hidden segment), the bias on the first (weight_grad.run; a reference-sized network reaches its chunk
    limit at ~2.4 M points)."""
    dev, n, H, L = x0.device, x0.shape[0], shape.hidden, shape.n_layers
    jobs, pick_dz, pick_x, pick_dw, pick_db = _grad_jobs(shape)
    dWs = [torch.empty_like(W) for W in weights]
    dbs = [torch.empty(W.shape[0], dtype=torch.float32, device=dev) for W in weights]
    dz0, acts0 = dz.data_ptr(), acts.data_ptr()
    at = [G.data_ptr(), x0.data_ptr(), *[dz0 + 4 * j * n * H for j in range(L - 1)], *[acts0 + 4 * j * n * H for j in range(L - 1)]]
    weight_grad.run(n, dev, jobs, pick_dz(at), pick_x(at), pick_dw(dWs), pick_db(dbs + [None]))
    return dWs, dbs


class _FusedMLPFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, h_in, shape: _Shape, slope: float, grad_enabled: bool, precision: str, *params):
        L = shape.n_layers
        weights = [_f32c(p) for p in params[:L]]
        biases = [_f32c(p) for p in params[L:]]
        x0 = F.pad(h_in.detach().to(torch.float32), (0, shape.mem_pad - shape.d_in)).contiguous()
        # needs_input_grad reflects requires_grad of the inputs, not the grad mode (inside forward() grad mode is always off):
        # under torch.no_grad() nothing will run backward, so the [L-1, N, hidden] activation stack is neither allocated nor written
        need = grad_enabled and any(ctx.needs_input_grad)
        y, acts, signs = _forward(shape, x0, weights, biases, slope, save=need, precision=precision)
        if need:
            ctx.shape, ctx.slope, ctx.precision = shape, slope, precision      # the backward runs in the precision of its forward
            ctx.save_for_backward(x0, acts, signs, y, *weights)
        return y

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, dY):
        shape, slope = ctx.shape, ctx.slope
        x0, acts, signs, y, *weights = ctx.saved_tensors
        L, d_in = shape.n_layers, shape.d_in
        need_input = ctx.needs_input_grad[0]
        dx0, G, dz = _backward(shape, x0, acts, y, dY.to(torch.float32).contiguous(), weights, slope, need_input, signs, ctx.precision)
        dWs, dbs = [None] * L, [None] * L
        if any(ctx.needs_input_grad[5:]):
            dWs, dbs = _weight_grads(shape, x0, acts, G, dz, weights)
            dWs = [g if ctx.needs_input_grad[5 + j] else None for j, g in enumerate(dWs)]
            dbs = [g if ctx.needs_input_grad[5 + L + j] else None for j, g in enumerate(dbs)]
        return (dx0[:, :d_in] if need_input else None, None, None, None, None, *dWs, *dbs)


class _FusedMLPPointsFn(torch.autograd.Function):
    """The same network fed from the points themselves: the input matrix [x | sin / cos encodings | features | padding] is
    built by one kernel (sr_mlp_input_forward) straight into the padded layout the chain kernel reads, and its backward
    (sr_mlp_input_backward) turns dL/dx0 into dL/dxyz and dL/dfeatures -- instead of ~60 small PyTorch kernels per network
    and step for the encoding, the concatenations, the padding and their backward."""

    @staticmethod
    def forward(ctx, xyz, feat, time, shape: _Shape, slope: float, multires: int, time_multires: int, grad_enabled: bool, precision: str,
                *params):
        lib = _lib.load()
        L = shape.n_layers
        weights = [_f32c(p) for p in params[:L]]
        biases = [_f32c(p) for p in params[L:]]
        dev, n = xyz.device, xyz.shape[0]
        x32 = _f32c(xyz)
        f32 = _f32c(feat) if feat is not None else None
        t32 = time.detach().to(torch.float32).reshape(-1).contiguous() if time is not None else None
        n_feat = 0 if f32 is None else f32.shape[1]
        x0 = torch.empty(n, shape.mem_pad, dtype=torch.float32, device=dev)
        with torch.cuda.device(dev):
            _lib.check(lib.sr_mlp_input_forward(n, multires, n_feat, time_multires, shape.mem_pad, _lib.ptr(x32), _lib.ptr(f32),
                                                _lib.ptr(t32), _lib.ptr(x0), _lib.stream(dev)))
        need = grad_enabled and any(ctx.needs_input_grad)
        y, acts, signs = _forward(shape, x0, weights, biases, slope, save=need, precision=precision)
        if need:
            ctx.shape, ctx.slope, ctx.multires, ctx.n_feat, ctx.precision = shape, slope, multires, n_feat, precision
            ctx.save_for_backward(x32, x0, acts, signs, y, *weights)
        return y

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, dY):
        lib = _lib.load()
        shape, slope = ctx.shape, ctx.slope
        x32, x0, acts, signs, y, *weights = ctx.saved_tensors
        L, dev, n = shape.n_layers, x0.device, x0.shape[0]
        need_xyz, need_feat = ctx.needs_input_grad[0], ctx.needs_input_grad[1] and ctx.n_feat > 0
        dx0, G, dz = _backward(shape, x0, acts, y, dY.to(torch.float32).contiguous(), weights, slope, need_xyz or need_feat, signs,
                               ctx.precision)
        d_xyz = torch.empty(n, 3, dtype=torch.float32, device=dev) if need_xyz else None
        d_feat = torch.empty(n, ctx.n_feat, dtype=torch.float32, device=dev) if need_feat else None
        if need_xyz or need_feat:
            with torch.cuda.device(dev):
                _lib.check(lib.sr_mlp_input_backward(n, ctx.multires, ctx.n_feat, shape.mem_pad, _lib.ptr(x32), _lib.ptr(dx0),
                                                     _lib.ptr(d_xyz), _lib.ptr(d_feat), _lib.stream(dev)))
        dWs, dbs = [None] * L, [None] * L
        if any(ctx.needs_input_grad[9:]):
            dWs, dbs = _weight_grads(shape, x0, acts, G, dz, weights)
            dWs = [g if ctx.needs_input_grad[9 + j] else None for j, g in enumerate(dWs)]
            dbs = [g if ctx.needs_input_grad[9 + L + j] else None for j, g in enumerate(dbs)]
        return (d_xyz, d_feat, None, None, None, None, None, None, None, *dWs, *dbs)


def fused_general_mlp_points(xyz: torch.Tensor, feat: Optional[torch.Tensor], multires: int, weights: Sequence[torch.Tensor],
                             biases: Sequence[torch.Tensor], skips: Sequence[int] = (), negative_slope: float = 0.01,
                             _shape: Optional[_Shape] = None, time: Optional[torch.Tensor] = None, time_multires: int = 0,
                             precision: Optional[str] = None) -> torch.Tensor:
    """`fused_general_mlp(cat([positional_encoding(xyz, multires), feat, positional_encoding(time, time_multires)]), ...)` with the
    input matrix built on the device in one kernel: xyz [N, 3], feat [N, F] or None, time [N] / [N, 1] or None (one time per point,
    no gradient), float32 on a HIP device.  `precision`: "fp32", "bf16", "bf16x3" or None (the process default, set_mlp_precision)."""
    _lib.load()
    precision = resolve_precision(precision)
    if not xyz.is_cuda:
        raise RuntimeError("fused_general_mlp_points has no CPU path: tensors must be on a HIP ('cuda') device")
    n_feat = 0 if feat is None else feat.shape[1]
    time_multires = int(max(time_multires, 0))
    n_time = 0 if time is None else 1 + 2 * time_multires
    d_in = 3 * (1 + 2 * max(multires, 0)) + n_feat + n_time
    shape = _shape or _Shape(weights, d_in, skips)
    if xyz.dim() != 2 or xyz.shape[1] != 3 or shape.d_in != d_in or (feat is not None and (feat.dim() != 2 or feat.shape[0] != xyz.shape[0])):
        raise ValueError(f"xyz must be [N, 3] and feat [N, {shape.d_in - 3 * (1 + 2 * max(multires, 0)) - n_time}]")
    if xyz.dtype != torch.float32 or (feat is not None and (feat.dtype != torch.float32 or feat.device != xyz.device)):
        raise ValueError("xyz and feat must be float32 tensors on the same device")
    if time is not None and (time.numel() != xyz.shape[0] or time.dtype != torch.float32 or time.device != xyz.device or time.requires_grad):
        raise ValueError("time must hold one float32 value per point on the same device and take no gradient")
    if not (0.0 <= negative_slope < 1.0) or len(biases) != shape.n_layers or len(weights) != shape.n_layers:
        raise ValueError("negative_slope must be in [0, 1) and there must be one weight and one bias per layer")
    if xyz.shape[0] == 0:
        return xyz.new_zeros(0, shape.out_features) + 0.0 * (xyz.sum() + sum(w.sum() for w in weights) + sum(b.sum() for b in biases))
    return _FusedMLPPointsFn.apply(xyz, feat, time, shape, float(negative_slope), int(max(multires, 0)), time_multires,
                                   torch.is_grad_enabled(), precision, *weights, *biases)


def fused_general_mlp(h_in: torch.Tensor, weights: Sequence[torch.Tensor], biases: Sequence[torch.Tensor], skips: Sequence[int] = (),
                      negative_slope: float = 0.01, _shape: Optional[_Shape] = None, precision: Optional[str] = None) -> torch.Tensor:
    """h_in [N, d_in] (positional encoding ++ features, as the reference builds it) -> [N, out_features]; differentiable with
    respect to h_in, the weights and the biases.  weights[j]: [out_j, in_j] on the device, biases[j]: [out_j]; in_0 = d_in,
    in_j = hidden (+ d_in when j - 1 is in `skips`); hidden width 64 or 128.  `precision`: "fp32" (exact fp32 MFMA), "bf16" (bf16
    matrix operands, fp32 accumulation and fp32 everything else), "bf16x3" (the same with every operand split into two bf16 values,
    three MFMAs per product) or None: the process default (set_mlp_precision)."""
    _lib.load()
    precision = resolve_precision(precision)
    if not h_in.is_cuda:
        raise RuntimeError("fused_general_mlp has no CPU path: tensors must be on a HIP ('cuda') device")
    shape = _shape or _Shape(weights, h_in.shape[1] if h_in.dim() == 2 else -1, skips)
    if h_in.dim() != 2 or h_in.shape[1] != shape.d_in:
        raise ValueError(f"h_in must be [N, {shape.d_in}]")
    if not (0.0 <= negative_slope < 1.0):
        raise ValueError("negative_slope must be in [0, 1)")
    if len(biases) != shape.n_layers:
        raise ValueError("one bias per layer")
    for j, (W, b) in enumerate(zip(weights, biases)):
        if tuple(b.shape) != (W.shape[0],):
            raise ValueError(f"layer {j}: bias must be [{W.shape[0]}]")
        for t in (W, b):
            if t.device != h_in.device or t.dtype != torch.float32:
                raise ValueError(f"layer {j}: weights and biases must be float32 tensors on {h_in.device}")
    if h_in.dtype != torch.float32:
        raise ValueError("h_in must be float32 (the reference network runs in fp32)")
    if h_in.shape[0] == 0:      # nothing to launch; keep the graph connected so that parameters still receive (zero) gradients
        return h_in.new_zeros(0, shape.out_features) + 0.0 * (h_in.sum() + sum(w.sum() for w in weights) + sum(b.sum() for b in biases))
    return _FusedMLPFn.apply(h_in, shape, float(negative_slope), torch.is_grad_enabled(), precision, *weights, *biases)


class _PointLinearFn(torch.autograd.Function):
    """y = x W^T + b for a tall matrix of per-point rows ([N, in], N ~ 10^5, in and out a few dozen): the products with the
    weight are library GEMMs, but dL/dW = dY^T x and dL/db = column sums of dY contract over the POINTS -- the shape library
    GEMMs and reductions serialise (0.29 ms per 48 x 48 x 100k product and 0.14 ms per bias on MI355X; the tri-plane refine MLP
    and the flow head were 1.4 ms of an 8.5 ms network step) -- and go through the slab kernel of the fused MLPs
    (weight_grad.run with one job, dY padded to a multiple of 4 columns: deterministic, ~0.03 ms)."""

    @staticmethod
    def forward(ctx, x, W, b):
        ctx.save_for_backward(x, W)
        ctx.has_bias = b is not None
        return torch.addmm(b, x, W.t()) if b is not None else x @ W.t()

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, dY):
        x, W = ctx.saved_tensors
        dev, n, m, k = x.device, x.shape[0], W.shape[0], W.shape[1]
        need_x, need_W = ctx.needs_input_grad[0], ctx.needs_input_grad[1]
        need_b = ctx.has_bias and ctx.needs_input_grad[2]
        dY = dY.contiguous()
        dX = dY @ W if need_x else None
        dW = db = None
        if need_W or need_b:
            m_pad = (m + 3) // 4 * 4
            dz = dY if m_pad == m else F.pad(dY, (0, m_pad - m))
            dW = torch.empty_like(W)
            db = torch.empty(m, dtype=torch.float32, device=dev)
            weight_grad.run(n, dev, weight_grad.job_list(((m_pad, m, k, k, k, 0),)), [dz.data_ptr()], [x.data_ptr()], [dW], [db])
        return dX, (dW if need_W else None), (db if need_b else None)


def point_linear(x: torch.Tensor, weight: torch.Tensor, bias: Optional[torch.Tensor] = None) -> torch.Tensor:
    """`F.linear(x, weight, bias)` for per-point rows x [N, in]; on a HIP device (float32, in a multiple of 4) the weight and
    bias gradients come from the fused MLPs' slab kernel instead of a library GEMM over N (see _PointLinearFn)."""
    ok = x.is_cuda and x.dim() == 2 and x.dtype == torch.float32 and weight.dtype == torch.float32 and x.shape[1] % 4 == 0 and \
        x.shape[0] > 0 and weight.device == x.device and (bias is None or (bias.dtype == torch.float32 and bias.device == x.device)) and \
        weight.shape[0] <= 64 * 255 and weight.shape[1] <= 64 * 255
    if not ok or not (torch.is_grad_enabled() and (weight.requires_grad or (bias is not None and bias.requires_grad))):
        return F.linear(x, weight, bias)
    return _PointLinearFn.apply(x.contiguous(), weight.contiguous(), bias)


class PointLinear(torch.nn.Linear):
    """`nn.Linear` (same parameters, initialisation and state-dict keys) applied to per-point rows through `point_linear`."""

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        return point_linear(x, self.weight, self.bias)


class FusedGeneralMLP:
    """Module-style wrapper: holds the weight / bias tensors (leaf parameters or per-step composed ResField weights may be
    swapped in through `weights` / `biases`) and the static shape."""

    def __init__(self, weights: Sequence[torch.Tensor], biases: Sequence[torch.Tensor], d_in: int, skips: Sequence[int] = (),
                 negative_slope: float = 0.01, precision: Optional[str] = None):
        self.precision = None if precision is None else _checked_precision(precision)    # None: the process default at call time
        self.weights, self.biases = list(weights), list(biases)
        self.slope = float(negative_slope)
        self.shape = _Shape(self.weights, d_in, skips)
        self.d_in, self.hidden, self.out_features = self.shape.d_in, self.shape.hidden, self.shape.out_features

    def __call__(self, h_in: torch.Tensor) -> torch.Tensor:
        return fused_general_mlp(h_in, self.weights, self.biases, negative_slope=self.slope, _shape=self.shape, precision=self.precision)


# ---- the head networks of a step as groups (opt-in: SplatFields(heads="grouped"), set_heads, SPLATFIELDS_HEADS) -----------------
# Several GeneralMLPs that read the same (xyz, features, time) run through ONE autograd function: one input kernel, one output
# kernel, one top-gradient kernel and one input-backward kernel for all of them, and per group of nets of one hidden width and
# precision one pack launch and one chain launch per direction (include/splatraster.h: sr_mlp_chain_group, sr_mlp_group_*; DESIGN.md
# section 20).  Weight gradients stay one _weight_grads call per net.

HEADS = ("separate", "grouped")
OUT_ACTIVATIONS = {"none": _lib.MLP_OUT_NONE, "sigmoid": _lib.MLP_OUT_SIGMOID, "normalize": _lib.MLP_OUT_NORMALIZE}


def _checked_heads(name) -> str:
    if name not in HEADS:
        raise ValueError(f"unknown heads mode {name!r}: expected one of {HEADS}")
    return name


# process default, read once: SPLATFIELDS_HEADS=grouped groups the heads of every SplatFields that does not name a mode itself
_HEADS = _checked_heads(os.environ.get("SPLATFIELDS_HEADS") or "separate")


def set_heads(name: str) -> str:
    """Process default of how a SplatFields step runs its head networks: "separate" (one chain of launches per network) or
    "grouped" (the networks of one width in one launch per phase).  Returns the previous setting."""
    global _HEADS
    prev, _HEADS = _HEADS, _checked_heads(name)
    return prev


def heads() -> str:
    return _HEADS


def resolve_heads(name: Optional[str]) -> str:
    """`None` -> the process default, at call time."""
    return _HEADS if name is None else _checked_heads(name)


class HeadSpec:
    """One network of a grouped step: its static shape, the frequencies of its positional encoding, its output activation
    (a key of OUT_ACTIVATIONS) and the slope of its leaky ReLU."""

    def __init__(self, name: str, shape: _Shape, multires: int, activation: str, slope: float):
        if activation not in OUT_ACTIVATIONS:
            raise ValueError(f"head {name!r}: the grouped path implements the output activations {tuple(OUT_ACTIVATIONS)}, not {activation!r}")
        self.name, self.shape, self.multires, self.activation, self.slope = name, shape, int(max(multires, 0)), activation, float(slope)


def net_op_count(shape: _Shape, precision: str = "fp32") -> int:
    """ops of the longer of the net's two chains: what it takes of a group's table (forward and backward use the same groups)"""
    return max(len(_forward_plan(shape, True, precision).ops), len(_backward_plan(shape, True, True, precision).ops))


def partition_heads(specs: Sequence[HeadSpec], precisions: Sequence[str]) -> List[List[int]]:
    """Indices of `specs`, grouped: one part per (hidden width, chain precision) in order of first appearance, a part cut where
    the next net would exceed SR_MLP_GROUP_MAX_NETS nets or SR_MLP_GROUP_MAX_OPS ops (the table is a kernel argument)."""
    parts: dict = {}
    for i, (s, p) in enumerate(zip(specs, precisions)):
        parts.setdefault((s.shape.hidden, _checked_precision(p)), []).append(i)
    groups = []
    for (_, precision), members in parts.items():
        cur, ops = [], 0
        for i in members:
            k = net_op_count(specs[i].shape, precision)
            if k > _lib.MLP_GROUP_MAX_OPS:
                raise ValueError(f"head {specs[i].name!r}: {k} ops do not fit one group table ({_lib.MLP_GROUP_MAX_OPS})")
            if cur and (len(cur) >= _lib.MLP_GROUP_MAX_NETS or ops + k > _lib.MLP_GROUP_MAX_OPS):
                groups.append(cur)
                cur, ops = [], 0
            cur.append(i)
            ops += k
        groups.append(cur)
    return groups


class _GroupPlan:
    """The plans of a group's nets as ONE pack job table and ONE op table (net after net, each net's entries exactly those of its
    own _Plan) + the net table of sr_mlp_chain_group; built once, pointers patched per call like _Plan."""

    def __init__(self, plans: Sequence[_Plan]):
        self.plans = list(plans)
        self.mode, self.bf16 = self.plans[0].mode, self.plans[0].bf16
        if any(p.mode != self.mode for p in self.plans):
            raise ValueError("the nets of a group share one chain precision")
        self._arrays = None
        self._lock = threading.Lock()

    def _freeze(self):
        counts = [len(p.ops) for p in self.plans]
        total = sum(counts)
        if len(self.plans) > _lib.MLP_GROUP_MAX_NETS or total > _lib.MLP_GROUP_MAX_OPS:
            raise ValueError("too many nets or ops for one group table")
        jobs, ops, nets = (_lib.SrMlpPackJob * total)(), (_lib.SrMlpOp * total)(), (_lib.SrMlpNet * len(self.plans))()
        binds, at, start = [], 0, 0
        for y, (plan, cnt) in enumerate(zip(self.plans, counts)):
            own, at = plan._fill(jobs, ops, start, at)
            binds += [(obj, field, None if sym == "buf" else y, sym, idx, off) for obj, field, sym, idx, off in own]
            nets[y].ops = C.cast(C.byref(ops, start * C.sizeof(_lib.SrMlpOp)), C.POINTER(_lib.SrMlpOp))
            nets[y].n_ops = cnt
            start += cnt
        self._arrays = (jobs, ops, nets, binds, at)

    def tables(self):
        """(pack jobs, ops, nets, binds, buffer bytes): the frozen arrays"""
        with self._lock:
            if self._arrays is None:
                self._freeze()
            return self._arrays

    def run(self, lib, ptrs_per_net: Sequence[dict], device, n_points: int, ht: int, slope: float, stream) -> torch.Tensor:
        jobs, ops, nets, binds, total = self.tables()
        with self._lock:      # the descriptor arrays are shared by every call with these shapes
            buf = torch.empty(total // 4, dtype=torch.float32, device=device)
            base = buf.data_ptr()
            for obj, field, y, sym, idx, off in binds:
                setattr(obj, field, (base if y is None else ptrs_per_net[y][sym][idx]) + off)
            pack, chain = _entries(lib, self.mode, group=True)
            step = _lib.MLP_MAX_PACK_JOBS
            for lo in range(0, len(jobs), step):          # all nets' matrices: 32 jobs per pack launch
                part = C.cast(C.byref(jobs, lo * C.sizeof(_lib.SrMlpPackJob)), C.POINTER(_lib.SrMlpPackJob))
                _lib.check(pack(min(step, len(jobs) - lo), part, stream))
            _lib.check(chain(n_points, ht, len(nets), nets, slope, stream))
        return buf


_GROUP_PLANS: dict = {}


def _group_plan(kind: str, shapes: Sequence[_Shape], flag: bool, precision: str) -> _GroupPlan:
    """kind "fwd": flag = save the activations; "bwd": flag = dL/dx0 is needed (leaky' always from the sign bits)"""
    key = (kind, flag, precision, tuple(id(s) for s in shapes))
    hit = _GROUP_PLANS.get(key)
    if hit is None:
        plans = [_forward_plan(s, flag, precision) if kind == "fwd" else _backward_plan(s, flag, True, precision) for s in shapes]
        hit = _GROUP_PLANS[key] = (list(shapes), _GroupPlan(plans))      # the shapes are kept: their ids are the key
    return hit[1]


class GroupSpec:
    """What one grouped call runs: the heads, the chain precision of each, the groups (lists of head indices, partition_heads),
    the time encoding's frequencies."""

    def __init__(self, specs: Sequence[HeadSpec], precisions: Sequence[str], time_multires: int = 0):
        self.heads = list(specs)
        self.precisions = [_checked_precision(p) for p in precisions]
        if len({h.slope for h in self.heads}) > 1:
            raise ValueError("the heads of a grouped step share one leaky-ReLU slope")
        self.slope = self.heads[0].slope
        self.time_multires = int(max(time_multires, 0))
        self.groups = partition_heads(self.heads, self.precisions)
        if len(self.heads) > _lib.MLP_GROUP_MAX_HEADS:
            raise ValueError(f"at most {_lib.MLP_GROUP_MAX_HEADS} heads per grouped step")


def grouped_inputs_ok(xyz, feat, time) -> bool:
    """whether the grouped input kernel can take these per-call inputs (otherwise the caller runs the separate path)"""
    if not (torch.is_tensor(xyz) and xyz.is_cuda and xyz.dim() == 2 and xyz.shape[1] == 3 and xyz.dtype == torch.float32 and xyz.shape[0] > 0):
        return False
    if feat is not None and not (feat.is_cuda and feat.dtype == torch.float32 and feat.dim() == 2 and feat.shape[0] == xyz.shape[0] and
                                 feat.device == xyz.device):
        return False
    if time is not None and not (torch.is_tensor(time) and time.is_cuda and time.dtype == torch.float32 and not time.requires_grad and
                                 time.numel() == xyz.shape[0] and time.device == xyz.device):
        return False
    return True


def _head_input_table(heads: Sequence[HeadSpec], x0s=None, dx0s=None):
    arr = (_lib.SrMlpHeadInput * len(heads))()
    for i, h in enumerate(heads):
        arr[i].multires, arr[i].row = h.multires, h.shape.mem_pad
        arr[i].x0 = x0s[i].data_ptr() if x0s is not None else None
        arr[i].dL_dx0 = dx0s[i].data_ptr() if dx0s is not None else None
    return arr


def _group_input_forward(lib, heads: Sequence[HeadSpec], time_multires: int, x32, f32, t32, x0s):
    """x0 of every head: one launch (sr_mlp_group_input_forward)"""
    dev = x32.device
    with torch.cuda.device(dev):
        _lib.check(lib.sr_mlp_group_input_forward(x32.shape[0], len(heads), _head_input_table(heads, x0s=x0s), 0 if f32 is None else f32.shape[1],
                                                  time_multires, _lib.ptr(x32), _lib.ptr(f32), _lib.ptr(t32), _lib.stream(dev)))


def _group_input_backward(lib, heads: Sequence[HeadSpec], n_feat: int, x32, dx0s, d_xyz, d_feat):
    """d_xyz and d_feat, summed over the heads in table order: one launch (sr_mlp_group_input_backward)"""
    dev = x32.device
    with torch.cuda.device(dev):
        _lib.check(lib.sr_mlp_group_input_backward(x32.shape[0], len(heads), _head_input_table(heads, dx0s=dx0s), n_feat, _lib.ptr(x32),
                                                   _lib.ptr(d_xyz), _lib.ptr(d_feat), _lib.stream(dev)))


def _head_output_table(heads: Sequence[HeadSpec], which, ys, outs=None, dOuts=None, Gs=None):
    arr = (_lib.SrMlpHeadOutput * max(len(which), 1))()
    for j, i in enumerate(which):
        h = heads[i]
        arr[j].y, arr[j].out_features, arr[j].row, arr[j].activation = ys[i].data_ptr(), h.shape.out_features, h.shape.out_pad, OUT_ACTIVATIONS[h.activation]
        arr[j].out = outs[i].data_ptr() if outs is not None else None
        arr[j].dL_dout = dOuts[i].data_ptr() if dOuts is not None and dOuts[i] is not None else None
        arr[j].g = Gs[i].data_ptr() if Gs is not None else None
    return arr


def _group_output(lib, heads: Sequence[HeadSpec], ys):
    """the heads' activated outputs: one launch for every head with an activation (sr_mlp_group_output); "none" is y itself"""
    which = [i for i, h in enumerate(heads) if h.activation != "none"]
    outs = [torch.empty_like(y) if i in which else y for i, y in enumerate(ys)]
    if which:
        dev = ys[0].device
        with torch.cuda.device(dev):
            _lib.check(lib.sr_mlp_group_output(ys[0].shape[0], len(which), _head_output_table(heads, which, ys, outs=outs), _lib.stream(dev)))
    return outs


def _group_top_gradient(lib, heads: Sequence[HeadSpec], ys, dOuts, slope: float, Gs):
    """G = dOut o act'(.) o leaky'(y), zero-padded, for every head (zeros where dOut is None): one launch (sr_mlp_group_top_gradient)"""
    dev = ys[0].device
    table = _head_output_table(heads, list(range(len(heads))), ys, dOuts=dOuts, Gs=Gs)
    with torch.cuda.device(dev):
        _lib.check(lib.sr_mlp_group_top_gradient(ys[0].shape[0], len(heads), table, slope, _lib.stream(dev)))


class _GroupedHeadsFn(torch.autograd.Function):
    """inputs: xyz, feat, time, spec, grad mode, then per head its weights and its biases; outputs: every head's activated output"""

    @staticmethod
    def forward(ctx, xyz, feat, time, spec: GroupSpec, grad_enabled: bool, *params):
        lib = _lib.load()
        heads_, weights, biases, k = spec.heads, [], [], 0
        for h in heads_:
            L = h.shape.n_layers
            weights.append([_f32c(p) for p in params[k:k + L]])
            biases.append([_f32c(p) for p in params[k + L:k + 2 * L]])
            k += 2 * L
        dev, n = xyz.device, xyz.shape[0]
        x32 = _f32c(xyz)
        f32 = _f32c(feat) if feat is not None else None
        t32 = time.detach().to(torch.float32).reshape(-1).contiguous() if time is not None else None
        x0s = [torch.empty(n, h.shape.mem_pad, dtype=torch.float32, device=dev) for h in heads_]
        _group_input_forward(lib, heads_, spec.time_multires, x32, f32, t32, x0s)
        need = grad_enabled and any(ctx.needs_input_grad)
        ys = [torch.empty(n, h.shape.out_features, dtype=torch.float32, device=dev) for h in heads_]
        acts = [torch.empty(h.shape.n_layers - 1, n, h.shape.hidden, dtype=torch.float32, device=dev) if need else None for h in heads_]
        signs = [torch.empty(h.shape.n_layers - 1, n, 4, dtype=torch.int32, device=dev) if need else None for h in heads_]
        for members in spec.groups:
            shapes = [heads_[i].shape for i in members]
            ptrs = []
            for i, sh in zip(members, shapes):
                H, L = sh.hidden, sh.n_layers
                ptrs.append({"W": [w.data_ptr() for w in weights[i]], "B": [b.data_ptr() for b in biases[i]], "x0": (x0s[i].data_ptr(),),
                             "y": (ys[i].data_ptr(),),
                             "acts": [acts[i].data_ptr() + 4 * j * n * H for j in range(L - 1)] if need else (),
                             "signs": [signs[i].data_ptr() + 16 * j * n for j in range(L - 1)] if need else ()})
            with torch.cuda.device(dev):
                _group_plan("fwd", shapes, need, spec.precisions[members[0]]).run(lib, ptrs, dev, n, shapes[0].ht, spec.slope, _lib.stream(dev))
        outs = _group_output(lib, heads_, ys)
        ctx.set_materialize_grads(False)      # a head nobody used arrives as None: its top gradient is written as zeros by the kernel
        if need:
            ctx.spec, ctx.n_feat = spec, 0 if f32 is None else f32.shape[1]
            ctx.save_for_backward(x32, *x0s, *acts, *signs, *ys, *[w for ws in weights for w in ws])
        return tuple(outs)

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, *dOuts):
        lib = _lib.load()
        spec = ctx.spec
        heads_, nh = spec.heads, len(spec.heads)
        x32, *rest = ctx.saved_tensors
        x0s, acts, signs, ys, flat = rest[:nh], rest[nh:2 * nh], rest[2 * nh:3 * nh], rest[3 * nh:4 * nh], rest[4 * nh:]
        weights, k = [], 0
        for h in heads_:
            weights.append(flat[k:k + h.shape.n_layers])
            k += h.shape.n_layers
        dev, n = x32.device, x32.shape[0]
        dOuts = [None if d is None else d.to(torch.float32).contiguous() for d in dOuts]
        Gs = [torch.empty(n, h.shape.out_pad, dtype=torch.float32, device=dev) for h in heads_]
        _group_top_gradient(lib, heads_, ys, dOuts, spec.slope, Gs)
        need_xyz, need_feat = ctx.needs_input_grad[0], ctx.needs_input_grad[1] and ctx.n_feat > 0
        need_input = need_xyz or need_feat
        dzs = [torch.empty(h.shape.n_layers - 1, n, h.shape.hidden, dtype=torch.float32, device=dev) for h in heads_]
        dx0s = [torch.empty(n, h.shape.mem_pad, dtype=torch.float32, device=dev) if need_input else None for h in heads_]
        for members in spec.groups:
            shapes = [heads_[i].shape for i in members]
            ptrs = []
            for i, sh in zip(members, shapes):
                H, L = sh.hidden, sh.n_layers
                ptrs.append({"W": [w.data_ptr() for w in weights[i]], "G": (Gs[i].data_ptr(),), "dx0": (dx0s[i].data_ptr() if need_input else 0,),
                             "acts": [acts[i].data_ptr() + 4 * j * n * H for j in range(L - 1)],
                             "dz": [dzs[i].data_ptr() + 4 * j * n * H for j in range(L - 1)],
                             "signs": [signs[i].data_ptr() + 16 * j * n for j in range(L - 1)]})
            with torch.cuda.device(dev):
                _group_plan("bwd", shapes, need_input, spec.precisions[members[0]]).run(lib, ptrs, dev, n, shapes[0].ht, spec.slope, _lib.stream(dev))
        d_xyz = torch.empty(n, 3, dtype=torch.float32, device=dev) if need_xyz else None
        d_feat = torch.empty(n, ctx.n_feat, dtype=torch.float32, device=dev) if need_feat else None
        if need_input:
            _group_input_backward(lib, heads_, ctx.n_feat, x32, dx0s, d_xyz, d_feat)
        grads, at = [], 5
        for i, h in enumerate(heads_):       # weight and bias gradients: one slab-kernel call per net, unchanged
            L = h.shape.n_layers
            want = ctx.needs_input_grad[at:at + 2 * L]
            if any(want):
                dWs, dbs = _weight_grads(h.shape, x0s[i], acts[i], Gs[i], dzs[i], weights[i])
                grads += [g if w else None for g, w in zip(list(dWs) + list(dbs), want)]
            else:
                grads += [None] * (2 * L)
            at += 2 * L
        return (d_xyz, d_feat, None, None, None, *grads)


def fused_grouped_heads(spec: GroupSpec, xyz: torch.Tensor, feat: Optional[torch.Tensor], time: Optional[torch.Tensor],
                        weights: Sequence[Sequence[torch.Tensor]], biases: Sequence[Sequence[torch.Tensor]]) -> Tuple[torch.Tensor, ...]:
    """Every head of `spec` on (xyz [N, 3], feat [N, F] or None, time [N] or None) -> the heads' activated outputs, differentiable
    with respect to xyz, feat and every weight and bias.  The caller has checked the inputs with `grouped_inputs_ok`."""
    _lib.load()
    n_feat = 0 if feat is None else feat.shape[1]
    n_time = 0 if time is None else 1 + 2 * spec.time_multires
    flat = []
    for h, ws, bs in zip(spec.heads, weights, biases):
        if h.shape.d_in != 3 * (1 + 2 * h.multires) + n_feat + n_time or len(ws) != h.shape.n_layers or len(bs) != h.shape.n_layers:
            raise ValueError(f"head {h.name!r}: the inputs do not make the {h.shape.d_in} input channels its first layer reads")
        flat += list(ws) + list(bs)
    return _GroupedHeadsFn.apply(xyz, feat, time, spec, torch.is_grad_enabled(), *flat)
