"""Plane generator of the deform network's encoder: the reference's `Tensorial2D` around `TimeVAEDecoder`
(scene/tripFields.py:176-204, :383-428, scene/time_decoders.py) on HIP kernels (csrc/planegen.hip).

The reference does not hold its tri-plane as a parameter: three small CNN decoders generate it from fixed noise maps on every
step (8 x 20 x 20 -> 16 x 160 x 160 each: conv_in, a mid block of two resnet blocks around one attention layer, four up blocks
of two resnet blocks, three of them followed by a nearest x2 upsample + convolution, GroupNorm, SiLU, conv_out).  This module
has the same classes with the reference's constructor keywords and exactly its parameter and buffer names, so the
`encoder.subs.*` tensors of a reference `deform.pth` load with `strict=True`.

Every 3 x 3 convolution with the GroupNorm + SiLU in front of it, the upsample and the residual add behind it is ONE kernel
launch for ALL planes (a job table with one row per plane); one `torch.autograd.Function` spans the whole generator, saves the
layer inputs and the GroupNorm statistics and recomputes the activations in the backward.  The mid block's attention (400
tokens x 32 channels) has two paths: "torch" (the default: float64 torch ops, the planes batched through `torch.bmm`, the
backward a second evaluation under autograd) and "fused" (opt-in: csrc/attention.hip, 3 launches forward and 6 backward for all
planes, double arithmetic inside the kernels, float32 tensors only); `set_attention`, SPLATFIELDS_PLANE_ATTENTION or the
`attention=` keyword of the modules select it.  What stays torch ops with "fused": the `weight + frame_weights[frame_id]` of
`layer_strategy='per_frame'` (indexed on the device).  Blocks that change width (a 1 x 1 `conv_shortcut`) do not occur in the
reference's configuration and are not built.  There is no CPU path.
"""
from __future__ import annotations

import ctypes as C
import math
import os
from typing import Optional, Sequence

import torch
import torch.nn.functional as F
from torch import nn

from . import _lib
from ._lib import f32c
from .triplane import TriPlaneSampler

EPS = 1e-6      # every GroupNorm of the decoder (time_decoders.py: resnet_eps, conv_norm_out)
_N_TENSORS = {"conv": 2, "res": 8, "attn": 10, "up": 2, "out": 4}

ATTENTIONS = ("torch", "fused")
ATTENTION_LAUNCHES = (3, 6)     # library launches of the "fused" attention layer: (forward, backward), whatever the number of planes


def _checked_attention(name) -> str:
    if name not in ATTENTIONS:
        raise ValueError(f"unknown plane-generator attention {name!r}: expected one of {ATTENTIONS}")
    return name


# process default of the mid block's attention layer, read once: SPLATFIELDS_PLANE_ATTENTION=fused turns the HIP kernels on for
# every generator that does not name a path itself
_ATTENTION = _checked_attention(os.environ.get("SPLATFIELDS_PLANE_ATTENTION") or "torch")


def set_attention(name: str) -> str:
    """Process default of the generator's attention layer: "torch" (float64 torch ops) or "fused" (csrc/attention.hip).
    Returns the previous setting."""
    global _ATTENTION
    prev, _ATTENTION = _ATTENTION, _checked_attention(name)
    return prev


def attention() -> str:
    return _ATTENTION


def resolve_attention(name: Optional[str]) -> str:
    """`None` -> the process default, at call time."""
    return _ATTENTION if name is None else _checked_attention(name)


# ---- the kernels behind one entry each -----------------------------------------------------------------------------------------
def _addr(v, i):
    """pointer of plane i: `v` is a list of per-plane tensors, a batched tensor [n, ...] or None"""
    if v is None:
        return None
    if isinstance(v, (list, tuple)):
        return None if v[i] is None else v[i].data_ptr()
    return v.data_ptr() + i * v.stride(0) * v.element_size()


class _Run:
    """the launches of one forward or backward: n planes, one device, the caller's stream"""

    def __init__(self, dev, n, groups):
        if n < 1 or n > _lib.PLANE_MAX_JOBS:
            raise ValueError(f"1 .. {_lib.PLANE_MAX_JOBS} planes go through one launch, got {n}")
        self.lib, self.dev, self.n, self.groups = _lib.load(), dev, n, groups
        self.stream = _lib.stream(dev)

    def jobs(self, **fields):
        arr = (_lib.SrPlaneJob * self.n)()
        for i in range(self.n):
            for name, v in fields.items():
                setattr(arr[i], name, _addr(v, i))
        return arr

    def attention_jobs(self, **fields):
        arr = (_lib.SrAttentionJob * self.n)()
        for i in range(self.n):
            for name, v in fields.items():
                setattr(arr[i], name, _addr(v, i))
        return arr

    def new(self, *shape):
        return torch.empty(self.n, *shape, dtype=torch.float32, device=self.dev)

    def call(self, fn, *args):
        if fn(*args) != 0:
            raise ValueError("libsplatraster: " + self.lib.sr_last_error().decode("utf-8", "replace"))

    def bytes(self, size):
        if size == 0:
            raise ValueError("libsplatraster: unsupported shape for the plane generator's kernels")
        return torch.empty(size, dtype=torch.uint8, device=self.dev)

    def stats(self, x, channels, h, w, groups=None):
        groups = self.groups if groups is None else groups
        out = self.new(groups, 4)      # mean, rstd, mean_lo, unused (include/splatraster.h)
        ws = self.bytes(self.lib.sr_groupnorm_stats_workspace(self.n, channels, groups, h, w))
        self.call(self.lib.sr_groupnorm_stats, self.n, self.jobs(x=x, stats=out), channels, groups, h, w, EPS, C.c_void_p(ws.data_ptr()), self.stream)
        return out

    def conv(self, x, w, b, cin, cout, h, wd, norm=None, up=False, residual=None, silu_out=False, groups=None):
        """x [cin, h, wd] per plane -> out [n, cout, H, W] (and the pre-activation with silu_out); norm = (gamma, beta, stats)"""
        flags = (_lib.CONV_PROLOGUE if norm else 0) | (_lib.CONV_UPSAMPLE if up else 0) | (_lib.CONV_RESIDUAL if residual is not None else 0) | \
            (_lib.CONV_SILU_OUT if silu_out else 0)
        H, W = (2 * h, 2 * wd) if up else (h, wd)
        out = self.new(cout, H, W)
        pre = self.new(cout, H, W) if silu_out else None
        g, be, st = norm if norm else (None, None, None)
        self.call(self.lib.sr_conv3x3_forward, self.n, self.jobs(x=x, weight=w, bias=b, gamma=g, beta=be, stats=st, residual=residual, out=out, pre=pre),
                  cin, cout, h, wd, self.groups if groups is None else groups, flags, self.stream)
        return (out, pre) if silu_out else out

    def backward_data(self, dy, w, cin, cout, h, wd, up=False, pre=None):
        flags = (_lib.CONV_UPSAMPLE if up else 0) | (_lib.CONV_SILU_OUT if pre is not None else 0)
        dx = self.new(cin, h, wd)
        self.call(self.lib.sr_conv3x3_backward_data, self.n, self.jobs(dy=dy, weight=w, dx=dx, pre=pre), cin, cout, h, wd, flags, self.stream)
        return dx

    def norm_backward(self, ga, x, norm, channels, h, wd, add=None, groups=None):
        groups = self.groups if groups is None else groups
        g, be, st = norm
        dx, dg, db = self.new(channels, h, wd), self.new(channels), self.new(channels)
        ws = self.bytes(self.lib.sr_groupnorm_silu_backward_workspace(self.n, channels, h, wd))
        self.call(self.lib.sr_groupnorm_silu_backward, self.n,
                  self.jobs(dx=ga, x=x, gamma=g, beta=be, stats=st, add=add, dx_out=dx, dgamma=dg, dbeta=db), channels, groups, h, wd,
                  EPS, C.c_void_p(ws.data_ptr()), self.stream)
        return dx, dg, db

    def weight_grad(self, dy, x, cin, cout, h, wd, norm=None, up=False, pre=None, want_residual=False, groups=None):
        flags = (_lib.CONV_PROLOGUE if norm else 0) | (_lib.CONV_UPSAMPLE if up else 0) | (_lib.CONV_SILU_OUT if pre is not None else 0)
        g, be, st = norm if norm else (None, None, None)
        dw, db = self.new(cout, cin, 3, 3), self.new(cout)
        H, W = (2 * h, 2 * wd) if up else (h, wd)
        dres = self.new(cout, H, W) if want_residual and pre is not None else None
        ws = self.bytes(self.lib.sr_conv3x3_weight_grad_workspace(self.n, cin, cout, h, wd, flags))
        self.call(self.lib.sr_conv3x3_weight_grad, self.n,
                  self.jobs(dy=dy, x=x, gamma=g, beta=be, stats=st, pre=pre, dweight=dw, dbias=db, d_residual=dres), cin, cout, h, wd,
                  self.groups if groups is None else groups, flags, C.c_void_p(ws.data_ptr()), self.stream)
        return (dw, db, dres) if want_residual else (dw, db)


    def attention_forward(self, x, p, channels, h, wd):
        """x [channels, h, wd] per plane, p = ten lists of per-plane tensors (group_norm w, b, q w, b, k w, b, v w, b, out w, b)
        -> out [n, channels, h, wd] and the buffer that carries the intermediates to `attention_backward`"""
        size = self.lib.sr_attention_saved_bytes(self.n, channels, self.groups, h, wd)
        saved = self.bytes(size).view(self.n, size // self.n if size else 1)
        out, stats = self.new(channels, h, wd), self.new(self.groups, 4)
        self.call(self.lib.sr_attention_forward, self.n,
                  self.attention_jobs(x=x, gamma=p[0], beta=p[1], stats=stats, wq=p[2], bq=p[3], wk=p[4], bk=p[5], wv=p[6], bv=p[7], wo=p[8],
                                      bo=p[9], out=out, saved=saved), channels, self.groups, h, wd, EPS, self.stream)
        return out, saved

    def attention_backward(self, dy, x, p, saved, channels, h, wd):
        """-> dx [n, channels, h, wd] and the ten parameter gradients [n, ...] in the order of `p`"""
        dx = self.new(channels, h, wd)
        mat, vec = (lambda: self.new(channels, channels)), (lambda: self.new(channels))
        dg, dbe, dwq, dbq, dwk, dbk, dwv, dbv, dwo, dbo = vec(), vec(), mat(), vec(), mat(), vec(), mat(), vec(), mat(), vec()
        ws = self.bytes(self.lib.sr_attention_backward_workspace(self.n, channels, self.groups, h, wd))
        self.call(self.lib.sr_attention_backward, self.n,
                  self.attention_jobs(x=x, gamma=p[0], beta=p[1], wq=p[2], wk=p[4], wv=p[6], wo=p[8], saved=saved, dy=dy, dx=dx, dgamma=dg,
                                      dbeta=dbe, dwq=dwq, dbq=dbq, dwk=dwk, dbk=dbk, dwv=dwv, dbv=dbv, dwo=dwo, dbo=dbo),
                  channels, self.groups, h, wd, EPS, C.c_void_p(ws.data_ptr()), self.stream)
        return dx, (dg, dbe, dwq, dbq, dwk, dbk, dwv, dbv, dwo, dbo)


def _no_cpu(*tensors):
    if not all(t.is_cuda for t in tensors):
        raise RuntimeError("splatfields_amd.plane_generator has no CPU path: tensors must be on a HIP ('cuda') device")


# ---- one fused layer (the unit the kernels are tested by) --------------------------------------------------------------------
class _FusedLayer(torch.autograd.Function):
    @staticmethod
    def forward(ctx, n, groups, prologue, upsample, silu_out, has_residual, *tensors):
        # per plane: x [cin, h, w], weight, bias, gamma, beta, residual (the last three may be absent -> None)
        _no_cpu(*[t for t in tensors if t is not None])
        P = [[None if t is None else f32c(t) for t in tensors[i * 6:(i + 1) * 6]] for i in range(n)]
        col = lambda j: [p[j] for p in P]
        x, w, b = col(0), col(1), col(2)
        cout, cin = w[0].shape[:2]
        h, wd = x[0].shape[-2:]
        run = _Run(x[0].device, n, groups)
        with torch.cuda.device(run.dev):
            norm = (col(3), col(4), run.stats(x, cin, h, wd)) if prologue else None
            res = run.conv(x, w, b, cin, cout, h, wd, norm=norm, up=upsample, residual=col(5) if has_residual else None, silu_out=silu_out)
        out, pre = res if silu_out else (res, None)
        ctx.P, ctx.norm, ctx.pre, ctx.args = P, norm, pre, (n, groups, prologue, upsample, silu_out, has_residual, cin, cout, h, wd)
        return out

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g):
        n, groups, prologue, upsample, silu_out, has_residual, cin, cout, h, wd = ctx.args
        P, norm, pre = ctx.P, ctx.norm, ctx.pre
        col = lambda j: [p[j] for p in P]
        g = f32c(g)
        run = _Run(g.device, n, groups)
        with torch.cuda.device(run.dev):
            dw, db, dres = run.weight_grad(g, col(0), cin, cout, h, wd, norm=norm, up=upsample, pre=pre, want_residual=True)
            ga = run.backward_data(g, col(1), cin, cout, h, wd, up=upsample, pre=pre)
            if prologue:
                dx, dg, dbe = run.norm_backward(ga, col(0), norm, cin, h, wd)
            else:
                dx, dg, dbe = ga, None, None
        if dres is None:
            dres = g
        grads = []
        for i in range(n):
            grads += [dx[i].view_as(P[i][0]), dw[i], db[i] if P[i][2] is not None else None, dg[i] if prologue else None,
                      dbe[i] if prologue else None, dres[i] if has_residual else None]
        return (None,) * 6 + tuple(grads)


def fused_layer(x: Sequence[torch.Tensor], weight, bias, gamma=None, beta=None, residual=None, groups: int = 1, upsample: bool = False,
                silu_out: bool = False) -> torch.Tensor:
    """One layer of the generator for n planes in one launch: every argument is a list of n per-plane tensors (x [Cin, h, w],
    weight [Cout, Cin, 3, 3], bias [Cout], gamma / beta [Cin] or None for no GroupNorm + SiLU prologue, residual [Cout, H, W] or
    None) -> [n, Cout, H, W].  Differentiable with respect to every tensor argument."""
    n = len(x)
    prologue, has_res = gamma is not None, residual is not None
    flat = []
    for i in range(n):
        flat += [x[i], weight[i], None if bias is None else bias[i], gamma[i] if prologue else None, beta[i] if prologue else None,
                 residual[i] if has_res else None]
    return _FusedLayer.apply(n, groups, prologue, upsample, silu_out, has_res, *flat)


# ---- the attention layer on its kernels (the unit they are tested by) ---------------------------------------------------------
class _FusedAttention(torch.autograd.Function):
    @staticmethod
    def forward(ctx, n, groups, *tensors):
        # per plane: x [C, h, w], then the ten parameters in the order of `TimeVAEDecoder.program`
        _no_cpu(*tensors)
        P = [[f32c(t) for t in tensors[i * 11:(i + 1) * 11]] for i in range(n)]
        col = lambda j: [p[j] for p in P]
        c, h, wd = P[0][0].shape[-3:]
        run = _Run(P[0][0].device, n, groups)
        with torch.cuda.device(run.dev):
            out, saved = run.attention_forward(col(0), [col(j) for j in range(1, 11)], c, h, wd)
        ctx.P, ctx.kept, ctx.args = P, saved, (n, groups, c, h, wd)
        return out

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g):
        n, groups, c, h, wd = ctx.args
        P = ctx.P
        col = lambda j: [p[j] for p in P]
        g = f32c(g)
        run = _Run(g.device, n, groups)
        with torch.cuda.device(run.dev):
            dx, dp = run.attention_backward(g, col(0), [col(j) for j in range(1, 11)], ctx.kept, c, h, wd)
        grads = []
        for i in range(n):
            grads += [dx[i].view_as(P[i][0])] + [d[i] for d in dp]
        return (None, None) + tuple(grads)


def fused_attention(x: Sequence[torch.Tensor], group_norm_weight, group_norm_bias, to_q_weight, to_q_bias, to_k_weight, to_k_bias,
                    to_v_weight, to_v_bias, to_out_weight, to_out_bias, groups: int = 1) -> torch.Tensor:
    """The mid block's attention layer for n planes on the kernels of csrc/attention.hip (3 launches forward, 6 backward): every
    argument is a list of n per-plane tensors (x [C, h, w], GroupNorm weight / bias [C], the four linears' weight [C, C] and
    bias [C]) -> x + to_out(softmax(q k^T / sqrt(C)) v) as [n, C, h, w].  Differentiable with respect to every tensor argument;
    the gradient of `to_k_bias` is exactly zero."""
    cols = (x, group_norm_weight, group_norm_bias, to_q_weight, to_q_bias, to_k_weight, to_k_bias, to_v_weight, to_v_bias, to_out_weight,
            to_out_bias)
    n = len(x)
    if any(len(c) != n for c in cols):
        raise ValueError("every argument of fused_attention is a list with one tensor per plane")
    return _FusedAttention.apply(n, groups, *[c[i] for i in range(n) for c in cols])


# ---- the whole generator -----------------------------------------------------------------------------------------------------
def _attention(x, params, groups):
    """the mid block's attention for n planes at once: x [n, C, H, W], params[i] = (group_norm w, b, q w, b, k w, b, v w, b, out w, b)"""
    # in float64, rounded to float32 once: softmax is invariant under the key bias, so to_k.bias has a gradient of exactly zero
    # that a float32 evaluation fills with rounding noise of the size of the other gradients' errors; at 400 x 32 the cost is nil
    n, c, h, w = x.shape
    x32, x = x, x.double()
    gw, gb, qw, qb, kw, kb, vw, vb, ow, ob = (torch.stack([p[j] for p in params]).double() for j in range(10))
    t = F.group_norm(x.reshape(1, n * c, h * w), n * groups, eps=EPS).view(n, c, h * w)
    t = (t * gw[:, :, None] + gb[:, :, None]).transpose(1, 2)                            # [n, H W, C]
    q = torch.baddbmm(qb[:, None, :], t, qw.transpose(1, 2))
    k = torch.baddbmm(kb[:, None, :], t, kw.transpose(1, 2))
    v = torch.baddbmm(vb[:, None, :], t, vw.transpose(1, 2))
    probs = (torch.bmm(q, k.transpose(1, 2)) * (1.0 / math.sqrt(c))).softmax(dim=-1)
    o = torch.baddbmm(ob[:, None, :], torch.bmm(probs, v), ow.transpose(1, 2))
    return (o.transpose(1, 2).reshape(n, c, h, w) + x).to(x32.dtype)


def _offsets(ops):
    offs, at = [], 1                      # tensor 0 of a plane is its noise map
    for op in ops:
        offs.append(at)
        at += _N_TENSORS[op]
    return offs, at


class _PlaneGenerator(torch.autograd.Function):
    @staticmethod
    def forward(ctx, ops, groups, n, attention, *tensors):
        _no_cpu(*tensors)
        offs, k = _offsets(ops)
        assert len(tensors) == n * k
        P = [[f32c(t) for t in tensors[i * k:(i + 1) * k]] for i in range(n)]
        col = lambda j: [p[j] for p in P]
        run = _Run(P[0][0].device, n, groups)
        saved = []
        h = col(0)                                     # per-plane noise [1, Cin, h, w]
        hh, ww = h[0].shape[-2:]
        ch = h[0].shape[-3]
        with torch.cuda.device(run.dev):
            for op, o in zip(ops, offs):
                if op == "conv":
                    cout = P[0][o].shape[0]
                    saved.append((h, ch, hh, ww))
                    h = run.conv(h, col(o), col(o + 1), ch, cout, hh, ww)
                    ch = cout
                elif op == "res":
                    s1 = run.stats(h, ch, hh, ww)
                    t = run.conv(h, col(o + 2), col(o + 3), ch, ch, hh, ww, norm=(col(o), col(o + 1), s1))
                    s2 = run.stats(t, ch, hh, ww)
                    out = run.conv(t, col(o + 6), col(o + 7), ch, ch, hh, ww, norm=(col(o + 4), col(o + 5), s2), residual=h)
                    saved.append((h, s1, t, s2, ch, hh, ww))
                    h = out
                elif op == "attn" and attention == "fused":
                    out, kept = run.attention_forward(h, [col(o + j) for j in range(10)], ch, hh, ww)
                    saved.append((h, kept, ch, hh, ww))
                    h = out
                elif op == "attn":
                    saved.append((h,))
                    h = _attention(h, [p[o:o + 10] for p in P], groups).contiguous()
                elif op == "up":
                    saved.append((h, ch, hh, ww))
                    h = run.conv(h, col(o), col(o + 1), ch, ch, hh, ww, up=True)
                    hh, ww = 2 * hh, 2 * ww
                elif op == "out":
                    cout = P[0][o + 2].shape[0]
                    s = run.stats(h, ch, hh, ww)
                    saved.append((h, s, ch, cout, hh, ww))
                    h = run.conv(h, col(o + 2), col(o + 3), ch, cout, hh, ww, norm=(col(o), col(o + 1), s))
        ctx.P, ctx.saved, ctx.spec = P, saved, (ops, groups, n, attention)
        return h

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g):
        ops, groups, n, attention = ctx.spec
        P, saved = ctx.P, ctx.saved
        offs, k = _offsets(ops)
        col = lambda j: [p[j] for p in P]
        G = [[None] * k for _ in range(n)]

        def put(j, batched):
            for i in range(n):
                G[i][j] = batched[i]

        g = f32c(g)
        run = _Run(g.device, n, groups)
        with torch.cuda.device(run.dev):
            for op, o, sv in zip(reversed(ops), reversed(offs), reversed(saved)):
                if op == "out":
                    h, s, ch, cout, hh, ww = sv
                    norm = (col(o), col(o + 1), s)
                    dw, db = run.weight_grad(g, h, ch, cout, hh, ww, norm=norm)
                    ga = run.backward_data(g, col(o + 2), ch, cout, hh, ww)
                    g, dg, dbe = run.norm_backward(ga, h, norm, ch, hh, ww)
                    put(o, dg); put(o + 1, dbe); put(o + 2, dw); put(o + 3, db)
                elif op == "up":
                    h, ch, hh, ww = sv
                    dw, db = run.weight_grad(g, h, ch, ch, hh, ww, up=True)
                    g = run.backward_data(g, col(o), ch, ch, hh, ww, up=True)
                    put(o, dw); put(o + 1, db)
                elif op == "attn" and attention == "fused":
                    h, kept, ch, hh, ww = sv
                    g, dp = run.attention_backward(g, h, [col(o + j) for j in range(10)], kept, ch, hh, ww)
                    for j, v in enumerate(dp):
                        put(o + j, v)
                elif op == "attn":
                    (h,) = sv
                    with torch.enable_grad():
                        x = h.detach().requires_grad_(True)
                        leaves = [[t.detach().requires_grad_(True) for t in p[o:o + 10]] for p in P]
                        y = _attention(x, leaves, groups)
                        got = torch.autograd.grad(y, [x] + [t for p in leaves for t in p], g)
                    g = got[0].contiguous()
                    for i in range(n):
                        G[i][o:o + 10] = got[1 + 10 * i:11 + 10 * i]
                elif op == "res":
                    h, s1, t, s2, ch, hh, ww = sv
                    n1, n2 = (col(o), col(o + 1), s1), (col(o + 4), col(o + 5), s2)
                    dw2, db2 = run.weight_grad(g, t, ch, ch, hh, ww, norm=n2)
                    ga = run.backward_data(g, col(o + 6), ch, ch, hh, ww)
                    gt, dg2, dbe2 = run.norm_backward(ga, t, n2, ch, hh, ww)
                    dw1, db1 = run.weight_grad(gt, h, ch, ch, hh, ww, norm=n1)
                    ga = run.backward_data(gt, col(o + 2), ch, ch, hh, ww)
                    g, dg1, dbe1 = run.norm_backward(ga, h, n1, ch, hh, ww, add=g)
                    for j, v in enumerate((dg1, dbe1, dw1, db1, dg2, dbe2, dw2, db2)):
                        put(o + j, v)
                elif op == "conv":
                    h, ch, hh, ww = sv
                    cout = P[0][o].shape[0]
                    dw, db = run.weight_grad(g, h, ch, cout, hh, ww)
                    put(o, dw); put(o + 1, db)
        return (None, None, None, None) + tuple(t for row in G for t in row)


# ---- modules with the reference's names --------------------------------------------------------------------------------------
class TimeConv2d(nn.Conv2d):
    """reference TimeLoRACompatibleConv (time_decoders.py:21-50): `frame_weights` [n_frames, *weight.shape] under 'per_frame',
    0.01 x the weight as the constructor drew it"""

    def __init__(self, *args, layer_kwargs=None, **kwargs):
        super().__init__(*args, **kwargs)
        layer_kwargs = layer_kwargs or {}
        self.n_frames = layer_kwargs.get("n_frames", 1)
        self.strategy = layer_kwargs.get("strategy", "none")
        if self.strategy == "per_frame":
            self.frame_weights = nn.Parameter(0.01 * self.weight.data[None].repeat_interleave(self.n_frames, dim=0))
        elif self.strategy != "none":
            raise NotImplementedError(self.strategy)

    def get_weights(self, frame_id):
        if self.strategy == "none" or self.n_frames <= 1:
            return self.weight
        if frame_id is None:
            raise ValueError("layer_strategy='per_frame' needs a frame_id (an int or a tensor holding one)")
        if torch.is_tensor(frame_id):                # the rounded tensor `_time2frame_id` returns: indexed on the device
            return self.weight + self.frame_weights.index_select(0, frame_id.reshape(1).long())[0]
        return self.weight + self.frame_weights[int(frame_id)]


class _ResnetBlock(nn.Module):
    def __init__(self, channels, groups, layer_kwargs):
        super().__init__()
        self.norm1 = nn.GroupNorm(groups, channels, eps=EPS)
        self.conv1 = TimeConv2d(channels, channels, 3, padding=1, layer_kwargs=layer_kwargs)
        self.norm2 = nn.GroupNorm(groups, channels, eps=EPS)
        self.conv2 = TimeConv2d(channels, channels, 3, padding=1, layer_kwargs=layer_kwargs)


class _Attention(nn.Module):
    def __init__(self, channels, groups):
        super().__init__()
        self.group_norm = nn.GroupNorm(groups, channels, eps=EPS)
        self.to_q, self.to_k, self.to_v = nn.Linear(channels, channels), nn.Linear(channels, channels), nn.Linear(channels, channels)
        self.to_out = nn.ModuleList([nn.Linear(channels, channels), nn.Dropout(0.0)])


class _Upsample(nn.Module):
    def __init__(self, channels):
        super().__init__()
        self.conv = nn.Conv2d(channels, channels, 3, padding=1)


class _MidBlock(nn.Module):
    def __init__(self, channels, groups, layer_kwargs):
        super().__init__()
        self.attentions = nn.ModuleList([_Attention(channels, groups)])
        self.resnets = nn.ModuleList([_ResnetBlock(channels, groups, layer_kwargs) for _ in range(2)])


class _UpBlock(nn.Module):
    def __init__(self, channels, groups, num_layers, add_upsample, layer_kwargs):
        super().__init__()
        self.resnets = nn.ModuleList([_ResnetBlock(channels, groups, layer_kwargs) for _ in range(num_layers)])
        self.upsamplers = nn.ModuleList([_Upsample(channels)]) if add_upsample else None


class TimeVAEDecoder(nn.Module):
    """reference scene/time_decoders.py:447-625 (`TimeDecoder` + `TimeVAEDecoder.init_weights`), same keywords."""

    def __init__(self, in_channels=12, out_channels=24, up_block_types=("TimeUpDecoderBlock2D",), block_out_channels=(64,), layers_per_block=2,
                 norm_num_groups=32, act_fn="silu", norm_type="group", zero_init_residual=True, layer_kwargs=None, attention=None):
        super().__init__()
        # path of the mid block's attention layer: "torch", "fused" or None = the process default at call time (set_attention)
        self.attention = None if attention is None else _checked_attention(attention)
        if any(t != "TimeUpDecoderBlock2D" for t in up_block_types) or act_fn not in ("silu", "swish") or norm_type != "group":
            raise NotImplementedError("TimeUpDecoderBlock2D blocks with SiLU and GroupNorm are implemented")
        if len(set(block_out_channels)) != 1:
            raise NotImplementedError("blocks that change width (conv_shortcut) are not implemented: the reference's configuration has none")
        width = block_out_channels[0]
        if width % norm_num_groups:
            raise ValueError("norm_num_groups must divide the block width")
        for c in (in_channels, out_channels, width):
            if c % 8 or not 8 <= c <= 64:
                raise ValueError(f"channel counts must be multiples of 8 in 8..64 (the convolution kernels), got {c}")
        layer_kwargs = dict(layer_kwargs or {})
        self.layers_per_block, self.norm_num_groups, self.zero_init_residual = layers_per_block, norm_num_groups, zero_init_residual
        self.conv_in = nn.Conv2d(in_channels, width, 3, padding=1)
        self.up_blocks = nn.ModuleList([_UpBlock(width, norm_num_groups, layers_per_block + 1, i != len(block_out_channels) - 1, layer_kwargs)
                                        for i in range(len(up_block_types))])
        self.mid_block = _MidBlock(width, norm_num_groups, layer_kwargs)
        self.conv_norm_out = nn.GroupNorm(norm_num_groups, width, eps=EPS)
        self.conv_out = nn.Conv2d(width, out_channels, 3, padding=1)
        self.init_weights()

    def init_weights(self):
        for m in self.modules():
            if isinstance(m, nn.Conv2d):
                nn.init.kaiming_normal_(m.weight, a=0, mode="fan_out", nonlinearity="relu")
                nn.init.zeros_(m.bias)
            elif isinstance(m, nn.GroupNorm):
                nn.init.ones_(m.weight)
                nn.init.zeros_(m.bias)
        if self.zero_init_residual:
            for m in self.modules():
                last = m.conv2 if isinstance(m, _ResnetBlock) else m.to_out[0] if isinstance(m, _Attention) else None
                if last is not None:
                    nn.init.zeros_(last.weight)
                    nn.init.zeros_(last.bias)

    def program(self, frame_id=None):
        """(ops, tensors): the layer list and the tensors it consumes in order, convolution weights as `get_weights(frame_id)`"""
        ops, ts = [], []

        def conv(c):
            ts.extend([c.get_weights(frame_id) if isinstance(c, TimeConv2d) else c.weight, c.bias])

        def res(r):
            ops.append("res")
            ts.extend([r.norm1.weight, r.norm1.bias]); conv(r.conv1)
            ts.extend([r.norm2.weight, r.norm2.bias]); conv(r.conv2)

        ops.append("conv"); conv(self.conv_in)
        res(self.mid_block.resnets[0])
        for a, r in zip(self.mid_block.attentions, self.mid_block.resnets[1:]):
            ops.append("attn")
            ts.extend([a.group_norm.weight, a.group_norm.bias, a.to_q.weight, a.to_q.bias, a.to_k.weight, a.to_k.bias, a.to_v.weight, a.to_v.bias,
                       a.to_out[0].weight, a.to_out[0].bias])
            res(r)
        for ub in self.up_blocks:
            for r in ub.resnets:
                res(r)
            if ub.upsamplers is not None:
                ops.append("up"); conv(ub.upsamplers[0].conv)
        ops.append("out")
        ts.extend([self.conv_norm_out.weight, self.conv_norm_out.bias]); conv(self.conv_out)
        return tuple(ops), ts

    def forward(self, z, latent_embeds=None, frame_id=None):
        return generate_planes([self], [z], frame_id)


def generate_planes(decoders: Sequence[TimeVAEDecoder], noises: Sequence[torch.Tensor], frame_id=None, attention: Optional[str] = None) -> torch.Tensor:
    """decoders of identical shape, one noise map [1, Cin, h, w] each -> [n, Cout, H, W]: every layer is one launch for all of them.
    `attention`: "torch", "fused" or None = what the first decoder names, else the process default (set_attention)."""
    mode = resolve_attention(attention if attention is not None else decoders[0].attention)
    flat, ops0 = [], None
    for net, z in zip(decoders, noises):
        ops, ts = net.program(frame_id)
        if ops0 is None:
            ops0, shapes0 = ops, [t.shape for t in ts] + [z.shape]
        elif ops != ops0 or [t.shape for t in ts] + [z.shape] != shapes0:
            raise ValueError("the decoders of one call must have identical shapes")
        flat += [z] + ts
    return _PlaneGenerator.apply(ops0, decoders[0].norm_num_groups, len(decoders), mode, *flat)


class Tensorial2D(nn.Module):
    """reference scene/tripFields.py:176-204: a fixed noise map (buffer `noise`) and the decoder `net` that turns it into a plane"""

    def __init__(self, noise_ch=8, out_ch=16, noise_res=20, layer_kwargs=None, attention=None):
        super().__init__()
        self.noise_ch, self.out_ch, self.noise_res = noise_ch, out_ch, noise_res
        self.upx = 16        # the reference's attribute; its forward (and this one) returns 8 x noise_res: three of four up blocks upsample
        self.register_buffer("noise", torch.randn(1, noise_ch, noise_res, noise_res))
        self.net = TimeVAEDecoder(in_channels=noise_ch, out_channels=out_ch, up_block_types=("TimeUpDecoderBlock2D",) * 4,
                                  block_out_channels=(32, 32, 32, 32), layers_per_block=1, layer_kwargs=layer_kwargs, attention=attention)

    def get_output_shape(self):
        return [self.out_ch, self.noise.size(-2) * self.upx, self.noise.size(-1) * self.upx]

    def forward(self, frame_id=None):
        return self.net(self.noise, frame_id=frame_id)


class VarTriPlaneEncoder(TriPlaneSampler):
    """reference scene/tripFields.py:383-436: three `Tensorial2D` generators (`subs`) + the per-point lookup of `TriPlaneSampler`.
    `config` holds the reference's keys: in_ch, out_ch, noise_res, fuse_mode, layer_kwargs (n_frames, strategy), and `attention`
    ("torch", "fused" or None: the path of the generators' attention layer, see `set_attention`)."""

    takes_frame_id = True     # SplatFields hands `frame_id` to an encoder that says so

    def __init__(self, config: Optional[dict] = None):
        config = dict(config or {})
        in_ch, out_ch, noise_res = config.get("in_ch", 8), config.get("out_ch", 16), config.get("noise_res", 20)
        super().__init__(out_ch=out_ch, resolution=8 * noise_res, fuse_mode=config.get("fuse_mode", "cat"), plane_source=self._generate)
        self.config = config
        self.in_ch, self.out_ch, self.noise_res = in_ch, out_ch, noise_res
        self.subs = nn.ModuleList([Tensorial2D(in_ch, out_ch, noise_res, layer_kwargs=config.get("layer_kwargs"), attention=config.get("attention")) for _ in ("xy", "yz", "zx")])

    def _generate(self, frame_id=None):
        return generate_planes([s.net for s in self.subs], [s.noise for s in self.subs], frame_id)

    def get_planes(self, frame_id=None) -> torch.Tensor:
        return self._generate(frame_id)
