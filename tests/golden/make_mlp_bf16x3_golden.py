"""Writes tests/golden/mlp_bf16x3_cases.npz: the reference's own GeneralMLP (utils/time_utils.py:123-191) on the six committed
general_mlp_*.npz cases (their states, inputs, probes and frames; 40 points = one full and one partial wavefront), run three ways:

    ref64    in float64, as it is
    emul64   in float64 with `torch.nn.functional.linear` replaced by a linear op that splits its operands into two bfloat16
             values, hi(v) = bf(v) and lo(v) = bf(v - hi(v)), and drops lo . lo:
             y = b + hi(x) hi(W)^T + lo(x) hi(W)^T + hi(x) lo(W)^T,
             straight-through backward dx = hi(dy) hi(W) + lo(dy) hi(W) + hi(dy) lo(W), dW = dy^T x, db = sum dy
    emul32   the same in float32

Run on a CPU where a reference checkout exists (make_golden.py's REF):    python tests/golden/make_mlp_bf16x3_golden.py

Numeric arrays only travel.  Per case `<name>` and tensor `<t>` (out, grad_xyz, grad_feat, grad:<parameter>):
    <name>/emul64/<t>     float64 -- except the `.weight` gradients, stored as float32, and the `.matrix_t` gradients, not stored:
                          d matrix_t = weights_t[frame] (x) d weight exactly, the tests rebuild them (as for mlp_bf16_cases.npz)
    <name>/e_fmt3/<t>     || emul64 - ref64 ||_2 / || ref64 ||_2     what the split format costs
    <name>/e_32/<t>       || emul32 - emul64 ||_2 / || emul64 ||_2   what float32 arithmetic around the same splitting costs
    <name>/max3/<t>       max | emul64 - ref64 | / max | ref64 |      the measure of tests/test_general_mlp.py, float64 emulation
    <name>/max3_32/<t>    max | emul32 - ref64 | / max | ref64 |      ... float32 emulation

The script fails unless e_fmt3 <= e_fmt / 64 for every tensor of mlp_bf16_cases.npz (per product bf16 loses 2 x 2^-8 and the split
3 x 2^-16: a ratio of 1/170) and max3, max3_32 stay within the project's fp32 tolerances (2e-5 outputs, 2e-4 gradients)."""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden  # noqa: E402  (case table, reference import)

FLOOR_OUT, FLOOR_GRAD = 2e-5, 2e-4


def bf(t):
    return t.to(torch.bfloat16).to(t.dtype)


def split(t):
    hi = bf(t)
    return hi, bf(t - hi)


class SplittingLinear(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, W, b):
        ctx.save_for_backward(x, W)
        (xh, xl), (Wh, Wl) = split(x), split(W)
        return xh @ Wh.t() + xl @ Wh.t() + xh @ Wl.t() + b

    @staticmethod
    def backward(ctx, dy):
        x, W = ctx.saved_tensors
        (dh, dl), (Wh, Wl) = split(dy), split(W)
        return dh @ Wh + dl @ Wh + dh @ Wl, dy.t() @ x, dy.sum(0)


def run(GeneralMLP, kwargs, data, dtype, splitting):
    net = GeneralMLP(**kwargs)
    net.load_state_dict({k[len("param:"):]: torch.from_numpy(data[k]) for k in data.files if k.startswith("param:")}, strict=True)
    net = net.to(dtype)
    xyz = torch.from_numpy(data["xyz"]).to(dtype).requires_grad_()
    feat = torch.from_numpy(data["feat"]).to(dtype).requires_grad_() if "feat" in data.files else None
    frame = int(data["frame_id"])
    keep = torch.nn.functional.linear
    if splitting:
        torch.nn.functional.linear = lambda x, W, b=None: SplittingLinear.apply(x, W, b)
    try:
        out = net(xyz, feat, frame_id=None if frame < 0 else torch.tensor(frame))
        (out * torch.from_numpy(data["probe"]).to(dtype)).sum().backward()
    finally:
        torch.nn.functional.linear = keep
    res = {"out": out.detach(), "grad_xyz": xyz.grad}
    if feat is not None:
        res["grad_feat"] = feat.grad
    for k, p in net.named_parameters():
        res["grad:" + k] = p.grad if p.grad is not None else torch.zeros_like(p)
    return {k: v.double() for k, v in res.items()}


def rel(a, b):
    return float((a - b).norm() / b.norm().clamp_min(1e-300))


def rel_max(a, b):
    return float((a - b).abs().max() / b.abs().max().clamp_min(1e-300))


def main():
    GeneralMLP = make_golden.import_time_utils().GeneralMLP
    bf16 = np.load(os.path.join(HERE, "mlp_bf16_cases.npz"))
    arrays, least, bad = {}, float("inf"), []
    for name, (kwargs, _, _) in make_golden.GENERAL_MLP_CASES.items():
        data = np.load(os.path.join(HERE, f"general_mlp_{name}.npz"))
        ref64 = run(GeneralMLP, kwargs, data, torch.float64, False)
        emul64 = run(GeneralMLP, kwargs, data, torch.float64, True)
        emul32 = run(GeneralMLP, kwargs, data, torch.float32, True)
        for t in ref64:
            e_fmt3, e_32 = rel(emul64[t], ref64[t]), rel(emul32[t], emul64[t])
            m64, m32 = rel_max(emul64[t], ref64[t]), rel_max(emul32[t], ref64[t])
            for key, v in (("e_fmt3", e_fmt3), ("e_32", e_32), ("max3", m64), ("max3_32", m32)):
                arrays[f"{name}/{key}/{t}"] = np.array(v)
            e_fmt = float(bf16[f"{name}/e_fmt/{t}"])
            gain = e_fmt / e_fmt3 if e_fmt3 > 0 else float("inf")
            if e_fmt > 0:
                least = min(least, gain)
            floor = FLOOR_OUT if t == "out" else FLOOR_GRAD
            if not e_fmt3 <= e_fmt / 64 or not max(m64, m32) <= floor:
                bad.append((name, t, e_fmt3, e_fmt, m64, m32))
            print(f"{name:12s} {t:28s} e_fmt3 {e_fmt3:.3e}  e_32 {e_32:.3e}  bf16 / bf16x3 {gain:8.1f}  max3 {m64:.2e}  max3_32 {m32:.2e}")
            if t.endswith(".matrix_t"):
                continue
            arrays[f"{name}/emul64/{t}"] = emul64[t].numpy().astype(np.float32 if t.endswith(".weight") else np.float64)
    print("smallest bf16 / bf16x3 ratio of e_fmt:", least)
    if bad:
        raise SystemExit(f"the split format does not keep what it should on these cases: {bad}")
    path = os.path.join(HERE, "mlp_bf16x3_cases.npz")
    np.savez_compressed(path, **arrays)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
