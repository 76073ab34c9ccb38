"""Writes tests/golden/mlp_bf16_cases.npz: the reference's own GeneralMLP (utils/time_utils.py:123-191) on the six committed
general_mlp_*.npz cases (their states, inputs, probes and frames; 40 points = one full and one partial wavefront), run three ways:

    ref64    in float64, as it is
    emul64   in float64 with `torch.nn.functional.linear` replaced by a linear op that rounds its operands to bfloat16:
             y = bf(x) bf(W)^T + b,  straight-through backward dx = bf(dy) bf(W), dW = dy^T x, db = sum dy
    emul32   the same in float32

Run on a CPU where a reference checkout exists (make_golden.py's REF):    python tests/golden/make_mlp_bf16_golden.py

Numeric arrays only travel.  Per case `<name>` and tensor `<t>` (out, grad_xyz, grad_feat, grad:<parameter>):
    <name>/emul64/<t>     float64 -- except the `.weight` gradients, stored as float32, and the `.matrix_t` gradients, not stored:
                          d matrix_t = weights_t[frame] (x) d weight exactly (the composed weight is W + weights_t[frame] @ matrix_t),
                          the tests rebuild them; the parameters are 240 k numbers and a committed file stays below 1 MiB
    <name>/ref64/<t>      float32, for out / grad_xyz / grad_feat only (the float32 run of the reference is in general_mlp_<name>.npz)
    <name>/e_fmt/<t>      || emul64 - ref64 ||_2 / || ref64 ||_2     what the number format costs
    <name>/e_32/<t>       || emul32 - emul64 ||_2 / || emul64 ||_2   what float32 arithmetic around the same rounding costs
    rho                   4 x max e_32 / e_fmt over the tensors with e_fmt >= 10 x floor; floor = the project's fp32 tolerances of
                          tests/test_general_mlp.py (2e-5 outputs, 2e-4 gradients).  The script fails if rho >= 0.5: the bound
                          max(floor, rho e_fmt) of tests/test_gpu_mlp_bf16.py would no longer separate the arithmetic from the format."""
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


class RoundingLinear(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, W, b):
        ctx.save_for_backward(x, W)
        return bf(x) @ bf(W).t() + b

    @staticmethod
    def backward(ctx, dy):
        x, W = ctx.saved_tensors
        return bf(dy) @ bf(W), dy.t() @ x, dy.sum(0)


def run(GeneralMLP, kwargs, data, dtype, rounding):
    net = GeneralMLP(**kwargs)
    net.load_state_dict({k[len("param:"):]: torch.from_numpy(data[k]) for k in data.files if k.startswith("param:")}, strict=True)
    net = net.to(dtype)
    xyz = torch.from_numpy(data["xyz"]).to(dtype).requires_grad_()
    feat = torch.from_numpy(data["feat"]).to(dtype).requires_grad_() if "feat" in data.files else None
    frame = int(data["frame_id"])
    keep = torch.nn.functional.linear
    if rounding:
        torch.nn.functional.linear = lambda x, W, b=None: RoundingLinear.apply(x, W, b)
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


def main():
    GeneralMLP = make_golden.import_time_utils().GeneralMLP
    arrays, worst = {}, 0.0
    for name, (kwargs, _, _) in make_golden.GENERAL_MLP_CASES.items():
        data = np.load(os.path.join(HERE, f"general_mlp_{name}.npz"))
        ref64 = run(GeneralMLP, kwargs, data, torch.float64, False)
        emul64 = run(GeneralMLP, kwargs, data, torch.float64, True)
        emul32 = run(GeneralMLP, kwargs, data, torch.float32, True)
        for t in ref64:
            e_fmt, e_32 = rel(emul64[t], ref64[t]), rel(emul32[t], emul64[t])
            arrays[f"{name}/e_fmt/{t}"], arrays[f"{name}/e_32/{t}"] = np.array(e_fmt), np.array(e_32)
            floor = FLOOR_OUT if t == "out" else FLOOR_GRAD
            if e_fmt >= 10 * floor:
                worst = max(worst, e_32 / e_fmt)
            if t.endswith(".matrix_t"):
                continue
            arrays[f"{name}/emul64/{t}"] = emul64[t].numpy().astype(np.float32 if t.endswith(".weight") else np.float64)
            if not t.startswith("grad:"):
                arrays[f"{name}/ref64/{t}"] = ref64[t].numpy().astype(np.float32)
            print(f"{name:12s} {t:28s} e_fmt {e_fmt:.3e}  e_32 {e_32:.3e}")
    rho = 4.0 * worst
    print("max e_32 / e_fmt =", worst, " rho =", rho)
    if not rho < 0.5:
        raise SystemExit("rho >= 0.5: float32 arithmetic is not small beside the format error on these cases")
    arrays["rho"] = np.array(rho)
    path = os.path.join(HERE, "mlp_bf16_cases.npz")
    np.savez_compressed(path, **arrays)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
