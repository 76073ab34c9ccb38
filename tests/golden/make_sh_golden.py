"""Writes tests/golden/sh_cases.npz: the reference's own SH colours -- `eval_sh` (utils/sh_utils.py:57-112) + 0.5 + clamp,
called as extract_geo.py:40-44 calls it -- for degrees 0..3 on 64 splats and 2 cameras, evaluated in float64 AND in float32,
with the autograd gradients w.r.t. the coefficients and the positions.  Run on a CPU where a reference checkout exists:

    python tests/golden/make_sh_golden.py /path/to/reference

Numeric arrays only travel:
    means [N,3], shs [N,16,3], campos [V,3], probe [V,N,3]                float32 inputs (probe = dL/dcolour)
    deg<d>/f64|f32/{colors [V,N,3], d_shs [N,16,3], d_means [N,3]}        d_* of sum_v (colors_v * probe_v).sum()
The float32 evaluation is the reference's own rounding error: the tolerance of the HIP kernels on these cases is derived from
its distance to the float64 one (tests/test_gpu_sh_edges.py).

Checked here: no pre-clamp channel lies within 1e-4 of zero (the clamp decision is the same in every float format), between a
fifth and a half of the channels clamp at every degree, and at degree 3 at least one splat clamps a channel in one view and
not in the other."""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
N, V, K = 64, 2, 16


def inputs():
    g = torch.Generator().manual_seed(2024)
    means = torch.rand(N, 3, generator=g) * 2.0 - 1.0
    shs = torch.randn(N, K, 3, generator=g)
    shs[:, 0] *= 3.0                      # the clamp at 0 bites
    shs[:, 1:] *= 0.8                     # ... and depends on the view
    campos = torch.tensor([[3.0, 0.5, 1.5], [-1.0, 2.5, -2.0]])
    probe = torch.randn(V, N, 3, generator=g)
    return means, shs, campos, probe


def reference_eval(eval_sh, means, shs, campos, probe, deg, dtype):
    m = means.to(dtype).clone().requires_grad_(True)
    s = shs.to(dtype).clone().requires_grad_(True)
    colors, pres = [], []
    for v in range(V):
        # what extract_geo.py:40-44 hands to eval_sh: coefficients channel-major [N,3,K], unit directions camera -> splat
        direction = m - campos[v].to(dtype)[None, :]
        direction = direction / direction.norm(dim=1, keepdim=True)
        pre = eval_sh(deg, s.permute(0, 2, 1), direction) + 0.5
        pres.append(pre)
        colors.append(pre.clamp_min(0.0))
    colors = torch.stack(colors)
    (colors * probe.to(dtype)).sum().backward()
    out = {"colors": colors, "d_shs": s.grad, "d_means": m.grad if m.grad is not None else torch.zeros_like(m)}
    return {k: t.detach().numpy().copy() for k, t in out.items()}, torch.stack(pres).detach()


def main():
    if len(sys.argv) != 2:
        sys.exit(__doc__)
    sys.path.insert(0, sys.argv[1])
    from utils.sh_utils import eval_sh
    torch.set_num_threads(1)
    means, shs, campos, probe = inputs()
    arrays = {"means": means.numpy(), "shs": shs.numpy(), "campos": campos.numpy(), "probe": probe.numpy()}
    for deg in range(4):
        for tag, dtype in (("f64", torch.float64), ("f32", torch.float32)):
            res, pre = reference_eval(eval_sh, means, shs, campos, probe, deg, dtype)
            for key, val in res.items():
                arrays[f"deg{deg}/{tag}/{key}"] = val
            if tag == "f64":
                share = (pre < 0).double().mean().item()
                split = ((pre[0] < 0) != (pre[1] < 0)).any(1).sum().item()
                print(f"degree {deg}: {share:.1%} of the channels clamp, closest to zero {pre.abs().min().item():.2e}, "
                      f"{split} splats clamp in one view only")
                assert pre.abs().min() > 1e-4 and 0.2 <= share <= 0.5 and (deg < 3 or split > 0)
    path = os.path.join(HERE, "sh_cases.npz")
    np.savez_compressed(path, **arrays)
    print(path, os.path.getsize(path), "bytes,", len(arrays), "arrays")


if __name__ == "__main__":
    main()
