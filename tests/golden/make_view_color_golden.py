"""Records what the reference computes for the view-dependent colours of V = 3 views of one step: its own
`SplatFields(use_view_dep_rgb=True)` (utils/time_utils.py:305-508) at the small configuration of make_golden.py's
"static_viewdep" case, N = 32 points, its `rgb_fnc` taken from the forward and evaluated per view with the expressions of its
`render()` (gaussian_renderer/__init__.py:44-46) on the network's own means3D.

  view_color_cases.npz   param:<key> (float32: the master values of both precisions), xyz [N, 3], t [N, 1], centres [V, 3]
                         (radius >= 3; the points lie in [-1, 1]^3), probes [V, N, 3], and per precision p in (f32, f64):
                         p/colours [V, N, 3], p/means3D, p/grad_xyz, p/grad:<key>  of  sum_v (probe_v . colour_v).sum()

Run where the reference checkout exists:  python tests/golden/make_view_color_golden.py /path/to/reference
The float64 evaluation runs under torch.set_default_dtype(torch.float64), with the float32 master values converted."""
import contextlib
import io
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
N, V = 32, 3


def evaluate(SplatFields, n_frames, kwargs, state, xyz, t, centres, probes, dtype):
    prev = torch.get_default_dtype()
    torch.set_default_dtype(dtype)
    try:
        with contextlib.redirect_stdout(io.StringIO()):            # the constructor prints the module
            net = SplatFields(radius=None, n_frames=n_frames, **kwargs)
        net.load_state_dict({k: v.to(dtype) for k, v in state.items()}, strict=True)
        pts = xyz.detach().to(dtype).clone().requires_grad_()
        out = net(pts, t.to(dtype))
        means3D, rgb_fnc = out["means3D"], out["rgb_fnc"]
        colours = []
        for centre in centres.to(dtype):
            ray_d = means3D - centre[None]
            ray_d = ray_d / torch.norm(ray_d, dim=-1, keepdim=True)
            colours.append(rgb_fnc(ray_d))
        sum((p * c).sum() for p, c in zip(probes.to(dtype), colours)).backward()
        res = {"colours": torch.stack(colours).detach(), "means3D": means3D.detach(), "grad_xyz": pts.grad}
        for k, p in net.named_parameters():
            res["grad:" + k] = p.grad if p.grad is not None else torch.zeros_like(p)
        return {k: v.numpy() for k, v in res.items()}
    finally:
        torch.set_default_dtype(prev)


def main(ref):
    from make_flow_head_golden import import_time_utils
    from make_golden import SPLATFIELDS_CASES
    SplatFields = import_time_utils(ref).SplatFields
    n_frames, kwargs, tval = SPLATFIELDS_CASES["static_viewdep"]
    torch.manual_seed(1900)
    with contextlib.redirect_stdout(io.StringIO()):
        net = SplatFields(radius=None, n_frames=n_frames, **kwargs)
    state = {k: v.detach().clone().float() for k, v in net.state_dict().items()}
    xyz = torch.rand(N, 3) * 2 - 1
    t = torch.full((N, 1), tval)
    centres = torch.nn.functional.normalize(torch.randn(V, 3), dim=-1) * (3.0 + torch.rand(V, 1))
    probes = torch.randn(V, N, 3)
    data = {"xyz": xyz.numpy(), "t": t.numpy(), "centres": centres.numpy(), "probes": probes.numpy()}
    for k, v in state.items():
        data["param:" + k] = v.numpy()
    for tag, dtype in (("f32", torch.float32), ("f64", torch.float64)):
        for k, v in evaluate(SplatFields, n_frames, kwargs, state, xyz, t, centres, probes, dtype).items():
            data[f"{tag}/{k}"] = v
    assert all(v.dtype in (np.float32, np.float64) for v in data.values())
    np.savez_compressed(os.path.join(HERE, "view_color_cases.npz"), **data)
    print("wrote", len(data), "arrays,", sum(v.size for v in data.values()), "values")


if __name__ == "__main__":
    main(sys.argv[1])
