"""What the view-dependent colour head costs on an MI355X on its two paths: "torch" (PyTorch ops, per view: the default) against
"fused" (csrc/view_color.hip, every view of a step in one launch).

    python tools/view_color_bench.py --out profiles/view_color_bench.json
        one process.  (a) The head alone: N = 100 k and 300 k points, F = 128, V = 1, 5 and 10 views, forward + backward of
        sum(colours . probe) through `ViewColor.for_cameras` with gradients for feature, means3D, weight and bias.  (b) The whole
        view-dependent step: SplatFields(use_view_dep_rgb=True) on 100 k points, then V = 10 x (render() at 800 x 800 + L1 loss),
        one backward -- the torch side hands `rgb_fnc` to every render() as the reference does, the fused side evaluates one
        `for_cameras` call and hands `rgbs[i]` to each render().  In each comparison both sides are warmed up, then five
        alternations torch / fused, every window timed with device events over at least --min-window seconds; then a few
        iterations of either side under torch.profiler for the launches per iteration, and the library's own count
        (sr_profile_collect).  Writes the JSON and prints it.  The "torch" side is the baseline; the exit status is 0 whichever
        side is faster (the fused path is opt-in).

Needs a HIP device; there is no CPU fallback."""
from __future__ import annotations

import argparse
import os
import sys
import types

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

from tools import benchkit  # noqa: E402


def head_steps(dev, n, width, n_views, seed=5):
    from splatfields_amd.deform_field import ViewColor
    torch.manual_seed(seed)
    head = torch.nn.Sequential(torch.nn.Linear(width + 3, 3), torch.nn.Sigmoid()).to(dev)
    params = list(head.parameters())
    feature = torch.randn(n, width, device=dev).requires_grad_(True)
    means3D = (torch.rand(n, 3, device=dev) * 2 - 1).requires_grad_(True)
    centres = torch.nn.functional.normalize(torch.randn(n_views, 3, device=dev), dim=-1) * 4.0
    probe = torch.randn(n_views, n, 3, device=dev)

    def step(path):
        def fn():
            for p in params:
                p.grad = None
            feature.grad, means3D.grad = None, None
            (ViewColor(head, feature, path).for_cameras(means3D, centres) * probe).sum().backward()
        return fn

    return {"torch": step("torch"), "fused": step("fused")}


def network_steps(dev, n, n_views, size, seed=0):
    from splatfields_amd import render
    from splatfields_amd.deform_field import SplatFields
    from splatfields_amd.synthetic import make_camera, make_splats
    sp = make_splats(n, seed=21, device=dev)
    xyz = sp["means3D"].clone().requires_grad_(True)
    t_emb = torch.zeros(n, 1, device=dev)
    cams = [make_camera(i, size, size, device=dev) for i in range(n_views)]
    centres = torch.stack([c.camera_center for c in cams])
    targets = [torch.rand(3, size, size, device=dev) for _ in range(n_views)]
    pipe, bg = types.SimpleNamespace(debug=False), torch.ones(3, device=dev)
    nets = {}
    for path in ("torch", "fused"):
        torch.manual_seed(seed)
        nets[path] = SplatFields(n_frames=0, use_view_dep_rgb=True, view_color=path).to(dev)
    nets["fused"].load_state_dict(nets["torch"].state_dict())

    def step(path):
        net = nets[path]
        params = list(net.parameters())

        def fn():
            for p in params:
                p.grad = None
            xyz.grad = None
            out = net(xyz, t_emb)
            pack = {"means3D": out["means3D"], "active_sh_degree": 0, "gaussian_opacity": out["opacity"],
                    "gaussian_scales": sp["scales"] + 0.01 * out["scales"], "gaussian_rotations": out["rotations"]}
            if path == "fused":      # one launch for all views, then a slice per render()
                rgbs = out["rgb_fnc"].for_cameras(out["means3D"], centres)
                colour = lambda i: {"gaussian_rgb": rgbs[i]}
            else:                    # the reference's loop: render() evaluates rgb_fnc per view
                colour = lambda i: {"gaussian_rgb_fnc": out["rgb_fnc"]}
            loss = 0.0
            for i, cam in enumerate(cams):
                image = render(cam, dict(pack, **colour(i)), pipe, bg)["render"]
                loss = loss + (image - targets[i]).abs().mean()
            loss.backward()
        return fn

    return {"torch": step("torch"), "fused": step("fused")}


def main():
    p = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    p.add_argument("--out", default=None)
    p.add_argument("--points", type=int, nargs="+", default=[100_000, 300_000])
    p.add_argument("--views", type=int, nargs="+", default=[1, 5, 10])
    p.add_argument("--width", type=int, default=128)
    p.add_argument("--step-points", type=int, default=100_000)
    p.add_argument("--step-views", type=int, default=10)
    p.add_argument("--step-size", type=int, default=800)
    p.add_argument("--repeats", type=int, default=5)
    p.add_argument("--warmup", type=int, default=10)
    p.add_argument("--min-window", type=float, default=0.3, help="seconds per timed window")
    p.add_argument("--profiled-iterations", type=int, default=3)
    a = p.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("view_color_bench needs a HIP device: there is no CPU fallback")
    dev = torch.device("cuda:0")
    from splatfields_amd.build import source_hash
    from splatfields_amd.view_color import VIEW_COLOR_LAUNCHES
    doc = {"device": torch.cuda.get_device_name(0), "torch": torch.__version__, "_source_hash": source_hash(),
           "workload": f"head alone: N in {a.points}, F = {a.width}, V in {a.views}, forward + backward of sum(colours . probe) through "
                       "ViewColor.for_cameras, gradients for feature, means3D, weight and bias; view-dependent step: SplatFields(use_view_dep_rgb) on "
                       f"{a.step_points} points + {a.step_views} x (render() at {a.step_size} x {a.step_size} + L1) + one backward",
           "protocol": f"one process; per comparison both sides warmed up ({a.warmup} iterations), then {a.repeats} alternations torch / fused, windows "
                       f">= {a.min_window} s between device events; launches from torch.profiler ({a.profiled_iterations} iterations per side) and from "
                       "sr_profile_collect (one iteration); 'torch' is the default path and the baseline",
           "view_color_launches": list(VIEW_COLOR_LAUNCHES), "head": {}}
    for n in a.points:
        for v in a.views:
            doc["head"][f"N={n} V={v}"] = benchkit.compare(head_steps(dev, n, a.width, v), a)
    doc["view_dependent_step"] = benchkit.compare(network_steps(dev, a.step_points, a.step_views, a.step_size), a)
    benchkit.write_doc(doc, a.out)
    return 0


if __name__ == "__main__":
    sys.exit(main())
