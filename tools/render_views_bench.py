"""What rendering the V views of a training step costs on an MI355X in its two forms: "loop", INTEGRATION.md's
`pkgs = [render(cam, ...) for cam in viewpoint_cam_list]` -> `training_objective` (one host wait per view, an autograd add per shared
input and view), against "views", `render_views` -> `training_objective` with the stacked tensors passed through (one host wait,
one sum launch).

    python tools/render_views_bench.py --out profiles/render_views_bench.json
        one process.  Two scenes from splatfields_amd.synthetic at 800 x 800: 100 k splats with precomputed colours and V = 5;
        300 k splats with SH of degree 3 and V = 10.  A step is: gradients cleared, the V renders, training_objective (L1 + D-SSIM,
        mask and depth L1 terms, so that all three outputs carry a gradient), one backward.  Both sides are warmed up, then five
        alternations loop / views.  The gain this change can have is on the host, so every window is timed by the WALL CLOCK of whole
        steps, fenced by a device synchronisation at both ends; the device time between two events over the same window, the
        launches per step (torch.profiler) and the host waits per step (sr_debug_counters) are reported beside it.
    python tools/render_views_bench.py --sides loop --out ...
        the loop alone: the form that also runs on a commit without render_views (the loop is code this change does not touch).

The exit status is 0 whichever side is faster.  Needs a HIP device; there is no CPU fallback."""
from __future__ import annotations

import argparse
import os
import sys
import time
import types

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

from tools import benchkit  # noqa: E402

LAMBDAS = dict(lambda_dssim=0.2, lambda_mask=0.1, lambda_depthl1=0.1)


def scene_steps(dev, n, n_views, size, use_sh, sides):
    from splatfields_amd import render
    from splatfields_amd.losses import training_objective
    from splatfields_amd.synthetic import make_camera, make_splats
    sp = make_splats(n, seed=21, device=dev)
    leaf = {k: sp[k].clone().requires_grad_(True) for k in ("means3D", "opacities", "scales", "rotations", "shs" if use_sh else "colors_precomp")}
    pack = {"means3D": leaf["means3D"], "active_sh_degree": 3 if use_sh else 0, "gaussian_opacity": leaf["opacities"],
            "gaussian_scales": leaf["scales"], "gaussian_rotations": leaf["rotations"]}
    pack["gaussian_features" if use_sh else "gaussian_rgb"] = leaf["shs" if use_sh else "colors_precomp"]
    cams = [make_camera(i, size, size, device=dev) for i in range(n_views)]
    g = torch.Generator().manual_seed(5)
    gt = torch.rand(n_views, 3, size, size, generator=g).to(dev)
    gt_mask = (torch.rand(n_views, 1, size, size, generator=g) > 0.5).float().to(dev)
    gt_depth = (torch.rand(n_views, 1, size, size, generator=g) * 4.0).to(dev)
    pipe, bg = types.SimpleNamespace(debug=False), torch.ones(3, device=dev)

    def clear():
        for t in leaf.values():
            t.grad = None

    def loop():
        clear()
        pkgs = [render(cam, pack, pipe, bg) for cam in cams]
        loss, _ = training_objective([p["render"] for p in pkgs], gt, opacities=[p["opacity"] for p in pkgs], gt_masks=gt_mask,
                                     depths=[p["depth"] for p in pkgs], gt_depths=gt_depth, **LAMBDAS)
        loss.backward()

    def views():
        from splatfields_amd import render_views
        clear()
        pkg = render_views(cams, pack, pipe, bg)
        loss, _ = training_objective(pkg["render"], gt, opacities=pkg["opacity"], gt_masks=gt_mask, depths=pkg["depth"], gt_depths=gt_depth,
                                     **LAMBDAS)
        loss.backward()

    return {name: fn for name, fn in (("loop", loop), ("views", views)) if name in sides}


def fenced_window(device_ms):
    """benchkit's window with the wall clock of the whole window as its figure -- synchronised before the first step and after the
    last --; the device time between two events over the same steps goes to device_ms[fn]"""
    def window(fn, iters):
        start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        start.record()
        for _ in range(iters):
            fn()
        end.record()
        torch.cuda.synchronize()
        wall = (time.perf_counter() - t0) * 1e3 / iters
        device_ms.setdefault(fn, []).append(start.elapsed_time(end) / iters)
        return wall
    return window


def host_waits_per_step(fn, steps=3):
    from splatfields_amd.rasterizer import host_sync_counters
    before = host_sync_counters()["forward_host_waits"]
    for _ in range(steps):
        fn()
    torch.cuda.synchronize()
    return (host_sync_counters()["forward_host_waits"] - before) / steps


def compare(fns, a):
    device_ms = {}
    doc, times = benchkit.alternate(fns, a.warmup, a.min_window, a.repeats, calibrate=3, digits=4, count_key="steps_per_window",
                                    window=fenced_window(device_ms))
    for name, fn in fns.items():
        doc[name] = {"wall_clock": doc[name],
                     "device": benchkit.window_stats(device_ms[fn][-a.repeats:], doc[name]["steps_per_window"], 4, "steps_per_window"),
                     "host_waits_per_step": host_waits_per_step(fn)}
    benchkit.with_launches(doc, fns, a.profiled_iterations, key="launches_per_step")
    if "loop" in fns and "views" in fns:
        doc["wall_clock_speedup_median"] = round(doc["loop"]["wall_clock"]["median_ms"] / doc["views"]["wall_clock"]["median_ms"], 3)
        doc["device_speedup_median"] = round(doc["loop"]["device"]["median_ms"] / doc["views"]["device"]["median_ms"], 3)
        doc["views_faster_in_every_alternation"] = all(v < l for l, v in zip(times["loop"], times["views"]))
    return doc


def main():
    p = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    p.add_argument("--out", default=None)
    p.add_argument("--sides", nargs="+", default=["loop", "views"], choices=["loop", "views"])
    p.add_argument("--size", type=int, default=800)
    p.add_argument("--repeats", type=int, default=5)
    p.add_argument("--warmup", type=int, default=10)
    p.add_argument("--min-window", type=float, default=0.5, help="seconds per timed window")
    p.add_argument("--profiled-iterations", type=int, default=2)
    a = p.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("render_views_bench needs a HIP device: there is no CPU fallback")
    dev = torch.device("cuda:0")
    from splatfields_amd.build import source_hash
    doc = {"device": torch.cuda.get_device_name(0), "torch": torch.__version__, "_source_hash": source_hash(), "lambdas": LAMBDAS,
           "workload": f"a step = gradients cleared + V renders at {a.size} x {a.size} + training_objective (L1 + D-SSIM, mask, depth L1) + one "
                       "backward; loop: [render(cam, ...) for cam in cams] with lists handed to training_objective; views: render_views with "
                       "the stacked tensors passed through",
           "protocol": f"one process; per scene both sides warmed up ({a.warmup} steps), then {a.repeats} alternations {' / '.join(a.sides)}; a "
                       f"window is >= {a.min_window} s of whole steps, wall clock between two device synchronisations (wall_clock) and device "
                       f"time between two events over the same steps (device); launches from torch.profiler ({a.profiled_iterations} steps per "
                       "side), host waits from sr_debug_counters (3 steps per side)",
           "scenes": {}}
    for name, n, v, use_sh in (("100k splats, precomputed colours, V = 5", 100_000, 5, False), ("300k splats, SH degree 3, V = 10", 300_000, 10, True)):
        doc["scenes"][name] = compare(scene_steps(dev, n, v, a.size, use_sh, a.sides), a)
        torch.cuda.empty_cache()
    benchkit.write_doc(doc, a.out)
    return 0


if __name__ == "__main__":
    sys.exit(main())
