"""What the fused tail of the objective (splatfields_amd/losses.py: splat_regularizers, depth_l1_loss, training_objective) buys on
an MI355X against the same expressions in PyTorch -- the reference's lines, which is what a user writes today.

    python tools/objective_bench.py --out profiles/objective_bench.json
        one process; per workload both sides warmed up, then five alternations pytorch / fused, every window timed with device
        events over at least --min-window seconds; then a few iterations of either side under torch.profiler for the launches
        per iteration.  Writes the JSON and prints it.  Exit status 1 unless the fused side is faster in EVERY alternation of
        every workload.

Workloads:
    splat_terms   lambda_norm, lambda_norm_mean and lambda_opacity together, forward + backward, N = 100 k, 300 k, 1 M
    depth_l1      train.py:224-229 on one 800x800 view, forward + backward
    objective     the whole objective of a step, V = 1 and V = 5 views of 800x800, N = 100 k, every term on: the literal per-view
                  loop of train.py:165-250 with this package's photometric_loss inside, against training_objective

Needs a HIP device; there is no CPU fallback."""
from __future__ import annotations

import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

from tools import benchkit  # noqa: E402
import torch.nn.functional as F  # noqa: E402

LAMBDAS = {"lambda_dssim": 0.2, "lambda_mask": 0.1, "lambda_norm": 0.01, "lambda_norm_mean": 0.01, "lambda_opacity": 0.01,
           "lambda_depthl1": 0.1}


def splat_steps(n, dev):
    from splatfields_amd.losses import splat_regularizers
    gen = torch.Generator().manual_seed(n)
    x = (torch.randn(n, 3, generator=gen) * 1.3).to(dev).requires_grad_(True)
    o = torch.rand(n, 1, generator=gen).to(dev).requires_grad_(True)
    lam_n, lam_nm, lam_o = LAMBDAS["lambda_norm"], LAMBDAS["lambda_norm_mean"], LAMBDAS["lambda_opacity"]

    def pytorch():
        x.grad = o.grad = None
        loss = lam_n * x.norm(dim=1).mean()                                               # train.py:195-197
        mean_val = x.detach().mean(dim=0, keepdim=True)                                   # train.py:198-201
        loss = loss + lam_nm * (x - mean_val).norm(dim=1).mean()
        loss = loss + lam_o * ((o - 1.0) ** 2).mean()                                     # train.py:244-246
        loss.backward()

    def fused():
        x.grad = o.grad = None
        splat_regularizers(x, o, lam_n, lam_nm, lam_o)[0].backward()

    return {"pytorch": pytorch, "fused": fused}


def depth_pair(height, width, seed, dev):
    gen = torch.Generator().manual_seed(seed)
    depth = torch.rand(1, height, width, generator=gen) * 4.0 + 0.5
    gt = torch.rand(1, height, width, generator=gen) * 4.0 + 0.5
    gt = torch.where(torch.rand(1, height, width, generator=gen) < 0.4, torch.zeros(()), gt)
    return depth.to(dev), gt.to(dev)


def reference_depth_l1(rnd_depth, gt_depth):
    _dmask = gt_depth > 0                                                                 # train.py:224-229
    return F.l1_loss((rnd_depth * _dmask).unsqueeze(-1), (gt_depth * _dmask).unsqueeze(-1))


def depth_steps(height, width, dev):
    from splatfields_amd.losses import depth_l1_loss
    depth, gt = depth_pair(height, width, 3, dev)
    depth.requires_grad_(True)

    def pytorch():
        depth.grad = None
        reference_depth_l1(depth.squeeze(), gt.squeeze()).backward()

    def fused():
        depth.grad = None
        depth_l1_loss(depth, gt).backward()

    return {"pytorch": pytorch, "fused": fused}


def objective_steps(n_views, n, height, width, dev):
    from splatfields_amd.losses import photometric_loss, training_objective
    from tests import loss_reference as R
    views = []
    for v in range(n_views):
        pred, target, opacity, mask = R.blob_scene(height, width, 1.0, seed=7 + v)
        depth, gt_depth = depth_pair(height, width, 20 + v, dev)
        views.append({"image": pred.to(dev).requires_grad_(True), "gt_image": target.to(dev), "opacity": opacity.to(dev).requires_grad_(True),
                      "gt_mask": mask.to(dev), "depth": depth.requires_grad_(True), "gt_depth": gt_depth})
    gen = torch.Generator().manual_seed(n)
    means3D = (torch.randn(n, 3, generator=gen) * 1.3).to(dev).requires_grad_(True)
    gaussian_opacity = torch.rand(n, 1, generator=gen).to(dev).requires_grad_(True)
    lam = LAMBDAS
    leaves = [means3D, gaussian_opacity] + [v[k] for v in views for k in ("image", "opacity", "depth")]

    def clear():
        for t in leaves:
            t.grad = None

    def pytorch():      # the loop of train.py:165-250, photometric_loss for :183-193
        clear()
        loss_list = []
        for view in views:
            _loss, _Ll1 = photometric_loss(view["image"], view["gt_image"], lam["lambda_dssim"], view["opacity"], view["gt_mask"], lam["lambda_mask"])
            _loss = _loss + lam["lambda_norm"] * means3D.norm(dim=1).mean()
            mean_val = means3D.detach().mean(dim=0, keepdim=True)
            _loss = _loss + lam["lambda_norm_mean"] * (means3D - mean_val).norm(dim=1).mean()
            _loss = _loss + lam["lambda_depthl1"] * reference_depth_l1(view["depth"].squeeze(), view["gt_depth"].squeeze())
            loss_list.append(_loss)
        loss = sum(loss_list) / len(loss_list)
        loss = loss + lam["lambda_opacity"] * ((gaussian_opacity - 1.0) ** 2).mean()
        loss.backward()

    keys = ("image", "gt_image", "opacity", "gt_mask", "depth", "gt_depth")
    lists = {k: [v[k] for v in views] for k in keys}

    def fused():
        clear()
        loss, _ = training_objective(lists["image"], lists["gt_image"], opacities=lists["opacity"], gt_masks=lists["gt_mask"],
                                     depths=lists["depth"], gt_depths=lists["gt_depth"], means3D=means3D,
                                     gaussian_opacity=gaussian_opacity, **lam)
        loss.backward()

    return {"pytorch": pytorch, "fused": fused}


def alternate(steps, warmup, min_window_s, repeats, profiled):
    """Both sides warmed up, then `repeats` alternations; every window lasts at least `min_window_s`."""
    out, times = benchkit.alternate(steps, warmup, min_window_s, repeats, calibrate=5, digits=5)
    p, f = out["pytorch"], out["fused"]
    out["speedup_median"] = round(p["median_ms"] / f["median_ms"], 3)
    out["saved_ms_median"] = round(p["median_ms"] - f["median_ms"], 5)
    out["fused_faster_in_every_alternation"] = all(b < a for a, b in zip(times["pytorch"], times["fused"]))
    return benchkit.with_launches(out, steps, profiled)


def main():
    p = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    p.add_argument("--out", default=None)
    p.add_argument("--height", type=int, default=800)
    p.add_argument("--width", type=int, default=800)
    p.add_argument("--splats", type=int, nargs="+", default=[100_000, 300_000, 1_000_000])
    p.add_argument("--views", type=int, nargs="+", default=[1, 5])
    p.add_argument("--objective-splats", type=int, default=100_000)
    p.add_argument("--repeats", type=int, default=5)
    p.add_argument("--warmup", type=int, default=20)
    p.add_argument("--min-window", type=float, default=0.5, help="seconds per timed window")
    p.add_argument("--profiled-iterations", type=int, default=5, help="iterations under torch.profiler per side (0: launches not measured)")
    a = p.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("objective_bench needs a HIP device: there is no CPU fallback")
    dev = torch.device("cuda:0")
    import gc
    from splatfields_amd.build import source_hash
    gc.collect()
    gc.disable()
    run = lambda steps: alternate(steps, a.warmup, a.min_window, a.repeats, a.profiled_iterations)
    doc = {"device": torch.cuda.get_device_name(0), "torch": torch.__version__, "_source_hash": source_hash(), "lambdas": LAMBDAS,
           "protocol": f"one process; per workload both sides warmed up ({a.warmup} iterations), then {a.repeats} alternations pytorch / "
                       f"fused, windows >= {a.min_window} s between device events; launches per iteration from torch.profiler "
                       f"({a.profiled_iterations} iterations per side, after the timed windows)",
           "splat_terms": {}, "objective": {}}
    for n in a.splats:
        doc["splat_terms"][str(n)] = run(splat_steps(n, dev))
        print(json.dumps({"splat_terms": n, **doc["splat_terms"][str(n)]}), flush=True)
    doc["depth_l1"] = dict(shape=[1, a.height, a.width], **run(depth_steps(a.height, a.width, dev)))
    print(json.dumps({"depth_l1": doc["depth_l1"]}), flush=True)
    for v in a.views:
        doc["objective"][str(v)] = dict(views=v, splats=a.objective_splats, shape=[3, a.height, a.width],
                                        **run(objective_steps(v, a.objective_splats, a.height, a.width, dev)))
        print(json.dumps({"objective": doc["objective"][str(v)]}), flush=True)
    workloads = list(doc["splat_terms"].values()) + [doc["depth_l1"]] + list(doc["objective"].values())
    doc["fused_faster_in_every_alternation_of_every_workload"] = all(w["fused_faster_in_every_alternation"] for w in workloads)
    benchkit.write_doc(doc, a.out)
    return 0 if doc["fused_faster_in_every_alternation_of_every_workload"] else 1


if __name__ == "__main__":
    sys.exit(main())
