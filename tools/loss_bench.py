"""What the fused photometric loss (splatfields_amd/losses.py) buys on an MI355X, against the PyTorch restatement of the
reference's loss (tests/loss_reference.py -- what a user of the rasterizer alone runs between render() and backward()).

    python tools/loss_bench.py --out profiles/loss_bench.json
        loss alone (800x800x3 with the mask term, forward + backward) and the whole view step (render() + loss + backward() at
        1 M splats, 800x800, SH 3), each: both sides warmed up, then five alternations restated / fused, every window timed
        with device events over at least 0.5 s.  Writes the JSON and prints it.
    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -o r -- python tools/loss_bench.py --trace fused|restated
        a run of its own for the profiler: --iters iterations of the loss alone, nothing else.
    python tools/loss_bench.py --merge fused=DIR restated=DIR --out profiles/loss_bench.json
        adds launches per iteration and kernel times from the two traces, and the two kernels' algorithmic bytes over their
        kernel time as a share of the HBM peak.

Needs a HIP device; there is no CPU fallback."""
from __future__ import annotations

import argparse
import json
import os
import sys
import types

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

from tools import benchkit  # noqa: E402

HBM_PEAK = 8.0e12        # bytes / s (specification)
FP32_PEAK = 157.3e12     # vector FLOP / s (specification)
LAMBDA_DSSIM, LAMBDA_MASK = 0.2, 0.1


def loss_inputs(height, width, dev):
    from tests import loss_reference as R
    pred, target, opacity, mask = R.blob_scene(height, width, 1.0, seed=7)
    return pred.to(dev), target.to(dev), opacity.to(dev), mask.to(dev)


def loss_alone_steps(height, width, dev):
    """-> {"restated": fn, "fused": fn}: one forward + backward of the loss each"""
    from splatfields_amd.losses import photometric_loss
    from tests import loss_reference as R
    pred, target, opacity, mask = loss_inputs(height, width, dev)
    x = pred.clone().requires_grad_(True)
    a = opacity.clone().requires_grad_(True)

    def restated():
        x.grad = a.grad = None
        R.photometric(x, target, LAMBDA_DSSIM, a, mask, LAMBDA_MASK)[0].backward()

    def fused():
        x.grad = a.grad = None
        photometric_loss(x, target, LAMBDA_DSSIM, a, mask, LAMBDA_MASK)[0].backward()

    return {"restated": restated, "fused": fused}


def view_steps(n, height, width, sh_degree, dev):
    """-> {"restated": fn, "fused": fn}: render() + loss + backward() of one view of the headline workload"""
    from splatfields_amd import render
    from splatfields_amd.losses import photometric_loss
    from splatfields_amd.synthetic import make_camera, make_splats
    from tests import loss_reference as R
    sp = make_splats(n, seed=1234, device=dev)
    pipe = types.SimpleNamespace(debug=False)
    bg = torch.ones(3, device=dev)
    cams = [make_camera(k, width, height, device=dev) for k in range(4)]
    names = ["means3D", "scales", "rotations", "opacities", "shs"]
    params = {k: sp[k].clone().requires_grad_(True) for k in names}
    pack = lambda p: {"means3D": p["means3D"], "active_sh_degree": sh_degree, "gaussian_opacity": p["opacities"],
                      "gaussian_features": p["shs"], "gaussian_scales": p["scales"], "gaussian_rotations": p["rotations"]}
    targets = []
    with torch.no_grad():   # targets: the same splats with other colours
        other = dict(sp, shs=sp["shs"] * 0.8 + 0.05)
        for cam in cams:
            t = render(cam, pack(other), pipe, bg)
            targets.append((t["render"].clone(), (t["opacity"] > 0.5).float()))
    count = [0]

    def step(loss_fn):
        i = count[0] % len(cams)
        count[0] += 1
        for p in params.values():
            p.grad = None
        pkg = render(cams[i], pack(params), pipe, bg)
        loss_fn(pkg["render"], targets[i][0], pkg["opacity"], targets[i][1]).backward()

    restated = lambda: step(lambda im, gt, op, m: R.photometric(im, gt, LAMBDA_DSSIM, op, m, LAMBDA_MASK)[0])
    fused = lambda: step(lambda im, gt, op, m: photometric_loss(im, gt, LAMBDA_DSSIM, op, m, LAMBDA_MASK)[0])
    return {"restated": restated, "fused": fused}


def alternate(steps, warmup, min_window_s, repeats):
    """Both sides warmed up, then `repeats` alternations; every window lasts at least `min_window_s`."""
    out = benchkit.alternate(steps, warmup, min_window_s, repeats, calibrate=5, digits=5)[0]
    r, f = out["restated"], out["fused"]
    out["speedup_median"] = round(r["median_ms"] / f["median_ms"], 3)
    out["saved_ms_median"] = round(r["median_ms"] - f["median_ms"], 5)
    out["fused_faster_in_every_repetition"] = f["max_ms"] < r["min_ms"]     # worst fused < best restated
    return out


def algorithmic_bytes(channels, height, width):
    """Bytes each kernel must move once, from the shapes (the derivative maps are stored by the forward and read by the backward)."""
    plane = 4 * height * width
    fwd = {"read": 2 * channels * plane + 2 * plane, "write": 3 * channels * plane}
    bwd = {"read": (3 + 2) * channels * plane + 2 * plane, "write": channels * plane + plane}
    # separable 11-tap filters: rows over tile + halo (42 / 32), then columns; 2 FLOP per tap
    px = channels * height * width
    flops = {"forward": px * (5 * 11 * 2 * (42 / 32 + 1) + 40), "backward": px * (3 * 11 * 2 * (42 / 32 + 1) + 10)}
    return {"forward": fwd, "backward": bwd, "flops": flops}


def merge(pairs, out_path, iters_total):
    doc = json.load(open(out_path))
    shape = doc["loss_alone"]["shape"]
    traces = {}
    for item in pairs:
        name, directory = item.split("=", 1)
        rows = benchkit.read_stats(directory)
        traces[name] = {"launches_per_iteration": round(sum(c for _, c, _, _ in rows) / iters_total, 2),
                        "kernel_us_per_iteration": round(sum(t for _, _, _, t in rows) / iters_total / 1e3, 3),
                        "distinct_kernels": len(rows), "iterations_traced": iters_total}
        if name == "fused":
            by = algorithmic_bytes(shape[0], shape[1], shape[2])
            kernels = {}
            for key, label in (("k_loss_forward", "forward"), ("k_loss_backward", "backward"), ("k_loss_reduce", "reduce")):
                hit = [r for r in rows if key in r[0]]
                if not hit:
                    continue
                us = hit[0][2] / 1e3
                entry = {"average_us": round(us, 3), "calls": hit[0][1]}
                if label in by:
                    b = by[label]["read"] + by[label]["write"]
                    t_mem, t_alu = b / HBM_PEAK, by["flops"][label] / FP32_PEAK
                    entry.update(algorithmic_bytes=b, bytes_per_s=round(b / (us * 1e-6), 1),
                                 share_of_hbm_peak=round(b / HBM_PEAK / (us * 1e-6), 4),
                                 least_time_us=round(max(t_mem, t_alu) * 1e6, 3), bound="memory" if t_mem >= t_alu else "compute",
                                 share_of_peak=round(max(t_mem, t_alu) / (us * 1e-6), 4))
                kernels[label] = entry
            traces[name]["kernels"] = kernels
    doc["kernel_trace"] = traces
    benchkit.write_doc(doc, out_path)


def main():
    p = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    p.add_argument("--out", default=None)
    p.add_argument("--height", type=int, default=800)
    p.add_argument("--width", type=int, default=800)
    p.add_argument("--splats", type=int, default=1_000_000)
    p.add_argument("--sh-degree", type=int, default=3)
    p.add_argument("--repeats", type=int, default=5)
    p.add_argument("--min-window", type=float, default=0.5, help="seconds per timed window")
    p.add_argument("--skip-view-step", action="store_true")
    p.add_argument("--trace", choices=["fused", "restated"], default=None)
    p.add_argument("--iters", type=int, default=50)
    p.add_argument("--merge", nargs="+", default=None, metavar="NAME=DIR")
    a = p.parse_args()
    if a.merge:
        return merge(a.merge, a.out, a.iters)
    if not torch.cuda.is_available():
        raise SystemExit("loss_bench needs a HIP device: there is no CPU fallback")
    dev = torch.device("cuda:0")
    if a.trace:
        fn = loss_alone_steps(a.height, a.width, dev)[a.trace]
        for _ in range(a.iters):
            fn()
        torch.cuda.synchronize()
        return
    import gc
    gc.collect()
    gc.disable()
    doc = {"device": torch.cuda.get_device_name(0), "protocol": f"device events, windows >= {a.min_window} s, {a.repeats} alternations "
           "restated / fused in one process after warming up both", "lambda_dssim": LAMBDA_DSSIM, "lambda_mask": LAMBDA_MASK}
    doc["loss_alone"] = dict(shape=[3, a.height, a.width], mask_term=True,
                             **alternate(loss_alone_steps(a.height, a.width, dev), 20, a.min_window, a.repeats))
    print(json.dumps(doc["loss_alone"]), flush=True)
    if not a.skip_view_step:
        doc["view_step"] = dict(splats=a.splats, shape=[3, a.height, a.width], sh_degree=a.sh_degree,
                                **alternate(view_steps(a.splats, a.height, a.width, a.sh_degree, dev), 10, a.min_window, a.repeats))
    doc["algorithmic_bytes"] = algorithmic_bytes(3, a.height, a.width)
    benchkit.write_doc(doc, a.out)


if __name__ == "__main__":
    main()
