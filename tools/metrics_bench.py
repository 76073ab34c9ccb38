"""What the fused evaluation metrics (splatfields_amd/metrics.py) buy on an MI355X, against the same formulas in plain PyTorch
(tests/metric_reference.py: the quantisation, `F.conv2d` valid filters and the partial-convolution normalisation) on the
device -- what a user could write without the kernel -- and on the CPU, where the reference evaluates.

    python tools/metrics_bench.py --out profiles/metrics_bench.json
        800x800x3 with quantize="png", batch 1 and 8, without and with a mask.  Device sides: both warmed up, then five
        alternations restated / fused, every window timed with device events over at least 0.5 s.  CPU side: the restatement in
        float32 under a host clock, best of --cpu-repeats runs.  Writes the JSON and prints it.
    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -o r -- python tools/metrics_bench.py --trace fused|restated
        a run of its own for the profiler: --iters calls at batch --trace-batch with a mask, nothing else.
    python tools/metrics_bench.py --merge fused=DIR restated=DIR --out profiles/metrics_bench.json
        adds launches per call and kernel times from the two traces, and the kernel's least time from the shapes.

Needs a HIP device; there is no CPU fallback for the fused side."""
from __future__ import annotations

import argparse
import json
import math
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

from tools import benchkit  # noqa: E402

HBM_PEAK = 8.0e12        # bytes / s (specification)
FP32_PEAK = 157.3e12     # vector FLOP / s (specification)
QUANTIZE = "png"


def inputs(batch, height, width, dev):
    """`batch` different views: (pred [B,3,H,W], gt, mask [B,H,W]) on `dev`"""
    from tests import metric_reference as R
    items = [R.textured_pair(height, width, seed=7 + i) for i in range(batch)]
    return tuple(torch.stack([it[k] for it in items]).to(dev) for k in range(3))


def restated_metrics(pred, gt, mask):
    """The same numbers from the restatement's pieces, on the tensors' device, without a host wait."""
    from tests import metric_reference as R
    x, y = R.quantize(pred, QUANTIZE), R.quantize(gt, QUANTIZE)
    b = x.shape[0]
    se = ((x - y) ** 2).reshape(b, 3, -1)
    m = None if mask is None else mask[:, None]
    return {"psnr": -10.0 / math.log(10) * torch.log(se.reshape(b, -1).mean(dim=1)),
            "psnr_channels": 20 * torch.log10(1.0 / torch.sqrt(se.mean(dim=2))),
            "ssim": R.ssim_map(x, y, m).reshape(b, -1).mean(dim=1)}


def device_steps(batch, height, width, masked, dev):
    from splatfields_amd.metrics import image_metrics
    pred, gt, mask = inputs(batch, height, width, dev)
    mask = mask if masked else None
    return {"restated": lambda: restated_metrics(pred, gt, mask),
            "fused": lambda: image_metrics(pred, gt, mask, quantize=QUANTIZE)}


def alternate(steps, warmup, min_window_s, repeats):
    """Both sides warmed up, then `repeats` alternations; every window lasts at least `min_window_s`."""
    out = benchkit.alternate(steps, warmup, min_window_s, repeats, calibrate=5, digits=5)[0]
    r, f = out["restated"], out["fused"]
    out["speedup_median"] = round(r["median_ms"] / f["median_ms"], 3)
    out["fused_faster_in_every_repetition"] = f["max_ms"] < r["min_ms"]     # worst fused < best restated
    return out


def cpu_ms(batch, height, width, masked, repeats):
    """The restatement in float32 on the CPU, all host threads: best of `repeats` after one warm-up, host clock."""
    pred, gt, mask = inputs(batch, height, width, "cpu")
    mask = mask if masked else None
    restated_metrics(pred, gt, mask)
    ts = []
    for _ in range(repeats):
        t0 = time.perf_counter()
        restated_metrics(pred, gt, mask)
        ts.append((time.perf_counter() - t0) * 1e3)
    return {"ms": [round(t, 3) for t in ts], "min_ms": round(min(ts), 3), "threads": torch.get_num_threads(), "dtype": "float32"}


def agreement(steps):
    """largest |difference| of the two device sides' results, per metric (both float32)"""
    a, b = steps["restated"](), steps["fused"]()
    return {k: float((a[k].double() - b[k].double()).abs().max()) for k in a}


def algorithmic(batch, height, width, masked):
    """What the kernel must move and compute once, from the shapes."""
    px = batch * 3 * height * width
    read = 2 * 4 * px + (4 * batch * height * width if masked else 0)
    # separable 11-tap filters of five quantities: rows over the 42-row region of a 32-row tile, then columns; 2 FLOP per tap;
    # about 60 more per output for the products, the similarity and the squared error
    flops = px * (5 * 11 * 2 * (42 / 32 + 1) + 60)
    t_mem, t_alu = read / HBM_PEAK, flops / FP32_PEAK
    return {"read_bytes": read, "flops": round(flops), "least_time_us": round(max(t_mem, t_alu) * 1e6, 3),
            "bound": "memory" if t_mem >= t_alu else "compute"}


def merge(pairs, out_path, iters_total, batch, height, width):
    doc = json.load(open(out_path))
    traces = {"batch": batch, "masked": True, "quantize": QUANTIZE}
    for item in pairs:
        name, directory = item.split("=", 1)
        rows = benchkit.read_stats(directory)
        traces[name] = {"launches_per_call": round(sum(c for _, c, _, _ in rows) / iters_total, 2),
                        "kernel_us_per_call": round(sum(t for _, _, _, t in rows) / iters_total / 1e3, 3),
                        "distinct_kernels": len(rows), "calls_traced": iters_total}
        if name == "fused":
            alg = algorithmic(batch, height, width, True)
            kernels = {}
            for key, label in (("k_metrics_reduce", "reduce"), ("k_metrics", "metrics")):
                hit = [r for r in rows if key in r[0] and not (label == "metrics" and "reduce" in r[0])]
                if not hit:
                    continue
                us = hit[0][2] / 1e3
                kernels[label] = {"average_us": round(us, 3), "calls": hit[0][1]}
                if label == "metrics":
                    kernels[label].update(alg, share_of_peak=round(alg["least_time_us"] / us, 4))
            traces[name]["kernels"] = kernels
    doc["kernel_trace"] = traces
    benchkit.write_doc(doc, out_path)


def main():
    p = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    p.add_argument("--out", default=None)
    p.add_argument("--height", type=int, default=800)
    p.add_argument("--width", type=int, default=800)
    p.add_argument("--batches", type=int, nargs="+", default=[1, 8])
    p.add_argument("--repeats", type=int, default=5)
    p.add_argument("--min-window", type=float, default=0.5, help="seconds per timed window")
    p.add_argument("--cpu-repeats", type=int, default=3, help="0: skip the CPU side")
    p.add_argument("--trace", choices=["fused", "restated"], default=None)
    p.add_argument("--trace-batch", type=int, default=8)
    p.add_argument("--iters", type=int, default=50)
    p.add_argument("--merge", nargs="+", default=None, metavar="NAME=DIR")
    a = p.parse_args()
    if a.merge:
        if not a.out:
            p.error("--merge adds to the JSON of an earlier run: --out is required")
        return merge(a.merge, a.out, a.iters, a.trace_batch, a.height, a.width)
    if not torch.cuda.is_available():
        raise SystemExit("metrics_bench needs a HIP device: there is no CPU fallback")
    dev = torch.device("cuda:0")
    if a.trace:
        fn = device_steps(a.trace_batch, a.height, a.width, True, dev)[a.trace]
        for _ in range(a.iters):
            fn()
        torch.cuda.synchronize()
        return
    import gc
    gc.collect()
    gc.disable()
    doc = {"device": torch.cuda.get_device_name(0), "shape": [3, a.height, a.width], "quantize": QUANTIZE,
           "protocol": f"device events, windows >= {a.min_window} s, {a.repeats} alternations restated / fused in one process after "
                       "warming up both; CPU: host clock, best of the repeats after one warm-up",
           "cases": []}
    for batch in a.batches:
        for masked in (False, True):
            steps = device_steps(batch, a.height, a.width, masked, dev)
            case = dict(batch=batch, masked=masked, **alternate(steps, 20, a.min_window, a.repeats))
            case["fused_us_per_view"] = round(case["fused"]["median_ms"] * 1e3 / batch, 3)
            case["largest_difference"] = agreement(steps)
            case["algorithmic"] = algorithmic(batch, a.height, a.width, masked)
            if a.cpu_repeats > 0:
                case["cpu_restated"] = cpu_ms(batch, a.height, a.width, masked, a.cpu_repeats)
                case["speedup_over_cpu"] = round(case["cpu_restated"]["min_ms"] / case["fused"]["median_ms"], 1)
            print(json.dumps(case), flush=True)
            doc["cases"].append(case)
    benchkit.write_doc(doc, a.out)


if __name__ == "__main__":
    main()
