"""What LPIPS (VGG) on HIP (splatfields_amd/lpips.py) costs on an MI355X, against the same network as float32 torch ops on the
device (`F.conv2d` / `F.max_pool2d` and the head: tests/lpips_reference.py, order "conv2d") -- what a user runs without the
kernels.  Random weights (LPIPSWeights.random): the published ones are not available here, and the time does not depend on them.

    python tools/lpips_bench.py --out profiles/lpips_bench.json
        800x800 with quantize="png", batch 1 and 8.  The baseline's first call (its library picks its algorithms there) is
        timed on its own with a host clock and recorded as a fact; then both sides are warmed up and alternate five times,
        every window timed with device events.  Launch counts of both sides and the time of the convolution launches come from
        the profiler afterwards, outside the timed windows.

Needs a HIP device; there is no CPU fallback for the HIP side."""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

from tools import benchkit  # noqa: E402

FP32_MFMA_PEAK = 157.3e12     # FLOP / s, f32-input MFMA (specification)
QUANTIZE = "png"
CONVS = ((3, 64), (64, 64), (64, 128), (128, 128), (128, 256), (256, 256), (256, 256), (256, 512), (512, 512), (512, 512), (512, 512),
         (512, 512), (512, 512))
GROUP_OF = (0, 0, 1, 1, 2, 2, 2, 3, 3, 3, 4, 4, 4)


def conv_flops(height, width, images=1):
    """2 x 9 x cin x cout x pixels over the 13 layers, per image (a pair is two images)"""
    return images * sum(2 * 9 * ci * co * (height >> g) * (width >> g) for (ci, co), g in zip(CONVS, GROUP_OF))


def torch_lpips(pred, gt, parts):
    """the network as torch ops on the tensors' device, float32, no host wait"""
    from tests import lpips_reference as R
    convs, lins, shift, scale = parts
    with torch.no_grad():
        n = pred.shape[0]
        feats = R.tap_features(torch.cat([R.quantise(pred, QUANTIZE), R.quantise(gt, QUANTIZE)]), convs, shift, scale, "conv2d")
        total = 0
        for f, lin in zip(feats, lins):
            f = f / (f.pow(2).sum(1, keepdim=True).sqrt() + R.EPS)
            total = total + ((f[:n] - f[n:]).pow(2) * lin.reshape(1, -1, 1, 1)).sum(1).mean((1, 2))
        return total


def conv_kernel_ms(fn, iters):
    """device milliseconds per call of the library's convolution launches, from the profiler's records"""
    from tests.launches import device_events
    events = [e for e in device_events(fn, iters) if "k_lpips_conv" in e.name]
    us = sum(getattr(e, "device_time", None) or getattr(e, "cuda_time", 0.0) for e in events)
    return us / 1e3 / iters, len(events) / iters


def main():
    p = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    p.add_argument("--out", default=None)
    p.add_argument("--height", type=int, default=800)
    p.add_argument("--width", type=int, default=800)
    p.add_argument("--batches", type=int, nargs="+", default=[1, 8])
    p.add_argument("--repeats", type=int, default=5)
    p.add_argument("--min-window", type=float, default=0.5, help="seconds per timed window")
    p.add_argument("--profiled-iterations", type=int, default=2)
    a = p.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("lpips_bench needs a HIP device: there is no CPU fallback")
    from splatfields_amd.lpips import DEFAULT_WORKSPACE_CAP, LPIPSWeights, lpips_vgg
    from tests import lpips_reference as R
    dev = torch.device("cuda:0")
    weights = LPIPSWeights.random(1, device=dev)
    weights.packed()
    parts = (weights.convs, weights.lins, weights.shift, weights.scale)
    doc = {"device": torch.cuda.get_device_name(0), "shape": [3, a.height, a.width], "quantize": QUANTIZE, "dtype": "float32 on both sides",
           "protocol": f"device events, windows >= {a.min_window} s, {a.repeats} alternations torch / hip in one process after warming up "
                       "both; the baseline's first call under a host clock, before anything else",
           "conv_flops_per_image": conv_flops(a.height, a.width), "fp32_mfma_peak_tflops": FP32_MFMA_PEAK / 1e12,
           "workspace_cap_bytes": DEFAULT_WORKSPACE_CAP, "cases": []}
    for batch in a.batches:
        pred, gt = (t.to(dev) for t in R.images(batch, a.height, a.width, seed=5))
        steps = {"torch": lambda: torch_lpips(pred, gt, parts), "hip": lambda: lpips_vgg(pred, gt, weights, quantize=QUANTIZE)}
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        first = steps["torch"]()
        torch.cuda.synchronize()
        first_ms = (time.perf_counter() - t0) * 1e3
        stats, times = benchkit.alternate(steps, 3, a.min_window, a.repeats, calibrate=2, digits=4)
        benchkit.with_launches(stats, steps, a.profiled_iterations)
        conv_ms, conv_launches = conv_kernel_ms(steps["hip"], a.profiled_iterations)
        flops = conv_flops(a.height, a.width, 2 * batch)
        case = dict(batch=batch, **stats)
        case["torch_first_call_ms"] = round(first_ms, 2)
        case["speedup_median"] = round(stats["torch"]["median_ms"] / stats["hip"]["median_ms"], 3)
        case["hip_faster_in_every_alternation"] = all(h < t for t, h in zip(times["torch"], times["hip"]))
        case["hip_ms_per_pair"] = round(stats["hip"]["median_ms"] / batch, 4)
        case["conv_launches_per_call"] = conv_launches
        case["conv_kernel_ms_per_call"] = round(conv_ms, 4)
        case["conv_tflops"] = round(flops / (conv_ms * 1e-3) / 1e12, 2) if conv_ms else "not measured"
        case["conv_share_of_peak"] = round(flops / (conv_ms * 1e-3) / FP32_MFMA_PEAK, 4) if conv_ms else "not measured"
        case["end_to_end_tflops"] = round(flops / (stats["hip"]["median_ms"] * 1e-3) / 1e12, 2)
        case["torch_end_to_end_tflops"] = round(flops / (stats["torch"]["median_ms"] * 1e-3) / 1e12, 2)
        case["largest_difference"] = float((first.double() - steps["hip"]().double()).abs().max())
        print(json.dumps(case), flush=True)
        doc["cases"].append(case)
        del pred, gt, steps, first
        torch.cuda.empty_cache()
    benchkit.write_doc(doc, a.out)


if __name__ == "__main__":
    main()
