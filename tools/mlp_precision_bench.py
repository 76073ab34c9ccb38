"""What the opt-in precisions of the fused MLP chains (splatfields_amd.set_mlp_precision / SplatFields(mlp_precision=),
csrc/mlp.hip: k_mlp_chain_bf16, csrc/mlp_bf16x3.h: k_mlp_chain_bf16x3) buy on an MI355X: the decoder-free SplatFields-shaped deform
network of tools/deform_step_profile.py at 100 k points, forward + backward, in fp32 and in bf16 -- or, with --precisions, in any
of fp32, bf16, bf16x3, alternated the same way.

    python tools/mlp_precision_bench.py --out profiles/mlp_precision_bench.json
        two networks with the same weights, one per precision, both warmed up, then `--repeats` alternations; in every alternation
        and for either precision a window of steps timed with device events and a second window under torch.profiler, from which
        the per-step sums of the chain / pack / weight-gradient kernels and the launches per step are taken.  Writes the JSON and
        prints it.  Exit status 1 if the summed chain-kernel time under bf16 is not below fp32's in every alternation.
    python tools/mlp_precision_bench.py --precisions fp32,bf16,bf16x3 --heads separate,grouped --out profiles/mlp_split_precision_bench.json
        the same protocol over three precisions, once per heads mode (SplatFields(heads=)); per precision also the 128-wide (<8>) and
        the 64-wide (<4>) chain kernels alone, and whether each precision's step and chain sum beat fp32's in every alternation.
        Always exit status 0: the numbers are a record, not a condition.
    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -o r -- python tools/mlp_precision_bench.py --trace bf16|fp32
        a run of its own for the profiler: --iters steps of one precision, nothing else.

Needs a HIP device; there is no CPU fallback."""
from __future__ import annotations

import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

from tools import benchkit  # noqa: E402

KERNEL_GROUPS = (("chain", "k_mlp_chain"), ("pack", "k_mlp_pack"), ("weight_grad", "k_mlp_weight_grad"))
WIDTH_GROUPS = (("chain8", "<8>"), ("chain4", "<4>"))      # the chain kernels of one hidden width (template argument HT)
VERDICT_ASK_MS = 3.5      # the network step at 100 k points


def make_steps(n, dev, precisions, heads=None):
    """-> {precision: step}: forward + backward of a generic loss, every network a copy of the same weights"""
    from splatfields_amd.deform_field import SplatFields
    torch.manual_seed(0)
    xyz = (torch.rand(n, 3, device=dev) * 2 - 1)
    t_emb = torch.full((n, 1), 0.37, device=dev)
    state, steps = None, {}
    for precision in precisions:
        net = SplatFields(n_frames=50, composition_rank=10, encoder=None, flow_model="offset", mlp_precision=precision,
                          **({} if heads is None else {"heads": heads})).to(dev)
        if state is None:
            state = {k: v.clone() for k, v in net.state_dict().items()}
        net.load_state_dict(state)
        params = list(net.parameters())
        pts = xyz.clone().requires_grad_(True)

        def step(net=net, params=params, pts=pts):
            for p in params:
                p.grad = None
            pts.grad = None
            out = net(pts, t_emb)
            sum((v * v).mean() for k, v in out.items() if torch.is_tensor(v) and k != "flow").backward()
        steps[precision] = step
    return steps


def kernel_sums(fn, iters):
    """per step: microseconds in each kernel group, in all kernels, and launches (torch.profiler's device kernel records)"""
    from torch.profiler import ProfilerActivity, profile
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CUDA]) as prof:
        for _ in range(iters):
            fn()
        torch.cuda.synchronize()
    out = {g: 0.0 for g, _ in KERNEL_GROUPS + WIDTH_GROUPS}
    out.update(all_kernels=0.0, launches=0.0)
    names = {}
    for ev in prof.events():
        if ev.device_type == torch.autograd.DeviceType.CPU or ev.name.startswith(("Memcpy", "Memset")):
            continue                                      # device records only, kernels only
        us = float(ev.device_time_total)
        if us <= 0.0:
            continue
        out["all_kernels"] += us
        out["launches"] += 1
        for g, key in KERNEL_GROUPS:
            if key in ev.name:
                out[g] += us
                names[ev.name[:72]] = names.get(ev.name[:72], 0.0) + us
        if "k_mlp_chain" in ev.name:
            for g, key in WIDTH_GROUPS:
                if key in ev.name:
                    out[g] += us
    if out["launches"] == 0:
        raise SystemExit("torch.profiler recorded no device kernels: the per-kernel sums cannot be taken on this installation")
    res = {k: round(v / iters, 3) for k, v in out.items()}
    res["kernels_us"] = {k: round(v / iters, 3) for k, v in sorted(names.items())}
    return res


def main():
    p = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    p.add_argument("--out", default=None)
    p.add_argument("--points", type=int, default=100_000)
    p.add_argument("--repeats", type=int, default=5)
    p.add_argument("--warmup", type=int, default=10)
    p.add_argument("--min-window", type=float, default=0.3, help="seconds per timed window")
    p.add_argument("--profiled-steps", type=int, default=5)
    p.add_argument("--trace", choices=["fp32", "bf16", "bf16x3"], default=None)
    p.add_argument("--precisions", default="fp32,bf16", help="comma-separated, fp32 first: the baseline")
    p.add_argument("--heads", default=None, help="comma-separated SplatFields(heads=) modes, one measurement each (default: the module's default)")
    p.add_argument("--iters", type=int, default=20)
    a = p.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("mlp_precision_bench needs a HIP device: there is no CPU fallback")
    dev = torch.device("cuda:0")
    if a.trace:
        fn = make_steps(a.points, dev, [a.trace])[a.trace]
        for _ in range(a.iters):
            fn()
        torch.cuda.synchronize()
        return 0
    if a.precisions != "fp32,bf16" or a.heads is not None:
        return main_split(a, dev)
    from splatfields_amd.build import source_hash
    import gc
    steps = make_steps(a.points, dev, ["fp32", "bf16"])
    gc.collect()
    gc.disable()
    iters = {}
    for name, fn in steps.items():
        for _ in range(a.warmup):
            fn()
        iters[name] = max(5, int(a.min_window * 1e3 / benchkit.window_ms(fn, 5)) + 1)
        kernel_sums(fn, 2)                                # the profiler's own first-use cost stays out of the alternations
    rounds = []
    for _ in range(a.repeats):
        r = {}
        for name, fn in steps.items():
            r[name] = dict(step_ms=round(benchkit.window_ms(fn, iters[name]), 5), **kernel_sums(fn, a.profiled_steps))
        rounds.append(r)
    med = lambda name, key: round(statistics.median(r[name][key] for r in rounds), 5)
    summary = {name: {key: med(name, key) for key in ("step_ms", "chain", "pack", "weight_grad", "all_kernels", "launches")}
               for name in steps}
    doc = {"device": torch.cuda.get_device_name(0), "torch": torch.__version__, "_source_hash": source_hash(), "points": a.points,
           "network": "SplatFields(n_frames=50, composition_rank=10, encoder=None, flow_model='offset'): six GeneralMLPs + flow head",
           "protocol": f"one process, both precisions warmed up ({a.warmup} steps), {a.repeats} alternations; per alternation and precision a "
                       f"window >= {a.min_window} s between device events (step_ms) and {a.profiled_steps} steps under torch.profiler "
                       "(kernel microseconds and launches per step)",
           "iterations_per_window": iters, "alternations": rounds, "median": summary,
           "chain_us_bf16_below_fp32_in_every_alternation": all(r["bf16"]["chain"] < r["fp32"]["chain"] for r in rounds),
           "chain_speedup_median": round(summary["fp32"]["chain"] / summary["bf16"]["chain"], 3),
           "step_speedup_median": round(summary["fp32"]["step_ms"] / summary["bf16"]["step_ms"], 3),
           "verdict_item6_ask_ms": VERDICT_ASK_MS}
    benchkit.write_doc(doc, a.out)
    return 0 if doc["chain_us_bf16_below_fp32_in_every_alternation"] else 1


def measure(a, dev, precisions, heads):
    """the protocol of main() for any list of precisions and one heads mode -> (iterations per window, alternations, medians)"""
    import gc
    steps = make_steps(a.points, dev, precisions, heads)
    gc.collect()
    gc.disable()
    iters = {}
    for name, fn in steps.items():
        for _ in range(a.warmup):
            fn()
        iters[name] = max(5, int(a.min_window * 1e3 / benchkit.window_ms(fn, 5)) + 1)
        kernel_sums(fn, 2)
    rounds = []
    for _ in range(a.repeats):
        rounds.append({name: dict(step_ms=round(benchkit.window_ms(fn, iters[name]), 5), **kernel_sums(fn, a.profiled_steps)) for name, fn in steps.items()})
    gc.enable()
    keys = ("step_ms", "chain", "chain8", "chain4", "pack", "weight_grad", "all_kernels", "launches")
    summary = {name: {key: round(statistics.median(r[name][key] for r in rounds), 5) for key in keys} for name in steps}
    return iters, rounds, summary


def main_split(a, dev):
    from splatfields_amd.build import source_hash
    precisions = a.precisions.split(",")
    if precisions[0] != "fp32":
        raise SystemExit("--precisions starts with fp32: it is the baseline of the same build")
    doc = {"device": torch.cuda.get_device_name(0), "torch": torch.__version__, "_source_hash": source_hash(), "points": a.points,
           "network": "SplatFields(n_frames=50, composition_rank=10, encoder=None, flow_model='offset'): six GeneralMLPs + flow head",
           "protocol": f"one process; per heads mode every precision warmed up ({a.warmup} steps), then {a.repeats} alternations over "
                       f"{precisions}; per alternation and precision a window >= {a.min_window} s between device events (step_ms) and "
                       f"{a.profiled_steps} steps under torch.profiler (kernel microseconds and launches per step; chain8 / chain4: the "
                       "chain kernels of hidden width 128 / 64 alone)",
           "baseline": "fp32 of the same build", "heads": {}}
    for heads in (a.heads.split(",") if a.heads else [None]):
        iters, rounds, summary = measure(a, dev, precisions, heads)
        entry = {"iterations_per_window": iters, "alternations": rounds, "median": summary, "against_fp32": {}}
        for name in precisions[1:]:
            entry["against_fp32"][name] = {
                "step_faster_in_every_alternation": all(r[name]["step_ms"] < r["fp32"]["step_ms"] for r in rounds),
                "chain_faster_in_every_alternation": all(r[name]["chain"] < r["fp32"]["chain"] for r in rounds),
                "step_speedup_median": round(summary["fp32"]["step_ms"] / summary[name]["step_ms"], 3),
                "chain_speedup_median": round(summary["fp32"]["chain"] / summary[name]["chain"], 3),
                "chain8_speedup_median": round(summary["fp32"]["chain8"] / summary[name]["chain8"], 3),
                "chain4_speedup_median": round(summary["fp32"]["chain4"] / summary[name]["chain4"], 3)}
        doc["heads"][heads or "default"] = entry
    benchkit.write_doc(doc, a.out)
    return 0


if __name__ == "__main__":
    sys.exit(main())
