"""What a step of the SplatFields network costs on an MI355X with its head networks run separately (heads="separate": one chain
of launches per network, the default) against grouped (heads="grouped": the networks of one width in one launch per phase;
csrc/mlp.hip: k_mlp_chain_group, k_mlp_group_*).

    python tools/heads_bench.py --out profiles/heads_bench.json
        one process.  Two networks at N = 100 k points and the default widths (W = 128 for the deform, colour and flow networks),
        forward + backward of a sum over every output with gradients for the positions and every parameter: the static network
        (four heads, composition_rank = 0) and the 4-D network (five heads, n_frames = 50, composition_rank = 40, flow_model =
        "se3"), each with the layer chains in fp32 and in bf16; decoder-free tri-plane sampler.  ONE module per configuration runs
        both sides (`net.heads` is switched), so both read the same parameters.  Both sides are warmed up, then five alternations
        separate / grouped, every window timed with device events over at least --min-window seconds; then a few iterations of
        either side under torch.profiler for the launches per iteration.  Writes the JSON and prints it.  "separate" is the
        baseline; the exit status is 0 whichever side is faster (the grouped path is opt-in).

Needs a HIP device; there is no CPU fallback."""
from __future__ import annotations

import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

from tools import benchkit  # noqa: E402

CONFIGS = {
    "static": dict(n_frames=0, composition_rank=0),
    "4d": dict(n_frames=50, composition_rank=40, flow_model="se3"),
}


def network_steps(dev, config, precision, n, seed=0):
    from splatfields_amd.deform_field import SplatFields
    torch.manual_seed(seed)
    net = SplatFields(encoder=None, mlp_precision=precision, **CONFIGS[config]).to(dev)
    xyz = (torch.rand(n, 3, device=dev) * 2 - 1).requires_grad_(True)
    t_emb = torch.full((n, 1), 0.37, device=dev)
    params = list(net.parameters())

    def step(mode):
        def fn():
            net.heads = mode
            for p in params:
                p.grad = None
            xyz.grad = None
            out = net(xyz, t_emb)
            sum((v * v).mean() for k, v in out.items() if torch.is_tensor(v) and k != "flow").backward()
        return fn

    return {"separate": step("separate"), "grouped": step("grouped")}, net


def compare(fns, a):
    doc, times = benchkit.alternate(fns, a.warmup, a.min_window, a.repeats, calibrate=3, digits=4)
    benchkit.with_launches(doc, fns, a.profiled_iterations)
    doc["grouped_minus_separate_median_ms"] = round(doc["grouped"]["median_ms"] - doc["separate"]["median_ms"], 4)
    doc["speedup_median"] = round(doc["separate"]["median_ms"] / doc["grouped"]["median_ms"], 3)
    doc["grouped_faster_in_every_alternation"] = all(g < s for s, g in zip(times["separate"], times["grouped"]))
    return doc


def main():
    p = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    p.add_argument("--out", default=None)
    p.add_argument("--points", type=int, default=100_000)
    p.add_argument("--repeats", type=int, default=5)
    p.add_argument("--warmup", type=int, default=10)
    p.add_argument("--min-window", type=float, default=0.3, help="seconds per timed window")
    p.add_argument("--profiled-iterations", type=int, default=3)
    a = p.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("heads_bench needs a HIP device: there is no CPU fallback")
    dev = torch.device("cuda:0")
    from splatfields_amd.build import source_hash
    doc = {"device": torch.cuda.get_device_name(0), "torch": torch.__version__, "_source_hash": source_hash(),
           "workload": f"SplatFields step, {a.points} points, default widths (W = 128), decoder-free tri-plane sampler, forward + backward of a sum "
                       "over every output but `flow`, gradients for the positions and every parameter; static: n_frames = 0, composition_rank = 0 "
                       "(four heads); 4d: n_frames = 50, composition_rank = 40, flow_model = 'se3' (five heads)",
           "protocol": f"one process; one module per configuration, `heads` switched; both sides warmed up ({a.warmup} iterations), then {a.repeats} "
                       f"alternations separate / grouped, windows >= {a.min_window} s between device events; launches from torch.profiler "
                       f"({a.profiled_iterations} iterations per side); 'separate' is the default path and the baseline",
           "steps": {}}
    for config in CONFIGS:
        for precision in ("fp32", "bf16"):
            fns, net = network_steps(dev, config, precision, a.points)
            entry = compare(fns, a)
            entry["groups"] = net._head_group.partition()
            doc["steps"][f"{config}_{precision}"] = entry
            del fns, net
            torch.cuda.empty_cache()
    benchkit.write_doc(doc, a.out)
    return 0


if __name__ == "__main__":
    sys.exit(main())
