"""What the attention layer of the plane generator costs on an MI355X on its two paths: attention="torch" (float64 torch ops, the
backward a second evaluation under autograd: the default) against attention="fused" (csrc/attention.hip).

    python tools/plane_attention_bench.py --out profiles/plane_attention_bench.json
        one process; the reference configuration (three planes, 8 x 20 x 20 -> 16 x 160 x 160, the attention at 400 tokens x 32
        channels), forward + backward.  Two comparisons: (a) the whole generator step, (b) the attention layer alone (for
        "torch": `_attention` and the re-evaluation under autograd exactly as `_PlaneGenerator` runs them; for "fused":
        `fused_attention`).  In each, both sides are warmed up, then five alternations torch / fused, every window timed with
        device events over at least --min-window seconds; then a few iterations of either side under torch.profiler for the
        launches per iteration, and the library's own count (sr_profile_collect).  Writes the JSON and prints it.  The "torch"
        side is the baseline; the exit status is 0 whichever side is faster (the fused path is opt-in).

Needs a HIP device; there is no CPU fallback."""
from __future__ import annotations

import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

from tools import benchkit  # noqa: E402


def generator_steps(dev, noise_res, seed=5):
    from splatfields_amd.plane_generator import VarTriPlaneEncoder, generate_planes
    torch.manual_seed(seed)
    enc = VarTriPlaneEncoder({"noise_res": noise_res, "layer_kwargs": {"n_frames": 0, "strategy": "none"}})
    with torch.no_grad():                               # the initialisation zeroes half the network: give every tensor a value
        for p in enc.parameters():
            if not p.any():
                p.normal_(0.0, 0.05)
    enc.to(dev)
    params = list(enc.parameters())
    probe = torch.randn(3, 16, 8 * noise_res, 8 * noise_res, device=dev)

    def step(mode):
        def fn():
            for p in params:
                p.grad = None
            out = generate_planes([s.net for s in enc.subs], [s.noise for s in enc.subs], attention=mode)
            (out * probe).sum().backward()
        return fn

    return {"torch": step("torch"), "fused": step("fused")}


def layer_steps(dev, noise_res, channels=32, groups=32, planes=3, seed=6):
    from splatfields_amd import plane_generator as pg
    g = torch.Generator().manual_seed(seed)
    rn = lambda *s: torch.randn(*s, generator=g).to(dev)
    x = rn(planes, channels, noise_res, noise_res)
    params = [[1.0 + 0.3 * rn(channels), 0.5 * rn(channels)] + [t for _ in range(4) for t in (rn(channels, channels) / channels ** 0.5, 0.3 * rn(channels))]
              for _ in range(planes)]
    dy = rn(planes, channels, noise_res, noise_res)

    def torch_path():              # the "attn" branches of _PlaneGenerator.forward and .backward
        with torch.no_grad():
            pg._attention(x, params, groups).contiguous()
        with torch.enable_grad():
            xx = x.detach().requires_grad_(True)
            leaves = [[t.detach().requires_grad_(True) for t in p] for p in params]
            y = pg._attention(xx, leaves, groups)
            torch.autograd.grad(y, [xx] + [t for p in leaves for t in p], dy)

    leaves = [[t.clone().requires_grad_(True) for t in p] for p in params]
    xs = [x[i].clone().requires_grad_(True) for i in range(planes)]

    def fused():
        y = pg.fused_attention(xs, *[[p[j] for p in leaves] for j in range(10)], groups=groups)
        torch.autograd.grad(y, xs + [t for p in leaves for t in p], dy)

    return {"torch": torch_path, "fused": fused}


def main():
    p = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    p.add_argument("--out", default=None)
    p.add_argument("--noise-res", type=int, default=20)
    p.add_argument("--repeats", type=int, default=5)
    p.add_argument("--warmup", type=int, default=10)
    p.add_argument("--min-window", type=float, default=0.5, help="seconds per timed window")
    p.add_argument("--profiled-iterations", type=int, default=3)
    a = p.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("plane_attention_bench needs a HIP device: there is no CPU fallback")
    dev = torch.device("cuda:0")
    from splatfields_amd.build import source_hash
    from splatfields_amd.plane_generator import ATTENTION_LAUNCHES
    doc = {"device": torch.cuda.get_device_name(0), "torch": torch.__version__, "_source_hash": source_hash(),
           "workload": f"three planes, 8 x {a.noise_res} x {a.noise_res} -> 16 x {8 * a.noise_res} x {8 * a.noise_res}, forward + backward; the attention "
                       f"layer at {a.noise_res * a.noise_res} tokens x 32 channels, 32 groups",
           "protocol": f"one process; per comparison both sides warmed up ({a.warmup} iterations), then {a.repeats} alternations torch / fused, windows "
                       f">= {a.min_window} s between device events; launches from torch.profiler ({a.profiled_iterations} iterations per side) and from "
                       "sr_profile_collect (one iteration); 'torch' is the default path and the baseline",
           "attention_launches": list(ATTENTION_LAUNCHES),
           "generator_step": benchkit.compare(generator_steps(dev, a.noise_res), a),
           "attention_layer": benchkit.compare(layer_steps(dev, a.noise_res), a)}
    benchkit.write_doc(doc, a.out)
    return 0


if __name__ == "__main__":
    sys.exit(main())
