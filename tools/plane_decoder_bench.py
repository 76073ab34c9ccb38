"""What the plane generator on HIP kernels (splatfields_amd/plane_generator.py) costs on an MI355X against the same network in
PyTorch (tests/plane_decoder_reference.py on the device in float32 -- what a user running the reference's classes gets).

    python tools/plane_decoder_bench.py --out profiles/plane_decoder_bench.json
        one process; the reference configuration (three planes, 8 x 20 x 20 -> 16 x 160 x 160), forward + backward; both sides
        warmed up, then five alternations pytorch / hip, every window timed with device events over at least --min-window
        seconds; then a few iterations of either side under torch.profiler for the launches per iteration, and the library's
        own count (sr_profile_collect) for the hip side.  Writes the JSON and prints it.  Exit status 1 unless the hip side is
        faster in EVERY alternation.

Needs a HIP device; there is no CPU fallback."""
from __future__ import annotations

import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

from tools import benchkit  # noqa: E402


def steps(dev, noise_res, seed=5):
    from splatfields_amd.plane_generator import VarTriPlaneEncoder
    from tests import plane_decoder_reference as R
    torch.manual_seed(seed)
    enc = VarTriPlaneEncoder({"noise_res": noise_res, "layer_kwargs": {"n_frames": 0, "strategy": "none"}})
    with torch.no_grad():                               # the initialisation zeroes half the network: give every tensor a value
        for p in enc.parameters():
            if not p.any():
                p.normal_(0.0, 0.05)
    enc.to(dev)
    params = list(enc.parameters())
    sd = dict(enc.state_dict(keep_vars=True))
    probe = torch.randn(3, 16, 8 * noise_res, 8 * noise_res, device=dev)

    def pytorch():
        for p in params:
            p.grad = None
        (R.planes(sd, 32) * probe).sum().backward()

    def hip():
        for p in params:
            p.grad = None
        (enc.get_planes(None) * probe).sum().backward()

    return {"pytorch": pytorch, "hip": hip}


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
        raise SystemExit("plane_decoder_bench needs a HIP device: there is no CPU fallback")
    dev = torch.device("cuda:0")
    from splatfields_amd.build import source_hash
    fns = steps(dev, a.noise_res)
    stats, times = benchkit.alternate(fns, a.warmup, a.min_window, a.repeats, calibrate=3, digits=4)
    doc = {"device": torch.cuda.get_device_name(0), "torch": torch.__version__, "_source_hash": source_hash(),
           "workload": f"three planes, 8 x {a.noise_res} x {a.noise_res} -> 16 x {8 * a.noise_res} x {8 * a.noise_res}, forward + backward, float32",
           "protocol": f"one process; both sides warmed up ({a.warmup} iterations), then {a.repeats} alternations pytorch / hip, windows >= "
                       f"{a.min_window} s between device events; launches from torch.profiler ({a.profiled_iterations} iterations per side) "
                       "and from sr_profile_collect (one iteration)"}
    doc.update(benchkit.with_launches(stats, fns, a.profiled_iterations))
    doc["hip"]["library_launches"] = benchkit.library_launches(fns["hip"])
    doc["speedup_median"] = round(doc["pytorch"]["median_ms"] / doc["hip"]["median_ms"], 3)
    doc["hip_faster_in_every_alternation"] = all(h < t for t, h in zip(times["pytorch"], times["hip"]))
    benchkit.write_doc(doc, a.out)
    return 0 if doc["hip_faster_in_every_alternation"] else 1


if __name__ == "__main__":
    sys.exit(main())
