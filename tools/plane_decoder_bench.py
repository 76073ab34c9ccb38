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
import ctypes as C
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402


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


def window_ms(fn, iters):
    start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    start.record()
    for _ in range(iters):
        fn()
    end.record()
    end.synchronize()
    return start.elapsed_time(end) / iters


def launches_per_iteration(fn, iters):
    from torch.profiler import ProfilerActivity, profile
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
        for _ in range(iters):
            fn()
        torch.cuda.synchronize()
    events = [e for e in prof.events() if e.device_type != torch.autograd.DeviceType.CPU and not e.name.startswith(("Memcpy", "Memset"))]
    if not events:
        return None
    return {"all": round(len(events) / iters, 2), "library": round(sum(1 for e in events if "sr::" in e.name) / iters, 2)}


def library_launches(fn):
    from splatfields_amd import _lib
    lib = _lib.load()
    ms, cnt = (C.c_double * _lib.PROFILE_STAGES)(), (C.c_longlong * _lib.PROFILE_STAGES)()
    lib.sr_profile_collect(ms, cnt)
    ms, cnt = (C.c_double * _lib.PROFILE_STAGES)(), (C.c_longlong * _lib.PROFILE_STAGES)()
    lib.sr_profile_enable(1)
    fn()
    torch.cuda.synchronize()
    lib.sr_profile_enable(0)
    lib.sr_profile_collect(ms, cnt)
    return {"forward": cnt[0], "backward": cnt[6], "kernel_ms_forward": round(ms[0], 4), "kernel_ms_backward": round(ms[6], 4)}


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
    iters = {}
    for name, fn in fns.items():
        for _ in range(a.warmup):
            fn()
        iters[name] = max(3, int(a.min_window * 1e3 / window_ms(fn, 3)) + 1)
    times = {name: [] for name in fns}
    for _ in range(a.repeats):
        for name, fn in fns.items():
            times[name].append(window_ms(fn, iters[name]))
    doc = {"device": torch.cuda.get_device_name(0), "torch": torch.__version__, "_source_hash": source_hash(),
           "workload": f"three planes, 8 x {a.noise_res} x {a.noise_res} -> 16 x {8 * a.noise_res} x {8 * a.noise_res}, forward + backward, float32",
           "protocol": f"one process; both sides warmed up ({a.warmup} iterations), then {a.repeats} alternations pytorch / hip, windows >= "
                       f"{a.min_window} s between device events; launches from torch.profiler ({a.profiled_iterations} iterations per side) "
                       "and from sr_profile_collect (one iteration)"}
    for name, ts in times.items():
        doc[name] = {"ms": [round(t, 4) for t in ts], "median_ms": round(statistics.median(ts), 4), "min_ms": round(min(ts), 4),
                     "max_ms": round(max(ts), 4), "iterations_per_window": iters[name],
                     "launches_per_iteration": launches_per_iteration(fns[name], a.profiled_iterations) if a.profiled_iterations else "not measured"}
    doc["hip"]["library_launches"] = library_launches(fns["hip"])
    doc["speedup_median"] = round(doc["pytorch"]["median_ms"] / doc["hip"]["median_ms"], 3)
    doc["hip_faster_in_every_alternation"] = all(h < t for t, h in zip(times["pytorch"], times["hip"]))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        json.dump(doc, open(a.out, "w"), indent=1)
    print(json.dumps(doc))
    return 0 if doc["hip_faster_in_every_alternation"] else 1


if __name__ == "__main__":
    sys.exit(main())
