"""What the Adam step of the deform network costs on an MI355X: NetworkAdam (splatfields_amd/network_optim.py -> sr_net_adam_step)
next to torch.optim.Adam, which is what the reference steps (scene/deform_model.py:23-34, train.py:318).

    python tools/network_adam_bench.py --out profiles/network_adam_bench.json

The protocol of tools/adam_bench.py: one process, every optimizer on its own copy of the tensors, fixed gradients, all sides
warmed up, then five rounds over all sides, every window at least 0.3 s between device events.  Inputs are the parameter shapes of
three real networks: static (n_frames=0), 4-D (n_frames=50, composition_rank=10) and 4-D with the plane generator
(layer_strategy='per_frame').  Sides: torch.optim.Adam default (the baseline), torch.optim.Adam(fused=True), SplatAdam (32 tensors a
launch) and NetworkAdam.  Per side: device time per step, host wall time of step() alone with the stream idle (issue cost),
launches per step and their summed duration (torch.profiler, one step, a run of its own) and the share of 6.29 TB/s at 28 B per element.  Then the whole step of
the 4-D network (forward + backward + optimizer step, 100 k points) with train_setting(optimizer="torch") and "fused".

Needs a HIP device; there is no CPU fallback."""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys
import time
import types

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

from tests.launches import device_events  # noqa: E402
from tools import benchkit  # noqa: E402
from tools.adam_bench import BYTES_PER_ELEMENT, HBM_ACHIEVABLE  # noqa: E402

CONFIGS = {
    "static": dict(n_frames=0),
    "4d": dict(n_frames=50, composition_rank=10),
    "4d_plane_generator": dict(n_frames=50, composition_rank=10, encoder_args={"generator": "decoder"}, layer_strategy="per_frame"),
}
LR = 8e-4          # position_lr_init 1.6e-4 x spatial_lr_scale 5


def shapes_of(config):
    from splatfields_amd.deform_field import SplatFields
    return [tuple(p.shape) for p in SplatFields(**CONFIGS[config]).parameters()]


def tensors(shapes, dev, seed=0):
    g = torch.Generator(device=dev).manual_seed(seed)
    params = [torch.nn.Parameter(torch.randn(s, device=dev, generator=g)) for s in shapes]
    for p in params:
        p.grad = torch.randn(p.shape, device=dev, generator=g) * 1e-3
    return params


def sides(shapes, dev):
    from splatfields_amd import NetworkAdam, SplatAdam
    group = lambda: [{"params": tensors(shapes, dev), "lr": LR, "name": "deform"}]
    return {"torch_default": torch.optim.Adam(group(), lr=0.0, eps=1e-15), "torch_fused": torch.optim.Adam(group(), lr=0.0, eps=1e-15, fused=True),
            "splat_adam": SplatAdam(group(), lr=0.0, eps=1e-15), "network_adam": NetworkAdam(group(), lr=0.0, eps=1e-15)}


def host_ms(step, repeats=30):
    """wall time of step() alone: the stream is idle when it starts, so this is what the host spends issuing it"""
    out = []
    for _ in range(repeats):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        step()
        out.append((time.perf_counter() - t0) * 1e3)
    torch.cuda.synchronize()
    return out


def launches(step):
    records = device_events(step, drop_host_ranges=True)
    return len(records), round(sum(e.time_range.elapsed_us() for e in records), 2)


def optimizer_alone(config, dev, min_window, repeats):
    shapes = shapes_of(config)
    elements = sum(int(torch.Size(s).numel()) for s in shapes)
    opts = sides(shapes, dev)
    out = benchkit.alternate({name: o.step for name, o in opts.items()}, 10, min_window, repeats, calibrate=5, digits=5)[0]
    for name, o in opts.items():
        r = out[name]
        h = host_ms(o.step)
        r["host_ms_median"], r["host_ms_min"], r["host_ms_max"] = round(statistics.median(h), 5), round(min(h), 5), round(max(h), 5)
        r["launches_per_step"], r["kernel_us_per_step"] = launches(o.step)      # the records' own durations: one traced step
        r["bytes_per_s"] = round(BYTES_PER_ELEMENT * elements / (r["median_ms"] * 1e-3), 1)
        r["share_of_achievable_hbm"] = round(r["bytes_per_s"] / HBM_ACHIEVABLE, 4)
    base, mine = out["torch_default"], out["network_adam"]
    return {"tensors": len(shapes), "elements": elements, "tensors_under_1024_elements": sum(torch.Size(s).numel() < 1024 for s in shapes),
            "floor_ms_at_6.29TBps": round(BYTES_PER_ELEMENT * elements / HBM_ACHIEVABLE * 1e3, 5), "steps": out,
            "network_adam_faster_than_torch_default_in_every_alternation": all(a < b for a, b in zip(mine["ms"], base["ms"])),
            "torch_default_over_network_adam_median": round(base["median_ms"] / mine["median_ms"], 3),
            "torch_default_over_network_adam_host_median": round(base["host_ms_median"] / mine["host_ms_median"], 3)}


def whole_step(dev, points, min_window, repeats):
    """forward + backward + optimizer step of the 4-D network, train_setting(optimizer="torch") against "fused" """
    from splatfields_amd.deform_field import SplatFieldsModel
    train = types.SimpleNamespace(position_lr_init=1.6e-4, position_lr_final=1.6e-6, position_lr_delay_mult=0.01, deform_lr_max_steps=40000)
    g = torch.Generator(device=dev).manual_seed(1)
    xyz = torch.rand(points, 3, device=dev, generator=g) * 1.6 - 0.8
    t = torch.full((points, 1), 17.0 / 49.0, device=dev)
    steps = {}
    for name in ("torch", "fused"):
        torch.manual_seed(0)
        model = SplatFieldsModel(types.SimpleNamespace(**CONFIGS["4d"]), radius=None, device=dev)
        with torch.no_grad():
            model.deform.encoder.planes.normal_(0.0, 0.3)
        model.train_setting(train, optimizer=name)

        def step(model=model):
            model.optimizer.zero_grad(set_to_none=True)
            out = model.step(xyz, t)
            sum(v.sum() for k, v in out.items() if torch.is_tensor(v) and k != "flow").backward()
            model.optimizer.step()
        steps[name] = step
    out = benchkit.alternate(steps, 10, min_window, repeats, calibrate=5, digits=5)[0]
    out["fused_faster_in_every_alternation"] = all(a < b for a, b in zip(out["fused"]["ms"], out["torch"]["ms"]))
    out["saved_ms_median"] = round(out["torch"]["median_ms"] - out["fused"]["median_ms"], 5)
    return dict(points=points, what="forward + backward + optimizer step of SplatFields(n_frames=50, composition_rank=10)", **out)


def main():
    p = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    p.add_argument("--out", default=None)
    p.add_argument("--configs", nargs="*", default=list(CONFIGS))
    p.add_argument("--points", type=int, default=100_000)
    p.add_argument("--repeats", type=int, default=5)
    p.add_argument("--min-window", type=float, default=0.3, help="seconds per timed window")
    p.add_argument("--only-optimizer", action="store_true")
    a = p.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("network_adam_bench needs a HIP device: there is no CPU fallback")
    dev = torch.device("cuda:0")
    import gc
    gc.collect()
    gc.disable()
    from splatfields_amd import _lib
    from splatfields_amd.build import source_hash
    doc = {"device": torch.cuda.get_device_name(0), "torch": torch.__version__, "_source_hash": source_hash(),
           "protocol": f"device events, windows >= {a.min_window} s, {a.repeats} rounds over all sides in one process after warming up every "
                       "side; host time: wall clock of step() with the stream idle, 30 calls; launches: torch.profiler, one step, a run of its own",
           "baseline": "torch_default", "bytes_per_element": BYTES_PER_ELEMENT, "hbm_achievable_bytes_per_s": HBM_ACHIEVABLE,
           "max_grads_per_launch": _lib.NET_ADAM_MAX_GRADS, "optimizer_alone": {}}
    for config in a.configs:
        doc["optimizer_alone"][config] = optimizer_alone(config, dev, a.min_window, a.repeats)
        print(json.dumps(doc["optimizer_alone"][config]), flush=True)
        torch.cuda.empty_cache()
    if not a.only_optimizer:
        doc["whole_step_4d"] = whole_step(dev, a.points, a.min_window, a.repeats)
        print(json.dumps(doc["whole_step_4d"]), flush=True)
    benchkit.write_doc(doc, a.out)


if __name__ == "__main__":
    main()
