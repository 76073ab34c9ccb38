"""What the fused Adam step (splatfields_amd/optim.py: SplatAdam -> sr_adam_step) costs on an MI355X next to torch.optim.Adam,
which is what the reference steps (scene/gaussian_model.py:130-139, train.py:314-322).

    python tools/adam_bench.py --out profiles/adam_bench.json
        optimizer step alone at 1 M and 300 k splats (SH degree 3, the reference's six groups and learning rates): torch.optim.Adam
        default (foreach), torch.optim.Adam(fused=True), SplatAdam, and SplatAdam with the visibility mask of each of the bench's
        eight views; the whole iteration render() + photometric_loss + backward() + step with torch's Adam and with SplatAdam; and
        the plain render step (forward + backward, as bench.py times it) with and without a SplatAdam step between the timed
        steps, outside the timing marks.  Every comparison: all sides warmed up, then alternating windows timed with device
        events.  Writes the JSON and prints it.
    python tools/adam_bench.py --variants nt=/path/libsplatraster_nt.so unroll4=/path/lib_unroll4.so ...
        adds A/B windows of other builds of the library (python -m splatfields_amd.build OUT.so SR_ADAM_NONTEMPORAL=1) to the
        optimizer-alone comparison.
    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -o r -- python tools/adam_bench.py --trace torch|fused|splat|masked
        a run of its own for the profiler: --iters steps of the optimizer alone at --splats, nothing else.
    python tools/adam_bench.py --merge torch=DIR fused=DIR splat=DIR masked=DIR --out profiles/adam_bench.json
        adds launches per step and kernel time per step from the traces.

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

HBM_ACHIEVABLE = 6.29e12     # bytes / s: a float4 copy on this part (79 % of the 8.0e12 specification)
BYTES_PER_ELEMENT = 28       # read parameter, gradient and both moments, write three of them back
SHAPES = {"xyz": (3,), "f_dc": (1, 3), "f_rest": (15, 3), "opacity": (1,), "scaling": (3,), "rotation": (4,)}
# reference arguments/__init__.py: position_lr_init 1.6e-4 (x spatial_lr_scale, 5 here), feature_lr 2.5e-3 (rest / 20),
# opacity_lr 0.05, scaling_lr 5e-3, rotation_lr 1e-3
LRS = {"xyz": 8e-4, "f_dc": 2.5e-3, "f_rest": 2.5e-3 / 20, "opacity": 5e-2, "scaling": 5e-3, "rotation": 1e-3}
ELEMENTS_PER_SPLAT = 59


def six_groups(n, dev, seed=0):
    g = torch.Generator(device=dev).manual_seed(seed)
    params = {k: torch.nn.Parameter(torch.randn((n,) + s, device=dev, generator=g)) for k, s in SHAPES.items()}
    for p in params.values():
        p.grad = torch.randn(p.shape, device=dev, generator=g) * 1e-3
    return params, [{"params": [p], "lr": LRS[k], "name": k} for k, p in params.items()]


def view_masks(n, height, width, sh_degree, dev):
    """radii > 0 of the bench's eight views of the bench's cloud: what a training loop would pass as `visible`"""
    from splatfields_amd import render
    from splatfields_amd.synthetic import make_camera, make_splats
    sp = make_splats(n, seed=1234, device=dev)
    pack = {"means3D": sp["means3D"], "active_sh_degree": sh_degree, "gaussian_opacity": sp["opacities"],
            "gaussian_features": sp["shs"], "gaussian_scales": sp["scales"], "gaussian_rotations": sp["rotations"]}
    pipe, bg = types.SimpleNamespace(debug=False), torch.ones(3, device=dev)
    with torch.no_grad():
        return [render(make_camera(k, width, height, device=dev), pack, pipe, bg)["visibility_filter"].clone() for k in range(8)]


def optimizer_steps(n, dev, masks=(), variants=(), only=None):
    """-> {name: fn}: one optimizer step each, every optimizer on its own copy of the six tensors (`only`: just that one)"""
    from splatfields_amd import SplatAdam, _lib
    steps = {}
    for name, make in (("torch_default", lambda g: torch.optim.Adam(g, lr=0.0, eps=1e-15)),
                       ("torch_fused", lambda g: torch.optim.Adam(g, lr=0.0, eps=1e-15, fused=True)),
                       ("splat", lambda g: SplatAdam(g, lr=0.0, eps=1e-15))):
        if only in (None, name):
            _, groups = six_groups(n, dev)
            steps[name] = make(groups).step
    if only is not None and not masks:
        return steps
    _, groups = six_groups(n, dev)
    shared = SplatAdam(groups, lr=0.0, eps=1e-15)       # the masked steps and the other builds share one set of tensors
    for k, mask in enumerate(masks):
        steps[f"splat_masked_view{k}"] = (lambda m: lambda: shared.step(visible=m))(mask)
    for label, path in variants:
        ctx = _lib.use_library(path)

        def with_library(ctx=ctx, mask=None):
            with ctx:
                shared.step(visible=mask)
        steps[f"splat_{label}"] = with_library
        if masks:
            steps[f"splat_{label}_masked_view0"] = (lambda c, m: lambda: with_library(c, m))(ctx, masks[0])
    return steps


def alternate(steps, warmup, min_window_s, repeats):
    """All sides warmed up, then `repeats` rounds over all of them; every window lasts at least `min_window_s`."""
    return benchkit.alternate(steps, warmup, min_window_s, repeats, calibrate=5, digits=5)[0]


def optimizer_alone(n, height, width, sh_degree, dev, variants, min_window, repeats):
    masks = view_masks(n, height, width, sh_degree, dev)
    out = alternate(optimizer_steps(n, dev, masks, variants), 10, min_window, repeats)
    elements = n * ELEMENTS_PER_SPLAT
    for name, r in out.items():
        r["algorithmic_bytes"] = BYTES_PER_ELEMENT * elements
        if "masked_view" in name:
            frac = masks[int(name.rsplit("view", 1)[1])].float().mean().item()
            # every tensor's pass reads the mask once: 6 N bytes; the visible rows move 28 B an element
            r.update(visible_fraction=round(frac, 4), algorithmic_bytes=int(BYTES_PER_ELEMENT * elements * frac) + len(SHAPES) * n,
                     mask_bytes=len(SHAPES) * n)
        r["bytes_per_s"] = round(r["algorithmic_bytes"] / (r["median_ms"] * 1e-3), 1)
        r["share_of_achievable_hbm"] = round(r["bytes_per_s"] / HBM_ACHIEVABLE, 4)
    doc = {"splats": n, "elements": elements, "floor_ms_at_6.29TBps": round(BYTES_PER_ELEMENT * elements / HBM_ACHIEVABLE * 1e3, 5),
           "steps": out}
    doc["splat_faster_than_torch_default_in_every_repetition"] = out["splat"]["max_ms"] < out["torch_default"]["min_ms"]
    doc["splat_over_torch_default_median"] = round(out["torch_default"]["median_ms"] / out["splat"]["median_ms"], 3)
    doc["splat_over_torch_fused_median"] = round(out["torch_fused"]["median_ms"] / out["splat"]["median_ms"], 3)
    return doc


def render_scene(n, height, width, sh_degree, dev):
    from splatfields_amd import render
    from splatfields_amd.synthetic import make_camera, make_splats
    sp = make_splats(n, seed=1234, device=dev)
    pipe, bg = types.SimpleNamespace(debug=False), torch.ones(3, device=dev)
    cams = [make_camera(k, width, height, device=dev) for k in range(8)]
    names = ["means3D", "scales", "rotations", "opacities", "shs"]
    pack = lambda p: {"means3D": p["means3D"], "active_sh_degree": sh_degree, "gaussian_opacity": p["opacities"],
                      "gaussian_features": p["shs"], "gaussian_scales": p["scales"], "gaussian_rotations": p["rotations"]}
    fresh = lambda: {k: sp[k].clone().requires_grad_(True) for k in names}
    return sp, fresh, pack, lambda i, p: render(cams[i % len(cams)], pack(p), pipe, bg)


def iteration_steps(n, height, width, sh_degree, dev):
    """-> {"torch_default": fn, "splat": fn}: render() + photometric_loss + backward() + optimizer step of one view"""
    from splatfields_amd import SplatAdam
    from splatfields_amd.losses import photometric_loss
    sp, fresh, pack, draw = render_scene(n, height, width, sh_degree, dev)
    targets = []
    with torch.no_grad():
        other = dict(sp, shs=sp["shs"] * 0.8 + 0.05)
        for i in range(4):
            t = draw(i, other)
            targets.append((t["render"].clone(), (t["opacity"] > 0.5).float()))
    steps = {}
    for name, make in (("torch_default", torch.optim.Adam), ("splat", SplatAdam)):
        params = fresh()
        opt = make([{"params": [p], "lr": 1e-5} for p in params.values()], lr=0.0, eps=1e-15)
        count = [0]

        def step(params=params, opt=opt, count=count):
            i = count[0] % len(targets)
            count[0] += 1
            opt.zero_grad(set_to_none=True)
            pkg = draw(i, params)
            photometric_loss(pkg["render"], targets[i][0], 0.2, pkg["opacity"], targets[i][1], 0.1)[0].backward()
            opt.step()
        steps[name] = step
    return steps


def render_step_with_optimizer_between(n, height, width, sh_degree, dev, steps_per_window, repeats):
    """The render step as bench.py times it (forward + backward with fixed upstream gradients), every step between its own
    pair of events; in one series a SplatAdam step runs after each timed step, outside the marks, so the next step finds the
    parameters rewritten (and the moments, not the parameters, last in the Infinity Cache)."""
    from splatfields_amd import SplatAdam
    from splatfields_amd.synthetic import make_upstream_grads
    _, fresh, _, draw = render_scene(n, height, width, sh_degree, dev)
    ups = make_upstream_grads(height, width, device=dev)
    series = {}
    for name in ("render_step_alone", "render_step_with_splat_adam_between"):
        params = fresh()
        opt = SplatAdam([{"params": [p], "lr": 1e-5} for p in params.values()], lr=0.0, eps=1e-15)
        series[name] = (params, opt, name.endswith("between"))
    out = {name: [] for name in series}

    def window(params, opt, between, count):
        marks = []
        for i in range(count):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            for p in params.values():
                p.grad = None
            a.record()
            pkg = draw(i, params)
            torch.autograd.backward((pkg["render"], pkg["depth"], pkg["opacity"]), ups)
            b.record()
            marks.append((a, b))
            if between:
                opt.step()
        torch.cuda.synchronize()
        return sum(a.elapsed_time(b) for a, b in marks) / count

    for params, opt, between in series.values():
        window(params, opt, between, 10)
    for _ in range(repeats):
        for name, (params, opt, between) in series.items():
            out[name].append(window(params, opt, between, steps_per_window))
    return {name: benchkit.window_stats(ts, steps_per_window, 5, "steps_per_window") for name, ts in out.items()}


def merge(pairs, out_path, iters_total, n):
    doc = json.load(open(out_path))
    traces = {}
    for item in pairs:
        name, directory = item.split("=", 1)
        # the kernels of a step run in every step: the fills of the set-up and of the first step's state do not count
        rows = [r for r in benchkit.read_stats(directory) if r[1] >= iters_total]
        traces[name] = {"launches_per_step": round(sum(c for _, c, _, _ in rows) / iters_total, 2),
                        "kernel_us_per_step": round(sum(t for _, _, _, t in rows) / iters_total / 1e3, 3),
                        "distinct_kernels": len(rows), "steps_traced": iters_total, "splats": n,
                        "kernels": {r[0][:60]: {"calls": r[1], "average_us": round(r[2] / 1e3, 3)} for r in rows}}
        us = traces[name]["kernel_us_per_step"]
        if name != "masked" and us > 0:
            traces[name]["share_of_achievable_hbm_in_kernel_time"] = round(BYTES_PER_ELEMENT * ELEMENTS_PER_SPLAT * n / (us * 1e-6) / HBM_ACHIEVABLE, 4)
    doc["kernel_trace"] = traces
    benchkit.write_doc(doc, out_path)


def main():
    p = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    p.add_argument("--out", default=None)
    p.add_argument("--height", type=int, default=800)
    p.add_argument("--width", type=int, default=800)
    p.add_argument("--splats", type=int, default=1_000_000)
    p.add_argument("--small-splats", type=int, default=300_000)
    p.add_argument("--sh-degree", type=int, default=3)
    p.add_argument("--repeats", type=int, default=5)
    p.add_argument("--min-window", type=float, default=0.3, help="seconds per timed window")
    p.add_argument("--variants", nargs="*", default=[], metavar="NAME=LIB", help="other builds of libsplatraster.so to time next to the shipped one")
    p.add_argument("--only-optimizer", action="store_true")
    p.add_argument("--trace", choices=["torch", "fused", "splat", "masked"], default=None)
    p.add_argument("--iters", type=int, default=50)
    p.add_argument("--merge", nargs="+", default=None, metavar="NAME=DIR")
    a = p.parse_args()
    if a.merge:
        return merge(a.merge, a.out, a.iters, a.splats)
    if not torch.cuda.is_available():
        raise SystemExit("adam_bench needs a HIP device: there is no CPU fallback")
    dev = torch.device("cuda:0")
    if a.trace:
        mask = [torch.rand(a.splats, device=dev) < 0.35] if a.trace == "masked" else []
        key = {"torch": "torch_default", "fused": "torch_fused", "splat": "splat", "masked": "splat_masked_view0"}[a.trace]
        fn = optimizer_steps(a.splats, dev, mask, only=key)[key]
        for _ in range(a.iters):
            fn()
        torch.cuda.synchronize()
        return
    import gc
    gc.collect()
    gc.disable()
    variants = [tuple(v.split("=", 1)) for v in a.variants]
    doc = {"device": torch.cuda.get_device_name(0), "torch": torch.__version__,
           "protocol": f"device events, windows >= {a.min_window} s, {a.repeats} rounds over all sides in one process after warming up every side",
           "bytes_per_element": BYTES_PER_ELEMENT, "hbm_achievable_bytes_per_s": HBM_ACHIEVABLE,
           "learning_rates": LRS, "variants": dict(variants)}
    doc["optimizer_alone"] = {}
    for n in (a.splats, a.small_splats):
        doc["optimizer_alone"][str(n)] = optimizer_alone(n, a.height, a.width, a.sh_degree, dev, variants, a.min_window, a.repeats)
        print(json.dumps(doc["optimizer_alone"][str(n)]), flush=True)
        torch.cuda.empty_cache()
    if not a.only_optimizer:
        it = alternate(iteration_steps(a.splats, a.height, a.width, a.sh_degree, dev), 10, a.min_window, a.repeats)
        it["saved_ms_median"] = round(it["torch_default"]["median_ms"] - it["splat"]["median_ms"], 5)
        doc["whole_iteration"] = dict(splats=a.splats, shape=[3, a.height, a.width], sh_degree=a.sh_degree,
                                      what="render() + photometric_loss + backward() + optimizer step", **it)
        print(json.dumps(doc["whole_iteration"]), flush=True)
        torch.cuda.empty_cache()
        doc["render_step_optimizer_between"] = dict(
            splats=a.splats, shape=[3, a.height, a.width], sh_degree=a.sh_degree,
            **render_step_with_optimizer_between(a.splats, a.height, a.width, a.sh_degree, dev, 40, a.repeats))
    benchkit.write_doc(doc, a.out)


if __name__ == "__main__":
    main()
