"""What a subset step (`--n_splats`, splatfields_amd/subset.py, csrc/subset.hip) costs on an MI355X, in three parts:

    (i)   the bookkeeping of the step -- the draw, the gather of xyz / scaling / features and the scatter of the densification
          statistics -- against the reference's form restated in PyTorch as the baseline: a HOST torch.randperm(N)[:n] and its
          upload, indexing of get_xyz / get_scaling / get_features (the exp and the cat over all N rows), and the `_idx` clone /
          mask / assign updates (train.py:56-60, :281-286, scene/gaussian_model.py:431-438).  N = 300 k and 1 M, n = 100 k, SH 3.
    (ii)  draw_rows(M, 100 k) against torch.randperm(M, device)[:100 k] at M = 14.3 M, the depth initialisation's case: time and peak
          device memory, both orders of the draw.
    (iii) the 4-D network step (forward + backward) at 100 k points against n_splats = 30 k of them: what the subset buys.

    python tools/subset_bench.py --out profiles/subset_bench.json
        one process; per comparison both sides warmed up, then five alternations baseline / new, every window timed with device events
        over at least --min-window seconds; then a few iterations under torch.profiler for the launches per call, and one call each
        for the peak device memory.  No speed figure is a condition: the exit status is 0 whichever side is faster, and the file
        says which was, per alternation.

Needs a HIP device; there is no CPU fallback."""
from __future__ import annotations

import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

from tools import benchkit  # noqa: E402


def compare(steps, a, baseline, new):
    doc, times = benchkit.alternate(steps, a.warmup, a.min_window, a.repeats, calibrate=3, digits=4, count_key="calls_per_window")
    benchkit.with_launches(doc, steps, a.profiled_iterations, key="launches_per_call")
    for name, fn in steps.items():
        doc[name]["peak_device_mib"] = benchkit.peak_mib(fn)
    doc["baseline"] = baseline
    for name in new:
        doc[f"speedup_median_{name}"] = round(doc[baseline]["median_ms"] / doc[name]["median_ms"], 2)
        doc[f"{name}_faster_in_every_alternation"] = all(x < b for b, x in zip(times[baseline], times[name]))
    return doc


def bookkeeping(dev, N, n):
    """the two forms of a subset step's bookkeeping on the same model and the same rendered-view tensors"""
    from splatfields_amd import densification_stats, draw_rows, gather_rows
    from tests import subset_reference as R
    gs = R.StandInGaussians(N, sh_degree=3, device=dev, requires_grad=False)
    g = torch.Generator().manual_seed(1)
    grad = torch.randn(n, 3, generator=g).to(dev)
    radii = (torch.randint(1, 40, (n,), generator=g, dtype=torch.int32) * (torch.rand(n, generator=g) < 0.5)).to(torch.int32).to(dev)
    accum, denom, maxr = torch.zeros(N, 1, device=dev), torch.zeros(N, 1, device=dev), torch.zeros(N, device=dev)

    def reference():
        idx = torch.randperm(N)[:n]                                          # on the host, as train.py:57
        xyz, scaling, feats = gs.get_xyz.detach()[idx], gs.get_scaling.detach()[idx], gs.get_features[idx]
        R.stats_through_idx(grad, radii, idx.to(dev), accum, denom, maxr)
        return xyz, scaling, feats

    def new(order):
        def fn():
            idx = draw_rows(N, n, order=order, device=dev)
            out = gather_rows(idx, gs._xyz, gs._scaling, (gs._features_dc, gs._features_rest), ops=("copy", "exp", "copy"))
            densification_stats(grad, radii, accum, denom, maxr, idx=idx)
            return out
        return fn

    return {"pytorch_reference_form": reference, "hip_ascending": new("ascending"), "hip_draw_order": new("draw")}


def draws(dev, M, n):
    from splatfields_amd import draw_rows
    return {"torch_randperm_device": lambda: torch.randperm(M, device=dev)[:n],
            "hip_draw_order": lambda: draw_rows(M, n, device=dev),
            "hip_ascending": lambda: draw_rows(M, n, order="ascending", device=dev)}


def network(dev, n_all, n_sub):
    from splatfields_amd import draw_rows, gather_rows
    from tools.heads_bench import CONFIGS
    from splatfields_amd.deform_field import SplatFields
    torch.manual_seed(0)
    net = SplatFields(encoder=None, mlp_precision="fp32", **CONFIGS["4d"]).to(dev)
    xyz_all = torch.rand(n_all, 3, device=dev) * 2 - 1
    params = list(net.parameters())

    def step(n_splats):
        def fn():
            for p in params:
                p.grad = None
            xyz = xyz_all
            if 0 < n_splats < n_all:
                xyz, = gather_rows(draw_rows(n_all, n_splats, order="ascending", device=dev), xyz_all)
            out = net(xyz, torch.full((xyz.shape[0], 1), 0.37, device=dev))
            sum((v * v).mean() for k, v in out.items() if torch.is_tensor(v) and k != "flow").backward()
        return fn

    return {"all_points": step(-1), "subset": step(n_sub)}


def main():
    p = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    p.add_argument("--out", default=None)
    p.add_argument("--n", type=int, default=100_000)
    p.add_argument("--rows", type=int, nargs="+", default=[300_000, 1_000_000])
    p.add_argument("--cloud", type=int, default=14_300_000, help="M of part (ii)")
    p.add_argument("--network-points", type=int, default=100_000)
    p.add_argument("--network-subset", type=int, default=30_000)
    p.add_argument("--repeats", type=int, default=5)
    p.add_argument("--warmup", type=int, default=5)
    p.add_argument("--min-window", type=float, default=0.3, help="seconds per timed window")
    p.add_argument("--profiled-iterations", type=int, default=3)
    a = p.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("subset_bench needs a HIP device: there is no CPU fallback")
    from splatfields_amd.build import source_hash
    dev = torch.device("cuda:0")
    doc = {"device": torch.cuda.get_device_name(0), "torch": torch.__version__, "_source_hash": source_hash(),
           "protocol": f"one process; per comparison every side warmed up ({a.warmup} calls), then {a.repeats} alternations over the sides in the "
                       f"order listed, windows >= {a.min_window} s between device events; the first side is the baseline; launches per call "
                       f"from torch.profiler ({a.profiled_iterations} calls per side), peak device memory of one call above what was allocated "
                       "before it; (i) draws without a seed, so every call draws new rows from torch's CPU generator, and the baseline's "
                       "randperm runs on the host as the reference's does; (iii) forward + backward of the 4-D SplatFields network "
                       "(n_frames = 50, composition_rank = 40, flow_model = 'se3', fp32), the subset side including its draw and gather",
           "bookkeeping": {}, "draw": {}, "network_step": {}}
    for N in a.rows:
        doc["bookkeeping"][f"N={N},n={a.n},sh_degree=3"] = compare(bookkeeping(dev, N, a.n), a, "pytorch_reference_form", ("hip_ascending", "hip_draw_order"))
    doc["draw"][f"M={a.cloud},n={a.n}"] = compare(draws(dev, a.cloud, a.n), a, "torch_randperm_device", ("hip_draw_order", "hip_ascending"))
    doc["network_step"][f"points={a.network_points},n_splats={a.network_subset}"] = compare(
        network(dev, a.network_points, a.network_subset), a, "all_points", ("subset",))
    benchkit.write_doc(doc, a.out)
    return 0


if __name__ == "__main__":
    sys.exit(main())
