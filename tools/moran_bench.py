"""What the fused Moran's I regulariser (splatfields_amd/moran.py) costs on an MI355X, against a PyTorch restatement of the
reference's `query_nn` + four `morans_loss` calls (extract_geo.py:100-143, train.py:203-210) that takes its neighbour indices
from our k-NN -- pytorch3d does not exist for ROCm, so that is the only way the reference's form runs here at all.

    python tools/moran_bench.py --out profiles/moran_bench.json
        100 000 and 300 000 points with the four reference tensors (3, 4, 1, 48 channels), forward + backward, neighbour
        search included on both sides: both warmed up, then five alternations restated / fused, every window timed with
        device events over at least 0.5 s; peak memory of each side.  Writes the JSON and prints it.
    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -o r -- python tools/moran_bench.py --trace fused --points N
        a run of its own for the profiler: --iters iterations, nothing else.
    python tools/moran_bench.py --merge 100000=DIR 300000=DIR --out profiles/moran_bench.json
        adds launches per iteration and the kernel times split into k-NN / forward / backward, and the kernels' algorithmic
        bytes over their time as a share of the HBM and Infinity-Cache rates.

Needs a HIP device; there is no CPU fallback."""
from __future__ import annotations

import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

from tools import benchkit  # noqa: E402

HBM_PEAK = 8.0e12            # bytes / s (specification)
GATHER_INFINITY_CACHE = 8.6e12   # bytes / s: random 1 KiB rows of a 38 MB table gathered chip-wide (measured figure of the kernel guide)
WIDTHS = (3, 4, 1, 48)
K = 5


def inputs(n, dev):
    from tests import moran_reference as R
    points = R.cloud("uniform", n, 44)
    features = R.smooth_features(points, WIDTHS, 0.5, 51, wavelength=0.2)
    return points.to(dev), [f.to(dev) for f in features]


def restated_query_nn(pts, nn_ix, eps=1e-5):
    """extract_geo.py:104-108 with the indices given"""
    d = torch.cdist(pts[nn_ix], pts[nn_ix])
    w = torch.full_like(d, eps)
    w[d > eps] = 1.0 / d[d > eps]
    return w / w.sum(-1).sum(-1)[:, None, None].clamp_min(1e-5)


def restated_morans_loss(weight, feature):
    """extract_geo.py:111-143: the [B, F, n, n] products are materialised, as there"""
    n = feature.shape[1]
    w_ij = (n / weight.sum(-1).sum(-1)[:, None, None]) * weight
    denom = (feature ** 2).sum(dim=1)
    x = feature.permute(0, 2, 1)                                   # B x F x n
    corr = x.unsqueeze(-1) * x.unsqueeze(-2)                       # B x F x n x n
    moran = (w_ij.unsqueeze(1) * corr).sum(-1).sum(-1) / (denom + 1e-4)
    return 1.0 - moran.mean().clamp(0, 1)


def steps(n, dev):
    """-> {"restated": fn, "fused": fn}: neighbour search + the four terms + backward, one call each"""
    from splatfields_amd.moran import knn_graph, moran_loss
    points, features = inputs(n, dev)
    p = points.clone().requires_grad_(True)
    feats = [f.clone().requires_grad_(True) for f in features]

    def clear():
        p.grad = None
        for f in feats:
            f.grad = None

    def restated():
        clear()
        nn_ix = knn_graph(p, K).nn_ix.long()
        weights = restated_query_nn(p, nn_ix)
        sum(restated_morans_loss(weights, f[nn_ix]) for f in feats).backward()

    def fused():
        clear()
        moran_loss(p, feats, K)[0].backward()

    return {"restated": restated, "fused": fused}


def alternate(both, warmup, min_window_s, repeats):
    """Both sides warmed up, then `repeats` alternations; every window lasts at least `min_window_s`.  A side that runs out of
    memory is recorded as such."""
    iters, peak, failed = {}, {}, {}
    for name, fn in both.items():
        torch.cuda.synchronize()
        torch.cuda.empty_cache()
        torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        try:
            for _ in range(warmup):
                fn()
            per = benchkit.window_ms(fn, 3)
        except torch.cuda.OutOfMemoryError as e:
            failed[name] = f"out of memory: {str(e).splitlines()[0]}"
            continue
        iters[name] = max(3, int(min_window_s * 1e3 / per) + 1)
        peak[name] = {"peak_bytes": torch.cuda.max_memory_allocated(), "resident_inputs_bytes": base}
    times = {name: [] for name in iters}
    for _ in range(repeats):
        for name in iters:
            times[name].append(benchkit.window_ms(both[name], iters[name]))
    out = {}
    for name, ts in times.items():
        out[name] = {**benchkit.window_stats(ts, iters[name], 5, "iterations_per_window"), **peak[name]}
    for name, why in failed.items():
        out[name] = {"failed": why}
    if "restated" in times and "fused" in times:
        r, f = out["restated"], out["fused"]
        out["speedup_median"] = round(r["median_ms"] / f["median_ms"], 3)
        out["fused_faster_in_every_repetition"] = f["max_ms"] < r["min_ms"]     # worst fused < best restated
        out["fused_peak_memory_is_lower"] = f["peak_bytes"] < r["peak_bytes"]
    return out


def algorithmic_bytes(n):
    """Bytes each kernel must move once, from the shapes: positions, K gathered rows of every tensor, gradients."""
    c = sum(WIDTHS)
    gathered = n * K * (12 + 4 * c) + n * K * 4                    # K positions and K rows per point, and their indices
    edges = n * K * (c + 3) * 4                                    # the per-edge contributions
    return {"forward": gathered, "backward_edges": gathered + edges, "backward_collect": edges + n * K * 4 + n * (c + 3) * 4,
            "feature_table_bytes": n * c * 4}


GROUPS = (("forward", ("k_moran_forward", "k_moran_reduce")), ("backward_edges", ("k_moran_edges",)), ("backward_collect", ("k_moran_collect",)),
          ("knn", ("k_knn_", "k_rank_segments", "k_rev_")))


def merge(pairs, out_path, iters_total):
    doc = json.load(open(out_path))
    traces = {}
    for item in pairs:
        n, directory = item.split("=", 1)
        rows = benchkit.read_stats(directory)
        by = algorithmic_bytes(int(n))
        entry = {"launches_per_iteration": round(sum(c for _, c, _, _ in rows) / iters_total, 2),
                 "kernel_us_per_iteration": round(sum(t for _, _, _, t in rows) / iters_total / 1e3, 3), "iterations_traced": iters_total,
                 "groups": {}}
        for label, keys in GROUPS:
            hit = [r for r in rows if any(k in r[0] for k in keys)]
            us = sum(t for _, _, _, t in hit) / iters_total / 1e3
            g = {"us_per_iteration": round(us, 3), "launches_per_iteration": round(sum(c for _, c, _, _ in hit) / iters_total, 2)}
            if label in by and us > 0:
                g.update(algorithmic_bytes=by[label], bytes_per_s=round(by[label] / (us * 1e-6), 1),
                         share_of_hbm_peak=round(by[label] / HBM_PEAK / (us * 1e-6), 4),
                         share_of_infinity_cache_gather_rate=round(by[label] / GATHER_INFINITY_CACHE / (us * 1e-6), 4))
            entry["groups"][label] = g
        other = [r for r in rows if not any(k in r[0] for _, keys in GROUPS for k in keys)]
        entry["groups"]["other (torch)"] = {"us_per_iteration": round(sum(t for _, _, _, t in other) / iters_total / 1e3, 3),
                                            "launches_per_iteration": round(sum(c for _, c, _, _ in other) / iters_total, 2)}
        traces[n] = entry
    doc["kernel_trace_fused"] = traces
    benchkit.write_doc(doc, out_path)


def main():
    p = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    p.add_argument("--out", default=None)
    p.add_argument("--sizes", type=int, nargs="+", default=[100_000, 300_000])
    p.add_argument("--repeats", type=int, default=5)
    p.add_argument("--min-window", type=float, default=0.5, help="seconds per timed window")
    p.add_argument("--trace", choices=["fused", "restated"], default=None)
    p.add_argument("--points", type=int, default=300_000)
    p.add_argument("--iters", type=int, default=50)
    p.add_argument("--merge", nargs="+", default=None, metavar="POINTS=DIR")
    a = p.parse_args()
    if a.merge:
        return merge(a.merge, a.out, a.iters)
    if not torch.cuda.is_available():
        raise SystemExit("moran_bench needs a HIP device: there is no CPU fallback")
    dev = torch.device("cuda:0")
    if a.trace:
        fn = steps(a.points, dev)[a.trace]
        for _ in range(a.iters):
            fn()
        torch.cuda.synchronize()
        return
    import gc
    gc.collect()
    gc.disable()
    doc = {"device": torch.cuda.get_device_name(0), "protocol": f"device events, windows >= {a.min_window} s, {a.repeats} alternations "
           "restated / fused in one process after warming up both; neighbour search (ours) + four terms + backward on both sides",
           "widths": list(WIDTHS), "n_neighbors": K, "sizes": {}}
    for n in a.sizes:
        doc["sizes"][str(n)] = dict(algorithmic_bytes=algorithmic_bytes(n), **alternate(steps(n, dev), 5, a.min_window, a.repeats))
        print(json.dumps({n: doc["sizes"][str(n)]}), flush=True)
    benchkit.write_doc(doc, a.out)


if __name__ == "__main__":
    main()
