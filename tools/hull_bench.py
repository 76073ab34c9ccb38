"""What the visual-hull kernels (splatfields_amd/init.py: visual_hull, csrc/hull.hip) buy on an MI355X against
    (a) the same arithmetic as float64 PyTorch ops on the device -- what a user who ports the reference's numpy lines gets, and
    (b) the float64 numpy restatement on the host (tests/hull_reference.py) -- what the reference does today.

    python tools/hull_bench.py --out profiles/hull_bench.json
        one process; per convention ("krt", "ndc") both device sides warmed up, then five alternations pytorch / hip, every window
        timed with device events over at least --min-window seconds; then a few iterations of either side under torch.profiler for
        the launches per call, and one call each for the peak device memory.  (b) is timed once with the wall clock.  The three
        survivor lists are compared.  Writes the JSON and prints it.  Exit status 1 unless the kernels are faster than (a) in EVERY
        alternation of both conventions.

Workload: a 256^3 grid, 8 views of 800x800 around the origin, elliptical silhouettes.

Needs a HIP device; there is no CPU fallback."""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from tools import benchkit  # noqa: E402


def look_at(center, up):
    z = -center / np.linalg.norm(center)
    x = np.cross(up, z)
    x /= np.linalg.norm(x)
    return np.stack([x, np.cross(z, x), z])


def workload(convention, n_views, size, seed=3):
    """masks [V,S,S] uint8 and the matrix stack of `convention`: pinhole cameras at distance 4 with a field of view of 0.62 rad"""
    rng = np.random.default_rng(seed)
    t = np.tan(0.31)
    mats = []
    for _ in range(n_views):
        c = rng.normal(size=3)
        c = 4.0 * c / np.linalg.norm(c)
        Rw = look_at(c, rng.normal(size=3))
        Rt = np.concatenate([Rw, (-Rw @ c)[:, None]], axis=1)
        if convention == "krt":
            f = (size / 2) / t
            mats.append(np.array([[f, 0, (size - 1) / 2], [0, f, (size - 1) / 2], [0, 0, 1.0]]) @ Rt)
        else:
            w2c = np.eye(4)
            w2c[:3] = Rt
            P = np.zeros((4, 4))
            P[0, 0], P[1, 1], P[3, 2], P[2, 2], P[2, 3] = 1 / t, 1 / t, 1.0, 100.0 / 99.99, -1.0 / 99.99
            mats.append((P @ w2c).T)
    yy, xx = np.mgrid[:size, :size]
    masks = np.stack([((yy - size * rng.uniform(0.45, 0.55)) / (0.3 * size)) ** 2 + ((xx - size * rng.uniform(0.45, 0.55)) / (0.24 * size)) ** 2 <= 1.0
                      for _ in range(n_views)]).astype(np.uint8)
    return masks, np.stack(mats)


def torch_hull(masks, rows, convention, tables, G):
    """the arithmetic of csrc/hull.hip as float64 PyTorch ops on the device ("carve" policy): (int32 indices, float32 coordinates)"""
    dev = masks.device
    i = torch.arange(G ** 3, device=dev)
    ix, iy, iz = (i // G) % G, i // (G * G), i % G
    x, y, z = tables[0][ix], tables[1][iy], tables[2][iz]
    alive = torch.ones(G ** 3, dtype=torch.bool, device=dev)
    for m, mask in zip(rows, masks):
        H, W = mask.shape
        h0 = m[0, 0] * x + m[0, 1] * y + m[0, 2] * z + m[0, 3]
        h1 = m[1, 0] * x + m[1, 1] * y + m[1, 2] * z + m[1, 3]
        h2 = m[2, 0] * x + m[2, 1] * y + m[2, 2] * z + m[2, 3]
        u, v = h0 / h2, h1 / h2
        if convention == "krt":
            px = ((2.0 * (u / (W - 1.0)) - 1.0 + 1.0) / 2.0) * (W - 1.0)
            py = ((2.0 * (v / (H - 1.0)) - 1.0 + 1.0) / 2.0) * (H - 1.0)
        else:
            px, py = ((u + 1.0) * W - 1.0) * 0.5, ((v + 1.0) * H - 1.0) * 0.5
        rx, ry = torch.round(px), torch.round(py)                      # halves to even
        inside = torch.isfinite(px) & torch.isfinite(py) & (rx >= 0) & (rx <= W - 1) & (ry >= 0) & (ry <= H - 1)
        at = torch.where(inside, ry * W + rx, torch.zeros_like(rx)).long()
        alive &= inside & (mask.reshape(-1)[at] > 0)
    idx = torch.nonzero(alive).reshape(-1)
    return idx.int(), torch.stack([x[idx], y[idx], z[idx]], dim=1).float()


def alternate(steps, warmup, min_window_s, repeats, profiled):
    out, times = benchkit.alternate(steps, warmup, min_window_s, repeats, calibrate=3, digits=4, count_key="calls_per_window")
    out["speedup_median"] = round(out["pytorch"]["median_ms"] / out["hip"]["median_ms"], 2)
    out["hip_faster_in_every_alternation"] = all(b < a for a, b in zip(times["pytorch"], times["hip"]))
    benchkit.with_launches(out, steps, profiled, key="launches_per_call")
    for name, fn in steps.items():
        out[name]["peak_device_mib"] = benchkit.peak_mib(fn)
    return out


def main():
    p = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    p.add_argument("--out", default=None)
    p.add_argument("--grid", type=int, default=256)
    p.add_argument("--views", type=int, default=8)
    p.add_argument("--size", type=int, default=800)
    p.add_argument("--repeats", type=int, default=5)
    p.add_argument("--warmup", type=int, default=3)
    p.add_argument("--min-window", type=float, default=0.5, help="seconds per timed window")
    p.add_argument("--profiled-iterations", type=int, default=3)
    p.add_argument("--skip-cpu", action="store_true", help="leave (b), the numpy restatement on the host, out")
    a = p.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("hull_bench needs a HIP device: there is no CPU fallback")
    from splatfields_amd import visual_hull
    from splatfields_amd.build import source_hash
    from tests import hull_reference as R
    dev = torch.device("cuda:0")
    G, aabb = a.grid, (-1.5, 1.5)
    doc = {"device": torch.cuda.get_device_name(0), "torch": torch.__version__, "_source_hash": source_hash(),
           "workload": {"grid": G, "views": a.views, "image": [a.size, a.size], "aabb": list(aabb), "outside": "carve"},
           "protocol": f"one process; per convention both device sides warmed up ({a.warmup} calls), then {a.repeats} alternations pytorch / hip, "
                       f"windows >= {a.min_window} s between device events; every call ends with the host read of the survivor count; launches "
                       f"per call from torch.profiler, peak device memory of one call above what was allocated before it; the numpy "
                       f"restatement on the host is timed once with the wall clock",
           "conventions": {}}
    for convention in ("krt", "ndc"):
        masks_np, mats = workload(convention, a.views, a.size)
        masks = torch.from_numpy(masks_np).to(dev)
        rows = torch.from_numpy(R.rows_of(mats, convention)).to(dev)
        tables = torch.from_numpy(R.axis_tables(aabb, G)).to(dev)
        steps = {"pytorch": lambda: torch_hull(masks, rows, convention, tables, G),
                 "hip": lambda: visual_hull(masks, mats, convention=convention, grid_resolution=G, aabb=aabb, return_indices=True)}
        ti, tx = steps["pytorch"]()
        hx, hi = steps["hip"]()
        res = alternate(steps, a.warmup, a.min_window, a.repeats, a.profiled_iterations)
        res["survivors"] = int(hi.shape[0])
        res["hip_equals_pytorch"] = bool(torch.equal(ti, hi) and torch.equal(tx, hx))
        if not a.skip_cpu:
            t0 = time.perf_counter()
            want, _ = R.hull_grid(masks_np, mats, aabb, G, convention)
            res["numpy_host"] = {"seconds": round(time.perf_counter() - t0, 2)}
            res["hip_equals_numpy_host"] = bool(np.array_equal(want, hi.cpu().numpy()))
            res["speedup_over_numpy_host"] = round(res["numpy_host"]["seconds"] * 1e3 / res["hip"]["median_ms"], 1)
        doc["conventions"][convention] = res
        print(json.dumps({convention: res}), flush=True)
    doc["hip_faster_in_every_alternation_of_both_conventions"] = all(r["hip_faster_in_every_alternation"] for r in doc["conventions"].values())
    benchkit.write_doc(doc, a.out)
    return 0 if doc["hip_faster_in_every_alternation_of_both_conventions"] else 1


if __name__ == "__main__":
    sys.exit(main())
