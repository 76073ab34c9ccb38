"""What the depth-map initialisation kernels (splatfields_amd/init.py: depth_points_bounds + depth_points, csrc/depth_init.hip) cost
on an MI355X against
    (a) the same arithmetic as the reference's back-projection (scene/dataset_readers.py:1476-1491), restated over the whole batch
        as float32 PyTorch ops on the device, the cloud materialised, then its min / max and a randperm pick -- what a user who
        moves that computation to the device gets, and
    (b) the float64 numpy restatement on the host (tests/depth_init_reference.py), timed once.

    python tools/depth_init_bench.py --out profiles/depth_init_bench.json
        one process; both device sides warmed up, then five alternations pytorch / hip, every window timed with device events over
        at least --min-window seconds; then a few iterations of either side under torch.profiler for the launches per call, the
        library's own launch count (sr_profile_collect), and one call each for the peak device memory.  Writes the JSON and prints
        it.  No speed figure is a condition: the exit status is 0 whichever side is faster, and the file says which was.

Workload: 64 depth maps of 800x800 with about 35 % valid pixels (an elliptical silhouette, -1 outside), uint8 images; both sides
end with the two bounds and 100 000 rows (coordinates and colours) on the device.

Needs a HIP device; there is no CPU fallback."""
from __future__ import annotations

import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from tests.launches import stage_counts  # noqa: E402
from tools import benchkit  # noqa: E402
from tools.hull_bench import look_at  # noqa: E402


def workload(n_images, size, seed=3):
    """(depths [B,S,S] float32, Kinv [B,3,3], pose [B,4,4] float64, images [B,S,S,3] uint8): pinhole cameras at distance 3 looking at
    the origin, depths around that distance inside an ellipse that covers about 35 % of the image, -1 outside"""
    rng = np.random.default_rng(seed)
    f = (size / 2) / np.tan(0.31)
    K = np.array([[f, 0.0, (size - 1) / 2], [0.0, f, (size - 1) / 2], [0.0, 0.0, 1.0]])
    kinv, pose = [], []
    for _ in range(n_images):
        c = rng.normal(size=3)
        c = 3.0 * c / np.linalg.norm(c)
        c2w = np.eye(4)
        c2w[:3, :3], c2w[:3, 3] = look_at(c, rng.normal(size=3)).T, c
        kinv.append(np.linalg.inv(K))
        pose.append(c2w)
    yy, xx = np.mgrid[:size, :size]
    depths = np.empty((n_images, size, size), np.float32)
    for b in range(n_images):
        inside = ((yy - size * rng.uniform(0.45, 0.55)) / (0.37 * size)) ** 2 + ((xx - size * rng.uniform(0.45, 0.55)) / (0.30 * size)) ** 2 <= 1.0
        depths[b] = np.where(inside, rng.uniform(2.5, 3.5, (size, size)), -1.0)
    images = rng.integers(0, 256, (n_images, size, size, 3), dtype=np.uint8)
    return depths, np.stack(kinv), np.stack(pose), images


def torch_cloud(depths, kinv, pose, images, n_pts):
    """the five steps of csrc/depth_init.hip (Kinv (x, y, 1), normalise, rotate, scale by the depth, add the camera centre) as
    float32 PyTorch ops over the whole batch, every intermediate a [B,H,W,3] tensor: (lo, hi, xyz [n_pts,3], rgb [n_pts,3])"""
    B, H, W = depths.shape
    dev = depths.device
    col = torch.arange(W, device=dev, dtype=torch.float32).expand(H, W)
    row = torch.arange(H, device=dev, dtype=torch.float32)[:, None].expand(H, W)
    pixel = torch.stack([col, row, torch.ones(H, W, device=dev)], dim=2)                                  # [H,W,3]: (x, y, 1)
    # either 3x3 product is a broadcast multiply and a sum over the last axis: as a matmul it would be B H W problems of 3x3
    cam = (kinv[:, None, None, :3, :3] * pixel[None, :, :, None, :]).sum(dim=4)                            # [B,H,W,3]
    unit = cam / torch.linalg.vector_norm(cam, dim=3, keepdim=True)
    world = (pose[:, None, None, :3, :3] * unit[:, :, :, None, :]).sum(dim=4)
    cloud = pose[:, None, None, :3, 3] + depths[:, :, :, None] * world
    keep = depths > 0
    xyz, rgb = cloud[keep], images[keep]
    pick = torch.randperm(xyz.shape[0], device=dev)[:n_pts]
    return xyz.min(), xyz.max(), xyz[pick], rgb[pick]


def main():
    p = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    p.add_argument("--out", default=None)
    p.add_argument("--images", type=int, default=64)
    p.add_argument("--size", type=int, default=800)
    p.add_argument("--n-pts", type=int, default=100_000)
    p.add_argument("--repeats", type=int, default=5)
    p.add_argument("--warmup", type=int, default=3)
    p.add_argument("--min-window", type=float, default=0.5, help="seconds per timed window")
    p.add_argument("--profiled-iterations", type=int, default=3)
    p.add_argument("--skip-cpu", action="store_true", help="leave (b), the numpy restatement on the host, out")
    a = p.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("depth_init_bench needs a HIP device: there is no CPU fallback")
    from splatfields_amd import depth_points, depth_points_bounds
    from splatfields_amd.build import source_hash
    from tests import depth_init_reference as R
    dev = torch.device("cuda:0")
    depths_np, kinv, pose, images_np = workload(a.images, a.size)
    depths, images = torch.from_numpy(depths_np).to(dev), torch.from_numpy(images_np).to(dev)
    kinv32, pose32 = torch.from_numpy(kinv).float().to(dev), torch.from_numpy(pose).float().to(dev)

    def hip():
        bounds = depth_points_bounds(depths, kinv, pose)
        xyz, rgb = depth_points(depths, kinv, pose, images=images, n_pts=a.n_pts)
        return bounds, xyz, rgb

    steps = {"pytorch": lambda: torch_cloud(depths, kinv32, pose32, images, a.n_pts), "hip": hip}
    lo, hi, _, _ = steps["pytorch"]()
    bounds, xyz, rgb = steps["hip"]()
    valid = int((depths > 0).sum())
    doc = {"device": torch.cuda.get_device_name(0), "torch": torch.__version__, "_source_hash": source_hash(),
           "workload": {"images": a.images, "image": [a.size, a.size], "valid_pixels": valid, "valid_share": round(valid / depths.numel(), 4),
                        "n_pts": a.n_pts, "depth_dtype": "float32", "image_dtype": "uint8"},
           "protocol": f"one process; both device sides warmed up ({a.warmup} calls), then {a.repeats} alternations pytorch / hip, windows >= "
                       f"{a.min_window} s between device events; inputs are on the device for both sides (the 3x3 and 3x4 matrices of the hip "
                       f"side on the host: their upload is part of its call); the hip side is depth_points_bounds + depth_points(n_pts), which "
                       f"ends with the host read of the count, the pytorch side is the float32 cloud, its min / max and a randperm pick; "
                       f"launches per call from torch.profiler and, for the hip side, from sr_profile_collect; peak device memory of one "
                       f"call above what was allocated before it; the numpy restatement on the host is timed once with the wall clock"}
    sides, times = benchkit.alternate(steps, a.warmup, a.min_window, a.repeats, calibrate=3, digits=4, count_key="calls_per_window")
    doc.update(benchkit.with_launches(sides, steps, a.profiled_iterations, key="launches_per_call"))
    doc["speedup_median"] = round(doc["pytorch"]["median_ms"] / doc["hip"]["median_ms"], 2)
    doc["hip_faster_in_every_alternation"] = all(b < a_ for a_, b in zip(times["pytorch"], times["hip"]))
    for name, fn in steps.items():
        doc[name]["peak_device_mib"] = benchkit.peak_mib(fn)
    doc["hip"]["library_launches_per_call"] = int(sum(stage_counts(hip)[1]))
    doc["rows"] = int(xyz.shape[0])
    doc["bounds"] = {"hip": bounds.tolist(), "pytorch_float32": [float(lo), float(hi)]}
    if not a.skip_cpu:
        t0 = time.perf_counter()
        want, _, _ = R.back_project(depths_np, kinv, pose)
        doc["numpy_host"] = {"seconds": round(time.perf_counter() - t0, 2), "rows": int(want.shape[0])}
        doc["hip_bounds_equal_numpy_host_rounded"] = bounds.tolist() == [float(np.float32(want.min())), float(np.float32(want.max()))]
        doc["speedup_over_numpy_host"] = round(doc["numpy_host"]["seconds"] * 1e3 / doc["hip"]["median_ms"], 1)
    benchkit.write_doc(doc, a.out)
    return 0


if __name__ == "__main__":
    sys.exit(main())
