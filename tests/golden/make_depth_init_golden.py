"""Writes tests/golden/depth_init_cases.npz: the outputs of the reference's OWN `_gen_3dpoints` (scene/dataset_readers.py:1476-1491)
on small inputs.  Run on a CPU where a reference checkout exists:

    python tests/golden/make_depth_init_golden.py /path/to/reference

scene/dataset_readers.py is imported as it is, through the stub packages of make_hull_golden.py (import_readers).  Nothing of the
reference's text is copied; its function is CALLED, per case and for img_idx 0 and 2 of a batch of three images,

    in float32                              as the readers call it (:1376, :1463): float32 tensors, uint8 image;
    in float64                              under torch.set_default_dtype(torch.float64) (its pixel grid follows the default dtype)
                                            with the same inputs widened.

Cases (H x W): 5x7, 64x48 and 130x70; generic cameras (a pinhole with skew seen from three poses around the origin, none aligned
with an axis), depth maps that contain 0, the readers' -1 and valid values around the camera distance.

Numbers only travel.  Per case <name>: H, W, kinv [3,4,4] and pose [3,4,4] (float64, float32-representable, so that both runs see
the same numbers), depths [3,H,W] float32, images [3,H,W,3] uint8, and per img_idx k in (0, 2): pts32_k [M,3] float32, rgb32_k
[M,3] uint8, pts64_k [M,3] float64, rgb64_k [M,3] uint8."""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from make_hull_golden import import_readers, look_at  # noqa: E402

CASES = (("img5x7", 5, 7), ("img64x48", 64, 48), ("img130x70", 130, 70))


def cameras(H, W, seed):
    """(kinv [3,4,4], pose [3,4,4]) float64 holding float32-representable numbers"""
    rng = np.random.default_rng(seed)
    kinv, pose = [], []
    for _ in range(3):
        K = np.eye(4)
        f = 1.2 * W * rng.uniform(0.9, 1.1)
        K[0, 0], K[1, 1], K[0, 1] = f, f * rng.uniform(0.95, 1.05), rng.uniform(-0.5, 0.5)
        K[0, 2], K[1, 2] = (W - 1) / 2 + rng.uniform(-1, 1), (H - 1) / 2 + rng.uniform(-1, 1)
        c = rng.normal(size=3)
        c = 3.0 * c / np.linalg.norm(c)
        c2w = np.eye(4)
        c2w[:3, :3], c2w[:3, 3] = look_at(c).T, c               # camera axes as columns, the camera centre as the origin
        kinv.append(np.linalg.inv(K).astype(np.float32).astype(np.float64))
        pose.append(c2w.astype(np.float32).astype(np.float64))
    return np.stack(kinv), np.stack(pose)


def depth_maps(H, W, seed):
    rng = np.random.default_rng(seed)
    d = rng.uniform(2.2, 3.8, (3, H, W)).astype(np.float32)
    kind = rng.uniform(size=(3, H, W))
    d[kind < 0.25] = 0.0
    d[(kind >= 0.25) & (kind < 0.5)] = -1.0
    return d


def main():
    if len(sys.argv) != 2:
        sys.exit(__doc__)
    R = import_readers(sys.argv[1])
    arrays = {}
    for n, (name, H, W) in enumerate(CASES):
        kinv, pose = cameras(H, W, 40 + n)
        depths = depth_maps(H, W, 50 + n)
        images = np.random.default_rng(60 + n).integers(0, 256, (3, H, W, 3), dtype=np.uint8)
        for k, v in (("H", np.int32(H)), ("W", np.int32(W)), ("kinv", kinv), ("pose", pose), ("depths", depths), ("images", images)):
            arrays[f"{name}/{k}"] = v
        for idx in (0, 2):
            assert torch.get_default_dtype() is torch.float32
            pts32, rgb32 = R._gen_3dpoints(idx, H, W, torch.from_numpy(kinv).float(), torch.from_numpy(pose).float(), torch.from_numpy(depths),
                                           torch.from_numpy(images[idx]))
            torch.set_default_dtype(torch.float64)
            try:
                pts64, rgb64 = R._gen_3dpoints(idx, H, W, torch.from_numpy(kinv), torch.from_numpy(pose), torch.from_numpy(depths).double(),
                                               torch.from_numpy(images[idx]))
            finally:
                torch.set_default_dtype(torch.float32)
            assert pts32.dtype == np.float32 and pts64.dtype == np.float64 and rgb32.dtype == np.uint8 and pts32.shape == pts64.shape
            assert 0 < len(pts32) < H * W
            for k, v in (("pts32", pts32), ("rgb32", rgb32), ("pts64", pts64), ("rgb64", rgb64)):
                arrays[f"{name}/{k}_{idx}"] = v
            print(name, "img_idx", idx, len(pts32), "rows, float32 against float64:", float(np.abs(pts32 - pts64).max()))
    path = os.path.join(HERE, "depth_init_cases.npz")
    np.savez_compressed(path, **arrays)
    print(path, os.path.getsize(path), "bytes,", len(arrays), "arrays")
    assert os.path.getsize(path) <= 1_000_000


if __name__ == "__main__":
    main()
