"""float64 numpy restatement of the depth-map back-projection (the contract of include/splatraster.h `sr_depth_points_*`), written
from its description, for the tests of splatfields_amd.init.depth_points.

For image b of a batch [B,H,W] and the pixel (x, y), x in 0..W-1, y in 0..H-1 (integers, no half-pixel offset), everything in
double and every product and sum rounded on its own, each three-term sum left to right:
    p = Kinv[b,:3,:3] (x, y, 1),  v = p / sqrt(p0 p0 + p1 p1 + p2 p2),  v' = pose[b,:3,:3] v,  point = pose[b,:3,3] + depth[b,y,x] v'
A pixel is kept iff depth > 0 (0, -0, negatives and NaN are dropped, +inf is kept) and, when masks are given, mask > 0.  Rows
follow the pixels in row-major (y, x) order, image after image; the colour of a row is image[b,y,x,:] unchanged."""
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "depth_init_cases.npz")


def back_project(depths, intrinsics_inv, poses, images=None, masks=None):
    """(xyz float64 [M,3], colors [M,3] or None, flat pixel indices int64 [M])"""
    d = np.asarray(depths)
    B, H, W = d.shape
    K = np.asarray(intrinsics_inv, np.float64)[:, :3, :3]
    P = np.asarray(poses, np.float64)[:, :3, :4]
    keep = d > 0
    if masks is not None:
        m = np.asarray(masks)
        keep &= (m[..., 0] if m.ndim == 4 else m) > 0
    idx = np.nonzero(keep.reshape(-1))[0].astype(np.int64)
    b, r = idx // (H * W), idx % (H * W)
    x, y, one = (r % W).astype(np.float64), (r // W).astype(np.float64), 1.0
    dd = d.reshape(-1)[idx].astype(np.float64)
    with np.errstate(all="ignore"):
        p = [K[b, a, 0] * x + K[b, a, 1] * y + K[b, a, 2] * one for a in range(3)]
        length = np.sqrt(p[0] * p[0] + p[1] * p[1] + p[2] * p[2])
        v = [c / length for c in p]
        w = [P[b, a, 0] * v[0] + P[b, a, 1] * v[1] + P[b, a, 2] * v[2] for a in range(3)]
        xyz = np.stack([P[b, a, 3] + dd * w[a] for a in range(3)], axis=-1) if len(idx) else np.zeros((0, 3))
    colors = None if images is None else np.asarray(images).reshape(B * H * W, 3)[idx]
    return xyz, colors, idx


def ulp32(x):
    """the spacing of float32 at |x| (float64 array in, float64 out; the smallest subnormal below the normal range)"""
    m, e = np.frexp(np.abs(np.asarray(x, np.float64)))            # |x| = m 2^e, m in [0.5, 1): the binade of the double itself
    return np.ldexp(1.0, np.where(m == 0, -149, np.maximum(e - 24, -149)))


def coordinate_bound(ref64):
    """what ONE rounding to float32 of a double evaluation allows per coordinate: 0.5 ulp32(|ref64|) for the rounding, plus
    1e-12 max|ref64| for the double evaluation itself (~15 operations of relative error 1.1e-16 each, with cancellation between the
    origin and the ray bounded by the largest coordinate; four orders of magnitude of head-room, and 5 orders below the ulp term)"""
    ref64 = np.asarray(ref64, np.float64)
    top = np.max(np.abs(ref64)) if ref64.size else 0.0
    return 0.5 * ulp32(ref64) + 1e-12 * top


def golden_cases():
    """name -> dict(H, W, kinv [3,4,4], pose [3,4,4], depths [3,H,W] float32, images [3,H,W,3] uint8 and, per img_idx in (0, 2),
    pts32_<k> / rgb32_<k> (the reference in float32) and pts64_<k> / rgb64_<k> (the reference in float64))"""
    z = np.load(GOLDEN)
    cases = {}
    for key in z.files:
        name, field = key.split("/")
        cases.setdefault(name, {})[field] = z[key]
    return cases
