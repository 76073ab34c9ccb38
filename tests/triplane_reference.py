"""The tri-plane lookup restated in plain PyTorch (CPU, float64 or float32): the yardstick of csrc/triplane.hip on machines where
the reference checkout is absent.  tests/test_triplane_reference.py pins it to the reference's own VarTriPlaneEncoder.forward
through the fixtures tests/golden/triplane_*.npz.

Reference scene/tripFields.py:430-436, for planes [3, C, H, W] and points [..., 3]:

    coord = stack([pts[..., (0, 1)], pts[..., (1, 2)], pts[..., (2, 0)]])
    feat  = F.grid_sample(planes, coord)            bilinear, zero padding, align_corners = False: pixel = ((v + 1) S - 1) / 2
    out   = _fuse_feat(feat.permute(2, 3, 0, 1))    'cat': [.., 3 C] plane-major; 'add' AND 'mean': the sum over the planes (:423-428)

The derivative with respect to a point is discontinuous where a pixel coordinate crosses an integer (the 2 x 2 footprint moves
on by one texel): `fragile_points` names the points at which two float32 evaluations may legitimately pick different cells.
Values and the plane gradient are continuous there and are never exempted."""
from __future__ import annotations

import math
from collections import namedtuple

import torch

from tests.scan_round import SCAN_ROUND

AXES = ([0, 1], [1, 2], [2, 0])           # xy, yz, zx (reference scene/tripFields.py:399)
TENSORS = ("out", "d_planes", "d_pts")


def features(planes: torch.Tensor, pts: torch.Tensor, fuse: str = "cat") -> torch.Tensor:
    """planes [3, C, H, W], pts [B, N, 3] -> [B, N, 3 C] ('cat') or [B, N, C] ('add', 'mean'): the reference's forward."""
    coord = torch.stack([pts[..., ax] for ax in AXES])                                    # [3, B, N, 2]
    feat = torch.nn.functional.grid_sample(planes, coord, mode="bilinear", padding_mode="zeros", align_corners=False)
    feat = feat.permute(2, 3, 0, 1)                                                       # [B, N, 3, C]
    if fuse == "cat":
        return feat.reshape(feat.shape[0], feat.shape[1], -1)
    if fuse in ("add", "mean"):
        return feat.sum(dim=2)
    raise NotImplementedError(fuse)


def lookup(planes, pts, probe, dtype=torch.float64, fuse: str = "cat") -> dict:
    """out [N, F], d_planes [3, C, H, W] and d_pts [N, 3] of the loss sum(out * probe), evaluated on the CPU in `dtype` from leaf
    copies of the inputs and returned as float64.  pts [N, 3] (or [B, N, 3]: then out is [B, N, F])."""
    p = planes.detach().cpu().to(dtype).clone().requires_grad_(True)
    x = pts.detach().cpu().to(dtype).clone().requires_grad_(True)
    g = probe.detach().cpu().to(dtype)
    out = features(p, x if x.dim() == 3 else x[None], fuse)
    out = out if x.dim() == 3 else out[0]
    (out * g).sum().backward()
    return {"out": out.detach().double(), "d_planes": p.grad.double(), "d_pts": x.grad.double()}


def pixel_coordinates(pts: torch.Tensor, H: int, W: int):
    """float64 (ix, iy) [N, 3]: column p is the pixel coordinate of the point on plane p (x along W, y along H)."""
    v = pts.detach().cpu().double().reshape(-1, 3)
    ix = ((v[:, [a[0] for a in AXES]] + 1.0) * W - 1.0) / 2.0
    iy = ((v[:, [a[1] for a in AXES]] + 1.0) * H - 1.0) / 2.0
    return ix, iy


def fragile_points(pts: torch.Tensor, H: int, W: int) -> torch.Tensor:
    """bool [N]: on one of the three planes the float64 ix or iy lies within S 2^-20 of an integer (S = the plane's extent along
    that axis).  A float32 evaluation of ((v + 1) S - 1) / 2 for |v| <= 1.1 rounds v + 1 <= 2.1 (2^-23, times S), the product
    <= 2.1 S and the difference (2.1 S 2^-24 each; a fused multiply-add rounds once), then halves: less than S 2^-22 in all.
    Four times that bound is the margin, so outside this set every float32 evaluation, contracted or not, samples the same cell
    as float64.  Only dL/dpts of these points is exempt."""
    ix, iy = pixel_coordinates(pts, H, W)
    near = lambda t, s: (t - t.round()).abs() <= s * 2.0 ** -20
    return (near(ix, W) | near(iy, H)).any(dim=1)


def padded_points(pts: torch.Tensor, H: int, W: int) -> torch.Tensor:
    """bool [N]: at least one of the point's 12 corners lies outside its plane (zero padding)."""
    ix, iy = pixel_coordinates(pts, H, W)
    return ((ix < 0) | (ix > W - 1) | (iy < 0) | (iy > H - 1)).any(dim=1)


def fixed_point_resolution(gmax: float, n_points: int) -> float:
    """The contract in the header of csrc/triplane.hip: the plane gradient is summed in 64-bit fixed point whose unit is a power
    of two chosen from max |dL/dout| < 2^eg and the number of contributions a texel can receive, 4 n < 2^en, so that the worst
    case (every point on one texel) stays inside 62 bits: one unit = 2^(eg + en - 62)."""
    eg, en = math.frexp(float(gmax))[1], math.frexp(4.0 * n_points + 1.0)[1]
    return 2.0 ** (eg + en - 62)


def own_error(ref32: dict, ref64: dict, rows=None) -> dict:
    """r per tensor: max |float32 evaluation - float64 evaluation| (d_pts over `rows` only, the non-fragile points)."""
    r = {k: (ref32[k] - ref64[k]).abs() for k in TENSORS}
    if rows is not None:
        r["d_pts"] = r["d_pts"][rows]
    return {k: (v.max().item() if v.numel() else 0.0) for k, v in r.items()}


# ---- the parity cases of tests/test_gpu_triplane_edges.py (the CPU test holds the caps on fragile and padded points) ----

Case = namedtuple("Case", "name C H W N seed wide reaches")
CASES = (
    Case("c4_5x3", 4, 5, 3, 1000, 101, False, "cq = 1, plane smaller than a tile"),
    Case("c12_20x28", 12, 20, 28, 4099, 102, False, "cq = 3, ragged N, partial tiles"),
    Case("c32_16x16", 32, 16, 16, 4099, 103, False, "tile 16 at the 64 KiB LDS ceiling, exactly one tile"),
    Case("c32_33x17", 32, 33, 17, 4099, 104, False, "tile 16 at the ceiling, partial last tile in both directions"),
    Case("c36_17x33", 36, 17, 33, 4099, 105, False, "smallest C on the tile-8 path, partial tiles"),
    Case("c128_9x40", 128, 9, 40, 2053, 106, False, "tile-8 path at the 64 KiB ceiling"),
    Case("c16_1x1", 16, 1, 1, 257, 107, False, "degenerate plane"),
    Case("c8_1x64", 8, 1, 64, 1000, 108, False, "one row"),
    Case("c8_64x1", 8, 64, 1, 1000, 109, False, "one column"),
    Case("c16_24x24_wide", 16, 24, 24, 4099, 110, True, "probe rows scaled per point by 2^u, u uniform in [-30, 0]"),
    # one row of 16 x 16 tiles, 3 planes x 32 counter copies = 96 bins a tile: the first tile count whose bins exceed SCAN_ROUND
    Case(f"c4_16x{16 * (SCAN_ROUND // 96) + 1}_scan", 4, 16, 16 * (SCAN_ROUND // 96) + 1, 4099, 111, False,
         "the bin scan's second round of ordered_scan, partial last tile"),
)
SCAN_CASE = CASES[-1].name
CASE_BY_NAME = {c.name: c for c in CASES}


def make_case(case: Case, fuse: str = "cat"):
    """(planes [3, C, H, W] ~ N(0, 1), pts [N, 3] uniform in [-1.1, 1.1]^3, probe [N, F] ~ N(0, 1)), float32, on the CPU."""
    gen = torch.Generator().manual_seed(case.seed)
    planes = torch.randn(3, case.C, case.H, case.W, generator=gen)
    pts = torch.rand(case.N, 3, generator=gen) * 2.2 - 1.1
    probe = torch.randn(case.N, 3 * case.C, generator=gen)
    if case.wide:
        probe = probe * torch.exp2(-30.0 * torch.rand(case.N, 1, generator=gen))
    if fuse != "cat":
        probe = probe[:, :case.C].contiguous()
    return planes, pts, probe


_EVALUATED: dict = {}


def evaluated(name: str, fuse: str = "cat") -> dict:
    """The case's inputs, its float64 and float32 evaluations, the fragile mask and r, computed once and shared (read-only)."""
    key = (name, fuse)
    if key not in _EVALUATED:
        case = CASE_BY_NAME[name]
        planes, pts, probe = make_case(case, fuse)
        ref64, ref32 = lookup(planes, pts, probe, torch.float64, fuse), lookup(planes, pts, probe, torch.float32, fuse)
        fragile = fragile_points(pts, case.H, case.W)
        _EVALUATED[key] = {"case": case, "planes": planes, "pts": pts, "probe": probe, "f64": ref64, "f32": ref32, "fragile": fragile,
                           "r": own_error(ref32, ref64, ~fragile)}
    return _EVALUATED[key]
