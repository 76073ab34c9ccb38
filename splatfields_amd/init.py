"""Initialisation on the device: masks, depth maps and cameras in, trainable splat tensors out.  The visual hull first; the
back-projection of the depth maps that gives the hull its box, or the initial cloud itself, stands below it (`depth_points`).

Replaces the hull test of reference scene/dataset_readers.py -- :1385-1417 (`visual_hull_samples`), :1419-1458
(`visual_hull_samples_list`), :605-644 (the Blender `hull` branch of `readNerfSyntheticInfo`) and :544-588 (its `load` branch) --
and the tensor construction of `GaussianModel.create_from_pcd` (scene/gaussian_model.py:95-121) behind it.

Two pixel mappings (``convention``), both evaluated in double in the reference's order of operations (csrc/hull.hip):

  ``"krt"``  matrices [V,3,4] = the reference's ``KRT``; h = KRT [p;1], u = h0/h2, the normalisation to [-1, 1] and
             ``grid_sample``'s un-normalisation with ``align_corners=True`` are both kept: px = ((2 (u/(W-1)) - 1 + 1)/2) (W-1).
  ``"ndc"``  matrices [V,4,4] = ``full_proj_transform`` in the reference's transposed storage (scene/cameras.py:68-73:
             clip = [p 1] @ M); columns 0, 1 and 2 are used, so the divisor is clip z, not w, as at :625.  px = ((u+1) W - 1) / 2,
             py = ((v+1) H - 1) / 2.  The reference swaps H and W in both the scale and the bounds test, which is only
             well-defined for square images: this mapping equals the reference's for square images.

The nearest pixel is ``rint`` (halves to even, what ``np.round`` and ``grid_sample`` do).  A voxel survives a view iff that pixel
is inside the image and ``mask > 0`` there; there is no test on the sign of h2 (the reference has none: a voxel behind a camera that
projects into the mask survives).  ``outside="carve"``: a voxel outside the image is carved (`visual_hull_samples`, both Blender
branches); ``outside="keep"``: a view keeps a voxel whose normalised coordinate lies outside [-1, 1]
(`visual_hull_samples_list` :1443,1450).  Non-finite pixel coordinates are carved under both.

There is no CPU path: a missing library or a CPU device is an error."""
from __future__ import annotations

from typing import Optional, Sequence

import numpy as np
import torch

from . import _lib
from ._lib import ptr

_CONVENTIONS = {"krt": _lib.HULL_KRT, "ndc": _lib.HULL_NDC}
_OUTSIDE = {"carve": _lib.HULL_OUTSIDE_CARVE, "keep": _lib.HULL_OUTSIDE_KEEP}
SH_C0 = 0.28209479177387814


def _device_of(*things, device=None) -> torch.device:
    if device is not None:
        return torch.device(device)
    for t in things:
        for item in (t if isinstance(t, (list, tuple)) else (t,)):
            if torch.is_tensor(item) and item.is_cuda:
                return item.device
    return torch.device("cuda", torch.cuda.current_device())


def _mask_items(masks) -> list:
    """[V,H,W(,1)] tensor / array, or a list of [H_i,W_i(,1)] items -> list of 2-D items"""
    items = list(masks) if isinstance(masks, (list, tuple)) else [masks[k] for k in range(len(masks))]
    out = []
    for m in items:
        m = m if torch.is_tensor(m) else torch.from_numpy(np.ascontiguousarray(m))
        if m.dim() == 3 and m.shape[-1] == 1:
            m = m[..., 0]
        if m.dim() != 2:
            raise ValueError("every mask must be [H, W] or [H, W, 1]")
        out.append(m)
    return out


def _view_table(masks, matrices, convention: str, outside: str, dev):
    """the host table of SrHullView records and the flat uint8 buffer (mask > 0) on the device"""
    if convention not in _CONVENTIONS:
        raise ValueError(f"convention must be 'krt' or 'ndc', not {convention!r}")
    if outside not in _OUTSIDE:
        raise ValueError(f"outside must be 'carve' or 'keep', not {outside!r}")
    items = _mask_items(masks)
    mats = matrices.detach().cpu().numpy() if torch.is_tensor(matrices) else np.asarray(matrices)
    mats = mats.astype(np.float64)
    if convention == "krt":
        if mats.ndim != 3 or mats.shape[1:] != (3, 4):
            raise ValueError("convention 'krt' takes matrices of shape [V, 3, 4]")
        rows = mats
    else:
        if mats.ndim != 3 or mats.shape[1:] != (4, 4):
            raise ValueError("convention 'ndc' takes full_proj_transform matrices of shape [V, 4, 4]")
        rows = np.ascontiguousarray(mats[:, :, :3].transpose(0, 2, 1))       # columns 0, 1, 2 of [p 1] @ M as rows of M' [p;1]
    if len(items) != rows.shape[0]:
        raise ValueError(f"{len(items)} masks for {rows.shape[0]} matrices")
    if not 1 <= len(items) <= _lib.HULL_MAX_VIEWS:
        raise ValueError(f"between 1 and {_lib.HULL_MAX_VIEWS} views are supported, not {len(items)}")
    table = (_lib.SrHullView * len(items))()
    offset = 0
    for k, m in enumerate(items):
        rec = table[k]
        rec.m[:] = rows[k].reshape(-1).tolist()
        rec.mask_offset, rec.height, rec.width = offset, int(m.shape[0]), int(m.shape[1])
        rec.convention, rec.outside = _CONVENTIONS[convention], _OUTSIDE[outside]
        offset += int(m.shape[0]) * int(m.shape[1])
    flat = torch.cat([(m.to(dev) > 0).reshape(-1) for m in items]).to(torch.uint8).contiguous()
    return table, flat


def _carve(table, flat, grid, G, points, n, dev):
    """sr_hull_carve -> (workspace, device count); nothing waits"""
    lib = _lib.load()
    ws = torch.empty(lib.sr_hull_workspace_bytes(n), dtype=torch.uint8, device=dev)
    count = torch.zeros(1, dtype=torch.int32, device=dev)
    _lib.check(lib.sr_hull_carve(len(table), table, ptr(flat), flat.numel(), ptr(grid), G, ptr(points), 0 if points is None else n,
                                 int(points is not None and points.dtype is torch.float64), ptr(ws), ptr(count), _lib.stream(dev)))
    return ws, count


def _gather(grid, G, points, n, ws, capacity, dev, want_points=True):
    lib = _lib.load()
    idx = torch.empty(capacity, dtype=torch.int32, device=dev)
    xyz = torch.empty(capacity, 3, dtype=torch.float32, device=dev) if want_points else None
    _lib.check(lib.sr_hull_gather(ptr(grid), G, ptr(points), 0 if points is None else n,
                                  int(points is not None and points.dtype is torch.float64), ptr(ws), capacity, ptr(idx), ptr(xyz),
                                  _lib.stream(dev)))
    return idx, xyz


def _axis_tables(aabb, G: int) -> np.ndarray:
    """[3, G] float64: np.linspace per axis.  aabb = (lo, hi) for a cube (the reference's), or ((lo_x, lo_y, lo_z), (hi_x, hi_y, hi_z))"""
    lo, hi = aabb
    lo = np.broadcast_to(np.asarray(lo, np.float64), (3,))
    hi = np.broadcast_to(np.asarray(hi, np.float64), (3,))
    return np.stack([np.linspace(lo[a], hi[a], G) for a in range(3)])


def visual_hull(masks, matrices, *, convention: str = "krt", outside: str = "carve", grid_resolution: int = 256, aabb=(-1., 1.),
                n_pts: Optional[int] = None, generator: Optional[torch.Generator] = None, return_indices: bool = False,
                capacity: Optional[int] = None, draw: str = "permutation", device=None):
    """The voxels of a ``grid_resolution``^3 grid over ``aabb`` that every view keeps: float32 [M,3] on the device, in grid order
    (linear index (iy G + ix) G + iz at (g[ix], g[iy], g[iz]): the order of ``np.meshgrid(g, g, g)`` flattened, g =
    ``np.linspace(*aabb, G)`` made on the host in float64 and uploaded).

    masks: [V,H,W] or [V,H,W,1] tensor / array of any dtype (``> 0`` is inside), or a list of [H_i,W_i(,1)] items of different
    sizes.  matrices: see the module docstring.  aabb: (lo, hi), or a pair of 3-vectors for a non-cubic box.

    One host read, of the survivor count: it is inherent in an output whose size depends on the data.  ``capacity`` (an upper
    bound the caller knows) replaces nothing of that read; it only bounds the rows written -- an ordered prefix when it is short.

    n_pts: keep ``torch.randperm(M, generator=generator)[:n_pts]`` of the rows, drawn on the device -- a uniform subset without
    replacement, as the reference's ``np.random.shuffle(...)[:n_pts]`` and ``np.random.choice(..., replace=False)`` are; numpy's
    random streams themselves cannot be reproduced.  draw="keyed": the rows are picked by `splatfields_amd.subset.draw_rows(M,
    n_pts, generator=generator)` instead (a CPU generator or None; draw order): a uniform subset as well, at a cost and a memory
    that scale with n_pts, not with M.  return_indices: also return the int32 linear indices of the rows."""
    dev = _device_of(masks, matrices, device=device)
    if dev.type != "cuda":
        raise RuntimeError("splatfields_amd.init has no CPU path: the device must be a HIP ('cuda') device")
    G = int(grid_resolution)
    if G < 1 or G ** 3 > 2 ** 31 - 1:
        raise ValueError("grid_resolution must be at least 1 with grid_resolution^3 <= 2^31 - 1")
    _check_draw(draw)
    with torch.cuda.device(dev):
        table, flat = _view_table(masks, matrices, convention, outside, dev)
        grid = torch.from_numpy(_axis_tables(aabb, G)).to(dev).contiguous()
        ws, count = _carve(table, flat, grid, G, None, G ** 3, dev)
        m = int(count.item())                                  # the one host read
        rows = m if capacity is None else min(m, int(capacity))
        idx, xyz = _gather(grid, G, None, G ** 3, ws, rows, dev)
        if n_pts is not None and rows > n_pts:
            pick = _pick_rows(rows, n_pts, generator, draw, dev).to(dev)
            idx, xyz = idx[pick], xyz[pick]
    return (xyz, idx) if return_indices else xyz


def _check_draw(draw: str) -> None:
    if draw not in ("permutation", "keyed"):
        raise ValueError(f"draw must be 'permutation' or 'keyed', not {draw!r}")


def _pick_rows(rows: int, n_pts: int, generator, draw: str, dev) -> torch.Tensor:
    """n_pts of `rows` row numbers: the head of a permutation of all of them, or the keyed draw of subset.draw_rows"""
    if draw == "keyed":
        from .subset import draw_rows
        return draw_rows(rows, n_pts, generator=generator, device=dev)
    gen_dev = dev if generator is None else generator.device
    return torch.randperm(rows, generator=generator, device=gen_dev)[:n_pts]


def hull_filter(points, masks, matrices, *, convention: str = "krt", outside: str = "carve", device=None) -> torch.Tensor:
    """[N] bool on the device: which rows of ``points`` [N,3] (float32 or float64, widened to double) every view keeps -- the
    reference's `load` branch (scene/dataset_readers.py:544-588: ``xyz[xyz_mask]``) with ``convention="ndc"``.  One host read (the
    count)."""
    dev = _device_of(points, masks, device=device)
    if dev.type != "cuda":
        raise RuntimeError("splatfields_amd.init has no CPU path: the device must be a HIP ('cuda') device")
    pts = points if torch.is_tensor(points) else torch.from_numpy(np.ascontiguousarray(points))
    if pts.dim() != 2 or pts.shape[1] != 3:
        raise ValueError("points must be [N, 3]")
    if pts.dtype is not torch.float64:
        pts = pts.to(torch.float32)
    pts = pts.detach().to(dev).contiguous()
    n = pts.shape[0]
    keep = torch.zeros(n, dtype=torch.bool, device=dev)
    if n == 0:
        return keep
    with torch.cuda.device(dev):
        table, flat = _view_table(masks, matrices, convention, outside, dev)
        ws, count = _carve(table, flat, None, 0, pts, n, dev)
        idx, _ = _gather(None, 0, pts, n, ws, int(count.item()), dev, want_points=False)
        keep[idx.long()] = True
    return keep


def _samples(masks, KRT, n_pts, grid_resolution, aabb, outside):
    xyz, idx = visual_hull(masks, KRT, convention="krt", outside=outside, grid_resolution=grid_resolution, aabb=aabb, return_indices=True)
    idx = idx[torch.randperm(idx.shape[0], device=idx.device)[:n_pts]].cpu().numpy().astype(np.int64)
    G = int(grid_resolution)
    g = _axis_tables(aabb, G)
    return np.stack([g[0][(idx // G) % G], g[1][idx // (G * G)], g[2][idx % G]], axis=-1)   # float64 rows of the reference's grid_loc


def visual_hull_samples(masks, KRT, n_pts=100_000, grid_resolution=256, aabb=(-1., 1.)):
    """Drop-in for reference scene/dataset_readers.py:1385-1417: numpy in, float64 numpy [<= n_pts, 3] out, shuffled (a uniform
    subset without replacement; not numpy's stream)."""
    return _samples(masks, KRT, n_pts, grid_resolution, aabb, "carve")


def visual_hull_samples_list(masks_list, KRT, n_pts=100_000, grid_resolution=256, aabb=(-1., 1.)):
    """Drop-in for reference scene/dataset_readers.py:1419-1458 (masks of different sizes; a voxel outside a view is kept by it)."""
    return _samples(list(masks_list), KRT, n_pts, grid_resolution, aabb, "keep")


def hull_matrices(cameras: Sequence, convention: str = "krt") -> np.ndarray:
    """The matrix stack of `visual_hull` from camera objects: ``cam.KRT`` [3,4] each for "krt", ``cam.full_proj_transform`` [4,4]
    (the reference's transposed storage, scene/cameras.py:68-73) each for "ndc".  float64 numpy."""
    name = {"krt": "KRT", "ndc": "full_proj_transform"}.get(convention)
    if name is None:
        raise ValueError(f"convention must be 'krt' or 'ndc', not {convention!r}")
    mats = []
    for cam in cameras:
        m = getattr(cam, name)
        mats.append(m.detach().cpu().double().numpy() if torch.is_tensor(m) else np.asarray(m, np.float64))
    return np.stack(mats)


# ---- depth-map initialisation (csrc/depth_init.hip) --------------------------------------------------------------------------
# Replaces `_gen_3dpoints` of reference scene/dataset_readers.py:1476-1491 (called per camera and frame at :1376 and :1463) and
# what `readNeuSceneInfo` takes from the concatenated cloud: its bounds (:1603-1613) or `num_pts` random rows (:1653-1658).
# For image b and the pixel (x, y), integers: p = Kinv[b,:3,:3] (x, y, 1), v = p / |p|, point = pose[b,:3,3] + depth[b,y,x]
# pose[b,:3,:3] v, in double, rounded to float32 once.  A pixel is kept iff depth > 0 (and mask > 0 when masks are given); rows
# follow the pixels in row-major (y, x) order, image after image.

def _host64(a, name, shapes):
    a = a.detach().cpu().numpy() if torch.is_tensor(a) else np.asarray(a)
    if a.ndim != 3 or a.shape[1:] not in shapes:
        raise ValueError(f"{name} must be " + " or ".join(f"[B, {s[0]}, {s[1]}]" for s in shapes))
    return a.astype(np.float64)


class _DepthBatch:
    """the arguments every sr_depth_points_* call shares, on the device"""

    def __init__(self, depths, intrinsics_inv, poses, images, masks, dev):
        d = depths if torch.is_tensor(depths) else torch.from_numpy(np.ascontiguousarray(depths))
        if d.dim() != 3:
            raise ValueError("depths must be [B, H, W]")
        if d.dtype is not torch.float64:
            d = d.to(torch.float32)
        self.depths = d.detach().to(dev).contiguous()
        self.B, self.H, self.W = (int(s) for s in d.shape)
        if self.H < 1 or self.W < 1:
            raise ValueError("H and W must be at least 1")
        if self.B * self.H * self.W > 2 ** 31 - 1:
            raise ValueError("B H W must not exceed 2^31 - 1: split the batch")
        kinv = _host64(intrinsics_inv, "intrinsics_inv", ((3, 3), (4, 4)))[:, :3, :3]
        pose = _host64(poses, "poses", ((3, 4), (4, 4)))[:, :3, :4]
        if kinv.shape[0] != self.B or pose.shape[0] != self.B:
            raise ValueError(f"{self.B} depth maps for {kinv.shape[0]} intrinsics and {pose.shape[0]} poses")
        table = np.concatenate([kinv.reshape(self.B, 9), pose.reshape(self.B, 12)], axis=1)          # SrDepthCamera records
        self.cameras = torch.from_numpy(np.ascontiguousarray(table)).to(dev)
        self.masks = None
        if masks is not None:
            m = masks if torch.is_tensor(masks) else torch.from_numpy(np.ascontiguousarray(masks))
            if m.dim() == 4 and m.shape[-1] == 1:
                m = m[..., 0]
            if tuple(m.shape) != (self.B, self.H, self.W):
                raise ValueError("masks must be [B, H, W] or [B, H, W, 1]")
            self.masks = (m.to(dev) > 0).to(torch.uint8).contiguous()
        self.images = None
        if images is not None:
            im = images if torch.is_tensor(images) else torch.from_numpy(np.ascontiguousarray(images))
            if tuple(im.shape) != (self.B, self.H, self.W, 3):
                raise ValueError("images must be [B, H, W, 3]")
            if im.element_size() not in (1, 4, 8):
                raise ValueError(f"images of {im.dtype} are not supported: the element size must be 1, 4 or 8 bytes")
            self.images = im.detach().to(dev).contiguous()
        self.dev = dev

    @property
    def n(self):
        return self.B * self.H * self.W

    def head(self):
        return (self.B, self.H, self.W, _lib.depth_cameras_arg(self.cameras), ptr(self.depths), int(self.depths.dtype is torch.float64))

    def mark(self, want_count=True, want_bounds=False):
        """sr_depth_points_mark -> (workspace, device count or None, device bounds or None); nothing waits.  B >= 1: the scan
        launch writes both words"""
        lib = _lib.load()
        ws = torch.empty(lib.sr_depth_points_workspace_bytes(self.n), dtype=torch.uint8, device=self.dev)
        count = torch.empty(1, dtype=torch.int32, device=self.dev) if want_count else None
        bounds = torch.empty(2, dtype=torch.float32, device=self.dev) if want_bounds else None
        _lib.check(lib.sr_depth_points_mark(*self.head(), ptr(self.masks), ptr(ws), ptr(count), ptr(bounds), _lib.stream(self.dev)))
        return ws, count, bounds

    def _outputs(self, rows, want_indices):
        xyz = torch.empty(rows, 3, dtype=torch.float32, device=self.dev)
        colors = None if self.images is None else torch.empty(rows, 3, dtype=self.images.dtype, device=self.dev)
        idx = torch.empty(rows, dtype=torch.int64, device=self.dev) if want_indices else None
        return xyz, colors, idx

    def _images_arg(self):
        return (ptr(self.images), 0 if self.images is None else self.images.element_size())

    def gather(self, ws, rows, want_indices=False):
        xyz, colors, idx = self._outputs(rows, want_indices)
        _lib.check(_lib.load().sr_depth_points_gather(*self.head(), *self._images_arg(), ptr(ws), rows, ptr(xyz), ptr(colors), ptr(idx),
                                                      _lib.stream(self.dev)))
        return xyz, colors, idx

    def select(self, ws, ranks, want_indices=False):
        """rows ranks[j] of the cloud and the device flag word (1 when a rank was out of range)"""
        ranks = ranks.detach().to(self.dev, torch.int64).contiguous()
        xyz, colors, idx = self._outputs(ranks.numel(), want_indices)
        flag = torch.zeros(1, dtype=torch.int32, device=self.dev)
        _lib.check(_lib.load().sr_depth_points_select(*self.head(), *self._images_arg(), ptr(ws), ptr(ranks), ranks.numel(), ptr(xyz),
                                                      ptr(colors), ptr(idx), ptr(flag), _lib.stream(self.dev)))
        return xyz, colors, idx, flag


def _depth_device(device, *things):
    dev = _device_of(*things, device=device)
    if dev.type != "cuda":
        raise RuntimeError("splatfields_amd.init has no CPU path: the device must be a HIP ('cuda') device")
    return dev


def depth_points(depths, intrinsics_inv, poses, *, images=None, masks=None, n_pts: Optional[int] = None,
                 generator: Optional[torch.Generator] = None, ranks=None, capacity: Optional[int] = None, return_indices: bool = False,
                 return_flag: bool = False, draw: str = "permutation", device=None):
    """The back-projected pixels of a batch of depth maps: ``(xyz float32 [M,3], colors [M,3] or None[, indices int64 [M]])`` on the
    device, in pixel order (image after image, row-major inside an image); ``indices`` are the flat pixel indices b H W + y W + x.

    depths: [B,H,W], float32 or float64 (anything else is converted to float32); intrinsics_inv: [B,3,3] or [B,4,4]; poses
    (camera to world): [B,3,4] or [B,4,4], both widened to float64 on the host; images: [B,H,W,3] of 1-, 4- or 8-byte elements,
    copied unchanged; masks: [B,H,W] or [B,H,W,1] of any dtype, ``> 0`` is inside -- the reader's ``depths[~(mask > 0)] = -1``
    (:1325) without rewriting the depth maps.  Tensors or numpy arrays.

    A full gather needs one host read, of the count.  ``capacity`` bounds the rows written: an ordered prefix when it is short.
    n_pts: keep ``torch.randperm(M, generator=generator)[:n_pts]`` of the rows (the convention of `visual_hull`), picked by rank
    on the device without materialising the cloud; draw="keyed": the ranks come from `splatfields_amd.subset.draw_rows(M, n_pts,
    generator=generator)` instead of the permutation of M (a CPU generator or None), through the same selection.  ranks: the caller's own draw instead, an int64 sequence of any order, repeats
    allowed: row j is survivor number ranks[j], and nothing is read back; a rank outside [0, M) gives a row of NaN coordinates,
    zero colours and the index -1.  return_flag (with ranks only): the select kernel's report is appended to the result, an int32
    [1] device tensor that is 1 when any rank was outside [0, M) and 0 otherwise -- still no host read."""
    dev = _depth_device(device, depths, images, masks)
    if ranks is not None and (n_pts is not None or capacity is not None):
        raise ValueError("ranks excludes n_pts and capacity")
    if return_flag and ranks is None:
        raise ValueError("return_flag needs ranks: only the caller's own ranks can be out of range")
    _check_draw(draw)
    flag = None
    with torch.cuda.device(dev):
        b = _DepthBatch(depths, intrinsics_inv, poses, images, masks, dev)
        if b.B == 0:
            if ranks is not None and len(ranks):
                raise ValueError("an empty batch has no row to select")
            out = b._outputs(0, return_indices)
            flag = torch.zeros(1, dtype=torch.int32, device=dev) if return_flag else None
        elif ranks is not None:
            r = ranks if torch.is_tensor(ranks) else torch.as_tensor(np.asarray(ranks, np.int64))
            ws, _, _ = b.mark()
            *out, flag = b.select(ws, r.reshape(-1), return_indices)
        else:
            ws, count, _ = b.mark()
            m = int(count.item())                                  # the one host read
            rows = m if capacity is None else min(m, int(capacity))
            if n_pts is not None and rows > n_pts:
                out = b.select(ws, _pick_rows(rows, n_pts, generator, draw, dev), return_indices)[:3]
            else:
                out = b.gather(ws, rows, return_indices)
    out = tuple(out) if return_indices else tuple(out[:2])
    return out + (flag,) if return_flag else out


def depth_points_bounds(depths, intrinsics_inv, poses, *, masks=None, as_aabb: bool = False, device=None):
    """(lo, hi): the smallest and the largest coordinate of `depth_points`' cloud, all three components together -- the reference's
    ``all_pc[0].min(), all_pc[0].max()`` (:1607) -- as a float32 [2] device tensor, with no host read and no cloud.  (+inf, -inf)
    when no pixel is valid; a NaN coordinate (possible only where the depth is +inf) takes no part.  as_aabb=True: the pair of
    Python floats `visual_hull(aabb=...)` takes, with one read."""
    dev = _depth_device(device, depths, masks)
    with torch.cuda.device(dev):
        b = _DepthBatch(depths, intrinsics_inv, poses, None, masks, dev)
        if b.B == 0:
            bounds = torch.tensor([float("inf"), float("-inf")], dtype=torch.float32, device=dev)
        else:
            bounds = b.mark(want_count=False, want_bounds=True)[2]
    if as_aabb:
        lo, hi = bounds.tolist()
        return lo, hi
    return bounds


def gen_3dpoints(img_idx, H, W, intrinsics_all_inv, pose_all, depths, image):
    """Drop-in for reference scene/dataset_readers.py:1476-1491: the same arguments (``depths`` [n_images,H,W], ``image`` [H,W,3] of
    image ``img_idx``), ``(pts float32 [M,3], rgb [M,3])`` as numpy arrays."""
    d, k, p = depths[img_idx], intrinsics_all_inv[img_idx], pose_all[img_idx]
    if tuple(d.shape) != (H, W):
        raise ValueError(f"depths[{img_idx}] is {tuple(d.shape)}, not ({H}, {W})")
    xyz, rgb = depth_points(d[None], k[None], p[None], images=image[None])
    return xyz.cpu().numpy(), rgb.cpu().numpy()


def depth_point_cloud(depths, intrinsics_inv, poses, images, num_pts: int, *, masks=None, generator: Optional[torch.Generator] = None,
                      device=None):
    """The `depth` branch of `readNeuSceneInfo` (reference scene/dataset_readers.py:1653-1658): at most ``num_pts`` rows of the
    back-projected cloud, a uniform subset without replacement, as ``(xyz float32 [n,3], colors float32 [n,3])`` on the device for
    `splats_from_points`.  uint8 images are scaled by 1/255, as the reference's round trip through its .ply file does."""
    if images is None:
        raise ValueError("depth_point_cloud needs the images: the cloud's colours come from them")
    xyz, colors = depth_points(depths, intrinsics_inv, poses, images=images, masks=masks, n_pts=int(num_pts), generator=generator, device=device)
    return xyz, colors.float() / 255.0 if colors.dtype is torch.uint8 else colors.float()


def splats_from_points(points, colors=None, sh_degree: int = 3, isotropic: bool = False, generator: Optional[torch.Generator] = None):
    """The raw tensors `GaussianModel.create_from_pcd` builds (reference scene/gaussian_model.py:97-121), as a dict: ``_xyz`` [N,3],
    ``_features_dc`` [N,1,3] (RGB2SH of the colours), ``_features_rest`` [N,(sh_degree+1)^2-1,3] zeros, ``_scaling`` =
    log(sqrt(clamp_min(distCUDA2(xyz), 1e-7))) in 3 columns (1 when isotropic), ``_rotation`` (1,0,0,0), ``_opacity`` =
    inverse_sigmoid(0.1), and ``max_radii2D`` zeros.  colors=None: the reference's ``random / 255``, drawn from ``generator``."""
    from simple_knn._C import distCUDA2
    xyz = (points if torch.is_tensor(points) else torch.from_numpy(np.ascontiguousarray(points))).detach()
    if not xyz.is_cuda:
        xyz = xyz.cuda()
    xyz = xyz.float().contiguous()
    n, dev = xyz.shape[0], xyz.device
    if colors is None:
        gen_dev = dev if generator is None else generator.device
        colors = torch.rand(n, 3, generator=generator, device=gen_dev) / 255.0
    colors = (colors if torch.is_tensor(colors) else torch.from_numpy(np.ascontiguousarray(colors))).to(dev).float()
    scales = torch.log(torch.sqrt(torch.clamp_min(distCUDA2(xyz), 0.0000001)))[..., None]
    rots = torch.zeros(n, 4, device=dev)
    rots[:, 0] = 1
    tenth = 0.1 * torch.ones(n, 1, dtype=torch.float, device=dev)
    return {"_xyz": xyz,
            "_features_dc": ((colors - 0.5) / SH_C0)[:, None, :].contiguous(),
            "_features_rest": torch.zeros(n, (sh_degree + 1) ** 2 - 1, 3, device=dev),
            "_scaling": scales if isotropic else scales.repeat(1, 3),
            "_rotation": rots,
            "_opacity": torch.log(tenth / (1 - tenth)),                      # inverse_sigmoid, in float32 as the reference
            "max_radii2D": torch.zeros(n, device=dev)}
