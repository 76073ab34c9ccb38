"""Writes tests/golden/hull_cases.npz: the survivor sets of the reference's OWN visual-hull code on small inputs.  Run on a CPU
where a reference checkout exists:

    python tests/golden/make_hull_golden.py /path/to/reference

scene/dataset_readers.py is imported as it is, through a stub `scene` package whose __path__ points at the reference's scene/
(its __init__ drags in the whole training stack) and empty stand-ins for the packages that are not installed (trimesh, cv2,
imageio, plyfile, ...).  Nothing of the reference's text is copied; four of its entry points are CALLED:

    samples_krt    visual_hull_samples       (:1385-1417)   G = 32, 4 rotated pinhole cameras at distance 3, elliptical 40x52 masks
    samples_list   visual_hull_samples_list  (:1419-1458)   the same cameras, two views cropped (ragged sizes, "keep" policy)
    blender_hull   readNerfSyntheticInfo(pts_samples='hull') (:605-644)   its fixed 256^3 grid over [-1.5, 1.5], 3 square 48x48
                   views with small disc masks; computes in float32
    blender_load   readNerfSyntheticInfo(pts_samples='load') (:544-588)   6000 points filtered by the same test, float32

For the two Blender calls `readCamerasFromTransforms` is replaced by fabricated CameraInfo records (the reference's own reader
fails under a current Pillow at Image.fromarray(..., np.byte)), `storePly` by a function that records its xyz, `fetchPly` by a
no-op and trimesh.load by a function that returns the fabricated points; num_pts is huge, so that nothing is subsampled.

Numbers only travel.  Per case <name>: n_views, mask0 .. mask{V-1} (uint8), matrices (float64: the KRT, or the float32
full_proj_transform the reference computed, widened), convention, outside, float32 (did the reference compute in float32),
G and aabb or points, and indices: the sorted int32 linear indices (rows, for points) of the survivors."""
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))


class _Stub(types.ModuleType):
    __path__ = []

    def __getattr__(self, name):
        if name.startswith("__"):
            raise AttributeError(name)
        return object


def import_readers(ref):
    sys.path.insert(0, ref)
    for name in ["trimesh", "cv2", "imageio", "plyfile", "simple_knn", "simple_knn._C", "lpips", "torchvision", "mmgen", "mmgen.models",
                 "mmcv", "mmcv.cnn", "mmcv.runner", "diffusers", "diffusers.models", "diffusers.models.resnet",
                 "diffusers.models.attention", "sklearn", "sklearn.cluster", "sklearn.neighbors", "tqdm", "pytorch3d", "pytorch3d.ops"]:
        if name not in sys.modules:
            try:
                __import__(name)
            except Exception:
                sys.modules[name] = _Stub(name)
    pkg = types.ModuleType("scene")
    pkg.__path__ = [os.path.join(ref, "scene")]
    saved = sys.modules.get("scene")
    sys.modules["scene"] = pkg
    try:
        from scene import dataset_readers
    finally:
        if saved is None:
            sys.modules.pop("scene", None)
        else:
            sys.modules["scene"] = saved
    return dataset_readers


def look_at(center):
    """world-to-camera rotation (rows: camera x, y, z in world) of a camera at `center` looking at the origin along +z, rolled a
    little so that no axis is aligned with the grid"""
    z = -center / np.linalg.norm(center)
    x = np.cross(np.array([0.13, 0.31, 0.94]), z)
    x /= np.linalg.norm(x)
    return np.stack([x, np.cross(z, x), z])


def ellipse(h, w, ry, rx, cy=None, cx=None):
    cy, cx = (h - 1) / 2 if cy is None else cy, (w - 1) / 2 if cx is None else cx
    yy, xx = np.mgrid[:h, :w]
    return (((yy - cy) / ry) ** 2 + ((xx - cx) / rx) ** 2 <= 1.0).astype(np.uint8)


def grid_indices(xyz, tables):
    """linear voxel indices (iy G + ix) G + iz of grid positions, by exact lookup in the coordinate tables"""
    G = tables.shape[1]
    ijk = [np.searchsorted(tables[a], xyz[:, a]) for a in range(3)]
    for a in range(3):
        assert np.array_equal(tables[a][ijk[a]], xyz[:, a]), "a stored position is not a grid position"
    return np.sort((ijk[1].astype(np.int64) * G + ijk[0]) * G + ijk[2]).astype(np.int32)


def pack(arrays, name, masks, matrices, convention, outside, float32, indices, **extra):
    arrays[f"{name}/n_views"] = np.int32(len(masks))
    for k, m in enumerate(masks):
        arrays[f"{name}/mask{k}"] = np.asarray(m, np.uint8)
    arrays[f"{name}/matrices"] = np.asarray(matrices, np.float64)
    arrays[f"{name}/convention"], arrays[f"{name}/outside"] = np.array(convention), np.array(outside)
    arrays[f"{name}/float32"] = np.bool_(float32)
    arrays[f"{name}/indices"] = np.asarray(indices, np.int32)
    for k, v in extra.items():
        arrays[f"{name}/{k}"] = v
    print(name, len(masks), "views,", len(indices), "survivors")


def samples_cases(R, arrays):
    G, aabb, H, W = 32, (-1.0, 1.0), 40, 52
    K = np.array([[58.0, 0.0, 25.1], [0.0, 57.0, 19.7], [0.0, 0.0, 1.0]])
    centers = [np.array(c, np.float64) for c in ((2.1, 0.9, 1.95), (-1.7, 2.2, 1.1), (0.6, -2.5, 1.55), (-1.3, -1.2, -2.44))]
    KRT = []
    for c in centers:
        c = 3.0 * c / np.linalg.norm(c)
        Rw = look_at(c)
        KRT.append(K @ np.concatenate([Rw, (-Rw @ c)[:, None]], axis=1))
    KRT = np.stack(KRT)
    masks = np.stack([ellipse(H, W, 15.5 - k, 21.0 - 2 * k, 19.0 + k, 25.5 - k) for k in range(4)])
    tables = np.stack([np.linspace(aabb[0], aabb[1], G)] * 3)
    xyz = R.visual_hull_samples(masks.astype(np.float64), KRT, n_pts=10 ** 9, grid_resolution=G, aabb=aabb)
    pack(arrays, "samples_krt", masks, KRT, "krt", "carve", False, grid_indices(xyz, tables), G=np.int32(G), aabb=np.array(aabb))
    # two views cropped to other sizes: their principal point moves with the crop
    crops = [(0, 0, H, W), (4, 6, 30, 38), (0, 0, H, W), (7, 3, 33, 41)]          # (y0, x0, h, w)
    KRT_l, masks_l = [], []
    for k, (y0, x0, h, w) in enumerate(crops):
        shift = np.array([[1.0, 0.0, -x0], [0.0, 1.0, -y0], [0.0, 0.0, 1.0]])
        KRT_l.append(shift @ KRT[k])
        masks_l.append(masks[k][y0:y0 + h, x0:x0 + w])
    KRT_l = np.stack(KRT_l)
    xyz = R.visual_hull_samples_list([m.astype(np.float64) for m in masks_l], KRT_l, n_pts=10 ** 9, grid_resolution=G, aabb=aabb)
    pack(arrays, "samples_list", masks_l, KRT_l, "krt", "keep", False, grid_indices(xyz, tables), G=np.int32(G),
         aabb=np.array(aabb))


def blender_cases(R, arrays):
    from utils.graphics_utils import getProjectionMatrix, getWorld2View2
    S, fov = 48, 0.62
    cams, full = [], []
    for k, c in enumerate(((3.1, 1.2, 2.0), (-2.2, 2.9, 1.3), (0.7, -2.6, 2.8))):
        c = np.array(c, np.float64)
        Rw = look_at(c)
        Rc, T = Rw.T, -Rw @ c                                   # the reader stores the rotation transposed (getWorld2View2 undoes it)
        mask = 255 * ellipse(S, S, 5.5 + 0.5 * k, 5.5 + 0.5 * k, 23.0 + k, 24.5 - k)
        cams.append(R.CameraInfo(uid=k, R=Rc, T=T, FovY=fov, FovX=fov, image=types.SimpleNamespace(size=(S, S)), image_path="", image_name=str(k),
                                 width=S, height=S, fid=0.0, mask=mask))
        # the matrix the reference builds at :620-622, with its own helpers, in float32 as there
        w2v = torch.tensor(getWorld2View2(Rc, T, np.array([0.0, 0.0, 0.0]), 1.0)).transpose(0, 1)
        prj = getProjectionMatrix(znear=0.01, zfar=100.0, fovX=fov, fovY=fov).transpose(0, 1)
        m = (w2v.unsqueeze(0).bmm(prj.unsqueeze(0))).squeeze(0)
        assert m.dtype == torch.float32
        full.append(m.double().numpy())
    full = np.stack(full)
    masks = [np.asarray(c.mask > 0, np.uint8) for c in cams]
    rng = np.random.default_rng(5)
    cloud = rng.uniform(-0.7, 0.7, (6000, 3)).astype(np.float32).astype(np.float64)     # float32-representable: the reference rounds them
    recorded = []
    saved = (R.readCamerasFromTransforms, R.storePly, R.fetchPly)
    R.readCamerasFromTransforms = lambda path, name, *a, **k: list(cams) if "train" in name else []
    R.storePly = lambda path, xyz, rgb: recorded.append(np.array(xyz))
    R.fetchPly = lambda path: None
    R.trimesh.load = lambda path: types.SimpleNamespace(vertices=cloud)
    try:
        R.readNerfSyntheticInfo("", False, True, num_pts=10 ** 9, pts_samples="hull")
        R.readNerfSyntheticInfo("", False, True, num_pts=10 ** 9, pts_samples="load", pc_path=os.path.abspath(__file__))
    finally:
        R.readCamerasFromTransforms, R.storePly, R.fetchPly = saved
    hull_xyz, load_xyz = recorded
    G, aabb = 256, (-1.5, 1.5)
    assert hull_xyz.dtype == np.float32
    tables = np.stack([np.linspace(aabb[0], aabb[1], G).astype(np.float32)] * 3)        # the reference's `.float()` of the grid
    pack(arrays, "blender_hull", masks, full, "ndc", "carve", True, grid_indices(hull_xyz, tables), G=np.int32(G), aabb=np.array(aabb))
    row_of = {cloud[i].tobytes(): i for i in range(len(cloud))}
    assert len(row_of) == len(cloud)
    rows = np.array([row_of[np.asarray(p, np.float64).tobytes()] for p in load_xyz], np.int32)
    assert np.all(np.diff(rows) > 0)
    pack(arrays, "blender_load", masks, full, "ndc", "carve", True, rows, points=cloud)


def main():
    if len(sys.argv) != 2:
        sys.exit(__doc__)
    R = import_readers(sys.argv[1])
    np.random.seed(0)
    arrays = {}
    samples_cases(R, arrays)
    blender_cases(R, arrays)
    path = os.path.join(HERE, "hull_cases.npz")
    np.savez_compressed(path, **arrays)
    print(path, os.path.getsize(path), "bytes,", len(arrays), "arrays")
    assert os.path.getsize(path) <= 500_000


if __name__ == "__main__":
    main()
