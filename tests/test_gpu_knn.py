"""distCUDA2 counterpart against an exact CPU k-NN (scipy cKDTree): the reference calls it once at
initialisation (scene/gaussian_model.py:105) to get the mean squared distance to the 3 nearest neighbours."""
import numpy as np
import pytest
import torch
from scipy.spatial import cKDTree

from tests.scan_round import SCAN_ROUND

pytestmark = pytest.mark.gpu


def oracle_mean_dist2(pts: np.ndarray) -> np.ndarray:
    n = len(pts)
    if n == 0:
        return np.zeros(0, np.float32)
    k = min(4, n)
    d, idx = cKDTree(pts.astype(np.float64)).query(pts.astype(np.float64), k=k)
    d = d.reshape(n, k); idx = idx.reshape(n, k)
    out = np.zeros(n)
    for i in range(n) if n < 8 else []:
        others = [dd for dd, j in zip(d[i], idx[i]) if j != i][:3]
        out[i] = sum(x * x for x in others) / 3.0
    if n >= 8:
        # self is one of the zero-distance hits; drop exactly one zero per row (duplicates keep theirs)
        self_pos = np.argmax(idx == np.arange(n)[:, None], axis=1)
        has_self = (idx == np.arange(n)[:, None]).any(axis=1)
        d2 = d ** 2
        d2[np.arange(n), np.where(has_self, self_pos, k - 1)] = 0.0
        out = d2.sum(axis=1) / 3.0
    return out


@pytest.mark.parametrize("n,kind", [(1, "uniform"), (2, "uniform"), (3, "uniform"), (5, "uniform"), (1000, "uniform"),
                                     (20000, "clustered"), (300000, "uniform"), (5000, "duplicates"), (4000, "planar"),
                                     (SCAN_ROUND - 1, "uniform"), (SCAN_ROUND, "uniform"), (SCAN_ROUND + 1, "uniform")])
def test_matches_exact_knn(hip_device, n, kind):
    from simple_knn._C import distCUDA2
    rng = np.random.default_rng(n)
    pts = rng.uniform(-1, 1, size=(n, 3)).astype(np.float32)
    if kind == "clustered":
        centres = rng.uniform(-1, 1, size=(20, 3))
        pts = (centres[rng.integers(0, 20, n)] + 0.01 * rng.standard_normal((n, 3))).astype(np.float32)
        pts[:50] = rng.uniform(-30, 30, size=(50, 3))  # far outliers stretch the grid
    if kind == "duplicates":
        pts[1000:2000] = pts[:1000]
    if kind == "planar":
        pts[:, 2] = 0.25
    got = distCUDA2(torch.from_numpy(pts).to(hip_device)).cpu().numpy()
    ref = oracle_mean_dist2(pts)
    assert got.shape == (n,)
    np.testing.assert_allclose(got, ref, rtol=2e-5, atol=1e-12)


def degenerate_cloud(kind):
    rng = np.random.default_rng(len(kind))
    if kind == "four":                      # exactly three neighbours each
        return rng.uniform(-1, 1, size=(4, 3)).astype(np.float32)
    if kind == "collinear":                 # two axes without extent: both sit on the floor that make_grid gives thin axes
        pts = np.empty((3000, 3), np.float32)
        pts[:, 0], pts[:, 1], pts[:, 2] = rng.uniform(-1, 1, 3000), 0.25, -0.5
        return pts
    if kind == "identical":                 # no extent at all: one cell
        return np.full((2000, 3), 0.375, np.float32)
    pts = rng.uniform(-1, 1, size=(2001, 3)).astype(np.float32)
    pts[777] = (1e30, 0.5, -0.5) if kind == "far_point_x" else (1e30, 1e30, 1e30)    # its squared distances overflow float32
    return pts


@pytest.mark.parametrize("kind", ["four", "collinear", "identical", "far_point_x", "far_point_xyz"])
def test_degenerate_clouds_match_exact_knn(hip_device, kind):
    """The exact search in the output's number format: a mean that float32 cannot hold (the point at 1e30) is +inf there, as the
    published code's sum of FLT_MAX entries is."""
    from simple_knn._C import distCUDA2
    pts = degenerate_cloud(kind)
    got = distCUDA2(torch.from_numpy(pts).to(hip_device)).cpu().numpy()
    with np.errstate(over="ignore"):
        ref = oracle_mean_dist2(pts).astype(np.float32)
    assert got.shape == (len(pts),) and got.dtype == np.float32
    np.testing.assert_allclose(got, ref, rtol=2e-5, atol=1e-12)
    if kind == "identical":
        assert (got == 0).all()
    if kind.startswith("far_point"):
        assert np.isinf(ref[777]) and np.isfinite(np.delete(ref, 777)).all() and (np.delete(ref, 777) > 0).all()


def test_non_finite_rows_leave_the_finite_rows_exact(hip_device):
    """2000 points of which 5 rows hold a NaN and 5 an infinity: every finite row gets the exact search over the finite rows
    only; the others are only required to be written (NaN or inf will do)."""
    from splatfields_amd import _lib
    from tests.moran_reference import cloud_with_non_finite_rows
    points, finite = cloud_with_non_finite_rows()
    n = points.shape[0]
    lib = _lib.load()
    pts = points.to(hip_device)
    out = torch.full((n,), -7.0, device=hip_device)              # no mean of squares is negative
    work = torch.empty(lib.sr_knn_workspace_bytes(n), dtype=torch.uint8, device=hip_device)
    _lib.check(lib.sr_knn3_mean_dist2(n, _lib.ptr(pts), _lib.ptr(out), _lib.ptr(work), _lib.stream(hip_device)))
    got = out.cpu().numpy()
    assert (got != -7.0).all()
    f = finite.numpy()
    np.testing.assert_allclose(got[f], oracle_mean_dist2(points[finite].numpy()), rtol=2e-5, atol=1e-12)
    from simple_knn._C import distCUDA2
    assert np.array_equal(distCUDA2(pts).cpu().numpy(), got, equal_nan=True)


def test_initial_scales_as_the_reference_computes_them(hip_device):
    """scene/gaussian_model.py:105-109: scales = log(sqrt(clamp_min(distCUDA2(points), 1e-7)))"""
    from simple_knn._C import distCUDA2
    g = torch.Generator().manual_seed(0)
    pts = torch.rand(10000, 3, generator=g).to(hip_device)
    dist2 = torch.clamp_min(distCUDA2(pts), 0.0000001)
    scales = torch.log(torch.sqrt(dist2))[..., None].repeat(1, 3)
    assert scales.shape == (10000, 3) and torch.isfinite(scales).all()
    assert abs(torch.exp(scales).mean().item() - 0.045) < 0.02  # ~ N^(-1/3) spacing of a unit cube
