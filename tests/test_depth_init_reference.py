"""The float64 restatement of the depth-map back-projection (tests/depth_init_reference.py) against the reference's own
`_gen_3dpoints` (tests/golden/depth_init_cases.npz, written by tests/golden/make_depth_init_golden.py from calls of it): the
float64 run within 1e-14 relative, and EQUAL in row count, order and colours; the float32 run, as the readers make it, as far
from the float64 one as float32 arithmetic explains."""
import numpy as np
import pytest

from tests import depth_init_reference as R

CASES = R.golden_cases()


def test_fixture_inventory():
    assert sorted(CASES) == ["img130x70", "img5x7", "img64x48"]
    for name, (H, W) in (("img5x7", (5, 7)), ("img64x48", (64, 48)), ("img130x70", (130, 70))):
        c = CASES[name]
        assert (int(c["H"]), int(c["W"])) == (H, W)
        assert c["depths"].shape == (3, H, W) and c["depths"].dtype == np.float32
        assert c["images"].shape == (3, H, W, 3) and c["images"].dtype == np.uint8
        assert c["kinv"].shape == (3, 4, 4) and c["pose"].shape == (3, 4, 4) and c["kinv"].dtype == np.float64
        for k in (0, 2):
            d = c["depths"][k]
            assert (d == 0).any() and (d == -1).any() and (d > 0).any()
            assert c[f"pts32_{k}"].dtype == np.float32 and c[f"pts64_{k}"].dtype == np.float64
            assert c[f"pts32_{k}"].shape == c[f"pts64_{k}"].shape == (int((d > 0).sum()), 3)
            assert np.array_equal(c[f"rgb32_{k}"], c[f"rgb64_{k}"]) and c[f"rgb64_{k}"].dtype == np.uint8


@pytest.mark.parametrize("name", sorted(CASES))
def test_restatement_reproduces_the_reference(name):
    c = CASES[name]
    H, W = int(c["H"]), int(c["W"])
    xyz, rgb, idx = R.back_project(c["depths"], c["kinv"], c["pose"], images=c["images"])
    assert np.all(np.diff(idx) > 0) and len(idx) == int((c["depths"] > 0).sum())
    for k in (0, 2):
        rows = (idx >= k * H * W) & (idx < (k + 1) * H * W)
        want = c[f"pts64_{k}"]
        assert xyz[rows].shape == want.shape                                       # the row count
        assert np.array_equal(rgb[rows], c[f"rgb64_{k}"])                           # the colours, hence the order (random images)
        err = np.abs(xyz[rows] - want).max() / np.abs(want).max()
        err32 = np.abs(c[f"pts32_{k}"].astype(np.float64) - want).max()
        print(f"{name} img_idx {k}: {len(want)} rows, restatement against the reference in float64 {err:.2e} relative; "
              f"the reference's float32 run is {err32:.2e} away")
        assert err <= 1e-14
        assert err32 <= 64 * 2.0 ** -24 * np.abs(want).max()                        # float32 arithmetic, a dozen operations
        # a batch of one image gives the same rows as the slice of the batch of three
        one = R.back_project(c["depths"][k:k + 1], c["kinv"][k:k + 1], c["pose"][k:k + 1], images=c["images"][k:k + 1])
        assert np.array_equal(one[0], xyz[rows]) and np.array_equal(one[2], idx[rows] - k * H * W)


def test_restatement_edge_rules():
    """`> 0` decides: 0, -0, -1 and NaN are dropped, +inf, the smallest subnormal and 1e30 are kept; masks as `mask > 0`; 1 x N and
    N x 1 images are defined by the formula"""
    d = np.array([[[0.0, -0.0, -1.0, np.nan, np.inf, 1e-45, 1e30, 2.0, 3.0]]], np.float32)            # 1 x 9
    eye = np.eye(4)[None]
    xyz, _, idx = R.back_project(d, eye, eye)
    assert idx.tolist() == [4, 5, 6, 7, 8]
    assert np.isinf(xyz[0]).any() and np.all(np.isfinite(xyz[1:]))
    x = 7.0
    assert np.array_equal(xyz[3], 2.0 * (np.array([x, 0.0, 1.0]) / np.sqrt(x * x + 0.0 + 1.0)))
    mask = np.array([[[1, 1, 1, 1, 0, 1, 0, 0.5, -1]]])
    assert R.back_project(d, eye, eye, masks=mask)[2].tolist() == [5, 7]
    assert R.back_project(d, eye, eye, masks=mask[..., None])[2].tolist() == [5, 7]
    xyz_t, _, idx_t = R.back_project(d.transpose(0, 2, 1), eye, eye)                                  # 9 x 1
    assert idx_t.tolist() == [4, 5, 6, 7, 8] and np.array_equal(xyz_t[3], 2.0 * (np.array([0.0, x, 1.0]) / np.sqrt(0.0 + x * x + 1.0)))
    empty = R.back_project(np.zeros((2, 3, 4), np.float32), np.eye(4)[None].repeat(2, 0), np.eye(4)[None].repeat(2, 0))
    assert empty[0].shape == (0, 3) and empty[2].shape == (0,)


def test_coordinate_bound_is_half_an_ulp_plus_the_double_term():
    assert R.ulp32(np.array([1.0, 1.5, 2.0, 3.0, 0.75]))[:].tolist() == [2.0 ** -23, 2.0 ** -23, 2.0 ** -22, 2.0 ** -22, 2.0 ** -24]
    assert R.ulp32(np.array([0.0, 1e-46])).tolist() == [2.0 ** -149, 2.0 ** -149]
    ref = np.array([[1.0, -3.0, 0.5]])
    assert np.array_equal(R.coordinate_bound(ref), 0.5 * np.array([[2.0 ** -23, 2.0 ** -22, 2.0 ** -24]]) + 3e-12)
