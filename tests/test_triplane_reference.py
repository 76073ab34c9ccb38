"""tests/triplane_reference.py (the plain-PyTorch yardstick of csrc/triplane.hip) against the reference's own
VarTriPlaneEncoder.forward through the fixtures tests/golden/triplane_*.npz, the caps that keep the GPU parity cases of
tests/test_gpu_triplane_edges.py honest, and the fixed-point contract the kernel's header states.  No GPU."""
import os

import numpy as np
import pytest
import torch

from tests import triplane_reference as R

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
FIXTURES = ("c16_24x24", "c8_20x28")


@pytest.mark.parametrize("name", FIXTURES)
def test_lookup_reproduces_the_reference_class(name):
    z = np.load(os.path.join(GOLDEN, f"triplane_{name}.npz"))
    assert z["axis"].tolist() == [list(a) for a in R.AXES]
    planes, pts, probe = (torch.as_tensor(z[k]) for k in ("planes", "pts", "probe"))     # pts [1, N, 3] like encoder(x[None])
    want = {"out": z["out"], "d_planes": z["grad_planes"], "d_pts": z["grad_pts"]}
    ref64, ref32 = R.lookup(planes, pts, probe, torch.float64), R.lookup(planes, pts, probe, torch.float32)
    fragile = R.fragile_points(pts, planes.shape[2], planes.shape[3])
    print(f"[triplane] {name}: {int(fragile.sum())} fragile points of {fragile.numel()}")
    for k in R.TENSORS:
        w = torch.as_tensor(want[k]).double()
        assert ref64[k].shape == w.shape == ref32[k].shape, k
        top = w.abs().max().item()
        r = (ref32[k] - ref64[k]).abs().max().item()
        d64, d32 = (ref64[k] - w).abs().max().item(), (ref32[k] - w).abs().max().item()
        print(f"[triplane] {name} {k}: float32 run - fixture {d32 / top:.2e}, float64 run - fixture {d64 / top:.2e}, own error {r / top:.2e} (relative)")
        assert d32 <= 1e-6 * top, (k, d32 / top)
        # the fixture IS a float32 evaluation: the float64 run is no farther from it than from the float32 run beside it
        assert 0.0 < r and d64 <= r, (k, d64, r)


@pytest.mark.parametrize("case", R.CASES, ids=lambda c: c.name)
def test_parity_cases_keep_their_caps(case):
    e = R.evaluated(case.name)
    planes, pts, probe = e["planes"], e["pts"], e["probe"]
    assert tuple(planes.shape) == (3, case.C, case.H, case.W) and tuple(pts.shape) == (case.N, 3) and tuple(probe.shape) == (case.N, 3 * case.C)
    assert all(t.dtype == torch.float32 for t in (planes, pts, probe)) and pts.abs().max() <= 1.1 and pts.abs().max() > 1.0
    again = R.make_case(case)
    assert all(torch.equal(a, b) for a, b in zip(again, (planes, pts, probe)))            # the CPU and the GPU test see the same inputs
    fragile, padded = e["fragile"].double().mean().item(), R.padded_points(pts, case.H, case.W).double().mean().item()
    print(f"[triplane] {case.name}: fragile {int(e['fragile'].sum())} of {case.N}, padded share {padded:.3f}, own float32 error "
          + "  ".join(f"{k} {e['r'][k]:.2e} (max {e['f64'][k].abs().max().item():.2e})" for k in R.TENSORS))
    assert fragile <= 0.01 and padded >= 0.05
    for k in R.TENSORS:
        assert torch.isfinite(e["f64"][k]).all() and torch.isfinite(e["f32"][k]).all()
        assert np.isfinite(e["r"][k]) and e["r"][k] > 0.0, k
    if case.wide:     # thirty binades of upstream magnitudes, the largest about 1
        top = probe.abs().amax(dim=1)
        assert top.max() > 0.5 and top.min() < 2.0 ** -24


def test_fragile_and_padded_masks_name_the_right_points():
    H, W = 6, 10
    centre = lambda k, s: (2 * k + 1) / s - 1.0             # texel centre k of an axis with s texels: pixel coordinate k exactly
    pts = torch.tensor([[centre(3, W), 0.01, 0.02],         # ix of plane xy is an integer
                        [0.013, 0.017, 0.019],              # nothing near an integer
                        [0.013, centre(2, H) + 1e-7, 0.019],  # iy of plane xy within H 2^-20 of an integer
                        [0.013, centre(2, H) + 1e-4, 0.019],  # ... and outside it
                        [1.05, 0.017, 0.019]], dtype=torch.float64)
    assert R.fragile_points(pts, H, W).tolist() == [True, False, True, False, False]
    assert R.padded_points(pts, H, W).tolist() == [False, False, False, False, True]
    ix, iy = R.pixel_coordinates(pts, H, W)
    assert ix[0, 0] == 3.0 and abs(iy[2, 0] - 2.0) < H * 2.0 ** -20 < abs(iy[3, 0] - 2.0)
    # the margin scales with the extent along the axis: in units of the coordinate itself it is 2^-19 at every plane size
    for s in (4, 4096):
        v = torch.tensor([[centre(1, s) + 1.5e-6, 0.3, 0.3], [centre(1, s) + 2.5e-6, 0.3, 0.3]], dtype=torch.float64)
        assert R.fragile_points(v, 3, s).tolist() == [True, False], s


def test_fuse_modes_follow_the_reference():
    case = R.CASE_BY_NAME["c12_20x28"]
    planes, pts, probe = R.make_case(case, fuse="add")
    assert tuple(probe.shape) == (case.N, case.C)
    cat = R.features(planes.double(), pts.double()[None], "cat")[0]
    add = R.lookup(planes, pts, probe, torch.float64, fuse="add")
    mean = R.lookup(planes, pts, probe, torch.float64, fuse="mean")
    assert torch.equal(add["out"], cat.reshape(case.N, 3, case.C).sum(1))                # the reference sums for 'add' AND 'mean'
    assert all(torch.equal(add[k], mean[k]) for k in R.TENSORS)
    with pytest.raises(NotImplementedError):
        R.features(planes, pts[None], "max")


def test_fixed_point_resolution_restates_the_header():
    assert R.fixed_point_resolution(1.0, 100_000) == 2.0 ** -42      # the header's "2^-43 of the largest upstream value", within its factor two
    assert R.fixed_point_resolution(0.75, 100_000) == 2.0 ** -43
    # the values tests/test_gpu_triplane_edges.py relies on
    for n in (4097, 4099, 8191):
        for g in (2.0 ** 20, 1.5 * 2.0 ** 20, float(np.nextafter(np.float32(2.0 ** 21), np.float32(0)))):
            assert R.fixed_point_resolution(g, n) == 2.0 ** -26, (g, n)
    assert R.fixed_point_resolution(float(np.nextafter(np.float32(2), np.float32(0))), 4099) == 2.0 ** -46
    assert R.fixed_point_resolution(2.0 ** -140, 1) == 2.0 ** (-139 + 3 - 62)
    # no overflow in the worst case: 4 n contributions of gmax each stay below 2^62 units
    for g, n in ((1.0, 100_000), (2.0 ** 20, 4099), (3.9, 1), (2.0 ** -140, 7)):
        assert 4 * n * g / R.fixed_point_resolution(g, n) < 2.0 ** 62
