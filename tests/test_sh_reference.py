"""tests/sh_reference.py (the yardstick of the SH stage's GPU tests) pinned to oracle.torch_oracle.sh_to_rgb and, through
tests/golden/sh_cases.npz, to the reference's own eval_sh + 0.5 + clamp as extract_geo.py:40-44 calls it (the fixture is
written by tests/golden/make_sh_golden.py).  CPU only."""
import os

import numpy as np
import pytest
import torch

from oracle import torch_oracle as O
from tests import sh_reference as R

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "sh_cases.npz")


@pytest.fixture(scope="module")
def golden():
    z = np.load(GOLDEN)
    return {k: torch.from_numpy(z[k]) for k in z.files}


def rel(a, b):
    return (a - b).abs().max().item() / max(b.abs().max().item(), 1e-300)


@pytest.mark.parametrize("deg", range(4))
def test_fixture_float64(golden, deg):
    """Outputs and both gradients of the reference's float64 run, to 1e-12 of each tensor's largest magnitude."""
    g = golden
    means, shs, campos, probe = (g[k].double() for k in ("means", "shs", "campos", "probe"))
    pre, colors, keep = R.forward_views(means, shs, campos, deg)
    assert pre.shape == (2, 64, 3) and pre.dtype == torch.float64 and keep.dtype == torch.bool
    assert pre.abs().min() > 1e-4                                        # no clamp decision hangs on rounding
    want = {k: g[f"deg{deg}/f64/{k}"] for k in ("colors", "d_shs", "d_means")}
    assert torch.equal(colors == 0, want["colors"] == 0) and torch.equal(keep, want["colors"] > 0)
    assert (colors == 0).double().mean() > 0.2
    assert rel(colors, want["colors"]) <= 1e-12
    d_shs, d_means = R.backward(means, shs, campos, probe * keep, deg, 1.0)
    assert d_shs.shape == shs.shape and d_means.shape == means.shape
    assert rel(d_shs, want["d_shs"]) <= 1e-12
    assert (d_shs[:, (deg + 1) ** 2:] == 0).all() and (want["d_shs"][:, (deg + 1) ** 2:] == 0).all()
    if deg == 0:
        assert (d_means == 0).all() and (want["d_means"] == 0).all()
    else:
        assert rel(d_means, want["d_means"]) <= 1e-12
    # scale is a factor of the whole gradient
    half_shs, half_means = R.backward(means, shs, campos, probe * keep, deg, 0.5)
    assert torch.equal(half_shs, 0.5 * d_shs) and torch.equal(half_means, 0.5 * d_means)


@pytest.mark.parametrize("deg", range(4))
def test_fixture_float32(golden, deg):
    """In float32 the restatement is another rounding of the same formula: it stays as close to float64 as the reference's own
    float32 run does (4x, the margin the kernels get), and clamps the same channels."""
    g = golden
    means, shs, campos, probe = (g[k] for k in ("means", "shs", "campos", "probe"))
    pre, colors, keep = R.forward_views(means, shs, campos, deg)
    assert pre.dtype == torch.float32
    d_shs, d_means = R.backward(means, shs, campos, probe * keep, deg, 1.0)
    assert torch.equal(keep, g[f"deg{deg}/f64/colors"] > 0)
    for name, ours in (("colors", colors), ("d_shs", d_shs), ("d_means", d_means)):
        w64, w32 = g[f"deg{deg}/f64/{name}"], g[f"deg{deg}/f32/{name}"]
        assert w32.dtype == torch.float32 and w64.dtype == torch.float64
        r = max((w32.double() - w64).abs().max().item(), float(np.spacing(np.float32(w64.abs().max().item()))))
        assert (ours.double() - w64).abs().max().item() <= 4 * r, (name, deg)


@pytest.mark.parametrize("deg", range(4))
def test_against_the_oracle(deg):
    from splatfields_amd.synthetic import make_camera, make_splats
    sp = make_splats(300, seed=3)
    means, shs = sp["means3D"].double(), sp["shs"].double() * 3.0
    for view in (0, 2):
        campos = make_camera(view, 64, 64).camera_center.double()
        m = means.clone().requires_grad_(True)
        s = shs.clone().requires_grad_(True)
        want = O.sh_to_rgb(deg, s, m, campos)
        probe = torch.randn(300, 3, dtype=torch.float64, generator=torch.Generator().manual_seed(deg))
        (want * probe).sum().backward()
        pre, colors, keep = R.forward_views(means, shs, campos[None], deg)
        assert (pre < 0).any() and rel(colors[0], want.detach()) <= 1e-13
        d_shs, d_means = R.backward(means, shs, campos[None], probe[None] * keep, deg)
        assert rel(d_shs, s.grad) <= 1e-13
        if deg > 0:
            assert rel(d_means, m.grad) <= 1e-12
        else:
            assert m.grad is None or (m.grad == 0).all()


def test_unused_rows_are_never_read_and_the_clamp_byte():
    from splatfields_amd.synthetic import make_splats
    sp = make_splats(50, seed=5, sh_coeffs=25)
    means, shs, campos = sp["means3D"].double(), sp["shs"].double() * 3.0, torch.tensor([[2.0, 1.0, 0.5], [0.0, -3.0, 1.0]], dtype=torch.float64)
    for deg in range(4):
        nb = (deg + 1) ** 2
        dirty = shs.clone()
        dirty[:, nb:] = float("nan")
        clean = R.forward_views(means, shs, campos, deg)
        assert all(torch.equal(a, b) for a, b in zip(clean, R.forward_views(means, dirty, campos, deg)))
        probe = torch.ones(2, 50, 3, dtype=torch.float64) * clean[2]
        a, b = R.backward(means, shs, campos, probe, deg), R.backward(means, dirty, campos, probe, deg)
        assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]) and (a[0][:, nb:] == 0).all()
    pre = torch.tensor([[-1.0, 2.0, -0.0], [0.0, -1e-30, 5.0], [-1.0, -2.0, -3.0]])
    assert R.clamp_bits(pre).tolist() == [1, 2, 7] and R.clamp_bits(pre).dtype == torch.uint8
    assert R.forward_views(means, shs, campos, 0)[2].dtype == torch.bool


def test_the_exact_boundary_of_the_clamp_in_float32():
    """What tests/test_gpu_sh_edges.py expects of the kernels at degree 0: with dc = float32(-0.5) / float32(C0) the one-term
    sum lands on 0.0 exactly, and its float32 neighbours land one step to either side."""
    c0 = np.float32(R.C0)
    dc = np.float32(-0.5) / c0
    assert abs(float(dc) + 1.7724538) < 1e-6
    below, above = np.nextafter(dc, np.float32(-np.inf)), np.nextafter(dc, np.float32(np.inf))
    pre = [float(np.float32(c0 * x) + np.float32(0.5)) for x in (below, dc, above)]
    assert pre[1] == 0.0 and pre[0] == pytest.approx(-5.96e-8, rel=1e-2) and pre[2] == pytest.approx(2.98e-8, rel=1e-2)
    shs = torch.tensor([below, dc, above], dtype=torch.float32).reshape(3, 1, 1).repeat(1, 1, 3)
    got, colors, keep = R.forward_views(torch.rand(3, 3), shs, torch.zeros(1, 3) + 5.0, 0)
    assert got[0, :, 0].tolist() == pre and keep[0, :, 0].tolist() == [False, True, True] and colors[0, :, 0].tolist() == [0.0, 0.0, pre[2]]
    assert R.clamp_bits(got[0]).tolist() == [7, 0, 0]
