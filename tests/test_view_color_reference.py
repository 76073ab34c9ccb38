"""The view-dependent colour head on its PyTorch-op path against what the reference computes for V = 3 views of one step
(tests/golden/view_color_cases.npz, made by tests/golden/make_view_color_golden.py from the reference's own SplatFields and the
expressions of its render()), and the `ViewColor` object `out["rgb_fnc"]` has become against the lambda it replaces."""
import os

import numpy as np
import pytest
import torch

from test_deform_field import case_config
from test_general_mlp import GOLDEN, formula

FIXTURE = os.path.join(GOLDEN, "view_color_cases.npz")


def load_fixture():
    data = np.load(FIXTURE)
    assert all(data[k].dtype in (np.float32, np.float64) for k in data.files)      # arrays of numbers only
    return data


def build_network(data, dtype, **extra):
    from splatfields_amd.deform_field import SplatFields
    n_frames, kwargs, _ = case_config("static_viewdep")
    net = SplatFields(radius=None, n_frames=n_frames, **kwargs, **extra)
    state = {k[len("param:"):]: torch.from_numpy(data[k]) for k in data.files if k.startswith("param:")}
    assert {k: tuple(v.shape) for k, v in net.state_dict().items()} == {k: tuple(v.shape) for k, v in state.items()}
    net.load_state_dict(state, strict=True)
    return net.to(dtype)


def run_fixture(data, dtype, device, **extra):
    """colours [V, N, 3] through for_cameras on the network's own means3D, and every gradient of sum_v (probe_v . colour_v).sum()"""
    net = build_network(data, dtype, **extra).to(device)
    xyz = torch.from_numpy(data["xyz"]).to(dtype).to(device).requires_grad_()
    out = net(xyz, torch.from_numpy(data["t"]).to(dtype).to(device))
    colours = out["rgb_fnc"].for_cameras(out["means3D"], torch.from_numpy(data["centres"]).to(dtype).to(device))
    (colours * torch.from_numpy(data["probes"]).to(dtype).to(device)).sum().backward()
    res = {"colours": colours.detach(), "means3D": out["means3D"].detach(), "grad_xyz": xyz.grad}
    for k, p in net.named_parameters():
        res["grad:" + k] = p.grad if p.grad is not None else torch.zeros_like(p)
    return res


@pytest.fixture()
def formula_mlp(monkeypatch):
    from splatfields_amd import general_mlp
    monkeypatch.setattr(general_mlp, "fused_general_mlp", formula)


def test_torch_path_reproduces_the_float64_record_to_float64_rounding(formula_mlp):
    data = load_fixture()
    got = run_fixture(data, torch.float64, torch.device("cpu"))
    assert set(got) == {k[len("f64/"):] for k in data.files if k.startswith("f64/")}
    assert tuple(got["colours"].shape) == (3, 32, 3)
    for k, v in got.items():
        want = torch.from_numpy(data["f64/" + k])
        assert want.dtype == torch.float64 and v.shape == want.shape, k
        # a few hundred float64 roundings in another order (the MLP formula's matmuls), relative to the tensor's largest magnitude
        assert (v - want).abs().max().item() <= 1e-12 * max(want.abs().max().item(), 1e-30), k


def test_torch_path_reproduces_the_float32_record_within_the_network_bound(formula_mlp):
    """the bounds of tests/test_deform_field.py::test_host_side_matches_the_reference_network: outputs 2e-5 and gradients 2e-4 of
    the tensor's largest magnitude (+ 1e-8)"""
    data = load_fixture()
    got = run_fixture(data, torch.float32, torch.device("cpu"))
    for k, v in got.items():
        want = torch.from_numpy(data["f32/" + k])
        err, top = (v - want).abs().max().item(), want.abs().max().item()
        if k.startswith("grad"):
            assert err <= 2e-4 * top + 1e-8, (k, err, top)
        else:
            assert err <= 2e-5 * max(top, 1e-6), (k, err, top)


def small_network(**extra):
    from splatfields_amd.deform_field import SplatFields
    torch.manual_seed(3)
    quick = dict(encoder_type="none", deform_d=2, rgb_d=2, scale_d=2, opacity_d=2, rotation_d=2, deform_skips=[0], rgb_skips=[0], scale_skips=[0],
                 opacity_skips=[0], rgb_w=64, use_view_dep_rgb=True)
    return SplatFields(n_frames=0, **quick, **extra)


def test_the_call_with_a_view_direction_is_the_expression_it_replaces(formula_mlp):
    from splatfields_amd.deform_field import ViewColor
    net = small_network()
    xyz = torch.rand(50, 3) * 2 - 1
    out = net(xyz, torch.zeros(50, 1))
    fnc = out["rgb_fnc"]
    assert isinstance(fnc, ViewColor) and fnc.path == "torch" and "rgb" not in out
    viewdir = torch.nn.functional.normalize(torch.randn(50, 3), dim=-1)
    want = net.mlp_rgb_viewdep(torch.cat([fnc.feature, viewdir], dim=-1))
    assert torch.equal(fnc(viewdir), want)
    assert isinstance(net.mlp_rgb_viewdep, torch.nn.Sequential) and list(net.mlp_rgb_viewdep.state_dict()) == ["0.weight", "0.bias"]


def test_for_cameras_on_the_torch_path_is_the_per_view_loop(formula_mlp):
    net = small_network()
    centres = torch.nn.functional.normalize(torch.randn(4, 3), dim=-1) * 3.5
    probes = torch.randn(4, 50, 3)
    x0 = torch.rand(50, 3) * 2 - 1
    results = []
    for batched in (True, False):
        net.zero_grad(set_to_none=True)
        xyz = x0.clone().requires_grad_()
        out = net(xyz, torch.zeros(50, 1))
        means3D, fnc = out["means3D"], out["rgb_fnc"]
        if batched:
            colours = fnc.for_cameras(means3D, centres)
            assert tuple(colours.shape) == (4, 50, 3)
            (colours * probes).sum().backward()
        else:       # what render() does per view, every view's loss added to one scalar, one backward: autograd accumulates
            per_view = []
            for c in centres:
                ray_d = means3D - c[None]
                ray_d = ray_d / torch.norm(ray_d, dim=-1, keepdim=True)
                per_view.append(net.mlp_rgb_viewdep(torch.cat([fnc.feature, ray_d], dim=-1)))
            colours = torch.stack(per_view)
            (colours * probes).sum().backward()
        results.append([colours.detach(), xyz.grad] + [p.grad for p in net.parameters() if p.grad is not None])
    assert len(results[0]) == len(results[1]) > 4
    for a, b in zip(*results):
        assert torch.equal(a, b)


def test_the_fused_path_has_no_cpu_path_and_refuses_what_the_kernels_cannot_run(formula_mlp):
    from splatfields_amd.deform_field import SplatFields
    from splatfields_amd.view_color import fused_view_color
    net = small_network(view_color="fused")
    out = net(torch.rand(5, 3), torch.zeros(5, 1))
    assert out["rgb_fnc"].path == "fused"
    with pytest.raises(RuntimeError, match="no CPU path"):
        out["rgb_fnc"](torch.randn(5, 3))
    with pytest.raises(RuntimeError, match="no CPU path"):
        out["rgb_fnc"].for_cameras(out["means3D"], torch.randn(2, 3))
    f, w, b = torch.randn(5, 8), torch.randn(3, 11), torch.randn(3)
    with pytest.raises(RuntimeError, match="no CPU path"):
        fused_view_color(f, w, b, dirs=torch.randn(1, 5, 3))
    for kw in (dict(), dict(means3D=torch.randn(5, 3)), dict(camera_centers=torch.randn(2, 3)),
               dict(means3D=torch.randn(5, 3), camera_centers=torch.randn(2, 3), dirs=torch.randn(2, 5, 3))):
        with pytest.raises(ValueError, match="either"):
            fused_view_color(f, w, b, **kw)
    quick = dict(encoder_type="none", deform_d=2, rgb_d=2, scale_d=2, opacity_d=2, rotation_d=2, deform_skips=[0], rgb_skips=[0], scale_skips=[0],
                 opacity_skips=[0], use_view_dep_rgb=True)
    for rgb_w in (130, 260, 2):
        with pytest.raises(ValueError, match="fused"):
            SplatFields(n_frames=0, rgb_w=rgb_w, view_color="fused", **quick)
        SplatFields(n_frames=0, rgb_w=rgb_w, **quick)              # the PyTorch-op path has no such limit
    SplatFields(n_frames=0, rgb_w=130, view_color="fused", **dict(quick, use_view_dep_rgb=False))      # no such head: nothing to refuse
