"""`FlowHead` (splatfields_amd/deform_field.py) on its PyTorch-op path against the reference's own class for all seven flow models:
the fixtures of tests/golden/make_flow_head_golden.py hold the reference's state dict, inputs, `flow`, `means3D` and every input
and parameter gradient of sum(probe . output), evaluated in float32 and in float64.

  * float64: both sides are float64 evaluations of the same formulas: 1e-12 relative to each tensor's largest magnitude (the bound
    of the splatfields_* goldens);
  * float32: d = max |ours32 - reference64| is at most 4 r, r = max |reference32 - reference64| on the same inputs.  r is floored at
    one float32 ulp of the tensor's largest magnitude, as everywhere in this suite: a float32 result cannot be asked to be nearer
    than its own spacing, and where the reference happens to be exact (r = 0: the sum of a handful of probes) the rule would
    otherwise demand exactness of a differently ordered sum."""
import json
import os

import numpy as np
import pytest
import torch

from splatfields_amd.deform_field import FLOW_MODELS, FlowHead, SplatFields, dct_basis, se3_transform

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
W, K, N_FRAMES = 32, 4, 6


@pytest.fixture(scope="module")
def cases():
    z = np.load(os.path.join(GOLDEN, "flow_head_cases.npz"))
    return {k: torch.as_tensor(z[k]) for k in z.files}


def evaluate(cases, model, dtype, path="torch"):
    pre = model + "/"
    state = {k[len(pre + "param/"):]: v.to(dtype) for k, v in cases.items() if k.startswith(pre + "param/")}
    head = FlowHead(W=W, flow_model=model, num_basis=K, n_frames=N_FRAMES, path=path).to(dtype)
    head.load_state_dict(state, strict=True)
    hidden = cases[pre + "hidden"].to(dtype).requires_grad_()
    pts = cases[pre + "pts"].to(dtype).requires_grad_()
    flow, means = head(hidden, pts, time_step=cases[pre + "time_step"].to(dtype), frame_id=cases[pre + "frame_id"])
    ((flow * cases[pre + "probe_flow"].to(dtype)).sum() + (means * cases[pre + "probe_means"].to(dtype)).sum()).backward()
    out = {"flow": flow.detach(), "means3D": means.detach(), "grad/hidden": hidden.grad, "grad/pts": pts.grad}
    for k, p in head.named_parameters():
        out["grad/" + k] = p.grad if p.grad is not None else torch.zeros_like(p)
    return out


def reference(cases, model, tag):
    pre = f"{model}/{tag}/"
    return {k[len(pre):]: v for k, v in cases.items() if k.startswith(pre)}


@pytest.mark.parametrize("model", FLOW_MODELS)
def test_state_dict_keys_are_the_references_and_load_strictly(cases, model):
    keys = json.load(open(os.path.join(GOLDEN, "flow_head_keys.json")))
    assert set(keys) == set(FLOW_MODELS)
    head = FlowHead(W=W, flow_model=model, num_basis=K, n_frames=N_FRAMES)
    assert list(head.state_dict()) == keys[model]
    pre = model + "/param/"
    state = {k[len(pre):]: v for k, v in cases.items() if k.startswith(pre)}
    assert set(state) == set(keys[model])
    head.load_state_dict(state, strict=True)
    for k, v in head.state_dict().items():
        assert v.shape == state[k].shape and torch.equal(v, state[k]), k


def test_parameter_shapes_and_initialisation():
    assert tuple(FlowHead(W=W, flow_model="affine").branch_w.weight.shape) == (9, W)
    assert tuple(FlowHead(W=W, flow_model="se3Scaled").branch_scale.weight.shape) == (1, W)
    for model in ("dct", "dct_siren"):
        head = FlowHead(W=W, flow_model=model, num_basis=K, n_frames=N_FRAMES)
        assert torch.count_nonzero(head.branch_coeff.weight) == 0 and torch.count_nonzero(head.branch_coeff.bias) == 0
    net = FlowHead(W=W, flow_model="dct_siren", num_basis=K, n_frames=N_FRAMES).basis_net.net
    assert [tuple(l.weight.shape) for l in net] == [(128, 1), (128, 128), (K, 128)]
    assert net[0].weight.abs().max() <= 1.0 and net[0].weight.abs().max() > 0.5                 # +-1 / fan_in, fan_in = 1
    bound = (6.0 / 128) ** 0.5 / 30
    assert net[1].weight.abs().max() <= bound and net[1].weight.abs().max() > 0.9 * bound       # +-sqrt(6 / fan_in) / 30
    with pytest.raises(NotImplementedError):
        FlowHead(W=W, flow_model="spline")


@pytest.mark.parametrize("model", FLOW_MODELS)
def test_float64_reproduces_the_reference(cases, model):
    got, ref = evaluate(cases, model, torch.float64), reference(cases, model, "f64")
    assert set(got) == set(ref)
    for k, r in ref.items():
        assert got[k].dtype == torch.float64 and got[k].shape == r.shape, k
        top = r.abs().max().item()
        d = (got[k] - r).abs().max().item()
        assert d <= 1e-12 * max(top, 1e-300), (model, k, d, top)


@pytest.mark.parametrize("model", FLOW_MODELS)
def test_float32_is_within_four_times_the_references_own_error(cases, model):
    got, r64, r32 = evaluate(cases, model, torch.float32), reference(cases, model, "f64"), reference(cases, model, "f32")
    for k, w in r64.items():
        assert got[k].dtype == torch.float32, k
        top = w.abs().max().item()
        r = max((r32[k].double() - w).abs().max().item(), float(np.spacing(np.float32(top))))
        d = (got[k].double() - w).abs().max().item()
        print(f"[flow_head] {model} {k}: d/4r {d / (4 * r):.3f}")
        assert d <= 4 * r, (model, k, d, 4 * r)


@pytest.mark.parametrize("model", FLOW_MODELS)
def test_splatfields_constructs_and_runs_with_every_flow_model(monkeypatch, model):
    """on CPU tensors, with the fused MLP op replaced by its formula as tests/test_deform_field.py does"""
    from splatfields_amd import general_mlp
    from test_general_mlp import formula
    monkeypatch.setattr(general_mlp, "fused_general_mlp", formula)
    torch.manual_seed(3)
    net = SplatFields(n_frames=6, flow_model=model, encoder_type="none", deform_d=2, rgb_d=2, scale_d=2, opacity_d=2, rotation_d=2, flow_d=2,
                      deform_skips=[], rgb_skips=[], scale_skips=[], opacity_skips=[], rotation_skips=[], flow_skips=[])
    assert net.mlp_flow_head.flow_model == model and net.mlp_flow_head.path is None
    with torch.no_grad():
        if model in ("dct", "dct_siren"):
            net.mlp_flow_head.branch_coeff.weight.normal_(std=0.1)
    x = torch.rand(50, 3) * 2 - 1
    out = net(x, torch.full((50, 1), 0.4))
    assert tuple(out["means3D"].shape) == (50, 3) and tuple(out["flow"].shape) == ((50, 4, 4) if model == "se3" else (50, 3))
    assert torch.isfinite(out["means3D"]).all() and torch.isfinite(out["flow"]).all()
    out["means3D"].sum().backward()
    grads = [p.grad for p in net.mlp_flow_head.parameters() if p.grad is not None]
    assert grads and all(torch.isfinite(g).all() for g in grads)


def test_the_three_earlier_models_are_bit_for_bit_what_they_were(cases):
    """the formulas of the head before the other four models arrived, called directly"""
    for model in ("offset", "se3", "dct"):
        pre = model + "/"
        state = {k[len(pre + "param/"):]: v for k, v in cases.items() if k.startswith(pre + "param/")}
        head = FlowHead(W=W, flow_model=model, num_basis=K, n_frames=N_FRAMES)
        head.load_state_dict(state)
        hidden, pts, frame_id = cases[pre + "hidden"], cases[pre + "pts"], cases[pre + "frame_id"]
        lin = lambda name: torch.nn.functional.linear(hidden, state[name + ".weight"], state[name + ".bias"])
        if model == "offset":
            flow = lin("gaussian_warp")
            means = pts + flow
        elif model == "se3":
            w, v = lin("branch_w"), lin("branch_v")
            theta = torch.norm(w, dim=-1, keepdim=True)
            flow = se3_transform(w / theta + 1e-5, v / theta + 1e-5, theta)
            means = (flow[:, :3, :3] * pts[:, None, :]).sum(-1) + flow[:, :3, 3]
        else:
            coeff = lin("branch_coeff").view(-1, 3, K)
            flow = (coeff * state["trajectory_basis"][frame_id.long()].view(1, 1, -1)).sum(-1)
            means = pts + flow
        with torch.no_grad():
            got_flow, got_means = head(hidden, pts, time_step=cases[pre + "time_step"], frame_id=frame_id)
        assert torch.equal(got_flow, flow) and torch.equal(got_means, means), model
    assert torch.equal(FlowHead(W=W, flow_model="dct", num_basis=K, n_frames=N_FRAMES).trajectory_basis, dct_basis(K, 2 * N_FRAMES))
