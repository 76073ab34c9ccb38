"""Host side of the grouped head networks (splatfields_amd/fused_mlp.py: partition_heads, _GroupPlan, _GroupedHeadsFn;
general_mlp.HeadGroup; SplatFields(heads="grouped")) without a GPU: the partition, the group tables against each net's own
tables, splitting at the limits, a grouped step on the CPU with the launches interpreted, and the switch."""
import ctypes as C
import os
import subprocess
import sys
import types

import pytest
import torch

import heads_reference as hr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
QUICK = dict(encoder_type="none")


def fields_equal(a, b, skip=()):
    return all(getattr(a, f) == getattr(b, f) for f, _ in a._fields_ if f not in skip)


def test_partition_of_the_default_configurations():
    from splatfields_amd.deform_field import SplatFields
    static = SplatFields(n_frames=0, heads="grouped", **QUICK)
    assert static._head_group.partition() == [["scales", "opacity", "rotations"], ["rgb"]]
    dynamic = SplatFields(n_frames=5, heads="grouped", composition_rank=4, **QUICK)
    assert dynamic._head_group.partition() == [["scales", "opacity", "rotations"], ["rgb", "flow"]]
    viewdep = SplatFields(n_frames=0, heads="grouped", use_view_dep_rgb=True, **QUICK)
    assert viewdep._head_group.partition() == [["scales", "opacity", "rotations"], ["rgb"]]
    assert viewdep._head_group.specs[3].activation == "none" and static._head_group.specs[3].activation == "sigmoid"
    # the chain precision is part of the key: a bf16 net does not share a group with an fp32 net of its width
    assert dynamic._head_group.partition(("fp32", "bf16", "fp32", "bf16", "bf16")) == [["scales", "rotations"], ["opacity"], ["rgb", "flow"]]
    assert dynamic._head_group.partition(("bf16",) * 5) == [["scales", "opacity", "rotations"], ["rgb", "flow"]]
    # the residual layers of the default groups fit one ResField launch each (8 and 10 of 16)
    from splatfields_amd import _lib
    full = SplatFields(n_frames=5, heads="grouped", composition_rank=4)
    for members in (("mlp_scale", "mlp_opacity", "mlp_rotation"), ("mlp_rgb", "mlp_flow")):
        n = sum(1 for m in members for l in getattr(full, m).net if l.has_residual)
        assert n in (8, 10) and n <= _lib.RESFIELD_MAX_JOBS
    assert full._head_group.partition() == [["scales", "opacity", "rotations"], ["rgb", "flow"]]


@pytest.mark.parametrize("precision", ["fp32", "bf16"])
def test_group_tables_are_the_nets_own_tables_concatenated(precision):
    from splatfields_amd import _lib, fused_mlp as fm
    from splatfields_amd.deform_field import SplatFields
    net = SplatFields(n_frames=5, heads="grouped", composition_rank=4)
    specs = net._head_group.specs
    for members in net._head_group.spec((precision,) * 5).groups:
        shapes = [specs[i].shape for i in members]
        for kind, flag in (("fwd", True), ("fwd", False), ("bwd", True), ("bwd", False)):
            plan = fm._group_plan(kind, shapes, flag, precision)
            jobs, ops, nets, binds, total = plan.tables()
            assert len(nets) == len(members) <= _lib.MLP_GROUP_MAX_NETS and len(ops) == len(jobs) <= _lib.MLP_GROUP_MAX_OPS
            start, at = 0, 0
            for y, shape in enumerate(shapes):
                own = fm._forward_plan(shape, flag, precision) if kind == "fwd" else fm._backward_plan(shape, flag, True, precision)
                assert plan.plans[y] is own
                own._freeze()
                ojobs, oops, obinds, osize = own._arrays
                assert nets[y].n_ops == len(oops)
                assert C.addressof(nets[y].ops.contents) == C.addressof(ops) + start * C.sizeof(_lib.SrMlpOp)
                for j in range(len(oops)):       # every static field; pointer fields are patched per call
                    assert fields_equal(ops[start + j], oops[j], skip=("w_packed", "bias") + fm._OP_PTRS), (kind, y, j)
                    assert fields_equal(jobs[start + j], ojobs[j], skip=("dst", "bias_dst") + fm._PACK_PTRS), (kind, y, j)
                # the same symbolic pointers, net y's; packed matrices at the net's offset of the shared buffer
                mine = [(field, sym, idx, off) for obj, field, net_i, sym, idx, off in binds if net_i == y]
                theirs = [(field, sym, idx, off) for obj, field, sym, idx, off in obinds if sym != "buf"]
                assert mine == theirs
                start += len(oops)
                at += osize
            assert start == len(ops) and at == total and total % 16 == 0
            buf = [(field, off) for obj, field, net_i, sym, idx, off in binds if net_i is None]
            assert all(off % 16 == 0 and off < total for _, off in buf)


def test_splitting_at_the_net_and_op_limits(monkeypatch):
    from splatfields_amd import _lib, fused_mlp as fm
    from splatfields_amd.deform_field import SplatFields
    net = SplatFields(n_frames=5, heads="grouped", composition_rank=0)
    specs = net._head_group.specs
    counts = [fm.net_op_count(s.shape) for s in specs]
    assert counts == [9, 9, 6, 9, 9]               # the backward chains are the longer ones (the default configuration with features)
    plain = SplatFields(n_frames=5, heads="grouped", **QUICK)
    assert [fm.net_op_count(s.shape) for s in plain._head_group.specs] == [7, 7, 5, 9, 9]     # narrower inputs: one input-gradient op per layer
    fp = ("fp32",) * 5
    assert fm.partition_heads(specs, fp) == [[0, 1, 2], [3, 4]]
    monkeypatch.setattr(_lib, "MLP_GROUP_MAX_NETS", 2)
    assert fm.partition_heads(specs, fp) == [[0, 1], [2], [3, 4]]
    monkeypatch.setattr(_lib, "MLP_GROUP_MAX_NETS", 1)
    assert fm.partition_heads(specs, fp) == [[0], [1], [2], [3], [4]]          # a part of one net is a valid group
    monkeypatch.setattr(_lib, "MLP_GROUP_MAX_NETS", 8)
    monkeypatch.setattr(_lib, "MLP_GROUP_MAX_OPS", 18)
    assert fm.partition_heads(specs, fp) == [[0, 1], [2], [3, 4]]
    monkeypatch.setattr(_lib, "MLP_GROUP_MAX_OPS", 17)
    assert fm.partition_heads(specs, fp) == [[0], [1, 2], [3], [4]]
    monkeypatch.setattr(_lib, "MLP_GROUP_MAX_OPS", 8)
    with pytest.raises(ValueError, match="do not fit"):
        fm.partition_heads(specs, fp)
    monkeypatch.undo()
    # many nets of one width: no group's table exceeds either limit
    many = [specs[i % 3] for i in range(20)]
    groups = fm.partition_heads(many, ("fp32",) * 20)
    assert [i for g in groups for i in g] == list(range(20))
    for g in groups:
        assert len(g) <= _lib.MLP_GROUP_MAX_NETS and sum(fm.net_op_count(many[i].shape) for i in g) <= _lib.MLP_GROUP_MAX_OPS
        fm._GroupPlan([fm._backward_plan(many[i].shape, True, True) for i in g]).tables()
    with pytest.raises(ValueError, match="too many nets or ops"):
        fm._GroupPlan([fm._backward_plan(specs[0].shape, True, True)] * 5).tables()
    with pytest.raises(ValueError, match="too many nets or ops"):
        fm._GroupPlan([fm._forward_plan(specs[2].shape, True)] * 9).tables()
    # the header's limits keep the table a kernel argument
    assert 4 + 4 * (_lib.MLP_GROUP_MAX_NETS + 1) + _lib.MLP_GROUP_MAX_OPS * C.sizeof(_lib.SrMlpOp) + 8 < 4096


def test_compose_is_called_once_per_group(monkeypatch):
    from splatfields_amd import general_mlp
    from splatfields_amd.deform_field import SplatFields
    net = SplatFields(n_frames=5, heads="grouped", composition_rank=4, **QUICK)
    calls = []
    real = general_mlp.compose_resfield_weights
    monkeypatch.setattr(general_mlp, "compose_resfield_weights", lambda layers, frame_id: calls.append(len(layers)) or real(layers, frame_id))
    group = [net.mlp_scale, net.mlp_opacity, net.mlp_rotation]
    ws = general_mlp.compose_group_weights(group, 2)
    assert calls == [6 + 6 + 5] and [len(w) for w in ws] == [6, 6, 5]
    for m, w in zip(group, ws):
        for layer, got in zip(m.net, w):
            assert torch.equal(got, layer.effective(2))
    monkeypatch.setattr(general_mlp._lib, "RESFIELD_MAX_JOBS", 5)
    calls.clear()
    general_mlp.compose_group_weights(group, 2)
    assert calls == [6, 6 + 5]                     # 3 | 3 + 2 residual layers


CONFIGS = {
    "static": dict(n_frames=0, kwargs=dict(QUICK)),
    "dynamic_se3": dict(n_frames=6, kwargs=dict(QUICK, composition_rank=3, flow_model="se3")),
    "viewdep": dict(n_frames=0, kwargs=dict(QUICK, use_view_dep_rgb=True, rgb_w=64)),
}


@pytest.mark.parametrize("with_encoder", [False, True])
@pytest.mark.parametrize("name", sorted(CONFIGS))
def test_grouped_step_on_the_cpu_matches_the_float64_formula_path(monkeypatch, name, with_encoder):
    """every output and gradient of a grouped step (launches interpreted, small kernels as formulas) against the separate
    formula path in float64, within the CPU tolerances of tests/test_deform_field.py (2e-5 outputs, 2e-4 gradients)"""
    from splatfields_amd.deform_field import SplatFields
    cfg = CONFIGS[name]
    torch.manual_seed(3)
    enc = dict(encoder=hr.LinearEncoder()) if with_encoder else {}
    net = SplatFields(n_frames=cfg["n_frames"], heads="grouped", **enc, **cfg["kwargs"])
    n = 37
    g = torch.Generator().manual_seed(5)
    xyz = 0.7 * torch.randn(n, 3, generator=g)
    t = torch.full((n, 1), 0.4)
    viewdir = torch.nn.functional.normalize(torch.randn(n, 3, generator=g), dim=-1)
    counts = hr.on_cpu(monkeypatch)
    net.heads = "separate"
    probe_out, _ = hr.step(net, xyz, t, viewdir, {k: 1.0 * torch.ones(1) for k in ("scales", "opacity", "rotations", "rgb", "flow", "means3D")})
    probes = {k: torch.randn(v.shape, generator=g) for k, v in probe_out.items()}
    assert not counts
    ref = SplatFields(n_frames=cfg["n_frames"], heads="separate", **({"encoder": hr.LinearEncoder()} if with_encoder else {}), **cfg["kwargs"]).double()
    ref.load_state_dict({k: v.double() for k, v in net.state_dict().items()})
    want_out, want_grad = hr.step(ref, xyz.double(), t.double(), viewdir.double(), probes)
    net.heads = "grouped"
    got_out, got_grad = hr.step(net, xyz, t, viewdir, probes)
    n_groups = len(net._head_group.partition())
    assert n_groups == (1 if name == "viewdep" else 2)      # rgb_w=64 is also the colour net's hidden width: one 64-wide group
    assert counts == {"input_forward": 1, "chain_group": 2 * n_groups, "output": 1, "top_gradient": 1, "input_backward": 1}
    assert sorted(got_out) == sorted(want_out)
    for k in want_out:
        assert got_out[k].dtype == torch.float32
        assert (got_out[k].double() - want_out[k]).abs().max().item() <= 2e-5 * max(want_out[k].abs().max().item(), 1e-6), k
    assert sorted(got_grad) == sorted(want_grad)
    for k in want_grad:
        err = (got_grad[k].double() - want_grad[k]).abs().max().item()
        assert err <= 2e-4 * want_grad[k].abs().max().item() + 1e-8, (k, err)


@pytest.mark.parametrize("name", ["dynamic_se3", "dynamic_dct", "static_viewdep"])
def test_fixtures_pass_grouped_on_the_cpu(monkeypatch, name):
    import splatfields_amd
    from test_deform_field import run_case
    counts = hr.on_cpu(monkeypatch)
    prev = splatfields_amd.set_heads("grouped")
    try:
        run_case(name, torch.device("cpu"), 2e-5, 2e-4)
    finally:
        splatfields_amd.set_heads(prev)
    assert counts.get("chain_group") in (2, 4) and counts.get("input_forward") == 1 and counts.get("input_backward") == 1


def test_a_head_without_upstream_gradient_and_calls_the_input_kernel_cannot_take(monkeypatch):
    from splatfields_amd import fused_mlp as fm
    from splatfields_amd.deform_field import SplatFields
    torch.manual_seed(1)
    net = SplatFields(n_frames=0, heads="grouped", **QUICK)
    xyz = torch.randn(9, 3)
    # CPU tensors, as they are: the per-call check sends the step down the separate path (here: its formula stand-in)
    assert not fm.grouped_inputs_ok(xyz, None, None)
    counts = hr.on_cpu(monkeypatch)
    x = xyz.clone().requires_grad_()
    out = net(x, None)
    (out["opacity"].sum() + out["means3D"].sum()).backward()           # scales, rotations and rgb receive no gradient
    assert counts["top_gradient"] == 1
    assert net.mlp_scale.net[0].weight.grad.abs().max().item() == 0 and net.mlp_opacity.net[0].weight.grad.abs().max().item() > 0
    net.heads = "separate"
    x2 = xyz.clone().requires_grad_()
    out2 = net(x2, None)
    (out2["opacity"].sum() + out2["means3D"].sum()).backward()
    assert (x.grad - x2.grad).abs().max().item() <= 1e-5 * x2.grad.abs().max().item()
    # no points: the separate path
    monkeypatch.undo()
    assert not fm.grouped_inputs_ok(torch.zeros(0, 3), None, None)


def test_the_switch():
    """keyword > set_heads > SPLATFIELDS_HEADS > "separate"; the keyword also arrives through SplatFieldsModel's hyper_args"""
    import splatfields_amd
    from splatfields_amd import fused_mlp as fm
    from splatfields_amd.deform_field import SplatFields, SplatFieldsModel
    assert os.environ.get("SPLATFIELDS_HEADS") or splatfields_amd.heads() == "separate"
    assert fm.HEADS == ("separate", "grouped")
    small = dict(QUICK, deform_d=2, rgb_d=2, flow_d=2, scale_d=2, opacity_d=2, rotation_d=2, deform_skips=[0], rgb_skips=[0], flow_skips=[0],
                 scale_skips=[0], opacity_skips=[], rotation_skips=[])
    prev = splatfields_amd.set_heads("grouped")
    try:
        assert splatfields_amd.heads() == "grouped" and fm.resolve_heads(None) == "grouped" and fm.resolve_heads("separate") == "separate"
        assert SplatFields(n_frames=3, **small)._head_group is not None             # the process default, checked at construction
        assert SplatFields(n_frames=3, heads="separate", **small)._head_group is None
        assert splatfields_amd.set_heads("separate") == "grouped" and fm.resolve_heads(None) == "separate" and fm.resolve_heads("grouped") == "grouped"
        with pytest.raises(ValueError, match="unknown heads mode"):
            splatfields_amd.set_heads("fused")
        assert splatfields_amd.heads() == "separate"
    finally:
        splatfields_amd.set_heads(prev)
    with pytest.raises(ValueError, match="unknown heads mode"):
        SplatFields(n_frames=3, heads="fused", **small)
    default = SplatFields(n_frames=3, **small)
    assert default.heads is None and (default._head_group is None or splatfields_amd.heads() == "grouped")
    assert SplatFields(n_frames=3, heads="grouped", **small).heads == "grouped"
    model = SplatFieldsModel(types.SimpleNamespace(n_frames=3, heads="grouped", **small), device="cpu")
    assert model.deform.heads == "grouped" and model.deform._head_group.partition() == [["scales", "opacity", "rotations"], ["rgb", "flow"]]
    assert list(default.state_dict()) == list(model.deform.state_dict())              # the state dict does not know the mode
    # impossible at construction: the reason is named
    with pytest.raises(ValueError, match="geo_model_disable_pts"):
        SplatFields(n_frames=3, heads="grouped", geo_model_disable_pts=True, **small)
    SplatFields(n_frames=3, geo_model_disable_pts=True, **small)
    with pytest.raises(ValueError, match="hidden widths 64 and 128"):
        SplatFields(n_frames=3, heads="grouped", **dict(small, scale_w=96))
    from splatfields_amd.general_mlp import GeneralMLP, HeadGroup
    with pytest.raises(ValueError, match="output activation 'tanh'"):
        HeadGroup([("a", GeneralMLP(in_features=3, out_features=3, hidden_features=64, num_hidden_layers=2, skips=[], multires=2,
                                    out_activation="tanh", act="leaky_relu"))])
    code = "import splatfields_amd as s; from splatfields_amd import fused_mlp as f; print(s.heads(), f.resolve_heads(None), f.resolve_heads('separate'))"
    for value, want in (("grouped", "grouped grouped separate"), ("", "separate separate separate")):
        out = subprocess.run([sys.executable, "-c", code], cwd=ROOT, env=dict(os.environ, SPLATFIELDS_HEADS=value), capture_output=True, text=True)
        assert out.returncode == 0 and out.stdout.strip() == want, (value, out.stdout, out.stderr)
    bad = subprocess.run([sys.executable, "-c", code], cwd=ROOT, env=dict(os.environ, SPLATFIELDS_HEADS="fused"), capture_output=True, text=True)
    assert bad.returncode != 0 and "unknown heads mode" in bad.stderr
