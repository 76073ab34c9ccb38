"""The grouped head networks on the GPU (SplatFields(heads="grouped"); include/splatraster.h: sr_mlp_chain_group[_bf16],
sr_mlp_group_*): the group chain kernels bit for bit against the single-net kernels on the same op tables, the small kernels
against float64 formulas, the module against the float64 CPU formula path, the reference fixtures, determinism, the default
path untouched, and the launch budgets of the design."""
import pytest
import torch

import heads_reference as hr
from tests.heads_cases import (MODULE_CONFIGS, bound, build_net, chain_groups, cpu_references, default_specs, library, make_net,
                               module_inputs)
from tests.launches import device_records

pytestmark = pytest.mark.gpu
POINT_COUNTS = (1, 31, 32, 33, 127, 128, 129, 1000)      # the edges of a wavefront's 32 points and of a workgroup's 128
NEW_KERNELS = ("k_mlp_chain_group", "k_mlp_group_")


# ---- kernel against kernel ----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("precision", ["fp32", "bf16"])
@pytest.mark.parametrize("group", ["three_64", "two_128", "one_net", "net_limit"])
def test_group_chain_is_bit_identical_to_separate_chains(hip_device, group, precision):
    from splatfields_amd import _lib, fused_mlp as fm
    dev, lib, slope = hip_device, _lib.load(), 0.01
    shapes = chain_groups()[group]
    assert len(shapes) <= _lib.MLP_GROUP_MAX_NETS and (group != "net_limit" or len(shapes) == _lib.MLP_GROUP_MAX_NETS)
    for n in POINT_COUNTS:
        gen = torch.Generator().manual_seed(100 + n)
        nets = [make_net(s, n, gen, dev) for s in shapes]
        sep = []
        for s, (ws, bs, x0, dY) in zip(shapes, nets):        # n calls of sr_mlp_pack + sr_mlp_chain, forward and backward
            y, acts, signs = fm._forward(s, x0, ws, bs, slope, True, precision)
            dx0, G, dz = fm._backward(s, x0, acts, y, dY, ws, slope, True, signs, precision)
            sep.append((y, acts, signs, dx0, G, dz))
        ys = [torch.full_like(t[0], float("nan")) for t in sep]
        acts = [torch.full_like(t[1], float("nan")) for t in sep]
        signs = [torch.full_like(t[2], -1) for t in sep]
        ptrs = []
        for i, (s, (ws, bs, x0, _)) in enumerate(zip(shapes, nets)):
            H, L = s.hidden, s.n_layers
            ptrs.append({"W": [w.data_ptr() for w in ws], "B": [b.data_ptr() for b in bs], "x0": (x0.data_ptr(),), "y": (ys[i].data_ptr(),),
                         "acts": [acts[i].data_ptr() + 4 * j * n * H for j in range(L - 1)],
                         "signs": [signs[i].data_ptr() + 16 * j * n for j in range(L - 1)]})
        with torch.cuda.device(dev):
            keep = fm._group_plan("fwd", shapes, True, precision).run(lib, ptrs, dev, n, shapes[0].ht, slope, _lib.stream(dev))
        dzs = [torch.full_like(t[5], float("nan")) for t in sep]
        dx0s = [torch.full_like(t[3], float("nan")) for t in sep]
        ptrs = []
        for i, (s, (ws, bs, x0, _)) in enumerate(zip(shapes, nets)):
            H, L = s.hidden, s.n_layers
            ptrs.append({"W": [w.data_ptr() for w in ws], "G": (sep[i][4].data_ptr(),), "dx0": (dx0s[i].data_ptr(),),
                         "acts": [sep[i][1].data_ptr() + 4 * j * n * H for j in range(L - 1)],
                         "dz": [dzs[i].data_ptr() + 4 * j * n * H for j in range(L - 1)],
                         "signs": [sep[i][2].data_ptr() + 16 * j * n for j in range(L - 1)]})
        with torch.cuda.device(dev):
            keep2 = fm._group_plan("bwd", shapes, True, precision).run(lib, ptrs, dev, n, shapes[0].ht, slope, _lib.stream(dev))
        torch.cuda.synchronize()
        for i, t in enumerate(sep):
            assert torch.equal(ys[i], t[0]) and torch.isfinite(ys[i]).all(), (n, i, "y")
            assert torch.equal(acts[i], t[1]), (n, i, "saved activations")
            assert torch.equal(signs[i], t[2]), (n, i, "sign words")
            assert torch.equal(dzs[i], t[5]), (n, i, "dz")
            assert torch.equal(dx0s[i], t[3]) and torch.isfinite(dx0s[i]).all(), (n, i, "accumulated dL/dx0")
        del keep, keep2


# ---- the small kernels against float64 formulas ----------------------------------------------------------------------------------

def small_case(n, dev, seed=0):
    specs, tl = default_specs()
    gen = torch.Generator().manual_seed(seed + n)
    xyz = 1.5 * torch.randn(n, 3, generator=gen)
    feat = torch.randn(n, 16, generator=gen)
    time = torch.rand(n, generator=gen)
    return specs, tl, xyz, feat, time, gen


@pytest.mark.parametrize("n", [129, 1000])
def test_input_kernels_match_the_float64_formulas(hip_device, n):
    from splatfields_amd import _lib, fused_mlp as fm
    dev, lib = hip_device, _lib.load()
    specs, tl, xyz, feat, time, gen = small_case(n, dev)
    x0s = [torch.full((n, s.shape.mem_pad), float("nan"), device=dev) for s in specs]
    fm._group_input_forward(lib, specs, tl, xyz.to(dev), feat.to(dev), time.to(dev), x0s)
    for s, x0 in zip(specs, x0s):
        want = hr.input_matrix(xyz.double(), feat.double(), time.double(), s.multires, tl, s.shape.mem_pad)
        f32 = hr.input_matrix(xyz, feat, time, s.multires, tl, s.shape.mem_pad)
        d = (x0.double().cpu() - want).abs().max().item()
        print(f"input forward {s.name} n={n}: d / bound = {d / bound(want, f32):.3f}")
        assert d <= bound(want, f32), s.name
        assert (x0[:, s.shape.d_in:] == 0).all()
    # without features and without a time (the static network without an encoder)
    x0s = [torch.full((n, 32 * ((3 + 6 * s.multires + 31) // 32)), float("nan"), device=dev) for s in specs]
    table = fm._head_input_table(specs, x0s=x0s)
    for i, x0 in enumerate(x0s):
        table[i].row = x0.shape[1]
    xyz_dev = xyz.to(dev)
    _lib.check(lib.sr_mlp_group_input_forward(n, len(specs), table, 0, 0, _lib.ptr(xyz_dev), None, None, _lib.stream(dev)))
    for s, x0 in zip(specs, x0s):
        want = hr.input_matrix(xyz.double(), None, None, s.multires, 0, x0.shape[1])
        assert (x0.double().cpu() - want).abs().max().item() <= bound(want, hr.input_matrix(xyz, None, None, s.multires, 0, x0.shape[1])), s.name
    # more than eight octaves: the kernels restart their angle-doubling chains at octave 8 (multires 10 and 9, 0 beside them;
    # time_multires 9)
    many = (10, 9, 0)
    rows = [4 * ((3 + 6 * L + 16 + 1 + 2 * 9 + 3) // 4) for L in many]
    x0s = [torch.full((n, r), float("nan"), device=dev) for r in rows]
    gs = [torch.randn(n, r, generator=gen) for r in rows]
    gs_dev = [g.to(dev) for g in gs]
    table = (_lib.SrMlpHeadInput * 3)()
    for i, (L, r) in enumerate(zip(many, rows)):
        table[i].x0, table[i].dL_dx0, table[i].multires, table[i].row = x0s[i].data_ptr(), gs_dev[i].data_ptr(), L, r
    feat_dev, time_dev = feat.to(dev), time.to(dev)
    d_xyz, d_feat = torch.full((n, 3), float("nan"), device=dev), torch.full((n, 16), float("nan"), device=dev)
    _lib.check(lib.sr_mlp_group_input_forward(n, 3, table, 16, 9, _lib.ptr(xyz_dev), _lib.ptr(feat_dev), _lib.ptr(time_dev), _lib.stream(dev)))
    _lib.check(lib.sr_mlp_group_input_backward(n, 3, table, 16, _lib.ptr(xyz_dev), _lib.ptr(d_xyz), _lib.ptr(d_feat), _lib.stream(dev)))
    for L, r, x0 in zip(many, rows, x0s):
        want = hr.input_matrix(xyz.double(), feat.double(), time.double(), L, 9, r)
        d = (x0.double().cpu() - want).abs().max().item()
        print(f"input forward multires {L} n={n}: d / bound = {d / bound(want, hr.input_matrix(xyz, feat, time, L, 9, r)):.3f}")
        assert d <= bound(want, hr.input_matrix(xyz, feat, time, L, 9, r)), L
    want = hr.input_backward(xyz.double(), [g.double() for g in gs], many, 16)
    f32 = hr.input_backward(xyz, gs, many, 16)
    for name, got, w, f in (("d_xyz", d_xyz, want[0], f32[0]), ("d_feat", d_feat, want[1], f32[1])):
        d = (got.double().cpu() - w).abs().max().item()
        print(f"input backward {name} multires {many} n={n}: d / bound = {d / bound(w, f):.3f}")
        assert d <= bound(w, f), name
    # backward: the sum over the heads
    dx0s = [torch.randn(n, s.shape.mem_pad, generator=gen) for s in specs]
    for need_xyz, need_feat in ((True, True), (True, False), (False, True)):
        d_xyz = torch.full((n, 3), float("nan"), device=dev) if need_xyz else None
        d_feat = torch.full((n, 16), float("nan"), device=dev) if need_feat else None
        fm._group_input_backward(lib, specs, 16, xyz.to(dev), [g.to(dev) for g in dx0s], d_xyz, d_feat)
        want = hr.input_backward(xyz.double(), [g.double() for g in dx0s], [s.multires for s in specs], 16)
        f32 = hr.input_backward(xyz, dx0s, [s.multires for s in specs], 16)
        for name, got, w, f in (("d_xyz", d_xyz, want[0], f32[0]), ("d_feat", d_feat, want[1], f32[1])):
            if got is not None:
                d = (got.double().cpu() - w).abs().max().item()
                print(f"input backward {name} n={n}: d / bound = {d / bound(w, f):.3f}")
                assert d <= bound(w, f), name


@pytest.mark.parametrize("n", [129, 1000])
def test_output_and_top_gradient_kernels_match_the_float64_formulas(hip_device, n):
    from splatfields_amd import _lib, fused_mlp as fm
    dev, lib, slope = hip_device, _lib.load(), 0.01
    specs, tl, _, _, _, gen = small_case(n, dev, seed=7)
    ys = [torch.randn(n, s.shape.out_features, generator=gen) for s in specs]
    ys[1] = 8.0 * ys[1]                                    # opacity: a sigmoid driven to saturation
    ys[3] = 8.0 * ys[3]                                    # rgb
    tiny = torch.tensor([[3e-14, -1e-14, 0.0, 2e-14], [0.0, 0.0, 0.0, 0.0]])
    ys[2][:2] = tiny                                       # rotation rows with a norm below the clamp of F.normalize
    assert [s.activation for s in specs] == ["none", "sigmoid", "normalize", "sigmoid", "none"]
    ys_dev = [y.to(dev) for y in ys]
    outs = fm._group_output(lib, specs, ys_dev)
    for s, y, y_dev, out in zip(specs, ys, ys_dev, outs):
        if s.activation == "none":
            assert out is y_dev
            continue
        want = hr.output(y.double(), s.activation)
        d = (out.double().cpu() - want).abs().max().item()
        print(f"output {s.name} n={n}: d / bound = {d / bound(want, hr.output(y, s.activation)):.3f}")
        assert d <= bound(want, hr.output(y, s.activation)), s.name
    assert (outs[2][:2].cpu() == tiny / 1e-12).all() or (outs[2][:2].double().cpu() - tiny.double() / 1e-12).abs().max().item() <= 1e-8
    dOuts = [torch.randn(n, s.shape.out_features, generator=gen) for s in specs]
    dOuts[0] = None                                        # a head without upstream gradient
    Gs = [torch.full((n, s.shape.out_pad), float("nan"), device=dev) for s in specs]
    fm._group_top_gradient(lib, specs, ys_dev, [None if d is None else d.to(dev) for d in dOuts], slope, Gs)
    assert (Gs[0] == 0).all()
    for s, y, d, G in zip(specs, ys, dOuts, Gs):
        want = hr.top_gradient(y.double(), None if d is None else d.double(), s.activation, slope, s.shape.out_pad)
        f32 = hr.top_gradient(y, d, s.activation, slope, s.shape.out_pad)
        rows = [slice(None)] + ([slice(2, None)] if s.name == "rotations" else [])       # also without the rows below the clamp (1e12 large)
        for r in rows:
            err = (G.double().cpu()[r] - want[r]).abs().max().item()
            print(f"top gradient {s.name} n={n}: d / bound = {err / bound(want[r], f32[r]):.3f}")
            assert err <= bound(want[r], f32[r]), s.name
        assert (G[:, s.shape.out_features:] == 0).all()
    # rows below the clamp take the constant-norm branch: d / 1e-12
    want = dOuts[2][:2].double() / 1e-12 * torch.where(ys[2][:2] > 0, 1.0, slope).double()
    assert (Gs[2][:2, :4].double().cpu() - want).abs().max().item() <= 1e-6 * want.abs().max().item()


# ---- the module against the float64 CPU formula path --------------------------------------------------------------------------------

WORST = {}


@pytest.mark.parametrize("n", [129, 1000])
@pytest.mark.parametrize("precision", ["fp32", "bf16"])
@pytest.mark.parametrize("with_encoder", [False, True])
@pytest.mark.parametrize("name", sorted(MODULE_CONFIGS))
def test_grouped_module_matches_the_float64_formula_path(hip_device, name, with_encoder, precision, n):
    """d = max|grouped - f64| <= 4 r per tensor, r = max(error of the float32 CPU formula path, error of heads="separate" on the
    GPU in the same chain precision), floored at one float32 ulp of the tensor's maximum"""
    dev = hip_device
    state, probes, (out64, grad64), (out32, grad32) = cpu_references(name, with_encoder, n)
    xyz, t, viewdir, _ = module_inputs(n)
    net = build_net(name, with_encoder, mlp_precision=precision, heads="separate")
    net.load_state_dict(state)
    net = net.to(dev)
    args = (xyz.to(dev), t.to(dev), viewdir.to(dev), probes)
    out_sep, grad_sep = hr.step(net, *args)
    net.heads = "grouped"
    out_grp, grad_grp = hr.step(net, *args)
    assert net._head_group is not None and sorted(out_grp) == sorted(out64) and sorted(grad_grp) == sorted(grad64)
    worst = 0.0
    for kind, got, sep, f32, f64 in (("out", out_grp, out_sep, out32, out64), ("grad", grad_grp, grad_sep, grad32, grad64)):
        for k in f64:
            d = (got[k].double().cpu() - f64[k]).abs().max().item()
            b = bound(f64[k], f32[k], sep[k])
            worst = max(worst, d / b)
            assert got[k].shape == f64[k].shape and d <= b, (kind, k, d, b)
    WORST[(name, with_encoder, precision, n)] = worst
    print(f"grouped module {name} encoder={with_encoder} {precision} n={n}: worst d / 4r = {worst:.3f}")


# ---- fixtures, determinism, the default path, launch budgets -------------------------------------------------------------------------

@pytest.mark.parametrize("name", ["dynamic_dct", "dynamic_se3", "static_viewdep"])
def test_reference_fixtures_pass_grouped(hip_device, name, monkeypatch):
    import splatfields_amd
    from splatfields_amd import fused_mlp as fm
    from test_deform_field import run_case
    calls = []
    real = fm.fused_grouped_heads
    monkeypatch.setattr(fm, "fused_grouped_heads", lambda *a, **k: calls.append(1) or real(*a, **k))
    prev = splatfields_amd.set_heads("grouped")
    try:
        run_case(name, hip_device, 5e-5, 5e-4)
    finally:
        splatfields_amd.set_heads(prev)
    assert calls == [1]


def test_two_grouped_steps_are_bit_identical(hip_device):
    dev = hip_device
    xyz, t, viewdir, gen = module_inputs(1000)
    net = build_net("dynamic_se3", True, heads="grouped").to(dev)
    first, _ = hr.step(net, xyz.to(dev), t.to(dev), viewdir.to(dev), {k: torch.ones(1) for k in ("scales", "opacity", "rotations", "rgb", "flow", "means3D")})
    probes = {k: torch.randn(v.shape, generator=gen) for k, v in first.items()}
    a = hr.step(net, xyz.to(dev), t.to(dev), viewdir.to(dev), probes)
    b = hr.step(net, xyz.to(dev), t.to(dev), viewdir.to(dev), probes)
    for x, y in zip(a, b):
        for k in x:
            assert torch.equal(x[k], y[k]), k


def test_the_default_path_is_untouched(hip_device):
    """SplatFields() and heads="separate" are the same path bit for bit, and none of the new kernels runs on it"""
    import splatfields_amd
    dev = hip_device
    xyz, t, viewdir, gen = module_inputs(129)
    prev = splatfields_amd.set_heads("separate")           # the default, whatever the environment of this run says
    try:
        default = build_net("dynamic_se3", True).to(dev)
    finally:
        splatfields_amd.set_heads(prev)
    assert default.heads is None and default._head_group is None
    default.heads = "separate" if prev != "separate" else None
    named = build_net("dynamic_se3", True, heads="separate").to(dev)
    named.load_state_dict(default.state_dict())
    first, _ = hr.step(default, xyz.to(dev), t.to(dev), viewdir.to(dev), {k: torch.ones(1) for k in ("scales", "opacity", "rotations", "rgb", "flow", "means3D")})
    probes = {k: torch.randn(v.shape, generator=gen) for k, v in first.items()}
    held = {}
    names = device_records(lambda: held.update(a=hr.step(default, xyz.to(dev), t.to(dev), viewdir.to(dev), probes)))
    b = hr.step(named, xyz.to(dev), t.to(dev), viewdir.to(dev), probes)
    for x, y in zip(held["a"], b):
        for k in x:
            assert torch.equal(x[k], y[k]), k
    assert library(names), "the profiler recorded none of the library's kernels"
    assert not [n for n in names if any(new in n for new in NEW_KERNELS)]
    grouped = build_net("dynamic_se3", True, heads="grouped").to(dev)
    grouped.load_state_dict(default.state_dict())
    names = device_records(lambda: hr.step(grouped, xyz.to(dev), t.to(dev), viewdir.to(dev), probes))
    assert [n for n in names if "k_mlp_chain_group" in n] and [n for n in names if "k_mlp_group_" in n]


@pytest.mark.parametrize("precision", ["fp32", "bf16"])
@pytest.mark.parametrize("config", ["static", "dynamic"])
def test_launch_budgets(hip_device, config, precision):
    """conditions of the design: library launches of the heads alone (after xyz_can exists; without mlp_deform and the flow /
    view-colour tail) -- dynamic (five heads, rank 40, features): <= 8 forward, <= 20 backward; static (four heads, rank 0):
    <= 6 and <= 14 -- and fewer device kernels in the whole step than heads="separate" on the same module"""
    from splatfields_amd.deform_field import SplatFields
    dev, n = hip_device, 1000
    torch.manual_seed(5)
    if config == "dynamic":
        net = SplatFields(n_frames=10, heads="grouped", mlp_precision=precision, composition_rank=40, flow_model="se3", encoder=hr.LinearEncoder()).to(dev)
        budget = (8, 20)
    else:
        net = SplatFields(n_frames=0, heads="grouped", mlp_precision=precision, composition_rank=0, encoder=hr.LinearEncoder()).to(dev)
        budget = (6, 14)
    gen = torch.Generator().manual_seed(8)
    xyz = (0.6 * torch.randn(n, 3, generator=gen)).to(dev)
    t = torch.full((n, 1), 0.4, device=dev)
    xyz_can = xyz.clone().requires_grad_()
    feat = torch.randn(n, 16, generator=gen).to(dev).requires_grad_()
    frame = torch.tensor(4, device=dev) if config == "dynamic" else None
    held = {}

    def forward():
        held["out"] = net._head_group(xyz_can, feat, frame_id=frame, time=t.reshape(-1) if config == "dynamic" else None)

    forward()                                             # plans, tables and the allocator are warm
    fwd = library(device_records(forward))
    probes = {k: torch.randn(v.shape, generator=gen).to(dev) for k, v in held["out"].items()}
    loss = sum((held["out"][k] * probes[k]).sum() for k in sorted(probes))
    bwd = library(device_records(loss.backward))
    print(f"{config} {precision}: {len(fwd)} library launches forward, {len(bwd)} backward")
    assert fwd and bwd, "the profiler recorded none of the library's kernels"
    assert len(fwd) <= budget[0], fwd
    assert len(bwd) <= budget[1], bwd
    assert xyz_can.grad is not None and feat.grad is not None and net.mlp_scale.net[1].weight.grad is not None
    # the whole step, torch's kernels included, against heads="separate" on the same module
    totals = {}
    for mode in ("grouped", "separate"):
        net.heads = mode

        def step():
            out = net(xyz.clone().requires_grad_(), t)
            total = sum(v.sum() for k, v in sorted(out.items()) if torch.is_tensor(v))
            total.backward()

        step()
        names = device_records(step)
        assert library(names), "the profiler recorded none of the library's kernels"
        totals[mode] = len(names)
    print(f"{config} {precision}: {totals['grouped']} device kernels per step grouped, {totals['separate']} separate")
    assert totals["grouped"] < totals["separate"], totals
