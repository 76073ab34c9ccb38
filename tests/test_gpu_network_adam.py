"""NetworkAdam (splatfields_amd/network_optim.py -> sr_net_adam_step, csrc/network_adam.hip) on the MI355X.

The main statement is bitwise: the same initial values and the same gradient sequence through NetworkAdam and through SplatAdam
(tests/test_gpu_adam.py holds that one against torch) give torch.equal parameters and moments for every tensor -- sizes around the
vector width and the chunk, more tensors than one launch takes, gradients and parameters off the 16-byte boundary, two sets of
scalars, tensors that start stepping later.  Against torch.optim.Adam the rule is test_gpu_adam.py's, with its generators:
truth float64 on the CPU, yardstick float32 on the CPU, allowance 4 x the yardstick's max-abs deviation per tensor and kind, the
tensors of a handful of elements of one launch pooled.  The launch budget is counted with torch.profiler."""
import copy
import math
import types

import pytest
import torch
from torch import nn

import test_gpu_adam as A
from tests.launches import device_records

pytestmark = pytest.mark.gpu

KINDS = A.KINDS
SIZES_A = (1, 3, 4, 5, 7, 2047, 2048, 2049, 4099, 3 * 2048 + 1)
HANDFUL = 8                                                            # tensors of at most this many elements are pooled


def network_adam(*a, **k):
    from splatfields_amd import NetworkAdam
    return NetworkAdam(*a, **k)


def inputs(sizes, steps, seed, skip=None):
    """initial values and `steps` gradients per tensor; skip(step, tensor) -> True: no gradient there"""
    gen = torch.Generator().manual_seed(seed)
    init = [torch.randn(s, generator=gen) for s in sizes]
    seq = [[None if skip and skip(s, i) else A.gradients(tuple(t.shape), "uniform", gen) for i, t in enumerate(init)] for s in range(steps)]
    return init, seq


def offset_view(t, shift):
    """the values of t in storage that starts `shift` floats past a 16-byte boundary, zeros around them"""
    buf = torch.zeros(t.numel() + 8, device=t.device, dtype=t.dtype)
    buf[shift:shift + t.numel()] = t.reshape(-1)
    out = buf[shift:shift + t.numel()].reshape(t.shape)
    assert out.data_ptr() % 16 == 4 * shift and out.is_contiguous()
    return out


def drive(make, init, seq, dev, groups=None, place=None, grad_place=None, schedule=None):
    """groups: [(tensor indices, options)] (default: one group, lr 1e-3, eps 1e-15); place / grad_place(i, tensor) -> where the
    parameter / the gradient lies; schedule[s]: the learning rates written into the groups before step s."""
    place = place or (lambda i, t: t.clone())
    grad_place = grad_place or (lambda i, g: g)
    params = [nn.Parameter(place(i, t.to(dev))) for i, t in enumerate(init)]
    groups = groups or [(range(len(init)), dict(lr=1e-3))]
    opt = make([dict(params=[params[i] for i in idx], **kw) for idx, kw in groups], lr=0.0, eps=1e-15)
    for s, grads in enumerate(seq):
        if schedule is not None:
            for group, lr in zip(opt.param_groups, schedule[s]):
                group["lr"] = lr
        for i, (p, g) in enumerate(zip(params, grads)):
            p.grad = None if g is None else grad_place(i, g.to(dev))
        opt.step()
    return A.snapshot(opt, params), opt, params


def assert_bitwise(got, want, tag=""):
    assert len(got) == len(want)
    for i, (a, b) in enumerate(zip(got, want)):
        assert a["step"] == b["step"], (tag, i, a["step"], b["step"])
        for kind in KINDS:
            if b[kind] is None:
                assert a[kind] is None, (tag, i, kind)
            else:
                assert a[kind] is not None and torch.equal(a[kind].view(torch.int32), b[kind].view(torch.int32)), (tag, i, kind)


def both(init, seq, dev, **kw):
    net, opt, params = drive(network_adam, init, seq, dev, **kw)
    splat = drive(A.splat_adam, init, seq, dev, **kw)[0]
    return net, splat, opt, params


# --------------------------------------------------------------------------------------------------- bitwise against SplatAdam

def test_sizes_around_the_vector_and_the_chunk_are_bitwise_splat_adams(hip_device):
    init, seq = inputs(SIZES_A, 3, seed=1)
    net, splat, opt, _ = both(init, seq, hip_device)
    assert_bitwise(net, splat, "sizes")
    assert all(a["step"] == 3.0 for a in net) and opt.plans_built == 1
    assert not torch.equal(net[5]["param"], init[5])


def test_more_tensors_than_one_launch_takes(hip_device):
    """SR_NET_ADAM_MAX_GRADS + 1 tensors of 1 to 5 elements: the second launch starts at a table index and a chunk above 0"""
    from splatfields_amd import _lib
    sizes = [1 + i % 5 for i in range(_lib.NET_ADAM_MAX_GRADS + 1)]
    init, seq = inputs(sizes, 3, seed=2)
    net, splat, opt, _ = both(init, seq, hip_device)
    assert_bitwise(net, splat, "many")
    assert len(opt._plan.ranges) == 2 and opt._plan.ranges[1][0] == _lib.NET_ADAM_MAX_GRADS and opt._plan.table[_lib.NET_ADAM_MAX_GRADS - 1].chunk_end > 0


def test_gradients_off_the_boundary_take_the_element_path(hip_device):
    """gradients that are views at 1, 2 and 3 floats past a 16-byte boundary, parameters on it"""
    init, seq = inputs(SIZES_A, 3, seed=3)
    net, splat, _, params = both(init, seq, hip_device, grad_place=lambda i, g: offset_view(g, 1 + i % 3))
    assert all(p.data_ptr() % 16 == 0 for p in params if p.numel() > 4)
    assert_bitwise(net, splat, "gradient views")


def test_parameters_off_the_boundary(hip_device):
    """parameters that are such views themselves (the chunking starts at the boundary below them; NetworkAdam's moments share the
    offset: vector path with an element-wise head and tail); nothing is written around the tensors"""
    init, seq = inputs(SIZES_A, 3, seed=4)
    net, splat, opt, params = both(init, seq, hip_device, place=lambda i, t: offset_view(t, 1 + i % 3))
    assert_bitwise(net, splat, "parameter views")
    for i, p in enumerate(params):
        shift = 1 + i % 3
        st = opt.state[p]
        assert st["exp_avg"].data_ptr() % 16 == p.data_ptr() % 16 == 4 * shift == st["exp_avg_sq"].data_ptr() % 16
        whole = torch.as_strided(p.detach(), (p.numel() + 8,), (1,), p.storage_offset() - shift)
        assert (whole[:shift] == 0).all() and (whole[shift + p.numel():] == 0).all()


def test_two_groups_with_their_own_scalars(hip_device):
    init, seq = inputs(SIZES_A, 3, seed=5)
    groups = [(range(0, 10, 2), dict(lr=1e-3, betas=(0.9, 0.999), eps=1e-15)), (range(1, 10, 2), dict(lr=3e-2, betas=(0.8, 0.99), eps=1e-8))]
    net, splat, opt, _ = both(init, seq, hip_device, groups=groups)
    assert_bitwise(net, splat, "two groups")
    one = drive(network_adam, init, seq, hip_device)[0]
    assert torch.equal(one[0]["param"], net[0]["param"]) and not torch.equal(one[1]["param"], net[1]["param"])


def test_new_learning_rates_need_no_new_plan(hip_device):
    init, seq = inputs(SIZES_A, 3, seed=6)
    schedule = [(1e-3 * f,) for f in (1.0, 0.1, 3.0)]
    net, splat, opt, _ = both(init, seq, hip_device, schedule=schedule)
    assert_bitwise(net, splat, "schedule")
    assert opt.plans_built == 1
    fixed = drive(network_adam, init, seq, hip_device)[0]
    assert not torch.equal(fixed[5]["param"], net[5]["param"])        # the schedule matters


def test_gradients_of_another_dtype_or_layout_are_converted_and_sparse_ones_refused(hip_device):
    """as SplatAdam: float64 and non-contiguous gradients give the bits of the plain ones, in every step (no new plan for them)"""
    dev = hip_device
    init, seq = inputs([(40, 6), (7,), (33, 5)], 3, seed=14)
    plain = drive(network_adam, init, seq, dev)[0]
    outs = {}
    for variant in ("float64", "transposed"):
        params = [nn.Parameter(t.to(dev)) for t in init]
        opt = network_adam([dict(params=params, lr=1e-3)], lr=0.0, eps=1e-15)
        for grads in seq:
            for p, g in zip(params, grads):
                if variant == "float64" and hasattr(p, "grad_dtype"):
                    p.grad_dtype = None                                 # newer torch: a gradient of another dtype has to be allowed
                p.grad = g.to(dev).double() if variant == "float64" else (g.t().contiguous().to(dev).t() if g.dim() == 2 else g.to(dev))
            assert variant != "transposed" or not params[0].grad.is_contiguous()
            opt.step()
        assert opt.plans_built == 1
        outs[variant] = A.snapshot(opt, params)
        assert_bitwise(outs[variant], plain, variant)
    p = nn.Parameter(init[0].to(dev))
    opt = network_adam([p], lr=1e-3)
    p.grad = seq[0][0].to(dev).to_sparse()
    with pytest.raises(RuntimeError, match="sparse"):
        opt.step()
    assert len(opt.state) == 0 or len(opt.state[p]) == 0


# -------------------------------------------------------------------------------------------------------------------- skipping

def test_a_tensor_without_a_gradient_is_untouched_and_steps_later_on_its_own_count(hip_device):
    dev = hip_device
    late = 4
    init, seq = inputs(SIZES_A[:9], 3, seed=7, skip=lambda s, i: s == 0 and i == late)
    first, opt, params = drive(network_adam, init, seq[:1], dev)
    assert first[late]["step"] is None and first[late]["exp_avg"] is None and len(opt.state[params[late]]) == 0
    assert torch.equal(first[late]["param"].view(torch.int32), init[late].view(torch.int32))
    assert all(a["step"] == 1.0 for i, a in enumerate(first) if i != late)
    net, splat, opt, _ = both(init, seq, dev)
    assert [a["step"] for a in net] == [2.0 if i == late else 3.0 for i in range(9)]      # one group, two step counts
    assert_bitwise(net, splat, "late tensor")


# --------------------------------------------------------------------------------------------------------------- against torch

def split_rule(tag, got, f64, f32):
    """per tensor and kind; the tensors of a handful of elements are pooled"""
    small = [i for i, t in enumerate(f64) if t["param"].numel() <= HANDFUL]
    large = [i for i, t in enumerate(f64) if t["param"].numel() > HANDFUL]
    pick = lambda rows, idx: [rows[i] for i in idx]
    if small:
        A.assert_within(tag + " (small, pooled)", pick(got, small), pick(f64, small), pick(f32, small), pooled=True)
    if large:
        A.assert_within(tag, pick(got, large), pick(f64, large), pick(f32, large))


def test_twelve_steps_against_torch_adam(hip_device):
    init, seq = inputs(SIZES_A, 12, seed=8)
    lrs = (1e-3,) * len(init)
    f64, f32 = A.cpu_pair(("net", "sizes", 12), init, lrs, 1e-15, seq)
    got = A.run(network_adam, init, lrs, 1e-15, seq, hip_device, torch.float32)[0]
    split_rule("network adam, sizes, 12 steps", got, f64, f32)


def test_a_small_real_network_against_torch_adam(hip_device):
    """SplatFields(n_frames=4, composition_rank=2), 64 points, one forward and backward per step, NetworkAdam stepping it: the
    gradients of the 12 steps are recorded and replayed to torch.optim.Adam in float64 and float32 from the same start."""
    from splatfields_amd.deform_field import SplatFields
    dev = hip_device
    torch.manual_seed(0)
    net = SplatFields(n_frames=4, composition_rank=2).to(dev)
    with torch.no_grad():
        net.encoder.planes.normal_(0.0, 0.3)
    params = list(net.parameters())
    init = [p.detach().cpu().clone() for p in params]
    opt = network_adam([{"params": params, "lr": 8e-4, "name": "deform"}], lr=0.0, eps=1e-15)
    gen = torch.Generator().manual_seed(1)
    seq = []
    for s in range(12):
        xyz = (torch.rand(64, 3, generator=gen) * 1.6 - 0.8).to(dev)
        out = net(xyz, torch.full((64, 1), (s % 4) / 3.0, device=dev))
        opt.zero_grad(set_to_none=True)
        sum(v.sum() for k, v in out.items() if torch.is_tensor(v) and k != "flow").backward()
        seq.append([None if p.grad is None else p.grad.detach().cpu().clone() for p in params])
        opt.step()
    assert len(params) == 137 and sum(g is not None for g in seq[0]) > 100
    got = A.snapshot(opt, params)
    lrs = (8e-4,) * len(init)
    f64 = A.run(torch.optim.Adam, init, lrs, 1e-15, seq, "cpu", torch.float64)[0]
    f32 = A.run(torch.optim.Adam, init, lrs, 1e-15, seq, "cpu", torch.float32)[0]
    split_rule("network adam, SplatFields 4 frames", got, f64, f32)


# ----------------------------------------------------------------------------------------------------------------- re-planning

def continued_splat_adam(opt, params, dev):
    """a fresh SplatAdam over copies of the parameters, continued from a copy of the optimizer's state (load_state_dict keeps the
    `step` tensors it is given: without the copy both optimizers would count on the same ones)"""
    twins = [nn.Parameter(p.detach().clone()) for p in params]
    splat = A.splat_adam([dict(params=twins, lr=1e-3)], lr=0.0, eps=1e-15)
    splat.load_state_dict(copy.deepcopy(opt.state_dict()))
    return splat, twins


def step_both(opt, params, other, twins, grads, dev):
    for p, q, g in zip(params, twins, grads):
        p.grad, q.grad = g.to(dev), g.to(dev)
    opt.step()
    other.step()
    return A.snapshot(opt, params), A.snapshot(other, twins)


def test_a_replaced_parameter_tensor_is_planned_again(hip_device):
    dev = hip_device
    init, seq = inputs(SIZES_A, 3, seed=9)
    _, opt, params = drive(network_adam, init, seq[:2], dev)
    splat, twins = continued_splat_adam(opt, params, dev)
    old = params[6].data_ptr()
    params[6].data = params[6].data.clone()
    assert params[6].data_ptr() != old and opt.plans_built == 1
    net, want = step_both(opt, params, splat, twins, seq[2], dev)
    assert opt.plans_built == 2 and all(a["step"] == 3.0 for a in net)
    assert_bitwise(net, want, "p.data replaced")


def test_a_loaded_torch_state_is_planned_again(hip_device):
    dev = hip_device
    init, seq = inputs(SIZES_A, 3, seed=10)
    _, ref, ref_params = drive(torch.optim.Adam, init, seq[:2], dev)
    params = [nn.Parameter(p.detach().clone()) for p in ref_params]
    opt = network_adam([dict(params=params, lr=1e-3)], lr=0.0, eps=1e-15)
    for p, g in zip(params, seq[0]):                                    # a plan of its own first: the load has to invalidate it
        p.grad = g.to(dev)
    opt.step()
    with torch.no_grad():
        for p, q in zip(params, ref_params):
            p.copy_(q)
    opt.load_state_dict(copy.deepcopy(ref.state_dict()))
    assert all(opt.state[p]["step"].device.type == "cpu" and float(opt.state[p]["step"]) == 2.0 for p in params)
    splat, twins = continued_splat_adam(opt, params, dev)
    built = opt.plans_built
    net, want = step_both(opt, params, splat, twins, seq[2], dev)
    assert opt.plans_built == built + 1
    assert_bitwise(net, want, "load_state_dict")


def test_the_state_goes_to_torch_adam(hip_device):
    """state_dict() -> torch.optim.Adam.load_state_dict -> one torch step, next to one NetworkAdam step from the same state:
    the two float32 steps differ by at most 4 x the deviation of torch's float32 run from its float64 run of the same case."""
    dev = hip_device
    init, seq = inputs(SIZES_A, 3, seed=11)
    lrs = (1e-3,) * len(init)
    f64, f32 = A.cpu_pair(("net", "to torch", 3), init, lrs, 1e-15, seq)
    _, opt, params = drive(network_adam, init, seq[:2], dev)
    twins = [nn.Parameter(p.detach().clone()) for p in params]
    ref = torch.optim.Adam([dict(params=twins, lr=1e-3)], lr=0.0, eps=1e-15)
    ref.load_state_dict(copy.deepcopy(opt.state_dict()))
    net, want = step_both(opt, params, ref, twins, seq[2], dev)
    assert all(a["step"] == b["step"] == 3.0 for a, b in zip(net, want))
    small = [i for i, t in enumerate(init) if t.numel() <= HANDFUL]
    for kind in KINDS:
        dev_ = [(a[kind].double() - b[kind].double()).abs().max().item() for a, b in zip(net, want)]
        yard = [(y[kind].double() - t[kind]).abs().max().item() for y, t in zip(f32, f64)]
        pooled_dev, pooled_yard = max(dev_[i] for i in small), max(yard[i] for i in small)
        for i in range(len(init)):
            d, y = (pooled_dev, pooled_yard) if i in small else (dev_[i], yard[i])
            print(f"[network adam] to torch, tensor {i} {kind}: against torch float32 {d:.3e}, float32 against float64 {y:.3e} (allowed 4 x)")
            assert d <= 4.0 * y, (i, kind, d, y)


# --------------------------------------------------------------------------------------------------------------- launch budget

def check_budget(params, dev, tag):
    from splatfields_amd import _lib
    gen = torch.Generator().manual_seed(12)
    opt = network_adam([{"params": params, "lr": 8e-4, "name": "deform"}], lr=0.0, eps=1e-15)
    for p in params:
        p.grad = A.gradients(tuple(p.shape) or (1,), "uniform", gen).reshape(p.shape).to(dev)
    opt.step()                                                          # plans, creates the state
    opt.step()
    names = device_records(opt.step, drop_host_ranges=True)
    want = math.ceil(len(params) / _lib.NET_ADAM_MAX_GRADS)
    print(f"[network adam] {tag}: {len(params)} tensors, device records of a step: {names}")
    assert len(names) > 0, "the profiler recorded nothing: the budget was not checked"
    assert len(names) == want and all("k_net_adam" in n for n in names), (tag, want, names)
    assert opt.plans_built == 1


def test_launch_budget_of_the_4d_network(hip_device):
    from splatfields_amd.deform_field import SplatFields
    net = SplatFields(n_frames=4, composition_rank=2, encoder_args={"noise_res": 1}).to(hip_device)
    params = list(net.parameters())
    assert len(params) == 137
    check_budget(params, hip_device, "4-D network at reduced sizes")


def test_launch_budget_beyond_one_launch(hip_device):
    from splatfields_amd import _lib
    gen = torch.Generator().manual_seed(13)
    params = [nn.Parameter(torch.randn(1 + i % 5, generator=gen).to(hip_device)) for i in range(_lib.NET_ADAM_MAX_GRADS + 1)]
    check_budget(params, hip_device, "SR_NET_ADAM_MAX_GRADS + 1 tensors")


# ------------------------------------------------------------------------------------------------- run to run, and the default

def test_run_to_run_bit_identical(hip_device):
    init, seq = inputs(SIZES_A, 3, seed=1)
    first = drive(network_adam, init, seq, hip_device)[0]
    again = drive(network_adam, init, seq, hip_device)[0]
    assert_bitwise(first, again, "run to run")


def small_model(dev, seed=0):
    from splatfields_amd.deform_field import SplatFieldsModel
    torch.manual_seed(seed)
    hyper = types.SimpleNamespace(n_frames=4, composition_rank=2, encoder_args={"noise_res": 1})
    return SplatFieldsModel(hyper, radius=None, device=dev)


TRAIN = types.SimpleNamespace(position_lr_init=0.00016, position_lr_final=0.0000016, position_lr_delay_mult=0.01, deform_lr_max_steps=40000)


def training_step(model, dev):
    gen = torch.Generator().manual_seed(3)
    xyz = (torch.rand(64, 3, generator=gen) * 1.6 - 0.8).to(dev)
    model.update_learning_rate(100)
    model.optimizer.zero_grad(set_to_none=True)
    out = model.step(xyz, torch.full((64, 1), 1.0 / 3.0, device=dev))
    sum(v.sum() for k, v in out.items() if torch.is_tensor(v) and k != "flow").backward()
    model.optimizer.step()
    return [p.detach().clone() for p in model.deform.parameters()]


def test_the_default_is_torch_adam_and_the_switches_choose(hip_device, monkeypatch):
    import splatfields_amd
    from splatfields_amd import NetworkAdam, network_optim
    dev = hip_device
    monkeypatch.setattr(network_optim, "_NETWORK_OPTIMIZER", "torch")
    runs = {}
    for name, kw in (("default", {}), ("torch", dict(optimizer="torch")), ("fused", dict(optimizer="fused"))):
        model = small_model(dev)
        model.train_setting(TRAIN, **kw)
        assert type(model.optimizer) is (NetworkAdam if name == "fused" else torch.optim.Adam)
        group = model.optimizer.param_groups[0]
        assert group["name"] == "deform" and group["eps"] == 1e-15 and group["lr"] == TRAIN.position_lr_init * 5
        runs[name] = training_step(model, dev)
        assert model.optimizer.param_groups[0]["lr"] == model.update_learning_rate(100) != TRAIN.position_lr_init * 5
    start = [p.detach().clone() for p in small_model(dev).deform.parameters()]
    assert all(torch.equal(a, b) for a, b in zip(runs["default"], runs["torch"]))
    assert any(not torch.equal(a, s) for a, s in zip(runs["default"], start)) and any(not torch.equal(a, s) for a, s in zip(runs["fused"], start))
    # the process default and the argument
    model = small_model(dev)
    assert splatfields_amd.set_network_optimizer("fused") == "torch" and splatfields_amd.network_optimizer() == "fused"
    model.train_setting(TRAIN)
    assert type(model.optimizer) is NetworkAdam
    model.train_setting(TRAIN, optimizer="torch")
    assert type(model.optimizer) is torch.optim.Adam
    assert splatfields_amd.set_network_optimizer("torch") == "fused"
    model.train_setting(TRAIN, optimizer="fused")
    assert type(model.optimizer) is NetworkAdam
    model.train_setting(TRAIN)
    assert type(model.optimizer) is torch.optim.Adam
