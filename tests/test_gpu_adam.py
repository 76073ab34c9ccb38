"""The fused Adam step (splatfields_amd/optim.py -> sr_adam_step, csrc/adam.hip) on the MI355X against torch.optim.Adam itself,
which is what the reference steps (scene/gaussian_model.py:130-139, train.py:314-322).

Truth: torch.optim.Adam in float64 on the CPU.  Yardstick: torch.optim.Adam in float32 on the CPU, same float32 inputs and the
same gradient sequence.  Allowance: per tensor and per kind (parameter, exp_avg, exp_avg_sq) the kernel may deviate from the
truth by 4 x the max-abs deviation of the yardstick from the truth -- the kernel is another float32 evaluation of the same
formulas in another operation order (fused multiply-adds where torch rounds twice).  Where a launch is made of tensors of a
handful of elements (the vector-path edges, the 70-tensor list) one tensor's max-abs deviation is a draw of one to a few
roundings and can be exactly 0 for the yardstick by luck; those tensors share one learning rate and one gradient scale, so
their roundings are draws from one distribution and the maximum is taken over the launch's tensors of a kind (`pooled`).
Every case prints its ratio deviation / yardstick.  Bitwise statements (rows that never had a gradient, hidden rows, run to
run) are compared with torch.equal."""
import functools
import types

import pytest
import torch
from torch import nn

pytestmark = pytest.mark.gpu

KINDS = ("param", "exp_avg", "exp_avg_sq")
SIX_SHAPES = ((3,), (1, 3), (15, 3), (1,), (3,), (4,))                 # xyz, f_dc, f_rest, opacity, scaling, rotation
SIX_NAMES = ("xyz", "f_dc", "f_rest", "opacity", "scaling", "rotation")
SIX_LRS = (8e-4, 2.5e-3, 2.5e-3 / 20, 5e-2, 5e-3, 1e-3)                 # the reference's, spatial_lr_scale 5
N_SIX = 4099


# ---------------------------------------------------------------------------------------------------------------- inputs

def gradients(shape, family, gen):
    """One gradient of `shape` ([rows, ...]), every element sign x U(0.5, 1) x the magnitude of its row: 'uniform' 1e-3 for every
    row (the max-abs norm sees every row), 'lognormal' 1e-4 exp(min(2 z, 2)) with z ~ N(0, 1) per row -- magnitudes over four
    decades.  The max-abs deviation of a tensor is decided by the elements in its top binade, and a ratio of two such maxima
    means something only if many elements compete for it: an unclipped log-normal leaves the top binade to one row (three
    elements of xyz, one of opacity), where 4 x "the rounding torch happened to draw there" is a coin toss, not a bound.  The
    clip puts the 16 % of the rows with z > 1 at the top magnitude; the other rows reach down to 1e-4 exp(-8)."""
    sign = torch.sign(torch.randn(shape, generator=gen))
    level = 0.5 + 0.5 * torch.rand(shape, generator=gen)
    if family == "uniform":
        return sign * level * 1e-3
    z = torch.randn((shape[0],) + (1,) * (len(shape) - 1), generator=gen)
    return sign * level * 1e-4 * torch.exp(torch.clamp(2.0 * z, max=2.0))


@functools.lru_cache(maxsize=None)
def six_group_inputs(family, steps, n=N_SIX, seed=5):
    gen = torch.Generator().manual_seed(seed + steps)
    init = [torch.randn((n,) + s, generator=gen) for s in SIX_SHAPES]
    live = torch.rand(n, generator=gen) >= 0.4                         # 40 % of the rows never get a gradient
    seq = []
    for _ in range(steps):
        seq.append([gradients((n,) + s, family, gen) * live.reshape((n,) + (1,) * len(s)) for s in SIX_SHAPES])
    return init, seq, live


# ------------------------------------------------------------------------------------------------------------ the runners

def snapshot(opt, params):
    out = []
    for p in params:
        st = opt.state.get(p, {})
        out.append({"param": p.detach().cpu().clone(), "exp_avg": st["exp_avg"].detach().cpu().clone() if st else None,
                    "exp_avg_sq": st["exp_avg_sq"].detach().cpu().clone() if st else None,
                    "step": float(st["step"]) if st else None})
    return out


def masked_torch_step(opt, params, grads, mask):
    """The restatement of step(visible=mask): torch.optim.Adam on the gathered rows with the global step count, scattered back."""
    idx = mask.nonzero().flatten()
    for group, p, g in zip(opt.param_groups, params, grads):
        st = opt.state[p]
        if len(st) == 0:
            st["step"], st["exp_avg"], st["exp_avg_sq"] = torch.tensor(0.0), torch.zeros_like(p), torch.zeros_like(p)
        sub = nn.Parameter(p.detach()[idx].clone())
        sub.grad = g.to(p.dtype)[idx].clone()
        inner = torch.optim.Adam([sub], lr=group["lr"], betas=group["betas"], eps=group["eps"])
        inner.state[sub] = {"step": st["step"].clone(), "exp_avg": st["exp_avg"][idx].clone(), "exp_avg_sq": st["exp_avg_sq"][idx].clone()}
        inner.step()
        with torch.no_grad():
            p[idx] = sub.detach()
            st["exp_avg"][idx] = inner.state[sub]["exp_avg"]
            st["exp_avg_sq"][idx] = inner.state[sub]["exp_avg_sq"]
        st["step"] += 1


def run(make, init, lrs, eps, seq, device, dtype, masks=None, schedule=None, place=None):
    """`make(groups, lr=0.0, eps=eps)` builds the optimizer over parameters cloned from `init`; seq[s][i] is the gradient of
    tensor i in step s (None: no gradient); masks[s]: the row mask of step s; schedule[s]: the learning rates written into the
    groups before step s; place(i, tensor) -> a tensor of the same values where the caller wants it in memory."""
    place = place or (lambda i, t: t.clone())
    params = [nn.Parameter(place(i, t.to(device=device, dtype=dtype))) for i, t in enumerate(init)]
    opt = make([{"params": [p], "lr": lr, "name": f"t{i}"} for i, (p, lr) in enumerate(zip(params, lrs))], lr=0.0, eps=eps)
    hip = type(opt).__name__ == "SplatAdam"
    for s, grads in enumerate(seq):
        if schedule is not None:
            for group, lr in zip(opt.param_groups, schedule[s]):
                group["lr"] = lr
        for p, g in zip(params, grads):
            p.grad = None if g is None else g.to(device=device, dtype=dtype)
        if masks is None:
            opt.step()
        elif hip:
            opt.step(visible=masks[s].to(device))
        else:
            masked_torch_step(opt, params, grads, masks[s])
    return snapshot(opt, params), opt, params


def splat_adam(*a, **k):
    from splatfields_amd import SplatAdam
    return SplatAdam(*a, **k)


@functools.lru_cache(maxsize=None)
def _cpu_pair_cached(key):
    init, lrs, eps, seq, masks, schedule = _CASES[key]
    f64 = run(torch.optim.Adam, init, lrs, eps, seq, "cpu", torch.float64, masks, schedule)[0]
    f32 = run(torch.optim.Adam, init, lrs, eps, seq, "cpu", torch.float32, masks, schedule)[0]
    return f64, f32


_CASES = {}


def cpu_pair(key, init, lrs, eps, seq, masks=None, schedule=None):
    """(float64 truth, float32 yardstick) of a case, computed once per session and shared"""
    _CASES.setdefault(key, (init, lrs, eps, seq, masks, schedule))
    return _cpu_pair_cached(key)


def assert_within(tag, got, f64, f32, pooled=False):
    worst = 0.0
    for kind in KINDS:
        rows = []
        for i, (a, t, y) in enumerate(zip(got, f64, f32)):
            if t[kind] is None:
                assert a[kind] is None, (tag, i, kind)
                continue
            assert a[kind] is not None and a[kind].shape == t[kind].shape, (tag, i, kind)
            if t[kind].numel() == 0:
                continue
            rows.append((i, (a[kind].double() - t[kind]).abs().max().item(), (y[kind].double() - t[kind]).abs().max().item()))
        if pooled:
            rows = [("all", max(r[1] for r in rows), max(r[2] for r in rows))]
        for i, dev, yard in rows:
            ratio = dev / yard if yard > 0 else (0.0 if dev == 0 else float("inf"))
            worst = max(worst, ratio)
            print(f"[adam] {tag} tensor {i} {kind}: deviation {dev:.3e}, torch float32 {yard:.3e}, ratio {ratio:.2f} (allowed 4)")
            assert dev <= 4.0 * yard, (tag, i, kind, dev, yard)
    print(f"[adam] {tag}: worst ratio {worst:.2f}")
    for a, t in zip(got, f64):
        assert a["step"] == t["step"], (tag, a["step"], t["step"])


# ------------------------------------------------------------------------------------------------------------------ values

@pytest.mark.parametrize("eps", [1e-15, 1e-8])
@pytest.mark.parametrize("family", ["uniform", "lognormal"])
@pytest.mark.parametrize("steps", [1, 12])
def test_six_groups_against_torch_adam(hip_device, steps, family, eps):
    init, seq, live = six_group_inputs(family, steps)
    f64, f32 = cpu_pair(("six", family, steps, eps), init, SIX_LRS, eps, seq)
    got, opt, params = run(splat_adam, init, SIX_LRS, eps, seq, hip_device, torch.float32)
    assert_within(f"six groups {family} {steps} steps eps {eps}", got, f64, f32)
    # a row whose gradient was zero in every step: the parameter keeps its bits, both moments are exactly 0
    dead = ~live
    assert dead.sum() > 1000
    for a, start in zip(got, init):
        assert torch.equal(a["param"][dead].view(torch.int32), start[dead].view(torch.int32))
        assert (a["exp_avg"][dead].view(torch.int32) == 0).all() and (a["exp_avg_sq"][dead].view(torch.int32) == 0).all()
        assert not torch.equal(a["param"][live], start[live])
    for group, p in zip(opt.param_groups, params):                     # the layout torch.optim.Adam has
        st = opt.state[p]
        assert sorted(st) == ["exp_avg", "exp_avg_sq", "step"] and st["step"].device.type == "cpu" and st["step"].dtype == torch.float32
        assert st["exp_avg"].shape == p.shape and st["exp_avg"].device == p.device and group["params"] == [p]


def test_more_chunks_than_workgroups(hip_device):
    """8.9 M elements in one tensor: more chunks of 2048 (or 4096) elements than a grid of 8 workgroups on each of 256 CUs has
    workgroups -- the grid-stride loop --, next to a small tensor."""
    gen = torch.Generator().manual_seed(11)
    n = 2048 * 4096 + 512 * 1024 + 1027
    init = [torch.randn(n, generator=gen), torch.randn(77, 3, generator=gen)]
    seq = [[gradients((n,), "uniform", gen), gradients((77, 3), "uniform", gen)]]
    f64, f32 = cpu_pair("large", init, (1e-3, 1e-3), 1e-15, seq)
    got = run(splat_adam, init, (1e-3, 1e-3), 1e-15, seq, hip_device, torch.float32)[0]
    assert_within("8.9 M elements", got, f64, f32)


# ------------------------------------------------------------------------------------------- the edges of the vector path

EDGE_COUNTS = (1, 3, 4, 5, 1023, 1025)


def edge_inputs():
    gen = torch.Generator().manual_seed(3)
    init = [torch.randn(c, generator=gen) for c in EDGE_COUNTS] + [torch.randn(0, 3)] + [torch.randn(c, generator=gen) for c in EDGE_COUNTS]
    seq = [[gradients(tuple(t.shape), "uniform", gen) if t.numel() else torch.zeros(0, 3) for t in init] for _ in range(2)]
    return init, seq


@pytest.mark.parametrize("offset", [0, 1, 2, 3, "mixed"])
def test_small_and_misaligned_tensors_in_one_launch(hip_device, offset):
    """Element counts around the vector width and the workgroup's slot count, twice each and with a zero-row tensor among
    them, in ONE launch (13 jobs: job boundaries fall inside a workgroup's chunk); storage that starts 4, 8 or 12 bytes past
    a 16-byte boundary for all four tensors of a job (vector body, element-wise head and tail) or for the parameter alone
    ('mixed': no vector path for that job)."""
    dev = hip_device
    init, seq = edge_inputs()
    lrs = (1e-3,) * len(init)
    f64, f32 = cpu_pair("edges", init, lrs, 1e-15, seq)
    shift = 1 if offset == "mixed" else offset

    def place(i, t):
        if shift == 0 or t.numel() == 0:
            return t.clone()
        buf = torch.zeros(t.numel() + 4, device=t.device, dtype=t.dtype)
        buf[shift:shift + t.numel()] = t.reshape(-1)
        out = buf[shift:shift + t.numel()].reshape(t.shape)
        assert out.data_ptr() % 16 == 4 * shift and out.is_contiguous()
        return out

    params = [nn.Parameter(place(i, t.to(dev))) for i, t in enumerate(init)]
    opt = splat_adam([{"params": [p], "lr": lr} for p, lr in zip(params, lrs)], lr=0.0, eps=1e-15)
    if offset != "mixed":     # the moments share the parameter's offset: torch's layout, placed by hand
        for i, p in enumerate(params):
            opt.state[p] = {"step": torch.tensor(0.0), "exp_avg": place(i, torch.zeros_like(p)), "exp_avg_sq": place(i, torch.zeros_like(p))}
    for grads in seq:
        for i, (p, g) in enumerate(zip(params, grads)):
            p.grad = place(i, g.to(dev)) if offset != "mixed" else g.to(dev)
        opt.step()
    got = snapshot(opt, params)
    assert_within(f"edges offset {offset}", got, f64, f32, pooled=True)
    assert got[len(EDGE_COUNTS)]["step"] == 2.0 and got[len(EDGE_COUNTS)]["param"].shape == (0, 3)
    if shift:   # nothing was written outside the tensors: the floats around them are still 0
        for p in params:
            placed = [p.detach()] + ([opt.state[p]["exp_avg"], opt.state[p]["exp_avg_sq"]] if offset != "mixed" else [])
            for t in placed if p.numel() else ():
                whole = torch.as_strided(t, (t.numel() + 4,), (1,), t.storage_offset() - shift)
                assert (whole[:shift] == 0).all() and (whole[shift + t.numel():] == 0).all()


def test_more_tensors_than_one_launch_takes(hip_device):
    """70 tensors of mixed sizes: three launches; every tensor is updated once and only once."""
    from splatfields_amd import _lib
    sizes = [(1,), (2,), (3,), (4,), (5,), (7, 3), (8,), (31,), (64,), (100, 3), (257,), (1023,), (1025,), (2049,), (4097,), (16, 16),
             (3, 5, 7)]
    assert 70 > 2 * _lib.ADAM_MAX_TENSORS
    gen = torch.Generator().manual_seed(70)
    init = [torch.randn(sizes[i % len(sizes)], generator=gen) for i in range(70)]
    seq = [[gradients(tuple(t.shape), "uniform", gen) for t in init]]
    lrs = (2e-3,) * 70
    f64, f32 = cpu_pair("seventy", init, lrs, 1e-8, seq)
    got = run(splat_adam, init, lrs, 1e-8, seq, hip_device, torch.float32)[0]
    assert_within("70 tensors", got, f64, f32, pooled=True)
    assert all(a["step"] == 1.0 for a in got)      # and a tensor stepped twice or not at all is off by lr = 2e-3, no rounding


def test_a_parameter_without_a_gradient_is_untouched_and_gets_no_state(hip_device):
    gen = torch.Generator().manual_seed(8)
    init = [torch.randn(33, 3, generator=gen), torch.randn(65, 4, generator=gen), torch.randn(9, generator=gen)]
    seq = [[gradients((33, 3), "uniform", gen), None, gradients((9,), "uniform", gen)] for _ in range(2)]
    lrs = (1e-3, 1e-3, 1e-3)
    f64, f32 = cpu_pair("no grad", init, lrs, 1e-15, seq)
    got, opt, params = run(splat_adam, init, lrs, 1e-15, seq, hip_device, torch.float32)
    assert_within("grad is None", got, f64, f32)
    assert got[1]["exp_avg"] is None and got[1]["step"] is None and len(opt.state[params[1]]) == 0
    assert torch.equal(got[1]["param"].view(torch.int32), init[1].view(torch.int32))


# -------------------------------------------------------------------------------------------------------------------- mask

def mask_inputs(steps=3, n=1031):
    gen = torch.Generator().manual_seed(17)
    shapes = [(n,) + s for s in SIX_SHAPES]
    init = [torch.randn(s, generator=gen) for s in shapes]
    seq = [[gradients(s, "uniform", gen) for s in shapes] for _ in range(steps)]
    masks = [torch.rand(n, generator=gen) < f for f in (0.5, 0.1, 0.9)][:steps]
    return init, seq, masks


def test_hidden_rows_keep_their_bits_and_visible_rows_equal_the_dense_step(hip_device):
    dev = hip_device
    init, seq, masks = mask_inputs()
    before = run(splat_adam, init, SIX_LRS, 1e-15, seq[:1], dev, torch.float32)[0]
    dense = run(splat_adam, init, SIX_LRS, 1e-15, seq[:2], dev, torch.float32)[0]
    for mask in (masks[0], masks[1], torch.zeros_like(masks[0]), torch.ones_like(masks[0])):
        for as_bytes in (False, True):
            given = mask.to(torch.uint8) * 7 if as_bytes else mask            # any non-zero byte counts as visible
            got = run(splat_adam, init, SIX_LRS, 1e-15, seq[:2], dev, torch.float32,
                      masks=[torch.ones_like(mask), given])[0]
            for a, b, d in zip(got, before, dense):
                for kind in KINDS:
                    assert torch.equal(a[kind][~mask].view(torch.int32), b[kind][~mask].view(torch.int32)), kind
                    assert torch.equal(a[kind][mask].view(torch.int32), d[kind][mask].view(torch.int32)), kind
                assert a["step"] == 2.0


def test_masked_steps_against_the_torch_restatement(hip_device):
    """Three steps, another mask each: torch.optim.Adam on the gathered rows, scattered back, with the global step count."""
    init, seq, masks = mask_inputs()
    f64, f32 = cpu_pair("masked", init, SIX_LRS, 1e-15, seq, tuple(masks))
    got = run(splat_adam, init, SIX_LRS, 1e-15, seq, hip_device, torch.float32, masks=masks)[0]
    assert_within("three masked steps", got, f64, f32)


def test_a_mask_needs_tensors_of_its_row_count(hip_device):
    dev = hip_device
    a, b = nn.Parameter(torch.zeros(10, 3, device=dev)), nn.Parameter(torch.zeros(12, 3, device=dev))
    opt = splat_adam([a, b], lr=1e-3)
    a.grad, b.grad = torch.ones_like(a), torch.ones_like(b)
    with pytest.raises(ValueError, match="visible has 10 rows"):
        opt.step(visible=torch.ones(10, dtype=torch.bool, device=dev))
    with pytest.raises(ValueError, match="bool or uint8"):
        opt.step(visible=torch.ones(10, device=dev))
    with pytest.raises(ValueError, match="no CPU path"):
        opt.step(visible=torch.ones(10, dtype=torch.bool))
    b.grad = None                                                      # without a gradient the other tensor does not take part
    opt.step(visible=torch.ones(10, dtype=torch.bool, device=dev))
    assert float(opt.state[a]["step"]) == 1.0 and len(opt.state[b]) == 0


# ------------------------------------------------------------------------------------------- run to run, schedule, inputs

def test_run_to_run_bit_identical(hip_device):
    init, seq, masks = mask_inputs()
    for kw in ({}, {"masks": masks}):
        first = run(splat_adam, init, SIX_LRS, 1e-15, seq, hip_device, torch.float32, **kw)[0]
        again = run(splat_adam, init, SIX_LRS, 1e-15, seq, hip_device, torch.float32, **kw)[0]
        for a, b in zip(first, again):
            assert all(torch.equal(a[k].view(torch.int32), b[k].view(torch.int32)) for k in KINDS)


def test_a_new_learning_rate_takes_effect_in_the_next_step(hip_device):
    """`update_learning_rate` writes group['lr'] (reference scene/gaussian_model.py:148-154); the next step reads it."""
    init, seq, _ = mask_inputs()
    schedule = [tuple(lr * f for lr in SIX_LRS) for f in (1.0, 0.1, 3.0)]
    f64, f32 = cpu_pair("schedule", init, SIX_LRS, 1e-15, seq, None, tuple(schedule))
    got = run(splat_adam, init, SIX_LRS, 1e-15, seq, hip_device, torch.float32, schedule=schedule)[0]
    assert_within("learning-rate schedule", got, f64, f32)
    fixed = cpu_pair("fixed rates", init, SIX_LRS, 1e-15, seq)[0]
    assert (fixed[0]["param"] - f64[0]["param"]).abs().max() > 1e-4    # the schedule matters at this size


def test_gradients_are_converted_and_sparse_ones_refused(hip_device):
    dev = hip_device
    gen = torch.Generator().manual_seed(2)
    w0 = torch.randn(40, 6, generator=gen)
    g = gradients((40, 6), "uniform", gen)
    outs = []
    for variant in ("plain", "float64", "transposed"):
        p = nn.Parameter(w0.to(dev))
        opt = splat_adam([p], lr=1e-3, eps=1e-15)
        if variant == "float64" and hasattr(p, "grad_dtype"):
            p.grad_dtype = None                                         # newer torch: a gradient of another dtype has to be allowed
        p.grad = {"plain": g.to(dev), "float64": g.to(dev).double(), "transposed": g.t().contiguous().to(dev).t()}[variant]
        assert variant != "transposed" or not p.grad.is_contiguous()
        opt.step()
        outs.append(p.detach().cpu())
    assert torch.equal(outs[0], outs[1]) and torch.equal(outs[0], outs[2]) and not torch.equal(outs[0], w0)
    p = nn.Parameter(w0.to(dev))
    opt = splat_adam([p], lr=1e-3)
    p.grad = g.to(dev).to_sparse()
    with pytest.raises(RuntimeError, match="sparse"):
        opt.step()
    with pytest.raises(ValueError, match="float32"):
        splat_adam([nn.Parameter(w0.double().to(dev))], lr=1e-3)
    with pytest.raises(ValueError, match="contiguous"):
        splat_adam([nn.Parameter(w0.to(dev).t())], lr=1e-3)
    with pytest.raises(ValueError, match="no CPU path"):
        splat_adam([nn.Parameter(w0.clone())], lr=1e-3)


# ------------------------------------------------------------------------------------------------------- state interchange

@pytest.mark.parametrize("first", ["torch", "splat"])
def test_state_dict_goes_to_and_from_torch_adam(hip_device, first):
    dev = hip_device
    init, seq6, _ = six_group_inputs("uniform", 6, n=517, seed=40)
    f64, f32 = cpu_pair("interchange", init, SIX_LRS, 1e-15, seq6)
    makers = {"torch": torch.optim.Adam, "splat": splat_adam}
    second = "splat" if first == "torch" else "torch"
    _, opt_a, params = run(makers[first], init, SIX_LRS, 1e-15, seq6[:3], dev, torch.float32)
    saved = opt_a.state_dict()
    opt_b = makers[second]([{"params": [p], "lr": lr, "name": f"t{i}"} for i, (p, lr) in enumerate(zip(params, SIX_LRS))], lr=0.0, eps=1e-15)
    opt_b.load_state_dict(saved)
    assert [g["lr"] for g in opt_b.param_groups] == list(SIX_LRS) and all(g["eps"] == 1e-15 for g in opt_b.param_groups)
    for grads in seq6[3:]:
        for p, g in zip(params, grads):
            p.grad = g.to(dev)
        opt_b.step()
    got = snapshot(opt_b, params)
    assert_within(f"3 steps {first}, 3 steps {second}", got, f64, f32)
    assert all(a["step"] == 6.0 for a in got)
    assert all(opt_b.state[p]["step"].device.type == "cpu" for p in params)


# ----------------------------------------------------------------------------------------------------------- densification

ATTR = {"xyz": "_xyz", "f_dc": "_features_dc", "f_rest": "_features_rest", "opacity": "_opacity", "scaling": "_scaling",
        "rotation": "_rotation"}


def densify_inputs(n=300):
    gen = torch.Generator().manual_seed(300)
    r = lambda *s: torch.randn(*s, generator=gen)
    import math
    start = {"xyz": r(n, 3), "f_dc": r(n, 1, 3), "f_rest": r(n, 15, 3) * 0.1, "opacity": r(n, 1) * 2.5,
             "scaling": math.log(0.03) + 1.2 * r(n, 3), "rotation": r(n, 4)}
    denom = torch.randint(0, 6, (n, 1), generator=gen).float()
    accum = torch.rand(n, 1, generator=gen) * 0.01
    accum[denom == 0] = 0.0
    unit = torch.randn(2, n, 3, generator=gen)
    grads = lambda rows: {k: gradients((rows,) + tuple(v.shape[1:]), "uniform", gen) for k, v in start.items()}
    return start, accum, denom, unit, grads(n), grads


def test_step_densify_step_like_torch_adam(hip_device):
    """Step, densify_and_prune, step -- once on SplatAdam and once on torch.optim.Adam: the same rows, the same `step`, new rows'
    moments start at zero, and the values of the two float32 runs differ by at most 4 x the deviation of torch's float32 step
    from its float64 step before the densification (the rebuilt rows have no float64 counterpart: the plan is float32)."""
    from splatfields_amd.densify import densify_and_prune
    dev = hip_device
    start, accum, denom, unit, g1, more = densify_inputs()
    lrs = dict(zip(SIX_NAMES, SIX_LRS))
    init = [start[k] for k in SIX_NAMES]
    f64, f32 = cpu_pair("densify first step", init, SIX_LRS, 1e-15, [[g1[k] for k in SIX_NAMES]])
    yard = {k: {kind: (f32[i][kind].double() - f64[i][kind]).abs().max().item() for kind in KINDS} for i, k in enumerate(SIX_NAMES)}
    g2 = None
    runs = {}
    for name, make in (("splat", splat_adam), ("torch", torch.optim.Adam)):
        h = types.SimpleNamespace(percent_dense=0.01)
        groups = []
        for k in SIX_NAMES:
            p = nn.Parameter(start[k].clone().to(dev))
            setattr(h, ATTR[k], p)
            groups.append({"params": [p], "lr": lrs[k], "name": k})
        h.optimizer = make(groups, lr=0.0, eps=1e-15)
        h.xyz_gradient_accum, h.denom, h.max_radii2D = accum.clone().to(dev), denom.clone().to(dev), torch.zeros(300, device=dev)
        for k in SIX_NAMES:
            getattr(h, ATTR[k]).grad = g1[k].to(dev)
        h.optimizer.step()
        counts = densify_and_prune(h, 0.0035, 0.1, 4.0, None, unit_normals=unit.to(dev))
        assert counts["clones"] > 0 and counts["children"] > 0 and counts["kept"] < 300
        new_rows = counts["total"] - counts["kept"]
        for k in SIX_NAMES:
            p = getattr(h, ATTR[k])
            st = h.optimizer.state[p]
            assert p.shape[0] == counts["total"] and st["exp_avg"].shape == p.shape and float(st["step"]) == 1.0
            assert not st["exp_avg"][counts["kept"]:].any() and not st["exp_avg_sq"][counts["kept"]:].any() and new_rows > 0
        if g2 is None:
            g2 = more(counts["total"])
        assert g2["xyz"].shape[0] == counts["total"]                       # both runs plan the same rows
        for k in SIX_NAMES:
            getattr(h, ATTR[k]).grad = g2[k].to(dev)
        h.optimizer.step()
        runs[name] = (counts, {k: snapshot(h.optimizer, [getattr(h, ATTR[k])])[0] for k in SIX_NAMES})
    assert runs["splat"][0] == runs["torch"][0]
    for k in SIX_NAMES:
        a, b = runs["splat"][1][k], runs["torch"][1][k]
        assert a["step"] == b["step"] == 2.0
        for kind in KINDS:
            dev_ = (a[kind].double() - b[kind].double()).abs().max().item()
            print(f"[adam] densify {k} {kind}: SplatAdam against torch float32 {dev_:.3e}, float32 against float64 before {yard[k][kind]:.3e}, "
                  f"ratio {dev_ / yard[k][kind]:.2f} (allowed 4)")
            assert dev_ <= 4.0 * yard[k][kind], (k, kind, dev_, yard[k][kind])


# ------------------------------------------------------------------------------------------------------------ no host wait

def test_no_host_wait_from_the_python_side(hip_device):
    dev = hip_device
    init, seq, masks = mask_inputs()
    params = [nn.Parameter(t.to(dev)) for t in init]
    opt = splat_adam([{"params": [p], "lr": lr} for p, lr in zip(params, SIX_LRS)], lr=0.0, eps=1e-15)
    late = nn.Parameter(torch.randn(50, 3).to(dev))                     # its state is created inside the checked region
    opt.add_param_group({"params": [late], "lr": 1e-3})
    grads = [[g.to(dev) for g in step] for step in seq]
    late_grad, mask = torch.ones_like(late), masks[0].to(dev)
    for p, g in zip(params, grads[0]):
        p.grad = g
    opt.step()                                                          # warm up: library load, allocator
    torch.cuda.synchronize()
    try:
        torch.cuda.set_sync_debug_mode("error")
    except Exception as e:   # noqa: BLE001
        pytest.skip(f"this torch build does not implement set_sync_debug_mode: {e}")
    try:
        for p, g in zip(params, grads[1]):
            p.grad = g
        late.grad = late_grad
        opt.step()
        late.grad = None
        opt.step(visible=mask)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    torch.cuda.synchronize()
    assert all(torch.isfinite(p).all() for p in params) and float(opt.state[params[0]]["step"]) == 3.0
    assert float(opt.state[late]["step"]) == 1.0


# -------------------------------------------------------------------------------------------------------------- end to end

def test_fitting_a_target_view_reduces_the_loss(hip_device):
    """The fitting loop of tests/test_gpu_training_smoke.py with SplatAdam in place of torch.optim.Adam; the same criterion."""
    from splatfields_amd import SplatAdam
    from splatfields_amd.render import render
    from splatfields_amd.synthetic import make_camera, make_splats
    dev = hip_device
    torch.manual_seed(0)
    n, W, H = 4000, 160, 128
    target_sp = make_splats(n, seed=21, mean_scale=0.05, device=dev)
    pipe = types.SimpleNamespace(debug=False)
    bg = torch.ones(3, device=dev)
    cams = [make_camera(k, W, H, device=dev) for k in (0, 2, 5)]

    def pack(sp, deg=1):
        return {"means3D": sp["means3D"], "active_sh_degree": deg, "gaussian_opacity": sp["opacities"],
                "gaussian_features": sp["shs"], "gaussian_scales": sp["scales"], "gaussian_rotations": sp["rotations"]}

    with torch.no_grad():
        targets = [(render(c, pack(target_sp), pipe, bg)["render"], render(c, pack(target_sp), pipe, bg)["opacity"]) for c in cams]

    # learnable pre-activation parameters, as scene/gaussian_model.py:64-86 activates them
    xyz = (target_sp["means3D"] + 0.02 * torch.randn(n, 3, device=dev)).requires_grad_(True)
    log_scale = torch.log(target_sp["scales"] * 1.3).requires_grad_(True)
    rot = target_sp["rotations"].clone().requires_grad_(True)
    opacity_logit = torch.logit(target_sp["opacities"].clamp(0.05, 0.95) * 0.8).requires_grad_(True)
    shs = (target_sp["shs"] + 0.2 * torch.randn_like(target_sp["shs"])).requires_grad_(True)
    opt = SplatAdam([{"params": [xyz], "lr": 2e-4}, {"params": [log_scale], "lr": 5e-3}, {"params": [rot], "lr": 1e-3},
                     {"params": [opacity_logit], "lr": 2e-2}, {"params": [shs], "lr": 5e-3}])
    losses = []
    for it in range(60):
        opt.zero_grad(set_to_none=True)
        total = 0.0
        for cam, (img_t, alpha_t) in zip(cams, targets):  # view loop of train.py:169, mean of the losses (:242)
            gd = {"means3D": xyz, "active_sh_degree": 1, "gaussian_opacity": torch.sigmoid(opacity_logit),
                  "gaussian_features": shs, "gaussian_scales": torch.exp(log_scale),
                  "gaussian_rotations": torch.nn.functional.normalize(rot)}
            pkg = render(cam, gd, pipe, bg)
            total = total + (pkg["render"] - img_t).abs().mean() + 0.1 * (pkg["opacity"] - alpha_t).abs().mean()
        loss = total / len(cams)
        loss.backward()
        assert pkg["viewspace_points"].grad is not None  # densification statistics input (train.py:307)
        opt.step()
        losses.append(loss.item())
    assert losses[-1] < 0.6 * losses[0], (losses[0], losses[-1])
    assert all(torch.isfinite(p).all() for p in (xyz, log_scale, rot, opacity_logit, shs))
