"""The tail of the training objective on the MI355X (splatfields_amd/losses.py -> sr_splat_reg_* / sr_depth_l1_*,
csrc/objective.hip) and training_objective, against the float64 restatement tests/objective_reference.py.

Tolerance (the rule of tests/test_gpu_losses.py::assert_within, per input): for every value and every gradient tensor the
deviation from the float64 restatement may be 4 r, where r is the deviation of the float32 restatement from the float64 one on
the SAME inputs, computed on the CPU in the test.  Where r is 0 the result must equal the float64 value rounded to float32.
Values: |d value|.  Gradient tensors: max |d grad| / max |grad|.  Nothing is exempted."""
import pytest
import torch

from tests import objective_reference as R
from tests.launches import device_records

pytestmark = pytest.mark.gpu

SPLAT_SIZES = (1, 2, 63, 64, 65, 255, 256, 257, 1000, 70001)     # a lane, a wavefront +-1, a workgroup +-1, many workgroups + tail
DEPTH_SHAPES = ((1, 1, 1), (1, 3, 5), (2, 17, 33), (3, 130, 70))
ALONE = {"norm": (1.0, 0.0, 0.0), "norm_mean": (0.0, 1.0, 0.0), "opacity": (0.0, 0.0, 1.0)}
TOGETHER = (0.01, 0.02, 0.03)
OBJECTIVE_LAMBDAS = {"lambda_dssim": 0.2, "lambda_mask": 0.1, "lambda_norm": 0.01, "lambda_norm_mean": 0.02, "lambda_opacity": 0.03,
                     "lambda_depthl1": 0.05, "lambda_gradient": 0.5}
VALUE_KEYS, GRAD_KEYS = ("loss", "norm", "norm_mean", "opacity", "depthl1", "items"), ("d_means3D", "d_opacity", "d_depth")


def splat_inputs(n, scale=1.0):
    gen = torch.Generator().manual_seed(1000 + n)
    x = torch.randn(n, 3, generator=gen) * 1.3
    o = torch.rand(n, 1, generator=gen)
    if n > 2:
        x[1] = 0.0
    return x * scale, o


def depth_inputs(shape, seed=0):
    gen = torch.Generator().manual_seed(77 + seed + shape[1] * shape[2])
    d = torch.rand(shape, generator=gen) * 4.0 + 0.5
    g = torch.rand(shape, generator=gen) * 4.0 + 0.5
    pick = torch.rand(shape, generator=gen)
    g = torch.where(pick < 0.4, torch.zeros(()), torch.where(pick < 0.45, -g, g))     # about 40 % zeros, some negative values
    return d, g


def assert_within(tag, got, f32, f64):
    """got / f32 / f64: dicts of the same keys (values and gradient tensors); prints every figure before it asserts."""
    failures = []
    for k, want in f64.items():
        dev = R.grad_deviation if k in GRAD_KEYS else R.value_deviation
        r, d = dev(f32[k], want), dev(got[k], want)
        print(f"[objective] {tag} {k}: deviation {d:.3e}  r {r:.3e}  allowed {4 * r:.3e}")
        if r == 0.0:
            if not torch.equal(torch.as_tensor(got[k]).cpu().float().reshape(-1), want.float().reshape(-1)):
                failures.append((k, "r = 0: must equal the float64 value rounded to float32", d))
        elif not d <= 4.0 * r:
            failures.append((k, d, 4.0 * r))
    assert not failures, (tag, failures)


def hip_splat(dev, x, o, lam, upstream=1.0):
    from splatfields_amd.losses import splat_regularizers
    xd = x.to(dev).requires_grad_(True) if (lam[0] or lam[1]) else None
    od = o.to(dev).requires_grad_(True) if lam[2] else None
    loss, terms = splat_regularizers(xd, od, *lam)
    assert loss.dim() == 0 and loss.requires_grad and not any(t.requires_grad for t in terms.values())
    (loss if upstream == 1.0 else upstream * loss).backward()
    out = {"loss": loss.detach(), **terms}
    if xd is not None:
        out["d_means3D"] = xd.grad
    if od is not None:
        out["d_opacity"] = od.grad
    return {k: v.cpu() for k, v in out.items()}


def restated_splat(x, o, lam):
    return (R.splat_terms(x, o, *lam, dtype=torch.float32), R.splat_terms(x, o, *lam, dtype=torch.float64))


# ---------------------------------------------------------------------------------------------------------- splat terms

@pytest.mark.parametrize("n", SPLAT_SIZES)
def test_splat_terms_alone_and_together(hip_device, n):
    from splatfields_amd.losses import centered_position_norm, opacity_regularizer, position_norm
    x, o = splat_inputs(n)
    drop_in = {"norm": lambda: position_norm(xd), "norm_mean": lambda: centered_position_norm(xd), "opacity": lambda: opacity_regularizer(od)}
    for name, lam in ALONE.items():
        xd, od = x.to(hip_device).requires_grad_(True), o.to(hip_device).requires_grad_(True)
        value = drop_in[name]()
        assert value.dim() == 0 and value.dtype == torch.float32
        value.backward()
        got = {"loss": value.detach().cpu(), name: value.detach().cpu()}
        if name == "opacity":
            got["d_opacity"] = od.grad.cpu()
            assert xd.grad is None and od.grad.shape == o.shape
        else:
            got["d_means3D"] = xd.grad.cpu()
            assert od.grad is None
            if n > 2 and name == "norm":
                assert torch.equal(got["d_means3D"][1], torch.zeros(3)), "the zero row's gradient must be exactly 0"
        f32, f64 = restated_splat(x, o, lam)
        assert_within(f"n={n} {name}", got, f32, f64)
    f32, f64 = restated_splat(x, o, TOGETHER)
    assert_within(f"n={n} together", hip_splat(hip_device, x, o, TOGETHER), f32, f64)


@pytest.mark.parametrize("scale", [1e-6, 1e6])
def test_scaled_coordinates(hip_device, scale):
    x, o = splat_inputs(1000, scale)
    f32, f64 = restated_splat(x, o, TOGETHER)
    assert_within(f"scale {scale}", hip_splat(hip_device, x, o, TOGETHER), f32, f64)


def exact_case():
    """256 rows from (1,2,2) (length 3) and (2,3,6) (length 7), every row beside its negation: the mean is exactly 0, every sum
    is exact in float32.  96 + 32 = 128 pairs."""
    a, b = torch.tensor([1.0, 2.0, 2.0]), torch.tensor([2.0, 3.0, 6.0])
    signs = torch.tensor([[1.0, 1, 1], [1, -1, 1], [-1, 1, 1], [1, 1, -1]])
    half = torch.cat([(a * signs[i % 4])[None] for i in range(96)] + [(b * signs[i % 4])[None] for i in range(32)])
    x = torch.stack([half, -half], dim=1).reshape(256, 3)
    lengths = torch.tensor([3.0] * 96 + [7.0] * 32).repeat_interleave(2)
    o = torch.tensor([0.0, 0.5, 1.0, 0.5]).repeat(64)[:, None]
    return x, lengths, o


def test_exact_arithmetic_case(hip_device):
    x, lengths, o = exact_case()
    norm = torch.tensor((192 * 3 + 64 * 7) / 256)               # 4.0
    opacity = torch.tensor((64 * 1.0 + 128 * 0.25) / 256)       # 0.375
    unit = (x.double() / lengths.double()[:, None])
    for lam in (ALONE["norm"], ALONE["norm_mean"], (1.0, 1.0, 0.0), (0.5, 0.25, 2.0)):
        got = hip_splat(hip_device, x, o, lam)
        if lam[0]:
            assert torch.equal(got["norm"], norm)
        if lam[1]:
            assert torch.equal(got["norm_mean"], norm)            # the mean is 0: the centred norm is the norm
        if lam[2]:
            assert torch.equal(got["opacity"], opacity)
            assert torch.equal(got["d_opacity"], (lam[2] * 2 * (o.double() - 1) / 256).float())
        assert torch.equal(got["loss"], lam[0] * norm + lam[1] * norm + lam[2] * (opacity if lam[2] else 0.0))
        assert torch.equal(got["d_means3D"], ((lam[0] + lam[1]) * unit / 256).float())


def test_identical_rows_have_centred_norm_zero_and_gradient_exactly_zero(hip_device):
    from splatfields_amd.losses import centered_position_norm
    for n in (1, 5, 300):
        x = torch.tensor([[3.0, -7.0, 11.0]]).repeat(n, 1).to(hip_device).requires_grad_(True)
        v = centered_position_norm(x)
        v.backward()
        assert v.item() == 0.0 and torch.equal(x.grad, torch.zeros_like(x)), n


# ---------------------------------------------------------------------------------------------------------- depth L1

def hip_depth(dev, d, g, item_weights=None):
    from splatfields_amd.losses import depth_l1_loss
    dd = d.to(dev).requires_grad_(True)
    if item_weights is None:
        v = depth_l1_loss(dd, g.to(dev))
        assert v.dim() == 0
        v.backward()
        return {"depthl1": v.detach().cpu(), "d_depth": dd.grad.cpu()}
    items = depth_l1_loss(dd, g.to(dev), size_average=False)
    assert tuple(items.shape) == (d.shape[0],)
    (items * item_weights.to(dev)).sum().backward()
    return {"items": items.detach().cpu(), "d_depth": dd.grad.cpu()}


@pytest.mark.parametrize("shape", DEPTH_SHAPES)
def test_depth_l1_values_and_gradients(hip_device, shape):
    d, g = depth_inputs(shape)
    weights = torch.tensor([1.0, -2.0, 0.37])[:shape[0]]
    for tag, dm, gm in (("random", d, g), ("all valid", d, g.abs() + 0.25), ("all invalid", d, -g.abs())):
        got = hip_depth(hip_device, dm, gm)
        assert_within(f"{shape} {tag}", got, R.depth_terms(dm, gm, torch.float32), R.depth_terms(dm, gm, torch.float64))
        if tag == "all invalid":
            assert got["depthl1"].item() == 0.0 and torch.equal(got["d_depth"], torch.zeros(shape))
        got = hip_depth(hip_device, dm, gm, weights)
        assert_within(f"{shape} {tag} per item", got, R.depth_terms(dm, gm, torch.float32, weights), R.depth_terms(dm, gm, torch.float64, weights))
    # d == g on the valid pixels: sign(0) = 0
    same = torch.where(g > 0, g, d)
    got = hip_depth(hip_device, same, g)
    assert got["depthl1"].item() == 0.0 and torch.equal(got["d_depth"], torch.zeros(shape))
    # the masked pixels count in the divisor, the valid ones get +-1 / (B H W)
    got = hip_depth(hip_device, d, g)
    want = (torch.sign(d - g) * (g > 0)).double() / d.numel()
    assert torch.equal(got["d_depth"], want.float())


def test_depth_shapes_hw_and_1hw(hip_device):
    from splatfields_amd.losses import depth_l1_loss
    d, g = depth_inputs((1, 17, 33))
    base = hip_depth(hip_device, d, g)
    for ds, gs in ((d[0], g[0]), (d, g[0]), (d[0], g)):
        x = ds.to(hip_device).requires_grad_(True)
        v = depth_l1_loss(x, gs.to(hip_device))
        v.backward()
        assert torch.equal(v.detach().cpu(), base["depthl1"]) and x.grad.shape == ds.shape
        assert torch.equal(x.grad.cpu().reshape(-1), base["d_depth"].reshape(-1))


# ---------------------------------------------------------------------------------------------------------- interface

def test_half_precision_render_does_not_round_the_target(hip_device):
    from splatfields_amd.losses import depth_l1_loss
    d, g = depth_inputs((2, 17, 33))
    half = d.half().to(hip_device).requires_grad_(True)
    v = depth_l1_loss(half, g.to(hip_device))               # float32 target beside a float16 render
    v.backward()
    base = hip_depth(hip_device, d.half().float(), g)
    assert v.dtype == torch.float16 and half.grad.dtype == torch.float16
    assert torch.equal(v.detach().cpu(), base["depthl1"].half()) and torch.equal(half.grad.cpu(), base["d_depth"].half())


def test_float64_and_non_contiguous_inputs(hip_device):
    from splatfields_amd.losses import depth_l1_loss, splat_regularizers
    dev = hip_device
    x, o = splat_inputs(257)
    base = hip_splat(dev, x, o, TOGETHER)
    x64, o64 = x.double().to(dev).requires_grad_(True), o.double().to(dev).requires_grad_(True)
    loss, terms = splat_regularizers(x64, o64, *TOGETHER)
    loss.backward()
    assert loss.dtype == torch.float64 and terms["norm"].dtype == torch.float64 and x64.grad.dtype == torch.float64 and o64.grad.dtype == torch.float64
    assert torch.equal(loss.detach().float().cpu(), base["loss"]) and torch.equal(x64.grad.float().cpu(), base["d_means3D"])
    assert torch.equal(o64.grad.float().cpu(), base["d_opacity"])
    xt = x.t().contiguous().to(dev).requires_grad_(True)            # [3, N] storage, read through a transposed view
    wide = torch.zeros(257, 4, device=dev)
    wide[:, :1] = o.to(dev)
    wide.requires_grad_(True)
    assert not xt.t().is_contiguous() and not wide[:, :1].is_contiguous()
    loss, _ = splat_regularizers(xt.t(), wide[:, :1], *TOGETHER)
    loss.backward()
    assert torch.equal(loss.detach().cpu(), base["loss"]) and torch.equal(xt.grad.t().cpu(), base["d_means3D"])
    assert torch.equal(wide.grad[:, :1].cpu(), base["d_opacity"]) and (wide.grad[:, 1:] == 0).all()
    d, g = depth_inputs((2, 17, 33))
    base = hip_depth(dev, d, g)
    pad = torch.zeros(2, 17, 40, device=dev)
    pad[:, :, :33] = d.to(dev)
    pad.requires_grad_(True)
    v = depth_l1_loss(pad[:, :, :33], g.double().to(dev))           # a strided view and a float64 target
    v.backward()
    assert torch.equal(v.detach().cpu(), base["depthl1"]) and torch.equal(pad.grad[:, :, :33].cpu(), base["d_depth"])


@pytest.mark.parametrize("skip", [1, 2, 3])
def test_slices_with_a_storage_offset(hip_device, skip):
    """means3D[k:] is contiguous and only 4-byte aligned: rows start on a 16-byte boundary at another phase."""
    from splatfields_amd.losses import depth_l1_loss, splat_regularizers
    dev = hip_device
    x, o = splat_inputs(1000)
    xs, os_ = x[skip:], o[skip:]
    f32, f64 = restated_splat(xs, os_, TOGETHER)
    for opacity_sliced in (True, False):        # the opacities in phase with the rows, and out of phase (element by element)
        xd, od = x.to(dev).requires_grad_(True), (o if opacity_sliced else os_.clone()).to(dev).requires_grad_(True)
        view, oview = xd[skip:], (od[skip:] if opacity_sliced else od)
        assert view.data_ptr() % 16 != 0 and view.is_contiguous()
        loss, terms = splat_regularizers(view, oview, *TOGETHER)
        loss.backward()
        got = {"loss": loss.detach(), **terms, "d_means3D": xd.grad[skip:], "d_opacity": od.grad[skip:] if opacity_sliced else od.grad}
        assert_within(f"slice {skip} opacity sliced {opacity_sliced}", {k: v.cpu() for k, v in got.items()}, f32, f64)
        assert (xd.grad[:skip] == 0).all()
    # without the centred norm a row's gradient does not depend on how the rows are grouped: the aligned copy gives the same bits
    lam = (0.01, 0.0, 0.03)
    aligned = hip_splat(dev, xs.clone(), os_.clone(), lam)
    sliced = _slice_run(x.to(dev).requires_grad_(True), o.to(dev).requires_grad_(True), skip, lam)
    assert torch.equal(aligned["d_means3D"], sliced["d_means3D"]) and torch.equal(aligned["d_opacity"], sliced["d_opacity"])
    d, g = depth_inputs((2, 17, 33))
    base = hip_depth(dev, d, g)
    flat_d = torch.zeros(d.numel() + skip, device=dev)
    flat_d[skip:] = d.to(dev).reshape(-1)
    flat_d.requires_grad_(True)
    flat_g = torch.zeros(g.numel() + skip, device=dev)
    flat_g[skip:] = g.to(dev).reshape(-1)
    for target in (flat_g[skip:].view(2, 17, 33), g.to(dev)):       # in phase with the depth (vectors), and out of phase
        flat_d.grad = None
        v = depth_l1_loss(flat_d[skip:].view(2, 17, 33), target)
        v.backward()
        assert torch.equal(v.detach().cpu(), base["depthl1"]) and torch.equal(flat_d.grad[skip:].cpu(), base["d_depth"].reshape(-1))


def _slice_run(xd, od, skip, lam):
    from splatfields_amd.losses import splat_regularizers
    loss, terms = splat_regularizers(xd[skip:], od[skip:], *lam)
    loss.backward()
    out = {"loss": loss.detach(), **terms, "d_means3D": xd.grad[skip:], "d_opacity": od.grad[skip:]}
    return {k: v.cpu() for k, v in out.items()}


def test_upstream_gradient_retain_graph_and_inputs_without_grad(hip_device):
    from splatfields_amd.losses import depth_l1_loss, splat_regularizers
    dev = hip_device
    x, o = splat_inputs(1000)
    f32, f64 = restated_splat(x, o, TOGETHER)
    scaled = lambda t: {k: 3.0 * v for k, v in t.items() if k in GRAD_KEYS}
    got = hip_splat(dev, x, o, TOGETHER, upstream=3.0)              # the factor lives on the device: (3 * loss).backward()
    assert_within("upstream 3", {k: got[k] for k in ("d_means3D", "d_opacity")}, scaled(f32), scaled(f64))
    xd, od = x.to(dev).requires_grad_(True), o.to(dev)              # the opacities do not require grad
    loss, _ = splat_regularizers(xd, od, *TOGETHER)
    loss.backward(retain_graph=True)
    first = xd.grad.clone()
    xd.grad = None
    loss.backward()
    assert torch.equal(xd.grad, first) and od.grad is None
    assert torch.equal(first.cpu(), hip_splat(dev, x, o, TOGETHER)["d_means3D"])
    plain, _ = splat_regularizers(x.to(dev), o.to(dev), *TOGETHER)   # nothing requires grad: no graph
    assert not plain.requires_grad and torch.equal(plain.cpu(), loss.detach().cpu())
    with torch.no_grad():
        quiet, _ = splat_regularizers(xd, od, *TOGETHER)
    assert quiet.grad_fn is None and torch.equal(quiet, plain)
    d, g = depth_inputs((2, 17, 33))
    dd = d.to(dev).requires_grad_(True)
    v = depth_l1_loss(dd, g.to(dev))
    (3.0 * v).backward(retain_graph=True)
    first = dd.grad.clone()
    dd.grad = None
    (3.0 * v).backward()
    want = R.depth_terms(d, g, torch.float64)["d_depth"] * 3.0
    assert torch.equal(dd.grad, first) and torch.equal(first.cpu(), want.float())     # 3 / 1122 rounds once either way
    assert not depth_l1_loss(d.to(dev), g.to(dev)).requires_grad


def test_bit_reproducible(hip_device):
    x, o = splat_inputs(70001)
    d, g = depth_inputs((3, 130, 70))
    first = None
    for _ in range(3):
        a, b = hip_splat(hip_device, x, o, TOGETHER), hip_depth(hip_device, d, g)
        got = list(a.values()) + list(b.values())
        first = first or got
        assert all(torch.equal(p, q) for p, q in zip(got, first))


def test_empty_inputs_and_errors(hip_device):
    from splatfields_amd.losses import centered_position_norm, depth_l1_loss, opacity_regularizer, position_norm, splat_regularizers
    dev = hip_device
    empty = torch.zeros(0, 3, device=dev, requires_grad=True)
    v = position_norm(empty)
    v.backward()
    assert torch.isnan(v) and empty.grad.shape == (0, 3)            # the mean of nothing, as the reference's expression gives
    assert torch.isnan(centered_position_norm(torch.zeros(0, 3, device=dev))) and torch.isnan(opacity_regularizer(torch.zeros(0, 1, device=dev)))
    assert torch.isnan(depth_l1_loss(torch.zeros(1, 0, 5, device=dev), torch.zeros(1, 0, 5, device=dev)))
    x, o = torch.rand(8, 3), torch.rand(8, 1)
    for call in (lambda: position_norm(x), lambda: opacity_regularizer(o), lambda: depth_l1_loss(x, x)):
        with pytest.raises(RuntimeError, match="no CPU path"):
            call()
    with pytest.raises(RuntimeError, match=r"must be \[N,3\]"):
        position_norm(torch.rand(8, 4, device=dev))
    with pytest.raises(RuntimeError, match="opacities"):
        splat_regularizers(x.to(dev), torch.rand(7, 1, device=dev), 0.1, 0.0, 0.1)
    with pytest.raises(RuntimeError, match="without opacity"):
        splat_regularizers(x.to(dev), None, 0.1, 0.0, 0.1)
    with pytest.raises(RuntimeError, match="same size"):
        depth_l1_loss(torch.rand(2, 4, 5, device=dev), torch.rand(2, 5, 4, device=dev))
    with pytest.raises(RuntimeError, match="target requires grad"):
        depth_l1_loss(torch.rand(2, 4, 5, device=dev), torch.rand(2, 4, 5, device=dev, requires_grad=True))


def test_no_host_wait_from_the_python_side(hip_device):
    from splatfields_amd.losses import depth_l1_loss, splat_regularizers, training_objective
    dev = hip_device
    x, o = splat_inputs(1000)
    xd, od = x.to(dev).requires_grad_(True), o.to(dev).requires_grad_(True)
    d, g = depth_inputs((2, 17, 33))
    dd, gd = d.to(dev).requires_grad_(True), g.to(dev)
    step = objective_step(dev, [(32, 48)] * 2)

    def run():
        loss, _ = splat_regularizers(xd, od, *TOGETHER)
        (3 * loss).backward()
        (0.5 * depth_l1_loss(dd, gd)).backward()
        total, log = training_objective(**step["kwargs"], **OBJECTIVE_LAMBDAS)
        total.backward()
        return loss, total, log

    run()                                                            # warm up: library load, allocator
    torch.cuda.synchronize()
    try:
        torch.cuda.set_sync_debug_mode("error")
    except Exception as e:   # noqa: BLE001
        pytest.skip(f"this torch build does not implement set_sync_debug_mode: {e}")
    try:
        loss, total, log = run()
    finally:
        torch.cuda.set_sync_debug_mode("default")
    torch.cuda.synchronize()
    assert torch.isfinite(loss) and torch.isfinite(total) and all(torch.isfinite(v) for v in log.values())


def library_launches(fn):
    """device records of this library's objective kernels while fn runs"""
    return [n for n in device_records(fn) if "k_splat_reg" in n or "k_depth_l1" in n]


def test_launch_counts_are_within_the_budgets(hip_device):
    """Conditions of the design: splat terms forward <= 2 launches, <= 3 with the centred norm, backward 1; depth L1 forward
    <= 2, backward 1."""
    from splatfields_amd.losses import depth_l1_loss, splat_regularizers
    dev = hip_device
    x, o = splat_inputs(70001)
    xd, od = x.to(dev).requires_grad_(True), o.to(dev).requires_grad_(True)
    d, g = depth_inputs((3, 130, 70))
    dd, gd = d.to(dev).requires_grad_(True), g.to(dev)
    held = {}
    splat_regularizers(xd, od, *TOGETHER)[0].backward()               # warm up
    depth_l1_loss(dd, gd).backward()
    seen = 0
    for lam, budget in ((TOGETHER, 3), ((0.01, 0.0, 0.03), 2), (ALONE["norm_mean"], 3), (ALONE["opacity"], 2)):
        fwd = library_launches(lambda: held.update(loss=splat_regularizers(xd, od, *lam)[0]))
        bwd = library_launches(lambda: held["loss"].backward())
        print(f"[objective] launches {lam}: forward {fwd}, backward {bwd}")
        assert len(fwd) <= budget and len(bwd) <= 1, (lam, fwd, bwd)
        seen += len(fwd) + len(bwd)
    fwd = library_launches(lambda: held.update(loss=depth_l1_loss(dd, gd)))
    bwd = library_launches(lambda: held["loss"].backward())
    print(f"[objective] launches depth L1: forward {fwd}, backward {bwd}")
    assert len(fwd) <= 2 and len(bwd) <= 1
    assert seen + len(fwd) + len(bwd) > 0, "the profiler recorded none of the library's kernels: the budgets were not checked"


# ---------------------------------------------------------------------------------------------------------- the objective

STEP_CACHE = {}


def objective_step(dev, shapes):
    """The seeded step of these shapes with N = 1000 splats, its literal loop in float32 and float64 (computed once), and the
    keyword arguments of training_objective as lists of leaves on the device."""
    key = tuple(shapes)
    if key not in STEP_CACHE:
        views, splats, gradient_error, extra = R.make_step(shapes, 1000, seed=11 + len(shapes))
        STEP_CACHE[key] = {"inputs": (views, splats, gradient_error, extra),
                           "f32": R.evaluate_loop(views, splats, gradient_error, extra, OBJECTIVE_LAMBDAS, torch.float32),
                           "f64": R.evaluate_loop(views, splats, gradient_error, extra, OBJECTIVE_LAMBDAS, torch.float64)}
    step = dict(STEP_CACHE[key])
    views, splats, gradient_error, extra = step["inputs"]
    leaf = lambda t: t.to(dev).requires_grad_(True)
    step["kwargs"] = dict(images=[leaf(v["image"]) for v in views], gt_images=[v["gt_image"].to(dev) for v in views],
                          opacities=[leaf(v["opacity"]) for v in views], gt_masks=[v["gt_mask"].to(dev) for v in views],
                          depths=[leaf(v["depth"]) for v in views], gt_depths=[v["gt_depth"].to(dev) for v in views],
                          means3D=leaf(splats["means3D"]), gaussian_opacity=leaf(splats["gaussian_opacity"]),
                          gradient_error=gradient_error.to(dev), extra=extra.to(dev))
    return step


def flatten(result):
    """{"loss", "log", "grads"} -> one flat dict of values and per-view gradient tensors"""
    out = {"loss": result["loss"]}
    out.update({f"log/{k}": v for k, v in result["log"].items()})
    for k, g in result["grads"].items():
        if isinstance(g, list):
            out.update({f"d_{k}/{i}": t for i, t in enumerate(g)})
        else:
            out[f"d_{k}"] = g
    return out


def run_objective(kwargs, stacked=False):
    from splatfields_amd.losses import training_objective
    kw = dict(kwargs)
    per_view = ("images", "gt_images", "opacities", "gt_masks", "depths", "gt_depths")
    for t in [t for k in per_view for t in kwargs[k]] + [kwargs["means3D"], kwargs["gaussian_opacity"]]:
        t.grad = None
    if stacked:
        kw.update({k: torch.stack(kwargs[k]) for k in per_view})
    loss, log = training_objective(**kw, **OBJECTIVE_LAMBDAS)
    assert loss.dim() == 0 and set(log) == {"Ll1", "mask", "depthl1", "opacity", "loss_gradient"}
    assert not any(v.requires_grad for v in log.values()) and all(v.is_cuda for v in log.values())
    loss.backward()
    grads = {"image": [t.grad for t in kwargs["images"]], "opacity": [t.grad for t in kwargs["opacities"]],
             "depth": [t.grad for t in kwargs["depths"]], "means3D": kwargs["means3D"].grad, "gaussian_opacity": kwargs["gaussian_opacity"].grad}
    return {k: v.detach().cpu() for k, v in flatten({"loss": loss, "log": log, "grads": grads}).items()}


def assert_objective_within(tag, got, step):
    f32, f64 = flatten(step["f32"]), flatten(step["f64"])
    failures = []
    for k, want in f64.items():
        dev = R.grad_deviation if k.startswith("d_") else R.value_deviation
        r, d = dev(f32[k], want), dev(got[k], want)
        print(f"[objective] {tag} {k}: deviation {d:.3e}  r {r:.3e}  allowed {4 * r:.3e}")
        assert got[k].shape == want.shape, (k, got[k].shape, want.shape)
        if r == 0.0:
            if not torch.equal(got[k].float(), want.float()):
                failures.append((k, "r = 0: must equal the float64 value rounded to float32", d))
        elif not d <= 4.0 * r:
            failures.append((k, d, 4.0 * r))
    assert not failures, (tag, failures)


@pytest.mark.parametrize("n_views", [1, 3])
def test_training_objective_list_and_stacked(hip_device, n_views):
    step = objective_step(hip_device, [(32, 48)] * n_views)
    as_list = run_objective(step["kwargs"])
    assert_objective_within(f"V={n_views}", as_list, step)
    as_stack = run_objective(step["kwargs"], stacked=True)
    assert all(torch.equal(as_list[k], as_stack[k]) for k in as_list), "a list of views and the stacked tensor must give identical bits"


def test_training_objective_views_of_two_shapes(hip_device):
    step = objective_step(hip_device, [(32, 48), (20, 36)])
    assert_objective_within("V=2, two shapes", run_objective(step["kwargs"]), step)


def test_training_objective_with_every_optional_term_off_is_the_photometric_loss(hip_device):
    from splatfields_amd.losses import photometric_loss, training_objective
    kw = objective_step(hip_device, [(32, 48)] * 3)["kwargs"]
    images, gts = torch.stack([t.detach() for t in kw["images"]]), torch.stack(kw["gt_images"])
    x = images.clone().requires_grad_(True)
    want, want_l1 = photometric_loss(x, gts, 0.2)
    want.backward()
    y = images.clone().requires_grad_(True)
    loss, log = training_objective(y, gts, lambda_dssim=0.2)
    loss.backward()
    assert torch.equal(loss.detach(), want.detach()) and torch.equal(log["Ll1"], want_l1) and torch.equal(y.grad, x.grad)
    assert all(log[k].item() == 0.0 for k in ("mask", "depthl1", "opacity", "loss_gradient"))
    # tensors given with their weights at 0 are not touched either (the reference tests `> 0`)
    z = images.clone().requires_grad_(True)
    loss, _ = training_objective(z, gts, opacities=kw["opacities"], gt_masks=kw["gt_masks"], depths=kw["depths"], gt_depths=kw["gt_depths"],
                                 means3D=kw["means3D"], gaussian_opacity=kw["gaussian_opacity"], gradient_error=kw["gradient_error"],
                                 lambda_dssim=0.2)
    assert torch.equal(loss.detach(), want.detach())
