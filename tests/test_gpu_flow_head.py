"""The fused flow head (splatfields_amd/csrc/flow_head.hip, `FlowHead(path="fused")`) on the MI355X against the PyTorch-op path of
the same module on the CPU, which tests/test_flow_head.py pins to the reference's own classes.

The measure is the suite's rule (tests/accuracy.py), with r from the float32 torch path on the CPU.  No element is left out; the
inputs never hold an exactly-zero w_raw (the one stated limit of the SE(3) models, shared with the reference).

Shapes: N = 1 (one lane), 63 / 64 / 65 (a wavefront's edge), 255 / 256 / 257 (the workgroup's edge: a workgroup is 256 points),
1000 (several workgroups); widths 4 (one vector), 36 (not a multiple of the 16 columns a pass moves), 128 (the reference's) and
256 (the limit); K = 1, 4, 10 bases.  Branch weights scaled by 1e-3, 1 and 8 put theta between ~1e-3 (the cancellation in
theta - sin theta) and beyond 2 pi (the range reduction of sin / cos)."""
import pytest
import torch

from splatfields_amd.deform_field import FLOW_MODELS, FlowHead, SplatFields
from tests.accuracy import within
from tests.launches import device_records

pytestmark = pytest.mark.gpu
N_FRAMES, FRAME_ID, TIME_STEP = 6, 3, 0.625
NS = (1, 63, 64, 65, 255, 256, 257, 1000)
WIDTHS = (4, 36, 128, 256)


def make_case(model, n, width, k=4, scale=1.0, seed=0, integers=False):
    """a head with random branches (weights and biases times `scale`), inputs and probes, all float32 values on the CPU"""
    g = torch.Generator().manual_seed(1000 * seed + 7 * n + width + 13 * k)
    rn = lambda *s: torch.randn(*s, generator=g)
    head = FlowHead(W=width, flow_model=model, num_basis=k, n_frames=N_FRAMES)
    with torch.no_grad():
        for name, p in head.named_parameters():
            if name.startswith("branch_") or name.startswith("gaussian_warp"):
                p.copy_(rn(*p.shape) * scale * (0.5 if name.endswith("bias") else 1.0 / width ** 0.5))
                if integers:
                    p.copy_(torch.randint(-3, 4, p.shape, generator=g).float())
            elif name.startswith("basis_net"):           # the SIREN's initialisation, from this case's generator
                fan_in = p.shape[-1] if name.endswith("weight") else dict(head.named_parameters())[name[:-4] + "weight"].shape[-1]
                bound = 1.0 / fan_in if name.endswith("weight") and name.startswith("basis_net.net.0") else \
                    ((6.0 / fan_in) ** 0.5 / 30 if name.endswith("weight") else 1.0 / fan_in ** 0.5)
                p.copy_((torch.rand(p.shape, generator=g) * 2 - 1) * bound)
    t = {"hidden": rn(n, width), "pts": torch.rand(n, 3, generator=g) * 2 - 1, "probe_flow": rn(*((n, 4, 4) if model == "se3" else (n, 3))),
         "probe_means": rn(n, 3)}
    if integers:
        t = {k_: torch.randint(-4, 5, v.shape, generator=g).float() for k_, v in t.items()}
    return head, t


def run(head, t, dtype, device, path, upstream="both", gain=1.0):
    """flow, means3D and every gradient of sum(probe . output) * gain; `upstream`: "both" or "means" (nothing reads `flow`)"""
    import copy
    h = copy.deepcopy(head).to(dtype).to(device)
    h.path = path
    hidden = t["hidden"].detach().to(dtype).to(device).clone().requires_grad_()
    pts = t["pts"].detach().to(dtype).to(device).clone().requires_grad_()
    flow, means = h(hidden, pts, time_step=torch.tensor(TIME_STEP, dtype=dtype, device=device), frame_id=torch.tensor(FRAME_ID, device=device))
    loss = (means * (t["probe_means"] * gain).to(dtype).to(device)).sum()
    if upstream == "both":
        loss = loss + (flow * (t["probe_flow"] * gain).to(dtype).to(device)).sum()
    loss.backward()
    out = {"flow": flow.detach(), "means3D": means.detach(), "d_hidden": hidden.grad, "d_pts": pts.grad}
    for name, p in h.named_parameters():
        out["d_" + name] = p.grad if p.grad is not None else torch.zeros_like(p)
    return out


def check(tag, head, t, dev, **kw):
    cpu = torch.device("cpu")
    r64, r32 = (run(head, t, dt, cpu, "torch", **kw) for dt in (torch.float64, torch.float32))
    got = run(head, t, torch.float32, dev, "fused", **kw)
    assert set(got) == set(r64)
    assert got["flow"].dtype == torch.float32 and got["flow"].shape == r64["flow"].shape
    return within("flow_head", tag, got, r64, r32)


@pytest.mark.parametrize("model", FLOW_MODELS)
def test_every_model_at_the_reference_width(hip_device, model):
    head, t = make_case(model, 257, 128)
    check(f"{model} N=257 W=128", head, t, hip_device)


@pytest.mark.parametrize("width", WIDTHS)
@pytest.mark.parametrize("model", ("se3", "se3Scaled"))
def test_point_counts_and_widths(hip_device, model, width):
    for n in NS:
        head, t = make_case(model, n, width, seed=1)
        check(f"{model} N={n} W={width}", head, t, hip_device)


@pytest.mark.parametrize("k", (1, 4, 10))
@pytest.mark.parametrize("model", ("dct", "dct_siren"))
def test_basis_counts(hip_device, model, k):
    for n in (65, 257, 1000):
        head, t = make_case(model, n, 128, k=k, seed=2)
        check(f"{model} K={k} N={n}", head, t, hip_device)


@pytest.mark.parametrize("scale", (1e-3, 1.0, 8.0))
@pytest.mark.parametrize("model", ("se3", "se3Affine", "se3Scaled"))
def test_weight_scales_from_tiny_angles_to_several_turns(hip_device, model, scale):
    head, t = make_case(model, 257, 128, scale=scale, seed=3)
    with torch.no_grad():
        w = torch.nn.functional.linear(t["hidden"], head.branch_w.weight, head.branch_w.bias).norm(dim=-1)
    print(f"[flow_head] {model} scale {scale}: theta in [{w.min().item():.2e}, {w.max().item():.2e}]")
    assert w.min().item() > 0
    check(f"{model} scale={scale}", head, t, hip_device)


@pytest.mark.parametrize("model", FLOW_MODELS)
def test_upstream_gradients(hip_device, model):
    """nothing reads `flow` (the training loop: dL/dflow is null), and both outputs at magnitudes 2^-20 and 2^20"""
    head, t = make_case(model, 257, 36, seed=4)
    check(f"{model} means only", head, t, hip_device, upstream="means")
    for e in (-20, 20):
        check(f"{model} gain 2^{e}", head, t, hip_device, gain=2.0 ** e)


@pytest.mark.parametrize("model", FLOW_MODELS)
def test_two_identical_calls_are_bit_identical(hip_device, model):
    head, t = make_case(model, 1000, 128, k=10, seed=5)
    a, b = (run(head, t, torch.float32, hip_device, "fused") for _ in range(2))
    for k in a:
        assert torch.equal(a[k], b[k]), (model, k)


def test_offset_with_small_integers_is_exact(hip_device):
    head, t = make_case("offset", 257, 36, seed=6, integers=True)
    ref = run(head, t, torch.float32, torch.device("cpu"), "torch")
    got = run(head, t, torch.float32, hip_device, "fused")
    for k in ref:
        assert torch.equal(got[k].cpu(), ref[k]), k


@pytest.mark.parametrize("model", FLOW_MODELS)
def test_no_points(hip_device, model):
    head, t = make_case(model, 0, 128, seed=7)
    got = run(head, t, torch.float32, hip_device, "fused")
    assert tuple(got["flow"].shape) == ((0, 4, 4) if model == "se3" else (0, 3)) and tuple(got["means3D"].shape) == (0, 3)
    assert tuple(got["d_hidden"].shape) == (0, 128) and tuple(got["d_pts"].shape) == (0, 3)
    for k, v in got.items():
        if k.startswith("d_branch") or k.startswith("d_gaussian_warp"):
            assert v.shape == dict(head.named_parameters())[k[2:]].shape and torch.count_nonzero(v).item() == 0, k


def test_float64_and_autocast_inputs_are_converted_at_the_boundary(hip_device):
    head, t = make_case("se3Scaled", 65, 36, seed=8)
    want = run(head, t, torch.float32, hip_device, "fused")
    h = FlowHead(W=36, flow_model="se3Scaled", path="fused").to(hip_device)
    h.load_state_dict(head.state_dict())
    hidden64 = t["hidden"].double().to(hip_device).requires_grad_()
    flow, means = h(hidden64, t["pts"].double().to(hip_device))
    (means * t["probe_means"].to(hip_device)).sum().backward()
    assert flow.dtype == torch.float32 and torch.equal(means, want["means3D"]) and hidden64.grad.dtype == torch.float64
    with torch.autocast("cuda", dtype=torch.bfloat16):
        flow, means = h(t["hidden"].to(hip_device), t["pts"].to(hip_device))
    assert means.dtype == torch.float32 and torch.equal(means, want["means3D"]) and torch.equal(flow, want["flow"])


def library_launches(fn):
    """device records of the flow head's kernels and of the weight-gradient kernels it calls while fn runs"""
    return [n for n in device_records(fn) if "k_flow_head" in n or "k_mlp_weight_grad" in n]


@pytest.mark.parametrize("model", FLOW_MODELS)
def test_launch_counts_are_within_the_budget(hip_device, model):
    """a condition of the design: 1 library kernel forward, at most 3 backward (the epilogue's and sr_mlp_weight_grad's two)"""
    from splatfields_amd.flow_head import FLOW_HEAD_LAUNCHES
    assert FLOW_HEAD_LAUNCHES == (1, 3)
    dev = hip_device
    head, t = make_case(model, 1000, 128, seed=9)
    h = head.to(dev)
    h.path = "fused"
    hidden, pts = t["hidden"].to(dev).requires_grad_(), t["pts"].to(dev).requires_grad_()
    args = dict(time_step=torch.tensor(TIME_STEP, device=dev), frame_id=torch.tensor(FRAME_ID, device=dev))
    held = {}

    def forward():
        flow, means = h(hidden, pts, **args)
        held["loss"] = (means * t["probe_means"].to(dev)).sum() + (flow * t["probe_flow"].to(dev)).sum()

    forward()
    held["loss"].backward()            # warm up
    fwd = library_launches(forward)
    bwd = library_launches(lambda: held["loss"].backward())
    print(f"[flow_head] launches {model}: forward {fwd}, backward {bwd}")
    assert len(fwd) <= 1 and len(bwd) <= 3, (model, fwd, bwd)
    assert len(fwd) + len(bwd) > 0, "the profiler recorded none of the library's kernels: the budget was not checked"
    assert len(fwd) == 1 and any("k_flow_head_backward" in n for n in bwd)


def test_rows_beyond_two_gigabytes_are_addressed_with_64_bits(hip_device):
    """N W 4 bytes > 2^31: the last rows equal a call on those rows alone (every point is independent and summed in the same
    order), and the weight gradients of the two chunks the slab kernel needs add up to the whole call's"""
    dev = hip_device
    n, width = (1 << 21) + 300, 256
    assert 4 * n * width > 1 << 31
    head, _ = make_case("se3", 1, width, seed=10)
    h = head.to(dev)
    h.path = "fused"
    g = torch.Generator(device=dev).manual_seed(11)
    hidden = torch.randn(n, width, device=dev, generator=g).requires_grad_()
    pts = torch.rand(n, 3, device=dev, generator=g)
    probe = torch.randn(n, 3, device=dev, generator=g)
    flow, means = h(hidden, pts)
    (means * probe).sum().backward()
    whole = [means, flow, hidden.grad] + [p.grad.clone() for p in h.parameters()]
    n_max = ((1 << 31) - 1) // (4 * width) // 64 * 64
    assert n_max < n
    parts = []
    for lo, hi in ((0, n_max), (n_max, n)):
        for p in h.parameters():
            p.grad = None
        x = hidden.detach()[lo:hi].clone().requires_grad_()
        fl, me = h(x, pts[lo:hi])
        (me * probe[lo:hi]).sum().backward()
        assert torch.equal(me, whole[0][lo:hi]) and torch.equal(fl, whole[1][lo:hi]) and torch.equal(x.grad, whole[2][lo:hi]), (lo, hi)
        parts.append([p.grad.clone() for p in h.parameters()])
    for total, a, b in zip(whole[3:], *parts):
        assert torch.equal(total, a + b)


@pytest.mark.parametrize("model", ("se3", "se3Scaled", "dct_siren"))
def test_whole_network(hip_device, monkeypatch, model):
    """SplatFields(flow_head="fused") against flow_head="torch" with the same weights, 300 points, no plane features, depth-2 MLPs.
    The float64 side is the network on the CPU with the fused MLP op replaced by its formula (as tests/test_deform_field.py runs
    it).  The rule is applied twice: with r from the float32 torch-path network on the CPU (the same formula), and with r from
    the float32 network with the torch head ON THE DEVICE, where the MLP kernels' own rounding, which both heads sit behind, is in
    r and in d alike."""
    from splatfields_amd import general_mlp
    from test_general_mlp import formula
    dev = hip_device
    quick = dict(encoder_type="none", deform_d=2, rgb_d=2, flow_d=2, scale_d=2, opacity_d=2, rotation_d=2, flow_model=model,
                 deform_skips=[0], rgb_skips=[0], flow_skips=[0], scale_skips=[0], opacity_skips=[0])
    torch.manual_seed(12)
    nets = {p: SplatFields(n_frames=6, flow_head=p, **quick) for p in ("torch", "fused")}
    with torch.no_grad():
        for name, p in nets["torch"].mlp_flow_head.named_parameters():
            if name.startswith("branch_"):
                p.copy_(torch.randn(p.shape) * (0.5 if name.endswith("bias") else 0.1))
    nets["fused"].load_state_dict(nets["torch"].state_dict(), strict=True)
    assert list(nets["fused"].state_dict()) == list(nets["torch"].state_dict())
    x = torch.rand(300, 3) * 2 - 1
    t = torch.full((300, 1), 0.4)
    probes = None

    def step(net, dtype, device):
        nonlocal probes
        net = net.to(dtype).to(device)
        xyz = x.to(dtype).to(device).clone().requires_grad_()
        out = net(xyz, t.to(dtype).to(device))
        out = {k: v for k, v in out.items() if torch.is_tensor(v)}
        if probes is None:
            g = torch.Generator().manual_seed(13)
            probes = {k: torch.randn(v.shape, generator=g) for k, v in out.items()}
        sum((v * probes[k].to(dtype).to(device)).sum() for k, v in out.items()).backward()
        res = {"out_" + k: v.detach() for k, v in out.items()}
        res["d_xyz"] = xyz.grad
        for name, p in net.named_parameters():
            res["d_" + name] = p.grad if p.grad is not None else torch.zeros_like(p)
        return res

    import copy
    with monkeypatch.context() as m:
        m.setattr(general_mlp, "fused_general_mlp", formula)
        r64 = step(copy.deepcopy(nets["torch"]), torch.float64, torch.device("cpu"))
        r32_cpu = step(copy.deepcopy(nets["torch"]), torch.float32, torch.device("cpu"))
    r32 = step(nets["torch"], torch.float32, dev)
    got = step(nets["fused"], torch.float32, dev)
    r64 = {k: v.double().cpu() for k, v in r64.items()}
    within("flow_head", f"network {model}, r from the CPU", got, r64, r32_cpu)
    within("flow_head", f"network {model}, r from the device", got, r64, {k: v.cpu() for k, v in r32.items()})
