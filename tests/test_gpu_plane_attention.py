"""The plane generator's attention layer on its HIP kernels (splatfields_amd/csrc/attention.hip, `fused_attention`,
`attention="fused"`) on the MI355X against the plain-PyTorch restatement tests/plane_decoder_reference.py in float64.

The measure is the suite's rule (tests/accuracy.py), with r from the float32 restatement.  The kernels compute in double and round
once, so what the allowance has to absorb is their order of summation; a ratio d / 4r above about 0.3 points at a float32
intermediate.

Two tensors are outside that rule, for reasons of the mathematics and not of the kernels:
  * the gradient of `to_k.bias` is analytically zero (a key bias shifts a whole score row, which the softmax does not see); its
    float64 "reference" is rounding residue.  Ours must be exactly zero, in every case;
  * with a single token (T = 1) the softmax is the constant 1 and the gradients of `to_q.weight`, `to_q.bias` and `to_k.weight` are
    identically zero in both restatements, so the ulp floor of the rule is zero as well.  Ours are checked to be finite and at
    most one float32 ulp of the largest magnitude among the case's other parameter gradients."""
import functools
import json
import os

import pytest
import torch

from tests import accuracy
from tests import plane_decoder_reference as R
from tests.accuracy import ulp32
from tests.launches import stage_counts
from tests.plane_cases import GOLDEN, SMALL, load, params_of, run_module

pytestmark = pytest.mark.gpu
within = functools.partial(accuracy.within, "plane_attention")
NAMES = ("group_norm.weight", "group_norm.bias", "to_q.weight", "to_q.bias", "to_k.weight", "to_k.bias", "to_v.weight", "to_v.bias",
         "to_out.0.weight", "to_out.0.bias")
QK_SIDE = ("to_q.weight", "to_q.bias", "to_k.weight")


# ---- the layer alone --------------------------------------------------------------------------------------------------------
CHANNELS = ((8, 1), (8, 8), (24, 4), (32, 32), (64, 4))
SPATIAL = ((1, 1), (1, 2), (3, 5), (5, 13), (9, 9), (20, 20))      # T = 1, 2, 15, 65, 81, 400
PLANES = 2      # two planes with different tensors in every call: the job table
LAYER_CASES = [(c, g, h, w) for c, g in CHANNELS for h, w in SPATIAL if (c // g) * h * w >= 2]     # group_norm refuses a group of one value


def layer_inputs(c, h, w, seed, key_bias=None):
    g = torch.Generator().manual_seed(seed)
    rn = lambda *s: torch.randn(*s, generator=g)
    planes = []
    for _ in range(PLANES):
        t = {"x": rn(1, c, h, w), "group_norm.weight": 1.0 + 0.3 * rn(c), "group_norm.bias": 0.5 * rn(c)}
        for name in ("to_q", "to_k", "to_v", "to_out.0"):
            t[name + ".weight"] = rn(c, c) / c ** 0.5
            t[name + ".bias"] = 0.3 * rn(c)
        t["probe"] = rn(1, c, h, w)
        if key_bias is not None:
            t["to_k.bias"] = key_bias * torch.sign(rn(c))
        planes.append(t)
    return planes


def layer_reference(t, groups, dtype):
    leaf = {k: v.to(dtype).clone().requires_grad_(k != "probe") for k, v in t.items()}
    out = R.attention({"a." + k: leaf[k] for k in NAMES}, "a", leaf["x"], groups)
    (out * leaf["probe"]).sum().backward()
    return {"out": out.detach().double(), "d_x": leaf["x"].grad.double(), **{"d_" + k: leaf[k].grad.double() for k in NAMES}}


def run_layer(ts, groups, dev):
    from splatfields_amd.plane_generator import fused_attention
    leaves = [{k: v.to(dev).requires_grad_(k != "probe") for k, v in t.items()} for t in ts]
    out = fused_attention([d["x"][0] for d in leaves], *[[d[k] for d in leaves] for k in NAMES], groups=groups)
    assert tuple(out.shape) == (len(ts),) + tuple(ts[0]["x"].shape[1:])
    (out * torch.cat([d["probe"] for d in leaves])).sum().backward()
    return [{"out": out[i], "d_x": d["x"].grad, **{"d_" + k: d[k].grad for k in NAMES}} for i, d in enumerate(leaves)]


def check_layer(tag, ts, groups, dev):
    """the comparison of one call for every plane; returns the worst d / 4r"""
    single = ts[0]["x"].shape[-2] * ts[0]["x"].shape[-1] == 1
    worst = 0.0
    for i, (t, got) in enumerate(zip(ts, run_layer(ts, groups, dev))):
        r64, r32 = (layer_reference(t, groups, dt) for dt in (torch.float64, torch.float32))
        assert torch.count_nonzero(got["d_to_k.bias"]).item() == 0, (tag, i, "the gradient of to_k.bias is exactly zero")
        skip = {"d_to_k.bias"} | ({"d_" + k for k in QK_SIDE} if single else set())
        worst = max(worst, within(f"{tag} plane {i}", got, {k: v for k, v in r64.items() if k not in skip}, r32))
        if single:
            top = max(r64["d_" + k].abs().max().item() for k in NAMES if k not in QK_SIDE and k != "to_k.bias")
            for k in QK_SIDE:
                assert r64["d_" + k].abs().max().item() == 0.0, (tag, k, "identically zero in the reference")
                g = got["d_" + k].double().cpu()
                assert torch.isfinite(g).all() and g.abs().max().item() <= ulp32(top), (tag, i, k, g.abs().max().item(), ulp32(top))
    return worst


@pytest.mark.parametrize("case", LAYER_CASES, ids=lambda s: f"c{s[0]}g{s[1]}-{s[2]}x{s[3]}")
def test_fused_attention_against_float64(hip_device, case):
    c, groups, h, w = case
    ts = layer_inputs(c, h, w, seed=10000 * c + 100 * groups + 10 * h + w)
    check_layer(f"{c} channels, {groups} groups, {h}x{w}", ts, groups, hip_device)


def test_every_shape_is_covered():
    assert len(LAYER_CASES) == len(CHANNELS) * len(SPATIAL) - 2        # (8, 8) and (32, 32) at one token: one value per group
    assert sorted({h * w for _, _, h, w in LAYER_CASES}) == [1, 2, 15, 65, 81, 400]


def test_chunks_of_several_token_blocks(hip_device):
    """beyond 16 blocks of 32 tokens the partial sums of the parameter gradients run over several blocks per chunk: 575 tokens
    are 18 blocks (the last one short), two per chunk"""
    ts = layer_inputs(8, 23, 25, seed=575)
    check_layer("8 channels, 2 groups, 23x25", ts, 2, hip_device)


@pytest.mark.parametrize("case", ((32, 4, 3, 5), (8, 1, 13, 5), (64, 64, 20, 20)), ids=lambda s: f"c{s[0]}g{s[1]}-{s[2]}x{s[3]}")
def test_large_logits_do_not_saturate(hip_device, case):
    """to_k.bias = +-1000: every score row is shifted by q_i . b / sqrt(C), far beyond what exp takes in double (709) -- the
    softmax does not change, but only a row maximum subtracted first keeps it finite"""
    c, groups, h, w = case
    ts = layer_inputs(c, h, w, seed=77 + c, key_bias=1000.0)
    for t in ts:          # on the reference alone: the shift is what the case is about, and no compared tensor is residue
        r64 = layer_reference(t, groups, torch.float64)
        x = t["x"].double()
        tok = torch.nn.functional.group_norm(x.view(1, c, h * w), groups, t["group_norm.weight"].double(), t["group_norm.bias"].double(),
                                             R.EPS).transpose(1, 2)[0]
        q = tok @ t["to_q.weight"].double().T + t["to_q.bias"].double()
        shift = q @ t["to_k.bias"].double() / c ** 0.5
        assert shift.abs().max().item() > 709.0, shift.abs().max().item()
        for k, v in r64.items():
            if k != "d_to_k.bias":
                assert v.abs().max().item() >= 1e-3, (k, v.abs().max().item())
    check_layer(f"key bias +-1000, {c} channels, {groups} groups, {h}x{w}", ts, groups, hip_device)


def test_bad_shapes_raise_before_any_launch(hip_device):
    from splatfields_amd.plane_generator import fused_attention

    def call(c, h, w, groups, dev=hip_device):
        z = lambda *s: torch.zeros(*s, device=dev)
        return fused_attention([z(c, h, w)], [z(c)], [z(c)], *([z(c, c)], [z(c)]) * 4, groups=groups)

    for c, h, w, groups in ((12, 4, 4, 4), (72, 4, 4, 4), (8, 4, 4, 3), (8, 1, 4097, 1), (8, 4097, 1, 1), (8, 1, 1, 8)):
        with pytest.raises(ValueError):
            call(c, h, w, groups)
    with pytest.raises(RuntimeError, match="no CPU path"):
        call(8, 4, 4, 1, dev="cpu")
    assert tuple(call(8, 64, 64, 2).shape) == (1, 8, 64, 64)          # the largest token count is inside


# ---- the fixtures through the module ------------------------------------------------------------------------------------------
def test_small_fixture_through_the_module(hip_device):
    from splatfields_amd.plane_generator import TimeVAEDecoder
    z = load("small")
    sd = params_of(z)
    net = TimeVAEDecoder(**SMALL, attention="fused")
    net.load_state_dict(sd, strict=True)
    net.to(hip_device)
    out, grads = run_module(net, z["noise"].to(hip_device), z["probe"].to(hip_device))
    fn = lambda s: R.decoder(s, z["noise"].double(), int(z["groups"]))
    r64 = R.run(fn, sd, z["probe"], torch.float64)
    want64 = {"out": r64["out"], **{"grad/" + k: v for k, v in r64["grads"].items()}}
    ref32 = {"out": z["out"], **{k: v for k, v in z.items() if k.startswith("grad/")}}       # the reference's own float32 run
    assert set(want64) == set(ref32)
    within("small fixture", {"out": out, **{"grad/" + k: v for k, v in grads.items()}}, want64, ref32)
    out2, grads2 = run_module(net, z["noise"].to(hip_device), z["probe"].to(hip_device))
    assert torch.equal(out, out2) and all(torch.equal(grads[k], grads2[k]) for k in grads), "repeated calls are bit-identical"


def test_per_frame_fixture_through_the_module(hip_device):
    from splatfields_amd.plane_generator import TimeVAEDecoder
    z = load("per_frame")
    sd = params_of(z)
    net = TimeVAEDecoder(**SMALL, layer_kwargs={"n_frames": 3, "strategy": "per_frame"}, attention="fused")
    net.load_state_dict(sd, strict=True)
    net.to(hip_device)
    for n, fid in enumerate(int(f) for f in z["frame_ids"]):
        frame_id = fid if n == 0 else torch.tensor(float(fid), device=hip_device)     # once an int, once the rounded device tensor
        out, grads = run_module(net, z["noise"].to(hip_device), z[f"probe/{fid}"].to(hip_device), frame_id=frame_id)
        fn = lambda s: R.decoder(s, z["noise"].double(), int(z["groups"]), frame_id=fid)
        r64 = R.run(fn, sd, z[f"probe/{fid}"], torch.float64)
        ref32 = {"out": z[f"out/{fid}"], **{"grad/" + k[len(f"grad/{fid}/"):]: v for k, v in z.items() if k.startswith(f"grad/{fid}/")}}
        want64 = {"out": r64["out"], **{k: r64["grads"][k[len("grad/"):]] for k in ref32 if k != "out"}}
        within(f"per_frame fixture, frame {fid}", {"out": out, **{"grad/" + k: v for k, v in grads.items()}}, want64, ref32)


def test_tensorial2d_fixture_through_the_module(hip_device):
    from splatfields_amd.plane_generator import Tensorial2D
    z = load("tensorial2d")
    sd = {**params_of(z), "noise": z["noise"]}
    mod = Tensorial2D(8, 16, 2, layer_kwargs={"n_frames": 0, "strategy": "none"}, attention="fused")
    mod.load_state_dict(sd, strict=True)
    mod.to(hip_device)
    mod.zero_grad()
    out = mod(frame_id=None)
    assert tuple(out.shape) == (1, 16, 16, 16)
    (out * z["probe"].to(hip_device)).sum().backward()
    grads = {"grad/" + n: p.grad for n, p in mod.named_parameters()}
    r64 = R.run(lambda s: R.tensorial2d(s, 32), sd, z["probe"], torch.float64)
    ref32 = {"out": z["out"], **{k: v for k, v in z.items() if k.startswith("grad/")}}
    want64 = {"out": r64["out"], **{k: r64["grads"][k[len("grad/"):]] for k in ref32 if k != "out"}}
    within("tensorial2d fixture", {"out": out, **grads}, want64, ref32)


# ---- reference size ---------------------------------------------------------------------------------------------------------
def randomise(module, seed):
    """every parameter random and non-zero (the reference's initialisation zeroes half the network, `to_out` of the attention
    included), GroupNorm biases of order 1"""
    g = torch.Generator().manual_seed(seed)
    norms = {id(p) for m in module.modules() if isinstance(m, torch.nn.GroupNorm) for p in m.parameters()}
    with torch.no_grad():
        for name, p in module.named_parameters():
            r = torch.randn(p.shape, generator=g)
            if id(p) in norms:
                v = 1.0 + 0.3 * r if name.endswith("weight") else r
            elif name.endswith("frame_weights"):
                v = r / p[0][0].numel() ** 0.5
            elif p.dim() > 1:
                v = r / p[0].numel() ** 0.5
            else:
                v = 0.3 * r
            p.copy_(v)


def test_reference_size_three_planes_and_repeats(hip_device):
    from splatfields_amd.plane_generator import VarTriPlaneEncoder
    enc = VarTriPlaneEncoder({"layer_kwargs": {"n_frames": 0, "strategy": "none"}, "attention": "fused"})
    randomise(enc, 7)
    sd = {k: v.detach().clone() for k, v in enc.state_dict().items()}
    probe = torch.randn(3, 16, 160, 160, generator=torch.Generator().manual_seed(8))
    r64, r32 = (R.run(lambda s: R.planes(s, 32), sd, probe, dt) for dt in (torch.float64, torch.float32))
    enc.to(hip_device)
    runs = []
    for _ in range(2):
        enc.zero_grad()
        planes = enc.get_planes(None)
        assert tuple(planes.shape) == (3, 16, 160, 160)
        (planes * probe.to(hip_device)).sum().backward()
        runs.append((planes.detach().clone(), {n: p.grad.detach().clone() for n, p in enc.named_parameters()}))
    assert set(runs[0][1]) == set(r64["grads"]), "a gradient for every parameter"
    for k, v in runs[0][1].items():
        if k.endswith("to_k.bias"):
            assert torch.count_nonzero(v).item() == 0, k
    flat = lambda out, grads: {"out": out, **{"grad/" + k: v for k, v in grads.items()}}
    within("reference size", flat(*runs[0]), flat(r64["out"], r64["grads"]), flat(r32["out"], r32["grads"]))
    assert torch.equal(runs[0][0], runs[1][0]) and all(torch.equal(runs[0][1][k], runs[1][1][k]) for k in runs[0][1]), \
        "repeated calls are bit-identical"


# ---- launch budget ----------------------------------------------------------------------------------------------------------
def test_launch_budget_of_both_paths(hip_device):
    from splatfields_amd.plane_generator import ATTENTION_LAUNCHES, Tensorial2D, generate_planes
    subs = [Tensorial2D(8, 16, 4).to(hip_device) for _ in range(3)]

    def step(k, attention):
        def fn():
            out = generate_planes([s.net for s in subs[:k]], [s.noise for s in subs[:k]], attention=attention)
            out.sum().backward()
        return fn

    fwd, bwd = ATTENTION_LAUNCHES
    assert fwd <= 4 and bwd <= 8
    one, three = stage_counts(step(1, "fused"))[1], stage_counts(step(3, "fused"))[1]
    print(f"[plane_attention] library launches per step, fused: one plane {one}, three planes {three} (stage 0 forward, stage 6 backward)")
    assert one == three
    assert one[0] == 67 + fwd and one[6] == 116 + bwd and sum(one) == 183 + fwd + bwd
    one, three = stage_counts(step(1, "torch"))[1], stage_counts(step(3, "torch"))[1]
    assert one == three and one[0] == 67 and one[6] == 116 and sum(one) == 183


# ---- the default is what it was -----------------------------------------------------------------------------------------------
def test_the_default_is_the_torch_path(hip_device):
    from splatfields_amd import plane_generator as pg
    start = pg.attention()
    assert start == "torch" or os.environ.get("SPLATFIELDS_PLANE_ATTENTION") == start
    subs = [pg.Tensorial2D(8, 16, 4).to(hip_device) for _ in range(3)]
    for s in subs:
        randomise(s, 5)
    probe = torch.randn(3, 16, 32, 32, generator=torch.Generator().manual_seed(6)).to(hip_device)

    def run(**kw):
        for s in subs:
            s.zero_grad()
        out = pg.generate_planes([s.net for s in subs], [s.noise for s in subs], **kw)
        (out * probe).sum().backward()
        return out.detach().clone(), [p.grad.detach().clone() for s in subs for p in s.parameters()]

    pg.set_attention("torch")
    try:
        (o0, g0), (o1, g1), (o2, g2) = run(), run(attention="torch"), run(attention="fused")
    finally:
        pg.set_attention(start)
    assert torch.equal(o0, o1) and len(g0) == len(g1) and all(torch.equal(a, b) for a, b in zip(g0, g1))
    assert torch.allclose(o0, o2, rtol=1e-4, atol=1e-4 * o0.abs().max().item())


def test_splatfields_with_the_fused_attention_end_to_end(hip_device):
    """Every `encoder.subs.*` parameter but `to_k.bias` must receive a finite, non-zero gradient (the parameters are first
    overwritten with random non-zero values, as in tests/test_gpu_plane_generator.py); `to_k.bias` receives its exact zeros."""
    from splatfields_amd.deform_field import SplatFields
    torch.manual_seed(3)
    model = SplatFields(encoder_args={"generator": "decoder", "noise_res": 4, "attention": "fused"}, n_frames=4, layer_strategy="per_frame")
    assert all(s.net.attention == "fused" for s in model.encoder.subs)
    randomise(model.encoder, 11)
    model.to(hip_device)
    xyz = (torch.rand(2000, 3, device=hip_device) * 2 - 1) * 0.9
    t = torch.full((2000, 1), 2.0 / 3.0, device=hip_device)             # frame 2 of 0..3
    out = model(xyz, t)
    loss = sum(v.square().sum() for k, v in out.items() if torch.is_tensor(v))
    loss.backward()
    checked = 0
    for name, p in model.named_parameters():
        if name.startswith("encoder.subs."):
            assert p.grad is not None and torch.isfinite(p.grad).all(), name
            if name.endswith("to_k.bias"):
                assert torch.count_nonzero(p.grad).item() == 0, name
            else:
                assert p.grad.abs().max() > 0, name
            checked += 1
    keys = json.load(open(os.path.join(GOLDEN, "plane_decoder_keys.json")))["per_frame"]
    assert checked == sum(1 for k, _ in keys if not k.endswith("noise"))
