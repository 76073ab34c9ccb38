"""The plane generator (splatfields_amd/plane_generator.py, csrc/planegen.hip) on the MI355X against the plain-PyTorch restatement
tests/plane_decoder_reference.py, which tests/test_plane_decoder_reference.py pins to runs of the reference's own classes.

The measure is the suite's rule (tests/accuracy.py), with r from the float32 restatement; for the fixtures the float32 evaluation
is the reference's own run (the fixture)."""
import functools
import itertools
import json
import os

import pytest
import torch

from tests import accuracy
from tests import plane_decoder_reference as R
from tests.launches import stage_counts
from tests.plane_cases import GOLDEN, SMALL, load, params_of, run_module

pytestmark = pytest.mark.gpu
within = functools.partial(accuracy.within, "plane_generator")


# ---- single fused layer ------------------------------------------------------------------------------------------------------
CHANNELS = ((8, 32), (32, 32), (32, 16), (24, 40))
SPATIAL = ((1, 2), (3, 5), (7, 7), (20, 20))
PLANES = 2      # two planes with different tensors in every call: the job table


def layer_inputs(cin, cout, h, w, up, seed):
    g = torch.Generator().manual_seed(seed)
    H, W = (2 * h, 2 * w) if up else (h, w)
    rn = lambda *s: torch.randn(*s, generator=g)
    return [dict(x=rn(1, cin, h, w), weight=rn(cout, cin, 3, 3) / (9 * cin) ** 0.5, bias=0.3 * rn(cout), gamma=1.0 + 0.3 * rn(cin),
                 beta=1.0 + 0.5 * rn(cin), residual=rn(1, cout, H, W), probe=rn(1, cout, H, W)) for _ in range(PLANES)]


def layer_reference(t, groups, prologue, up, res, silu, dtype):
    leaf = {k: v.to(dtype).clone().requires_grad_(k != "probe") for k, v in t.items()}
    out = R.layer(leaf["x"], leaf["weight"], leaf["bias"], leaf["gamma"], leaf["beta"], leaf["residual"] if res else None, groups, prologue, up, silu)
    (out * leaf["probe"]).sum().backward()
    names = ["x", "weight", "bias"] + (["gamma", "beta"] if prologue else []) + (["residual"] if res else [])
    return {"out": out.detach().double(), **{"d_" + k: leaf[k].grad.double() for k in names}}


@pytest.mark.parametrize("hw", SPATIAL, ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("ch", CHANNELS, ids=lambda c: f"{c[0]}to{c[1]}")
def test_fused_layer_every_flag_combination(hip_device, ch, hw):
    from splatfields_amd.plane_generator import fused_layer
    (cin, cout), (h, w) = ch, hw
    worst = 0.0
    for ci, (prologue, up, res, silu) in enumerate(itertools.product((False, True), repeat=4)):
        for groups in ((1, 4, cin) if prologue else (1,)):
            ts = layer_inputs(cin, cout, h, w, up, seed=1000 * cin + 100 * h + ci)
            dev = [{k: v.to(hip_device).requires_grad_(k != "probe") for k, v in t.items()} for t in ts]
            col = lambda k: [d[k][0] if k in ("x", "residual") else d[k] for d in dev]      # per plane: without the batch dimension
            out = fused_layer(col("x"), col("weight"), col("bias"), col("gamma") if prologue else None, col("beta") if prologue else None,
                              col("residual") if res else None, groups=groups, upsample=up, silu_out=silu)
            assert out.shape[0] == PLANES
            (out * torch.cat([d["probe"] for d in dev])).sum().backward()
            for i, t in enumerate(ts):
                r64, r32 = (layer_reference(t, groups, prologue, up, res, silu, dt) for dt in (torch.float64, torch.float32))
                got = {"out": out[i], **{k: dev[i][k[2:]].grad for k in r64 if k != "out"}}
                tag = f"{cin}->{cout} {h}x{w} groups {groups} prologue {int(prologue)} up {int(up)} res {int(res)} silu {int(silu)} plane {i}"
                worst = max(worst, within(tag, got, r64, r32))
    print(f"[plane_generator] layer {cin}->{cout} {h}x{w}: worst d/4r over all combinations {worst:.3f}")


def test_padding_applies_to_the_activated_tensor(hip_device):
    """x = 0, gamma = 0, beta = 1.5: the activated tensor is the constant SiLU(1.5); a ones-kernel counts the taps inside"""
    from splatfields_amd.plane_generator import fused_layer
    z = lambda *s: torch.zeros(*s, device=hip_device)
    out = fused_layer([z(8, 3, 5)], [torch.ones(8, 8, 3, 3, device=hip_device)], [z(8)], [z(8)], [torch.full((8,), 1.5, device=hip_device)], groups=1)
    s = torch.nn.functional.silu(torch.tensor(1.5)).item()
    assert abs(out[0, 0, 0, 0].item() - 32 * s) < 1e-4 and abs(out[0, 0, 1, 2].item() - 72 * s) < 1e-4 and abs(out[0, 3, 2, 4].item() - 32 * s) < 1e-4


def test_bad_shapes_raise_value_error_before_any_launch(hip_device):
    from splatfields_amd.plane_generator import fused_layer
    t = lambda *s: torch.zeros(*s, device=hip_device)
    with pytest.raises(ValueError):
        fused_layer([t(12, 4, 4)], [t(16, 12, 3, 3)], [t(16)])
    with pytest.raises(ValueError):
        fused_layer([t(8, 4, 4)], [t(72, 8, 3, 3)], [t(72)])
    with pytest.raises(ValueError):
        fused_layer([t(8, 4, 4)], [t(8, 8, 3, 3)], [t(8)], [t(8)], [t(8)], groups=3)
    with pytest.raises(RuntimeError, match="no CPU path"):
        fused_layer([torch.zeros(8, 4, 4)], [torch.zeros(8, 8, 3, 3)], [torch.zeros(8)])


# ---- the fixtures through the module ------------------------------------------------------------------------------------------
def test_small_fixture_through_the_module(hip_device):
    from splatfields_amd.plane_generator import TimeVAEDecoder
    z = load("small")
    sd = params_of(z)
    net = TimeVAEDecoder(**SMALL)
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
    net = TimeVAEDecoder(**SMALL, layer_kwargs={"n_frames": 3, "strategy": "per_frame"})
    net.load_state_dict(sd, strict=True)
    net.to(hip_device)
    outs = []
    for n, fid in enumerate(int(f) for f in z["frame_ids"]):
        frame_id = fid if n == 0 else torch.tensor(float(fid), device=hip_device)     # once an int, once the rounded device tensor
        out, grads = run_module(net, z["noise"].to(hip_device), z[f"probe/{fid}"].to(hip_device), frame_id=frame_id)
        outs.append(out)
        fn = lambda s: R.decoder(s, z["noise"].double(), int(z["groups"]), frame_id=fid)
        r64 = R.run(fn, sd, z[f"probe/{fid}"], torch.float64)
        ref32 = {"out": z[f"out/{fid}"], **{"grad/" + k[len(f"grad/{fid}/"):]: v for k, v in z.items() if k.startswith(f"grad/{fid}/")}}
        want64 = {"out": r64["out"], **{k: r64["grads"][k[len("grad/"):]] for k in ref32 if k != "out"}}
        assert any(k.endswith("frame_weights") for k in want64)
        within(f"per_frame fixture, frame {fid}", {"out": out, **{"grad/" + k: v for k, v in grads.items()}}, want64, ref32)
    assert not torch.equal(outs[0], outs[1]), "the two frames differ"


def test_tensorial2d_fixture_through_the_module(hip_device):
    from splatfields_amd.plane_generator import Tensorial2D
    z = load("tensorial2d")
    sd = {**params_of(z), "noise": z["noise"]}
    mod = Tensorial2D(8, 16, 2, layer_kwargs={"n_frames": 0, "strategy": "none"})
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
    """every parameter random and non-zero (the reference's initialisation zeroes half the network), GroupNorm biases of order 1"""
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
    enc = VarTriPlaneEncoder({"layer_kwargs": {"n_frames": 0, "strategy": "none"}})
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
    flat = lambda out, grads: {"out": out, **{"grad/" + k: v for k, v in grads.items()}}
    within("reference size", flat(*runs[0]), flat(r64["out"], r64["grads"]), flat(r32["out"], r32["grads"]))
    assert torch.equal(runs[0][0], runs[1][0]) and all(torch.equal(runs[0][1][k], runs[1][1][k]) for k in runs[0][1]), \
        "repeated calls are bit-identical"


# ---- launch budget ----------------------------------------------------------------------------------------------------------
def test_three_planes_cost_the_launches_of_one(hip_device):
    from splatfields_amd.plane_generator import Tensorial2D, generate_planes
    subs = [Tensorial2D(8, 16, 4).to(hip_device) for _ in range(3)]

    def step(k):
        def fn():
            out = generate_planes([s.net for s in subs[:k]], [s.noise for s in subs[:k]])
            out.sum().backward()
        return fn

    one, three = stage_counts(step(1))[1], stage_counts(step(3))[1]
    print(f"[plane_generator] library launches per step: one plane {one}, three planes {three} (stage 0 forward, stage 6 backward)")
    assert one == three
    # conv_in 1, ten resnet blocks x (2 statistics x 2 + 2 convolutions), three upsamplers, conv_out 2 + 1;
    # backward: per convolution 2 (weight gradient) + 1 (data gradient, not for conv_in), per GroupNorm 2
    assert one[0] == 1 + 10 * 6 + 3 + 3 == 67 and one[6] == 2 + 10 * 10 + 3 * 3 + 5 == 116 and sum(one) == 183


# ---- end to end -------------------------------------------------------------------------------------------------------------
def test_splatfields_with_the_generator_end_to_end(hip_device):
    """Every `encoder.subs.*` parameter must receive a finite, non-zero gradient.  At the reference's initialisation that is
    impossible for the tensors in front of a zeroed `conv2` (their gradient is exactly zero in exact arithmetic), so the
    parameters are first overwritten with random non-zero values: nothing is left at zero and EVERY parameter is checked."""
    from splatfields_amd.deform_field import SplatFields
    torch.manual_seed(3)
    model = SplatFields(encoder_args={"generator": "decoder", "noise_res": 4}, n_frames=4, layer_strategy="per_frame")
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
            assert p.grad is not None and torch.isfinite(p.grad).all() and p.grad.abs().max() > 0, name
            if name.endswith("frame_weights"):
                assert p.grad[2].abs().max() > 0 and p.grad[0].abs().max() == 0, name      # the selected frame, and only it
            checked += 1
    keys = json.load(open(os.path.join(GOLDEN, "plane_decoder_keys.json")))["per_frame"]
    assert checked == sum(1 for k, _ in keys if not k.endswith("noise"))
    twin = SplatFields(encoder_args={"generator": "decoder", "noise_res": 4}, n_frames=4, layer_strategy="per_frame").to(hip_device)
    twin.load_state_dict(model.state_dict(), strict=True)
    with torch.no_grad():
        a, b = model(xyz, t), twin(xyz, t)
    assert all(torch.equal(a[k], b[k]) for k in a if torch.is_tensor(a[k])), "a state_dict round trip reproduces the output bit for bit"
