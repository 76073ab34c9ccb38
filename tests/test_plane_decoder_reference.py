"""tests/plane_decoder_reference.py (the plain-PyTorch yardstick of splatfields_amd/plane_generator.py) against runs of the
reference's own TimeVAEDecoder / Tensorial2D classes, through the fixtures tests/golden/plane_decoder_*.npz.  No GPU.

The bound is the one tests/test_triplane_reference.py holds its fixtures to: the float32 restatement is within 1e-6 of the
tensor's largest magnitude of the fixture, and -- the fixture being a float32 evaluation -- the float64 restatement is no
farther from it than from the float32 restatement beside it."""
import os

import numpy as np
import pytest
import torch

from tests import plane_decoder_reference as R

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def load(name):
    z = np.load(os.path.join(GOLDEN, f"plane_decoder_{name}.npz"))
    return {k: torch.as_tensor(z[k].astype(np.float32) if z[k].dtype == np.float16 else z[k]) for k in z.files}


def state_dict(z, prefix=""):
    sd = {prefix + k[len("param/"):]: v for k, v in z.items() if k.startswith("param/")}
    return sd


def compare(tag, want, run64, run32):
    """want: {name: fixture tensor}; run64 / run32: {name: restatement tensors}"""
    assert want, tag
    for k, w in want.items():
        w = w.double()
        a64, a32 = run64[k], run32[k]
        assert a64.shape == w.shape == a32.shape, (tag, k)
        top = w.abs().max().item()
        r = (a32 - a64).abs().max().item()
        d64, d32 = (a64 - w).abs().max().item(), (a32 - w).abs().max().item()
        print(f"[plane_decoder] {tag} {k}: float32 run - fixture {d32 / top:.2e}, float64 run - fixture {d64 / top:.2e}, own error r {r / top:.2e} (relative)")
        assert d32 <= 1e-6 * top, (tag, k, d32 / top)
        assert 0.0 < r and d64 <= r, (tag, k, d64, r)


def flat(res):
    return {"out": res["out"], **{"grad/" + k: v for k, v in res["grads"].items()}}


def test_decoder_reproduces_the_reference_class():
    z = load("small")
    sd, groups = state_dict(z), int(z["groups"])
    fn = lambda s: R.decoder(s, z["noise"].to(next(iter(s.values())).dtype), groups)
    r64, r32 = (flat(R.run(fn, sd, z["probe"], dt)) for dt in (torch.float64, torch.float32))
    want = {"out": z["out"], **{k: v for k, v in z.items() if k.startswith("grad/")}}
    assert set(want) == set(r64), "the fixture holds a gradient for every parameter"
    compare("small", want, r64, r32)


def test_per_frame_weights_follow_the_reference_class():
    z = load("per_frame")
    sd, groups = state_dict(z), int(z["groups"])
    fids = [int(f) for f in z["frame_ids"]]
    assert len(set(fids)) == 2 and not torch.equal(z[f"out/{fids[0]}"], z[f"out/{fids[1]}"])
    for fid in fids:
        for frame_id in (fid, torch.tensor(float(fid))):       # an int, and the rounded tensor `_time2frame_id` returns
            fn = lambda s: R.decoder(s, z["noise"].to(next(iter(s.values())).dtype), groups, frame_id=frame_id)
            r64, r32 = (flat(R.run(fn, sd, z[f"probe/{fid}"], dt)) for dt in (torch.float64, torch.float32))
            want = {"out": z[f"out/{fid}"], **{"grad/" + k[len(f"grad/{fid}/"):]: v for k, v in z.items() if k.startswith(f"grad/{fid}/")}}
            assert any(k.endswith("frame_weights") for k in want)
            compare(f"per_frame[{fid}]", want, r64, r32)


def test_tensorial2d_reproduces_the_reference_class():
    z = load("tensorial2d")
    sd, groups = state_dict(z), int(z["groups"])
    sd["noise"] = z["noise"]
    assert groups == 32 and tuple(z["out"].shape) == (1, 16, 16, 16)       # noise_res 2, three of the four up blocks upsample
    fn = lambda s: R.tensorial2d(s, groups)
    r64, r32 = (flat(R.run(fn, sd, z["probe"], dt)) for dt in (torch.float64, torch.float32))
    want = {"out": z["out"], **{k: v for k, v in z.items() if k.startswith("grad/")}}
    compare("tensorial2d", want, r64, r32)


def test_fused_layer_restatement_pads_the_activated_tensor():
    """a border tap contributes 0, not SiLU(beta): with x = 0, gamma = 0 the activated tensor is the constant SiLU(beta), and a
    ones-kernel counts the taps inside the image"""
    x = torch.zeros(1, 8, 3, 5, dtype=torch.float64)
    w = torch.ones(8, 8, 3, 3, dtype=torch.float64)
    beta = torch.full((8,), 1.5, dtype=torch.float64)
    out = R.layer(x, w, None, torch.zeros(8, dtype=torch.float64), beta, None, 1, True, False, False)
    s = torch.nn.functional.silu(beta[0]).item()
    assert abs(out[0, 0, 0, 0].item() - 4 * 8 * s) < 1e-12 and abs(out[0, 0, 1, 2].item() - 9 * 8 * s) < 1e-12
