"""tests/mlp_bf16_reference.py -- the plain-PyTorch statement of the bf16 precision of the fused MLP chains that the GPU tests
compare the HIP kernels with -- pinned on CPU: its rounding is torch's bfloat16 conversion, it reproduces the reference's own
GeneralMLP run with a rounding linear op (tests/golden/mlp_bf16_cases.npz, float64), and the exact-arithmetic networks of
`exact_case` are exact: float32 in two summation orders equals float64 bit for bit."""
import os

import numpy as np
import pytest
import torch

import mlp_bf16_reference as R

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
CASES = ["scale", "opacity", "rotation", "deform", "static_rgb", "no_features"]


def test_rounding_is_torch_bfloat16_conversion_ties_included():
    g = torch.Generator().manual_seed(5)
    bits = torch.randint(-2 ** 31, 2 ** 31 - 1, (200000,), generator=g, dtype=torch.int64).to(torch.int32)
    hi = bits & ~0xFFFF
    ties = torch.cat([hi | 0x8000, hi | 0x7FFF, hi | 0x8001, hi])           # exactly half way (both parities above), either side, exact
    special = torch.tensor([0.0, -0.0, float("inf"), -float("inf"), 3.3895314e38, -3.3895314e38, 1e-40, -1e-45, 1.0, 1.00390625,
                            1.01171875, 255.5, 0.00390625]).view(torch.int32)
    x = torch.cat([bits, ties, special]).view(torch.float32)
    got, want = R.bf16_round(x), x.to(torch.bfloat16).to(torch.float32)
    finite = ~torch.isnan(want)
    assert torch.equal(torch.isnan(got), torch.isnan(want))
    assert torch.equal(got[finite].view(torch.int32), want[finite].view(torch.int32))
    assert R.bf16_round(torch.tensor([1.00390625, 1.01171875])).tolist() == [1.0, 1.015625]   # ties: down to even, up to even
    x64 = torch.randn(1000, generator=g, dtype=torch.float64)
    assert R.bf16_round(x64).dtype == torch.float64 and torch.equal(R.bf16_round(x64), x64.to(torch.bfloat16).double())


@pytest.mark.parametrize("name", CASES)
def test_restatement_reproduces_the_reference_with_a_rounding_linear(name):
    """float64, <= 1e-12 relative L2 per tensor; the `.weight` gradients travel as float32 (<= 2^-23), the `.matrix_t` gradients
    as the outer product of those with the frame's coefficients that they are (tests/golden/make_mlp_bf16_golden.py)."""
    kwargs, data, emul, _, _ = R.load_fixture_case(GOLDEN, name)
    params = {k[len("param:"):]: torch.from_numpy(data[k]).double().requires_grad_() for k in data.files if k.startswith("param:")}
    xyz = torch.from_numpy(data["xyz"]).double().requires_grad_()
    feat = torch.from_numpy(data["feat"]).double().requires_grad_() if "feat" in data.files else None
    frame = int(data["frame_id"])
    out = R.general_mlp(params, kwargs, xyz, feat, None if frame < 0 else frame)
    (out * torch.from_numpy(data["probe"]).double()).sum().backward()
    got = {"out": out.detach(), "grad_xyz": xyz.grad}
    if feat is not None:
        got["grad_feat"] = feat.grad
    got.update({"grad:" + k: (p.grad if p.grad is not None else torch.zeros_like(p)) for k, p in params.items()})
    assert set(got) == set(emul)
    for k, v in got.items():
        want = torch.from_numpy(emul[k])
        err = ((v - want).norm() / want.norm().clamp_min(1e-300)).item()
        assert err <= (2.0 ** -23 if k.endswith((".weight", ".matrix_t")) else 1e-12), (k, err)


@pytest.mark.parametrize("shape", sorted(R.EXACT_SHAPES))
@pytest.mark.parametrize("n_points", [77, 1])
def test_exact_networks_are_exact_in_float32(shape, n_points):
    """outputs and dL/dinput of the exact-arithmetic networks: float32 adding first-to-last, float32 adding last-to-first and
    float64 agree bit for bit (the weight gradients sum over the points and are only float32-accurate)."""
    case = R.exact_case(shape, n_points)
    want = R.run_chain(*case, dtype=torch.float64)
    assert (want["y"] != 0).double().mean() > 0.9 and (want["d_in"] != 0).double().mean() > 0.9      # nothing degenerate
    for mm in (R.sequential_mm("forward"), R.sequential_mm("backward"), torch.matmul):
        got = R.run_chain(*case, mm=mm, dtype=torch.float32)
        assert torch.equal(got["y"].double(), want["y"]) and torch.equal(got["d_in"].double(), want["d_in"])
        for a, b in zip(got["dW"] + got["db"], want["dW"] + want["db"]):
            assert (a.double() - b).abs().max().item() <= 2e-4 * b.abs().max().item()
    # the rounding is at work: without it the networks compute something else
    plain = R.run_chain(*case, mm=lambda a, b: a @ b, dtype=torch.float64)
    import torch.nn.functional as F
    h = case[0].double()
    for i, (W, b) in enumerate(zip(case[1], case[2])):
        h = F.leaky_relu(F.linear(h, W.double(), b.double()), R.EXACT_SLOPE)
        if i in case[3] and i != len(case[1]) - 1:
            h = torch.cat([case[0].double(), h], dim=-1)
    assert not torch.equal(h, plain["y"])
