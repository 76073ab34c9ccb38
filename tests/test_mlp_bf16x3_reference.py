"""tests/mlp_bf16x3_reference.py -- the plain-PyTorch statement of the split-bf16 ("bf16x3") precision of the fused MLP chains that
the GPU tests compare the HIP kernels with -- pinned on CPU: its split is torch's bfloat16 conversion applied twice, it reproduces
the reference's own GeneralMLP run with a splitting linear op (tests/golden/mlp_bf16x3_cases.npz, float64), the fixture shows what
the format buys over bf16, and the exact-arithmetic networks of `exact_case` are exact: float32 in two summation orders equals
float64 bit for bit, while any other choice of the four partial products computes something else."""
import os

import numpy as np
import pytest
import torch

import mlp_bf16x3_reference as R

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
CASES = ["scale", "opacity", "rotation", "deform", "static_rgb", "no_features"]
POINT_COUNTS = [131, 77, 1]


def test_split_is_two_bfloat16_conversions_and_keeps_sixteen_bits():
    g = torch.Generator().manual_seed(6)
    x = torch.cat([torch.randn(100000, generator=g) * 10.0 ** torch.randint(-6, 7, (100000,), generator=g).float(),
                   torch.tensor([0.0, -0.0, 1.0, 1.00390625, 1.001953125, -255.5, 2.0 ** -120])])
    hi, lo = R.split(x)
    want_hi = x.to(torch.bfloat16).float()
    want_lo = (x - want_hi).to(torch.bfloat16).float()
    assert torch.equal(hi, want_hi) and torch.equal(lo, want_lo)
    assert ((hi + lo - x).abs() <= 2.0 ** -16 * x.abs()).all()              # hi + lo: 16 significant bits (2^-17 but for ties)
    assert (lo != 0).float().mean() > 0.9
    hi64, lo64 = R.split(x.double())
    assert hi64.dtype == torch.float64 and torch.equal(hi64, hi.double()) and torch.equal(lo64, lo.double())
    # what is not finite has no low part (NaN); a finite value that bfloat16 rounds to infinity has the opposite infinity
    hi, lo = R.split(torch.tensor([float("inf"), -float("inf"), float("nan"), 3.4e38]))
    assert torch.isinf(hi[[0, 1, 3]]).all() and torch.isnan(hi[2]) and torch.isnan(lo[:3]).all() and lo[3] == -float("inf")


@pytest.mark.parametrize("name", CASES)
def test_restatement_reproduces_the_reference_with_a_splitting_linear(name):
    """float64, <= 1e-12 relative L2 per tensor; the `.weight` gradients travel as float32 (<= 2^-23), the `.matrix_t` gradients
    as the outer product of those with the frame's coefficients that they are (tests/golden/make_mlp_bf16x3_golden.py)."""
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


@pytest.mark.parametrize("name", CASES)
def test_fixture_shows_what_the_format_buys(name):
    """For every tensor with an e_fmt in mlp_bf16_cases.npz: e_fmt3 <= e_fmt / 64.  Per product bf16 loses 2 x 2^-8 and the split
    3 x 2^-16, a ratio of 1/170; the emulation gives >= 127 on every tensor, so 64 leaves a factor of two.  And the emulation
    alone, float64 and float32, stays inside the tolerances tests/test_general_mlp.py applies to the fp32 path."""
    import mlp_bf16_reference as B
    _, _, _, e_fmt, _ = B.load_fixture_case(GOLDEN, name)
    _, _, emul, e_fmt3, e_32 = R.load_fixture_case(GOLDEN, name)
    fx = np.load(os.path.join(GOLDEN, "mlp_bf16x3_cases.npz"))
    assert set(e_fmt3) == set(e_fmt) == set(e_32) == set(emul) and len(e_fmt) >= 8
    for k in sorted(e_fmt):
        assert e_fmt3[k] <= e_fmt[k] / 64, (k, e_fmt3[k], e_fmt[k])
        floor = 2e-5 if k == "out" else 2e-4
        assert float(fx[f"{name}/max3/{k}"]) <= floor and float(fx[f"{name}/max3_32/{k}"]) <= floor, k
    assert all(v.dtype.kind == "f" for v in (fx[k] for k in fx.files))         # numeric arrays only


@pytest.fixture(scope="module")
def exact_references():
    return {(shape, n): R.run_chain(*R.exact_case(shape, n), dtype=torch.float64) for shape in R.EXACT_SHAPES for n in POINT_COUNTS}


@pytest.mark.parametrize("shape", sorted(R.EXACT_SHAPES))
@pytest.mark.parametrize("n_points", POINT_COUNTS)
def test_exact_networks_are_exact_in_float32(exact_references, shape, n_points):
    """outputs and dL/dinput of the exact-arithmetic networks: float32 adding first-to-last, float32 adding last-to-first, torch's
    own order and float64 agree bit for bit (the weight gradients sum over the points and are only float32-accurate)."""
    case = R.exact_case(shape, n_points)
    want = exact_references[(shape, n_points)]
    assert (want["y"] != 0).double().mean() > 0.9 and (want["d_in"] != 0).double().mean() > 0.3      # nothing degenerate
    for mm in (R.sequential_mm("forward"), R.sequential_mm("backward"), torch.matmul):
        got = R.run_chain(*case, mm=mm, dtype=torch.float32)
        assert torch.equal(got["y"].double(), want["y"]) and torch.equal(got["d_in"].double(), want["d_in"])
        for a, b in zip(got["dW"] + got["db"], want["dW"] + want["db"]):
            assert (a.double() - b).abs().max().item() <= 2e-4 * b.abs().max().item()
    # both widths put low parts into every kind of operand
    h_in, weights, _, _, dY = case
    assert (R.split(h_in)[1] != 0).any() and (R.split(weights[0])[1] != 0).sum() == 2 * weights[0].shape[0]
    assert (R.split(dY)[1] != 0).any() or n_points == 1


@pytest.mark.parametrize("shape", sorted(R.EXACT_SHAPES))
@pytest.mark.parametrize("n_points", [131, 77])
def test_every_other_choice_of_partial_products_computes_something_else(exact_references, shape, n_points):
    """Dropping hi(W) . lo(x), dropping lo(W) . hi(x), dropping both (plain bf16) or adding lo . lo (the full product of the split
    operands) changes y AND dL/dh_in on these cases: a kernel that computes any of them cannot pass the bitwise GPU test."""
    case = R.exact_case(shape, n_points)
    want = exact_references[(shape, n_points)]
    for terms in (("hh", "lh"), ("hh", "hl"), ("hh",), ("hh", "hl", "lh", "ll")):
        other = R.run_chain(*case, dtype=torch.float64, terms=terms)
        changed = (other["y"] != want["y"]).double().mean().item(), (other["d_in"] != want["d_in"]).double().mean().item()
        assert changed[0] > 0.25 and changed[1] > 0.05, (terms, changed)
    import torch.nn.functional as F                       # ... and so does the unsplit float64 network
    h = case[0].double()
    for i, (W, b) in enumerate(zip(case[1], case[2])):
        h = F.leaky_relu(F.linear(h, W.double(), b.double()), R.EXACT_SLOPE)
        if i in case[3] and i != len(case[1]) - 1:
            h = torch.cat([case[0].double(), h], dim=-1)
    assert not torch.equal(h, want["y"])
