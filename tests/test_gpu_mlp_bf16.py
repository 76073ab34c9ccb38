"""The opt-in bf16 precision of the fused MLP chains on the GPU (csrc/mlp.hip: k_mlp_pack_bf16, k_mlp_chain_bf16), against
tests/mlp_bf16_reference.py (the semantics in plain PyTorch) and tests/golden/mlp_bf16_cases.npz (the reference's own GeneralMLP run
with a rounding linear op, float64):

* networks on which the semantics are exact arithmetic come out BIT-identical, outputs and dL/dinput;
* the six committed GeneralMLP cases stay within max(floor, rho * e_fmt) of the float64 emulation per tensor (relative L2), where
  e_fmt is what the number format itself costs on that tensor, rho = 4 x the largest share of e_fmt that float32 arithmetic
  around the same rounding costs (0.12, from the fixture) and floor the fp32 path's own tolerance (2e-5 outputs, 2e-4 gradients);
* the default stays fp32 to the bit, the switches select what they say, two bf16 runs are bit-identical, and SplatFields hands
  the precision to all of its networks."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

import mlp_bf16_reference as R
from mlp_bf16_reference import run_module

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
CASES = ["scale", "opacity", "rotation", "deform", "static_rgb", "no_features"]
FLOOR_OUT, FLOOR_GRAD = 2e-5, 2e-4


def test_device_packer_writes_the_documented_layout(hip_device):
    """sr_mlp_pack_bf16 against its PyTorch statement: a plain and a transposed job with padding in rows, input and hidden block"""
    from splatfields_amd import _lib
    from splatfields_amd.fused_mlp import pack_layer_weight_bf16
    lib = _lib.load()
    g = torch.Generator().manual_seed(3)
    M, n_mem, n_reg, mem_pad, reg_width, MT = 40, 21, 50, 32, 64, 3
    W = torch.randn(M, n_mem + n_reg, generator=g).to(hip_device)
    bias = torch.randn(M, generator=g).to(hip_device)
    count = 16 * MT * (mem_pad + reg_width)
    dst = torch.full((2, count), -1.0, dtype=torch.bfloat16, device=hip_device)
    bias_dst = torch.full((16 * MT,), -1.0, device=hip_device)
    Wt = W.t().contiguous()                                   # the second job reads the same matrix through `transposed`
    jobs = (_lib.SrMlpPackJob * 2)()
    for j, (src, ld, tr) in enumerate(((W, W.shape[1], 0), (Wt, Wt.shape[1], 1))):
        J = jobs[j]
        J.w, J.dst, J.ld, J.transposed, J.row0, J.n_rows = src.data_ptr(), dst[j].data_ptr(), ld, tr, 0, M
        J.n_mem, J.mem_pad, J.mem_col0, J.n_reg, J.reg_width, J.reg_col0, J.out_tiles = n_mem, mem_pad, 0, n_reg, reg_width, n_mem, MT
    jobs[0].bias_src, jobs[0].bias_dst, jobs[0].n_bias = bias.data_ptr(), bias_dst.data_ptr(), M
    _lib.check(lib.sr_mlp_pack_bf16(2, jobs, C.c_void_p(torch.cuda.current_stream(hip_device).cuda_stream)))
    want = pack_layer_weight_bf16(W.cpu(), n_mem, mem_pad, reg_width, MT)
    assert torch.equal(dst[0].cpu().view(torch.int16), want.view(torch.int16))
    assert torch.equal(dst[1].cpu().view(torch.int16), want.view(torch.int16))
    assert torch.equal(bias_dst[:M], bias) and (bias_dst[M:] == 0).all()


@pytest.fixture(scope="module")
def exact_references():
    """the restatement's float64 results of the exact networks, computed once"""
    return {(shape, n): R.run_chain(*R.exact_case(shape, n), dtype=torch.float64) for shape in R.EXACT_SHAPES for n in (77, 1)}


@pytest.mark.parametrize("shape", sorted(R.EXACT_SHAPES))
@pytest.mark.parametrize("n_points", [77, 1])
def test_exact_arithmetic_chains_are_bit_identical(hip_device, exact_references, shape, n_points):
    """hidden_tiles 8 and 4, memory + register tiles in one op, out_tiles < hidden_tiles, an output row of 3 floats, two full
    wavefronts + 13 points and a single point, every backward op kind.  y and dL/dh_in: bitwise; dW, db (fp32 sums over the
    points): within 2e-4 of each tensor's largest entry."""
    from splatfields_amd.fused_mlp import fused_general_mlp
    h_in, weights, biases, skips, dY = R.exact_case(shape, n_points)
    want = exact_references[(shape, n_points)]
    x = h_in.to(hip_device).requires_grad_()
    ws, bs = [w.to(hip_device).requires_grad_() for w in weights], [b.to(hip_device).requires_grad_() for b in biases]
    y = fused_general_mlp(x, ws, bs, skips=skips, negative_slope=R.EXACT_SLOPE, precision="bf16")
    y.backward(dY.to(hip_device))
    torch.cuda.synchronize()
    bad_y = int((y.detach().cpu().double() != want["y"]).sum()), int((x.grad.cpu().double() != want["d_in"]).sum())
    print(f"{shape} n={n_points}: entries of y / dL/dh_in that differ: {bad_y}")
    assert torch.equal(y.detach().cpu().double(), want["y"])
    assert torch.equal(x.grad.cpu().double(), want["d_in"])
    for got, ref in zip([w.grad for w in ws] + [b.grad for b in bs], want["dW"] + want["db"]):
        assert (got.cpu().double() - ref).abs().max().item() <= 2e-4 * ref.abs().max().item()


@pytest.mark.parametrize("name", CASES)
def test_fixture_cases_stay_within_the_format_error(hip_device, name):
    """per tensor || hip - emul64 || / || emul64 || <= max(floor, rho e_fmt); observed on MI355X: <= 1.2e-6, at most 0.0023 of the
    bound.  The distance to the reference itself is printed beside e_fmt (it IS e_fmt: the kernels add nothing to the format)."""
    kwargs, data, emul, e_fmt, rho = R.load_fixture_case(GOLDEN, name)
    assert rho < 0.5
    got = run_module(name, hip_device, "bf16", data, kwargs)
    assert set(got) == set(emul)
    ref32 = {"out": data["out"], "grad_xyz": data["grad_xyz"]}          # the reference itself (its float32 run: general_mlp_<name>.npz)
    if "feat" in data.files:
        ref32["grad_feat"] = data["grad_feat"]
    ref32.update({k: data[k] for k in data.files if k.startswith("grad:")})
    failed = []
    for k in sorted(got):
        want = torch.from_numpy(emul[k])
        ref = torch.from_numpy(ref32[k]).double()
        err = ((got[k] - want).norm() / want.norm().clamp_min(1e-300)).item()
        to_ref = ((got[k] - ref).norm() / ref.norm().clamp_min(1e-300)).item()
        bound = max(FLOOR_OUT if k == "out" else FLOOR_GRAD, rho * e_fmt[k])
        print(f"{name:12s} {k:26s} |hip - emul64| {err:.3e}  bound {bound:.3e}  ratio {err / bound:.3f}   |hip - ref| {to_ref:.3e}  e_fmt {e_fmt[k]:.3e}")
        if not err <= bound:
            failed.append((k, err, bound))
    assert not failed, failed


def test_default_is_unchanged_and_the_switches_select(hip_device):
    import splatfields_amd
    kwargs, data, _, _, _ = R.load_fixture_case(GOLDEN, "deform")
    start = splatfields_amd.mlp_precision()
    assert start == "fp32" or os.environ.get("SPLATFIELDS_MLP_PRECISION") == start
    try:
        assert splatfields_amd.set_mlp_precision("fp32") == start
        plain = run_module("deform", hip_device, "unset", data, kwargs)
        named = run_module("deform", hip_device, "fp32", data, kwargs)
        none = run_module("deform", hip_device, None, data, kwargs)
        bf = run_module("deform", hip_device, "bf16", data, kwargs)
        assert splatfields_amd.set_mlp_precision("bf16") == "fp32"
        by_default = run_module("deform", hip_device, "unset", data, kwargs)          # no argument: the process default, now bf16
        overridden = run_module("deform", hip_device, "fp32", data, kwargs)           # precision= on the module wins
        assert splatfields_amd.set_mlp_precision("fp32") == "bf16"
    finally:
        splatfields_amd.set_mlp_precision(start)
    for k in plain:
        assert torch.equal(plain[k], named[k]) and torch.equal(plain[k], none[k]) and torch.equal(plain[k], overridden[k]), k
        assert torch.equal(bf[k], by_default[k]), k
    assert not torch.equal(plain["out"], bf["out"]) and not torch.equal(plain["grad_xyz"], bf["grad_xyz"])
    assert sum(not torch.equal(plain[k], bf[k]) for k in plain) >= len(plain) - 1
    # fp32 is still the fp32 of the committed fixture
    ref = torch.from_numpy(data["out"]).double()
    assert (plain["out"] - ref).abs().max().item() <= 2e-5 * ref.abs().max().item()


@pytest.mark.parametrize("name", ["deform", "scale"])
def test_bf16_runs_are_bit_identical(hip_device, name):
    kwargs, data, _, _, _ = R.load_fixture_case(GOLDEN, name)
    a, b = run_module(name, hip_device, "bf16", data, kwargs), run_module(name, hip_device, "bf16", data, kwargs)
    assert set(a) == set(b) and all(torch.equal(a[k], b[k]) for k in a)


def test_splatfields_runs_all_its_networks_in_bf16(hip_device):
    from splatfields_amd.deform_field import SplatFields
    from splatfields_amd.general_mlp import GeneralMLP
    from test_deform_field import case_config
    data = np.load(os.path.join(GOLDEN, "splatfields_dynamic_se3.npz"))
    n_frames, kwargs, _ = case_config("dynamic_se3")
    state = {k[len("param:"):]: torch.from_numpy(data[k]) for k in data.files if k.startswith("param:")}
    results = {}
    for precision in ("fp32", "bf16"):
        net = SplatFields(radius=None, n_frames=n_frames, mlp_precision=precision, **kwargs)
        net.load_state_dict(state, strict=True)
        net = net.to(hip_device)
        inner = [m for m in net.modules() if isinstance(m, GeneralMLP)]
        assert len(inner) == 6 and all(m.precision == precision for m in inner)
        xyz = torch.from_numpy(data["xyz"]).to(hip_device).requires_grad_()
        out = net(xyz, torch.from_numpy(data["t"]).to(hip_device))
        out = {k: v for k, v in out.items() if v is not None}
        sum((v * torch.from_numpy(data["probe:" + k]).to(hip_device)).sum() for k, v in out.items()).backward()
        grads = {k: p.grad for k, p in net.named_parameters()}
        assert all(g is not None for g in grads.values())
        results[precision] = ({k: v.detach().cpu() for k, v in out.items()}, dict(grads, xyz=xyz.grad))
    (out32, g32), (out16, g16) = results["fp32"], results["bf16"]
    assert set(out32) == set(out16) and set(g32) == set(g16)
    for k in out32:
        assert out16[k].shape == out32[k].shape and torch.isfinite(out16[k]).all(), k
        err = ((out16[k] - out32[k]).norm() / out32[k].norm()).item()
        print(f"SplatFields {k:10s} |bf16 - fp32| / |fp32| = {err:.3e}")
        assert err <= 5e-2, (k, err)                       # sanity only: a layout error gives O(1), the format costs <= 5e-3 on outputs
    assert any(not torch.equal(out16[k], out32[k]) for k in out32)
    for k in g32:
        assert g16[k].shape == g32[k].shape and torch.isfinite(g16[k]).all(), k
