"""Every kernel path of the tri-plane lookup (splatfields_amd/triplane.py, csrc/triplane.hip) on the MI355X against the plain
float64 restatement tests/triplane_reference.py (pinned to the reference's own class by tests/test_triplane_reference.py), or
against exact arithmetic.

Tolerance of the parity cases: per tensor, d = max |ours - float64| may be 4 r, r = max |the reference's own float32 evaluation -
its float64 evaluation| on the same inputs: the kernels are another float32 evaluation of the same formulas.  dL/dpts is
discontinuous where a pixel coordinate crosses an integer; the points within S 2^-20 of such a crossing
(triplane_reference.fragile_points, at most 1 % of a case, enforced on the CPU) are left out of d and r for dL/dpts only and must
merely be finite.  Values and the plane gradient are never exempted.  All shapes are small: what they reach is listed in
triplane_reference.CASES.

Every case prints its d / (4 r) per tensor (run with -s)."""
import pytest
import torch

from tests import triplane_reference as R
from tests.accuracy import same_bits

pytestmark = pytest.mark.gpu


def hip_lookup(dev, planes, pts, g, planes_grad=True, pts_grad=True):
    """out, d_planes, d_pts (on the CPU; None where no gradient was asked for) of triplane_lookup for the upstream gradient g
    (g = probe: the loss sum(out * probe))."""
    from splatfields_amd.triplane import triplane_lookup
    p = planes.to(dev).requires_grad_(planes_grad)
    x = pts.to(dev).requires_grad_(pts_grad)
    out = triplane_lookup(p, x)
    assert tuple(out.shape) == (pts.shape[0], 3 * planes.shape[1])
    if planes_grad or pts_grad:
        out.backward(g.to(dev))
    cpu = lambda t: None if t is None else t.detach().cpu()
    return {"out": cpu(out), "d_planes": cpu(p.grad), "d_pts": cpu(x.grad)}


def assert_within(tag, got, ref64, r, fragile, tensors=R.TENSORS):
    """d <= 4 r per tensor (dL/dpts over the non-fragile points; finite at the others)."""
    ratios = {}
    for k in tensors:
        assert got[k].shape == ref64[k].shape and got[k].dtype == torch.float32, (tag, k)
        diff = (got[k].double() - ref64[k]).abs()
        if k == "d_pts":
            assert torch.isfinite(got[k]).all(), (tag, "dL/dpts is not finite")
            diff = diff[~fragile]
        assert torch.isfinite(diff).all(), (tag, k)
        ratios[k] = (diff.max().item(), 4.0 * r[k])
    print(f"[triplane] {tag}: " + "  ".join(f"{k} d {d:.3e} / 4r {b:.3e} = {d / b:.3f}" for k, (d, b) in ratios.items()))
    for k, (d, b) in ratios.items():
        assert d <= b, (tag, k, d, b)


# ---- parity table ----

@pytest.mark.parametrize("name", [c.name for c in R.CASES])
def test_every_kernel_path_against_the_float64_reference(hip_device, name):
    e = R.evaluated(name)
    got = hip_lookup(hip_device, e["planes"], e["pts"], e["probe"])
    again = hip_lookup(hip_device, e["planes"], e["pts"], e["probe"])
    assert same_bits(got, again, R.TENSORS), (name, "a second forward + backward differs")
    assert_within(name, got, e["f64"], e["r"], e["fragile"])


# ---- exactly representable coordinates ----

def test_texel_centres_borders_and_the_first_coordinate_outside_are_exact(hip_device):
    """C = 8, 16 x 16: every coordinate is a multiple of 1/16, every weight one of 0, 1/4, 1/2, 1, planes and probe hold small
    integers -- each intermediate is exact in float32 whatever the contraction, so values and the plane gradient must EQUAL the
    float64 reference.  These are the points where dL/dpts is not defined, so it only has to be finite -- except at the eight
    points with all three coordinates on a border (half-integer pixels), where it is defined, and exact as well."""
    C, S = 8, 16
    centres = [(2 * k + 1) / S - 1.0 for k in range(S)]                  # pixel coordinate k exactly: one corner with weight 1
    border = [-1.0, 1.0]                                                 # pixel -1/2 and S - 1/2: the outer corner is padding, weight 1/2
    outside = [-1.0 - 1.0 / S, 1.0 + 1.0 / S]                            # pixel -1 and S: nothing of the plane is left
    v = torch.tensor(centres + border + outside, dtype=torch.float32)
    assert torch.equal(v.double(), torch.tensor(centres + border + outside, dtype=torch.float64))
    pts = torch.cartesian_prod(v, v, v)                                  # every class on every plane, in every combination
    gen = torch.Generator().manual_seed(201)
    planes = torch.randint(-8, 9, (3, C, S, S), generator=gen).float()
    probe = torch.randint(-4, 5, (pts.shape[0], 3 * C), generator=gen).float()
    ref = R.lookup(planes, pts, probe, torch.float64)
    smooth = ~R.fragile_points(pts, S, S)                                # all three coordinates on a border: half-integer pixels
    assert int(smooth.sum()) == 8 and (pts[smooth].abs() == 1.0).all()
    corner = ref["out"][(pts == 1.0).all(1)].reshape(3, C)               # the point (1, 1, 1): a quarter of each plane's last texel
    assert torch.equal(corner, 0.25 * planes[:, :, S - 1, S - 1].double())
    assert not ref["out"][(pts.abs() > 1.0).all(1)].any()
    got = hip_lookup(hip_device, planes, pts, probe)
    assert torch.equal(got["out"], ref["out"].float()) and torch.equal(ref["out"].float().double(), ref["out"])
    assert torch.equal(got["d_planes"], ref["d_planes"].float()) and torch.equal(ref["d_planes"].float().double(), ref["d_planes"])
    assert torch.isfinite(got["d_pts"]).all()
    assert torch.equal(got["d_pts"][smooth], ref["d_pts"][smooth].float()) and ref["d_pts"][smooth].abs().max() > 0


# ---- the fixed-point contract of the plane gradient ----

FP_C, FP_S, FP_N = 4, 16, 4099
FP_TEXEL = (3, 7, 12)          # the texel along x, y, z: plane xy collects at [y = 7, x = 3], yz at [12, 7], zx at [3, 12]


def pile(dev, rows):
    """FP_N identical points on one texel centre per plane; rows [FP_N] -> the upstream gradient of every channel of that point.
    Returns dL/dplanes and, per plane, the [y, x] of the texel."""
    pts = torch.tensor([[(2 * k + 1) / FP_S - 1.0 for k in FP_TEXEL]], dtype=torch.float32).repeat(FP_N, 1)
    planes = torch.randn(3, FP_C, FP_S, FP_S, generator=torch.Generator().manual_seed(202))
    g = rows.to(torch.float32)[:, None].repeat(1, 3 * FP_C)
    assert torch.equal(g[:, 0].double(), rows.double())
    yx = [(FP_TEXEL[R.AXES[p][1]], FP_TEXEL[R.AXES[p][0]]) for p in range(3)]
    ref = R.lookup(planes, pts, g, torch.float64)["d_planes"]
    return hip_lookup(dev, planes, pts, g)["d_planes"], yx, ref


def one_texel(value: float, yx) -> torch.Tensor:
    want = torch.zeros(3, FP_C, FP_S, FP_S, dtype=torch.float64)
    for p, (y, x) in enumerate(yx):
        want[p, :, y, x] = value
    return want


def test_every_point_on_one_texel_does_not_overflow(hip_device):
    g = float(torch.nextafter(torch.tensor(2.0), torch.tensor(0.0)))     # the largest value below 2^1: 24 one-bits
    got, yx, ref = pile(hip_device, torch.full((FP_N,), g, dtype=torch.float64))
    want = one_texel(FP_N * g, yx)                                       # exact in float64: 4099 (2^24 - 1) 2^-23
    assert torch.equal(ref, want)
    assert torch.equal(got, want.float()), (got[0, 0, yx[0][0], yx[0][1]].item(), FP_N * g)


def test_a_tiny_contribution_survives_the_cancellation_of_large_ones(hip_device):
    """2049 points with +2^20, 2049 with -2^20, one with 2^-10, all on one texel: a float32 sum in any order that has 2^20 in it
    while the small term arrives loses it (2^-3 is the spacing there); the fixed-point unit is 2^-26."""
    unit = R.fixed_point_resolution(2.0 ** 20, FP_N)
    assert unit == 2.0 ** -26 and (2.0 ** -10 / unit).is_integer()
    rows = torch.full((FP_N,), 2.0 ** 20, dtype=torch.float64)
    rows[1::2] = -2.0 ** 20
    rows[FP_N // 2 + 1] = 2.0 ** -10
    assert int((rows > 1).sum()) == int((rows < -1).sum()) == 2049
    got, yx, ref = pile(hip_device, rows)
    want = one_texel(2.0 ** -10, yx)
    assert torch.equal(ref, want)
    assert torch.equal(got, want.float())


def test_zero_upstream_gradient_gives_exact_zeros(hip_device):
    e = R.evaluated("c12_20x28")
    got = hip_lookup(hip_device, e["planes"], e["pts"], torch.zeros_like(e["probe"]))
    assert torch.equal(got["out"], hip_lookup(hip_device, e["planes"], e["pts"], e["probe"])["out"])
    assert got["d_planes"].shape == e["planes"].shape and not got["d_planes"].any()
    assert got["d_pts"].shape == e["pts"].shape and not got["d_pts"].any()


def test_a_nan_upstream_entry_is_dropped_from_the_plane_gradient(hip_device):
    e = R.evaluated("c12_20x28")
    planes, pts, probe = e["planes"], e["pts"], e["probe"]
    n0 = int(torch.nonzero((pts.abs() < 0.9).all(1))[0])                 # a point with all 12 corners inside
    j0 = int(probe[n0].abs().argmax())
    assert 0.5 < probe[n0, j0].abs() < probe.abs().max()                  # not the entry the power-of-two scale is chosen from
    g_nan, g_zero = probe.clone(), probe.clone()
    g_nan[n0, j0], g_zero[n0, j0] = float("nan"), 0.0
    ref64, ref32 = R.lookup(planes, pts, g_zero, torch.float64), R.lookup(planes, pts, g_zero, torch.float32)
    assert (ref64["d_planes"] - e["f64"]["d_planes"]).abs().max() > 0.01  # the entry matters
    got = hip_lookup(hip_device, planes, pts, g_nan)
    own = hip_lookup(hip_device, planes, pts, g_zero)
    assert torch.isfinite(got["d_planes"]).all()
    assert_within("NaN upstream entry", got, ref64, R.own_error(ref32, ref64), e["fragile"], tensors=("out", "d_planes"))
    assert torch.equal(got["d_planes"], own["d_planes"])                  # same max |g|, same scale: the same integers are summed
    others = torch.arange(pts.shape[0]) != n0
    assert torch.equal(got["d_pts"][others], own["d_pts"][others])


# ---- non-finite points ----

def test_non_finite_points_sample_nothing_and_disturb_nobody(hip_device):
    """Run A: rows of NaN, +-inf, +-3e38 (infinite after the first multiplication), +-1e10 and a mixed row.  Run B: (5, 5, 5) in
    their place -- finite and outside every plane, and N, hence the fixed-point scale, is the same.  corners_of invalidates
    corners by comparisons that a NaN fails and converts a coordinate to an integer only inside [-1, S - 1]."""
    e = R.evaluated("c12_20x28")
    planes, probe = e["planes"], e["probe"]
    nan, inf = float("nan"), float("inf")
    bad = torch.tensor([[nan] * 3, [inf] * 3, [-inf] * 3, [3e38] * 3, [-3e38] * 3, [1e10] * 3, [-1e10] * 3, [nan, inf, -inf], [-inf, nan, 3e38]])
    rows = torch.tensor([0, 1, 63, 64, 255, 1000, 2048, 4097, 4098])
    pts_a, pts_b = e["pts"].clone(), e["pts"].clone()
    pts_a[rows], pts_b[rows] = bad, 5.0
    a = hip_lookup(hip_device, planes, pts_a, probe)
    b = hip_lookup(hip_device, planes, pts_b, probe)
    assert not a["out"][rows].any() and not b["out"][rows].any()
    assert torch.equal(a["d_planes"], b["d_planes"])
    others = torch.ones(pts_a.shape[0], dtype=torch.bool)
    others[rows] = False
    assert torch.equal(a["out"][others], b["out"][others]) and torch.equal(a["d_pts"][others], b["d_pts"][others])
    assert torch.isfinite(a["d_pts"][others]).all() and not b["d_pts"][rows].any()
    # and run B is what the reference computes for it
    ref64, ref32 = R.lookup(planes, pts_b, probe, torch.float64), R.lookup(planes, pts_b, probe, torch.float32)
    fragile = R.fragile_points(pts_b, planes.shape[2], planes.shape[3])
    assert_within("(5, 5, 5) in place of the non-finite rows", b, ref64, R.own_error(ref32, ref64, ~fragile), fragile)


# ---- the Python wrapper ----

def sampler_for(planes_leaf, fuse):
    from splatfields_amd.triplane import TriPlaneSampler
    return TriPlaneSampler(out_ch=planes_leaf.shape[1], fuse_mode=fuse, plane_source=lambda frame_id: planes_leaf)


@pytest.mark.parametrize("fuse", ["add", "mean"])
def test_fused_modes_sum_over_the_planes(hip_device, fuse):
    e = R.evaluated("c12_20x28", fuse)
    case = e["case"]
    p = e["planes"].to(hip_device).requires_grad_(True)
    x = e["pts"].to(hip_device).requires_grad_(True)
    enc = sampler_for(p, fuse)
    assert enc.out_dim == case.C
    out = enc(x[None])
    assert tuple(out.shape) == (1, case.N, case.C)
    (out * e["probe"].to(hip_device)[None]).sum().backward()
    got = {"out": out.detach().cpu()[0], "d_planes": p.grad.cpu(), "d_pts": x.grad.cpu()}
    assert_within(f"fuse_mode={fuse}", got, e["f64"], e["r"], e["fragile"])


def test_batched_non_contiguous_points(hip_device):
    e = R.evaluated("c12_20x28")
    case, dev = e["case"], hip_device
    n = 1000
    gen = torch.Generator().manual_seed(204)
    big = (torch.rand(2, n, 6, generator=gen) * 2.2 - 1.1).to(dev).requires_grad_(True)
    g = torch.randn(2, n, 3 * case.C, generator=gen).to(dev)
    view = big[..., 1::2]
    assert tuple(view.shape) == (2, n, 3) and not view.is_contiguous()
    p1 = e["planes"].to(dev).requires_grad_(True)
    out1 = sampler_for(p1, "cat")(view)
    assert tuple(out1.shape) == (2, n, 3 * case.C)
    out1.backward(g)
    p2 = e["planes"].to(dev).requires_grad_(True)
    x2 = view.detach().contiguous().requires_grad_(True)
    out2 = sampler_for(p2, "cat")(x2)
    out2.backward(g)
    assert torch.equal(out1, out2) and torch.equal(p1.grad, p2.grad)
    assert torch.equal(big.grad[..., 1::2], x2.grad) and not big.grad[..., 0::2].any() and x2.grad.abs().max() > 0
    # and the batch is the flat list of its points
    flat = hip_lookup(dev, e["planes"], x2.detach().reshape(-1, 3).cpu(), g.reshape(-1, 3 * case.C).cpu())
    assert torch.equal(out1.detach().cpu().reshape(-1, 3 * case.C), flat["out"]) and torch.equal(p1.grad.cpu(), flat["d_planes"])


@pytest.mark.parametrize("what,dtype", [("planes", torch.float64), ("planes", torch.float16), ("planes", torch.bfloat16), ("points", torch.float64)])
def test_other_dtypes_are_the_float32_call_cast(hip_device, what, dtype):
    """The output follows the planes' dtype, each gradient its input's; the values are those of the float32 call on the float32
    images of the inputs, cast."""
    from splatfields_amd.triplane import triplane_lookup
    e = R.evaluated("c12_20x28")
    dev = hip_device
    planes, pts = e["planes"], e["pts"]
    if what == "planes":
        planes = (planes.double() * (1.0 + 2.0 ** -30)).to(dtype)             # float64: not float32 numbers
        assert dtype != torch.float64 or not torch.equal(planes.float().double(), planes)
    else:
        pts = pts.double() * (1.0 + 2.0 ** -30)
        assert not torch.equal(pts.float().double(), pts)
    out_dtype = planes.dtype
    g = e["probe"].to(out_dtype)
    p = planes.to(dev).requires_grad_(True)
    x = pts.to(dev).requires_grad_(True)
    out = triplane_lookup(p, x)
    out.backward(g.to(dev))
    p32 = planes.float().to(dev).requires_grad_(True)
    x32 = pts.float().to(dev).requires_grad_(True)
    out32 = triplane_lookup(p32, x32)
    out32.backward(g.float().to(dev))
    assert out.dtype == out_dtype and p.grad.dtype == planes.dtype and x.grad.dtype == pts.dtype
    assert out32.dtype == p32.grad.dtype == x32.grad.dtype == torch.float32
    assert torch.equal(out, out32.to(out_dtype)) and out32.abs().max() > 1
    assert torch.equal(p.grad, p32.grad.to(planes.dtype)) and torch.equal(x.grad, x32.grad.to(pts.dtype))
    assert torch.isfinite(p.grad).all() and p32.grad.abs().max() > 1 and x32.grad.abs().max() > 1


def test_gradient_subsets_and_no_grad(hip_device):
    from splatfields_amd.triplane import triplane_lookup
    e = R.evaluated("c12_20x28")
    dev = hip_device
    both = hip_lookup(dev, e["planes"], e["pts"], e["probe"])
    only_planes = hip_lookup(dev, e["planes"], e["pts"], e["probe"], pts_grad=False)
    only_points = hip_lookup(dev, e["planes"], e["pts"], e["probe"], planes_grad=False)
    assert only_planes["d_pts"] is None and torch.equal(only_planes["d_planes"], both["d_planes"]) and torch.equal(only_planes["out"], both["out"])
    assert only_points["d_planes"] is None and torch.equal(only_points["d_pts"], both["d_pts"]) and torch.equal(only_points["out"], both["out"])
    p = e["planes"].to(dev).requires_grad_(True)
    x = e["pts"].to(dev).requires_grad_(True)
    with torch.no_grad():
        out = triplane_lookup(p, x)
    assert out.grad_fn is None and not out.requires_grad and torch.equal(out.cpu(), both["out"])
    plain = triplane_lookup(p.detach(), x.detach())                          # nothing requires grad: no graph either
    assert plain.grad_fn is None and torch.equal(plain.cpu(), both["out"])


def test_backward_without_points(hip_device):
    from splatfields_amd.triplane import triplane_lookup
    dev = hip_device
    for shape in ((3, 8, 5, 7), (3, 36, 17, 9)):
        p = torch.randn(*shape, device=dev).requires_grad_(True)
        x = torch.zeros(0, 3, device=dev, requires_grad=True)
        out = triplane_lookup(p, x)
        assert tuple(out.shape) == (0, 3 * shape[1])
        out.sum().backward()
        assert p.grad.shape == p.shape and not p.grad.any() and tuple(x.grad.shape) == (0, 3)


def test_more_than_128_channels(hip_device):
    """The forward and the gradient to the points take any multiple of 4; the plane gradient's LDS tile ends at 128 channels and
    says so from the host check."""
    from splatfields_amd.triplane import triplane_lookup
    dev = hip_device
    C, H, W, N = 132, 6, 7, 300
    gen = torch.Generator().manual_seed(205)
    planes, pts, probe = torch.randn(3, C, H, W, generator=gen), torch.rand(N, 3, generator=gen) * 2.2 - 1.1, torch.randn(N, 3 * C, generator=gen)
    ref64, ref32 = R.lookup(planes, pts, probe, torch.float64), R.lookup(planes, pts, probe, torch.float32)
    fragile = R.fragile_points(pts, H, W)
    assert fragile.double().mean() <= 0.01
    r = R.own_error(ref32, ref64, ~fragile)
    got = hip_lookup(dev, planes, pts, probe, planes_grad=False)
    assert_within("C = 132, points only", got, ref64, r, fragile, tensors=("out", "d_pts"))
    p = planes.to(dev).requires_grad_(True)
    out = triplane_lookup(p, pts.to(dev))
    assert torch.equal(out.detach().cpu(), got["out"])
    with pytest.raises(RuntimeError, match=r"sr_triplane_backward: channels must be .* 4\.\.128"):
        out.backward(probe.to(dev))
    assert p.grad is None
    torch.cuda.synchronize(dev)                                               # refused on the host: nothing was launched, nothing is pending
    assert same_bits(hip_lookup(dev, planes, pts, probe, planes_grad=False), got, ("out", "d_pts"))
