"""The stand-alone SH stage (splatfields_amd/sh.py -> sr_sh_forward, sr_sh_forward_views, sr_sh_backward; csrc/sh.hip,
csrc/sh_stage.h) on the MI355X against the float64 restatement tests/sh_reference.py, which tests/test_sh_reference.py pins to
the reference's own eval_sh.

Which case launches which kernel (K coefficients per splat, active degree deg):
    k_sh_forward<true>          K = 16 and deg >= 2                      ids K16-deg2-*, K16-deg3-*
    k_sh_forward<false>         every other (K, deg)                     ids K16-deg0/1-*, K1-*, K4-*, K9-*, K25-*
    k_sh_forward_views<true>    K = 16                                   ids K16-*
    k_sh_forward_views<false>   K != 16                                  ids K1-*, K4-*, K9-*, K25-*
    k_sh_backward<true>         K = 16 with d_shs                        ids K16-*
    k_sh_backward<false>        K != 16, or want_shs=False               ids K1-*, K4-*, K9-*, K25-*; test_want_shs_false
The LDS staging (stage_sh_in / stage_sh_out) meets a partial only workgroup at N = 1 and 255, a whole one at 256, a whole one
and a partial second at 257, and two whole ones and a partial third at 700.

The measure is the suite's rule (tests/accuracy.py), with r from the float32 restatement; for the fixture cases r is the
reference's own float32 run (tests/golden/sh_cases.npz).  Clamp decisions are exact: the inputs are built so that no float64
pre-clamp channel lies within 1e-4 of zero (asserted), and then the clamp byte and `keep` equal the restatement's bit for bit.

Worst d / (4 r) seen on the MI355X over every case of this module, per entry point and tensor:
    sr_sh_forward        colours 0.51 (K16-deg3-N257, fifth camera)
    sr_sh_forward_views  colours 0.46 (K25-deg3-N257, three cameras)
    sr_sh_backward       dL/dshs 0.51 (K25-deg3-N1), dL/dmeans 0.45 (K16-deg3-N256)
    sh_to_rgb            colours 0.45, dL/dshs 0.51, dL/dmeans 0.45 (the same kernels, one camera)"""
import os

import numpy as np
import pytest
import torch

from tests import accuracy
from tests import sh_reference as R

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "sh_cases.npz")
NAN = float("nan")

WORST = {}      # entry point -> the worst d / (4 r) so far in this run (printed with every case)

K_DEG = ((16, 0), (16, 1), (16, 2), (16, 3), (1, 0), (4, 1), (9, 2), (9, 1), (25, 3), (25, 1))
SIZES = (1, 255, 256, 257, 700)
VIEWS = (1, 3, 5)


def kd_ids(pairs):
    return [f"K{k}-deg{deg}" for k, deg in pairs]


def held(entry, tag, got, ref64, ref32):
    """the suite's rule on every tensor of ref64; keeps the worst ratio per entry point"""
    worst = accuracy.within("sh", f"{entry} {tag}", got, ref64, ref32, show=None)
    WORST[entry] = max(WORST.get(entry, 0.0), worst)
    print(f"[sh]    (worst of {entry} so far {WORST[entry]:.3f})")
    return worst


def camera_centres(v=5):
    from splatfields_amd.synthetic import make_camera
    return torch.stack([make_camera(i, 64, 64).camera_center for i in range(v)]).float().contiguous()


def settle(means, shs, campos, deg):
    """Moves the DC coefficient of every channel whose float64 pre-clamp value lies within 1e-4 of zero in any view, and asserts
    that none remains: a clamp decision then cannot hang on float32 rounding."""
    moved = 0
    for _ in range(8):
        pre = R.pre_clamp(means.double(), shs.double(), campos.double(), deg)
        near = torch.nonzero(pre.abs() < 1e-4)
        if near.numel() == 0:
            break
        for _, i, c in near.tolist():
            shs[i, 0, c] += 0.05 if pre[:, i, c].sum() >= 0 else -0.05
            moved += 1
    pre = R.pre_clamp(means.double(), shs.double(), campos.double(), deg)
    assert (pre.abs() >= 1e-4).all()
    return moved


_SCENES = {}


def scene(n, k, deg, seed=3):
    """float32 CPU inputs, made once per (n, k, deg) and never modified afterwards: means [n,3], shs [n,k,3] scaled so that about
    three channels in ten clamp, campos [5,3], probe [5,n,3] (dL/dcolour)."""
    key = (n, k, deg, seed)
    if key not in _SCENES:
        from splatfields_amd.synthetic import make_splats
        sp = make_splats(n, seed=seed + 7 * k, sh_coeffs=k)
        means, shs = sp["means3D"].contiguous(), (sp["shs"] * 3.0).contiguous()
        campos = camera_centres()
        moved = settle(means, shs, campos, deg)
        probe = torch.randn(5, n, 3, generator=torch.Generator().manual_seed(seed + n))
        pre = R.pre_clamp(means.double(), shs.double(), campos.double(), deg)
        if n >= 255:
            share = (pre < 0).double().mean().item()
            assert 0.2 <= share <= 0.4, share
            assert moved <= 0.002 * pre.numel()
        _SCENES[key] = (means, shs, campos, probe)
    return _SCENES[key]


def reference(means, shs, campos, probe, deg, dtype, scale=1.0):
    """The restatement in `dtype`; the backward gets the colour gradient masked with the float64 decisions (they are exact)."""
    m, s, c = means.to(dtype), shs.to(dtype), campos.to(dtype)
    pre, colors, _ = R.forward_views(m, s, c, deg)
    keep = R.pre_clamp(means.double(), shs.double(), campos.double(), deg) >= 0
    d_shs, d_means = R.backward(m, s, c, (probe * keep).to(dtype), deg, scale)
    return {"pre": pre, "colors": colors, "keep": keep, "d_shs": d_shs, "d_means": d_means}


def hip_backward(dev, means, shs, campos, dcol, deg, **kw):
    """-> (d_shs or None, d_means) with d_means overwritten into a NaN-filled tensor."""
    from splatfields_amd.sh import sh_backward
    d_means = torch.full((means.shape[0], 3), NAN, device=dev)
    d_shs = sh_backward(means.to(dev), shs.to(dev), campos.to(dev), dcol.to(dev), deg, means_grad=d_means, accumulate_means=False, **kw)
    return d_shs, d_means


# ---- every template and branch against the restatement ---------------------------------------------------------------------

@pytest.mark.parametrize("n", SIZES, ids=lambda n: f"N{n}")
@pytest.mark.parametrize("k,deg", K_DEG, ids=kd_ids(K_DEG))
def test_every_kernel_path_against_the_restatement(hip_device, k, deg, n):
    from splatfields_amd.sh import sh_forward, sh_forward_views, sh_to_rgb
    dev = hip_device
    means, shs, campos5, probe5 = scene(n, k, deg)
    name = f"K{k}-deg{deg}-N{n}"
    md, sd = means.to(dev), shs.to(dev)
    for v in VIEWS:
        campos, probe = campos5[:v].contiguous(), probe5[:v].contiguous()
        r64 = reference(means, shs, campos, probe, deg, torch.float64)
        r32 = reference(means, shs, campos, probe, deg, torch.float32)
        keep = r64["keep"]
        if v > 1 and deg > 0 and n >= 255:       # the clamp depends on the view: a splat clamped in one view and not in another
            assert (keep.any(0) & ~keep.all(0)).any()
        tag = f"{name}-V{v}"
        # sr_sh_forward, camera by camera
        for vi in range(v):
            colors, clamped = sh_forward(md, sd, campos[vi].to(dev), deg)
            assert colors.shape == (n, 3) and clamped.shape == (n,) and clamped.dtype == torch.uint8
            held("sh_forward", f"{tag} view {vi}", {"colors": colors}, {"colors": r64["colors"][vi]}, {"colors": r32["colors"][vi]})
            assert torch.equal(clamped.cpu(), R.clamp_bits(r64["pre"][vi])), (tag, vi)
            assert torch.equal(colors.cpu() == 0, ~keep[vi]), (tag, vi)
        # sr_sh_forward_views: with keep, without, and into a caller's buffer
        colors, got_keep = sh_forward_views(md, sd, campos.to(dev), deg)
        assert colors.shape == (v, n, 3) and got_keep.shape == (v, n, 3) and got_keep.dtype == torch.float32
        held("sh_forward_views", tag, {"colors": colors}, {"colors": r64["colors"]}, {"colors": r32["colors"]})
        assert torch.equal(got_keep.cpu(), keep.float()), tag
        bare, none = sh_forward_views(md, sd, campos.to(dev), deg, want_keep=False)
        assert none is None and torch.equal(bare, colors)
        buf = torch.full((v, n, 3), NAN, device=dev)
        into, keep2 = sh_forward_views(md, sd, campos.to(dev), deg, out=buf)
        assert into is buf and torch.equal(buf, colors) and torch.equal(keep2, got_keep)
        # sr_sh_backward
        dcol = probe * keep
        d_shs, d_means = hip_backward(dev, means, shs, campos, dcol, deg)
        assert d_shs.shape == (n, k, 3) and d_shs.dtype == torch.float32
        held("sh_backward", tag, {"d_shs": d_shs, "d_means": d_means}, {x: r64[x] for x in ("d_shs", "d_means")}, r32)
        assert (d_shs[:, (deg + 1) ** 2:] == 0).all()
    # sh_to_rgb end to end, first camera: the clamp mask is the forward's own
    m, s = md.clone().requires_grad_(True), sd.clone().requires_grad_(True)
    col = sh_to_rgb(m, s, campos5[0].to(dev), deg)
    (col * probe5[0].to(dev)).sum().backward()
    r64 = reference(means, shs, campos5[:1], probe5[:1], deg, torch.float64)
    r32 = reference(means, shs, campos5[:1], probe5[:1], deg, torch.float32)
    held("sh_to_rgb", name, {"colors": col, "d_shs": s.grad, "d_means": m.grad},
           {"colors": r64["colors"][0], "d_shs": r64["d_shs"], "d_means": r64["d_means"]},
           {"colors": r32["colors"][0], "d_shs": r32["d_shs"], "d_means": r32["d_means"]})


@pytest.mark.parametrize("deg", range(4))
def test_fixture_cases(hip_device, deg):
    """tests/golden/sh_cases.npz: r is the reference's own float32 run against its float64 run."""
    from splatfields_amd.sh import sh_forward, sh_forward_views
    dev = hip_device
    z = np.load(GOLDEN)
    g = {k: torch.from_numpy(z[k]) for k in z.files}
    means, shs, campos, probe = g["means"], g["shs"], g["campos"], g["probe"]
    want = {k: g[f"deg{deg}/f64/{k}"] for k in ("colors", "d_shs", "d_means")}
    ref32 = {k: g[f"deg{deg}/f32/{k}"] for k in ("colors", "d_shs", "d_means")}
    pre = R.pre_clamp(means.double(), shs.double(), campos.double(), deg)
    assert (pre.abs() > 1e-4).all()
    colors, keep = sh_forward_views(means.to(dev), shs.to(dev), campos.to(dev), deg)
    assert torch.equal(keep.cpu().bool(), pre >= 0) and torch.equal(keep.cpu().bool(), want["colors"] > 0)
    held("sh_forward_views", f"fixture deg{deg}", {"colors": colors}, {"colors": want["colors"]}, ref32)
    for vi in range(2):
        one, clamped = sh_forward(means.to(dev), shs.to(dev), campos[vi].to(dev), deg)
        held("sh_forward", f"fixture deg{deg} view {vi}", {"colors": one}, {"colors": want["colors"][vi]}, {"colors": ref32["colors"][vi]})
        assert torch.equal(clamped.cpu(), R.clamp_bits(pre[vi]))
    d_shs, d_means = hip_backward(dev, means, shs, campos, probe * keep.cpu(), deg)
    held("sh_backward", f"fixture deg{deg}", {"d_shs": d_shs, "d_means": d_means}, {k: want[k] for k in ("d_shs", "d_means")}, ref32)


# ---- the clamp boundary ------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("k", (1, 16), ids=lambda k: f"K{k}")
def test_the_clamp_boundary_is_the_references(hip_device, k):
    """Degree 0 is a one-term sum, the same with or without FMA contraction: dc = float32(-0.5) / float32(SH_C0) gives pre == 0.0
    exactly, its float32 neighbours -5.96e-8 and +2.98e-8 (tests/test_sh_reference.py).  The reference clamps where
    `result < 0`: zero itself is kept.  K = 16 takes k_sh_forward<false> (degree < 2) and k_sh_forward_views<true>."""
    from splatfields_amd.sh import sh_forward, sh_forward_views, sh_to_rgb
    dev = hip_device
    c0 = np.float32(R.C0)
    dc = np.float32(-0.5) / c0
    below, above = np.nextafter(dc, np.float32(-np.inf)), np.nextafter(dc, np.float32(np.inf))
    pre = [float(np.float32(c0 * x) + np.float32(0.5)) for x in (below, dc, above)]
    assert pre[1] == 0.0 and pre[0] < 0 < pre[2]
    shs = torch.zeros(3, k, 3)
    shs[:, 0, :] = torch.tensor([below, dc, above])[:, None]
    means, campos = torch.rand(3, 3, generator=torch.Generator().manual_seed(1)), torch.tensor([[3.0, 1.0, 2.0], [-2.0, 0.5, 1.0]])
    colors, clamped = sh_forward(means.to(dev), shs.to(dev), campos[0].to(dev), 0)
    assert colors.cpu()[:, 0].tolist() == [0.0, 0.0, pre[2]] and torch.equal(colors[:, :1].expand(3, 3), colors)
    assert clamped.cpu().tolist() == [7, 0, 0]
    views, keep = sh_forward_views(means.to(dev), shs.to(dev), campos.to(dev), 0)
    assert torch.equal(views[0], colors) and torch.equal(views[1], colors)
    assert keep.cpu()[:, :, 0].tolist() == [[0.0, 1.0, 1.0]] * 2 and torch.equal(keep[:, :, :1].expand(2, 3, 3), keep)
    s = shs.to(dev).requires_grad_(True)
    sh_to_rgb(means.to(dev), s, campos[0].to(dev), 0).sum().backward()           # the gradient passes at zero, stops below
    assert s.grad.cpu()[:, 0, 0].tolist() == [0.0, float(c0), float(c0)]


# ---- edge cases, each alone --------------------------------------------------------------------------------------------------

def run_all(dev, means, shs, campos, dcol, deg, **kw):
    """Every entry point once -> dict of device tensors."""
    from splatfields_amd.sh import sh_forward, sh_forward_views
    colors, clamped = sh_forward(means.to(dev), shs.to(dev), campos[0].to(dev), deg)
    views, keep = sh_forward_views(means.to(dev), shs.to(dev), campos.to(dev), deg)
    d_shs, d_means = hip_backward(dev, means, shs, campos, dcol, deg, **kw)
    return {"colors": colors, "clamped": clamped, "views": views, "keep": keep, "d_shs": d_shs, "d_means": d_means}


def masked_probe(means, shs, campos, probe, deg):
    return probe * (R.pre_clamp(means.double(), shs.double(), campos.double(), deg) >= 0)


@pytest.mark.parametrize("k,deg", ((16, 0), (16, 1), (16, 2), (9, 1), (25, 1), (25, 3), (4, 0)), ids=kd_ids(((16, 0), (16, 1), (16, 2), (9, 1), (25, 1), (25, 3), (4, 0))))
def test_unused_bands_are_never_read_and_get_exact_zeros(hip_device, k, deg):
    """Coefficient bands above the active degree hold NaN: nothing may depend on them, through the LDS staging (K = 16) or not,
    and their gradient rows are written as exact zeros -- also the rows k >= 16 at K = 25."""
    means, shs, campos5, probe5 = scene(300, k, deg)
    campos, nb = campos5[:3].contiguous(), (deg + 1) ** 2
    dcol = masked_probe(means, shs, campos, probe5[:3], deg)
    dirty = shs.clone()
    dirty[:, nb:] = NAN
    assert nb < k and torch.isnan(dirty).any()
    clean, got = run_all(hip_device, means, shs, campos, dcol, deg), run_all(hip_device, means, dirty, campos, dcol, deg)
    for name in clean:
        assert torch.isfinite(got[name].float()).all(), name
        assert torch.equal(got[name], clean[name]), name
    assert (got["d_shs"][:, nb:] == 0).all() and (got["d_shs"][:, :nb] != 0).any()


@pytest.mark.parametrize("k,deg", ((16, 3), (9, 2), (25, 3)), ids=kd_ids(((16, 3), (9, 2), (25, 3))))
def test_out_writes_a_row_range_and_nothing_else(hip_device, k, deg):
    """What the sliced exchange of the view-parallel step relies on: dL/dshs of rows [lo, hi) written into d_shs[lo:hi] of the
    whole cloud's gradient, lo and hi no multiples of the workgroup's 256 rows."""
    from splatfields_amd.sh import sh_backward
    dev = hip_device
    n, lo, hi, sentinel = 900, 130, 643, 12345.0
    means, shs, campos5, probe5 = scene(n, k, deg)
    campos = campos5[:2].contiguous()
    dcol = masked_probe(means, shs, campos, probe5[:2], deg)
    md, sd, cd, dd = means.to(dev), shs.to(dev), campos.to(dev), dcol.to(dev)
    plain = sh_backward(md[lo:hi], sd[lo:hi], cd, dd[:, lo:hi], deg)
    big = torch.full((n, k, 3), sentinel, device=dev)
    ret = sh_backward(md[lo:hi], sd[lo:hi], cd, dd[:, lo:hi], deg, out=big[lo:hi])
    assert ret.data_ptr() == big[lo:hi].data_ptr()
    assert (big[:lo] == sentinel).all() and (big[hi:] == sentinel).all()
    assert torch.equal(big[lo:hi], plain) and (plain != sentinel).all()
    whole = sh_backward(md, sd, cd, dd, deg)                  # a splat's row does not depend on where its range begins
    assert torch.equal(whole[lo:hi], plain)


@pytest.mark.parametrize("k,deg", ((16, 3), (16, 0), (9, 2)), ids=kd_ids(((16, 3), (16, 0), (9, 2))))
def test_accumulate_means_adds_or_overwrites(hip_device, k, deg):
    from splatfields_amd.sh import sh_backward
    dev = hip_device
    means, shs, campos5, probe5 = scene(257, k, deg)
    campos, probe = campos5[:3].contiguous(), probe5[:3].contiguous()
    r64 = reference(means, shs, campos, probe, deg, torch.float64)
    r32 = reference(means, shs, campos, probe, deg, torch.float32)
    dcol = probe * r64["keep"]
    args = (means.to(dev), shs.to(dev), campos.to(dev), dcol.to(dev), deg)
    prefill = torch.randn(257, 3, generator=torch.Generator().manual_seed(5))
    acc = prefill.to(dev)
    sh_backward(*args, means_grad=acc, accumulate_means=True)
    held("sh_backward", f"accumulate K{k}-deg{deg}", {"d_means": acc}, {"d_means": prefill.double() + r64["d_means"]},
           {"d_means": prefill + r32["d_means"]})
    over = torch.full((257, 3), NAN, device=dev)
    sh_backward(*args, means_grad=over, accumulate_means=False)
    held("sh_backward", f"overwrite K{k}-deg{deg}", {"d_means": over}, {"d_means": r64["d_means"]}, r32)
    if deg == 0:
        assert (over == 0).all() and torch.equal(acc.cpu(), prefill)
    default = prefill.to(dev)                                   # accumulate is the default
    sh_backward(*args, means_grad=default)
    assert torch.equal(default, acc)


@pytest.mark.parametrize("k", (16, 9), ids=lambda k: f"K{k}")
def test_want_shs_false(hip_device, k):
    """K = 16 without d_shs runs k_sh_backward<false>: the position gradient is the one of the staged kernel, bit for bit."""
    means, shs, campos5, probe5 = scene(257, k, 2)
    campos = campos5[:3].contiguous()
    dcol = masked_probe(means, shs, campos, probe5[:3], 2)
    d_shs, d_means = hip_backward(hip_device, means, shs, campos, dcol, 2)
    none, alone = hip_backward(hip_device, means, shs, campos, dcol, 2, want_shs=False)
    assert none is None and d_shs is not None and torch.equal(alone, d_means) and (d_means != 0).any()


@pytest.mark.parametrize("k,deg", ((16, 3), (25, 1)), ids=kd_ids(((16, 3), (25, 1))))
def test_scale_one_half_halves_exactly(hip_device, k, deg):
    means, shs, campos5, probe5 = scene(257, k, deg)
    campos = campos5[:3].contiguous()
    dcol = masked_probe(means, shs, campos, probe5[:3], deg)
    one, half = hip_backward(hip_device, means, shs, campos, dcol, deg), hip_backward(hip_device, means, shs, campos, dcol, deg, scale=0.5)
    for a, b in zip(half, one):
        assert torch.equal(a, 0.5 * b) and (b != 0).any()
    r64 = {k_: 0.5 * v for k_, v in reference(means, shs, campos, probe5[:3], deg, torch.float64).items() if k_ in ("d_shs", "d_means")}
    r32 = reference(means, shs, campos, probe5[:3], deg, torch.float32, scale=0.5)
    held("sh_backward", f"scale 0.5 K{k}-deg{deg}", {"d_shs": half[0], "d_means": half[1]}, r64, r32)


@pytest.mark.parametrize("k", (16, 4), ids=lambda k: f"K{k}")
def test_a_view_without_gradient_contributes_nothing(hip_device, k):
    """Three views of which the middle one has an all-zero colour gradient == the other two alone, bit for bit."""
    deg = 3 if k == 16 else 1
    means, shs, campos5, probe5 = scene(300, k, deg)
    campos = campos5[:3].contiguous()
    dcol = masked_probe(means, shs, campos, probe5[:3], deg)
    dcol[1] = 0.0
    three = hip_backward(hip_device, means, shs, campos, dcol, deg)
    two = hip_backward(hip_device, means, shs, campos[[0, 2]], dcol[[0, 2]], deg)
    assert torch.equal(three[0], two[0]) and torch.equal(three[1], two[1]) and (two[0] != 0).any() and (two[1] != 0).any()
    zero = hip_backward(hip_device, means, shs, campos, torch.zeros_like(dcol), deg)     # and no view at all: exact zeros
    assert (zero[0] == 0).all() and (zero[1] == 0).all()


@pytest.mark.parametrize("k", (16, 9), ids=lambda k: f"K{k}")
def test_a_splat_at_the_camera_centre_spoils_only_its_own_row(hip_device, k):
    """Its direction is 0/0: that row may be NaN, every other row is the one of the run without it -- through the LDS staging
    (K = 16), too."""
    deg, j = 2, 100
    means, shs, campos5, probe5 = scene(300, k, deg)
    campos = campos5[:2].contiguous()
    dcol = masked_probe(means, shs, campos, probe5[:2], deg)
    dcol[:, j] = 1.0
    moved = means.clone()
    moved[j] = campos[0]
    clean, got = run_all(hip_device, means, shs, campos, dcol, deg), run_all(hip_device, moved, shs, campos, dcol, deg)
    others = torch.arange(300) != j
    for name in ("colors", "clamped", "d_shs", "d_means"):
        assert torch.equal(got[name][others], clean[name][others]), name
    for name in ("views", "keep"):
        assert torch.equal(got[name][:, others], clean[name][:, others]), name
    assert torch.isfinite(got["views"][1]).all()                # the second camera sees the splat from a distance


def test_the_same_call_twice_is_bit_identical(hip_device):
    means, shs, campos5, probe5 = scene(700, 16, 3)
    dcol = masked_probe(means, shs, campos5, probe5, 3)
    first = run_all(hip_device, means, shs, campos5, dcol, 3)
    for _ in range(2):
        again = run_all(hip_device, means, shs, campos5, dcol, 3)
        assert all(torch.equal(again[name], first[name]) for name in first)


@pytest.mark.parametrize("k", (16, 9), ids=lambda k: f"K{k}")
def test_converted_inputs_equal_the_plain_call(hip_device, k):
    """float64 tensors (of float32 values) and non-contiguous views are converted, not reinterpreted."""
    dev, deg = hip_device, 2
    means, shs, campos5, probe5 = scene(257, k, deg)
    campos = campos5[:3].contiguous()
    dcol = masked_probe(means, shs, campos, probe5[:3], deg)
    plain = run_all(dev, means, shs, campos, dcol, deg)
    wide = run_all(dev, means.double(), shs.double(), campos.double(), dcol.double(), deg)
    strided = run_all(dev, torch.cat([means, means + 1], 1)[:, :3], shs.transpose(0, 1).contiguous().transpose(0, 1),
                      torch.cat([campos, campos], 1)[:, :3], dcol.permute(1, 0, 2).contiguous().permute(1, 0, 2), deg)
    for name in plain:
        assert torch.equal(wide[name], plain[name]) and wide[name].dtype == plain[name].dtype, name
        assert torch.equal(strided[name], plain[name]), name


def test_entry_points_refuse_mismatched_tensors(hip_device):
    """The shape and device checks of splatfields_amd/sh.py that need device tensors to get past the first guard.  Every call
    raises on the host: nothing is launched."""
    from splatfields_amd.sh import sh_backward, sh_forward, sh_forward_views
    dev = hip_device
    n, v = 10, 2
    means, shs, campos, dcol = (t.to(dev) for t in (torch.rand(n, 3), torch.rand(n, 16, 3), torch.rand(v, 3), torch.rand(v, n, 3)))
    for call in (sh_forward, sh_forward_views):
        with pytest.raises(RuntimeError, match="no CPU path"):
            call(means, shs.cpu(), campos, 3)
        with pytest.raises(RuntimeError, match="one row per splat"):
            call(means, shs[:5], campos, 3)
        with pytest.raises(RuntimeError, match=r"means3D must be \[N,3\]"):
            call(means.reshape(-1), shs, campos, 3)
    bad = dict(
        cpu_shs=(lambda: sh_backward(means, shs.cpu(), campos, dcol, 3), "no CPU path"),
        cpu_dcol=(lambda: sh_backward(means, shs, campos, dcol.cpu(), 3), "no CPU path"),
        short_shs=(lambda: sh_backward(means, shs[:5], campos, dcol, 3), "one row per splat"),
        flat_shs=(lambda: sh_backward(means, shs.reshape(n, 48), campos, dcol, 3), "one row per splat"),
        short_dcol=(lambda: sh_backward(means, shs, campos, dcol[:, :5], 3), r"dcolors_views must be \[V,N,3\]"),
        one_view_short=(lambda: sh_backward(means, shs, campos, dcol[:1], 3), r"dcolors_views must be \[V,N,3\]"),
        short_means_grad=(lambda: sh_backward(means, shs, campos, dcol, 3, means_grad=torch.zeros(5, 3, device=dev)), "means_grad must be"),
        flat_means_grad=(lambda: sh_backward(means, shs, campos, dcol, 3, means_grad=torch.zeros(3 * n, device=dev)), "means_grad must be"),
        cpu_means_grad=(lambda: sh_backward(means, shs, campos, dcol, 3, means_grad=torch.zeros(n, 3)), "means_grad must be"),
        f64_means_grad=(lambda: sh_backward(means, shs, campos, dcol, 3, means_grad=torch.zeros(n, 3, device=dev, dtype=torch.float64)),
                        "means_grad must be"),
        cpu_out=(lambda: sh_backward(means, shs, campos, dcol, 3, out=torch.zeros(n, 16, 3)), "out must be"),
        short_out=(lambda: sh_backward(means, shs, campos, dcol, 3, out=torch.zeros(5, 16, 3, device=dev)), "out must be"),
        strided_out=(lambda: sh_backward(means, shs, campos, dcol, 3, out=torch.zeros(n, 32, 3, device=dev)[:, ::2]), "out must be"),
        too_few_coefficients=(lambda: sh_backward(means, shs[:, :9].contiguous(), campos, dcol, 3), "bad arguments to sr_sh_backward"),
    )
    for name, (call, msg) in bad.items():
        with pytest.raises(RuntimeError, match=msg):
            call()
