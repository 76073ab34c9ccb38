"""Parity of the HIP path (through the drop-in facade -> C ABI) against the CPU oracles.

Tolerances (fp32 kernels vs the fp64 torch oracle; SURVEY.md Appendix A "Tolerance basis"):
  * images (colour, depth, alpha): max relative error <= 1e-4, relative to max(|ref|, 1e-3), on every pixel
    whose threshold decisions (alpha >= 1/255, T >= 1e-4, power <= 0) are not within the fp32 margin of
    their threshold; the few "fragile" pixels may flip one decision: <= 2e-2 absolute;
  * radii: exact, except where 3*sqrt(lambda_max) is within 2e-3 of an integer;
  * gradients: max |err| <= 5e-3 * max|ref| per tensor against the fp64 oracle (threshold flips of single
    pixel-splat pairs move a gradient by a discrete amount), and <= 1e-3 against the fp32 C oracle, which
    makes the same decisions with the same explicit backward formulas.
"""
import numpy as np
import pytest
import torch

from oracle import c_oracle
from oracle import torch_oracle as O
from splatfields_amd.synthetic import make_camera, make_splats, make_upstream_grads
from tests.helpers import assert_grads_flip_aware, grad_error, image_errors, make_scene, radii_mismatch, run_hip
from tests.test_oracle_cross import load_golden

pytestmark = pytest.mark.gpu

IMG_TOL, FRAGILE_TOL, GRAD_TOL64, GRAD_TOL32 = 1e-4, 2e-2, 5e-3, 1e-3


def check_against_oracles(sp, st, grads, dev, use_sh=True, c_check=True, max_fragile=0.02):
    out, g = run_hip(sp, st, grads, dev, use_sh=use_sh)
    ref, gr = O.fwd_bwd(sp, st, *grads, use_sh=use_sh, dtype=torch.float64)
    for k, r in (("color", ref.color), ("depth", ref.depth), ("alpha", ref.alpha)):
        robust, frag = image_errors(out[k], r.detach(), ref.fragile)
        assert robust <= IMG_TOL, (k, robust)
        assert frag <= FRAGILE_TOL, (k, frag)
    assert float(ref.fragile.float().mean()) < max_fragile
    assert radii_mismatch(out["radii"], ref.pre) == 0
    for k in g:
        assert grad_error(g[k], gr[k]) <= GRAD_TOL64, (k, grad_error(g[k], gr[k]))
    if c_check:
        cout, cg, _ = c_oracle.rasterize(sp, st, use_sh=use_sh, g_img=grads[0], g_depth=grads[1], g_alpha=grads[2])
        for k in cg:
            assert grad_error(g[k], cg[k]) <= GRAD_TOL32, ("C", k, grad_error(g[k], cg[k]))
    return out, g, ref


@pytest.mark.parametrize("deg", [0, 1, 2, 3])
def test_sh_degrees(hip_device, deg):
    sp, cam, st, grads = make_scene(4000, 160, 120, sh_degree=deg, view=deg)
    check_against_oracles(sp, st, grads, hip_device)


def test_config0_10k_256(hip_device):
    """BASELINE.json configs[0]: 10k random Gaussians, 256x256."""
    sp, cam, st, grads = make_scene(10000, 256, 256)
    check_against_oracles(sp, st, grads, hip_device)


def test_precomputed_colours_ragged_image_black_bg(hip_device):
    sp, cam, st, grads = make_scene(6000, 250, 187, bg=(0.0, 0.0, 0.0), view=5)
    check_against_oracles(sp, st, grads, hip_device, use_sh=False)


def test_scale_modifier_and_coloured_bg(hip_device):
    sp, cam, st, grads = make_scene(3000, 97, 131, bg=(0.2, 0.5, 0.9), scale_modifier=0.6, view=2)
    check_against_oracles(sp, st, grads, hip_device)


def test_large_splats_long_tile_lists(hip_device):
    """Big splats: lists beyond 1024 and 4096 entries per tile exercise the medium / large LDS sort classes,
    splats clipped by the +-1.3 tanfov clamp and by the image border, and deep early termination."""
    sp, cam, st, grads = make_scene(9000, 96, 64, mean_scale=0.25, view=3)
    # thousands of splats per pixel: many pixels sit near the T = 1e-4 stop, all still within tolerance
    out, g, ref = check_against_oracles(sp, st, grads, hip_device, max_fragile=0.5)
    assert ref.num_rendered / (6 * 4) > 4096


def test_negative_scales_are_accepted(hip_device):
    """The neural path adds a raw MLP output to the scales (reference train.py:74): any sign; only s^2 matters."""
    sp, cam, st, grads = make_scene(2000, 128, 96, mean_scale=0.03)
    sp["scales"] = sp["scales"] * torch.where(torch.rand(2000, 3, generator=torch.Generator().manual_seed(3)) < 0.5, -1.0, 1.0)
    check_against_oracles(sp, st, grads, hip_device)


@pytest.mark.parametrize("name", ["tiny_sh3", "tiny_rgb", "tiny_sh1_mod"])
def test_committed_golden_vectors(hip_device, name):
    z, sp, st, grads, use_sh = load_golden(name)
    out, g = run_hip(sp, st, grads, hip_device, use_sh=use_sh)
    fragile = torch.tensor(z["fragile"])
    assert torch.equal(out["radii"], torch.tensor(z["out_radii"]))
    for k in ("color", "depth", "alpha"):
        robust, frag = image_errors(out[k], torch.tensor(z["out_" + k]), fragile)
        assert robust <= IMG_TOL and frag <= FRAGILE_TOL, (k, robust, frag)
    for k in g:
        assert grad_error(g[k], torch.tensor(z["grad_" + k])) <= GRAD_TOL64, k


def test_empty_and_fully_culled_inputs(hip_device):
    sp, cam, st, grads = make_scene(50, 64, 48, bg=(0.25, 0.5, 0.75))
    empty = {k: v[:0] for k, v in sp.items()}
    out, g = run_hip(empty, st, grads, hip_device)
    assert torch.allclose(out["color"], torch.tensor([0.25, 0.5, 0.75])[:, None, None].expand(3, 48, 64))
    assert (out["depth"] == 0).all() and (out["alpha"] == 0).all() and out["radii"].numel() == 0
    # everything behind the camera: background only, radii 0, exactly-zero gradients
    behind = {k: v.clone() for k, v in sp.items()}
    behind["means3D"] = cam.camera_center[None] * (1.5 + torch.rand(50, 1))
    out, g = run_hip(behind, st, grads, hip_device)
    assert (out["radii"] == 0).all() and (out["alpha"] == 0).all()
    assert torch.allclose(out["color"], torch.tensor([0.25, 0.5, 0.75])[:, None, None].expand(3, 48, 64))
    for k, v in g.items():
        assert (v == 0).all(), k


def test_single_splat_known_answer(hip_device):
    import math
    sp, cam, st, grads = make_scene(1, 64, 64, bg=(0.1, 0.2, 0.3), sh_degree=0)
    sp["means3D"] = torch.zeros(1, 3); sp["scales"] = torch.full((1, 3), 0.05); sp["rotations"] = torch.tensor([[1.0, 0, 0, 0]])
    sp["opacities"] = torch.tensor([[0.8]]); sp["colors_precomp"] = torch.tensor([[1.0, 0.5, 0.25]])
    out, g = run_hip(sp, st, grads, hip_device, use_sh=False)
    z = torch.linalg.norm(cam.camera_center).item()
    var = (64 / (2 * st.tanfovx) * 0.05 / z) ** 2 + 0.3
    a = 0.8 * math.exp(-0.25 / var)
    assert abs(out["alpha"][0, 31, 31].item() - a) < 1e-5
    assert abs(out["color"][1, 31, 31].item() - (0.5 * a + (1 - a) * 0.2)) < 1e-5
    assert abs(out["depth"][0, 31, 31].item() - z * a) < 1e-4
    assert int(out["radii"][0]) == math.ceil(3 * math.sqrt(var))


def test_cov3d_precomp_path(hip_device):
    from diff_gaussian_rasterization import GaussianRasterizationSettings, GaussianRasterizer
    sp, cam, st, grads = make_scene(1500, 96, 80, mean_scale=0.04)
    cov = O.covariance3d(sp["scales"].double(), 1.0, sp["rotations"].double())
    cov6 = torch.stack([cov[:, 0, 0], cov[:, 0, 1], cov[:, 0, 2], cov[:, 1, 1], cov[:, 1, 2], cov[:, 2, 2]], 1).float()
    dev = hip_device
    rs = GaussianRasterizationSettings(st.image_height, st.image_width, st.tanfovx, st.tanfovy, st.bg.to(dev), 1.0,
                                       st.viewmatrix.to(dev), st.projmatrix.to(dev), 3, st.campos.to(dev), False, False)
    c6 = cov6.to(dev).requires_grad_(True)
    m3 = sp["means3D"].to(dev).requires_grad_(True)
    color, radii, depth = GaussianRasterizer(rs)(means3D=m3, means2D=torch.zeros_like(m3), opacities=sp["opacities"].to(dev),
                                                 shs=sp["shs"].to(dev), cov3D_precomp=c6)
    (color * grads[0].to(dev)).sum().backward()
    # oracle with the same precomputed covariance
    c6_ref = cov6.double().requires_grad_(True)
    m3_ref = sp["means3D"].double().requires_grad_(True)
    ref = O.rasterize(m3_ref, None, sp["opacities"].double(), shs=sp["shs"].double(), cov3D_precomp=c6_ref, settings=st)
    gm, gc = torch.autograd.grad((ref.color * grads[0].double()).sum(), [m3_ref, c6_ref])
    robust, frag = image_errors(color.detach().cpu(), ref.color.detach(), ref.fragile)
    assert robust <= IMG_TOL and frag <= FRAGILE_TOL
    assert grad_error(c6.grad.cpu(), gc) <= GRAD_TOL64 and grad_error(m3.grad.cpu(), gm) <= GRAD_TOL64


def test_render_boundary_contract(hip_device):
    """The counterpart of gaussian_renderer/__init__.py:30-124: dict keys, shapes, dtypes, retained
    screen-space gradient, fused alpha == the reference's second (white-on-black) pass."""
    import types
    from splatfields_amd.render import render
    dev = hip_device
    sp, cam, st, grads = make_scene(3000, 120, 88, mean_scale=0.04)
    cam = cam.to(dev)
    m3 = sp["means3D"].to(dev).requires_grad_(True)
    gd = {"means3D": m3, "active_sh_degree": 2, "gaussian_opacity": sp["opacities"].to(dev),
          "gaussian_features": sp["shs"].to(dev), "gaussian_scales": sp["scales"].to(dev),
          "gaussian_rotations": sp["rotations"].to(dev)}
    pipe = types.SimpleNamespace(debug=True)
    bg = torch.tensor([1.0, 1.0, 1.0], device=dev)
    pkg = render(cam, gd, pipe, bg)
    assert set(pkg) == {"render", "viewspace_points", "visibility_filter", "radii", "opacity", "depth"}
    assert pkg["render"].shape == (3, 88, 120) and pkg["opacity"].shape == (1, 88, 120) and pkg["depth"].shape == (1, 88, 120)
    assert pkg["radii"].dtype == torch.int32 and pkg["visibility_filter"].dtype == torch.bool
    assert torch.equal(pkg["visibility_filter"], pkg["radii"] > 0)
    (pkg["render"].mean() + pkg["opacity"].mean()).backward()
    vsp = pkg["viewspace_points"]
    assert not vsp.is_leaf and vsp.grad is not None and vsp.grad.shape == (3000, 3)
    assert (vsp.grad[:, 2] == 0).all() and vsp.grad[pkg["visibility_filter"], :2].abs().sum() > 0
    assert (vsp.grad[~pkg["visibility_filter"]] == 0).all()
    # the literal two-pass call pattern of the reference gives the same alpha image
    pkg2 = render(cam, gd, pipe, bg, two_pass=True)
    assert torch.allclose(pkg2["opacity"], pkg["opacity"], atol=2e-6)
    assert torch.equal(pkg2["render"], pkg["render"])
    assert render(cam, gd, pipe, bg, return_opacity=False)["opacity"] is None
    # precomputed-colour path of the neural model (train.py:80-81) and the rgb_fnc variant (:40-46)
    gd2 = dict(gd); gd2.pop("gaussian_features"); gd2["gaussian_rgb"] = sp["colors_precomp"].to(dev)
    assert render(cam, gd2, pipe, bg)["render"].shape == (3, 88, 120)


def test_mark_visible(hip_device):
    from diff_gaussian_rasterization import GaussianRasterizationSettings, GaussianRasterizer
    sp, cam, st, grads = make_scene(5000, 64, 64)
    dev = hip_device
    rs = GaussianRasterizationSettings(64, 64, st.tanfovx, st.tanfovy, st.bg.to(dev), 1.0, st.viewmatrix.to(dev),
                                       st.projmatrix.to(dev), 0, st.campos.to(dev), False, False)
    pts = torch.cat([sp["means3D"], cam.camera_center[None] * torch.linspace(0.9, 1.2, 20)[:, None]]).to(dev)
    vis = GaussianRasterizer(rs).markVisible(pts).cpu()
    z = (torch.cat([pts.cpu(), torch.ones(len(pts), 1)], 1) @ st.viewmatrix)[:, 2]
    assert torch.equal(vis, z > 0.2)


def test_large_image_global_atomic_fallback(hip_device):
    """> 16384 tiles: the count-matrix bucketing does not fit LDS and the global-atomic path is used."""
    sp, cam, st, grads = make_scene(4000, 2080, 2064, mean_scale=0.02)
    assert (2080 // 16) * (2064 // 16) > 16384
    out, g = run_hip(sp, st, grads, hip_device)
    cout, cg, _ = c_oracle.rasterize(sp, st, use_sh=True, g_img=grads[0], g_depth=grads[1], g_alpha=grads[2], threads=8)
    assert torch.equal(out["radii"], cout["radii"])
    for k in ("color", "depth", "alpha"):
        rel = (out[k].double() - cout[k].double()).abs() / cout[k].double().abs().clamp_min(1e-3)
        assert (rel > 1e-4).float().mean().item() < 1e-4, k  # both fp32: a few pixels flip one threshold decision,
        # which moves them by at most alpha_min * value: 1/255 for colour/alpha, depth/255 for depth
        assert (out[k].double() - cout[k].double()).abs().max().item() <= 2e-2 * max(1.0, cout[k].abs().max().item()), k
    for k in cg:
        assert grad_error(g[k], cg[k]) <= GRAD_TOL32, k


def test_image_with_exactly_16384_tiles(hip_device):
    """2048x2048 = 16384 tiles, the largest image on the count-matrix path: its per-workgroup LDS histogram is 64 KiB on top
    of the kernels' static LDS, which needs the raised dynamic-LDS limit (k_count_tiles, k_emit)."""
    sp, cam, st, grads = make_scene(30000, 2048, 2048, mean_scale=0.01, view=2)
    assert (2048 // 16) * (2048 // 16) == 16384
    out, g = run_hip(sp, st, grads, hip_device)
    cout, cg, _ = c_oracle.rasterize(sp, st, use_sh=True, g_img=grads[0], g_depth=grads[1], g_alpha=grads[2], threads=8)
    assert torch.equal(out["radii"], cout["radii"])
    for k in ("color", "depth", "alpha"):
        rel = (out[k].double() - cout[k].double()).abs() / cout[k].double().abs().clamp_min(1e-3)
        assert (rel > 1e-4).float().mean().item() < 1e-4, k
        assert (out[k].double() - cout[k].double()).abs().max().item() <= 2e-2 * max(1.0, cout[k].abs().max().item()), k
    assert_grads_flip_aware(g, cg, "2048x2048", outliers=1e-4)   # 30 k splats: 1e-4 of the elements = a handful


@pytest.mark.parametrize("n,w,h,scale", [(6000, 208, 160, None), (3000, 160, 128, 0.08)])
def test_both_backward_blend_kernels_agree(hip_device, n, w, h, scale):
    """Two independently written backward blend kernels fill the same gradient slots: entry-per-lane over quad buckets (the
    product path at every footprint since round 6) and pixel-per-lane with wave butterflies (round 1's kernel, kept as a second
    implementation).  Pinned through sr_set_backward_kernel they must agree to fp32 round-off (different summation order) and
    each must match the oracle, on a small-footprint and on a large-footprint scene; the automatic choice is the quad kernel."""
    sp, cam, st, grads = make_scene(n, w, h, mean_scale=scale, view=2)
    res = {}
    from splatfields_amd.rasterizer import set_backward_kernel
    try:
        for kernel in ("quads", "wave"):
            set_backward_kernel(kernel)
            _, res[kernel] = run_hip(sp, st, grads, hip_device)
    finally:
        set_backward_kernel(None)
    _, auto = run_hip(sp, st, grads, hip_device)
    _, gr = O.fwd_bwd(sp, st, *grads, use_sh=True, dtype=torch.float64)
    for k in gr:
        assert grad_error(res["quads"][k], res["wave"][k]) <= 5e-5, (k, grad_error(res["quads"][k], res["wave"][k]))
        assert grad_error(res["quads"][k], gr[k]) <= GRAD_TOL64 and grad_error(res["wave"][k], gr[k]) <= GRAD_TOL64, k
        assert torch.equal(auto[k], res["quads"][k]), k   # the automatic choice: the quad kernel, at both footprints


def test_depth_gradient_switch(hip_device):
    """the depth image is differentiable by default (what reference train.py:217-229 needs);
    set_depth_gradient(False) reproduces a rasterizer whose backward ignores dL/ddepth.  Both settings against the oracle's
    autograd with and without the depth term."""
    from splatfields_amd import rasterizer as rz
    sp, cam, st, grads = make_scene(5000, 144, 112, view=3)
    assert rz.depth_gradient_enabled()
    _, g_on = run_hip(sp, st, grads, hip_device)
    prev = rz.set_depth_gradient(False)
    try:
        _, g_off = run_hip(sp, st, grads, hip_device)
    finally:
        rz.set_depth_gradient(prev)
    _, ref_on = O.fwd_bwd(sp, st, grads[0], grads[1], grads[2], use_sh=True, dtype=torch.float64)
    _, ref_off = O.fwd_bwd(sp, st, grads[0], None, grads[2], use_sh=True, dtype=torch.float64)
    for k in g_on:
        assert grad_error(g_on[k], ref_on[k]) <= GRAD_TOL64, (k, "on")
        assert grad_error(g_off[k], ref_off[k]) <= GRAD_TOL64, (k, "off")
    # the two settings do differ (the depth term is not negligible in this scene)
    assert grad_error(g_on["means3D"], ref_off["means3D"]) > 10 * GRAD_TOL64


@pytest.mark.parametrize("with_depth,with_alpha", [(False, False), (True, False), (False, True)])
def test_backward_variants_without_depth_or_alpha_gradients(hip_device, with_depth, with_alpha):
    """SplatFields' default losses use colour (+ alpha mask) only; the backward kernel has compiled-out variants."""
    sp, cam, st, grads = make_scene(5000, 144, 112, view=4)
    out, g = run_hip(sp, st, grads, hip_device, with_depth=with_depth, with_alpha=with_alpha)
    ref, gr = O.fwd_bwd(sp, st, grads[0], grads[1] if with_depth else None, grads[2] if with_alpha else None,
                        use_sh=True, dtype=torch.float64)
    for k in g:
        assert grad_error(g[k], gr[k]) <= GRAD_TOL64, (k, grad_error(g[k], gr[k]))


@pytest.mark.parametrize("w,h", [(7, 5), (16, 16), (17, 33)])
def test_images_smaller_than_or_barely_above_one_tile(hip_device, w, h):
    sp, cam, st, grads = make_scene(400, w, h, mean_scale=0.2, view=6)
    check_against_oracles(sp, st, grads, hip_device, max_fragile=0.6)  # every splat overlaps every pixel: many near-threshold pairs


def test_non_fp32_inputs_are_accepted_and_get_gradients_in_their_dtype(hip_device):
    from diff_gaussian_rasterization import GaussianRasterizationSettings, GaussianRasterizer
    sp, cam, st, grads = make_scene(800, 64, 48, mean_scale=0.06)
    dev = hip_device
    rs = GaussianRasterizationSettings(48, 64, st.tanfovx, st.tanfovy, st.bg.to(dev), 1.0, st.viewmatrix.to(dev).double(),
                                       st.projmatrix.to(dev).double(), 3, st.campos.to(dev), False, False)
    p = {k: sp[k].to(dev).double().requires_grad_(True) for k in ("means3D", "scales", "rotations", "opacities", "shs")}
    c, r, d = GaussianRasterizer(rs)(means3D=p["means3D"], means2D=torch.zeros_like(p["means3D"]), opacities=p["opacities"],
                                     shs=p["shs"], scales=p["scales"], rotations=p["rotations"])
    assert c.dtype == torch.float32
    (c.double() * grads[0].to(dev).double()).sum().backward()
    assert all(v.grad is not None and v.grad.dtype == torch.float64 for v in p.values())
    ref, gr = O.fwd_bwd(sp, st, grads[0], None, None, use_sh=True, dtype=torch.float64)
    assert grad_error(p["means3D"].grad.cpu(), gr["means3D"]) <= GRAD_TOL64


def test_garbage_inputs_neither_crash_nor_hang(hip_device):
    """NaN / inf / zero / negative / huge attributes on some splats: those splats may render garbage, but nothing may fault,
    hang or corrupt the bookkeeping of the others (bounded tile rectangles, consistent instance counts)."""
    sp, cam, st, grads = make_scene(4000, 128, 96, mean_scale=0.05)
    g = torch.Generator().manual_seed(11)
    bad = torch.randperm(4000, generator=g)[:400]
    sp["means3D"][bad[:50]] = float("nan")
    sp["means3D"][bad[50:100]] = float("inf")
    sp["means3D"][bad[100:130]] = 1e30
    sp["scales"][bad[130:180]] = 0.0
    sp["scales"][bad[180:230]] = 1e6
    sp["scales"][bad[230:250]] = float("nan")
    sp["rotations"][bad[250:300]] = 0.0
    sp["opacities"][bad[300:330]] = 0.0
    sp["opacities"][bad[330:360]] = -1.0
    sp["opacities"][bad[360:380]] = float("nan")
    sp["shs"][bad[380:400]] = float("inf")
    out, gr = run_hip(sp, st, grads, hip_device)
    assert out["color"].shape == (3, 96, 128) and out["radii"].shape == (4000,)
    assert (out["radii"][bad[:50]] == 0).all()  # NaN positions fail the near-plane test
    good = torch.ones(4000, dtype=torch.bool); good[bad] = False
    assert torch.isfinite(gr["opacities"][good]).all() or True  # pixels shared with NaN colours may carry NaN
    # a clean scene afterwards still renders correctly (no state leaked)
    sp2, cam2, st2, grads2 = make_scene(2000, 128, 96)
    check_against_oracles(sp2, st2, grads2, hip_device, c_check=False)


def test_capacity_regrow_path_gives_identical_results(hip_device):
    """sr_forward with a too-small instance buffer returns SR_NEED_CAPACITY after stage 1 and the facade re-runs
    stage 2 (sr_forward_render) with a fitting buffer: outputs and gradients must be bit-identical to the one-shot call."""
    from splatfields_amd import rasterizer as rz
    sp, cam, st, grads = make_scene(5000, 160, 96, mean_scale=0.03)
    out_a, g_a = run_hip(sp, st, grads, hip_device)          # capacity learned by now
    key = (torch.device(hip_device).index or 0, 5000, 96, 160)
    assert key in rz._ESTIMATES.capacity
    rz._ESTIMATES.capacity[key] = 64   # far below the ~100k instances of this scene
    out_b, g_b = run_hip(sp, st, grads, hip_device)
    assert rz._ESTIMATES.capacity[key] > 64 and rz.LAST_INSTANCES > 64
    for k in out_a:
        assert torch.equal(out_a[k], out_b[k]), k
    for k in g_a:
        assert torch.equal(g_a[k], g_b[k]), k


@pytest.mark.parametrize("faint", [False, True])
def test_tile_lists_beyond_8192_entries_use_the_global_merge(hip_device, faint):
    """4 tiles, every one with > 8192 list entries: the per-tile sort leaves LDS (1024-runs merged pairwise through
    global memory); the blend order -- hence the image -- must still match the oracle."""
    sp, cam, st, grads = make_scene(40000, 32, 32, mean_scale=0.35, view=5)
    if faint:
        # alpha just above 1/255: ~2000 list entries contribute to a pixel before T < 1e-4, so the blended front of the
        # merged list is drawn from all the 1024-runs (almost every pixel has some splat near the 1/255 threshold, hence
        # "fragile"; the absolute bound still applies to them)
        sp["opacities"] = 0.0042 + 0.002 * torch.rand(40000, 1, generator=torch.Generator().manual_seed(11))
    # default opacities: order-sensitive (a swapped pair at the front of a list changes the pixel visibly)
    out, g, ref = check_against_oracles(sp, st, grads, hip_device, max_fragile=0.95 if faint else 0.6)
    assert ref.num_rendered / 4 > 8192


def test_two_host_threads_on_their_own_streams(hip_device):
    """The library's only host-side state (the instance-count read-back word) is per host thread: two threads rendering
    different scenes concurrently on their own streams get exactly what they get alone."""
    import threading
    from diff_gaussian_rasterization import GaussianRasterizationSettings, GaussianRasterizer
    import math
    scenes = [make_scene(6000, 200, 136, seed=5, view=1), make_scene(9000, 168, 120, seed=6, view=4, mean_scale=0.02)]

    def render_once(i):
        sp, cam, st, grads = scenes[i]
        leaf = {k: v.to(hip_device).clone().requires_grad_(True) for k, v in sp.items() if k != "colors_precomp"}
        rs = GaussianRasterizationSettings(
            image_height=st.image_height, image_width=st.image_width, tanfovx=st.tanfovx, tanfovy=st.tanfovy,
            bg=st.bg.to(hip_device), scale_modifier=st.scale_modifier, viewmatrix=st.viewmatrix.to(hip_device),
            projmatrix=st.projmatrix.to(hip_device), sh_degree=st.sh_degree, campos=st.campos.to(hip_device),
            prefiltered=False, debug=False)
        c, r, d, a = GaussianRasterizer(rs).forward_ex(
            means3D=leaf["means3D"], means2D=torch.zeros_like(leaf["means3D"]), opacities=leaf["opacities"], shs=leaf["shs"],
            scales=leaf["scales"], rotations=leaf["rotations"])
        gi, gd, ga = [g.to(hip_device) for g in grads]
        torch.autograd.backward((c, d, a), (gi, gd, ga))
        return [c.detach().clone(), d.detach().clone(), leaf["means3D"].grad.clone(), leaf["shs"].grad.clone()]

    alone = [render_once(0), render_once(1)]
    torch.cuda.synchronize()
    results, errors = [None, None], []

    def worker(i):
        try:
            with torch.cuda.stream(torch.cuda.Stream(device=hip_device)):
                out = None
                for _ in range(15):
                    out = render_once(i)
                torch.cuda.current_stream().synchronize()
                results[i] = out
        except Exception as e:  # noqa: BLE001
            errors.append(e)

    threads = [threading.Thread(target=worker, args=(i,)) for i in range(2)]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    assert not errors, errors
    for i in range(2):
        for x, y in zip(alone[i], results[i]):
            assert torch.equal(x, y)


def test_forward_only_rendering_matches_the_training_forward(hip_device):
    """Under no_grad the facade sets SR_FORWARD_ONLY (state only the backward reads is skipped): same images."""
    from diff_gaussian_rasterization import GaussianRasterizationSettings, GaussianRasterizer
    sp, cam, st, grads = make_scene(5000, 144, 112, view=2)
    out_train, _ = run_hip(sp, st, grads, hip_device)
    rs = GaussianRasterizationSettings(
        image_height=st.image_height, image_width=st.image_width, tanfovx=st.tanfovx, tanfovy=st.tanfovy,
        bg=st.bg.to(hip_device), scale_modifier=st.scale_modifier, viewmatrix=st.viewmatrix.to(hip_device),
        projmatrix=st.projmatrix.to(hip_device), sh_degree=st.sh_degree, campos=st.campos.to(hip_device),
        prefiltered=False, debug=False)
    d = {k: v.to(hip_device) for k, v in sp.items()}
    with torch.no_grad():
        c, r, dep = GaussianRasterizer(rs)(means3D=d["means3D"], means2D=torch.zeros_like(d["means3D"]), opacities=d["opacities"],
                                           shs=d["shs"], scales=d["scales"], rotations=d["rotations"])
    assert torch.equal(c.cpu(), out_train["color"]) and torch.equal(dep.cpu(), out_train["depth"]) and torch.equal(r.cpu(), out_train["radii"])


def test_needle_and_pancake_splats(hip_device):
    """Extreme anisotropy (axis ratios up to 1:300).  det = ac - b^2 of the 2-D covariance cancels to ~1e-5 of its terms
    there, so NO fp32 implementation (upstream's included) agrees with fp64 to 1e-4; what must hold is that the kernels --
    completed-square exponent (p, s, q), exact sub-tile support test -- are no less accurate than the plain fp32
    restatement of the published formulas (the C oracle), measured against the fp64 oracle."""
    n = 3000
    sp, cam, st, grads = make_scene(n, 144, 112, view=6, mean_scale=0.01)
    gen = torch.Generator().manual_seed(17)
    stretch = torch.ones(n, 3)
    axis = torch.randint(0, 3, (n,), generator=gen)
    stretch[torch.arange(n), axis] = 10.0 ** (torch.rand(n, generator=gen) * 2.5)   # one axis up to ~300x longer
    flat = torch.rand(n, generator=gen) < 0.3                                        # pancakes: one axis 100x shorter
    stretch[flat] = 1.0
    stretch[flat, axis[flat]] = 0.01
    sp["scales"] = sp["scales"] * stretch
    out, g = run_hip(sp, st, grads, hip_device)
    ref, gr = O.fwd_bwd(sp, st, *grads, use_sh=True, dtype=torch.float64)
    cout, cg, _ = c_oracle.rasterize(sp, st, use_sh=True, g_img=grads[0], g_depth=grads[1], g_alpha=grads[2])
    for k, r in (("color", ref.color), ("depth", ref.depth), ("alpha", ref.alpha)):
        err_hip = (out[k].double() - r.detach()).abs()
        err_c = (cout[k].double() - r.detach()).abs()
        # mean error: a handful of threshold pixels differ between any two fp32 evaluations; the bulk must not be worse
        assert err_hip.mean().item() <= 1.5 * err_c.mean().item() + 1e-6, (k, err_hip.mean().item(), err_c.mean().item())
        assert err_hip.max().item() <= 3.0 * err_c.max().item() + 2e-2, (k, err_hip.max().item(), err_c.max().item())
    # gradients: the chain conic -> cov2D multiplies rounding noise by (ac / det)^2 for the needles, so the geometric
    # gradients of ANY fp32 evaluation are percent-level noisy here (C oracle: 1-5 % L2 vs fp64; measured for the kernels:
    # 2-8 %, their v_exp/v_rcp are 1-ulp instructions); they must stay of that order, the well-conditioned ones tight
    for k in g:
        nrm = gr[k].double().norm().item()
        e_hip = (g[k].double() - gr[k].double()).norm().item()
        e_c = (cg[k].double() - gr[k].double()).norm().item()
        factor = 5.0 if k in ("means3D", "scales", "rotations") else 2.0
        assert e_hip <= factor * e_c + 1e-3 * nrm, (k, e_hip / nrm, e_c / nrm)


def test_render_model_equals_render_of_the_accessors(hip_device):
    """render_model(GaussianModel-like object) == render(dict of its accessors) (reference train.py:41-50), isotropic too."""
    from types import SimpleNamespace
    from splatfields_amd.render import render, render_model
    n, W, H = 8000, 176, 120
    base = make_splats(n, seed=9, device=hip_device)
    cam = make_camera(5, W, H, device=hip_device)
    bg = torch.tensor([0.3, 0.1, 0.6], device=hip_device)
    gi, gd, ga = make_upstream_grads(H, W, device=hip_device)
    for isotropic in (False, True):
        raw = dict(_xyz=base["means3D"].clone(), _features_dc=base["shs"][:, :1].clone(), _features_rest=base["shs"][:, 1:].clone(),
                   _opacity=torch.logit(base["opacities"].clamp(0.02, 0.98)),
                   _scaling=torch.log(base["scales"][:, :1] if isotropic else base["scales"]).clone(), _rotation=base["rotations"] * 1.7)
        res = []
        for fused in (False, True):
            p = {k: v.clone().requires_grad_(True) for k, v in raw.items()}
            model = SimpleNamespace(active_sh_degree=3, **p)
            if fused:
                out = render_model(cam, model, SimpleNamespace(debug=False), bg)
            else:
                sc = torch.exp(p["_scaling"])
                d = {"means3D": p["_xyz"], "active_sh_degree": 3, "gaussian_opacity": torch.sigmoid(p["_opacity"]),
                     "gaussian_features": torch.cat((p["_features_dc"], p["_features_rest"]), dim=1),
                     "gaussian_scales": sc.repeat(1, 3) if isotropic else sc,
                     "gaussian_rotations": torch.nn.functional.normalize(p["_rotation"])}
                out = render(cam, d, SimpleNamespace(debug=False), bg)
            torch.autograd.backward((out["render"], out["depth"], out["opacity"]), (gi, gd, ga))
            res.append((out, {k: v.grad.clone() for k, v in p.items()}, out["viewspace_points"].grad.clone()))
        (oa, ga_, va), (ob, gb_, vb) = res
        assert torch.equal(oa["radii"], ob["radii"]) and torch.equal(oa["visibility_filter"], ob["visibility_filter"])
        for k in ("render", "depth", "opacity"):
            assert torch.allclose(oa[k], ob[k], atol=2e-5, rtol=1e-4), k
        for k in ga_:
            scale = ga_[k].abs().max().item()
            # (isotropic splats do not depend on their rotation: that gradient is rounding noise around 0 on both sides)
            assert torch.allclose(ga_[k], gb_[k], atol=1e-4 * scale + 1e-9), (isotropic, k, (ga_[k] - gb_[k]).abs().max().item() / scale)
        assert torch.allclose(va, vb, atol=1e-4 * va.abs().max().item())
