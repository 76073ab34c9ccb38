"""`render_views` / `rasterizer.rasterize_views` (sr_forward_prepare_views, sr_forward_render_views, sr_sum_views) against the loop
it replaces, `[render(cam, ...) for cam in cameras]` with one `backward()`:

  outputs    render / depth / opacity / radii / visibility_filter of every view: torch.equal;
  gradients  precomputed colours, shared [N,3] and per view [V,N,3]: the gradient of every input and viewspace_points.grad[v]
             torch.equal to the loop's, for sum(l) / V and for a stacked loss -- the view sum adds in autograd's order;
             SH input: images equal; dL/dshs (one sr_sh_backward over the views instead of V added tensors) and dL/dmeans3D by the
             suite's accuracy rule against the float64 torch oracle with the float32 loop as the other float32 evaluation; every
             other gradient torch.equal;
  shapes     40 x 56 images (3 x 4 tiles, partial tiles both ways), N = 1500, V = 1, 2, 5 and 17 (17 crosses the 16-view chunk of
             the sum), a camera that looks away (no instance at all), N = 0, and two sort scenes of tests/boundary_scenes.py whose
             longest lists have 2049 and 4097 entries: the figures handed to stage 2 must select the sort classes a waiting
             forward selects;
  behaviour  two calls and a repeated backward (retain_graph) are bit-identical; no_grad gives the grad-mode outputs; one host
             wait per call where the loop has V; library launches = the loop's + 1 (+ 1 sr_sh_backward on the SH path), launches
             of all kernels strictly fewer.
Every test fails without render_views."""
import ctypes as C
import math

import numpy as np
import pytest
import torch

from oracle import torch_oracle as O
from splatfields_amd import synthetic
from splatfields_amd.synthetic import make_camera, make_splats
from tests import accuracy, launches
from tests import boundary_scenes as B

pytestmark = pytest.mark.gpu

W, H, N = 56, 40, 1500
INPUTS = ["means3D", "opacities", "scales", "rotations"]


def looking_away(width, height):
    """make_camera's camera 3 turned round: it looks from its position away from the cloud, which lies behind it"""
    base = make_camera(3, width, height)
    pos = base.camera_center.double().numpy()
    w2c = np.float32(synthetic.world_to_view(pos, target=2.0 * pos))
    wvt = torch.tensor(w2c).transpose(0, 1)
    proj_t = torch.tensor(np.float32(synthetic.projection(synthetic.ZNEAR, synthetic.ZFAR, base.FoVx, base.FoVy))).transpose(0, 1)
    full = wvt.unsqueeze(0).bmm(proj_t.unsqueeze(0)).squeeze(0)
    return synthetic.SyntheticCamera(base.FoVx, base.FoVy, height, width, wvt, full, wvt.inverse()[3, :3])


def cameras(V, device, away=None):
    cams = [make_camera(v, W, H, elevation_deg=12.0 + 4.0 * v) for v in range(V)]
    if away is not None:
        cams[away] = looking_away(W, H)
    return [c.to(device) for c in cams]


def upstream(V, device, h=H, w=W, seed=7):
    """different random dL/dimage, dL/ddepth, dL/dalpha for every view"""
    g = torch.Generator().manual_seed(seed)
    return [tuple((torch.randn(c, h, w, generator=g) / (h * w)).to(device) for c in (3, 1, 1)) for _ in range(V)]


def backgrounds(V, device):
    return torch.rand(V, 3, generator=torch.Generator().manual_seed(3)).to(device)


def leaves(sp, device, V, colours):
    """fresh leaf tensors: the geometry, and `shared` colours [N,3], `per_view` colours [V,N,3] or `sh` coefficients"""
    out = {k: sp[k].detach().to(device).clone().requires_grad_(True) for k in INPUTS}
    if colours == "sh":
        out["colour"] = sp["shs"].detach().to(device).clone().requires_grad_(True)
    elif colours == "shared":
        out["colour"] = sp["colors_precomp"].detach().to(device).clone().requires_grad_(True)
    else:
        g = torch.Generator().manual_seed(11)
        out["colour"] = torch.rand(V, sp["means3D"].shape[0], 3, generator=g).to(device).requires_grad_(True)
    return out


def gaussian_dict(leaf, colours, v=None):
    d = dict(means3D=leaf["means3D"], active_sh_degree=3, gaussian_opacity=leaf["opacities"], gaussian_scales=leaf["scales"],
             gaussian_rotations=leaf["rotations"])
    if colours == "sh":
        d["gaussian_features"] = leaf["colour"]
    else:
        d["gaussian_rgb"] = leaf["colour"][v] if (colours == "per_view" and v is not None) else leaf["colour"]
    return d


def view_loss(pkg, up, v=None):
    pick = (lambda t: t) if v is None else (lambda t: t[v])
    return (pick(pkg["render"]) * up[0]).sum() + (pick(pkg["depth"]) * up[1]).sum() + (pick(pkg["opacity"]) * up[2]).sum()


def total_loss(losses, form):
    if form == "sum_over_V":
        return sum(losses) / len(losses)
    if form == "plain_sum":
        return sum(losses)
    return torch.stack(losses).mean()


def collect(leaf, pkgs_or_pkg, stacked):
    """outputs and gradients on the CPU, stacked over the views"""
    if stacked:
        p = pkgs_or_pkg
        out = {k: p[k].detach().cpu() for k in ("render", "depth", "opacity", "radii", "visibility_filter")}
        vsp = p["viewspace_points"].grad
    else:
        out = {k: torch.stack([p[k].detach() for p in pkgs_or_pkg]).cpu() for k in ("render", "depth", "opacity", "radii", "visibility_filter")}
        vsp = torch.stack([p["viewspace_points"].grad for p in pkgs_or_pkg])
    grads = {k: t.grad.detach().cpu() for k, t in leaf.items()}
    grads["viewspace_points"] = vsp.detach().cpu()
    return out, grads


def run_loop(sp, cams, bgs, ups, device, colours, form, backward=True, gather=True):
    from splatfields_amd import render
    leaf = leaves(sp, device, len(cams), colours)
    pkgs = [render(cam, gaussian_dict(leaf, colours, v), None, bgs[v]) for v, cam in enumerate(cams)]   # the INTEGRATION.md loop
    if not backward:
        return pkgs
    total_loss([view_loss(p, ups[v]) for v, p in enumerate(pkgs)], "stack_mean" if form == "stacked" else form).backward()
    return collect(leaf, pkgs, stacked=False) if gather else None


def run_views(sp, cams, bgs, ups, device, colours, form, backward=True, gather=True):
    from splatfields_amd import render_views
    leaf = leaves(sp, device, len(cams), colours)
    pkg = render_views(cams, gaussian_dict(leaf, colours), None, bgs)
    if not backward:
        return pkg
    if form == "stacked":   # one expression over the stacked tensors
        up = [torch.stack([u[i] for u in ups]) for i in range(3)]
        per_view = (pkg["render"] * up[0]).sum((1, 2, 3)) + (pkg["depth"] * up[1]).sum((1, 2, 3)) + (pkg["opacity"] * up[2]).sum((1, 2, 3))
        per_view.mean().backward()
    else:
        total_loss([view_loss(pkg, ups[v], v) for v in range(len(cams))], form).backward()
    return collect(leaf, pkg, stacked=True) if gather else None


@pytest.fixture(scope="module")
def scene():
    return make_splats(N, seed=4321, mean_scale=0.07)


def assert_same(a: dict, b: dict, tag, skip=()):
    for k in a:
        if k not in skip:
            assert a[k].shape == b[k].shape and torch.equal(a[k], b[k]), (tag, k, (a[k].double() - b[k].double()).abs().max().item())


@pytest.mark.parametrize("form", ["sum_over_V", "stacked"])
@pytest.mark.parametrize("colours", ["shared", "per_view"])
@pytest.mark.parametrize("V", [1, 2, 5, 17])
def test_precomputed_colours_outputs_and_every_gradient_have_the_bits_of_the_loop(hip_device, scene, V, colours, form):
    cams, bgs, ups = cameras(V, hip_device), backgrounds(V, hip_device), upstream(V, hip_device)
    out_l, g_l = run_loop(scene, cams, bgs, ups, hip_device, colours, form)
    out_v, g_v = run_views(scene, cams, bgs, ups, hip_device, colours, form)
    assert out_v["render"].shape == (V, 3, H, W) and out_v["depth"].shape == out_v["opacity"].shape == (V, 1, H, W)
    assert out_v["radii"].shape == (V, N) and out_v["radii"].dtype == torch.int32 and out_v["visibility_filter"].dtype == torch.bool
    assert int((out_v["radii"] > 0).sum()) > V * N // 2 and torch.isfinite(out_v["render"]).all()      # the views show the cloud
    assert_same(out_l, out_v, ("outputs", V, colours, form))
    assert set(g_v) == set(INPUTS) | {"colour", "viewspace_points"} and g_v["viewspace_points"].shape == (V, N, 3)
    assert all(float(g.abs().max()) > 0 for g in g_v.values())
    assert_same(g_l, g_v, ("gradients", V, colours, form))


def test_one_shared_background_and_a_camera_that_looks_away(hip_device, scene):
    V = 5
    cams, ups = cameras(V, hip_device, away=2), upstream(V, hip_device)
    bg = torch.tensor([0.2, 0.5, 0.9], device=hip_device)
    out_l, g_l = run_loop(scene, cams, [bg] * V, ups, hip_device, "shared", "sum_over_V")
    out_v, g_v = run_views(scene, cams, bg, ups, hip_device, "shared", "sum_over_V")
    assert int((out_v["radii"][2] > 0).sum()) == 0 and float(out_v["opacity"][2].abs().max()) == 0.0     # no instance in that view
    assert torch.equal(out_v["render"][2], bg.cpu().reshape(3, 1, 1).expand(3, H, W))
    assert float(g_v["viewspace_points"][2].abs().max()) == 0.0 and float(g_v["viewspace_points"][1].abs().max()) > 0
    assert_same(out_l, out_v, "away outputs")
    assert_same(g_l, g_v, "away gradients")


def test_no_splats(hip_device, scene):
    V = 2
    empty = {k: v[:0] for k, v in scene.items()}
    cams, bgs, ups = cameras(V, hip_device), backgrounds(V, hip_device), upstream(V, hip_device)
    from splatfields_amd import render_views
    leaf = leaves(empty, hip_device, V, "shared")
    pkg = render_views(cams, gaussian_dict(leaf, "shared"), None, bgs)
    assert pkg["render"].shape == (V, 3, H, W) and pkg["radii"].shape == (V, 0) and pkg["viewspace_points"].shape == (V, 0, 3)
    assert torch.equal(pkg["render"], bgs.reshape(V, 3, 1, 1).expand(V, 3, H, W))
    assert float(pkg["depth"].detach().abs().max()) == 0.0 and float(pkg["opacity"].detach().abs().max()) == 0.0
    total_loss([view_loss(pkg, ups[v], v) for v in range(V)], "sum_over_V").backward()          # nothing to differentiate, nothing raised
    pkgs = run_loop(empty, cams, bgs, ups, hip_device, "shared", "sum_over_V", backward=False)
    for v in range(V):
        assert torch.equal(pkg["render"][v], pkgs[v]["render"])


@pytest.mark.parametrize("V", [1, 2, 3, 16, 17, 33])
def test_view_sum_alone_every_alignment_and_tail(hip_device, V):
    """sr_sum_views on its own: element counts around the 4-float slot and the 256-slot chunk, dst and src on every 4-byte
    offset of a 16-byte line (agreeing: vector body with an element-wise head and tail; disagreeing, or a stride that is no
    multiple of 4: element by element), all in one launch per 16 views; the bits of the descending fold, and not a float
    outside dst is written."""
    from splatfields_amd import _lib
    lib = _lib.load()
    g = torch.Generator().manual_seed(100 + V)
    cases = [(1, 0, 0, 1), (3, 1, 1, 4), (4, 2, 2, 8), (5, 3, 3, 8), (1023, 0, 0, 1024), (1024, 1, 3, 1024), (1025, 2, 2, 1028),
             (4501, 0, 0, 4504), (4501, 3, 3, 4504), (2049, 3, 1, 2051), (6000, 0, 0, 6000), (1027, 1, 1, 1029), (0, 0, 0, 0)]
    assert len(cases) <= _lib.SUM_MAX_JOBS                      # (elems, dst offset, src offset, view stride) in floats
    jobs, keep = [], []
    for elems, d_off, s_off, stride in cases:
        src = (torch.randn(V * stride + 8, generator=g) * 10.0 ** torch.randint(-3, 4, (V * stride + 8,), generator=g).float()).to(hip_device)
        dst = torch.full((elems + 16,), 777.0, device=hip_device)
        jobs.append(_lib.SrSumJob(dst.data_ptr() + 4 * (4 + d_off), src.data_ptr() + 4 * s_off, elems, stride))
        keep.append((elems, d_off, s_off, stride, src, dst))
    table = (_lib.SrSumJob * len(jobs))(*jobs)
    with torch.cuda.device(hip_device):
        _lib.check(lib.sr_sum_views(len(jobs), table, V, _lib.stream(hip_device)))
    torch.cuda.synchronize()
    for elems, d_off, s_off, stride, src, dst in keep:
        views = [src[s_off + v * stride:s_off + v * stride + elems] for v in range(V)]
        want = views[-1].clone() if elems else src[:0]
        for t in reversed(views[:-1]):
            want = want + t
        lo = 4 + d_off
        assert torch.equal(dst[lo:lo + elems], want), (V, elems, d_off, s_off, stride)
        assert bool((dst[:lo] == 777.0).all()) and bool((dst[lo + elems:] == 777.0).all()), (V, elems, d_off, "wrote outside dst")


def sort_counters(reset=False):
    from splatfields_amd import _lib
    out = (C.c_longlong * 4)()
    _lib.check(_lib.load().sr_debug_sort_counters(out, 1 if reset else 0))
    return list(out)


@pytest.mark.parametrize("name,classes", [("longest2049", [0, 0, 0, 0]), ("longest4097", [0, 1, 1, 0])])
def test_known_figures_select_the_sort_classes_of_a_waiting_forward(hip_device, name, classes):
    """longest2049: one tile beyond 2048 entries and nothing beyond 4096 -- the forward blend sorts it, no class is launched;
    longest4097: five tiles beyond 2048 and one beyond 4096 -- the 2049..4096 and the 4097..8192 class, once per view."""
    sc = B.sort_scene_by_name(name)
    w, h, V = sc.st.image_width, sc.st.image_height, 2
    cams = [make_camera(1, w, h).to(hip_device)] * V                 # the camera the scene was designed for
    bgs, ups = backgrounds(V, hip_device), upstream(V, hip_device, h, w)
    sp = {k: sc.sp[k] for k in INPUTS + ["colors_precomp", "shs"]}
    sort_counters(reset=True)
    out_l, g_l = run_loop(sp, cams, bgs, ups, hip_device, "shared", "sum_over_V")
    loop_classes = sort_counters(reset=True)
    out_v, g_v = run_views(sp, cams, bgs, ups, hip_device, "shared", "sum_over_V")
    views_classes = sort_counters(reset=True)
    assert views_classes == [V * c for c in classes], (name, views_classes)
    # the loop's first render of a size may run stage 2 twice (capacity); it launches no class the views do not
    assert all((a > 0) == (b > 0) for a, b in zip(loop_classes, views_classes)), (loop_classes, views_classes)
    assert torch.isfinite(out_v["render"]).all() and int((out_v["radii"] > 0).sum()) == V * sum(sc.lengths)
    assert_same(out_l, out_v, (name, "outputs"))
    assert_same(g_l, g_v, (name, "gradients"))


_oracle = {}


def oracle_sum(scene, cams_cpu, bgs, ups):
    """float64: the gradients of sum_v loss_v, from the torch oracle view by view"""
    if "sum" not in _oracle:
        total = None
        for v, cam in enumerate(cams_cpu):
            st = O.settings_from_camera(cam, bgs[v].cpu(), 3)
            _, g = O.fwd_bwd(scene, st, *[u.cpu() for u in ups[v]], use_sh=True)
            total = g if total is None else {k: total[k] + g[k] for k in g}
        _oracle["sum"] = total
    return _oracle["sum"]


def test_sh_input_images_equal_sh_and_position_gradients_within_the_accuracy_rule(hip_device, scene):
    V = 5
    cams, bgs, ups = cameras(V, hip_device), backgrounds(V, hip_device), upstream(V, hip_device)
    out_l, g_l = run_loop(scene, cams, bgs, ups, hip_device, "sh", "plain_sum")
    out_v, g_v = run_views(scene, cams, bgs, ups, hip_device, "sh", "plain_sum")
    assert_same(out_l, out_v, "sh outputs")
    assert g_v["colour"].shape == (N, 16, 3) and float(g_v["colour"][:, 1:].abs().max()) > 0
    assert_same(g_l, g_v, "sh gradients", skip=("colour", "means3D"))
    ref64 = oracle_sum(scene, [c.to("cpu") for c in cams], bgs, ups)
    names = {"colour": "shs", "means3D": "means3D"}
    accuracy.within("render_views", "SH degree 3, V = 5", {k: g_v[k] for k in names}, {k: ref64[n] for k, n in names.items()},
                    {k: g_l[k] for k in names}, show=None)


@pytest.mark.parametrize("colours", ["shared", "sh"])
def test_two_calls_and_a_repeated_backward_are_bit_identical(hip_device, scene, colours):
    from splatfields_amd import render_views
    V = 5
    cams, bgs, ups = cameras(V, hip_device), backgrounds(V, hip_device), upstream(V, hip_device)
    first = run_views(scene, cams, bgs, ups, hip_device, colours, "sum_over_V")
    second = run_views(scene, cams, bgs, ups, hip_device, colours, "sum_over_V")
    assert_same(first[0], second[0], "outputs of two calls")
    assert_same(first[1], second[1], "gradients of two calls")
    leaf = leaves(scene, hip_device, V, colours)
    pkg = render_views(cams, gaussian_dict(leaf, colours), None, bgs)
    loss = total_loss([view_loss(pkg, ups[v], v) for v in range(V)], "sum_over_V")
    wrt = list(leaf.values()) + [pkg["viewspace_points"]]
    once = torch.autograd.grad(loss, wrt, retain_graph=True)
    again = torch.autograd.grad(loss, wrt)
    for name, a, b, c in zip(list(leaf) + ["viewspace_points"], once, again, [first[1][k] for k in list(leaf) + ["viewspace_points"]]):
        assert torch.equal(a, b) and torch.equal(a.cpu(), c), name


def test_no_grad_gives_the_grad_mode_outputs(hip_device, scene):
    V = 5
    cams, bgs, ups = cameras(V, hip_device), backgrounds(V, hip_device), upstream(V, hip_device)
    for colours in ("shared", "sh"):
        with torch.no_grad():
            quiet = run_views(scene, cams, bgs, ups, hip_device, colours, None, backward=False)
        loud = run_views(scene, cams, bgs, ups, hip_device, colours, None, backward=False)
        assert not quiet["render"].requires_grad and loud["render"].requires_grad
        for k in ("render", "depth", "opacity", "radii", "visibility_filter"):
            assert torch.equal(quiet[k], loud[k]), (colours, k)


def test_set_depth_gradient_is_honoured(hip_device, scene):
    from splatfields_amd import rasterizer
    V = 2
    cams, bgs, ups = cameras(V, hip_device), backgrounds(V, hip_device), upstream(V, hip_device)
    with_depth = run_views(scene, cams, bgs, ups, hip_device, "shared", "sum_over_V")[1]
    prev = rasterizer.set_depth_gradient(False)
    try:
        loop = run_loop(scene, cams, bgs, ups, hip_device, "shared", "sum_over_V")[1]
        views = run_views(scene, cams, bgs, ups, hip_device, "shared", "sum_over_V")[1]
    finally:
        rasterizer.set_depth_gradient(prev)
    assert_same(loop, views, "without the depth gradient")
    assert not torch.equal(views["means3D"], with_depth["means3D"])


def test_one_host_wait_per_call(hip_device, scene):
    from splatfields_amd.rasterizer import host_sync_counters
    V = 5
    cams, bgs, ups = cameras(V, hip_device), backgrounds(V, hip_device), upstream(V, hip_device)
    run_loop(scene, cams, bgs, ups, hip_device, "shared", "sum_over_V")                      # the loop's capacities are learnt
    before = host_sync_counters()
    run_views(scene, cams, bgs, ups, hip_device, "shared", "sum_over_V")
    after_views = host_sync_counters()
    run_loop(scene, cams, bgs, ups, hip_device, "shared", "sum_over_V")
    after_loop = host_sync_counters()
    assert after_views["forward_host_waits"] - before["forward_host_waits"] == 1
    assert after_loop["forward_host_waits"] - after_views["forward_host_waits"] == V
    for k in ("async_forwards", "tickets_waited_for"):
        assert after_views[k] == before[k], k                                                 # no asynchronous launch, no ticket redeemed
    run_views(scene, cams, bgs, ups, hip_device, "shared", "sum_over_V")
    assert host_sync_counters()["tickets_created"] == after_views["tickets_created"] <= before["tickets_created"] + V   # blocks are reused


@pytest.mark.parametrize("colours,extra", [("shared", 1), ("per_view", 1), ("sh", 2)])
def test_launch_counts_against_the_warm_loop(hip_device, scene, colours, extra):
    """library launches: the loop's + the view sum (+ one sr_sh_backward on the SH path, whose per-view work the loop does inside
    the per-splat backward kernel it launches anyway); launches of all kernels: strictly fewer than the loop's"""
    V = 5
    cams, bgs, ups = cameras(V, hip_device), backgrounds(V, hip_device), upstream(V, hip_device)
    # forward, loss and backward only, and the loss as a training step forms it: per view in the loop, one expression over the
    # stacked tensors behind render_views
    loop = lambda: run_loop(scene, cams, bgs, ups, hip_device, colours, "stacked", gather=False)
    views = lambda: run_views(scene, cams, bgs, ups, hip_device, colours, "stacked", gather=False)
    loop(), loop(), views()                                                                   # warm: the loop's capacity estimates are learnt
    n_loop, n_views = launches.launches_per_iteration(loop, 1), launches.launches_per_iteration(views, 1)
    assert n_loop is not None and n_views is not None
    print(f"[render_views] launches {colours}: loop {n_loop}, render_views {n_views}")
    assert n_views["library"] == n_loop["library"] + extra, (n_loop, n_views)
    assert n_views["all"] < n_loop["all"], (n_loop, n_views)
