"""The fused view-dependent colour head (splatfields_amd/csrc/view_color.hip, `SplatFields(view_color="fused")`) on the MI355X against
the PyTorch-op path of the same object (`ViewColor`, path "torch") on the CPU, which tests/test_view_color_reference.py pins to the
reference's own network and render() expressions.

The measure is the suite's rule (tests/accuracy.py), with r from the float32 torch path on the CPU.  No element is left out:
points lie in [-1, 1]^3 and camera centres at radius >= 3, so the reference is finite everywhere (the one stated limit, a point
AT a camera centre, has its own test).  Tensors compared: the colours and the gradients of feature, means3D or dirs, weight and
bias.

Shapes: N = 1 (one lane), 63 / 64 / 65 (a wavefront's edge), 255 / 256 / 257 (the workgroup's edge: a workgroup is 256 points),
1000 (several workgroups); widths 4 (one vector), 36 (not a multiple of the 16 columns a pass moves), 64, 128 (the reference's)
and 256 (the limit); V = 1, 2, 5, 10, 16 (the limit of one launch) and 17 (two chunks on the Python side); both modes.  Weights
scaled by 1e-3, 1 and 8 take the sigmoid from linear to saturated; the upstream gradients span 30 binades."""
import copy
import os
import types

import pytest
import torch

from tests.accuracy import ulp32, within
from tests.launches import device_records

pytestmark = pytest.mark.gpu
NS = (1, 63, 64, 65, 255, 256, 257, 1000)
WIDTHS = (4, 36, 64, 128, 256)
VIEWS = (1, 2, 5, 10, 16, 17)
CAMERAS, DIRS = "cameras", "dirs"


def make_case(n, width, n_views, scale=1.0, seed=0, zero_view=None):
    """a head with random weights (times `scale`), features, points, camera centres, directions and upstream gradients, all
    float32 values on the CPU"""
    g = torch.Generator().manual_seed(100000 * seed + 97 * n + 7 * width + n_views)
    rn = lambda *s: torch.randn(*s, generator=g)
    head = torch.nn.Sequential(torch.nn.Linear(width + 3, 3), torch.nn.Sigmoid())
    with torch.no_grad():
        head[0].weight.copy_(rn(3, width + 3) * scale / width ** 0.5)
        head[0].bias.copy_(rn(3) * 0.5 * scale)
    probes = rn(n_views, n, 3) * torch.exp2(torch.randint(-15, 16, (n_views, n, 3), generator=g).float())      # 30 binades
    if zero_view is not None:
        probes[zero_view] = 0.0
    return {"head": head, "feature": rn(n, width), "means3D": torch.rand(n, 3, generator=g) * 2 - 1,
            "centres": torch.nn.functional.normalize(rn(n_views, 3), dim=-1) * (3.0 + torch.rand(n_views, 1, generator=g)),
            "dirs": torch.nn.functional.normalize(rn(n_views, n, 3), dim=-1), "probes": probes}


def run(case, mode, dtype, device, path, backward=True):
    """colours [V, N, 3] and every gradient of sum(probes . colours)"""
    from splatfields_amd.deform_field import ViewColor
    head = copy.deepcopy(case["head"]).to(dtype).to(device)
    leaf = lambda k: case[k].detach().to(dtype).to(device).clone().requires_grad_()
    feature = leaf("feature")
    fnc = ViewColor(head, feature, path)
    if mode == CAMERAS:
        pos = leaf("means3D")
        colours = fnc.for_cameras(pos, case["centres"].to(dtype).to(device))
    else:
        pos = leaf("dirs")
        if path == "fused":
            from splatfields_amd.view_color import fused_view_color
            colours = fused_view_color(feature, head[0].weight, head[0].bias, dirs=pos)
        else:
            colours = torch.stack([fnc(d) for d in pos])
    out = {"colours": colours.detach()}
    if backward:
        (colours * case["probes"].to(dtype).to(device)).sum().backward()
        out.update({"d_feature": feature.grad, "d_pos": pos.grad, "d_weight": head[0].weight.grad, "d_bias": head[0].bias.grad})
    return out


def check(tag, case, mode, dev):
    cpu = torch.device("cpu")
    r64, r32 = (run(case, mode, dt, cpu, "torch") for dt in (torch.float64, torch.float32))
    got = run(case, mode, torch.float32, dev, "fused")
    assert set(got) == set(r64) and got["colours"].dtype == torch.float32 and got["colours"].shape == r64["colours"].shape
    return within("view_color", f"{tag} {mode}", got, r64, r32)


@pytest.mark.parametrize("mode", (CAMERAS, DIRS))
@pytest.mark.parametrize("width", WIDTHS)
def test_point_counts_widths_and_view_counts(hip_device, width, mode):
    worst = 0.0
    for n in NS:
        for v in VIEWS:
            worst = max(worst, check(f"N={n} F={width} V={v}", make_case(n, width, v, seed=1), mode, hip_device))
    print(f"[view_color] F={width} {mode}: worst d/4r over {len(NS) * len(VIEWS)} shapes {worst:.3f}")


@pytest.mark.parametrize("mode", (CAMERAS, DIRS))
@pytest.mark.parametrize("scale", (1e-3, 1.0, 8.0))
def test_weight_scales_from_a_linear_to_a_saturated_sigmoid(hip_device, scale, mode):
    case = make_case(257, 128, 5, scale=scale, seed=2)
    with torch.no_grad():
        z = torch.nn.functional.linear(torch.cat([case["feature"], case["dirs"][0]], -1), case["head"][0].weight, case["head"][0].bias)
    print(f"[view_color] scale {scale}: |z| up to {z.abs().max().item():.2e}")
    check(f"scale={scale}", case, mode, hip_device)


@pytest.mark.parametrize("mode", (CAMERAS, DIRS))
def test_a_view_whose_upstream_is_all_zeros(hip_device, mode):
    case = make_case(257, 36, 5, seed=3, zero_view=2)
    check("zero upstream in view 2", case, mode, hip_device)
    if mode == DIRS:
        got = run(case, mode, torch.float32, hip_device, "fused")
        assert torch.count_nonzero(got["d_pos"][2]).item() == 0 and torch.count_nonzero(got["d_pos"][1]).item() > 0


@pytest.mark.parametrize("mode", (CAMERAS, DIRS))
def test_two_identical_calls_are_bit_identical(hip_device, mode):
    for v in (10, 17):
        case = make_case(1000, 128, v, seed=4)
        a, b = (run(case, mode, torch.float32, hip_device, "fused") for _ in range(2))
        for k in a:
            assert torch.equal(a[k], b[k]), (mode, v, k)


def test_no_points_and_converted_inputs(hip_device):
    from splatfields_amd.view_color import fused_view_color
    dev = hip_device
    for mode in (CAMERAS, DIRS):
        got = run(make_case(0, 128, 3, seed=5), mode, torch.float32, dev, "fused")
        assert tuple(got["colours"].shape) == (3, 0, 3) and tuple(got["d_feature"].shape) == (0, 128)
        assert tuple(got["d_weight"].shape) == (3, 131) and torch.count_nonzero(got["d_weight"]).item() == 0 and torch.count_nonzero(got["d_bias"]).item() == 0
    case = make_case(65, 36, 2, seed=6)
    want = run(case, CAMERAS, torch.float32, dev, "fused")
    head = copy.deepcopy(case["head"]).to(dev)
    feature64 = case["feature"].double().to(dev).requires_grad_()
    colours = fused_view_color(feature64, head[0].weight, head[0].bias, means3D=case["means3D"].double().to(dev), camera_centers=case["centres"].double().to(dev))
    (colours * case["probes"].to(dev)).sum().backward()
    assert colours.dtype == torch.float32 and torch.equal(colours, want["colours"]) and feature64.grad.dtype == torch.float64
    assert torch.equal(feature64.grad.float(), want["d_feature"])
    with torch.autocast("cuda", dtype=torch.bfloat16):
        colours = fused_view_color(case["feature"].to(dev), head[0].weight, head[0].bias, means3D=case["means3D"].to(dev), camera_centers=case["centres"].to(dev))
    assert colours.dtype == torch.float32 and torch.equal(colours, want["colours"])
    with pytest.raises(ValueError, match="camera_centers"):
        fused_view_color(case["feature"].to(dev), head[0].weight, head[0].bias, means3D=case["means3D"].to(dev),
                         camera_centers=case["centres"].to(dev).requires_grad_())


def library_launches(fn):
    """device records of the head's kernels and of the weight-gradient kernels it calls while fn runs"""
    return [n for n in device_records(fn) if "k_view_color" in n or "k_mlp_weight_grad" in n]


@pytest.mark.parametrize("mode", (CAMERAS, DIRS))
@pytest.mark.parametrize("v", (1, 10, 16))
def test_launch_counts_are_exactly_the_budget(hip_device, v, mode):
    """a condition of the design: 1 library kernel forward and 3 backward (its own and sr_mlp_weight_grad's two) for up to 16 views"""
    from splatfields_amd.view_color import VIEW_COLOR_LAUNCHES, fused_view_color
    assert VIEW_COLOR_LAUNCHES == (1, 3)
    dev = hip_device
    case = make_case(1000, 128, v, seed=7)
    head = case["head"].to(dev)
    feature = case["feature"].to(dev).requires_grad_()
    pos = case["means3D" if mode == CAMERAS else "dirs"].to(dev).requires_grad_()
    centres, probes = case["centres"].to(dev), case["probes"].to(dev)
    held = {}

    def forward():
        kw = dict(means3D=pos, camera_centers=centres) if mode == CAMERAS else dict(dirs=pos)
        held["loss"] = (fused_view_color(feature, head[0].weight, head[0].bias, **kw) * probes).sum()

    forward()
    held["loss"].backward()            # warm up
    fwd = library_launches(forward)
    bwd = library_launches(lambda: held["loss"].backward())
    print(f"[view_color] launches V={v} {mode}: forward {fwd}, backward {bwd}")
    assert len(fwd) == 1 and "k_view_color_forward" in fwd[0], fwd
    assert len(bwd) == 3 and sum("k_view_color_backward" in n for n in bwd) == 1 and sum("k_mlp_weight_grad" in n for n in bwd) == 2, bwd


def test_a_point_at_a_camera_centre_is_non_finite_in_that_view_only(hip_device):
    """the one stated limit, forward only: 0 / 0 in the direction, as in the reference"""
    case = make_case(300, 36, 3, seed=8)
    case["means3D"][:] = case["means3D"] * 0.2 + case["centres"][1]      # a cloud around camera 1 ...
    case["means3D"][77] = case["centres"][1]                              # ... with point 77 exactly at its centre
    cpu = torch.device("cpu")
    r64, r32 = (run(case, CAMERAS, dt, cpu, "torch", backward=False) for dt in (torch.float64, torch.float32))
    got = run(case, CAMERAS, torch.float32, hip_device, "fused", backward=False)
    for res in (r64, r32, got):
        assert not torch.isfinite(res["colours"][1, 77]).any()
    mask = torch.ones(3, 300, 3, dtype=torch.bool)
    mask[1, 77] = False
    assert torch.isfinite(got["colours"].cpu()[mask]).all()
    pick = lambda res: {"colours": res["colours"].cpu()[mask]}
    within("view_color", "point at a camera centre, every other entry", pick(got), pick(r64), pick(r32))


def fixture_step(data, dtype, device, **extra):
    from test_view_color_reference import run_fixture
    return run_fixture(data, dtype, device, **extra)


def test_whole_network_against_the_reference_record(hip_device):
    """SplatFields(view_color="fused") with the reference's parameters on the device against the reference's own float64 record, r
    from the reference's own float32 record"""
    from test_view_color_reference import load_fixture
    data = load_fixture()
    got = fixture_step(data, torch.float32, hip_device, view_color="fused")
    names = [k[len("f64/"):] for k in data.files if k.startswith("f64/")]
    assert set(got) == set(names)
    r64 = {k: torch.from_numpy(data["f64/" + k]) for k in names}
    r32 = {k: torch.from_numpy(data["f32/" + k]) for k in names}
    within("view_color", "network, reference record", got, r64, r32)


def test_the_default_path_is_untouched(hip_device):
    """without opt-in `rgb_fnc` and `for_cameras` are the PyTorch expressions, bit for bit, on the device"""
    from splatfields_amd.deform_field import SplatFields, ViewColor
    from splatfields_amd.view_color import view_color_path
    assert os.environ.get("SPLATFIELDS_VIEW_COLOR") or view_color_path() == "torch"
    dev = hip_device
    torch.manual_seed(9)
    net = SplatFields(n_frames=0, encoder_type="none", use_view_dep_rgb=True, view_color="torch").to(dev)
    xyz = (torch.rand(300, 3, device=dev) * 2 - 1)
    out = net(xyz, torch.zeros(300, 1, device=dev))
    fnc = out["rgb_fnc"]
    assert isinstance(fnc, ViewColor) and fnc.path == "torch"
    centres = torch.nn.functional.normalize(torch.randn(3, 3, device=dev), dim=-1) * 4
    batched = fnc.for_cameras(out["means3D"], centres)
    for i, c in enumerate(centres):
        ray_d = out["means3D"] - c[None]
        ray_d = ray_d / torch.norm(ray_d, dim=-1, keepdim=True)
        want = net.mlp_rgb_viewdep(torch.cat([fnc.feature, ray_d], dim=-1))
        assert torch.equal(fnc(ray_d), want) and torch.equal(batched[i], want)


def scene(dev, n=3000, width=64, n_views=3, seed=10):
    """a head, features and splats on the device, V cameras and their upstream image gradients"""
    from splatfields_amd.synthetic import make_camera, make_splats, make_upstream_grads
    case = make_case(n, width, n_views, seed=seed)
    sp = make_splats(n, seed=21, device=dev)
    W, H = 128, 96
    cams = [make_camera(i, W, H, device=dev) for i in range(n_views)]
    gi = [make_upstream_grads(H, W, seed=99 + i, device=dev)[0] for i in range(n_views)]
    return case["head"].to(dev), case["feature"].to(dev), sp, cams, gi


def gaussian_dict(sp, means3D, **colour):
    return dict({"means3D": means3D, "active_sh_degree": 0, "gaussian_opacity": sp["opacities"], "gaussian_scales": sp["scales"],
                 "gaussian_rotations": sp["rotations"]}, **colour)


def test_render_with_the_fused_object_is_render_given_its_colours(hip_device):
    from splatfields_amd import render
    from splatfields_amd.deform_field import ViewColor
    dev = hip_device
    head, feature, sp, cams, _ = scene(dev)
    pipe, bg = types.SimpleNamespace(debug=False), torch.ones(3, device=dev)
    fnc = ViewColor(head, feature, "fused")
    with torch.no_grad():
        for cam in cams:
            a = render(cam, gaussian_dict(sp, sp["means3D"], gaussian_rgb_fnc=fnc), pipe, bg)["render"]
            rgb = fnc.for_cameras(sp["means3D"], cam.camera_center[None])[0]
            b = render(cam, gaussian_dict(sp, sp["means3D"], gaussian_rgb=rgb), pipe, bg)["render"]
            assert torch.equal(a, b) and a.abs().max() > 0
            # a `gaussian_rgb` given in the dict still wins, and any other callable is treated as before
            c = render(cam, gaussian_dict(sp, sp["means3D"], gaussian_rgb=rgb * 0.5, gaussian_rgb_fnc=fnc), pipe, bg)["render"]
            assert not torch.equal(c, a)
            d = render(cam, gaussian_dict(sp, sp["means3D"], gaussian_rgb_fnc=lambda ray_d: ViewColor(head, feature, "torch")(ray_d)), pipe, bg)["render"]
            assert (d - a).abs().max().item() <= 1e-5


def test_a_view_loop_fed_from_one_call_against_single_view_calls_in_view_order(hip_device):
    """V x render() fed from ONE for_cameras call (`gaussian_rgb = rgbs[i]`) against V x render() with the fused object (V
    single-view calls, each with its own backward).  Bit-identical: every image, every view's colours, and what reaches the head --
    the single-view head fed view i's slice of the V-view arrangement's dL/drgbs returns the single-view arrangement's gradient.
    What is summed over the views cannot be bit-identical between the two: the V-view call adds the views' dL/dz in double in VIEW
    ORDER and rounds dL/dfeature and its share of dL/dmeans3D once (include/splatraster.h), V single-view calls round V times; and
    autograd adds the rasterizer's V contributions to means3D and opacity in float32.  Those sums are held to the single-view
    gradients added in view order in float64: the two differ by at most one float32 rounding per stored value and per float32
    addition, 3 V + 1 half-ulps in all, so 2 V ulp of the largest magnitude involved.  (dL/dweight and dL/dbias are sums over the
    points by sr_mlp_weight_grad in float32; they are measured against float64 in the tests above.)"""
    from splatfields_amd import render
    from splatfields_amd.deform_field import ViewColor
    dev = hip_device
    head, feature, sp, cams, gi = scene(dev)
    V = len(cams)
    pipe, bg = types.SimpleNamespace(debug=False), torch.ones(3, device=dev)
    centres = torch.stack([cam.camera_center for cam in cams])
    params = [head[0].weight, head[0].bias]

    def leaves():
        for p in params:
            p.grad = None
        return feature.detach().clone().requires_grad_(), sp["means3D"].detach().clone().requires_grad_(), sp["opacities"].detach().clone().requires_grad_()

    # one call for all views
    f, m, o = leaves()
    rgbs = ViewColor(head, f, "fused").for_cameras(m, centres)
    rgbs.retain_grad()
    images = [render(cams[i], gaussian_dict(dict(sp, opacities=o), m, gaussian_rgb=rgbs[i]), pipe, bg)["render"] for i in range(V)]
    sum((img * g).sum() for img, g in zip(images, gi)).backward()
    one = {"feature": f.grad, "means3D": m.grad, "opacity": o.grad, "weight": head[0].weight.grad.clone(), "bias": head[0].bias.grad.clone()}
    d_rgbs = rgbs.grad

    # V single-view calls, each with its own backward
    singles = []
    for i in range(V):
        f, m, o = leaves()
        fnc = ViewColor(head, f, "fused")
        pkg = render(cams[i], gaussian_dict(dict(sp, opacities=o), m, gaussian_rgb_fnc=fnc), pipe, bg)
        assert torch.equal(pkg["render"], images[i]), i
        (pkg["render"] * gi[i]).sum().backward()
        singles.append({"feature": f.grad, "means3D": m.grad, "opacity": o.grad, "weight": head[0].weight.grad.clone(), "bias": head[0].bias.grad.clone()})
        # the same upstream reaches the head in both arrangements: the single-view head alone, fed view i's slice of dL/drgbs
        f2, m2, _ = leaves()
        alone = ViewColor(head, f2, "fused").for_cameras(m2, centres[i:i + 1])
        alone.backward(d_rgbs[i:i + 1])
        assert torch.equal(alone[0], rgbs[i]) and torch.equal(f2.grad, singles[-1]["feature"]), i
    for k in ("feature", "means3D", "opacity"):
        total = sum(s[k].double() for s in singles)                      # view order
        top = max([total.abs().max().item()] + [s[k].abs().max().item() for s in singles])
        d = (one[k].double() - total).abs().max().item()
        ulp = ulp32(top)
        print(f"[view_color] view loop {k}: max difference {d:.3e}, float32 ulp at the largest magnitude {ulp:.3e}")
        assert top > 0 and d <= 2 * V * ulp, (k, d, ulp)
