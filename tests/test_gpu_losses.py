"""The fused photometric loss (splatfields_amd/losses.py -> sr_photometric_forward / _backward) on the MI355X against the
reference's own float64 evaluation (tests/golden/loss_cases.npz) and, at full size, against the restatement
tests/loss_reference.py that test_loss_reference.py pins to the reference.

Tolerance: for each metric -- |d ssim|, |d loss|, max|d grad| / max|grad|, relative L2 of the gradient -- r is the largest
deviation over ALL golden cases of the reference's own float32 evaluation from its float64 evaluation (for a full-size input:
the larger of that and the restatement's float32-against-float64 deviation on that input).  The kernels are another float32
evaluation of the same formulas in another summation order and may deviate from float64 by 4 r.  l1 and the mask term are held
to the bound of the loss they are blended into.  Nothing is exempted: every pixel of every case counts."""
import types

import pytest
import torch

from tests import loss_reference as R
from tests.accuracy import assert_deviations

pytestmark = pytest.mark.gpu

CASES = R.load_golden_cases()
R_GOLDEN = R.reference_error(CASES)


def hip_evaluate(dev, image, gt, opacity=None, gt_mask=None, lambda_dssim=0.2, lambda_mask=0.0):
    from splatfields_amd.losses import photometric_loss
    x = image.to(dev).requires_grad_(True)
    a = None if opacity is None else opacity.to(dev).requires_grad_(True)
    m = None if gt_mask is None else gt_mask.to(dev)
    loss, l1, terms = photometric_loss(x, gt.to(dev), lambda_dssim, a, m, lambda_mask, return_terms=True)
    assert loss.requires_grad and not l1.requires_grad and not terms["ssim"].requires_grad
    loss.backward()
    out = {"loss": loss, "l1": l1, "ssim": terms["ssim"], "d_image": x.grad}
    if a is not None:
        out["mask"], out["d_opacity"] = terms["mask"], a.grad
    return {k: v.detach().cpu() for k, v in out.items()}


def assert_within(tag, got, want, r):
    assert_deviations("loss", tag, R.deviations(got, want), r, R.METRICS)


@pytest.mark.parametrize("name", sorted(CASES))
def test_golden_cases_values_and_gradients(hip_device, name):
    c = CASES[name]
    lam, lam_mask = c["lambdas"].tolist()
    print("r over all golden cases:", R_GOLDEN)
    got = hip_evaluate(hip_device, c["image"], c["gt"], c.get("opacity"), c.get("gt_mask"), lam, lam_mask)
    assert got["d_image"].shape == c["image"].shape and got["loss"].dim() == 0
    assert_within(name, got, c["f64"], R_GOLDEN)


def test_golden_batch_per_item_ssim(hip_device):
    from splatfields_amd.losses import ssim
    c = CASES["batch"]
    x = c["image"].to(hip_device).requires_grad_(True)
    items = ssim(x, c["gt"].to(hip_device), size_average=False)
    assert tuple(items.shape) == (2,)
    (items * c["item_weights"].to(hip_device)).sum().backward()
    got = {"ssim_items": items.detach().cpu(), "d_image_items": x.grad.cpu()}
    want = {k: c["f64"][k] for k in got}
    assert_within("batch items", got, want, R_GOLDEN)


@pytest.mark.parametrize("height,width,background", [(800, 800, 1.0), (600, 800, 0.0)])
def test_full_size_with_mask_against_the_restatement(hip_device, height, width, background):
    pred, target, opacity, mask = R.blob_scene(height, width, background, seed=7)
    want = R.evaluate(pred, target, opacity, mask, 0.2, 0.1, dtype=torch.float64)
    own = R.deviations(R.evaluate(pred, target, opacity, mask, 0.2, 0.1, dtype=torch.float32), want)
    r = {k: max(R_GOLDEN[k], own[k]) for k in R.METRICS}
    print("restatement float32 against float64 on this input:", own)
    got = hip_evaluate(hip_device, pred, target, opacity, mask, 0.2, 0.1)
    assert_within(f"{height}x{width} bg {background}", got, want, r)


def test_drop_in_l1_and_ssim(hip_device):
    from splatfields_amd.losses import l1_loss, ssim
    dev = hip_device
    c = CASES["noise"]
    x = c["image"].to(dev).requires_grad_(True)
    y = c["gt"].to(dev)
    v = l1_loss(x, y)
    v.backward()
    assert v.dim() == 0 and abs(v.item() - c["f64"]["l1"].item()) <= 4 * R_GOLDEN["loss"]
    want = torch.sign(c["image"].double() - c["gt"].double()) / c["image"].numel()
    assert R.deviations({"d_image": x.grad.cpu()}, {"d_image": want})["grad_max"] <= 4 * R_GOLDEN["grad_max"]
    x.grad = None
    s = ssim(x, y)
    s.backward()
    xs = c["image"].double().requires_grad_(True)
    ws = R.ssim(xs, c["gt"].double())
    ws.backward()
    assert s.dim() == 0
    assert_within("ssim alone", {"ssim": s.detach().cpu(), "d_image": x.grad.cpu()}, {"ssim": ws.detach(), "d_image": xs.grad}, R_GOLDEN)
    # l1_loss takes any shape
    for shape in ((17,), (5, 3), (2, 3, 4, 5, 6)):
        p, q = torch.rand(shape), torch.rand(shape)
        assert abs(l1_loss(p.to(dev), q.to(dev)).item() - (p.double() - q.double()).abs().mean().item()) <= 4 * R_GOLDEN["loss"]
    # [B,C,H,W] with size_average=True is the mean over everything
    b = CASES["batch"]
    assert abs(ssim(b["image"].to(dev), b["gt"].to(dev)).item() - b["f64"]["ssim"].item()) <= 4 * R_GOLDEN["ssim"]


def test_depth_call_shape_hw1(hip_device):
    """train.py:221 calls ssim on [H,W,1] tensors: H planes of W x 1 out of the general indexing."""
    from splatfields_amd.losses import ssim
    c = CASES["depth_hw1"]
    x = c["image"].to(hip_device).requires_grad_(True)
    s = ssim(x, c["gt"].to(hip_device))
    s.backward()
    xs = c["image"].double().requires_grad_(True)
    ws = R.ssim(xs, c["gt"].double())
    ws.backward()
    assert abs(ws.item() - c["f64"]["ssim"].item()) <= 1e-12
    assert x.grad.shape == c["image"].shape
    assert_within("depth [H,W,1]", {"ssim": s.detach().cpu(), "d_image": x.grad.cpu()}, {"ssim": ws.detach(), "d_image": xs.grad}, R_GOLDEN)


def test_non_contiguous_and_float64_inputs_are_converted(hip_device):
    from splatfields_amd.losses import photometric_loss
    dev = hip_device
    c = CASES["noise"]
    rgba = torch.cat([c["image"], torch.rand(1, 37, 53)], dim=0).to(dev).requires_grad_(True)   # channel-sliced view of 4 channels
    view = rgba[:3]
    wide = torch.zeros(3, 37, 60, device=dev)
    wide[:, :, :53] = c["gt"].to(dev)
    gt_view = wide[:, :, :53]
    assert not gt_view.is_contiguous()
    loss, _ = photometric_loss(view, gt_view, 0.2)
    loss.backward()
    base = hip_evaluate(dev, c["image"], c["gt"])
    assert torch.equal(loss.detach().cpu(), base["loss"])
    assert torch.equal(rgba.grad[:3].cpu(), base["d_image"]) and (rgba.grad[3] == 0).all()
    x64 = c["image"].double().to(dev).requires_grad_(True)
    loss64, l1 = photometric_loss(x64, c["gt"].double().to(dev), 0.2)
    loss64.backward()
    assert loss64.dtype == torch.float64 and l1.dtype == torch.float64 and x64.grad.dtype == torch.float64
    assert torch.equal(x64.grad.float().cpu(), base["d_image"])


def test_upstream_gradient_scales_the_result(hip_device):
    from splatfields_amd.losses import photometric_loss
    dev = hip_device
    ca, cb = CASES["noise"], CASES["blob_black"]

    def grads(c):
        x = c["image"].to(dev).requires_grad_(True)
        a = c["opacity"].to(dev).requires_grad_(True)
        loss, _ = photometric_loss(x, c["gt"].to(dev), 0.2, a, c["gt_mask"].to(dev), 0.1)
        return x, a, loss

    xa, aa, la = grads(ca)
    la.backward()
    xb, ab, lb = grads(cb)
    lb.backward()
    # (0.3 * loss).backward(): 0.3 x, to float32 rounding of one multiplication
    x3, a3, l3 = grads(ca)
    (0.3 * l3).backward()
    for got, one in ((x3.grad, xa.grad), (a3.grad, aa.grad)):
        assert torch.allclose(got, 0.3 * one, rtol=3e-7, atol=0.0)
    # the view loop of train.py:242,252: sum(loss_list) / len(loss_list), one backward -- 0.5 is a power of two: bit-exact
    x1, a1, l1 = grads(ca)
    x2, a2, l2 = grads(cb)
    loss_list = [l1, l2]
    (sum(loss_list) / len(loss_list)).backward()
    for got, one in ((x1.grad, xa.grad), (a1.grad, aa.grad), (x2.grad, xb.grad), (a2.grad, ab.grad)):
        assert torch.equal(got, 0.5 * one)


def test_bit_reproducible(hip_device):
    first = None
    c = CASES["blob_white"]
    pred, target, opacity, mask = R.blob_scene(200, 333, 1.0, seed=3)
    for _ in range(10):
        got = hip_evaluate(hip_device, pred, target, opacity, mask, 0.2, 0.1)
        small = hip_evaluate(hip_device, c["image"], c["gt"])
        got = (got["loss"], got["d_image"], got["d_opacity"], small["loss"], small["d_image"])
        first = first or got
        assert all(torch.equal(p, q) for p, q in zip(got, first))


def test_equal_pixels_and_the_clamp_boundaries(hip_device):
    from splatfields_amd.losses import l1_loss, photometric_loss
    dev = hip_device
    x = torch.rand(3, 40, 50)
    y = x.clone()
    y[:, :, 25:] += 0.25
    xg = x.to(dev).requires_grad_(True)
    l1_loss(xg, y.to(dev)).backward()
    assert (xg.grad[:, :, :25] == 0).all() and (xg.grad[:, :, 25:] == -1.0 / x.numel()).all()
    a = torch.tensor([-0.5, -1e-6, 0.0, 0.25, 1.0, 1.0 + 1e-6, 3.0, 0.0, 1.0, 0.5]).repeat(20).reshape(1, 10, 20)
    m = torch.tensor([0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 1.0, 0.0, 1.0, 0.5]).repeat(20).reshape(1, 10, 20)
    ag = a.to(dev).requires_grad_(True)
    img = torch.rand(3, 10, 20, device=dev)
    loss, _ = photometric_loss(img.clone().requires_grad_(True), img, 0.2, ag, m.to(dev), 0.1)
    loss.backward()
    # outside [0, 1]: nothing; 0 and 1 pass (torch.clamp); sign(0) = 0 where the clamped opacity equals the mask
    weight = (torch.tensor(0.1, dtype=torch.float32).double() / 200).float()      # lambda_mask travels as a float; mean over 200
    want = torch.tensor([0.0, 0.0, -1.0, 1.0, 1.0, 0.0, 0.0, 0.0, 0.0, 0.0]).repeat(20).reshape(1, 10, 20) * weight
    assert torch.equal(ag.grad.cpu(), want)


def test_errors_and_no_grad(hip_device):
    from splatfields_amd.losses import l1_loss, photometric_loss, ssim
    dev = hip_device
    x, y = torch.rand(3, 16, 16), torch.rand(3, 16, 16)
    for fn in (l1_loss, ssim, photometric_loss):
        with pytest.raises(RuntimeError, match="no CPU path"):
            fn(x, y)
    xd, yd = x.to(dev), y.to(dev)
    with pytest.raises(ValueError, match="built for the reference's window"):
        ssim(xd, yd, window_size=7)
    with pytest.raises(RuntimeError, match="target requires grad"):
        photometric_loss(xd.clone().requires_grad_(True), yd.clone().requires_grad_(True))
    with pytest.raises(RuntimeError, match="target requires grad"):
        photometric_loss(xd.clone().requires_grad_(True), yd, 0.2, torch.rand(1, 16, 16, device=dev),
                         torch.rand(1, 16, 16, device=dev).requires_grad_(True), 0.1)
    with pytest.raises(RuntimeError, match="both or neither"):
        photometric_loss(xd, yd, 0.2, opacity=torch.rand(1, 16, 16, device=dev))
    with pytest.raises(RuntimeError, match="same shape"):
        ssim(xd, yd[:, :8])
    with pytest.raises(RuntimeError, match="no CPU path"):
        photometric_loss(xd, yd, 0.2, torch.rand(1, 16, 16), torch.rand(1, 16, 16), 0.1)
    xr = xd.clone().requires_grad_(True)
    with torch.no_grad():
        loss, l1 = photometric_loss(xr, yd)
    assert loss.grad_fn is None and not loss.requires_grad and not l1.requires_grad
    tracked, _ = photometric_loss(xr, yd)
    assert torch.equal(tracked.detach(), loss)          # the same kernels with and without the derivative maps
    plain, _ = photometric_loss(xd, yd)                  # nothing requires grad: no graph either
    assert plain.grad_fn is None and torch.equal(plain, loss)


def test_no_host_wait_from_the_python_side(hip_device):
    from splatfields_amd.losses import photometric_loss
    dev = hip_device
    c = CASES["noise"]
    x = c["image"].to(dev).requires_grad_(True)
    a = c["opacity"].to(dev).requires_grad_(True)
    y, m = c["gt"].to(dev), c["gt_mask"].to(dev)
    photometric_loss(x, y, 0.2, a, m, 0.1)[0].backward()    # warm up: library load, allocator
    torch.cuda.synchronize()
    try:
        torch.cuda.set_sync_debug_mode("error")
    except Exception as e:   # noqa: BLE001
        pytest.skip(f"this torch build does not implement set_sync_debug_mode: {e}")
    try:
        loss, _ = photometric_loss(x, y, 0.2, a, m, 0.1)
        (0.5 * loss).backward()
    finally:
        torch.cuda.set_sync_debug_mode("default")
    torch.cuda.synchronize()
    assert torch.isfinite(loss).all()


def test_end_to_end_through_the_rasterizer(hip_device):
    """render() -> photometric_loss -> backward() against render() -> restatement -> backward(): every parameter gradient within
    4 x the relative L2 by which the same rasterizer backward differs between the restatement's float32 and float64 dL/dimage."""
    from splatfields_amd import render
    from splatfields_amd.losses import photometric_loss
    from splatfields_amd.synthetic import make_camera, make_splats
    dev = hip_device
    torch.manual_seed(0)
    n, W, H = 4000, 160, 128
    target_sp = make_splats(n, seed=21, mean_scale=0.05, device=dev)
    pipe = types.SimpleNamespace(debug=False)
    bg = torch.ones(3, device=dev)
    cam = make_camera(2, W, H, device=dev)
    pack = lambda sp: {"means3D": sp["means3D"], "active_sh_degree": 1, "gaussian_opacity": sp["opacities"],
                       "gaussian_features": sp["shs"], "gaussian_scales": sp["scales"], "gaussian_rotations": sp["rotations"]}
    with torch.no_grad():
        t = render(cam, pack(target_sp), pipe, bg)
        gt_image, gt_mask = t["render"].clone(), (t["opacity"] > 0.5).float()
    start = {"means3D": target_sp["means3D"] + 0.02 * torch.randn(n, 3, device=dev), "scales": target_sp["scales"] * 1.3,
             "rotations": target_sp["rotations"].clone(), "opacities": target_sp["opacities"].clamp(0.05, 0.95) * 0.8,
             "shs": target_sp["shs"] + 0.2 * torch.randn_like(target_sp["shs"])}

    def run(loss_side):
        leaf = {k: v.clone().requires_grad_(True) for k, v in start.items()}
        pkg = render(cam, pack(leaf), pipe, bg)
        loss_side(pkg["render"], pkg["opacity"])
        return {k: v.grad.detach().cpu().double() for k, v in leaf.items()}

    def fused(image, opacity):
        photometric_loss(image, gt_image, 0.2, opacity, gt_mask, 0.1)[0].backward()

    def restated(dtype):
        def side(image, opacity):
            g = R.evaluate(image.cpu(), gt_image.cpu(), opacity.cpu(), gt_mask.cpu(), 0.2, 0.1, dtype=dtype)
            torch.autograd.backward([image, opacity], [g["d_image"].float().to(dev), g["d_opacity"].float().to(dev)])
        return side

    g_hip, g32, g64 = run(fused), run(restated(torch.float32)), run(restated(torch.float64))
    rel = lambda p, q: ((p - q).norm() / q.norm().clamp_min(1e-300)).item()
    for k in g64:
        yard, got = rel(g32[k], g64[k]), rel(g_hip[k], g64[k])
        print(f"[loss] end to end {k}: fused {got:.3e}, restatement float32 against float64 {yard:.3e}")
        assert g64[k].abs().max() > 0 and got <= 4.0 * yard, (k, got, yard)
