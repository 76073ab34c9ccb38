"""The fused evaluation metrics (splatfields_amd/metrics.py -> sr_image_metrics) on the MI355X against the reference's own
float64 evaluation (tests/golden/metric_cases.npz) and, at full size, against the restatement tests/metric_reference.py that
test_metric_reference.py pins to the reference.

Tolerance: for each metric -- |d ssim|, |d psnr| in dB (the per-channel PSNR counts as PSNR) -- r is the largest deviation over
ALL golden cases of the reference's own float32 evaluation from its float64 evaluation (for a full-size input: the larger of
that and the restatement's float32-against-float64 deviation on that input).  The kernel is another float32 evaluation of the
same formulas in another summation order and may deviate from float64 by 4 r.  Nothing is exempted: every case and every item
counts.  Everything the kernel promises exactly -- the quantised bytes, batch against single calls, the two layouts, repeated
calls, an empty mask -- is compared bit for bit."""
import functools
import types

import pytest
import torch

from tests import metric_reference as R
from tests.accuracy import assert_deviations, same_bits

pytestmark = pytest.mark.gpu

CASES = R.load_golden_cases()
R_GOLDEN = R.reference_error(CASES)
INF = float("inf")


def hip_metrics(dev, pred, gt, mask=None, **kw):
    from splatfields_amd.metrics import image_metrics
    out = image_metrics(pred.to(dev), gt.to(dev), None if mask is None else mask.to(dev), **kw)
    return {k: v.cpu() for k, v in out.items()}


def assert_within(tag, got, want, r):
    assert_deviations("metrics", tag, R.deviations(got, want), r, R.METRICS)


@pytest.mark.parametrize("name", sorted(CASES))
def test_golden_cases(hip_device, name):
    c = CASES[name]
    print("r over all golden cases:", R_GOLDEN)
    got = hip_metrics(hip_device, c["pred"], c["gt"], c.get("mask"))
    assert got["psnr"].dim() == 0 and got["ssim"].dim() == 0 and tuple(got["psnr_channels"].shape) == (3,)
    assert all(v.dtype == torch.float32 for v in got.values())
    assert_within(name, {"psnr": got["psnr"], "ssim": got["ssim"]}, c["f64"], R_GOLDEN)
    want = R.evaluate(c["pred"], c["gt"], c.get("mask"), dtype=torch.float64)       # pinned to the golden values on the CPU
    assert_within(name + " channels", got, want, R_GOLDEN)


def test_drop_ins_have_the_reference_signatures(hip_device):
    from splatfields_amd import compute_psnr, compute_ssim, psnr
    dev = hip_device
    c = CASES["mask_random"]
    img0, img1, mask = R.hwc(c["pred"]).contiguous().to(dev), R.hwc(c["gt"]).contiguous().to(dev), c["mask"][..., None].to(dev)
    p, s, sm = compute_psnr(img0, img1), compute_ssim(img0, img1), compute_ssim(img0, img1, mask)
    assert p.dim() == 0 and s.dim() == 0 and sm.dim() == 0 and p.dtype == torch.float32 and p.device == img0.device
    assert_within("drop-ins, masked", {"psnr": p.cpu(), "ssim": sm.cpu()}, c["f64"], R_GOLDEN)
    assert_within("drop-ins, no mask", {"ssim": s.cpu()}, CASES["mask_one"]["f64"], R_GOLDEN)
    assert torch.equal(compute_ssim(img0, img1, mask, 1.0, 11, 1.5, 0.01, 0.03), sm)      # the defaults, positionally
    per_channel = psnr(c["pred"].to(dev), c["gt"].to(dev))
    assert tuple(per_channel.shape) == (3, 1)
    want = R.evaluate(c["pred"], c["gt"])
    assert_within("utils.image_utils.psnr", {"psnr_channels": per_channel.cpu().reshape(3)}, want, R_GOLDEN)
    # another dtype is converted, and answered in kind
    p64 = compute_psnr(img0.double(), img1.double())
    assert p64.dtype == torch.float64 and p64.item() == p.item()
    assert compute_ssim(img0.half(), img1.half()).dtype == torch.float16
    for kw in (dict(filter_size=7), dict(filter_sigma=1.0), dict(k1=0.02), dict(k2=0.01), dict(max_val=255.0)):
        with pytest.raises(NotImplementedError, match="reference's defaults"):
            compute_ssim(img0, img1, **kw)
    with pytest.raises(ValueError, match="at least 11 x 11"):
        compute_ssim(img0[:10], img1[:10])
    with pytest.raises(ValueError, match="at least 11 x 11"):
        compute_ssim(img0[:, :7], img1[:, :7])
    with pytest.raises(RuntimeError, match="no CPU path"):
        compute_ssim(img0.cpu(), img1.cpu())
    with pytest.raises(RuntimeError, match=r"\[H,W,1\] mask"):
        compute_ssim(img0, img1, mask[..., 0])
    with pytest.raises(RuntimeError, match="same shape"):
        compute_psnr(img0, img1[:20])


def test_image_metrics_refuses_bad_calls(hip_device):
    from splatfields_amd import image_metrics
    x = torch.rand(3, 16, 16, device=hip_device)
    with pytest.raises(RuntimeError, match="no CPU path"):
        image_metrics(x.cpu(), x.cpu())
    with pytest.raises(RuntimeError, match="no CPU path"):
        image_metrics(x, x, torch.ones(16, 16))
    with pytest.raises(ValueError, match="layout"):
        image_metrics(x, x, layout="nchw")
    with pytest.raises(ValueError, match="quantize"):
        image_metrics(x, x, quantize="jpeg")
    with pytest.raises(ValueError, match="return_frames needs"):
        image_metrics(x, x, return_frames=True)
    with pytest.raises(RuntimeError, match="RGB"):
        image_metrics(x, x, layout="hwc")
    wide = torch.rand(2, 3, 16, 24, device=hip_device)
    for shape in ((16, 15), (24, 16), (16, 24, 2), (2, 24, 16), (1, 1, 16, 24), (2 * 16 * 24,)):   # the right count is not enough
        with pytest.raises(RuntimeError, match="the mask must be"):
            image_metrics(wide, wide, torch.ones(shape, device=hip_device))


def test_all_one_mask_against_no_mask_and_all_zero_mask(hip_device):
    c = CASES["mask_one"]
    plain = hip_metrics(hip_device, c["pred"], c["gt"])
    ones = hip_metrics(hip_device, c["pred"], c["gt"], torch.ones(37, 53))
    assert_within("no mask", plain, {"ssim": c["f64"]["ssim"], "psnr": c["f64"]["psnr"]}, R_GOLDEN)
    assert_within("all-one mask", ones, {"ssim": c["f64"]["ssim"], "psnr": c["f64"]["psnr"]}, R_GOLDEN)
    assert torch.equal(plain["psnr"], ones["psnr"]) and torch.equal(plain["psnr_channels"], ones["psnr_channels"])   # never masked
    # a mask is read as != 0
    assert same_bits(ones, hip_metrics(hip_device, c["pred"], c["gt"], torch.full((37, 53), 0.25)))
    for name in ("noise_11x11", "noise_43x75", "grid8"):
        k = CASES[name]
        h, w = k["pred"].shape[1:]
        zero = hip_metrics(hip_device, k["pred"], k["gt"], torch.zeros(h, w))
        assert zero["ssim"].item() == 1.0, name
        assert torch.equal(zero["psnr"], hip_metrics(hip_device, k["pred"], k["gt"])["psnr"])


def test_identical_images(hip_device):
    x = CASES["noise_43x75"]["pred"]
    for kw in (dict(), dict(quantize="png"), dict(mask=CASES["disc"]["mask"])):
        got = hip_metrics(hip_device, x, x.clone(), **kw)
        assert got["psnr"].item() == INF and (got["psnr_channels"] == INF).all(), kw
        assert abs(got["ssim"].item() - 1.0) <= 4.0 * R_GOLDEN["ssim"], kw
    # one channel identical: its PSNR alone is infinite
    y = x.clone()
    y[1:] = CASES["noise_43x75"]["gt"][1:]
    got = hip_metrics(hip_device, x, y)
    assert got["psnr_channels"][0].item() == INF and torch.isfinite(got["psnr_channels"][1:]).all() and torch.isfinite(got["psnr"])


def batch_of_three():
    a, b, c = CASES["mask_random"], CASES["near_equal"], CASES["mask_hole"]
    pred, gt = torch.stack([a["pred"], b["pred"], c["gt"]]), torch.stack([a["gt"], b["gt"], c["pred"] * 0.5])
    mask = torch.stack([a["mask"], torch.ones(37, 53), c["mask"]])
    return pred, gt, mask


@pytest.mark.parametrize("masked", [False, True])
def test_a_batch_equals_the_single_calls_bit_for_bit(hip_device, masked):
    pred, gt, mask = batch_of_three()
    for kw in (dict(), dict(quantize="png", return_frames=True)):
        got = hip_metrics(hip_device, pred, gt, mask if masked else None, **kw)
        assert tuple(got["psnr"].shape) == (3,) and tuple(got["ssim"].shape) == (3,) and tuple(got["psnr_channels"].shape) == (3, 3)
        for i in range(3):
            one = hip_metrics(hip_device, pred[i], gt[i], mask[i] if masked else None, **kw)
            assert same_bits(one, {k: v[i] for k, v in got.items()}), (i, kw)
        assert len({got["ssim"][i].item() for i in range(3)}) == 3
    want = R.evaluate(pred, gt, mask if masked else None)
    assert_within("batch", hip_metrics(hip_device, pred, gt, mask if masked else None), want, R_GOLDEN)
    if masked:   # one mask for the whole batch
        shared = hip_metrics(hip_device, pred, gt, mask[0])
        assert same_bits(shared, hip_metrics(hip_device, pred, gt, mask[0][None].expand(3, 37, 53).contiguous()))


def test_layouts_and_strides_agree_bit_for_bit(hip_device):
    from splatfields_amd import image_metrics
    dev = hip_device
    pred, gt, mask = (t.to(dev) for t in batch_of_three())
    kw = dict(quantize="to8b", return_frames=True)
    base = image_metrics(pred, gt, mask, **kw)
    hwc = image_metrics(R.hwc(pred).contiguous(), R.hwc(gt).contiguous(), mask[..., None], layout="hwc", **kw)
    assert same_bits(base, hwc)
    # views: a permuted HWC tensor read as CHW, a channel slice of RGBA, a crop of a wider image, a float64 target
    assert same_bits(base, image_metrics(R.chw(R.hwc(pred).contiguous()), gt, mask, **kw))
    rgba = torch.cat([pred, torch.rand(3, 1, 37, 53, device=dev)], dim=1)
    wide = torch.zeros(3, 3, 37, 64, device=dev)
    wide[..., 5:58] = gt
    assert not rgba[:, :3].is_contiguous() and not wide[..., 5:58].is_contiguous()
    assert same_bits(base, image_metrics(rgba[:, :3], wide[..., 5:58], mask, **kw))
    assert same_bits(base, image_metrics(pred, gt.double(), mask.bool(), **kw))
    # the 16-byte loads of a 4-aligned width against the element loads of a shifted view of the same pixels
    x, y = torch.rand(2, 3, 40, 64, device=dev), torch.rand(2, 3, 40, 64, device=dev)
    m = (torch.rand(2, 40, 64, device=dev) < 0.7).float()
    pad = lambda t: torch.nn.functional.pad(t, (1, 2))[..., 1:65]
    assert pad(x).data_ptr() % 16 != 0 and torch.equal(pad(x), x)
    for mm in (None, m):
        assert same_bits(image_metrics(x, y, mm, quantize="png", return_frames=True),
                         image_metrics(pad(x), pad(y), mm, quantize="png", return_frames=True))
    assert_within("40x64", {k: v.cpu() for k, v in image_metrics(x, y, m).items()}, R.evaluate(x.cpu(), y.cpu(), m.cpu()), R_GOLDEN)


def probe_image():
    """[3,43,75]: every level, every half-way point and its float32 neighbours, values outside [0, 1], noise"""
    gen = torch.Generator().manual_seed(11)
    x = (torch.rand(3 * 43 * 75, generator=gen) * 1.4 - 0.2)
    k = torch.arange(0, 256, dtype=torch.float32)
    half = (k + 0.5) / 255.0
    pts = torch.cat([k / 255.0, half, torch.nextafter(half, torch.tensor(0.0)), torch.nextafter(half, torch.tensor(2.0)),
                     torch.tensor([-0.3, -1e-9, 0.0, 1.0, 1.0 + 1e-6, 1.7])])
    x[torch.randperm(x.numel(), generator=gen)[: pts.numel()]] = pts
    return x.reshape(3, 43, 75)


@pytest.mark.parametrize("mode", ["png", "to8b"])
def test_quantised_frames_and_metrics_are_exact(hip_device, mode):
    x = probe_image()
    y = CASES["noise_43x75"]["gt"] * 1.2 - 0.1
    pred, gt = torch.stack([x, y]), torch.stack([y, x.flip(-1)])
    got = hip_metrics(hip_device, pred, gt, quantize=mode, return_frames=True)
    assert got["frames"].dtype == torch.uint8 and tuple(got["frames"].shape) == (2, 43, 75, 3)
    assert torch.equal(got["frames"], R.frames(pred, mode))                      # the bytes the reference writes
    one = hip_metrics(hip_device, x, y, quantize=mode, return_frames=True)
    assert tuple(one["frames"].shape) == (43, 75, 3) and torch.equal(one["frames"], got["frames"][0])
    # the metrics of the round trip are the metrics of the images that come back from it
    del got["frames"]
    assert same_bits(got, hip_metrics(hip_device, R.quantize(pred, mode), R.quantize(gt, mode)))
    assert same_bits(got, hip_metrics(hip_device, pred, gt, quantize=mode))     # with and without the frames
    assert_within(mode, got, R.evaluate(pred, gt, quantize_mode=mode), R_GOLDEN)
    if mode == "png":
        assert not same_bits(got, hip_metrics(hip_device, pred, gt))
        masked = hip_metrics(hip_device, pred, gt, CASES["disc"]["mask"], quantize=mode)
        assert same_bits(masked, hip_metrics(hip_device, R.quantize(pred, mode), R.quantize(gt, mode), CASES["disc"]["mask"]))


def test_repeated_calls_are_bit_identical(hip_device):
    pred, gt, mask = batch_of_three()
    p, t, m = R.textured_pair(200, 333, seed=3)
    first = None
    for _ in range(5):
        got = (hip_metrics(hip_device, pred, gt, mask, quantize="png", return_frames=True), hip_metrics(hip_device, p, t),
               hip_metrics(hip_device, p, t, m))
        first = first or got
        assert all(same_bits(a, b) for a, b in zip(got, first))


@functools.lru_cache(maxsize=None)
def full_size_case(height, width, masked):
    pred, target, disc = R.textured_pair(height, width, seed=7)
    mask = disc if masked else None
    want = R.evaluate(pred, target, mask, "png", dtype=torch.float64)
    own = R.deviations(R.evaluate(pred, target, mask, "png", dtype=torch.float32), want)
    return pred, target, mask, want, own


@pytest.mark.parametrize("height,width,masked", [(800, 800, False), (600, 800, True)])
def test_full_size_against_the_restatement(hip_device, height, width, masked):
    pred, target, mask, want, own = full_size_case(height, width, masked)
    r = {k: max(R_GOLDEN[k], own[k]) for k in R.METRICS}
    print("restatement float32 against float64 on this input:", own)
    got = hip_metrics(hip_device, pred, target, mask, quantize="png")
    assert_within(f"{height}x{width} masked={masked}", got, want, r)


def test_no_host_wait_from_the_python_side(hip_device):
    from splatfields_amd import image_metrics
    dev = hip_device
    pred, gt, mask = (t.to(dev) for t in batch_of_three())
    image_metrics(pred, gt, mask, quantize="png", return_frames=True)    # warm up: library load, allocator
    torch.cuda.synchronize()
    armed = True
    try:
        torch.cuda.set_sync_debug_mode("error")
    except Exception:   # noqa: BLE001  (a torch build without the switch: the call below still has to work)
        armed = False
    try:
        out = image_metrics(pred, gt, mask, quantize="png", return_frames=True)
        hwc = image_metrics(R.hwc(pred), R.hwc(gt), layout="hwc")
    finally:
        if armed:
            torch.cuda.set_sync_debug_mode("default")
    torch.cuda.synchronize()
    assert torch.isfinite(out["ssim"]).all() and torch.isfinite(hwc["psnr"]).all()


def test_end_to_end_through_the_rasterizer(hip_device):
    """render() -> image_metrics(quantize="png") on the [3,H,W] render as it leaves the rasterizer, against the restatement on
    the copied-out image."""
    from splatfields_amd import image_metrics, render
    from splatfields_amd.synthetic import make_camera, make_splats
    dev = hip_device
    torch.manual_seed(0)
    n, W, H = 4000, 160, 128
    sp = make_splats(n, seed=21, mean_scale=0.05, device=dev)
    pipe = types.SimpleNamespace(debug=False)
    bg = torch.ones(3, device=dev)
    cam = make_camera(2, W, H, device=dev)
    pack = lambda s: {"means3D": s["means3D"], "active_sh_degree": 1, "gaussian_opacity": s["opacities"],
                      "gaussian_features": s["shs"], "gaussian_scales": s["scales"], "gaussian_rotations": s["rotations"]}
    with torch.no_grad():
        t = render(cam, pack(sp), pipe, bg)
        target, mask = t["render"].clone(), (t["opacity"] > 0.5).float()
        moved = dict(sp, means3D=sp["means3D"] + 0.01 * torch.randn(n, 3, device=dev), shs=sp["shs"] + 0.1 * torch.randn_like(sp["shs"]))
        image = render(cam, pack(moved), pipe, bg)["render"]
        assert tuple(image.shape) == (3, H, W) and 0.0 < mask.mean().item() < 1.0    # background and foreground
        got = image_metrics(image, target, mask, quantize="png", return_frames=True)
    img, tgt, msk = image.cpu(), target.cpu(), mask.cpu()
    want = R.evaluate(img, tgt, msk, "png", dtype=torch.float64)
    own = R.deviations(R.evaluate(img, tgt, msk, "png", dtype=torch.float32), want)
    r = {k: max(R_GOLDEN[k], own[k]) for k in R.METRICS}
    assert torch.isfinite(want["psnr"]) and 0.0 < want["ssim"].item() < 1.0
    assert_within("render", {k: v.cpu() for k, v in got.items() if k != "frames"}, want, r)
    assert torch.equal(got["frames"].cpu(), R.frames(img, "png"))
