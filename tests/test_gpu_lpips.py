"""LPIPS (VGG) on the MI355X (splatfields_amd/lpips.py -> sr_lpips_forward) against the float64 restatement
tests/lpips_reference.py, with random weights (LPIPSWeights.random): the published weights are not available here.

Accuracy (tests/accuracy.py): every element of the five per-pixel maps may deviate from float64 by 4 r, r = the larger error of
the restatement's two float32 evaluation orders against float64 on the same input, floored at one float32 ulp of the map's
maximum.  A mean cannot err by more than its terms, so tap l may deviate by 4 r_l + 4 ulp32(tap_l) and the value by the sum of
the five bounds.  Everything the op promises exactly is compared bit for bit."""
import functools

import pytest
import torch

from tests import lpips_reference as R
from tests.accuracy import assert_deviations, ulp32
from tests.launches import device_records, launches_per_iteration

pytestmark = pytest.mark.gpu

# 16x16: relu5_3 is 1x1.  37x53: odd everywhere (37 -> 18 -> 9 -> 4 -> 2), partial tiles in every layer.  33x31 / 31x33: one
# past and one short of the convolution's 8x16-pixel tile (and of the first layer's 16x16) in either direction.
SHAPES = {"16x16": (4, 16, 16), "37x53": (4, 37, 53), "64x48": (3, 64, 48), "33x31": (2, 33, 31), "31x33": (2, 31, 33)}


@functools.lru_cache(maxsize=None)
def weights_cpu():
    from splatfields_amd.lpips import LPIPSWeights
    return LPIPSWeights.random(11)


@functools.lru_cache(maxsize=None)
def weights_on(dev):
    w = weights_cpu().to(dev)
    w.packed()
    return w


@functools.lru_cache(maxsize=None)
def case(name, quantize=None):
    """inputs, the float64 reference and r per map: computed once, shared, never modified"""
    b, h, w = SHAPES[name]
    pred, gt = R.images(b, h, w, seed=100 + h)
    p = R.parts(weights_cpu())
    ref = R.evaluate(pred, gt, *p, dtype=torch.float64, quantize=quantize)
    f32 = [R.evaluate(pred, gt, *p, dtype=torch.float32, order=o, quantize=quantize) for o in R.ORDERS]
    r = [max([(f["maps"][l].double() - ref["maps"][l]).abs().max().item() for f in f32] + [ulp32(ref["maps"][l].abs().max().item())])
         for l in range(5)]
    return pred, gt, ref, r


def run(dev, pred, gt, **kw):
    from splatfields_amd import lpips_vgg
    return lpips_vgg(pred.to(dev), gt.to(dev), weights_on(dev), **kw)


@pytest.mark.parametrize("name", sorted(SHAPES))
def test_maps_and_scalars_against_float64(hip_device, name):
    pred, gt, ref, r = case(name)
    value, taps, maps = run(hip_device, pred, gt, return_maps=True)
    b, h, w = SHAPES[name]
    assert tuple(value.shape) == (b,) and tuple(taps.shape) == (b, 5) and value.dtype == torch.float32
    assert [tuple(m.shape) for m in maps] == [(b, h >> l, w >> l) for l in range(5)]
    keys = [f"map{l}" for l in range(5)]
    d = {k: (m.double().cpu() - w64).abs().max().item() for k, m, w64 in zip(keys, maps, ref["maps"])}
    assert all(torch.isfinite(m).all() for m in maps)
    assert_deviations("lpips", name + " maps", d, dict(zip(keys, r)), keys)
    # scalars: FACTOR x (r_l + ulp32(tap_l)) per tap, their sum for the value (assert_deviations multiplies by FACTOR)
    tap_top = ref["taps"].abs().max(0).values
    rt = {f"tap{l}": r[l] + ulp32(tap_top[l].item()) for l in range(5)}
    dt = {f"tap{l}": (taps[:, l].double().cpu() - ref["taps"][:, l]).abs().max().item() for l in range(5)}
    rt["value"], dt["value"] = sum(rt.values()), (value.double().cpu() - ref["value"]).abs().max().item()
    assert_deviations("lpips", name + " scalars", dt, rt, list(rt))
    assert (ref["value"] > 1e-3).all()                       # the inputs differ enough for the comparison to mean something


def test_calls_batches_and_chunks_give_the_same_bits(hip_device):
    from splatfields_amd import _lib
    pred, gt, _, _ = case("37x53")
    first = run(hip_device, pred, gt, return_taps=True)
    second = run(hip_device, pred, gt, return_taps=True)
    assert torch.equal(first[0], second[0]) and torch.equal(first[1], second[1])
    assert torch.equal(run(hip_device, pred, gt), first[0])
    singles = [run(hip_device, pred[i], gt[i], return_taps=True) for i in range(4)]
    assert all(s[0].dim() == 0 and tuple(s[1].shape) == (5,) for s in singles)
    assert torch.equal(torch.stack([s[0] for s in singles]), first[0]) and torch.equal(torch.stack([s[1] for s in singles]), first[1])
    one = _lib.load().sr_lpips_workspace_bytes(1, 37, 53)
    for cap in (one, 2 * one + 4096):                        # chunks of one; chunks of two
        chunked = run(hip_device, pred, gt, return_taps=True, max_workspace_bytes=cap)
        assert torch.equal(chunked[0], first[0]) and torch.equal(chunked[1], first[1]), cap
    with pytest.raises(ValueError, match="max_workspace_bytes"):
        run(hip_device, pred, gt, max_workspace_bytes=one - 1)
    # the order of the items does not matter to an item
    flipped = run(hip_device, pred.flip(0), gt.flip(0))
    assert torch.equal(flipped.flip(0), first[0])


def test_layouts_and_strides_give_the_same_bits(hip_device):
    dev = hip_device
    pred, gt, _, _ = case("37x53")
    want = run(dev, pred, gt)
    p, g = pred.to(dev), gt.to(dev)
    w = weights_on(dev)
    from splatfields_amd import lpips_vgg
    assert torch.equal(lpips_vgg(p.permute(0, 2, 3, 1), g.permute(0, 2, 3, 1), w, layout="hwc"), want)               # views
    assert torch.equal(lpips_vgg(p.permute(0, 2, 3, 1).contiguous(), g.permute(0, 2, 3, 1).contiguous(), w, layout="hwc"), want)
    big_p, big_g = torch.rand(4, 3, 45, 64, device=dev), torch.rand(5, 3, 40, 60, device=dev)
    big_p[:, :, 3:40, 5:58], big_g[1:, :, 2:39, 7:60] = p, g
    assert torch.equal(lpips_vgg(big_p[:, :, 3:40, 5:58], big_g[1:, :, 2:39, 7:60], w), want)                          # slices
    assert torch.equal(lpips_vgg(p.double(), g.double(), w), want)                                                    # another dtype


@pytest.mark.parametrize("mode", ["png", "to8b"])
def test_quantisation_equals_images_quantised_beforehand(hip_device, mode):
    dev = hip_device
    pred, gt, _, _ = case("16x16")
    pred = pred * 1.2 - 0.1                                  # some values outside [0, 1]
    # quantised with torch on the CPU: on the device torch divides by a scalar as a multiplication with its reciprocal, which is
    # not the file round trip's `/ 255.` in the last bit
    q = (lambda x: (x * 255.0 + 0.5).clamp(0, 255).trunc() / 255.0) if mode == "png" else (lambda x: (255.0 * x.clamp(0, 1)).trunc() / 255.0)
    got = run(dev, pred, gt, quantize=mode)
    assert torch.equal(got, run(dev, q(pred), q(gt)))
    assert not torch.equal(got, run(dev, pred, gt))


def test_quantised_accuracy(hip_device):
    pred, gt, ref, r = case("16x16", "png")
    value, taps, maps = run(hip_device, pred, gt, quantize="png", return_maps=True)
    keys = [f"map{l}" for l in range(5)]
    d = {k: (m.double().cpu() - w64).abs().max().item() for k, m, w64 in zip(keys, maps, ref["maps"])}
    assert_deviations("lpips", "16x16 png maps", d, dict(zip(keys, r)), keys)


def test_image_metrics_adds_lpips_and_changes_nothing_else(hip_device):
    from splatfields_amd import image_metrics
    dev = hip_device
    pred, gt, _, _ = case("37x53")
    p, g, w = pred.to(dev), gt.to(dev), weights_on(dev)
    for kw in (dict(), dict(quantize="png"), dict(quantize="png", return_frames=True)):
        plain, with_lpips = image_metrics(p, g, **kw), image_metrics(p, g, lpips=w, **kw)
        assert set(with_lpips) == set(plain) | {"lpips"}
        assert all(torch.equal(with_lpips[k], plain[k]) for k in plain)
        assert torch.equal(with_lpips["lpips"], run(dev, pred, gt, quantize=kw.get("quantize")))
    hwc = image_metrics(p[0].permute(1, 2, 0), g[0].permute(1, 2, 0), layout="hwc", lpips=w)
    assert hwc["lpips"].dim() == 0 and torch.equal(hwc["lpips"], run(dev, pred, gt)[0])


def test_eval_lpips_is_a_drop_in(hip_device):
    from splatfields_amd import eval_lpips
    dev = hip_device
    pred, gt, _, _ = case("64x48")
    img0, img1 = pred[0].permute(1, 2, 0).contiguous().to(dev), gt[0].permute(1, 2, 0).contiguous().to(dev)
    w = weights_on(dev)
    v = eval_lpips(img0, img1, w)
    assert v.dim() == 0 and v.dtype == torch.float32 and torch.equal(v, run(dev, pred, gt)[0])
    assert torch.equal(eval_lpips(img1, img0, w), v)         # symmetric

    class Module:                                            # anything with a state_dict() in the published layout
        calls = 0

        def state_dict(self):
            Module.calls += 1
            return w.state_dict()

    m = Module()
    assert torch.equal(eval_lpips(img0, img1, m), v) and torch.equal(eval_lpips(img0, img1, m), v) and Module.calls == 1


def test_identical_images_give_exactly_zero(hip_device):
    pred, gt, _, _ = case("37x53")
    value, taps, maps = run(hip_device, gt, gt, return_maps=True, quantize="png")
    assert (value == 0).all() and (taps == 0).all() and all((m == 0).all() for m in maps)


def test_refusals_come_before_any_launch(hip_device):
    from splatfields_amd import lpips_vgg
    from splatfields_amd.lpips import LPIPSWeights
    dev = hip_device
    w = weights_on(dev)
    x = torch.rand(2, 3, 16, 16, device=dev)
    raised = []

    def expect(exc, match, fn):
        with pytest.raises(exc, match=match):
            fn()
        raised.append(match)

    def all_of_them():
        expect(ValueError, "at least 16 x 16", lambda: lpips_vgg(x[:, :, :15], x[:, :, :15], w))
        expect(ValueError, "at least 16 x 16", lambda: lpips_vgg(x[:, :, :, :15], x[:, :, :, :15], w))
        expect(RuntimeError, "RGB images are required", lambda: lpips_vgg(x[:, :2], x[:, :2], w))
        expect(RuntimeError, "no CPU path", lambda: lpips_vgg(x.cpu(), x.cpu(), w))
        expect(RuntimeError, "the weights are on cpu", lambda: lpips_vgg(x, x, weights_cpu()))
        expect(ValueError, "lin 2 must have 256 weights", lambda: LPIPSWeights(w.convs, w.lins[:2] + [w.lins[2][:255]] + w.lins[3:]))
        expect(RuntimeError, "same shape", lambda: lpips_vgg(x, x[:1], w))
        expect(ValueError, "layout must be", lambda: lpips_vgg(x, x, w, layout="nhwc"))
        expect(ValueError, "quantize must be", lambda: lpips_vgg(x, x, w, quantize="jpeg"))

    names = device_records(all_of_them)
    assert len(raised) == 9 and not [n for n in names if "sr::" in n], names


def test_launch_budget(hip_device):
    """csrc/lpips.hip: 13 convolutions + 5 heads + 1 reduction = 19 library launches per chunk"""
    from splatfields_amd import _lib
    from splatfields_amd.lpips import LAUNCHES_PER_CHUNK
    dev = hip_device
    pred, gt, _, _ = case("64x48")
    p, g = pred.to(dev), gt.to(dev)
    weights_on(dev)
    one = _lib.load().sr_lpips_workspace_bytes(1, 64, 48)
    single = launches_per_iteration(lambda: run(dev, p[:1], g[:1]), 2)
    chunked = launches_per_iteration(lambda: run(dev, p, g, max_workspace_bytes=one), 2)
    whole = launches_per_iteration(lambda: run(dev, p, g, return_taps=True), 2)
    print("launches", single, chunked, whole)
    assert LAUNCHES_PER_CHUNK == 19
    assert single["library"] == 19 and chunked["library"] == 3 * 19 and whole["library"] == 19
    assert single["all"] == single["library"] and whole["all"] == whole["library"]        # nothing beside the library's kernels
