"""tests/lpips_reference.py (the restatement the GPU tests of LPIPS compare with) against an independent direct evaluation in
numpy with explicit loops over the window's taps, the properties the formula promises, and LPIPSWeights' state-dict layout."""
import numpy as np
import pytest
import torch

from tests import lpips_reference as R


@pytest.fixture(scope="module")
def weights():
    from splatfields_amd.lpips import LPIPSWeights
    return LPIPSWeights.random(3)


def direct_numpy(pred, gt, convs, lins, shift, scale):
    """float64, nothing shared with the restatement: loops over the 9 taps, the pool by reshaping, the head per tap"""
    def conv(x, w, b):
        c, h, wd = x.shape
        xp = np.zeros((c, h + 2, wd + 2))
        xp[:, 1:-1, 1:-1] = x
        out = np.zeros((w.shape[0], h, wd)) + b[:, None, None]
        for ky in range(3):
            for kx in range(3):
                out += np.einsum("oc,chw->ohw", w[:, :, ky, kx], xp[:, ky:ky + h, kx:kx + wd])
        return np.maximum(out, 0.0)

    def features(img):
        x = ((img * 2.0 - 1.0) - shift[:, None, None]) / scale[:, None, None]
        taps, layer = [], 0
        for g, n in enumerate(R.GROUPS):
            if g:
                c, h, wd = x.shape
                x = x[:, :h // 2 * 2, :wd // 2 * 2].reshape(c, h // 2, 2, wd // 2, 2).max(axis=(2, 4))
            for _ in range(n):
                x = conv(x, *convs[layer])
                layer += 1
            taps.append(x)
        return taps

    values, all_taps = [], []
    for p, g in zip(pred, gt):
        taps = []
        for f0, f1, lin in zip(features(p), features(g), lins):
            n0 = f0 / (np.sqrt((f0 ** 2).sum(0, keepdims=True)) + 1e-10)
            n1 = f1 / (np.sqrt((f1 ** 2).sum(0, keepdims=True)) + 1e-10)
            taps.append(float(((n0 - n1) ** 2 * lin[:, None, None]).sum(0).mean()))
        all_taps.append(taps)
        values.append(sum(taps))
    return np.array(values), np.array(all_taps)


def test_restatement_against_direct_numpy_evaluation(weights):
    convs, lins, shift, scale = R.parts(weights)
    pred, gt = R.images(2, 16, 16, seed=1)
    want_v, want_t = direct_numpy(pred.double().numpy(), gt.double().numpy(), [(w.double().numpy(), b.double().numpy()) for w, b in convs],
                                  [v.double().numpy() for v in lins], shift.double().numpy(), scale.double().numpy())
    for order in R.ORDERS:
        got = R.evaluate(pred, gt, convs, lins, shift, scale, torch.float64, order)
        assert [tuple(m.shape) for m in got["maps"]] == [(2, 16, 16), (2, 8, 8), (2, 4, 4), (2, 2, 2), (2, 1, 1)]
        dv, dt = np.abs(got["value"].numpy() - want_v).max(), np.abs(got["taps"].numpy() - want_t).max()
        print(order, "value", dv, "taps", dt, "values", want_v)
        assert dv <= 1e-12 and dt <= 1e-12 and (want_v > 1e-3).all()


def test_identical_images_symmetry_and_batch_independence(weights):
    convs, lins, shift, scale = R.parts(weights)
    pred, gt = R.images(3, 20, 24, seed=2)
    for dtype in (torch.float64, torch.float32):
        same = R.evaluate(gt, gt, convs, lins, shift, scale, dtype)
        assert (same["value"] == 0).all() and all((m == 0).all() for m in same["maps"])
        a, b = R.evaluate(pred, gt, convs, lins, shift, scale, dtype), R.evaluate(gt, pred, convs, lins, shift, scale, dtype)
        assert torch.equal(a["value"], b["value"]) and torch.equal(a["taps"], b["taps"])
    whole = R.evaluate(pred, gt, convs, lins, shift, scale, torch.float64)
    for i in range(3):
        one = R.evaluate(pred[i:i + 1], gt[i:i + 1], convs, lins, shift, scale, torch.float64)
        assert (one["value"] - whole["value"][i:i + 1]).abs().max() <= 1e-13
        assert (one["taps"] - whole["taps"][i:i + 1]).abs().max() <= 1e-13


def test_pooling_floors_on_odd_sizes(weights):
    convs, lins, shift, scale = R.parts(weights)
    pred, gt = R.images(1, 37, 53, seed=3)
    got = R.evaluate(pred, gt, convs, lins, shift, scale, torch.float64)
    assert [tuple(m.shape[1:]) for m in got["maps"]] == [(37, 53), (18, 26), (9, 13), (4, 6), (2, 3)]
    # 17 x 19 -> 8 x 9 -> 4 x 4 -> 2 x 2 -> 1 x 1 against the direct evaluation, which crops to even sizes before it pools
    pred, gt = R.images(1, 17, 19, seed=4)
    want_v, want_t = direct_numpy(pred.double().numpy(), gt.double().numpy(), [(w.double().numpy(), b.double().numpy()) for w, b in convs],
                                  [v.double().numpy() for v in lins], shift.double().numpy(), scale.double().numpy())
    got = R.evaluate(pred, gt, convs, lins, shift, scale, torch.float64)
    assert [tuple(m.shape[1:]) for m in got["maps"]] == [(17, 19), (8, 9), (4, 4), (2, 2), (1, 1)]
    assert np.abs(got["taps"].numpy() - want_t).max() <= 1e-12 and np.abs(got["value"].numpy() - want_v).max() <= 1e-12


def test_quantisation_is_applied_before_the_network(weights):
    convs, lins, shift, scale = R.parts(weights)
    pred, gt = R.images(1, 16, 16, seed=5)
    q = R.evaluate(pred, gt, convs, lins, shift, scale, torch.float64, quantize="png")
    pre = R.evaluate(R.quantise(pred, "png"), R.quantise(gt, "png"), convs, lins, shift, scale, torch.float64)
    assert torch.equal(q["value"], pre["value"])
    assert not torch.equal(q["value"], R.evaluate(pred, gt, convs, lins, shift, scale, torch.float64)["value"])


def test_float32_orders_agree_on_the_size_of_their_error(weights):
    """the allowance of the GPU tests (4 x the larger float32 error) does not hinge on one library's summation order"""
    convs, lins, shift, scale = R.parts(weights)
    pred, gt = R.images(2, 16, 16, seed=6)
    ref = R.evaluate(pred, gt, convs, lins, shift, scale, torch.float64)
    errs = {o: [(m.double() - w).abs().max().item() for m, w in zip(R.evaluate(pred, gt, convs, lins, shift, scale, torch.float32, o)["maps"],
                                                                     ref["maps"])] for o in R.ORDERS}
    print(errs)
    for a, b in zip(errs["conv2d"], errs["chunked"]):
        assert 0 < a and 0 < b and max(a, b) / min(a, b) < 8.0


def test_random_weights_follow_the_recipe():
    from splatfields_amd.lpips import CONV_CHANNELS, TAP_CHANNELS, LPIPSWeights
    a, b = LPIPSWeights.random(7), LPIPSWeights.random(7)
    assert all(torch.equal(x[0], y[0]) and torch.equal(x[1], y[1]) for x, y in zip(a.convs, b.convs))
    assert not torch.equal(a.convs[0][0], LPIPSWeights.random(8).convs[0][0])
    for (w, bias), (cin, cout) in zip(a.convs, CONV_CHANNELS):
        assert tuple(w.shape) == (cout, cin, 3, 3) and tuple(bias.shape) == (cout,)
        if cin >= 64:
            assert abs(w.var().item() * 9 * cin / 2.0 - 1.0) < 0.05
    for v, c in zip(a.lins, TAP_CHANNELS):
        assert tuple(v.shape) == (c,) and 0 <= v.min() and v.max() <= 4.0 / c
    assert torch.equal(a.shift, torch.tensor([-.030, -.088, -.188])) and torch.equal(a.scale, torch.tensor([.458, .448, .450]))


def test_state_dict_round_trip_and_refusals(weights):
    from splatfields_amd.lpips import LIN_KEYS, TRUNK_KEYS, LPIPSWeights
    sd = weights.state_dict()
    assert set(sd) == {k + s for k in TRUNK_KEYS for s in (".weight", ".bias")} | set(LIN_KEYS) | {"scaling_layer.shift", "scaling_layer.scale"}
    assert TRUNK_KEYS[0] == "net.slice1.0" and TRUNK_KEYS[6] == "net.slice3.14" and TRUNK_KEYS[12] == "net.slice5.28"
    assert tuple(sd["lin3.model.1.weight"].shape) == (1, 512, 1, 1) and tuple(sd["scaling_layer.shift"].shape) == (1, 3, 1, 1)
    back = LPIPSWeights.from_state_dict(sd)
    assert all(torch.equal(x[0], y[0]) and torch.equal(x[1], y[1]) for x, y in zip(back.convs, weights.convs))
    assert all(torch.equal(x, y) for x, y in zip(back.lins, weights.lins))
    assert torch.equal(back.shift, weights.shift) and torch.equal(back.scale, weights.scale)
    missing = {k: v for k, v in sd.items() if k not in ("net.slice3.12.bias", "lin4.model.1.weight")}
    with pytest.raises(KeyError, match=r"net\.slice3\.12\.bias, lin4\.model\.1\.weight"):
        LPIPSWeights.from_state_dict(missing)
    wrong = dict(sd)
    wrong["net.slice2.5.weight"] = sd["net.slice2.5.weight"][:, :32]
    with pytest.raises(ValueError, match=r"convolution 2 must be \[128,64,3,3\]"):
        LPIPSWeights.from_state_dict(wrong)
    wrong = dict(sd)
    wrong["lin1.model.1.weight"] = sd["lin1.model.1.weight"][:, :64]
    with pytest.raises(ValueError, match="lin 1 must have 128 weights"):
        LPIPSWeights.from_state_dict(wrong)
    with pytest.raises(ValueError, match="13"):
        LPIPSWeights(weights.convs[:12], weights.lins)
    assert "unverified" in LPIPSWeights.from_state_dict.__doc__


def test_facade_has_no_cpu_path(weights):
    import splatfields_amd as S
    pred, gt = R.images(1, 16, 16, seed=1)
    for fn in (lambda: S.lpips_vgg(pred, gt, weights), lambda: S.eval_lpips(pred[0].permute(1, 2, 0), gt[0].permute(1, 2, 0), weights),
               lambda: S.image_metrics(pred, gt, lpips=weights)):
        with pytest.raises(RuntimeError, match="no CPU path"):
            fn()
    with pytest.raises(RuntimeError, match="no CPU path"):
        weights.packed()


def test_flop_count_of_the_benchmark():
    """tools/lpips_bench.py: 2 x 9 x cin x cout x pixels over the 13 layers, 0.39 TFLOP per 800 x 800 image"""
    from splatfields_amd.lpips import CONV_CHANNELS
    from tools import lpips_bench as B
    assert B.CONVS == CONV_CHANNELS and len(B.GROUP_OF) == 13 and [B.GROUP_OF.count(g) for g in range(5)] == list(R.GROUPS)
    assert B.conv_flops(800, 800) == 391_495_680_000 and B.conv_flops(800, 800, 2) == 2 * B.conv_flops(800, 800)
    assert B.conv_flops(16, 16) == 2 * 9 * (256 * (3 * 64 + 64 * 64) + 64 * (64 * 128 + 128 * 128) + 16 * (128 * 256 + 2 * 256 * 256)
                                            + 4 * (256 * 512 + 2 * 512 * 512) + 3 * 512 * 512)
