"""tests/metric_reference.py -- the PyTorch restatement the GPU tests and tools/metrics_bench.py measure the fused metrics
against -- reproduces the reference's own render.py (`compute_psnr`, `compute_ssim`) on every golden case
(tests/golden/metric_cases.npz) in float64; the kernel's tap literals and the 8-bit quantisation are pinned bit by bit."""
import os
import re
import struct

import numpy as np
import pytest
import torch

from tests import metric_reference as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = R.load_golden_cases()


def rel(a, b):
    a, b = torch.as_tensor(a).double(), torch.as_tensor(b).double()
    return ((a - b).abs().max() / b.abs().max().clamp_min(1e-300)).item()


def test_the_golden_set_has_the_cases_the_tolerance_is_derived_from():
    sizes = {(11, 11), (11, 64), (64, 11), (12, 30), (37, 53), (43, 75)}
    assert set(CASES) == {f"noise_{h}x{w}" for h, w in sizes} | {"near_equal", "grid8", "disc", "mask_random", "mask_hole",
                                                                  "mask_zero", "mask_one"}
    for h, w in sizes:
        c = CASES[f"noise_{h}x{w}"]
        assert tuple(c["pred"].shape) == (3, h, w) and "mask" not in c
    for name, c in CASES.items():
        assert c["pred"].dtype == torch.float32 and c["f64"]["ssim"].dtype == torch.float64 and c["f32"]["ssim"].dtype == torch.float32, name
    g = CASES["grid8"]
    assert torch.equal(g["pred"], R.quantize(g["pred"], "png")) and torch.equal(g["gt"], R.quantize(g["gt"], "png"))
    assert (CASES["near_equal"]["pred"] - CASES["near_equal"]["gt"]).abs().max() <= 1.01e-3
    frac = CASES["mask_random"]["mask"].mean().item()
    assert 0.6 < frac < 0.8 and set(CASES["mask_random"]["mask"].unique().tolist()) == {0.0, 1.0}
    hole = CASES["mask_hole"]["mask"]
    empty = torch.nn.functional.max_pool2d(hole[None, None], 11, stride=1) == 0      # windows without a mask pixel
    assert empty.any() and not empty.all()
    assert (CASES["mask_zero"]["mask"] == 0).all() and (CASES["mask_one"]["mask"] == 1).all()
    assert CASES["mask_zero"]["f64"]["ssim"].item() == 1.0 and CASES["mask_zero"]["f32"]["ssim"].item() == 1.0
    r = R.reference_error(CASES)
    print("reference float32 against float64 over all golden cases:", r)
    assert 0.0 < r["ssim"] < 1e-4 and 0.0 < r["psnr"] < 1e-4, r


@pytest.mark.parametrize("name", sorted(CASES))
def test_restatement_reproduces_the_reference_in_float64(name):
    c = CASES[name]
    got = R.evaluate(c["pred"], c["gt"], c.get("mask"), dtype=torch.float64)
    for k in ("psnr", "ssim"):
        assert got[k].dtype == torch.float64 and got[k].dim() == 0
        assert rel(got[k], c["f64"][k]) <= 1e-12, (name, k, rel(got[k], c["f64"][k]))
    # the per-channel form is the same squared error, channel by channel
    mse = 10.0 ** (-got["psnr_channels"] / 10.0)
    assert abs(-10.0 * torch.log10(mse.mean()).item() - got["psnr"].item()) <= 1e-10


def test_restatement_in_float32_is_as_close_as_the_reference_in_float32():
    """Not a tolerance of the product: a sanity check that the restatement's float32 rounding is of the reference's order."""
    r = R.reference_error(CASES)
    for name, c in CASES.items():
        d = R.deviations(R.evaluate(c["pred"], c["gt"], c.get("mask"), dtype=torch.float32), c["f64"])
        assert all(d[k] <= 4 * r[k] for k in R.METRICS), (name, d, r)


def test_batches_masks_and_the_degenerate_masks():
    a, b = CASES["mask_random"], CASES["near_equal"]
    pred, gt = torch.stack([a["pred"], b["pred"]]), torch.stack([a["gt"], b["gt"]])
    mask = torch.stack([a["mask"], torch.ones(37, 53)])
    got = R.evaluate(pred, gt, mask)
    assert tuple(got["psnr"].shape) == (2,) and tuple(got["psnr_channels"].shape) == (2, 3)
    for i, c in enumerate((a, b)):
        assert rel(got["ssim"][i], c["f64"]["ssim"]) <= 1e-12 and rel(got["psnr"][i], c["f64"]["psnr"]) <= 1e-12
    x, y = a["pred"], a["gt"]
    assert R.evaluate(x, y, torch.zeros(37, 53))["ssim"].item() == 1.0
    assert torch.equal(R.evaluate(x, y, torch.ones(37, 53))["ssim"], R.evaluate(x, y)["ssim"])
    assert R.evaluate(x, x)["psnr"].item() == float("inf") and (R.evaluate(x, x)["psnr_channels"] == float("inf")).all()
    with pytest.raises(ValueError):
        R.evaluate(x[:, :10], y[:, :10])


def test_kernel_taps_are_the_float32_filter_bit_for_bit():
    text = open(os.path.join(ROOT, "splatfields_amd", "csrc", "metrics.hip")).read()
    body = re.search(r"#define SR_METRIC_TAPS \{(.*?)\}", text, re.S).group(1).replace("\\", " ")
    taps = [float.fromhex(t.strip().rstrip("f")) for t in body.split(",")]
    want = R.filter_taps()
    assert len(taps) == R.TAPS and want.dtype == torch.float32
    assert [struct.pack("<f", t) for t in taps] == [struct.pack("<f", float(v)) for v in want]
    # not the window of the training loss: that one is evaluated through Python's math.exp and differs in the last bits
    from tests import loss_reference
    assert not torch.equal(want, loss_reference.window_taps())


def quantisation_probe():
    """levels, half-way points and their float32 neighbours, values outside [0, 1]"""
    k = torch.arange(0, 256, dtype=torch.float32)
    half = (k + 0.5) / 255.0
    pts = torch.cat([k / 255.0, half, torch.nextafter(half, torch.tensor(0.0)), torch.nextafter(half, torch.tensor(2.0)),
                     torch.tensor([-0.3, -1e-9, 0.0, 1.0, 1.0 + 1e-6, 1.7]), torch.rand(2000, generator=torch.Generator().manual_seed(1))])
    return pts[: 3 * (pts.numel() // 3)].reshape(3, 1, -1).contiguous()


def test_quantisation_is_the_torch_expression_exactly():
    x = quantisation_probe()
    # torchvision.utils.save_image's conversion, then eval_imgs' division
    png_bytes = x.clone().mul(255).add_(0.5).clamp_(0, 255).permute(1, 2, 0).to("cpu", torch.uint8).numpy()
    png = torch.from_numpy(png_bytes).float() / 255.
    assert torch.equal(R.quantize(x, "png"), png.permute(2, 0, 1)) and torch.equal(R.frames(x, "png"), torch.from_numpy(png_bytes))
    # render.py:282 on the numpy array
    to8b_bytes = (255 * np.clip(x.permute(1, 2, 0).numpy(), 0, 1)).astype(np.uint8)
    assert torch.equal(R.quantize(x, "to8b"), (torch.from_numpy(to8b_bytes).float() / 255.).permute(2, 0, 1))
    assert torch.equal(R.frames(x, "to8b"), torch.from_numpy(to8b_bytes))
    assert not np.array_equal(png_bytes, to8b_bytes)          # rounding against truncation
    for mode in ("png", "to8b"):                               # idempotent: the grid is a fixed point
        q = R.quantize(x, mode)
        assert torch.equal(R.quantize(q, "png"), q) and q.dtype == torch.float32
    assert R.quantize(x, None) is x
