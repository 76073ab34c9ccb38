"""tests/loss_reference.py -- the PyTorch restatement the GPU tests and tools/loss_bench.py measure the fused loss against --
reproduces the reference's own utils/loss_utils.py on every golden case (tests/golden/loss_cases.npz) in float64."""
import os
import re
import struct

import pytest
import torch

from tests import loss_reference as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = R.load_golden_cases()


def rel(a, b):
    a, b = torch.as_tensor(a).double(), torch.as_tensor(b).double()
    return ((a - b).abs().max() / b.abs().max().clamp_min(1e-300)).item()


def test_the_golden_set_has_the_cases_the_tolerance_is_derived_from():
    assert set(CASES) == {"noise", "blob_black", "blob_white", "near_equal", "one_channel", "tiny", "batch", "depth_hw1"}
    assert tuple(CASES["tiny"]["image"].shape) == (3, 7, 9) and tuple(CASES["depth_hw1"]["image"].shape) == (33, 29, 1)
    for name in ("blob_black", "blob_white"):    # flat background, prediction exactly equal to the target there
        c = CASES[name]
        assert (c["image"] == c["gt"]).float().mean() > 0.2
    for name in ("noise", "blob_black"):         # opacities exactly 0 and 1, and outside [0, 1]
        a = CASES[name]["opacity"]
        assert (a == 0).any() and (a == 1).any() and (a < 0).any() and (a > 1).any()
    r = R.reference_error(CASES)
    print("reference float32 against float64 over all golden cases:", r)
    assert all(0.0 < v < 1e-2 for v in r.values()), r


@pytest.mark.parametrize("name", sorted(CASES))
def test_restatement_reproduces_the_reference_in_float64(name):
    c = CASES[name]
    lam, lam_mask = c["lambdas"].tolist()
    got = R.evaluate(c["image"], c["gt"], c.get("opacity"), c.get("gt_mask"), lam, lam_mask, dtype=torch.float64)
    want = c["f64"]
    for k in got:
        assert got[k].dtype == torch.float64 and rel(got[k], want[k]) <= 1e-12, (name, k, rel(got[k], want[k]))
    assert ("d_opacity" in want) == ("opacity" in c) == ("d_opacity" in got)
    if name == "batch":
        x = c["image"].double().requires_grad_(True)
        items = R.ssim(x, c["gt"].double(), size_average=False)
        (items * c["item_weights"].double()).sum().backward()
        assert rel(items.detach(), want["ssim_items"]) <= 1e-12 and rel(x.grad, want["d_image_items"]) <= 1e-12


def test_restatement_in_float32_is_as_close_as_the_reference_in_float32():
    """Not a tolerance of the product: a sanity check that the restatement's float32 rounding is of the reference's order."""
    r = R.reference_error(CASES)
    for name, c in CASES.items():
        lam, lam_mask = c["lambdas"].tolist()
        got = R.evaluate(c["image"], c["gt"], c.get("opacity"), c.get("gt_mask"), lam, lam_mask, dtype=torch.float32)
        d = R.deviations(got, c["f64"])
        assert all(d[k] <= 4 * r[k] for k in R.METRICS), (name, d, r)


def test_kernel_taps_are_the_float32_window_bit_for_bit():
    text = open(os.path.join(ROOT, "splatfields_amd", "csrc", "loss.hip")).read()
    body = re.search(r"#define SR_LOSS_TAPS \{(.*?)\}", text, re.S).group(1).replace("\\", " ")
    taps = [float.fromhex(t.strip().rstrip("f")) for t in body.split(",")]
    want = R.window_taps()
    assert len(taps) == R.TAPS
    assert [struct.pack("<f", t) for t in taps] == [struct.pack("<f", float(v)) for v in want]
