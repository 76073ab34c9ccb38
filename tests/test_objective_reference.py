"""tests/objective_reference.py -- the restatement the HIP objective is tested against -- checked on its own: hand-computed
cases, the equality the fused call rests on (the reference's per-view loop = view terms averaged + view-independent terms
once), and torch's gradient of the norm of a zero row."""
import math

import pytest
import torch

from splatfields_amd.losses import (centered_position_norm, depth_l1_loss, opacity_regularizer, position_norm,  # noqa: F401
                                    splat_regularizers, training_objective)      # what the restatement stands for
from tests import objective_reference as R

LAMBDAS = {"lambda_dssim": 0.2, "lambda_mask": 0.1, "lambda_norm": 0.01, "lambda_norm_mean": 0.02, "lambda_opacity": 0.03,
           "lambda_depthl1": 0.05, "lambda_gradient": 0.5}


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
def test_hand_computed_values(dtype):
    x = torch.tensor([[1.0, 2.0, 2.0], [-2.0, 3.0, -6.0], [0.0, 0.0, 0.0], [1.0, -2.0, 2.0]], dtype=dtype)
    assert R.position_norm(x).item() == (3 + 7 + 0 + 3) / 4
    # mean (0, 0.75, -0.5): rows minus it have lengths sqrt(1 + 1.5625 + 6.25), sqrt(4 + 5.0625 + 30.25), ...
    want = (math.sqrt(1 + 1.25 ** 2 + 2.5 ** 2) + math.sqrt(4 + 2.25 ** 2 + 5.5 ** 2) + math.sqrt(0.75 ** 2 + 0.5 ** 2)
            + math.sqrt(1 + 2.75 ** 2 + 2.5 ** 2)) / 4
    assert abs(R.centered_position_norm(x).item() - want) <= (1e-6 if dtype is torch.float32 else 1e-15)
    o = torch.tensor([[0.0], [0.5], [1.0], [0.5]], dtype=dtype)
    assert R.opacity_regularizer(o).item() == (1 + 0.25 + 0 + 0.25) / 4
    d = torch.tensor([[1.0, 2.0, 3.0], [4.0, 5.0, 6.0]], dtype=dtype)
    g = torch.tensor([[2.0, 0.0, 3.0], [-1.0, 1.0, 7.0]], dtype=dtype)
    # valid: (0,0) |1-2|, (0,2) 0, (1,1) 4, (1,2) 1; the two invalid pixels count in the divisor
    assert R.depth_l1(d, g).item() == (1 + 0 + 4 + 1) / 6
    out = R.depth_terms(d, g, dtype)
    assert torch.equal(out["d_depth"], torch.tensor([[-1.0, 0.0, 0.0], [0.0, 1.0, -1.0]], dtype=dtype) / 6)
    out = R.depth_terms(d[None].repeat(2, 1, 1), g[None].repeat(2, 1, 1), dtype, item_weights=torch.tensor([1.0, -2.0]))
    assert torch.equal(out["items"], torch.full((2,), 1.0, dtype=dtype))
    assert torch.equal(out["d_depth"][1], -2 * torch.tensor([[-1.0, 0.0, 0.0], [0.0, 1.0, -1.0]], dtype=dtype) / 6)


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
def test_gradients_of_the_splat_terms(dtype):
    x = torch.tensor([[1.0, 2.0, 2.0], [0.0, 0.0, 0.0], [2.0, 3.0, 6.0], [-1.0, -2.0, -2.0]], dtype=dtype)
    o = torch.tensor([[0.0], [0.5], [1.0], [0.25]], dtype=dtype)
    out = R.splat_terms(x, o, 1.0, 0.0, 1.0, dtype)
    want = torch.tensor([[1 / 3, 2 / 3, 2 / 3], [0.0, 0.0, 0.0], [2 / 7, 3 / 7, 6 / 7], [-1 / 3, -2 / 3, -2 / 3]], dtype=torch.float64) / 4
    assert (out["d_means3D"].double() - want).abs().max() <= (1e-7 if dtype is torch.float32 else 1e-16)
    assert torch.equal(out["d_means3D"][1], torch.zeros(3, dtype=dtype))       # the zero row: exactly 0, no NaN
    assert torch.equal(out["d_opacity"], 2 * (o - 1) / 4)
    assert "norm_mean" not in out and out["loss"].item() == out["norm"].item() + out["opacity"].item()
    # the mean is detached: the centred norm's gradient is the unit vector of (x - m) / N and nothing flows through m
    same = torch.tensor([[3.0, -1.0, 2.0]] * 5, dtype=dtype)
    out = R.splat_terms(same, None, 0.0, 1.0, 0.0, dtype)
    assert out["norm_mean"].item() == 0.0 and torch.equal(out["d_means3D"], torch.zeros(5, 3, dtype=dtype))
    pair = torch.tensor([[1.0, 0.0, 0.0], [-1.0, 0.0, 0.0]], dtype=dtype)
    out = R.splat_terms(pair, None, 0.0, 1.0, 0.0, dtype)
    assert out["norm_mean"].item() == 1.0 and torch.equal(out["d_means3D"], pair / 2)


@pytest.mark.parametrize("shapes", [[(16, 20)], [(16, 20)] * 3, [(16, 20), (12, 14)]])
def test_the_view_loop_equals_view_terms_averaged_plus_independent_terms_once(shapes):
    views, splats, gradient_error, extra = R.make_step(shapes, 50, seed=5)
    f64 = lambda t: t.double()
    vs = [{k: f64(t) for k, t in v.items()} for v in views]
    sp = {k: f64(t) for k, t in splats.items()}
    loop, _ = R.objective_loop(vs, sp, LAMBDAS, f64(gradient_error), f64(extra))
    once = R.objective_once(vs, sp, LAMBDAS, f64(gradient_error), f64(extra))
    assert abs(loop.item() - once.item()) <= 1e-14 * abs(loop.item())
    # ... and term by term the loop's dict is what the formulas say
    _, log = R.objective_loop(vs, sp, LAMBDAS, f64(gradient_error), f64(extra))
    assert abs(log["depthl1"].item() - sum(R.depth_l1(v["depth"][0], v["gt_depth"][0]).item() for v in vs) / len(vs)) <= 1e-15
    assert log["opacity"].item() == R.opacity_regularizer(sp["gaussian_opacity"]).item()
    assert log["loss_gradient"].item() == f64(gradient_error).item()


def test_terms_that_are_off_are_zero_in_the_dict_and_absent_from_the_loss():
    views, splats, gradient_error, extra = R.make_step([(16, 20)] * 2, 20, seed=6)
    off = {"lambda_dssim": 0.2}
    loss, log = R.objective_loop(views, splats, off, gradient_error, None)
    want = sum(R.photometric(v["image"], v["gt_image"], 0.2)[0] for v in views) / 2
    assert torch.equal(loss, want)
    assert all(log[k].item() == 0.0 for k in ("mask", "depthl1", "opacity", "loss_gradient"))
    out = R.evaluate_loop(views, splats, gradient_error, extra, LAMBDAS, torch.float64)
    assert len(out["grads"]["image"]) == 2 and out["grads"]["means3D"].shape == (20, 3)
    assert all(g is not None and g.abs().max() > 0 for g in out["grads"]["depth"] + out["grads"]["opacity"])
