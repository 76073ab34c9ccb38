"""Writes tests/golden/loss_cases.npz: the reference's own photometric loss (utils/loss_utils.py `l1_loss` / `ssim`, blended
as in train.py:183-193) on small inputs, evaluated in float64 AND in float32.  Run on a CPU where a reference checkout exists:

    python tests/golden/make_loss_golden.py /path/to/reference

Numeric arrays only travel.  Per case `<name>`:
    <name>/image, /gt [, /opacity, /gt_mask]         float32 inputs
    <name>/lambdas                                   [lambda_dssim, lambda_mask]
    <name>/f64/{l1, ssim, loss, d_image[, mask, d_opacity]}   and the same under /f32
and for the batched case also ssim_items ([B], size_average=False), item_weights and d_image_items = d(sum_b weights_b
ssim_items_b)/d image.  The float32 evaluation is the reference's own rounding error: the tolerance of the HIP kernels is
derived from its distance to the float64 one (tests/test_gpu_losses.py)."""
import os
import sys

import numpy as np
import torch
import torch.nn.functional as F

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
from loss_reference import blob_scene  # noqa: E402  (input construction only)


def reference_eval(ref, image, gt, opacity, gt_mask, lambda_dssim, lambda_mask, dtype):
    x = image.to(dtype).clone().requires_grad_(True)
    y = gt.to(dtype)
    l1 = ref.l1_loss(x, y)
    s = ref.ssim(x, y)
    loss = (1.0 - lambda_dssim) * l1 + lambda_dssim * (1.0 - s)
    out = {}
    a = None
    if opacity is not None:
        a = opacity.to(dtype).clone().requires_grad_(True)
        m = F.l1_loss(torch.clamp(a, 0.0, 1.0).view(-1), gt_mask.to(dtype).view(-1))
        loss = loss + lambda_mask * m
        out["mask"] = m
    loss.backward()
    out.update(l1=l1, ssim=s, loss=loss, d_image=x.grad)
    if a is not None:
        out["d_opacity"] = a.grad
    return {k: v.detach().numpy().copy() for k, v in out.items()}


def cases():
    gen = torch.Generator().manual_seed(20240607)
    rand = lambda *s: torch.rand(*s, generator=gen)
    out = {}
    # noise, with the mask term: opacities outside [0, 1] and exactly 0 / 1
    op = rand(1, 37, 53) * 1.4 - 0.2
    op[0, ::5, ::7] = 0.0
    op[0, 2::5, 3::7] = 1.0
    out["noise"] = (rand(3, 37, 53), rand(3, 37, 53), op, (rand(1, 37, 53) > 0.5).float(), 0.2, 0.1)
    out["blob_black"] = blob_scene(32, 40, 0.0, seed=1) + (0.2, 0.1)
    p, t, _, _ = blob_scene(32, 40, 1.0, seed=2)
    out["blob_white"] = (p, t, None, None, 0.2, 0.0)
    t = 0.2 + 0.6 * rand(3, 24, 36)
    out["near_equal"] = ((t + 1e-3 * (2 * rand(3, 24, 36) - 1)), t, None, None, 0.2, 0.0)
    out["one_channel"] = (rand(1, 64, 48), rand(1, 64, 48), None, None, 0.2, 0.0)
    out["tiny"] = (rand(3, 7, 9), rand(3, 7, 9), rand(1, 7, 9), (rand(1, 7, 9) > 0.5).float(), 0.2, 0.1)
    out["batch"] = (rand(2, 3, 24, 40), rand(2, 3, 24, 40), None, None, 0.2, 0.0)
    d = 1.0 + 4.0 * rand(33, 29, 1)                       # the depth call of train.py:221: [H, W, 1]
    out["depth_hw1"] = (d + 0.2 * (rand(33, 29, 1) - 0.5), d, None, None, 0.2, 0.0)
    return out


def main():
    if len(sys.argv) != 2:
        sys.exit(__doc__)
    sys.path.insert(0, sys.argv[1])
    from utils import loss_utils as ref
    torch.set_num_threads(1)
    arrays = {}
    for name, (image, gt, opacity, gt_mask, lam, lam_mask) in cases().items():
        image, gt = image.float().contiguous(), gt.float().contiguous()
        arrays[f"{name}/image"], arrays[f"{name}/gt"] = image.numpy(), gt.numpy()
        arrays[f"{name}/lambdas"] = np.array([lam, lam_mask], dtype=np.float64)
        if opacity is not None:
            arrays[f"{name}/opacity"], arrays[f"{name}/gt_mask"] = opacity.float().numpy(), gt_mask.float().numpy()
        for tag, dtype in (("f64", torch.float64), ("f32", torch.float32)):
            for k, v in reference_eval(ref, image, gt, opacity, gt_mask, lam, lam_mask, dtype).items():
                arrays[f"{name}/{tag}/{k}"] = v
            if name == "batch":
                weights = torch.tensor([1.0, 0.5])
                x = image.to(dtype).clone().requires_grad_(True)
                items = ref.ssim(x, gt.to(dtype), size_average=False)
                (items * weights.to(dtype)).sum().backward()
                arrays[f"{name}/{tag}/ssim_items"] = items.detach().numpy().copy()
                arrays[f"{name}/{tag}/d_image_items"] = x.grad.numpy().copy()
                arrays[f"{name}/item_weights"] = weights.numpy()
    path = os.path.join(HERE, "loss_cases.npz")
    np.savez_compressed(path, **arrays)
    print(path, os.path.getsize(path), "bytes,", len(arrays), "arrays")


if __name__ == "__main__":
    main()
