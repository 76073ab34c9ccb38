"""Writes tests/golden/metric_cases.npz: the reference's own evaluation metrics (render.py `compute_psnr`, `compute_ssim`) on
small inputs, evaluated in float64 AND in float32.  Run on a CPU where a reference checkout and scipy exist:

    python tests/golden/make_metric_golden.py /path/to/reference

render.py itself cannot be imported without the reference's whole environment (torchvision, lpips, imageio, cv2, a scene), so
only the two function definitions are compiled out of the file, with `ast`, into a namespace that holds what they name: torch,
math, typing.Optional and scipy.signal.  Nothing of the reference's text is copied.

Numeric arrays only travel.  Per case `<name>` (tests/metric_reference.py `golden_inputs`):
    <name>/pred, /gt  [3,H,W] float32        [<name>/mask  [H,W] float32]
    <name>/f64/{psnr, ssim}  and the same under /f32
The reference takes [H,W,3] images and an [H,W,1] mask: the inputs are permuted on the way in.  The float32 evaluation is the
reference's own rounding error: the tolerance of the HIP kernel is derived from its distance to the float64 one
(tests/test_gpu_metrics.py)."""
import ast
import math
import os
import sys
from typing import Optional

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
from metric_reference import golden_inputs  # noqa: E402  (input construction only)


def reference_functions(reference_root):
    from scipy import signal
    path = os.path.join(reference_root, "render.py")
    tree = ast.parse(open(path).read(), filename=path)
    wanted = ("compute_psnr", "compute_ssim")
    tree.body = [node for node in tree.body if isinstance(node, ast.FunctionDef) and node.name in wanted]
    assert [node.name for node in tree.body] == list(wanted)
    space = {"torch": torch, "math": math, "Optional": Optional, "signal": signal}
    exec(compile(tree, path, "exec"), space)
    return space["compute_psnr"], space["compute_ssim"]


def main():
    if len(sys.argv) != 2:
        sys.exit(__doc__)
    compute_psnr, compute_ssim = reference_functions(sys.argv[1])
    torch.set_num_threads(1)
    arrays = {}
    for name, (pred, gt, mask) in golden_inputs().items():
        arrays[f"{name}/pred"], arrays[f"{name}/gt"] = pred.numpy(), gt.numpy()
        if mask is not None:
            arrays[f"{name}/mask"] = mask.float().numpy()
        for tag, dtype in (("f64", torch.float64), ("f32", torch.float32)):
            a, b = pred.permute(1, 2, 0).to(dtype).contiguous(), gt.permute(1, 2, 0).to(dtype).contiguous()
            m = None if mask is None else mask[..., None].to(dtype)
            arrays[f"{name}/{tag}/psnr"] = compute_psnr(a, b).numpy().copy()
            arrays[f"{name}/{tag}/ssim"] = compute_ssim(a, b, m).numpy().copy()
            print(name, tag, arrays[f"{name}/{tag}/psnr"], arrays[f"{name}/{tag}/ssim"], arrays[f"{name}/{tag}/ssim"].dtype)
    path = os.path.join(HERE, "metric_cases.npz")
    np.savez_compressed(path, **arrays)
    print(path, os.path.getsize(path), "bytes,", len(arrays), "arrays")


if __name__ == "__main__":
    main()
