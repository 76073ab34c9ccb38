"""The stand-alone SH stage restated in plain PyTorch (CPU, in the dtype of its inputs): the yardstick of csrc/sh.hip on
machines where the reference checkout is absent.  tests/test_sh_reference.py pins it to oracle.torch_oracle.sh_to_rgb and,
through tests/golden/sh_cases.npz, to the reference's own `eval_sh` + 0.5 + clamp (utils/sh_utils.py:57-112 as
extract_geo.py:40-44 calls it).  Model text only: nothing of the library is imported.

For splat positions means [N,3], coefficients shs [N,K,3], camera centres campos [V,3] and the active degree deg:

    dir_v   = normalize(mean - campos_v)
    pre_v   = sum_{k < (deg+1)^2} basis_k(dir_v) * shs[:, k] + 0.5          only the first (deg+1)^2 rows of shs are read
    colour  = max(pre, 0)        clamped where pre < 0        keep = 1 - clamped

The backward is the kernel's contract: it gets colour gradients that are ALREADY zero where the colour was clamped, and
returns scale * d/d(shs, means) of sum_v (pre_v * dcol_v).sum()."""
from __future__ import annotations

import torch

C0 = 0.28209479177387814
C1 = 0.4886025119029199
C2 = (1.0925484305920792, -1.0925484305920792, 0.31539156525252005, -1.0925484305920792, 0.5462742152960396)
C3 = (-0.5900435899266435, 2.890611442640554, -0.4570457994644658, 0.3731763325901154, -0.4570457994644658, 1.445305721320277,
      -0.5900435899266435)


def basis(d: torch.Tensor, deg: int) -> torch.Tensor:
    """[..., (deg+1)^2] real SH basis at unit directions d [..., 3]."""
    x, y, z = d[..., 0], d[..., 1], d[..., 2]
    cols = [torch.full_like(x, C0)]
    if deg > 0:
        cols += [-C1 * y, C1 * z, -C1 * x]
    if deg > 1:
        xx, yy, zz, xy, yz, xz = x * x, y * y, z * z, x * y, y * z, x * z
        cols += [C2[0] * xy, C2[1] * yz, C2[2] * (2.0 * zz - xx - yy), C2[3] * xz, C2[4] * (xx - yy)]
    if deg > 2:
        cols += [C3[0] * y * (3.0 * xx - yy), C3[1] * xy * z, C3[2] * y * (4.0 * zz - xx - yy), C3[3] * z * (2.0 * zz - 3.0 * xx - 3.0 * yy),
                 C3[4] * x * (4.0 * zz - xx - yy), C3[5] * z * (xx - yy), C3[6] * x * (xx - 3.0 * yy)]
    return torch.stack(cols, dim=-1)


def pre_clamp(means: torch.Tensor, shs: torch.Tensor, campos_views: torch.Tensor, deg: int) -> torch.Tensor:
    """pre [V,N,3]."""
    assert 0 <= deg <= 3 and shs.shape[1] >= (deg + 1) ** 2
    nb = (deg + 1) ** 2
    d = means[None, :, :] - campos_views.reshape(-1, 3)[:, None, :]
    d = d / d.norm(dim=-1, keepdim=True)
    return (basis(d, deg)[..., None] * shs[None, :, :nb, :]).sum(dim=2) + 0.5


def forward_views(means, shs, campos_views, deg):
    """-> (pre [V,N,3], colors = clamp_min(pre, 0), keep = pre >= 0)."""
    pre = pre_clamp(means, shs, campos_views, deg)
    return pre, pre.clamp_min(0.0), pre >= 0


def backward(means, shs, campos_views, dcol_masked, deg, scale=1.0):
    """-> (d_shs [N,K,3], d_means [N,3]) of scale * sum_v (pre_v * dcol_masked_v).sum(); rows k >= (deg+1)^2 of d_shs are zero,
    d_means is zero at degree 0 (no basis function depends on the direction)."""
    m = means.detach().clone().requires_grad_(True)
    s = shs.detach().clone().requires_grad_(True)
    pre = pre_clamp(m, s, campos_views.detach(), deg)
    total = scale * (pre * dcol_masked.detach().reshape(pre.shape).to(pre.dtype)).sum()
    d_shs, d_means = torch.autograd.grad(total, (s, m), allow_unused=True)
    return (d_shs if d_shs is not None else torch.zeros_like(s)), (d_means if d_means is not None else torch.zeros_like(m))


def clamp_bits(pre: torch.Tensor) -> torch.Tensor:
    """uint8 [...]: bit c (1 | 2 | 4) set where channel c of pre [..., 3] is below zero -- the `clamped` byte of sr_sh_forward."""
    return ((pre < 0).to(torch.uint8) * torch.tensor([1, 2, 4], dtype=torch.uint8)).sum(-1).to(torch.uint8)
