"""The tail of the reference's training objective restated in torch, parametrised by dtype: what the HIP kernels of
csrc/objective.hip and splatfields_amd.losses.training_objective are tested against (in float64) and what their tolerance is
taken from (the same expressions in float32).

Each function is the reference's expression, line for line; `objective_loop` is the literal per-view loop of train.py:165-250
with the photometric part (train.py:183-193, restated in tests/loss_reference.py and pinned to the reference there) inside.
Not restated: the depth "SSIM" of train.py:217-222 and `lambda_corr_color` ("Training objective")."""
from __future__ import annotations

import torch
import torch.nn.functional as F

from tests import loss_reference as L


def position_norm(means3D):
    """train.py:196  `gaussian_dict['means3D'].norm(dim=1).mean()`"""
    return means3D.norm(dim=1).mean()


def centered_position_norm(means3D):
    """train.py:199-200  `mean_val = means3D.detach().mean(dim=0, keepdim=True)`, `(means3D - mean_val).norm(dim=1).mean()`"""
    mean_val = means3D.detach().mean(dim=0, keepdim=True)
    return (means3D - mean_val).norm(dim=1).mean()


def opacity_regularizer(gaussian_opacity):
    """train.py:245  `((gaussian_dict['gaussian_opacity'] - 1.0)**2).mean()`"""
    return ((gaussian_opacity - 1.0) ** 2).mean()


def depth_l1(rnd_depth, gt_depth):
    """train.py:225-228  `_dmask = gt_depth > 0`, `F.l1_loss((rnd_depth*_dmask).unsqueeze(-1), (gt_depth*_dmask).unsqueeze(-1))`"""
    _dmask = gt_depth > 0
    return F.l1_loss((rnd_depth * _dmask).unsqueeze(-1), (gt_depth * _dmask).unsqueeze(-1))


def splat_terms(means3D, opacity, lambda_norm, lambda_norm_mean, lambda_opacity, dtype):
    """The weighted sum of the three splat terms and each term, with gradients: {"loss", "norm", "norm_mean", "opacity",
    "d_means3D", "d_opacity"} (entries of terms with weight 0 are missing)."""
    x = None if means3D is None else means3D.detach().to(dtype).requires_grad_(True)
    o = None if opacity is None else opacity.detach().to(dtype).requires_grad_(True)
    out, loss = {}, 0.0
    if lambda_norm != 0.0:
        out["norm"] = position_norm(x)
        loss = loss + lambda_norm * out["norm"]
    if lambda_norm_mean != 0.0:
        out["norm_mean"] = centered_position_norm(x)
        loss = loss + lambda_norm_mean * out["norm_mean"]
    if lambda_opacity != 0.0:
        out["opacity"] = opacity_regularizer(o)
        loss = loss + lambda_opacity * out["opacity"]
    loss.backward()
    out = {k: v.detach() for k, v in out.items()}
    out["loss"] = loss.detach()
    if x is not None and x.grad is not None:
        out["d_means3D"] = x.grad
    if o is not None and o.grad is not None:
        out["d_opacity"] = o.grad
    return out


def depth_terms(depth, gt_depth, dtype, item_weights=None):
    """{"depthl1", "d_depth"}; with item_weights [B]: {"items" [B], "d_depth" of sum_b w_b item_b}."""
    d = depth.detach().to(dtype).requires_grad_(True)
    g = gt_depth.detach().to(dtype)
    if item_weights is None:
        value = depth_l1(d, g)
        value.backward()
        return {"depthl1": value.detach(), "d_depth": d.grad}
    items = torch.stack([depth_l1(d[b], g[b]) for b in range(d.shape[0])])
    (items * item_weights.to(dtype)).sum().backward()
    return {"items": items.detach(), "d_depth": d.grad}


def photometric(image, gt_image, lambda_dssim):
    """train.py:183-184"""
    Ll1 = L.l1(image, gt_image)
    return (1.0 - lambda_dssim) * Ll1 + lambda_dssim * (1.0 - L.ssim(image, gt_image)), Ll1


def objective_loop(views, gaussian_dict, lam, gradient_error=None, extra=None):
    """The literal loop of train.py:165-250 over `views`, a list of dicts {"image", "gt_image", "opacity", "gt_mask", "depth",
    "gt_depth"} of one dtype; `lam` holds the weights.  Returns (loss, loss_dict) as train.py:242-264 builds them; loss_dict
    also carries "Ll1" = sum(Ll1_list) / len(Ll1_list)."""
    zero = lambda: torch.zeros((), dtype=views[0]["image"].dtype)
    loss_list, Ll1_list, loss_mask_list, loss_depthl1_list = [], [], [], []
    for view in views:
        image, gt_image = view["image"], view["gt_image"]
        _loss, _Ll1 = photometric(image, gt_image, lam["lambda_dssim"])
        _loss_mask, _loss_depthl1 = zero(), zero()
        if lam.get("lambda_mask", 0.0) > 0.0:
            opacity_image = torch.clamp(view["opacity"], 0.0, 1.0)
            _loss_mask = F.l1_loss(opacity_image.view(-1), view["gt_mask"].view(-1))
            _loss = _loss + lam["lambda_mask"] * _loss_mask
        if lam.get("lambda_norm", 0.0) > 0.0:
            _loss = _loss + lam["lambda_norm"] * position_norm(gaussian_dict["means3D"])
        if lam.get("lambda_norm_mean", 0.0) > 0.0:
            _loss = _loss + lam["lambda_norm_mean"] * centered_position_norm(gaussian_dict["means3D"])
        if lam.get("lambda_depthl1", 0.0) > 0.0:
            gt_depth = view["gt_depth"].squeeze()
            rnd_depth = view["depth"].squeeze()
            _loss_depthl1 = depth_l1(rnd_depth, gt_depth)
            _loss = _loss + lam["lambda_depthl1"] * _loss_depthl1
        loss_list.append(_loss)
        Ll1_list.append(_Ll1)
        loss_mask_list.append(_loss_mask)
        loss_depthl1_list.append(_loss_depthl1)
    loss = sum(loss_list) / len(loss_list)
    loss_opacity = zero()
    if lam.get("lambda_opacity", 0.0) > 0.0:
        loss_opacity = opacity_regularizer(gaussian_dict["gaussian_opacity"])
        loss = loss + lam["lambda_opacity"] * loss_opacity
    loss_gradient = zero()
    if lam.get("lambda_gradient", 0.0) > 0.0 and gradient_error is not None:
        loss_gradient = gradient_error
        loss = loss + lam["lambda_gradient"] * loss_gradient
    if extra is not None:           # the caller's lambda_corr * moran term: view-independent, added once
        loss = loss + extra
    loss_dict = {"Ll1": (sum(Ll1_list) / len(Ll1_list)).detach(), "mask": (sum(loss_mask_list) / len(loss_mask_list)).detach(),
                 "depthl1": (sum(loss_depthl1_list) / len(loss_depthl1_list)).detach(), "opacity": loss_opacity.detach(),
                 "loss_gradient": loss_gradient.detach()}
    return loss, loss_dict


def objective_once(views, gaussian_dict, lam, gradient_error=None, extra=None):
    """The same objective with the view terms averaged and every view-independent term evaluated ONCE: the form
    training_objective computes."""
    n = len(views)
    loss = 0.0
    for view in views:
        _loss, _ = photometric(view["image"], view["gt_image"], lam["lambda_dssim"])
        if lam.get("lambda_mask", 0.0) > 0.0:
            _loss = _loss + lam["lambda_mask"] * F.l1_loss(torch.clamp(view["opacity"], 0.0, 1.0).view(-1), view["gt_mask"].view(-1))
        if lam.get("lambda_depthl1", 0.0) > 0.0:
            _loss = _loss + lam["lambda_depthl1"] * depth_l1(view["depth"].squeeze(), view["gt_depth"].squeeze())
        loss = loss + _loss / n
    if lam.get("lambda_norm", 0.0) > 0.0:
        loss = loss + lam["lambda_norm"] * position_norm(gaussian_dict["means3D"])
    if lam.get("lambda_norm_mean", 0.0) > 0.0:
        loss = loss + lam["lambda_norm_mean"] * centered_position_norm(gaussian_dict["means3D"])
    if lam.get("lambda_opacity", 0.0) > 0.0:
        loss = loss + lam["lambda_opacity"] * opacity_regularizer(gaussian_dict["gaussian_opacity"])
    if lam.get("lambda_gradient", 0.0) > 0.0 and gradient_error is not None:
        loss = loss + lam["lambda_gradient"] * gradient_error
    if extra is not None:
        loss = loss + extra
    return loss


LEAVES = ("image", "opacity", "depth")


def make_step(shapes, n_splats, seed):
    """A seeded step: per view (height, width) of `shapes` a render, a target, an opacity image that leaves [0, 1] in places,
    a binary mask, a rendered depth and a target depth with about 40 % zeros and some negative values; means3D and opacities
    of n_splats splats, a gradient_error scalar and an `extra` scalar.  float32 CPU tensors."""
    gen = torch.Generator().manual_seed(seed)
    rand = lambda *s: torch.rand(*s, generator=gen)
    views = []
    for h, w in shapes:
        gt_depth = rand(h, w) * 4.0 + 0.5
        pick = rand(h, w)
        gt_depth = torch.where(pick < 0.4, torch.zeros(()), torch.where(pick < 0.45, -gt_depth, gt_depth))
        views.append({"image": rand(3, h, w), "gt_image": rand(3, h, w), "opacity": rand(1, h, w) * 1.2 - 0.1,
                      "gt_mask": (rand(1, h, w) > 0.5).float(), "depth": rand(1, h, w) * 4.0 + 0.5, "gt_depth": gt_depth[None]})
    splats = {"means3D": torch.randn(n_splats, 3, generator=gen) * 1.3, "gaussian_opacity": rand(n_splats, 1)}
    return views, splats, rand(()) * 0.1, rand(()) * 0.05


def evaluate_loop(views, splats, gradient_error, extra, lam, dtype):
    """The literal loop in `dtype` with gradients: {"loss", "log": {...}, "grads": {"image": [V], "opacity": [V], "depth": [V],
    "means3D", "gaussian_opacity"}}."""
    leaf = lambda t: t.detach().clone().to(dtype).requires_grad_(True)       # never the caller's tensor itself
    vs = [{k: (leaf(t) if k in LEAVES else t.to(dtype)) for k, t in v.items()} for v in views]
    sp = {k: leaf(t) for k, t in splats.items()}
    loss, log = objective_loop(vs, sp, lam, gradient_error.to(dtype), extra.to(dtype))
    loss.backward()
    grads = {k: [v[k].grad for v in vs] for k in LEAVES}
    grads.update({k: t.grad for k, t in sp.items()})
    return {"loss": loss.detach(), "log": log, "grads": grads}


def value_deviation(got, want) -> float:
    return (torch.as_tensor(got).double().cpu() - torch.as_tensor(want).double()).abs().max().item()


def grad_deviation(got, want) -> float:
    """max |got - want| / max |want| of one gradient tensor (the absolute maximum where want is all zero)."""
    g, w = torch.as_tensor(got).double().cpu().reshape(-1), torch.as_tensor(want).double().reshape(-1)
    return ((g - w).abs().max() / w.abs().max().clamp_min(1e-300)).item() if w.abs().max() > 0 else (g - w).abs().max().item()
