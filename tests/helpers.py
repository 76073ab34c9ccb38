"""Shared helpers of the parity tests: scene construction, HIP invocation through the facade
(-> C ABI), and tolerance-aware comparison against the oracle."""
from __future__ import annotations

import contextlib
import math

import torch
import torch.distributed as dist

from oracle import torch_oracle as O
from splatfields_amd.synthetic import make_camera, make_splats, make_upstream_grads

GRAD_NAMES_SH = ["means3D", "scales", "rotations", "opacities", "shs", "means2D"]


class CollectiveLog(list):
    """What `record_collectives` yields: one `(collective, reduce op, dtype, element count)` per call, in issue order (the
    count is that of the reduced tensor, of the gathered OUTPUT of an all-gather, of the INPUT of an all-to-all);
    `.tensors[i]` is that tensor of call i."""

    def __init__(self):
        super().__init__()
        self.tensors = []


@contextlib.contextmanager
def record_collectives():
    """Wraps the `torch.distributed` entry points splatfields_amd.view_parallel issues its collectives through and logs every
    call; the calls themselves go through unchanged."""
    log = CollectiveLog()
    ops = {dist.ReduceOp.SUM: "SUM", dist.ReduceOp.AVG: "AVG"}
    real = {k: getattr(dist, k) for k in ("all_reduce", "all_gather_into_tensor", "all_to_all_single")}

    def all_reduce(tensor, op=dist.ReduceOp.SUM, *a, **kw):
        log.append(("all_reduce", ops[op], tensor.dtype, tensor.numel()))
        log.tensors.append(tensor)
        return real["all_reduce"](tensor, op, *a, **kw)

    def all_gather_into_tensor(output_tensor, input_tensor, *a, **kw):
        log.append(("all_gather", None, output_tensor.dtype, output_tensor.numel()))
        log.tensors.append(output_tensor)
        return real["all_gather_into_tensor"](output_tensor, input_tensor, *a, **kw)

    def all_to_all_single(output, input, *a, **kw):
        log.append(("all_to_all", None, input.dtype, input.numel()))
        log.tensors.append(input)
        return real["all_to_all_single"](output, input, *a, **kw)

    wrapped = {"all_reduce": all_reduce, "all_gather_into_tensor": all_gather_into_tensor, "all_to_all_single": all_to_all_single}
    for k, f in wrapped.items():
        setattr(dist, k, f)
    try:
        yield log
    finally:
        for k, f in real.items():
            setattr(dist, k, f)


def make_scene(n, width, height, *, seed=1234, view=1, sh_degree=3, bg=(1.0, 1.0, 1.0), mean_scale=None,
               scale_modifier=1.0):
    sp = make_splats(n, seed=seed, mean_scale=mean_scale)
    cam = make_camera(view, width, height)
    st = O.settings_from_camera(cam, torch.tensor(bg, dtype=torch.float32), sh_degree, scale_modifier)
    gi, gd, ga = make_upstream_grads(height, width)
    return sp, cam, st, (gi, gd, ga)


def run_hip(sp, st, grads, device, *, use_sh=True, with_depth=True, with_alpha=True):
    """Forward + backward through the drop-in facade on `device`.  Returns (outputs dict, grads dict) on CPU."""
    from diff_gaussian_rasterization import GaussianRasterizationSettings, GaussianRasterizer
    gi, gd, ga = [g.to(device) for g in grads]
    leaf = {k: v.detach().to(device).clone().requires_grad_(True) for k, v in sp.items()}
    means2D = torch.zeros_like(leaf["means3D"], requires_grad=True)
    rs = GaussianRasterizationSettings(
        image_height=st.image_height, image_width=st.image_width, tanfovx=st.tanfovx, tanfovy=st.tanfovy,
        bg=st.bg.to(device), scale_modifier=st.scale_modifier, viewmatrix=st.viewmatrix.to(device),
        projmatrix=st.projmatrix.to(device), sh_degree=st.sh_degree, campos=st.campos.to(device),
        prefiltered=False, debug=False)
    rast = GaussianRasterizer(raster_settings=rs)
    color, radii, depth, alpha = rast.forward_ex(
        means3D=leaf["means3D"], means2D=means2D, opacities=leaf["opacities"],
        shs=leaf["shs"] if use_sh else None, colors_precomp=None if use_sh else leaf["colors_precomp"],
        scales=leaf["scales"], rotations=leaf["rotations"])
    loss = (color * gi).sum()
    if with_depth:
        loss = loss + (depth * gd).sum()
    if with_alpha:
        loss = loss + (alpha * ga).sum()
    loss.backward()
    torch.cuda.synchronize()
    names = ["means3D", "scales", "rotations", "opacities", "shs" if use_sh else "colors_precomp"]
    gz = lambda t: (torch.zeros_like(t) if t.grad is None else t.grad).detach().cpu()
    g = {k: gz(leaf[k]) for k in names}
    g["means2D"] = gz(means2D)
    out = dict(color=color.detach().cpu(), radii=radii.cpu(), depth=depth.detach().cpu(), alpha=alpha.detach().cpu())
    return out, g


def image_errors(hip: torch.Tensor, ref: torch.Tensor, fragile: torch.Tensor, floor: float = 1e-3):
    """max relative error on robust pixels (relative to max(|ref|, floor), SURVEY.md Appendix A
    "Tolerance basis") and max absolute error on threshold-fragile pixels."""
    ref = ref.to(torch.float64)
    err = (hip.to(torch.float64) - ref).abs()
    rel = err / ref.abs().clamp_min(floor)
    frag = fragile[None].expand_as(ref)
    robust = rel[~frag].max().item() if (~frag).any() else 0.0
    fr = err[frag].max().item() if frag.any() else 0.0
    return robust, fr


def grad_error(hip: torch.Tensor, ref: torch.Tensor):
    """max |hip - ref| relative to max |ref| of the tensor."""
    ref = ref.to(torch.float64)
    scale = ref.abs().max().clamp_min(1e-30)
    return ((hip.to(torch.float64) - ref).abs().max() / scale).item()


def radii_mismatch(hip_radii, pre, tol=2e-3):
    """number of radii that differ although 3*sqrt(lambda) is not within `tol` of an integer
    and the visibility decision is not marginal."""
    ref = pre.radii
    diff = hip_radii.to(torch.int64) != ref.to(torch.int64)
    raw = pre.radius_raw.to(torch.float64)
    near_int = (raw - raw.round()).abs() < tol * raw.clamp_min(1.0)
    near_cull = (pre.depth.to(torch.float64) - 0.2).abs() < 1e-5
    # marginal tile-rect emptiness: bounding square touches the tile grid edge within tol
    return int((diff & ~near_int & ~near_cull).sum())


def assert_grads_flip_aware(hip: dict, ref: dict, tag="", *, bulk_tol=1e-3, max_tol=5e-3, outliers=4e-6):
    """fp32 kernels vs the fp32 C oracle on LARGE scenes: among millions of gradient elements a handful sit on pixel-splat
    pairs whose threshold decision (alpha >= 1/255, T >= 1e-4) flips between the two fp32 evaluations, which moves them by a
    discrete amount.  Every element within `max_tol` of the tensor's maximum (the flip-aware bound of the fp64 comparisons),
    all but a fraction `outliers` within `bulk_tol` (the bound of the small-scene fp32 comparisons), median <= 1e-6.
    Observed at the headline size on MI355X (round 5, gpurun_out/parity_observed.jsonl): largest element 2.0e-3 of the tensor's
    maximum, 3.3e-7 of the elements beyond 1e-3 -- the defaults are ~2.5 x / ~12 x that (rounds 1-4 allowed 1e-5 outliers)."""
    for k in ref:
        b = ref[k].double()
        err = (hip[k].double() - b).abs() / b.abs().max().clamp_min(1e-30)
        assert err.max().item() <= max_tol, (tag, k, err.max().item())
        assert (err > bulk_tol).float().mean().item() <= outliers, (tag, k, (err > bulk_tol).float().mean().item())
        assert err.median().item() <= 1e-6, (tag, k)


def record_observed(tag: str, figures: dict) -> None:
    """The figures a large-scene comparison OBSERVED (not only whether they passed): printed (pytest shows them with -rP / on
    failure) and appended to gpurun_out/parity_observed.jsonl, which travels back from the GPU box -- the thresholds in the tests
    are set to at most 10 x what was observed on MI355X, and this file is the record they were set from."""
    import json
    import os
    line = json.dumps({"test": tag, **figures})
    print("[observed] " + line)
    try:
        root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
        os.makedirs(os.path.join(root, "gpurun_out"), exist_ok=True)
        with open(os.path.join(root, "gpurun_out", "parity_observed.jsonl"), "a") as f:
            f.write(line + "\n")
    except OSError:
        pass


# Float ulps of rounding assumed in a splat's stored screen-space centre (oracle/raster_ref.c `cond_bound`).  Against the oracle
# in double only the HIP side rounds: its ((x_ndc + 1) W - 1) / 2 in fp32 sits within ~2.3 ulp of the exact value, and the worst
# pixel of 32 full-size comparisons uses 0.92 of the allowance at 4 ulps (tools/parity_fullsize.py).  Against the oracle in float
# BOTH sides are fp32 evaluations, each within 1e-4 (+ its own centre rounding) of the exact value: two-sided tolerance 2e-4 (oracle/
# parity.py: compare_flagged(oracle_precision="fp32")) and 6 ulps.
XY_ULPS = {"fp64": 4.0, "fp32": 6.0}


def assert_parity_explained(out: dict, g: dict, sp: dict, st, grads, *, use_sh: bool, tag: str, precisions=("fp64", "fp32"),
                            threads=None) -> dict:
    """The large-scene parity statement: against the C oracle in double AND in float, with the
    oracle's own account of what may legitimately differ between two fp32 evaluations,
      (a) every pixel whose threshold decisions are clear of their thresholds (not `fragile`) is within 1e-4 relative
          (to max(|ref|, 1e-3): the north star's bound; against the oracle in float, itself an fp32 evaluation, 2e-4) plus the oracle's first-order bound for XY_ULPS float ulps of rounding in the
          splats' float screen-space centres -- a term that matters only where the rim of one or two faint splats is all a pixel
          shows -- and a fragile pixel is within one blended pair (2e-2 absolute);
      (b) every gradient element beyond 1e-3 of its tensor's maximum belongs to a splat that is blended into a fragile pixel
          (`splat_flag`), and no element anywhere is beyond 5e-2;
      (c) radii are equal except where 3 sqrt(lambda) is within rounding of an integer.
    `unexplained` -- anything outside (a)-(c) -- must be 0."""
    import os
    from oracle import c_oracle, parity as P
    threads = threads or min(128, os.cpu_count() or 8)
    figs = {}
    for prec in precisions:
        ref, rg, _ = c_oracle.rasterize(sp, st, use_sh=use_sh, g_img=grads[0], g_depth=grads[1], g_alpha=grads[2], threads=threads,
                                        precision=prec, fragile=True, xy_ulps=XY_ULPS[prec])
        fig = P.compare_flagged(out, g, ref, rg, oracle_precision=prec)
        figs[prec] = fig
        record_observed(f"{tag} vs {prec}", {
            "unexplained": fig["unexplained"], "radii": fig["radii"], "image_robust_max_rel": fig["image_robust_max_rel"],
            "image_robust_above_1e-4": fig["image_robust_above_1e-4"], "conditioning_limited": fig["image_conditioning_limited"],
            "max_err_over_allowance": max(v.get("max_err_over_allowance", 0.0) for v in fig["images"].values()),
            "fragile_share": fig["images"]["color"]["fragile_share"],
            "fragile_max_abs": max(v["fragile_max_abs"] for v in fig["images"].values()),
            "flagged_splat_share": fig["flagged_splat_share"], "grad_max": max(v["max_rel_to_tensor_max"] for v in fig["gradients"].values()),
            "grad_max_unflagged": fig["gradient_max_unflagged"]})
        assert fig["radii"]["unexplained"] == 0, (tag, prec, fig["radii"])
        for k, v in fig["images"].items():
            assert v["unexplained"] == 0, (tag, prec, k, v)
            assert v["median_rel"] < 1e-5, (tag, prec, k, v)
            assert v["fragile_max_abs"] <= 2e-2 * max(1.0, float(ref[k].abs().max())), (tag, prec, k, v)
        assert fig["images"]["color"]["fragile_share"] < 0.2, (tag, prec, fig["images"]["color"]["fragile_share"])
        for k, v in fig["gradients"].items():
            assert v["unexplained"] == 0, (tag, prec, k, v)
            assert v["max_rel_to_tensor_max"] <= 5e-2, (tag, prec, k, v)
            assert v["median_rel_to_tensor_max"] <= 1e-6, (tag, prec, k, v)
        assert fig["unexplained"] == 0, (tag, prec)
    return figs
