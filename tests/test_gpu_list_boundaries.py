"""The per-tile sort (csrc/binning.hip), the forward blend (csrc/render.hip) and both backward blends (csrc/blend_bwd.hip, the
pixel-per-lane kernel of csrc/render.hip) on the scenes of tests/boundary_scenes.py: every list length, stop position and
(quad, entry) pair count those kernels branch on, met exactly instead of by chance.  tests/test_boundary_scenes.py proves (CPU)
that no threshold decision of these scenes is close, so nothing here is exempt and the bounds are those of the arithmetic:

  sort    every tile's list equals the expected (depth level, splat index) sequence EXACTLY -- the levels are duplicated with
          bit-identical positions, so most neighbours in a list are depth ties --, the instance total is the splat count,
          and a second render of the same image gives the same lists and the same image;
  blend   radii equal; every pixel of colour, depth and alpha within 1e-4 (relative to max(|ref|, 1e-3)) of the C oracle in
          double; entries behind every pixel's stop get EXACTLY zero in every tensor, the entry at the designed last position
          a non-zero opacity gradient; the two backward kernels agree to 5e-5 of the tensor's maximum; a repeat is
          bit-identical.  With and without the depth gradient (another slot cap), once without the alpha gradient.
          Gradients, per tensor and splat group: the yardstick is d = max|hip - f64| <= 4 r, r = max|C oracle in float - f64|
          on the same scene and group (floored at one float ulp of the group's largest reference magnitude) -- the kernels
          are one more float evaluation of the same formulas in another summation order.
          FINDING: of these scenes' gradient tensors only B5's colours meet 4 r.  Observed on MI355X, worst d / 4r per family
          (both backward kernels alike): B1 4.8 (1.1 - 1.3 up to 129 entries, 2 - 3 at 255 - 257, 4.8 at 512), B2 9.6, B3 9.8
          (means2D / scales of faint entries behind 500 - 900 others), B4 2.5 -- and 23 on the rotations / scales of the
          isotropic single-quad entries, whose exact rotation gradient is zero: both figures are cancellation residue --,
          B5 3.4 (colours 0.64).  No entry is lost or counted twice: the excess grows with the number of entries in front,
          and it has two causes in how the kernels evaluate the same formulas:
            * alpha is ONE v_exp_f32 of a completed-square exponent in log2 units with the opacity folded in
              (common.h pair_alpha_px): for an opacity of 0.005 the exponent is ~7.6 and rounds at ulp(7.6) = 4.8e-7, where
              the oracle rounds a power of <= 0.2 and multiplies by the float opacity.  Emulated on the CPU for these scenes
              the float error of the kernels' expression is 3.5 x that of the oracle's (rms 1.7e-7 against 4.9e-8 relative);
              rounding log2(opacity) alone moves the gradients by only 0.1 r, so it is the per-pair rounding;
            * 1 / (1 - alpha) is v_rcp_f32 (1 ulp) where the oracle divides, and both feed the transmittance recurrence
              T_j = T_(j+1) / (1 - alpha_j) that the backward walks over the whole list.
          That is a precision trade of the kernels, not a bug (the largest deviation from the C oracle in float seen in any
          group of any scene is 1.1e-4 of its tensor's maximum), so -- a bound is never taken from the kernels' output -- those
          tensors are held to the suite's float-oracle bound GRAD_TOL32 = 1e-3 of the tensor's maximum against the C oracle in
          float, per splat group (FALLBACK below); d / 4r is still printed for every tensor and group, and its worst value
          per scene is recorded.
  stale   a 760-entry tile, then a tile whose every pixel stops at 256 with the same (N, H, W) (so buffers, learned estimates and
          the b.qmask words of never-staged batches are reused), and back: every render bit-identical to its first.
"""
import math

import pytest
import torch

from oracle import c_oracle
from tests import boundary_scenes as B
from tests.accuracy import ulp32
from tests.helpers import record_observed, run_hip
from tests.test_gpu_lists import check_tile_lists, hip_tile_lists

pytestmark = pytest.mark.gpu

IMG_TOL = 1e-4
KERNELS_AGREE = 5e-5   # of the tensor's maximum: the bound of test_both_backward_blend_kernels_agree
GRAD_TOL32 = 1e-3      # of the tensor's maximum, against the C oracle in float: the bound of tests/test_gpu_parity.py
_ALL = frozenset(["means3D", "means2D", "opacities", "scales", "rotations", "shs", "colors_precomp"])
# scene family -> tensors that cannot meet 4 r (module docstring: FINDING) and are held to GRAD_TOL32 instead
FALLBACK = {"B1": _ALL, "B2": _ALL, "B3": _ALL, "B4": _ALL, "B5": _ALL - {"colors_precomp"}}


# ------------------------------------------------------------------------------------------------ sort

@pytest.mark.parametrize("name", B.SORT_NAMES)
def test_every_tile_list_is_exactly_the_expected_sequence(hip_device, name):
    sc = B.sort_scene_by_name(name)
    n, w, h = sc.sp["means3D"].shape[0], sc.st.image_width, sc.st.image_height
    runs = [hip_tile_lists(sc.sp, sc.st, hip_device, with_image=True) for _ in range(2)]
    for tile_start, sorted_id, total, reported, radii, image in runs:
        assert total == reported == n == int(tile_start[-1]) == sorted_id.numel()
        assert (tile_start[1:] - tile_start[:-1]).tolist() == sc.lengths
        for t, want in enumerate(sc.expected):
            got = sorted_id[int(tile_start[t]):int(tile_start[t + 1])]
            if not torch.equal(got, want):
                bad = int(torch.nonzero(got != want)[0])
                raise AssertionError(f"{name}: tile {t} ({sc.lengths[t]} entries, {sc.levels[t]} depth levels) differs first at "
                                     f"position {bad}: got splat {int(got[bad])}, expected {int(want[bad])}")
        assert torch.isfinite(image).all()
    for a, b in zip(runs[0], runs[1]):
        assert a == b if isinstance(a, int) else torch.equal(a, b)
    # the oracle-side statement of the existing list test holds too, and it saw the ties
    lengths, ties = check_tile_lists(sc.sp, sc.st, n, w, h, hip_device, expect_missing=False)
    assert lengths.tolist() == sc.lengths
    assert ties > 0.8 * (n - sum(sc.levels)) and ties > 10000, ties


# ------------------------------------------------------------------------------------------------ blend

_refs = {}


def references(sc, with_depth, with_alpha):
    """(outputs, gradients) of the C oracle in double and in float, once per scene and loss."""
    key = (sc.name, with_depth, with_alpha)
    if key not in _refs:
        gi, gd, ga = B.upstream(sc)
        _refs[key] = {prec: c_oracle.rasterize(sc.sp, sc.st, use_sh=sc.use_sh, g_img=gi, g_depth=gd if with_depth else None,
                                               g_alpha=ga if with_alpha else None, precision=prec, threads=4)[:2]
                      for prec in ("fp64", "fp32")}
    return _refs[key]


worst_rel = [0.0]   # largest gradient deviation from the C oracle in float seen so far, relative to its tensor's maximum


def check_parity(sc, out, g, with_depth, with_alpha, tag, problems):
    """Appends every violated statement to `problems`; returns the worst d / 4r of the run."""
    ref = references(sc, with_depth, with_alpha)
    (o64, g64), (o32, g32) = ref["fp64"], ref["fp32"]
    if not torch.equal(out["radii"].to(torch.int32), o64["radii"].to(torch.int32)):
        problems.append(f"{tag}: radii differ")
    for k in ("color", "depth", "alpha"):
        r = o64[k].double()
        rel = ((out[k].double() - r).abs() / r.abs().clamp_min(1e-3)).max().item()
        if not rel <= IMG_TOL:
            problems.append(f"{tag}: image {k} {rel:.3g} > {IMG_TOL}")
    worst = 0.0
    for k in g64:
        ref64 = g64[k].double()
        d_all, r_all = (g[k].double() - ref64).abs(), (g32[k].double() - ref64).abs()
        for gname, idx in sc.groups.items():
            if idx.numel() == 0:
                continue
            d = d_all[idx].max().item()
            top = ref64[idx].abs().max().item()
            r = max(r_all[idx].max().item(), ulp32(top) if top > 0 else 0.0)       # an all-zero reference gets no floor
            ratio = d / (4 * r) if r > 0 else (0.0 if d == 0 else math.inf)
            worst = max(worst, ratio)
            e32 = (g[k].double() - g32[k].double()).abs()[idx].max().item() / max(g32[k].abs().max().item(), 1e-30)
            print(f"[d/4r] {tag} {k}/{gname}: d {d:.3g} r {r:.3g} ratio {ratio:.3g} vs-float-oracle/tensor-max {e32:.3g}")
            worst_rel[0] = max(worst_rel[0], e32)
            if k in FALLBACK[sc.family]:
                if not e32 <= GRAD_TOL32:
                    problems.append(f"{tag}: {k}/{gname} {e32:.3g} of the tensor's maximum from the C oracle in float > {GRAD_TOL32}")
            elif not d <= 4 * r:
                problems.append(f"{tag}: {k}/{gname} d {d:.3g} > 4 r = {4 * r:.3g} (ratio {ratio:.3g})")
        if sc.behind.numel() and not (g[k][sc.behind] == 0).all():
            problems.append(f"{tag}: {k} of an entry behind every stop is not exactly zero")
        culled = sc.pos == 0
        if culled.any() and not (g[k][culled] == 0).all():
            problems.append(f"{tag}: {k} of a culled splat is not exactly zero")
    if sc.last.numel() and not (g["opacities"][sc.last] != 0).all():
        problems.append(f"{tag}: the entry at the designed last position has no opacity gradient")
    return worst


def run_variants(sc, dev):
    """Every (kernel, loss) variant of one scene through the facade: {(kernel, with_depth, with_alpha): (out, grads)}."""
    from splatfields_amd.rasterizer import set_backward_kernel
    grads = B.upstream(sc)
    res = {}
    res["auto", True, True] = run_hip(sc.sp, sc.st, grads, dev, use_sh=sc.use_sh)
    res["repeat", True, True] = run_hip(sc.sp, sc.st, grads, dev, use_sh=sc.use_sh)
    res["auto", False, True] = run_hip(sc.sp, sc.st, grads, dev, use_sh=sc.use_sh, with_depth=False)
    res["auto", True, False] = run_hip(sc.sp, sc.st, grads, dev, use_sh=sc.use_sh, with_alpha=False)
    try:
        set_backward_kernel("wave")
        res["wave", True, True] = run_hip(sc.sp, sc.st, grads, dev, use_sh=sc.use_sh)
        res["wave", False, True] = run_hip(sc.sp, sc.st, grads, dev, use_sh=sc.use_sh, with_depth=False)
    finally:
        set_backward_kernel(None)
    return res


def check_scene(sc, dev):
    res = run_variants(sc, dev)
    problems, worst = [], {}
    for (kernel, wd, wa), (out, g) in res.items():
        if kernel == "repeat":
            continue
        tag = f"{sc.name} {kernel}{'' if wd else ' no-depth'}{'' if wa else ' no-alpha'}"
        worst[tag] = check_parity(sc, out, g, wd, wa, tag, problems)
    for wd in (True, False):
        gq, gw = res["auto", wd, True][1], res["wave", wd, True][1]
        for k in gq:
            scale = gq[k].abs().max().item()
            diff = (gq[k] - gw[k]).abs().max().item()
            if not diff <= KERNELS_AGREE * scale:
                problems.append(f"{sc.name}: kernels disagree on {k} (depth gradient {wd}): {diff:.3g} vs max {scale:.3g}")
    (o1, g1), (o2, g2) = res["auto", True, True], res["repeat", True, True]
    for k in o1:
        if not torch.equal(o1[k], o2[k]):
            problems.append(f"{sc.name}: repeat differs in output {k}")
    for k in g1:
        if not torch.equal(g1[k], g2[k]):
            problems.append(f"{sc.name}: repeat differs in gradient {k}")
    record_observed(f"list_boundaries {sc.name}", {"worst_d_over_4r": max(worst.values()), "family": sc.family,
                                                   "worst_vs_float_oracle_of_tensor_max_so_far": worst_rel[0]})
    assert not problems, "\n".join(problems)


@pytest.mark.parametrize("name", B.BLEND_NAMES)
def test_blend_parity_on_a_list_boundary(hip_device, name):
    check_scene(B.blend_scene(name), hip_device)


# ------------------------------------------------------------------------------------------------ stale state

def test_a_short_stop_after_a_long_list_and_back_leaves_nothing_behind(hip_device):
    long, short = B.stale_pair()
    assert long.sp["means3D"].shape == short.sp["means3D"].shape and long.st.image_width == short.st.image_width
    runs = []
    for sc in (long, short, long, short, long):
        runs.append((sc, run_hip(sc.sp, sc.st, B.upstream(sc), hip_device, use_sh=sc.use_sh)))
    first = {}
    problems = []
    for i, (sc, (out, g)) in enumerate(runs):
        if sc.name not in first:
            first[sc.name] = (out, g)
            check_parity(sc, out, g, True, True, f"stale {sc.name}", problems)
            continue
        o0, g0 = first[sc.name]
        for k in o0:
            assert torch.equal(out[k], o0[k]), (i, sc.name, k)
        for k in g0:
            assert torch.equal(g[k], g0[k]), (i, sc.name, k)
    # ... and in the opposite order: the short scene first
    for sc in (short, long):
        out, g = run_hip(sc.sp, sc.st, B.upstream(sc), hip_device, use_sh=sc.use_sh)
        o0, g0 = first[sc.name]
        assert all(torch.equal(out[k], o0[k]) for k in o0) and all(torch.equal(g[k], g0[k]) for k in g0), sc.name
    assert not problems, "\n".join(problems)
