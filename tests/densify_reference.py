"""The reference's densify_and_prune restated in plain PyTorch on the CPU: the yardstick of csrc/densify.hip and
splatfields_amd/densify.py on machines where the reference checkout is absent.  tests/test_densify_reference.py pins it to the
reference's own GaussianModel.densify_and_prune through the fixtures tests/golden/densify_*.npz.

The sequence of reference scene/gaussian_model.py:411-425 is followed step by step, on a growing and shrinking table of rows,
exactly as the reference grows and shrinks its tensors -- nothing plans the final rows ahead:

    grads = accum / denom, NaN -> 0                                                                        (:412-413)
    clone   rows with norm(grads) >= max_grad and max(exp(s)) <= percent_dense * extent are appended          (:394-409)
    split   on the grown table, grads padded with zeros: rows with grads >= max_grad and max(exp(s)) > percent_dense * extent
            get two children each (first children, then second children, appended), then the parents are removed (:355-380)
              child xyz = build_rotation(q) (unit * exp(s)) + xyz      child s = log(exp(s) / 1.6)
    prune   sigmoid(opacity) < min_opacity; if max_screen_size: or radius > max_screen_size or max(exp(s)) > 0.1 * extent (:418-423)

Appended rows get zero Adam moments (:316-319).  densification_postfix (:351-353) zeroes max_radii2D after the clone pass and
again after the split, so the reference's radius test never fires.  `screen_test_on_accumulated_radii=True` is this project's
extension: the radius a row had BEFORE the call stays with the row and goes to its clone (a copy of the row); split children
are new, smaller splats somewhere else and start with radius 0, as every appended row of the reference does.

Every comparison is a torch comparison of a float32 tensor with the Python scalar the caller passed (the product
percent_dense * extent is formed in double and rounded by torch), so thresholds are rounded as the reference rounds them.
Decisions are ALWAYS taken on float32 tensors; `dtype` only selects the arithmetic of the children's values.

Two places differ from the reference's text, both where its text cannot run: `.squeeze()` of the prune mask (:418) makes a
0-dim mask when one row is left, which indexes a new axis into every tensor -- the mask is flattened instead; and the samples
are unit * std with the caller's unit normals where the reference calls torch.normal(0, std)."""
from __future__ import annotations

import math
from collections import namedtuple

import torch

from tests.scan_round import BLOCK, SCAN_ROUND

PARAM_NAMES = ("xyz", "f_dc", "f_rest", "opacity", "scaling", "rotation")
KINDS = ("self", "clone", "first child", "second child")
Result = namedtuple("Result", "params moments counts source kind")


def build_rotation(q: torch.Tensor) -> torch.Tensor:
    """[S, 4] (r, x, y, z), any norm -> [S, 3, 3] (reference utils/general_utils.py:138-159)."""
    q = q / torch.sqrt((q * q)[:, 0] + (q * q)[:, 1] + (q * q)[:, 2] + (q * q)[:, 3])[:, None]
    r, x, y, z = q[:, 0], q[:, 1], q[:, 2], q[:, 3]
    R = torch.zeros(q.shape[0], 3, 3, dtype=q.dtype)
    R[:, 0, 0], R[:, 0, 1], R[:, 0, 2] = 1 - 2 * (y * y + z * z), 2 * (x * y - r * z), 2 * (x * z + r * y)
    R[:, 1, 0], R[:, 1, 1], R[:, 1, 2] = 2 * (x * y + r * z), 1 - 2 * (x * x + z * z), 2 * (y * z - r * x)
    R[:, 2, 0], R[:, 2, 1], R[:, 2, 2] = 2 * (x * z - r * y), 2 * (y * z + r * x), 1 - 2 * (x * x + y * y)
    return R


def _scales(log_scales: torch.Tensor) -> torch.Tensor:
    """get_scaling: exp, one column repeated to three (reference :65-68)."""
    s = torch.exp(log_scales.reshape(log_scales.shape[0], log_scales.shape[1:].numel()))
    return s.repeat(1, 3) if s.shape[1] == 1 else s


def densify_and_prune(params, moments, grad_accum, denom, max_radii2D, max_grad, min_opacity, extent, max_screen_size,
                      percent_dense=0.01, unit_normals=None, screen_test_on_accumulated_radii=False, dtype=torch.float32) -> Result:
    """params: name -> tensor of N rows; moments: name -> (exp_avg, exp_avg_sq) or None, or None; unit_normals [2, N, 3].
    Returns Result(params in `dtype`, moments in their own dtype, counts, source [M] long, kind [M] long): output row r came
    from input row source[r] as KINDS[kind[r]]."""
    cpu = lambda t: torch.as_tensor(t).detach().cpu()
    n = cpu(params["xyz"]).shape[0]
    cols = cpu(params["scaling"]).shape[1:].numel()
    iso = cols == 1
    # the table: one entry per tensor that the reference moves row by row
    T = {k: cpu(params[k]).to(torch.float32).to(dtype) for k in PARAM_NAMES}
    T["dec:scaling"] = cpu(params["scaling"]).to(torch.float32).reshape(n, cols)    # what the float32 reference decides on
    T["dec:opacity"] = cpu(params["opacity"]).to(torch.float32).reshape(n, 1)
    mom_names = [k for k in PARAM_NAMES if moments is not None and moments.get(k) is not None]
    for k in mom_names:
        T["m:" + k], T["v:" + k] = cpu(moments[k][0]).clone(), cpu(moments[k][1]).clone()
    T["source"] = torch.arange(n)
    T["kind"] = torch.zeros(n, dtype=torch.long)
    before = cpu(max_radii2D).to(torch.float32).reshape(-1) if (screen_test_on_accumulated_radii and max_radii2D is not None) else None
    T["radii"] = before.clone() if before is not None else torch.zeros(n)
    unit = cpu(unit_normals).to(dtype)

    def append(new):                                    # cat_tensors_to_optimizer + densification_postfix
        for k in list(T):
            if k[:2] in ("m:", "v:"):
                ext = torch.zeros((new["source"].shape[0],) + tuple(T[k].shape[1:]), dtype=T[k].dtype)
            else:
                ext = new[k]
            T[k] = torch.cat((T[k], ext), dim=0)
        if before is None:
            T["radii"] = torch.zeros(T["source"].shape[0])

    def keep(mask):                                     # prune_points(~mask)
        for k in list(T):
            T[k] = T[k][mask]

    grads = cpu(grad_accum).to(torch.float32).reshape(n, 1) / cpu(denom).to(torch.float32).reshape(n, 1)
    grads[grads.isnan()] = 0.0

    # densify_and_clone
    sel = torch.norm(grads, dim=-1) >= max_grad
    sel = torch.logical_and(sel, _scales(T["dec:scaling"]).max(dim=1).values <= percent_dense * extent) if n else sel
    new = {k: v[sel] for k, v in T.items()}
    new["kind"] = torch.full_like(new["kind"], 1)
    append(new)

    # densify_and_split
    rows = T["source"].shape[0]
    padded = torch.zeros(rows)
    padded[:n] = grads.reshape(-1)
    sel = padded >= max_grad
    sel = torch.logical_and(sel, _scales(T["dec:scaling"]).max(dim=1).values > percent_dense * extent) if rows else sel
    src = T["source"][sel]
    new = {k: v[sel].repeat((2,) + (1,) * (v.dim() - 1)) for k, v in T.items()}
    stds = _scales(T["scaling"][sel].reshape(src.shape[0], cols)).repeat(2, 1)
    samples = torch.cat((unit[0][src], unit[1][src]), dim=0) * stds
    rots = build_rotation(T["rotation"][sel].reshape(-1, 4)).repeat(2, 1, 1)
    new["xyz"] = torch.bmm(rots, samples.unsqueeze(-1)).squeeze(-1) + T["xyz"][sel].repeat(2, 1)
    child = torch.log(stds / (0.8 * 2))
    new["scaling"] = (child[:, :1] if iso else child).reshape((2 * src.shape[0],) + tuple(T["scaling"].shape[1:]))
    child32 = torch.log(_scales(T["dec:scaling"][sel]).repeat(2, 1) / (0.8 * 2))
    new["dec:scaling"] = child32[:, :1] if iso else child32
    new["kind"] = torch.cat((torch.full_like(src, 2), torch.full_like(src, 3)))
    new["radii"] = torch.zeros(2 * src.shape[0])
    append(new)
    keep(~torch.cat((sel, torch.zeros(2 * src.shape[0], dtype=torch.bool))))

    # the final prune
    prune = (torch.sigmoid(T["dec:opacity"]) < min_opacity).reshape(-1)
    if max_screen_size:
        big_vs = T["radii"] > max_screen_size
        big_ws = _scales(T["dec:scaling"]).max(dim=1).values > 0.1 * extent if T["source"].shape[0] else big_vs
        prune = torch.logical_or(torch.logical_or(prune, big_vs), big_ws)
    keep(~prune)

    kind = T["kind"]
    counts = dict(kept=int((kind == 0).sum()), clones=int((kind == 1).sum()), children=int((kind >= 2).sum()), total=int(kind.numel()))
    out_m = None
    if moments is not None:
        out_m = {k: ((T["m:" + k], T["v:" + k]) if k in mom_names else None) for k in PARAM_NAMES}
    return Result({k: T[k] for k in PARAM_NAMES}, out_m, counts, T["source"], kind)


# ------------------------------------------------------------------------------------------------------------------------------
# which rows a last-bit difference between two float32 evaluations could flip

def _is_power_of_two(d: torch.Tensor) -> torch.Tensor:
    m, _ = torch.frexp(d.double())
    return (d > 0) & torch.isfinite(d) & (m == 0.5)


def fragile_rows(inputs: dict, thresholds: dict) -> torch.Tensor:
    """bool [N]: rows whose decision a last-bit difference between the device's expf or division and the host's could flip.

    A row is fragile if its max scale, evaluated in float64, is within a relative 1e-5 of percent_dense * extent, 0.1 * extent
    or 1.6 * 0.1 * extent; or its sigmoid opacity within a relative 1e-5 of min_opacity; or |accum / denom| within a relative
    1e-6 of max_grad.  (An expf within 2 ulp and a correctly rounded division differ from the host's by 2.4e-7 and 0 relative.)
    Not fragile, although on or next to a threshold, are the rows whose float32 value is exact on any IEEE machine:
    the largest log-scale is exactly 0 (exp gives exactly 1); the logit is exactly 0 (1 / (1 + 1) is exactly 0.5);
    denom is a power of two or zero (the quotient is exact, or 0/0 and x/0) -- this holds accum = thr32 * d, the tie, and its
    float32 neighbours."""
    kw, case = thresholds, inputs
    n = case["params"]["xyz"].shape[0]
    s = case["params"]["scaling"].detach().cpu().to(torch.float32)
    s = s.reshape(n, s.shape[1:].numel())
    nan_row = torch.isnan(s).any(dim=1)
    top = torch.where(torch.isnan(s), torch.full_like(s, -math.inf), s).max(dim=1).values if n else s.reshape(0)
    ms = torch.exp(top.double())
    frag = torch.zeros(n, dtype=torch.bool)
    for t in (kw["percent_dense"] * kw["extent"], 0.1 * kw["extent"], 1.6 * 0.1 * kw["extent"]):
        frag |= ((ms - t).abs() <= 1e-5 * abs(t)) & (top != 0.0) & ~nan_row
    logit = case["params"]["opacity"].detach().cpu().to(torch.float32).reshape(-1)
    op = torch.sigmoid(logit.double())
    frag |= ((op - kw["min_opacity"]).abs() <= 1e-5 * abs(kw["min_opacity"])) & (logit != 0.0)
    a, d = case["accum"].to(torch.float32).reshape(-1), case["denom"].to(torch.float32).reshape(-1)
    g = (a.double() / d.double()).abs()
    frag |= ((g - kw["max_grad"]).abs() <= 1e-6 * abs(kw["max_grad"])) & ~(_is_power_of_two(d) | (d == 0))
    return frag


def products_agree(percent_dense: float, extent: float) -> bool:
    """True where float32(percent_dense * extent) (the reference: double product, rounded by the comparison) equals the product
    of the float32 factors (the kernel), and the same for 0.1 * extent: DESIGN.md section 14.3."""
    f = lambda v: torch.tensor(v, dtype=torch.float32)
    return bool(f(percent_dense * extent) == f(percent_dense) * f(extent)) and bool(f(0.1 * extent) == f(0.1) * f(extent))


# ------------------------------------------------------------------------------------------------------------------------------
# the comparison terms of tests/test_gpu_densify_edges.py that need no kernel

def position_scale(case: dict, res: Result) -> torch.Tensor:
    """M [rows, 3] float64 for the child rows of `res` (zeros elsewhere): |xyz_c| + sum_j |R_cj u_j s_j| from the normalised
    quaternion, the size against which a float32 evaluation of the child position rounds."""
    n = case["params"]["xyz"].shape[0]
    src, kind = res.source, res.kind
    M = torch.zeros(src.shape[0], 3, dtype=torch.float64)
    ch = kind >= 2
    if not bool(ch.any()):
        return M
    i = src[ch]
    f64 = lambda t: t.detach().cpu().to(torch.float32).double()
    R = build_rotation(f64(case["params"]["rotation"]).reshape(n, 4)[i])
    s = _scales(f64(case["params"]["scaling"])[i])
    u = f64(case["unit"])[kind[ch] - 2, i]
    M[ch] = f64(case["params"]["xyz"]).reshape(n, 3)[i].abs() + (R * (u * s)[:, None, :]).abs().sum(dim=2)
    return M


def own_position_error(case: dict):
    """(r, res32, res64, M): r = the largest |float32 restatement - float64 restatement| / M over the finite child positions."""
    args = (case["params"], case["moments"], case["accum"], case["denom"], case["radii"])
    r32 = densify_and_prune(*args, unit_normals=case["unit"], dtype=torch.float32, **case["kw"])
    r64 = densify_and_prune(*args, unit_normals=case["unit"], dtype=torch.float64, **case["kw"])
    M = position_scale(case, r64)
    ch = r64.kind >= 2
    ok = ch[:, None] & torch.isfinite(r64.params["xyz"]) & torch.isfinite(M) & (M > 0)
    err = (r32.params["xyz"].double() - r64.params["xyz"]).abs()
    r = float((err[ok] / M[ok]).max()) if bool(ok.any()) else 0.0
    return r, r32, r64, M


# ------------------------------------------------------------------------------------------------------------------------------
# case generators: functions of a seed; every value is drawn INSIDE its class's interval, 5 % or more away from every threshold

CLASSES = ("keep", "clone", "split", "prune")
DEFAULT_KW = dict(max_grad=0.0035, min_opacity=0.1, extent=4.0, max_screen_size=None, percent_dense=0.01,
                  screen_test_on_accumulated_radii=False)


def class_layout(n: int) -> list:
    """Row classes in runs of 63, 64 and 65 (N >= 255; shorter runs below, so that four classes fit), cycling through CLASSES;
    afterwards the first row of every wave of 64 is made to differ from the last row of the wave before it."""
    if n < 4:
        return ["clone", "split", "keep"][:n]
    runs = (63, 64, 65) if n >= 255 else (n // 4,)
    cls, k = [], 0
    while len(cls) < n:
        cls += [k % 4] * runs[k % len(runs)]
        k += 1
    cls = cls[:n]
    for b in range(64, n, 64):
        if cls[b] == cls[b - 1]:
            cls[b] = (cls[b - 1] + 1) % 4
    return [CLASSES[c] for c in cls]


def make_case(n: int, seed: int, classes=None, scale_cols: int = 3, with_moments: bool = True, param_dtype=torch.float32, **kw) -> dict:
    """A cloud of n rows whose row i belongs to classes[i] (default class_layout(n)):
      keep   cold gradient (a third of them 0 / 0), any scale that the world-size test lets live, opaque
      clone  hot, max scale in [0.1, 0.8] D                                   D = percent_dense * extent
      split  hot, max scale in [1.3 D, min(6 D, 0.9 W)]                       W = 0.1 * extent, only with a screen size
      prune  transparent; gradient and scale of any of the other three classes"""
    kw = dict(DEFAULT_KW, **kw)
    classes = list(classes) if classes is not None else class_layout(n)
    assert len(classes) == n
    g = torch.Generator().manual_seed(seed)
    U = lambda lo, hi, *shape: lo + (hi - lo) * torch.rand(*shape, generator=g)
    D, W = kw["percent_dense"] * kw["extent"], 0.1 * kw["extent"]
    big = min(6 * D, 0.9 * W) if kw["max_screen_size"] else 6 * D
    assert big > 1.3 * D * 1.05
    is_ = lambda name: torch.tensor([c == name for c in classes], dtype=torch.bool)
    like = torch.randint(0, 3, (n,), generator=g)                      # which class a pruned row imitates
    hot = is_("clone") | is_("split") | (is_("prune") & (like > 0))
    large = is_("split") | (is_("prune") & (like == 2)) | (is_("keep") & (U(0, 1, n) < 0.5))
    top = torch.where(large, U(math.log(1.3 * D), math.log(big), n), U(math.log(0.1 * D), math.log(0.8 * D), n))
    scaling = top[:, None] + torch.log(U(0.05, 0.95, n, scale_cols))
    if n:
        scaling[torch.arange(n), torch.randint(0, scale_cols, (n,), generator=g)] = top
    denom = torch.randint(1, 6, (n,), generator=g).float()
    accum = denom * kw["max_grad"] * torch.where(hot, U(1.2, 5.0, n), U(0.0, 0.8, n))
    zero = ~hot & (U(0, 1, n) < 1 / 3)
    denom[zero], accum[zero] = 0.0, 0.0
    edge = math.log(kw["min_opacity"] / (1 - kw["min_opacity"]))
    opacity = torch.where(is_("prune"), U(edge - 4.0, edge - 1.0, n), U(edge + 0.5, edge + 5.0, n))
    r = lambda *shape: torch.randn(*shape, generator=g)
    params = {"xyz": r(n, 3), "f_dc": r(n, 1, 3), "f_rest": r(n, 3, 3) * 0.1, "opacity": opacity[:, None], "scaling": scaling,
              "rotation": r(n, 4)}
    params = {k: v.to(param_dtype) for k, v in params.items()}
    moments = {k: (r(*v.shape) * 0.01, r(*v.shape) ** 2 * 1e-4) for k, v in params.items()} if with_moments else None
    return dict(params=params, moments=moments, accum=accum[:, None], denom=denom[:, None], radii=U(0.0, 40.0, n),
                unit=r(2, n, 3), kw=kw, classes=classes, empty=())


def _set_rows(case, rows, *, log_scale=None, logit=None, accum=None, denom=None, radius=None, quat=None, unit=None):
    """Overwrites the named fields of the given rows (a float, or one value per row; log-scales: a float or one row of columns per row)."""
    rows = torch.as_tensor(rows)
    p = case["params"]
    if log_scale is not None:
        p["scaling"][rows] = torch.as_tensor(log_scale, dtype=p["scaling"].dtype)
    if logit is not None:
        p["opacity"][rows, 0] = torch.as_tensor(logit, dtype=p["opacity"].dtype)
    if accum is not None:
        case["accum"][rows, 0] = torch.as_tensor(accum, dtype=torch.float32)
    if denom is not None:
        case["denom"][rows, 0] = torch.as_tensor(denom, dtype=torch.float32)
    if radius is not None:
        case["radii"][rows] = torch.as_tensor(radius, dtype=torch.float32)
    if quat is not None:
        p["rotation"][rows] = torch.as_tensor(quat, dtype=torch.float32)
    if unit is not None:
        case["unit"][:, rows] = torch.as_tensor(unit, dtype=torch.float32)


def f32(v: float) -> float:
    return float(torch.tensor(v, dtype=torch.float32))


def neighbour(v: float, up: bool) -> float:
    """The float32 next to float32(v)."""
    return float(torch.nextafter(torch.tensor(v, dtype=torch.float32), torch.tensor(math.inf if up else -math.inf, dtype=torch.float32)))


def _rows_of(case, name, count):
    idx = [i for i, c in enumerate(case["classes"]) if c == name]
    assert len(idx) >= count, (name, len(idx), count)
    step = len(idx) // count
    return idx[::step][:count]


POW2 = (1.0, 2.0, 4.0, 8.0)


def boundary_case(n: int, seed: int = 0) -> dict:
    if n == 1:
        raise ValueError("one row has one class: single_row_case")
    return make_case(n, seed * 1000 + n, max_screen_size=20.0)


def single_row_case(cls: str, seed: int = 0) -> dict:
    c = make_case(1, seed * 1000 + 1 + CLASSES.index(cls), classes=[cls], max_screen_size=20.0)
    c["empty"] = {"split": (0, 1), "clone": (2, 3), "keep": (1, 2, 3), "prune": (0, 1, 2, 3)}[cls]
    return c


def full_scan_pass_case(seed: int = 0) -> dict:
    """k_densify_scan is one ordered_scan (csrc/ordered_scan.h) over four counts per workgroup of 256 rows.  SCAN_ROUND / 4
    workgroups, the last one full: exactly one round of it.  No moments: 262 144 rows of them prove no more than 1000 do."""
    return make_case(SCAN_ROUND // 4 * BLOCK, seed * 1000 + 5, max_screen_size=20.0, with_moments=False)


def second_scan_pass_case(seed: int = 0) -> dict:
    """One row more than full_scan_pass_case: one workgroup, hence four counts -- the smallest step this scan's length takes --
    beyond a round of ordered_scan; the kinds' segments of 1025 counts straddle the round."""
    return make_case(SCAN_ROUND // 4 * BLOCK + 1, seed * 1000 + 7, max_screen_size=20.0, with_moments=False)


def segment_case(which: str, seed: int = 0, n: int = 1000) -> dict:
    s = seed * 1000 + 11
    if which == "none_hot":
        c = make_case(n, s, classes=[("keep", "prune")[i // 63 % 2] for i in range(n)], max_screen_size=20.0)
        hotp = (c["accum"] / c["denom"]).reshape(-1) >= c["kw"]["max_grad"]               # pruned rows that imitate hot ones
        c["accum"][hotp] = 0.0
        c["empty"] = (1, 2, 3)
    elif which == "all_cloned":
        c = make_case(n, s, classes=["clone"] * n, max_screen_size=20.0)
        c["empty"] = (2, 3)
    elif which == "all_split":
        c = make_case(n, s, classes=["split"] * n, max_screen_size=20.0)
        c["empty"] = (0, 1)
    elif which == "all_pruned":
        c = make_case(n, s, classes=["prune"] * n, max_screen_size=20.0)
        c["empty"] = (0, 1, 2, 3)
    elif which == "empty_input":
        c = make_case(0, s, max_screen_size=20.0)
        c["empty"] = (0, 1, 2, 3)
    elif which == "children_only":
        # hot, and so large that the row itself would fall to the world-size test (max scale in [1.05, 1.5] W) while its children,
        # 1.6 times smaller, pass it: nothing but first and second children is left
        c = make_case(n, s, classes=["split"] * n, max_screen_size=20.0)
        g = torch.Generator().manual_seed(s + 1)
        W = 0.1 * c["kw"]["extent"]
        top = math.log(1.05 * W) + (math.log(1.5 * W) - math.log(1.05 * W)) * torch.rand(n, generator=g)
        c["params"]["scaling"] = torch.minimum(c["params"]["scaling"] + 1.0, top[:, None])
        c["params"]["scaling"][torch.arange(n), torch.randint(0, 3, (n,), generator=g)] = top
        c["empty"] = (0, 1)
    else:
        raise KeyError(which)
    return c


def tie_case(which: str, seed: int = 0, n: int = 1000, scale_cols: int = 3) -> dict:
    """Rows exactly on a threshold, or its float32 neighbour, among ordinary rows.  c["ties"]: row -> the kinds it must leave."""
    s = seed * 1000 + 23
    thr = DEFAULT_KW["max_grad"]
    if which in ("dense", "dense_above"):
        # D = 1 exactly (0.25 * 4), or the float32 below 1: the scale exp(0) = 1 is then the float32 neighbour above D
        pd = 0.25 if which == "dense" else 0.25 * (1.0 - 2.0 ** -24)
        c = make_case(n, s, scale_cols=scale_cols, percent_dense=pd, extent=4.0)
        rows = _rows_of(c, "clone", 8)
        _set_rows(c, rows, log_scale=0.0)
        if scale_cols == 3:
            _set_rows(c, rows[:4], log_scale=[[0.0, -1.0, -2.0], [-0.5, 0.0, -3.0], [-1.0, -1.0, 0.0], [0.0, 0.0, -0.25]])
        c["ties"] = {r: ((0, 1) if which == "dense" else (2, 3)) for r in rows}
    elif which == "world":
        # W = 1 exactly (0.1 * 10 in double and in float32); a scale of exactly 1 is not larger
        c = make_case(n, s, scale_cols=scale_cols, percent_dense=2.0 ** -6, extent=10.0, max_screen_size=20.0)
        cold, hot = _rows_of(c, "keep", 4), _rows_of(c, "split", 4)
        _set_rows(c, cold + hot, log_scale=0.0)
        c["ties"] = {**{r: (0,) for r in cold}, **{r: (2, 3) for r in hot}}
    elif which == "opacity":
        c = make_case(n, s, scale_cols=scale_cols, min_opacity=0.5)
        rows = _rows_of(c, "keep", 3) + _rows_of(c, "clone", 3) + _rows_of(c, "split", 3)
        _set_rows(c, rows, logit=0.0)
        c["ties"] = dict(zip(rows, [(0,)] * 3 + [(0, 1)] * 3 + [(2, 3)] * 3))
    elif which == "grad":
        c = make_case(n, s, scale_cols=scale_cols)
        on_c, on_s = _rows_of(c, "clone", 8), _rows_of(c, "split", 8)
        d = torch.tensor(POW2 * 2)
        at = torch.tensor([f32(thr)] * 4 + [neighbour(thr, up=False)] * 4)
        for rows in (on_c, on_s):
            _set_rows(c, rows, accum=at * d, denom=d)
        c["ties"] = {**{r: ((0, 1) if j < 4 else (0,)) for j, r in enumerate(on_c)}, **{r: ((2, 3) if j < 4 else (0,)) for j, r in enumerate(on_s)}}
    elif which == "radius":
        c = make_case(n, s, scale_cols=scale_cols, max_screen_size=20.0, screen_test_on_accumulated_radii=True)
        c["radii"] = c["radii"] * 0.45                                    # ordinary rows: below 18
        k, cl, sp = _rows_of(c, "keep", 4), _rows_of(c, "clone", 4), _rows_of(c, "split", 4)
        for rows in (k, cl, sp):
            _set_rows(c, rows, radius=[20.0, neighbour(20.0, up=True), 20.0, 35.0])
        c["ties"] = {}
        for j in range(4):
            inside = j % 2 == 0
            c["ties"][k[j]] = (0,) if inside else ()
            c["ties"][cl[j]] = (0, 1) if inside else ()
            c["ties"][sp[j]] = (2, 3)                                     # the children are new splats: their radius is 0
    else:
        raise KeyError(which)
    return c


def isotropic_case(seed: int = 0) -> dict:
    """scale_cols = 1 at N = 257 with a scale tie (D = 1), gradient ties and an opacity tie (min_opacity = 0.5) in one cloud."""
    s = seed * 1000 + 31
    thr = DEFAULT_KW["max_grad"]
    c = make_case(257, s, scale_cols=1, percent_dense=0.25, extent=4.0, min_opacity=0.5)
    cl, sp, k = _rows_of(c, "clone", 6), _rows_of(c, "split", 4), _rows_of(c, "keep", 2)
    _set_rows(c, cl[:2], log_scale=0.0)
    _set_rows(c, cl[2:4], accum=[f32(thr) * 2, neighbour(thr, up=False) * 2], denom=[2.0, 2.0])
    _set_rows(c, sp[:2], accum=[f32(thr) * 4, neighbour(thr, up=False) * 4], denom=[4.0, 4.0])
    _set_rows(c, [cl[4], sp[2], k[0]], logit=0.0)
    c["ties"] = {cl[0]: (0, 1), cl[1]: (0, 1), cl[2]: (0, 1), cl[3]: (0,), sp[0]: (2, 3), sp[1]: (0,), cl[4]: (0, 1), sp[2]: (2, 3), k[0]: (0,)}
    return c


def gradient_case(seed: int = 0, n: int = 1000) -> dict:
    """Gradients that are not ordinary: 0 / 0, x / 0, and negative quotients at and beyond -max_grad."""
    c = make_case(n, seed * 1000 + 41, max_screen_size=20.0)
    thr = DEFAULT_KW["max_grad"]
    cl, sp = _rows_of(c, "clone", 8), _rows_of(c, "split", 8)
    for rows, hot in ((cl, (0, 1)), (sp, (2, 3))):
        _set_rows(c, rows[:2], accum=0.0, denom=0.0)                                      # NaN -> 0: not hot
        _set_rows(c, rows[2:4], accum=[1e-3, 7.0], denom=0.0)                             # +inf: hot
        _set_rows(c, rows[4:6], accum=[-f32(thr) * 2, -f32(thr) * 8], denom=[2.0, 8.0])   # exactly -thr
        _set_rows(c, rows[6:8], accum=[-3.0 * thr * 3, -1e3], denom=[3.0, 0.0])           # beyond: -3 thr and -inf
    # the reference clones on the norm and splits on the signed value: a small row is cloned, a large one is left alone
    c["ties"] = {**{r: ((0,) if j < 2 else (0, 1)) for j, r in enumerate(cl)}, **{r: ((2, 3) if 2 <= j < 4 else (0,)) for j, r in enumerate(sp)}}
    return c


def nonfinite_case(seed: int = 0, n: int = 1000) -> dict:
    """NaN and inf in single rows among ordinary rows (no screen size: a child of an infinite splat stays)."""
    c = make_case(n, seed * 1000 + 53)
    nan, inf = math.nan, math.inf
    cl, sp, k = _rows_of(c, "clone", 5), _rows_of(c, "split", 8), _rows_of(c, "keep", 2)
    # torch.max propagates NaN: neither `<=` nor `>` holds, the row is neither cloned nor split
    for rows in (cl, sp):
        big = [float(v) for v in c["params"]["scaling"][rows[0]]]
        _set_rows(c, rows[:3], log_scale=[[nan, big[1], big[2]], [big[0], nan, nan], [nan, nan, nan]])
    _set_rows(c, [cl[3], sp[3], k[0]], logit=nan)                          # NaN < min_opacity is false: the row lives
    _set_rows(c, [cl[4], sp[4], k[1]], log_scale=[[inf, -3.0, -3.0]] * 3)  # hot rows (both classes) split; children at inf
    _set_rows(c, sp[5:7], quat=0.0)                                        # 0 / 0: every child position is NaN
    c["ties"] = {**{r: (0,) for r in cl[:3] + sp[:3]}, cl[3]: (0, 1), sp[3]: (2, 3), k[0]: (0,), cl[4]: (2, 3), sp[4]: (2, 3), k[1]: (0,),
                 sp[5]: (2, 3), sp[6]: (2, 3)}
    return c


AXIS_QUATS = ((1, 0, 0, 0), (0, 1, 0, 0), (0, 0, 1, 0), (0, 0, 0, 1), (1, 1, 0, 0), (1, -1, 0, 0), (1, 0, 1, 0), (1, 0, -1, 0),
              (1, 0, 0, 1), (1, 0, 0, -1), (1, 1, 1, 1), (-1, 1, 1, 1), (1, -1, 1, -1), (0, 1, 1, 0), (0, 1, 0, -1), (0, 0, 1, 1))


def rotation_case(seed: int = 0, n: int = 1000) -> dict:
    """Every row is split.  Rows 0..47: the 16 quaternions of AXIS_QUATS (rotations by 90, 120 and 180 degrees: every entry of R
    is 0 or +-1 up to round-off), each with unit normals along x, y and z -- the first child gets +e_j, the second -2 e_k with
    k = j + 1: one column of R per child, signs included.  The rest: random quaternions scaled to norms 1e-3, 1 and 1e3.
    Positions are kept away from 0 so that M does not vanish where R_cj is 0."""
    c = make_case(n, seed * 1000 + 61, classes=["split"] * n)
    g = torch.Generator().manual_seed(seed * 1000 + 62)
    xyz = (0.5 + 1.5 * torch.rand(n, 3, generator=g)) * (torch.randint(0, 2, (n, 3), generator=g) * 2 - 1)
    c["params"]["xyz"] = xyz
    q = c["params"]["rotation"]
    q = q / q.norm(dim=1, keepdim=True)
    c["params"]["rotation"] = q * torch.tensor([1e-3, 1.0, 1e3])[torch.arange(n) % 3][:, None]
    eye = torch.eye(3)
    for a, quat in enumerate(AXIS_QUATS):
        for j in range(3):
            row = 3 * a + j
            _set_rows(c, [row], quat=[list(map(float, quat))], unit=torch.stack((eye[j], -2 * eye[(j + 1) % 3]))[:, None, :])
    c["empty"] = (0, 1)
    return c


def screen_case(max_screen_size, flag: bool, seed: int = 0, n: int = 1000) -> dict:
    return make_case(n, seed * 1000 + 71, max_screen_size=max_screen_size, screen_test_on_accumulated_radii=flag)


def dtype_case(dtype, seed: int = 0, n: int = 1000) -> dict:
    """Parameters held in `dtype`; the values are rounded to it before anything is decided."""
    return make_case(n, seed * 1000 + 83, max_screen_size=20.0, param_dtype=dtype)


def all_cases(seed: int = 0) -> dict:
    """name -> a function that builds the case: everything tests/test_gpu_densify_edges.py runs."""
    cases = {f"boundary_{n}": (lambda n=n: boundary_case(n, seed)) for n in (2, 63, 64, 65, 255, 256, 257, 511, 513)}
    cases.update({f"single_{k}": (lambda k=k: single_row_case(k, seed)) for k in ("split", "clone")})
    cases["full_scan_pass"] = lambda: full_scan_pass_case(seed)
    cases["second_scan_pass"] = lambda: second_scan_pass_case(seed)
    cases.update({f"segment_{k}": (lambda k=k: segment_case(k, seed)) for k in ("none_hot", "all_cloned", "all_split", "all_pruned", "empty_input", "children_only")})
    cases.update({f"tie_{k}": (lambda k=k: tie_case(k, seed)) for k in ("dense", "dense_above", "world", "opacity", "grad", "radius")})
    cases["isotropic"] = lambda: isotropic_case(seed)
    cases["gradient"] = lambda: gradient_case(seed)
    cases["nonfinite"] = lambda: nonfinite_case(seed)
    cases["rotation"] = lambda: rotation_case(seed)
    cases.update({f"screen_{m}_{'on' if f else 'off'}": (lambda m=m, f=f: screen_case(m, f, seed)) for m in (None, 0, 20.0) for f in (False, True)})
    cases.update({f"dtype_{str(d)[6:]}": (lambda d=d: dtype_case(d, seed)) for d in (torch.float64, torch.float16)})
    return cases
