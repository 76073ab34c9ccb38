"""Moran's I regulariser restated in plain PyTorch (CPU, float64 or float32): the yardstick of the HIP kernels on machines
where the reference checkout is absent.  tests/test_moran_reference.py pins it to the reference's own extract_geo.py
(`query_nn`, `morans_measure`, `morans_loss`) through tests/golden/moran_cases.npz (float64, 1e-12).

For points q [N,3], neighbour rows nn_ix [N,K] (the K nearest points, the point itself included) and eps:

    c[p,a,b] = 1 / |q_a - q_b| where that distance exceeds eps, eps elsewhere (the diagonal included),   q_a = q[nn_ix[p,a]]
    S[p]     = sum_ab c[p,a,b]                      weights[p] = c[p] / max(S[p], 1e-5)
    m[p,f]   = K sum_ab c[p,a,b] x_a x_b / (S[p] (sum_a x_a^2 + 1e-4)),                                    x_a = X[nn_ix[p,a], f]
    term     = 1 - clamp(mean_{p,f} m, 0, 1)        total = sum over the feature tensors of their terms

Everything is evaluated in chunks of points, so 300 000 points x 56 channels fit."""
from __future__ import annotations

import os

import numpy as np
import torch

from tests.scan_round import SCAN_ROUND

DENOM_EPS = 1e-4
METRICS = ("term", "total", "grad_max", "grad_l2")
REFERENCE_WIDTHS = (3, 4, 1, 48)          # scales, rotations, opacity, SH features (train.py:204-210)


def exact_knn(points: torch.Tensor, k: int, with_next: bool = False):
    """(nn_ix [N,k] int64, d2 [N,k+1] float64): the k nearest points of every point by (distance, index) in float64, and the
    squared distances of the k + 1 nearest (the last column is inf when N = k); with_next: also the (k+1)-th point [N] (N > k)."""
    from scipy.spatial import cKDTree
    p = points.detach().cpu().double().numpy()
    n = p.shape[0]
    kk = min(k + 1, n)
    dist, idx = cKDTree(p).query(p, k=kk)
    dist, idx = dist.reshape(n, kk), idx.reshape(n, kk)
    order = np.lexsort((idx, dist), axis=1)
    dist, idx = np.take_along_axis(dist, order, 1), np.take_along_axis(idx, order, 1)
    d2 = np.full((n, k + 1), np.inf)
    d2[:, :kk] = dist ** 2
    if with_next:
        return torch.from_numpy(idx[:, :k].astype(np.int64)), torch.from_numpy(d2), torch.from_numpy(idx[:, k].astype(np.int64))
    return torch.from_numpy(idx[:, :k].astype(np.int64)), torch.from_numpy(d2)


def ambiguous_share(d2: torch.Tensor, rel: float) -> float:
    """Share of the points whose k-th and (k+1)-th squared distances lie within `rel` of each other (relative)."""
    a, b = d2[:, -2], d2[:, -1]
    close = torch.isfinite(b) & ((b - a) <= rel * b)        # no (k+1)-th point when N = k
    return close.double().mean().item()


def pair_weights(q: torch.Tensor, eps: float):
    """c [P,K,K] and S [P] of gathered positions q [P,K,3]."""
    diff = q[:, :, None, :] - q[:, None, :, :]
    d2 = (diff * diff).sum(-1)
    d = torch.where(d2 > 0, torch.where(d2 > 0, d2, torch.ones_like(d2)).sqrt(), torch.zeros_like(d2))   # d/dq = 0 at distance 0, as cdist
    far = d > eps
    c = torch.where(far, 1.0 / torch.where(far, d, torch.ones_like(d)), torch.full_like(d, eps))
    return c, c.sum((1, 2))


def query_weights(points: torch.Tensor, nn_ix: torch.Tensor, eps: float = 1e-5) -> torch.Tensor:
    c, s = pair_weights(points[nn_ix], eps)
    return c / s.clamp_min(1e-5)[:, None, None]


def measure_items(c: torch.Tensor, s: torch.Tensor, x: torch.Tensor) -> torch.Tensor:
    """m [P,F] of weights c [P,K,K] with sum s [P] and gathered rows x [P,K,F]."""
    k = c.shape[1]
    a = torch.einsum("pab,paf,pbf->pf", c, x, x)
    return k * a / (s[:, None] * ((x * x).sum(1) + DENOM_EPS))


def morans_measure(weight: torch.Tensor, feature: torch.Tensor) -> torch.Tensor:
    return measure_items(weight, weight.sum((1, 2)), feature).mean()


def morans_loss(weight: torch.Tensor, feature: torch.Tensor) -> torch.Tensor:
    return 1.0 - morans_measure(weight, feature).clamp(0.0, 1.0)


def evaluate(points, features, nn_ix, eps=1e-5, dtype=torch.float64, chunk=16384, upstream=1.0, want_points=True):
    """Values and gradients of sum_t term_t in `dtype`: dict of detached CPU tensors total, terms [T], means [T],
    d_features (list) and d_points.  Two passes over chunks of points: the means, then, through the clamp's gate, the
    gradients."""
    pts = points.detach().cpu().to(dtype).requires_grad_(want_points)
    feats = [f.detach().cpu().to(dtype).reshape(f.shape[0], -1).requires_grad_(True) for f in features]
    nn_ix = nn_ix.detach().cpu().long()
    n = pts.shape[0]
    sums = [torch.zeros((), dtype=dtype) for _ in feats]
    with torch.no_grad():
        for lo in range(0, n, chunk):
            ix = nn_ix[lo:lo + chunk]
            c, s = pair_weights(pts[ix], eps)
            for t, x in enumerate(feats):
                sums[t] = sums[t] + measure_items(c, s, x[ix]).sum()
    means = torch.stack([v / (n * x.shape[1]) for v, x in zip(sums, feats)])
    terms = 1.0 - means.clamp(0.0, 1.0)
    gate = (means >= 0.0) & (means <= 1.0)
    for lo in range(0, n, chunk):
        ix = nn_ix[lo:lo + chunk]
        c, s = pair_weights(pts[ix], eps)
        part = None
        for t, x in enumerate(feats):
            if gate[t]:
                v = measure_items(c, s, x[ix]).sum() * (-upstream / (n * x.shape[1]))
                part = v if part is None else part + v
        if part is not None:
            part.backward()
    zero = lambda t: torch.zeros_like(t) if t.grad is None else t.grad
    return {"total": terms.sum().detach(), "terms": terms.detach(), "means": means.detach(),
            "d_features": [zero(x).detach().reshape(f.shape) for x, f in zip(feats, features)],
            "d_points": zero(pts).detach() if want_points else None}


def point_gradient_scale(points, features, nn_ix, eps=1e-5) -> float:
    """The magnitude of the terms that are ADDED into one point's gradient, before any of them cancel: the largest, over the
    points p, of sum_f sum_{a != b} |d term / d m[p,f]| K / (S D_f) (|x_a x_b| + |A_f| / S) |d c_ab / d q|, with
    |d c_ab / d q| = c_ab^2.  A float32 evaluation of such a sum is uncertain by about 2^-24 of this figure whatever the sum
    itself comes to -- for constant features it comes to exactly 0 (x_a x_b = A / S)."""
    pts = points.detach().cpu().double()
    nn_ix = nn_ix.detach().cpu().long()
    c, s = pair_weights(pts[nn_ix], eps)
    k = c.shape[1]
    slope = torch.where(c > eps, c * c, torch.zeros_like(c))
    total = torch.zeros(pts.shape[0], dtype=torch.float64)
    for f in features:
        x = f.detach().cpu().double().reshape(f.shape[0], -1)[nn_ix]                     # [N,K,F]
        a = torch.einsum("pab,paf,pbf->pf", c, x, x)
        d = (x * x).sum(1) + DENOM_EPS
        h = k / (s[:, None] * d) / (x.shape[0] * x.shape[2])                              # [N,F]
        xx = (x[:, :, None, :] * x[:, None, :, :]).abs() + (a.abs() / s[:, None])[:, None, None, :]
        total += torch.einsum("pab,pabf,pf->p", slope, xx, h)
    return total.max().item()


# ---- inputs ----

def cloud(kind: str, n: int, seed: int) -> torch.Tensor:
    """float32 [n,3]: 'uniform' in the unit cube, 'planar' (z = 0.3 exactly), 'clustered' (Gaussian clumps of very different
    sizes plus 1 % far outliers)."""
    gen = torch.Generator().manual_seed(seed)
    if kind == "uniform":
        p = torch.rand(n, 3, generator=gen, dtype=torch.float64)
    elif kind == "planar":
        p = torch.rand(n, 3, generator=gen, dtype=torch.float64)
        p[:, 2] = 0.3
    elif kind == "clustered":
        k = 12
        centres = 4.0 * torch.rand(k, 3, generator=gen, dtype=torch.float64) - 2.0
        sizes = 10.0 ** (-2.5 + 2.0 * torch.rand(k, generator=gen, dtype=torch.float64))
        which = torch.randint(0, k, (n,), generator=gen)
        p = centres[which] + sizes[which, None] * torch.randn(n, 3, generator=gen, dtype=torch.float64)
        far = torch.rand(n, generator=gen) < 0.01
        p[far] = 60.0 * torch.rand(int(far.sum()), 3, generator=gen, dtype=torch.float64) - 30.0
    else:
        raise ValueError(kind)
    return p.to(torch.float32)


def cloud_with_duplicates():
    """1500 points of which the last 500 repeat the first 500 exactly: every third row of the exact search has a twin pair
    astride its k-th place, which only the index can order."""
    points = cloud("uniform", 1500, 46)
    points[1000:] = points[:500]
    return points


def cloud_with_non_finite_rows():
    """2000 uniform points of which 5 rows hold a NaN and 5 an infinity, in one or in every coordinate."""
    points = cloud("uniform", 2000, 47)
    nan, inf = float("nan"), float("inf")
    points[[3, 700, 1999], 1] = nan
    points[[256, 1024]] = nan
    points[5, 0], points[900, 2] = inf, -inf
    points[1500] = inf
    points[1501] = torch.tensor([inf, -inf, 0.5])
    points[64] = -inf
    finite = torch.isfinite(points).all(1)
    assert int((~finite).sum()) == 10 and int(torch.isnan(points).any(1).sum()) == 5
    return points, finite


# the clouds on which the device's neighbour search is compared with the exact one: (kind, points, seed)
# SCAN_ROUND - 1, SCAN_ROUND, SCAN_ROUND + 1 points: k_rev_scan walks one count per point (the last full round of ordered_scan, and
# the first count of a second one; seeds whose cloud has no ambiguous point, since a single one is more than 1e-4 of so few); the
# full-size cloud stays last
KNN_CLOUDS = (("uniform", 1000, 45), ("clustered", 20000, 42), ("planar", 4000, 43), ("uniform", SCAN_ROUND - 1, 46),
              ("uniform", SCAN_ROUND, 47), ("uniform", SCAN_ROUND + 1, 50), ("uniform", 300000, 44))


def smooth_features(points: torch.Tensor, widths, noise: float, seed: int, wavelength: float = 1.0):
    """Per width one float32 [N,width] field: a smooth function of the position (plane waves with an offset) plus `noise`
    times white noise -- spatially autocorrelated, so Moran's I lies inside (0, 1)."""
    gen = torch.Generator().manual_seed(seed)
    p = points.double()
    span = (p.max(0).values - p.min(0).values).clamp_min(1e-6).max()
    out = []
    for w in widths:
        freq = (2.0 * torch.rand(3, w, generator=gen, dtype=torch.float64) - 1.0) * (3.0 / (wavelength * span))
        phase = 6.28 * torch.rand(w, generator=gen, dtype=torch.float64)
        field = torch.sin(p @ freq + phase) + 0.3 * torch.cos(0.5 * (p @ freq))
        out.append((field + noise * torch.randn(p.shape[0], w, generator=gen, dtype=torch.float64)).to(torch.float32))
    return out


# ---- the golden cases (tests/golden/moran_cases.npz, written by tests/golden/make_moran_golden.py from the reference itself) ----

def load_golden_cases() -> dict:
    """{case: {"points", "features": [..], "k", "eps", "nn_ix", "f64": {...}, "f32": {...}}} of torch tensors; the free-standing
    pair is {"weight", "feature", "f64", "f32"} under the name "free_pair"."""
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "moran_cases.npz")
    cases: dict = {}
    with np.load(path) as z:
        for key in z.files:
            parts = key.split("/")
            node = cases.setdefault(parts[0], {})
            for p in parts[1:-1]:
                node = node.setdefault(p, {})
            node[parts[-1]] = torch.from_numpy(z[key])
    for c in cases.values():
        if "points" in c:
            feats = [c[k] for k in sorted((k for k in c if k.startswith("feature_")), key=lambda s: int(s[8:]))]
            c["f64"]["d_points_scale"] = point_gradient_scale(c["points"], feats, c["nn_ix"], float(c["eps"]))
        for node in (c, c.get("f64", {}), c.get("f32", {})):
            for stem in ("feature_", "d_feature_"):
                keys = sorted((k for k in node if k.startswith(stem)), key=lambda s: int(s[len(stem):]))
                if keys:
                    node[stem[:-1] + "s"] = [node.pop(k) for k in keys]
    return cases


def deviations(got: dict, want: dict) -> dict:
    """The figures by which an evaluation differs from the float64 one: |d term| (terms, means, weights, a lone loss or
    measure), |d total|, and per gradient tensor max|d grad| / max|grad| and the relative L2 (the largest over the tensors)."""
    f = lambda t: torch.as_tensor(t).to(torch.float64)
    out = dict.fromkeys(METRICS, 0.0)
    for k in ("terms", "means", "weights", "loss", "measure"):
        if k in want and k in got and got[k] is not None:
            out["term"] = max(out["term"], (f(got[k]) - f(want[k])).abs().max().item())
    if "total" in want and "total" in got:
        out["total"] = (f(got["total"]) - f(want["total"])).abs().max().item()
    pairs = []
    for k in ("d_points", "d_weight", "d_feature"):
        if k in want and k in got and got[k] is not None and want[k] is not None:
            pairs.append((got[k], want[k], want.get(k + "_scale")))
    if "d_features" in want and "d_features" in got:
        pairs += [(g, w, None) for g, w in zip(got["d_features"], want["d_features"]) if g is not None]
    for g, w, scale in pairs:
        g, w = f(g).reshape(-1), f(w).reshape(-1)
        top, norm = w.abs().max().clamp_min(1e-300).item(), w.norm().clamp_min(1e-300).item()
        if scale is not None and top < 1e-6 * scale:
            # the float64 gradient is a cancellation of terms a million times larger (point_gradient_scale): a figure
            # relative to what is left of them measures nothing; the error is held against the terms themselves
            top, norm = scale, scale * w.numel() ** 0.5
        out["grad_max"] = max(out["grad_max"], (g - w).abs().max().item() / top)
        out["grad_l2"] = max(out["grad_l2"], (g - w).norm().item() / norm)
    return out


def reference_error(cases: dict) -> dict:
    """r per metric: the largest deviation, over ALL golden cases, of the reference's own float32 evaluation from its float64
    evaluation.  Another float32 evaluation of the same formulas (the HIP kernels) may deviate from float64 by 4 r."""
    r = dict.fromkeys(METRICS, 0.0)
    for c in cases.values():
        d = deviations(c["f32"], c["f64"])
        r = {k: max(r[k], d[k]) for k in METRICS}
    return r
