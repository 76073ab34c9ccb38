"""The Moran's I regulariser (splatfields_amd/moran.py -> sr_knn_graph, sr_moran_*) on the MI355X against the reference's own
float64 evaluation (tests/golden/moran_cases.npz) and, at full size, against the restatement tests/moran_reference.py that
test_moran_reference.py pins to the reference.

Tolerance: for each metric -- |d term| (terms, means, weights), |d total|, per gradient tensor max|d grad| / max|grad| and the
relative L2 -- r is the largest deviation over ALL golden cases of the reference's own float32 evaluation from its float64
evaluation (at full size: the larger of that and the restatement's float32-against-float64 deviation on that input).  The
kernels are another float32 evaluation of the same formulas in another summation order and may deviate from float64 by 4 r.
A gradient that is a complete cancellation in float64 (constant features: the point gradient) is held against the terms that
cancel, not against what is left of them (moran_reference.point_gradient_scale).  Nothing is exempted."""
import types

import pytest
import torch

from tests import moran_reference as R
from tests.accuracy import assert_deviations

pytestmark = pytest.mark.gpu

CASES = R.load_golden_cases()
GRAPH_CASES = sorted(k for k in CASES if k != "free_pair")
R_GOLDEN = R.reference_error(CASES)


def hip_evaluate(dev, points, features, k=5, eps=1e-5, graph=None, scale=None, want_points=True):
    from splatfields_amd.moran import moran_loss
    p = points.to(dev).requires_grad_(want_points)
    feats = [f.to(dev).requires_grad_(True) for f in features]
    total, terms, means = moran_loss(p, feats, k, eps, graph=graph, return_means=True)
    assert total.requires_grad and not terms.requires_grad and not means.requires_grad and total.dim() == 0
    (total if scale is None else scale * total).backward()
    return {"total": total.detach().cpu(), "terms": terms.cpu(), "means": means.cpu(), "d_features": [f.grad.cpu() for f in feats],
            "d_points": p.grad.cpu() if want_points else None}


def assert_within(tag, got, want, r):
    assert_deviations("moran", tag, R.deviations(got, want), r, R.METRICS)


def assert_same_neighbours(tag, nn_ix, points, k, swap_rel=1e-5, max_share=1e-4, ties_by_index=False):
    """nn_ix [N,k] (device search) against the exact search on the float64 points: the same set for every point, nearest first;
    a point whose k-th and (k+1)-th squared distances lie within swap_rel may differ by exactly that swap.
    ties_by_index (clouds with exact duplicates): where the k-th and the (k+1)-th point are one and the same position the two
    distances are equal in every number format, so nothing is ambiguous there: the lower index is the neighbour, as in
    R.exact_knn, and such rows get no allowance and do not count towards max_share."""
    want, d2, following = R.exact_knn(points, k, with_next=True)
    got = nn_ix.cpu().long()
    n = points.shape[0]
    assert got.shape == want.shape and (got >= 0).all() and (got < n).all()
    p = points.double()
    dist = ((p[got] - p[:, None, :]) ** 2).sum(-1)
    # nearest first, up to the rounding of a float32 squared distance
    assert (dist[:, 1:] >= dist[:, :-1] - 1e-6 * dist[:, 1:]).all(), tag
    same = (got.sort(1).values == want.sort(1).values).all(1)
    ambiguous = torch.isfinite(d2[:, -1]) & ((d2[:, -1] - d2[:, -2]) <= swap_rel * d2[:, -1])
    if ties_by_index:
        twins = (points[want[:, -1]] == points[following]).all(1)
        assert twins.any(), (tag, "no tie at the k-th place: the cloud does not test the index rule")
        ambiguous &= ~twins
        tied = (points[got[:, 1:]] == points[got[:, :-1]]).all(-1)          # inside a row, equal positions stand by index
        assert tied.any() and (got[:, 1:] > got[:, :-1])[tied].all(), tag
    share = ambiguous.double().mean().item()
    print(f"[moran] {tag}: {int((~same).sum())} of {n} rows differ from the exact search, {int(ambiguous.sum())} are ambiguous (share {share:.2e})")
    assert share <= max_share
    assert (same | ambiguous).all(), (tag, "a neighbour set differs where the exact search is unambiguous")
    for i in torch.nonzero(~same).flatten().tolist():       # exactly the swap: the k - 1 nearest agree, the last is the (k+1)-th
        assert set(got[i].tolist()) == set(want[i, :k - 1].tolist()) | {int(following[i])}, (tag, i)


@pytest.mark.parametrize("name", GRAPH_CASES)
def test_golden_cases_fused(hip_device, name):
    c = CASES[name]
    print("r over all golden cases:", R_GOLDEN)
    got = hip_evaluate(hip_device, c["points"], c["features"], int(c["k"]), float(c["eps"]))
    assert got["d_points"].shape == c["points"].shape and all(g.shape == f.shape for g, f in zip(got["d_features"], c["features"]))
    assert_within(name, got, c["f64"], R_GOLDEN)


@pytest.mark.parametrize("name", GRAPH_CASES)
def test_golden_cases_through_the_drop_ins(hip_device, name):
    """train.py:203-210 with only the import changed."""
    from splatfields_amd.moran import morans_loss, morans_measure, query_nn
    c = CASES[name]
    k = int(c["k"])
    p = c["points"].to(hip_device).requires_grad_(True)
    feats = [f.to(hip_device).requires_grad_(True) for f in c["features"]]
    weights, nn_ix = query_nn(p, n_neighbors=k, eps=float(c["eps"]))
    assert nn_ix.dtype == torch.int64 and tuple(weights.shape) == (p.shape[0], k, k) and weights.requires_grad
    terms = [morans_loss(weights, f[nn_ix]) for f in feats]
    means = [morans_measure(weights, f[nn_ix]) for f in feats]
    sum(terms).backward()
    # same neighbour sets as the reference; the order inside a row may differ where two float32 distances round differently,
    # so the weights are compared in the reference's order
    got_ix, want_ix = nn_ix.cpu(), c["nn_ix"].long()
    assert torch.equal(got_ix.sort(1).values, want_ix.sort(1).values)
    perm = (got_ix[:, None, :] == want_ix[:, :, None]).double().argmax(-1)                  # want slot -> got slot
    assert torch.equal(torch.gather(got_ix, 1, perm), want_ix)
    # nn_ix equals the reference's row for row, except where float32 cannot order what float64 can: every slot that differs
    # holds a neighbour whose squared distance is within 1e-6 (relative) of the one the reference has there
    differs = got_ix != want_ix
    pd = c["points"].double()
    d2 = lambda ix: ((pd[ix] - pd[:, None, :]) ** 2).sum(-1)
    d_got, d_want = d2(got_ix), d2(want_ix)
    rows = torch.nonzero(differs.any(1)).flatten().tolist()
    print(f"[moran] {name} drop-in: nn_ix rows in another order than the reference's: {rows}")
    assert ((d_got - d_want).abs()[differs] <= 1e-6 * d_want[differs]).all(), (name, rows)
    assert len(rows) <= 0.02 * got_ix.shape[0], (name, rows)
    w = weights.detach().cpu()
    w = torch.gather(torch.gather(w, 1, perm[:, :, None].expand_as(w)), 2, perm[:, None, :].expand_as(w))
    got = {"weights": w, "terms": torch.stack(terms).detach().cpu(), "means": torch.stack(means).detach().cpu(),
           "total": sum(terms).detach().cpu(), "d_points": p.grad.cpu(), "d_features": [f.grad.cpu() for f in feats]}
    assert_within(name + " drop-in", got, c["f64"], R_GOLDEN)


def test_free_standing_pair(hip_device):
    from splatfields_amd.moran import morans_loss, morans_measure
    c = CASES["free_pair"]
    w = c["weight"].to(hip_device).requires_grad_(True)
    x = c["feature"].to(hip_device).requires_grad_(True)
    loss = morans_loss(w, x)
    loss.backward()
    got = {"loss": loss.detach().cpu(), "d_weight": w.grad.cpu(), "d_feature": x.grad.cpu()}
    w.grad = x.grad = None
    measure = morans_measure(w, x)
    measure.backward()
    got["measure"] = measure.detach().cpu()
    assert_within("free pair", got, c["f64"], R_GOLDEN)
    # inside the clamp the loss is 1 - measure
    assert_within("free pair measure", {"d_weight": -w.grad.cpu(), "d_feature": -x.grad.cpu()}, c["f64"], R_GOLDEN)


@pytest.mark.parametrize("kind,n,seed", R.KNN_CLOUDS)
def test_neighbours_against_the_exact_search(hip_device, kind, n, seed):
    from splatfields_amd.moran import knn_graph
    points = R.cloud(kind, n, seed)
    graph = knn_graph(points.to(hip_device), 5)
    assert graph.nn_ix.dtype == torch.int32
    assert_same_neighbours(f"{kind} {n}", graph.nn_ix, points, 5)
    assert_reverse_adjacency(graph, n, 5)


def assert_reverse_adjacency(graph, n, k):
    """the reverse adjacency lists every edge once, under its target, in ascending order"""
    start, edges = graph.rev_start.cpu().long(), graph.rev_edges.cpu().long()
    assert start[0] == 0 and start[-1] == n * k and (start[1:] >= start[:-1]).all()
    assert torch.equal(edges.sort().values, torch.arange(n * k))
    target = torch.repeat_interleave(torch.arange(n), start[1:] - start[:-1])
    assert torch.equal(graph.nn_ix.cpu().long().reshape(-1)[edges], target)
    inner = torch.ones(n * k, dtype=torch.bool)
    inner[start[:-1][start[:-1] < n * k]] = False
    assert (edges[1:] > edges[:-1])[inner[1:]].all()
    assert torch.equal(graph.order.cpu().long().sort().values, torch.arange(n))


@pytest.mark.parametrize("kind", ("uniform", "duplicates"))
@pytest.mark.parametrize("k", (2, 4, 6, 7), ids=lambda k: f"K{k}")
def test_neighbours_at_every_other_width_of_the_search(hip_device, k, kind):
    """k_knn_search_k<K> is instantiated for K = 2 .. 8; the golden cases and the clouds above launch K = 3, 5 and 8 (the
    `default:` arm of the switch in launch_knn_graph).  These are k_knn_search_k<2>, <4>, <6> and <7>."""
    from splatfields_amd.moran import knn_graph
    points = R.cloud("uniform", 1000, 45) if kind == "uniform" else R.cloud_with_duplicates()
    n = points.shape[0]
    graph = knn_graph(points.to(hip_device), k)
    assert graph.nn_ix.dtype == torch.int32 and tuple(graph.nn_ix.shape) == (n, k)
    assert_same_neighbours(f"{kind} {n} K={k}", graph.nn_ix, points, k, ties_by_index=kind == "duplicates")
    assert (graph.nn_ix[:, 0].cpu().long() == torch.arange(n))[500 if kind == "duplicates" else 0:1000].all()    # itself first, unless a twin has the lower index
    assert_reverse_adjacency(graph, n, k)


def test_non_finite_rows_leave_the_finite_rows_exact(hip_device):
    """A NaN or infinite coordinate takes its row out of every other row's search (its distance to anything is no finite number)
    and out of the grid's bounds; the row itself names in-range indices only, so that every gather stays inside."""
    from splatfields_amd.moran import knn_graph
    points, finite = R.cloud_with_non_finite_rows()
    n, k = points.shape[0], 5
    graph = knn_graph(points.to(hip_device), k)
    got = graph.nn_ix.cpu().long()
    assert tuple(got.shape) == (n, k) and (got >= 0).all() and (got < n).all()
    index = torch.nonzero(finite).flatten()
    want, d2 = R.exact_knn(points[finite], k)
    assert R.ambiguous_share(d2, 1e-5) == 0.0
    assert torch.equal(got[finite].sort(1).values, index[want].sort(1).values)
    assert torch.equal(got[finite][:, 0], index)
    assert_reverse_adjacency(graph, n, k)


def test_full_size_against_the_restatement(hip_device):
    from splatfields_amd.moran import knn_graph
    kind, n, seed = R.KNN_CLOUDS[-1]
    assert n == 300000
    points = R.cloud(kind, n, seed)
    features = R.smooth_features(points, R.REFERENCE_WIDTHS, 0.5, 51, wavelength=0.2)
    graph = knn_graph(points.to(hip_device), 5)
    assert_same_neighbours("full size", graph.nn_ix, points, 5)
    nn_ix = graph.nn_ix.cpu().long()
    want = R.evaluate(points, features, nn_ix, dtype=torch.float64)
    assert ((want["means"] > 0.05) & (want["means"] < 0.95)).all(), want["means"]
    own = R.deviations(R.evaluate(points, features, nn_ix, dtype=torch.float32), want)
    r = {k: max(R_GOLDEN[k], own[k]) for k in R.METRICS}
    print("restatement float32 against float64 on this input:", own)
    got = hip_evaluate(hip_device, points, features, graph=graph)
    assert_within("300000 x (3, 4, 1, 48)", got, want, r)


def test_bit_reproducible_and_graph_reuse(hip_device):
    from splatfields_amd.moran import knn_graph
    points = R.cloud("clustered", 20000, 42)
    features = R.smooth_features(points, R.REFERENCE_WIDTHS, 0.5, 52)
    small = CASES["duplicates"]
    graph = knn_graph(points.to(hip_device), 5)
    first = None
    for i in range(6):
        rebuilt = knn_graph(points.to(hip_device), 5)
        assert all(torch.equal(a, b) for a, b in zip(graph, rebuilt))
        got = hip_evaluate(hip_device, points, features, graph=graph if i % 2 else None)
        tiny = hip_evaluate(hip_device, small["points"], small["features"])
        flat = [got["total"], got["terms"], got["means"], got["d_points"], *got["d_features"], tiny["total"], tiny["d_points"], *tiny["d_features"]]
        first = first or flat
        assert all(torch.equal(a, b) for a, b in zip(flat, first)), i


def test_upstream_gradient_of_one_half_halves_exactly(hip_device):
    c = CASES["smooth4"]
    one = hip_evaluate(hip_device, c["points"], c["features"])
    half = hip_evaluate(hip_device, c["points"], c["features"], scale=0.5)
    assert torch.equal(half["d_points"], 0.5 * one["d_points"]) and one["d_points"].abs().max() > 0
    for a, b in zip(half["d_features"], one["d_features"]):
        assert torch.equal(a, 0.5 * b) and b.abs().max() > 0


def test_gated_terms_give_exact_zeros(hip_device):
    c = CASES["noise"]
    got = hip_evaluate(hip_device, c["points"], c["features"])
    assert (got["means"] < 0).all() and (got["terms"] == 1.0).all() and got["total"] == 2.0
    assert all((g == 0).all() for g in got["d_features"]) and (got["d_points"] == 0).all()
    c = CASES["n_equals_k"]             # one term open, one shut: only the open one reaches its features, and the points
    got = hip_evaluate(hip_device, c["points"], c["features"])
    assert (got["d_features"][1] == 0).all() and (got["d_features"][0] != 0).any() and (got["d_points"] != 0).any()
    assert all(torch.isfinite(g).all() for g in got["d_features"])


def test_only_what_requires_grad_gets_one(hip_device):
    from splatfields_amd.moran import moran_loss
    dev = hip_device
    c = CASES["smooth4"]
    base = hip_evaluate(dev, c["points"], c["features"])
    p = c["points"].to(dev)
    feats = [f.to(dev) for f in c["features"]]
    feats[1].requires_grad_(True)
    total, _ = moran_loss(p, feats)
    total.backward()
    assert p.grad is None and feats[0].grad is None and feats[2].grad is None and feats[3].grad is None
    assert torch.equal(feats[1].grad.cpu(), base["d_features"][1])
    p2 = c["points"].to(dev).requires_grad_(True)
    total, _ = moran_loss(p2, [f.detach() for f in feats])
    total.backward()
    assert torch.equal(p2.grad.cpu(), base["d_points"])
    # [N, 16, 3] features are flattened to [N, 48] and the gradient comes back in the input's shape and dtype
    sh = c["features"][3].reshape(-1, 16, 3).double().to(dev).requires_grad_(True)
    total, terms = moran_loss(c["points"].double().to(dev), [sh])
    total.backward()
    assert total.dtype == torch.float64 and terms.dtype == torch.float64 and sh.grad.shape == sh.shape and sh.grad.dtype == torch.float64
    assert torch.equal(sh.grad.float().reshape(-1, 48).cpu(), base["d_features"][3])


def test_errors_and_no_grad(hip_device):
    from splatfields_amd.moran import knn_graph, moran_loss, morans_loss, morans_measure, query_nn
    dev = hip_device
    c = CASES["smooth4"]
    p, feats = c["points"], c["features"]
    for call in (lambda: moran_loss(p, feats), lambda: query_nn(p), lambda: knn_graph(p),
                 lambda: morans_loss(torch.rand(4, 5, 5), torch.rand(4, 5, 3)), lambda: morans_measure(torch.rand(4, 5, 5), torch.rand(4, 5, 3))):
        with pytest.raises(RuntimeError, match="no CPU path"):
            call()
    pd, fd = p.to(dev), [f.to(dev) for f in feats]
    with pytest.raises(RuntimeError, match="no CPU path"):
        moran_loss(pd, [fd[0], feats[1]])
    with pytest.raises(RuntimeError, match="fewer than n_neighbors"):
        moran_loss(pd[:4], [fd[0][:4]])
    with pytest.raises(RuntimeError, match="fewer than n_neighbors"):
        query_nn(pd[:4])
    with pytest.raises(ValueError, match="n_neighbors must be"):
        moran_loss(pd, fd, n_neighbors=9)
    with pytest.raises(RuntimeError, match="feature tensors in one call"):
        moran_loss(pd, [])
    with pytest.raises(RuntimeError, match="rows"):
        moran_loss(pd, [fd[0][:50]])
    with pytest.raises(RuntimeError, match="the graph is"):
        moran_loss(pd, fd, graph=knn_graph(pd, 3))
    with pytest.raises(RuntimeError, match="expected weight"):
        morans_loss(torch.rand(4, 9, 9, device=dev), torch.rand(4, 9, 3, device=dev))
    pr = pd.clone().requires_grad_(True)
    fr = [f.clone().requires_grad_(True) for f in fd]
    with torch.no_grad():
        total, terms = moran_loss(pr, fr)
    assert total.grad_fn is None and not total.requires_grad
    tracked, _ = moran_loss(pr, fr)
    assert tracked.grad_fn is not None and torch.equal(tracked.detach(), total)
    plain, _ = moran_loss(pd, fd)                      # nothing requires grad: no graph either
    assert plain.grad_fn is None and torch.equal(plain, total)


def test_no_host_wait_from_the_python_side(hip_device):
    from splatfields_amd.moran import moran_loss
    dev = hip_device
    c = CASES["smooth4"]
    p = c["points"].to(dev).requires_grad_(True)
    feats = [f.to(dev).requires_grad_(True) for f in c["features"]]
    moran_loss(p, feats)[0].backward()    # warm up: library load, allocator
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        total, _ = moran_loss(p, feats)
        (0.5 * total).backward()
    finally:
        torch.cuda.set_sync_debug_mode("default")
    torch.cuda.synchronize()
    assert torch.isfinite(total).all()


def test_one_training_shaped_step(hip_device):
    """render() + photometric_loss + 0.01 * moran_loss, one backward(): every leaf's gradient is the sum of the two losses'
    gradients taken separately."""
    from splatfields_amd import render
    from splatfields_amd.losses import photometric_loss
    from splatfields_amd.moran import moran_loss
    from splatfields_amd.synthetic import make_camera, make_splats
    dev = hip_device
    torch.manual_seed(0)
    n, W, H = 4000, 160, 128
    sp = make_splats(n, seed=21, mean_scale=0.05, device=dev)
    pipe = types.SimpleNamespace(debug=False)
    bg = torch.ones(3, device=dev)
    cam = make_camera(2, W, H, device=dev)
    pack = lambda s: {"means3D": s["means3D"], "active_sh_degree": 1, "gaussian_opacity": s["opacities"],
                      "gaussian_features": s["shs"], "gaussian_scales": s["scales"], "gaussian_rotations": s["rotations"]}
    with torch.no_grad():
        gt_image = render(cam, pack(sp), pipe, bg)["render"].clone()
    # attributes that vary smoothly over space (plus noise), as a trained scene's do: all four terms lie inside the clamp
    means = sp["means3D"] + 0.02 * torch.randn(n, 3, device=dev)
    wave = lambda width, seed: R.smooth_features(means.cpu(), (width,), 0.3, seed)[0].to(dev)
    start = {"means3D": means, "scales": sp["scales"] * 1.3 * torch.exp(0.3 * wave(3, 61)),
             "rotations": torch.nn.functional.normalize(wave(4, 62) + 0.5, dim=1), "opacities": 0.5 + 0.3 * torch.tanh(wave(1, 63)),
             "shs": sp["shs"] * 0.2 + wave(48, 64).reshape(n, 16, 3)}

    def run(with_photo, with_moran):
        leaf = {k: v.clone().requires_grad_(True) for k, v in start.items()}
        loss = 0.0
        if with_photo:
            loss = loss + photometric_loss(render(cam, pack(leaf), pipe, bg)["render"], gt_image, 0.2)[0]
        if with_moran:
            total, terms = moran_loss(leaf["means3D"], [leaf["scales"], leaf["rotations"], leaf["opacities"], leaf["shs"]])
            assert terms.shape == (4,) and ((terms > 0.02) & (terms < 0.98)).all(), terms
            loss = loss + 0.01 * total
        loss.backward()
        return {k: v.grad.detach().double().cpu() for k, v in leaf.items()}

    both, photo, moran = run(True, True), run(True, False), run(False, True)
    for k in both:
        want = photo[k] + moran[k]
        err = (both[k] - want).abs().max().item() / want.abs().max().item()
        print(f"[moran] training step {k}: |both - (photometric + moran)| / max = {err:.2e}, moran share {moran[k].abs().max().item() / want.abs().max().item():.2e}")
        assert moran[k].abs().max() > 0 and err <= 1e-6, (k, err)
