"""tests/moran_reference.py computes what the reference's extract_geo.py computes (tests/golden/moran_cases.npz, written by
tests/golden/make_moran_golden.py from `query_nn`, `morans_measure` and `morans_loss` themselves): float64 to 1e-12, and the
float32 evaluations within the reference's own float32 error."""
import pytest
import torch

from tests import moran_reference as R

CASES = R.load_golden_cases()
GRAPH_CASES = sorted(k for k in CASES if k != "free_pair")


def test_the_cases_the_issue_asks_for_are_there():
    assert set(GRAPH_CASES) == {"smooth4", "noise", "constant", "duplicates", "planar", "clustered", "k3", "k8", "n_equals_k"}
    assert [f.shape[1] for f in CASES["smooth4"]["features"]] == list(R.REFERENCE_WIDTHS)
    assert int(CASES["k3"]["k"]) == 3 and int(CASES["k8"]["k"]) == 8 and CASES["n_equals_k"]["points"].shape[0] == 5
    for name in ("smooth4", "duplicates", "planar", "k3", "k8"):
        m = CASES[name]["f64"]["means"]
        assert ((m >= 0.05) & (m <= 0.95)).all(), name
    assert (CASES["noise"]["f64"]["means"] < 0).all() and (CASES["noise"]["f64"]["terms"] == 1).all()
    assert all((g == 0).all() for g in CASES["noise"]["f64"]["d_features"]) and (CASES["noise"]["f64"]["d_points"] == 0).all()
    assert (CASES["constant"]["f64"]["terms"] < 0.01).all()
    p = CASES["duplicates"]["points"]
    assert len(torch.unique(p, dim=0)) == p.shape[0] - 5
    assert (CASES["planar"]["points"][:, 2] == CASES["planar"]["points"][0, 2]).all()


@pytest.mark.parametrize("name", GRAPH_CASES)
def test_neighbours_are_unambiguous_and_match_the_exact_search(name):
    c = CASES[name]
    nn_ix, d2 = R.exact_knn(c["points"], int(c["k"]))
    assert R.ambiguous_share(d2, 1e-4) == 0.0
    assert torch.equal(nn_ix, c["nn_ix"].long())


@pytest.mark.parametrize("name", GRAPH_CASES)
def test_restatement_equals_the_reference_in_float64(name):
    c = CASES[name]
    got = R.evaluate(c["points"], c["features"], c["nn_ix"], float(c["eps"]), torch.float64, chunk=64)
    got["weights"] = R.query_weights(c["points"].double(), c["nn_ix"].long(), float(c["eps"]))
    want = c["f64"]
    for k in ("total", "terms", "means", "weights", "d_points"):
        assert torch.allclose(got[k], want[k], rtol=1e-12, atol=1e-12), (name, k, (got[k] - want[k]).abs().max())
    for g, w in zip(got["d_features"], want["d_features"]):
        assert g.shape == w.shape and torch.allclose(g, w, rtol=1e-12, atol=1e-12), (name, (g - w).abs().max())


def test_chunking_does_not_change_the_result():
    c = CASES["smooth4"]
    a = R.evaluate(c["points"], c["features"], c["nn_ix"], chunk=7)
    b = R.evaluate(c["points"], c["features"], c["nn_ix"], chunk=100000)
    assert torch.allclose(a["total"], b["total"], rtol=1e-13, atol=0) and torch.allclose(a["d_points"], b["d_points"], rtol=1e-10, atol=1e-15)


def test_free_standing_pair_in_float64():
    c = CASES["free_pair"]
    w = c["weight"].double().requires_grad_(True)
    x = c["feature"].double().requires_grad_(True)
    loss = R.morans_loss(w, x)
    loss.backward()
    want = c["f64"]
    assert torch.allclose(loss.detach(), want["loss"], rtol=1e-12, atol=1e-12)
    assert torch.allclose(R.morans_measure(w, x).detach(), want["measure"], rtol=1e-12, atol=1e-12)
    assert torch.allclose(w.grad, want["d_weight"], rtol=1e-12, atol=1e-14) and torch.allclose(x.grad, want["d_feature"], rtol=1e-12, atol=1e-14)


def test_restatement_in_float32_is_as_good_as_the_reference_in_float32():
    r = R.reference_error(CASES)
    print("reference float32 against float64:", r)
    assert all(0 < r[k] < 1e-3 for k in R.METRICS), r
    for name in GRAPH_CASES:
        c = CASES[name]
        got = R.evaluate(c["points"], c["features"], c["nn_ix"], float(c["eps"]), torch.float32)
        d = R.deviations(got, c["f64"])
        assert all(d[k] <= 4.0 * r[k] for k in R.METRICS), (name, d, r)


def test_upstream_gradient_and_gates():
    c = CASES["n_equals_k"]
    one = R.evaluate(c["points"], c["features"], c["nn_ix"])
    half = R.evaluate(c["points"], c["features"], c["nn_ix"], upstream=0.5)
    assert torch.equal(half["d_points"], 0.5 * one["d_points"])
    assert (one["means"][1] < 0) and (one["d_features"][1] == 0).all() and (one["d_features"][0] != 0).any()


@pytest.mark.parametrize("kind,n,seed", R.KNN_CLOUDS)
def test_knn_comparison_clouds_are_nearly_unambiguous(kind, n, seed):
    """tests/test_gpu_moran.py lets a point whose 5th and 6th neighbours lie within 1e-5 (relative, squared distance) differ from
    the exact search by that swap; at most 1e-4 of the points may be such points, under the exact search alone."""
    _, d2 = R.exact_knn(R.cloud(kind, n, seed), 5)
    share = R.ambiguous_share(d2, 1e-5)
    print(kind, n, "ambiguous share", share)
    assert share <= 1e-4
