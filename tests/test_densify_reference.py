"""tests/densify_reference.py pinned to the reference itself -- the fixtures tests/golden/densify_*.npz hold what the reference's
own GaussianModel.densify_and_prune made of four clouds (tests/golden/make_golden.py: densify_cases) -- and the CONDITIONS that
every generated case of tests/test_gpu_densify_edges.py has to meet before a kernel is compared with it.  No GPU, no kernel."""
import os

import numpy as np
import pytest
import torch

from tests import densify_reference as R

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
CASES = R.all_cases()


def bits(t):
    return t.contiguous().view({4: torch.int32, 8: torch.int64, 2: torch.int16}[t.element_size()])


@pytest.mark.parametrize("name", ["aniso_screen", "aniso_noscreen", "isotropic_screen", "tiny"])
def test_float32_restatement_reproduces_the_recorded_reference(name):
    z = np.load(os.path.join(GOLDEN, f"densify_{name}.npz"))
    t = lambda key: torch.as_tensor(z[key])
    params = {k: t("in:" + k) for k in R.PARAM_NAMES}
    moments = {k: (t("in_m:" + k), t("in_v:" + k)) for k in R.PARAM_NAMES}
    res = R.densify_and_prune(params, moments, t("in:accum"), t("in:denom"), t("in:radii"), float(z["max_grad"]), float(z["min_opacity"]),
                              float(z["extent"]), float(z["max_screen_size"]) or None, float(z["percent_dense"]),
                              unit_normals=t("unit_normals"), dtype=torch.float32)
    n_out = z["out:xyz"].shape[0]
    assert res.counts["total"] == n_out == res.counts["kept"] + res.counts["clones"] + res.counts["children"]
    moved = res.kind < 2
    assert bool(t("split_mask")[res.source[res.kind >= 2]].all()) and not bool(t("split_mask")[res.source[res.kind == 0]].any())
    for k in R.PARAM_NAMES:
        ours, ref = res.params[k], t("out:" + k)
        assert ours.shape == ref.shape and ours.dtype == ref.dtype, k
        if k in ("xyz", "scaling"):
            assert torch.equal(bits(ours[moved]), bits(ref[moved])), k          # row order and every pure move: bit for bit
            # the fixture stores sample / std, and (sample / std) * std is not sample to the last bit
            assert torch.allclose(ours, ref, rtol=1e-5, atol=1e-6), k
        else:
            assert torch.equal(bits(ours), bits(ref)), k
        assert torch.equal(bits(res.moments[k][0]), bits(t("out_m:" + k))), k
        assert torch.equal(bits(res.moments[k][1]), bits(t("out_v:" + k))), k
    if name != "tiny":
        assert res.counts["clones"] > 0 and res.counts["children"] > 0 and res.counts["kept"] < z["in:xyz"].shape[0]


def test_the_map_of_the_restatement_describes_its_rows():
    """(source, kind) is what the GPU test trusts: pure moves are the source rows, new rows have moments of exactly +0."""
    c = CASES["boundary_513"]()
    res = R.densify_and_prune(c["params"], c["moments"], c["accum"], c["denom"], c["radii"], unit_normals=c["unit"], **c["kw"])
    assert sorted(set(res.kind.tolist())) == [0, 1, 2, 3]
    order = res.kind * (1 << 32) + res.source
    assert bool((order[1:] > order[:-1]).all())            # originals, clones, first children, second children; ascending inside
    for k in R.PARAM_NAMES:
        rows = res.kind < 2 if k in ("xyz", "scaling") else res.kind >= 0
        assert torch.equal(bits(res.params[k][rows]), bits(c["params"][k][res.source[rows]])), k
        for j in (0, 1):
            m = res.moments[k][j]
            assert torch.equal(bits(m[res.kind == 0]), bits(c["moments"][k][j][res.source[res.kind == 0]])), k
            assert not bits(m[res.kind > 0]).any(), k
    assert torch.equal(res.params["scaling"][res.kind >= 2], torch.log(torch.exp(c["params"]["scaling"][res.source[res.kind >= 2]]) / 1.6))


@pytest.mark.parametrize("name", sorted(CASES))
def test_every_generated_case_meets_its_conditions(name):
    c = CASES[name]()
    n = c["params"]["xyz"].shape[0]
    assert int(R.fragile_rows(c, c["kw"]).sum()) == 0
    assert R.products_agree(c["kw"]["percent_dense"], c["kw"]["extent"])
    s = c["params"]["scaling"].float()
    finite = s[torch.isfinite(s)]
    assert finite.numel() == 0 or (-20 <= float(finite.min()) and float(finite.max()) <= 10)
    r, r32, r64, M = R.own_position_error(c)
    assert r32.counts == r64.counts and torch.equal(r32.source, r64.source) and torch.equal(r32.kind, r64.kind)
    for kind in range(4):
        assert (int((r64.kind == kind).sum()) == 0) == (kind in c["empty"]), (kind, c["empty"])
    if r64.counts["children"]:
        assert 0.0 < r < 1e-5, r                     # the float32 restatement rounds, and only rounds
    assert r64.counts["total"] <= 3 * n
    # rows built by hand: what they must leave was written down from the reference's text, not taken from the restatement
    for row, kinds in c.get("ties", {}).items():
        assert tuple(r64.kind[r64.source == row].tolist()) == tuple(kinds), (row, kinds)
    # the layout: the last row of a wave of 64 and the first row of the next differ in class
    if name.startswith("boundary_") or name in ("full_scan_pass", "second_scan_pass"):
        cl = c["classes"]
        assert all(cl[b] != cl[b - 1] for b in range(64, n, 64))
        assert n < 255 or set(cl[:255]) == set(R.CLASSES)


def test_two_roundings_of_the_dense_threshold_differ_for_the_documented_pair():
    """the reference compares with float32(percent_dense * extent), the product in double; the kernel
    multiplies the float32 factors.  For this pair they are neighbours -- the limit is real, and stated."""
    pd, extent = 0.001, 999.99993896484375
    assert np.float32(extent) == extent
    reference, kernel = np.float32(pd * extent), np.float32(pd) * np.float32(extent)
    assert reference == np.float32(0.99999994) and kernel == np.float32(1.0) and reference != kernel
    assert np.nextafter(reference, np.float32(2)) == kernel
    assert not R.products_agree(pd, extent)
    assert R.products_agree(0.25, 4.0) and R.products_agree(0.25 * (1 - 2.0 ** -24), 4.0) and R.products_agree(2.0 ** -6, 10.0)
    assert np.float32(0.1 * 10.0) == np.float32(0.1) * np.float32(10.0) == np.float32(1.0)
