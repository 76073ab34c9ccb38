"""csrc/densify.hip and splatfields_amd/densify.py against tests/densify_reference.py (the reference's sequence restated, pinned
to the reference's recorded output by tests/test_densify_reference.py) at the sizes, thresholds and values where a plan of
prefix sums and a gather can go wrong.  Every case compares the WHOLE result:

  * the counts;
  * every pure row move and every Adam moment bit for bit, through the restatement's (source row, kind) of every output row;
  * the children's log-scales against the float64 restatement within 2^-23 (|s| + 1): one rounding of the constant log 1.6 and
    one of the subtraction;
  * the children's positions against the float64 restatement within 4 r M, element by element, where
    M = |xyz_c| + sum_j |R_cj u_j s_j| and r is the float32 restatement's own largest error / M over the case, measured on the
    CPU (the observed d / (4 r M) of every case is printed and tabulated there).

The cases are generated in tests/densify_reference.py; tests/test_densify_reference.py checks without a GPU that none of them
holds a row whose decision a last-bit difference could flip, so every decision here is compared exactly."""
import copy
import functools

import pytest
import torch
from torch import nn

from tests import densify_reference as R

pytestmark = pytest.mark.gpu
CASES = R.all_cases()
ATTR = {"xyz": "_xyz", "f_dc": "_features_dc", "f_rest": "_features_rest", "opacity": "_opacity", "scaling": "_scaling",
        "rotation": "_rotation"}


@functools.lru_cache(maxsize=None)
def reference(name):
    """(case, r, float64 restatement, M): computed once per case and never modified."""
    case = CASES[name]()
    r, _, r64, M = R.own_position_error(case)
    return case, r, r64, M


def bits(t):
    return t.contiguous().view({4: torch.int32, 8: torch.int64, 2: torch.int16}[t.element_size()])


def same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(bits(a), bits(b))


def run(case, dev, **changed):
    from splatfields_amd.densify import densify_and_prune_tensors
    c = dict(case, **changed)
    params = {k: v.to(dev) for k, v in c["params"].items()}
    moments = None if c["moments"] is None else {k: (None if m is None else (m[0].to(dev), m[1].to(dev))) for k, m in c["moments"].items()}
    return densify_and_prune_tensors(params, moments, c["accum"].to(dev), c["denom"].to(dev), c["radii"].to(dev), c["kw"]["max_grad"],
                                     c["kw"]["min_opacity"], c["kw"]["extent"], c["kw"]["max_screen_size"], c["kw"]["percent_dense"],
                                     unit_normals=c["unit"].to(dev),
                                     screen_test_on_accumulated_radii=c["kw"]["screen_test_on_accumulated_radii"])


def compare(case, out, r, r64, M, label=""):
    """Asserts everything listed at the top of this file; returns the largest d / (4 r M) over the children's positions."""
    new_params, new_moments, counts = out
    assert counts == r64.counts, (counts, r64.counts)
    src, kind = r64.source, r64.kind
    child = kind >= 2
    for k in R.PARAM_NAMES:
        given, ours = case["params"][k], new_params[k].detach().cpu()
        assert ours.dtype == given.dtype and tuple(ours.shape) == (counts["total"],) + tuple(given.shape[1:]), k
        moved = ~child if k in ("xyz", "scaling") else torch.ones_like(child)
        assert same_bits(ours[moved], given[src[moved]]), k
    # float16 parameters: the result is rounded once more, to 11 bits
    half = 2.0 ** -11 if case["params"]["xyz"].dtype == torch.float16 else 0.0
    ratio = 0.0
    if bool(child.any()):
        s_ref, s = r64.params["scaling"][child], new_params["scaling"].detach().cpu()[child].double()
        fin = torch.isfinite(s_ref)
        assert torch.equal(s[~fin], s_ref[~fin])                                        # +inf stays +inf
        assert bool(((s - s_ref).abs()[fin] <= (2.0 ** -23 * (s_ref.abs() + 1) + half * s_ref.abs())[fin]).all())
        x_ref, x, m = r64.params["xyz"][child], new_params["xyz"].detach().cpu()[child].double(), M[child]
        fin = torch.isfinite(x_ref)
        assert torch.equal(torch.isnan(x), torch.isnan(x_ref))                          # NaN exactly where the restatement's are
        assert torch.equal(x[torch.isinf(x_ref)], x_ref[torch.isinf(x_ref)])
        d, bound = (x - x_ref).abs()[fin], (4 * r * m + half * x_ref.abs())[fin]
        if d.numel():
            assert r > 0
            ratio = float((d / bound).max())
            print(f"densify edges {label}: rows {counts['total']} children {int(child.sum())} r {r:.3e} max d/(4 r M) {ratio:.4f}")
            assert bool((d <= bound).all()), ratio
    if case["moments"] is None:
        assert new_moments is None
    else:
        for k in R.PARAM_NAMES:
            if case["moments"][k] is None:
                assert new_moments[k] is None, k
                continue
            for j in (0, 1):
                given, ours = case["moments"][k][j], new_moments[k][j].detach().cpu()
                assert ours.dtype == given.dtype and tuple(ours.shape) == (counts["total"],) + tuple(given.shape[1:]), k
                assert same_bits(ours[kind == 0], given[src[kind == 0]]), k             # a row keeps its own moments
                assert not bool(bits(ours[kind > 0]).any()), k                          # new rows: +0.0 and nothing else
    return ratio


@pytest.mark.parametrize("name", sorted(CASES))
def test_whole_result_equals_the_restatement(hip_device, name):
    case, r, r64, M = reference(name)
    compare(case, run(case, hip_device), r, r64, M, name)


def test_radii_change_nothing_unless_they_are_asked_for(hip_device):
    case, r, r64, M = reference("screen_20.0_off")
    huge = run(case, hip_device, radii=case["radii"] * 1e6)
    none = run(case, hip_device, radii=torch.zeros_like(case["radii"]))
    for out in (huge, none):
        compare(case, out, r, r64, M, "screen_20.0_off, other radii")
    assert huge[2] == none[2] and all(same_bits(huge[0][k], none[0][k]) for k in R.PARAM_NAMES)
    on = reference("screen_20.0_on")[2]
    assert on.counts["total"] < r64.counts["total"]                     # the same cloud: with the flag the radii do prune


@pytest.mark.parametrize("which", ["no_moments", "one_entry_missing"])
def test_moments_may_be_absent(hip_device, which):
    case, r, r64, M = reference("boundary_513")
    moments = None if which == "no_moments" else dict(case["moments"], f_rest=None)
    changed = dict(case, moments=moments)
    compare(changed, run(changed, hip_device), r, r64, M, which)


def test_two_calls_give_equal_bits_and_leave_the_inputs_alone(hip_device):
    from splatfields_amd.densify import densify_and_prune_tensors
    case, r, r64, M = reference("screen_20.0_on")
    dev = hip_device
    params = {k: v.to(dev) for k, v in case["params"].items()}
    moments = {k: (m.to(dev), v.to(dev)) for k, (m, v) in case["moments"].items()}
    rest = [case[k].to(dev) for k in ("accum", "denom", "radii", "unit")]
    given = copy.deepcopy((params, moments, rest))
    kw = case["kw"]
    call = lambda: densify_and_prune_tensors(params, moments, rest[0], rest[1], rest[2], kw["max_grad"], kw["min_opacity"], kw["extent"],
                                             kw["max_screen_size"], kw["percent_dense"], unit_normals=rest[3],
                                             screen_test_on_accumulated_radii=True)
    a, b = call(), call()
    assert a[2] == b[2]
    for k in R.PARAM_NAMES:
        assert same_bits(a[0][k], b[0][k]) and same_bits(a[1][k][0], b[1][k][0]) and same_bits(a[1][k][1], b[1][k][1]), k
        assert same_bits(params[k], given[0][k]) and same_bits(moments[k][0], given[1][k][0]) and same_bits(moments[k][1], given[1][k][1]), k
    assert all(same_bits(t, g) for t, g in zip(rest, given[2]))
    compare(case, a, r, r64, M, "screen_20.0_on, first of two calls")


class Holder:
    """The attributes of the reference's GaussianModel that densify_and_prune touches."""

    def __init__(self, case, dev):
        self.percent_dense = case["kw"]["percent_dense"]
        groups = []
        for name, attr in ATTR.items():
            p = nn.Parameter(case["params"][name].clone().to(dev))
            setattr(self, attr, p)
            groups.append({"params": [p], "lr": 1e-3, "name": name})
        self.optimizer = torch.optim.Adam(groups, lr=0.0, eps=1e-15)
        for grp in groups:
            m, v = case["moments"][grp["name"]]
            self.optimizer.state[grp["params"][0]] = {"step": torch.tensor(3.0), "exp_avg": m.clone().to(dev), "exp_avg_sq": v.clone().to(dev)}
        self.xyz_gradient_accum = case["accum"].clone().to(dev)
        self.denom = case["denom"].clone().to(dev)
        self.max_radii2D = case["radii"].clone().to(dev)


@pytest.mark.parametrize("name", ["tie_dense", "segment_all_pruned"])
def test_drop_in_rebuilds_the_holder(hip_device, name):
    from splatfields_amd.densify import densify_and_prune
    case, r, r64, M = reference(name)
    kw = case["kw"]
    h = Holder(case, hip_device)
    counts = densify_and_prune(h, kw["max_grad"], kw["min_opacity"], kw["extent"], kw["max_screen_size"], unit_normals=case["unit"].to(hip_device),
                               screen_test_on_accumulated_radii=kw["screen_test_on_accumulated_radii"])
    total = r64.counts["total"]
    assert (total == 0) == (name == "segment_all_pruned")
    state = {k: h.optimizer.state[getattr(h, a)] for k, a in ATTR.items()}
    compare(case, ({k: getattr(h, a).detach() for k, a in ATTR.items()}, {k: (s["exp_avg"], s["exp_avg_sq"]) for k, s in state.items()}, counts),
            r, r64, M, name + ", drop-in")
    for grp in h.optimizer.param_groups:
        p = grp["params"][0]
        assert p is getattr(h, ATTR[grp["name"]]) and isinstance(p, nn.Parameter) and p.requires_grad and p.shape[0] == total
        assert float(h.optimizer.state[p]["step"]) == 3.0
    assert len(h.optimizer.state) == len(ATTR)
    for stat, shape in ((h.xyz_gradient_accum, (total, 1)), (h.denom, (total, 1)), (h.max_radii2D, (total,))):
        assert tuple(stat.shape) == shape and stat.device == getattr(h, "_xyz").device and not bool(stat.any())
    for grp in h.optimizer.param_groups:
        grp["params"][0].grad = torch.ones_like(grp["params"][0])
    h.optimizer.step()
    torch.cuda.synchronize()
    assert float(h.optimizer.state[h._xyz]["step"]) == 4.0
