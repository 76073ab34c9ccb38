"""The chunk loop of splatfields_amd/weight_grad.py on the MI355X, once per caller: tests/test_gpu_flow_head.py's
test_rows_beyond_two_gigabytes_are_addressed_with_64_bits restated at 200 points.

With the chunk limit forced to 64, one call on n points cuts its weight-gradient launch into chunks of 64 points.  Every chunk is
the launch an unchunked call on those rows alone makes (same kernel, same point count, same values at 16-byte-aligned rows), and the
driver adds the chunks' results in chunk order in float32, so:

* the PARAMETER gradients of the whole call equal, with torch.equal, the float32 sum in slice order of the parameter gradients of
  one unchunked call per row slice [0:64], [64:128], ...;
* the PER-POINT outputs and input gradients do not pass through the driver and depend on their own point only: every slice call's
  equal the whole call's rows.

For the view-colour head only dW[:, :F] comes from the slab kernel and is compared; dW[:, F:] and db are sums of per-workgroup
partials of 256 consecutive points, whose grouping a slice changes."""
import pytest
import torch

from splatfields_amd import _lib, weight_grad

pytestmark = pytest.mark.gpu
LIMIT = 64


def rn(*shape, seed, dev):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed)).to(dev)


def general_mlp_case(dev):
    """hidden 64, two layers and a skip: layer 1's dW has two column-block jobs (the input segment, the hidden segment)"""
    from splatfields_amd.fused_mlp import fused_general_mlp
    d_in, H, out = 27, 64, 3
    dims = [(H, d_in), (out, H + d_in)]
    params = [rn(*d, seed=10 + i, dev=dev) / d[1] ** 0.5 for i, d in enumerate(dims)] + [rn(d[0], seed=20 + i, dev=dev) * 0.1 for i, d in enumerate(dims)]
    call = lambda pts, ps: [fused_general_mlp(pts["h_in"], ps[:2], ps[2:], skips=(0,))]
    return call, {"h_in": lambda n: rn(n, d_in, seed=1, dev=dev)}, params, None


def point_linear_case(dev):
    from splatfields_amd.fused_mlp import point_linear
    k, m = 8, 5
    params = [rn(m, k, seed=30, dev=dev), rn(m, seed=31, dev=dev)]
    return (lambda pts, ps: [point_linear(pts["x"], ps[0], ps[1])]), {"x": lambda n: rn(n, k, seed=2, dev=dev)}, params, None


def view_color_case(dev):
    from splatfields_amd.view_color import fused_view_color
    width, views = 4, 2
    params = [rn(3, width + 3, seed=40, dev=dev), rn(3, seed=41, dev=dev)]
    centres = rn(views, 3, seed=42, dev=dev) * 4.0

    def call(pts, ps):      # [V, N, 3] -> points first
        return [fused_view_color(pts["feature"], ps[0], ps[1], means3D=pts["means3D"], camera_centers=centres).permute(1, 0, 2)]

    points = {"feature": lambda n: rn(n, width, seed=3, dev=dev), "means3D": lambda n: rn(n, 3, seed=4, dev=dev)}
    return call, points, params, [lambda g: g[:, :width], None]          # of the parameter gradients, only dW[:, :F] is compared


def flow_head_case(dev):
    from splatfields_amd.flow_head import fused_flow_head
    width = 8
    params = [rn(3, width, seed=50 + i, dev=dev) / width ** 0.5 for i in range(2)] + [rn(3, seed=52 + i, dev=dev) * 0.5 for i in range(2)]
    call = lambda pts, ps: list(fused_flow_head("se3", pts["hidden"], pts["pts"], ps[:2], ps[2:]))
    return call, {"hidden": lambda n: rn(n, width, seed=5, dev=dev), "pts": lambda n: rn(n, 3, seed=6, dev=dev)}, params, None


def step(call, points, params, probes, lo, hi):
    """outputs, input gradients and parameter gradients of one call on the rows [lo:hi]"""
    pts = {k: v[lo:hi].clone().requires_grad_() for k, v in points.items()}
    ps = [p.clone().requires_grad_() for p in params]
    outs = call(pts, ps)
    if probes is None:
        return outs
    sum((o * pr[lo:hi]).sum() for o, pr in zip(outs, probes)).backward()
    return [o.detach() for o in outs], {k: v.grad for k, v in pts.items()}, [p.grad for p in ps]


def slab_launches(monkeypatch):
    """the point counts of every slab-kernel launch from here on"""
    lib, counts = _lib.load(), []
    launch = lib.sr_mlp_weight_grad
    monkeypatch.setattr(lib, "sr_mlp_weight_grad", lambda n, *rest: counts.append(n) or launch(n, *rest))
    return counts


CASES = [(general_mlp_case, 200), (point_linear_case, 200), (point_linear_case, 65), (view_color_case, 200), (flow_head_case, 200)]


@pytest.mark.parametrize("case, n", CASES, ids=[f"{c.__name__[:-5]}-{n}" for c, n in CASES])
def test_a_chunked_call_is_the_sum_in_order_of_its_slices(hip_device, monkeypatch, case, n):
    call, make_points, params, compared = case(hip_device)
    points = {k: make(n) for k, make in make_points.items()}
    with torch.no_grad():
        shapes = [o.shape for o in step(call, points, params, None, 0, n)]
    probes = [rn(*s, seed=60 + i, dev=hip_device) for i, s in enumerate(shapes)]
    counts = slab_launches(monkeypatch)
    slices = [(lo, min(lo + LIMIT, n)) for lo in range(0, n, LIMIT)]

    monkeypatch.setattr(weight_grad, "chunk_limit_override", LIMIT)
    outs, d_points, d_params = step(call, points, params, probes, 0, n)
    assert counts == [hi - lo for lo, hi in slices], "the whole call was not cut into the chunks this test is about"

    monkeypatch.setattr(weight_grad, "chunk_limit_override", None)
    del counts[:]
    total = None
    for lo, hi in slices:
        o, dp, dq = step(call, points, params, probes, lo, hi)
        for a, b in zip(o, outs):
            assert torch.equal(a, b[lo:hi]), (lo, hi)
        for k in dp:
            assert torch.equal(dp[k], d_points[k][lo:hi]), (k, lo, hi)
        total = dq if total is None else [t + g for t, g in zip(total, dq)]
    assert counts == [hi - lo for lo, hi in slices]
    compared = compared or [lambda g: g] * len(params)
    assert any(compared)
    for i, (pick, whole, parts) in enumerate(zip(compared, d_params, total)):
        if pick is not None:
            assert torch.isfinite(pick(whole)).all() and torch.equal(pick(whole), pick(parts)), i
