"""The subset step on the device (csrc/subset.hip, splatfields_amd/subset.py) against tests/subset_reference.py: the draw bit for
bit against the numpy restatement, the gather and its backward against PyTorch indexing, the statistics through the row list
against gather / update / scatter with the existing op, one training step end to end, and the keyed draw of the two
initialisations.  Launch counts through tests/launches.py."""
import types

import numpy as np
import pytest
import torch

import accuracy
import launches
import subset_reference as R

pytestmark = pytest.mark.gpu

SEED = 0x5EED5EED5EED


def _kernels(fn):
    """(library kernels, other kernels, memsets) among the device records of fn"""
    names = [n for n in launches.device_records(fn) if not n.startswith("Memcpy")]
    lib = [n for n in names if "sr::" in n]
    fills = [n for n in names if n.startswith("Memset") or "fill" in n.lower()]
    return lib, [n for n in names if n not in lib and n not in fills], fills


@pytest.mark.parametrize("N", [1, 2, 3, 255, 256, 257, 65536, 65537, 1_000_003])
def test_draw_rows_equals_the_restatement(hip_device, N):
    from splatfields_amd import draw_rows
    for n in sorted({1, N // 3, N - 1, N}):
        want = R.draw_rows(N, n, SEED)
        assert np.unique(want).size == n and (n == 0 or (want.min() >= 0 and want.max() < N))
        got, flag = draw_rows(N, n, seed=SEED, device=hip_device, return_flag=True)
        asc, flag_a = draw_rows(N, n, seed=SEED, order="ascending", device=hip_device, return_flag=True)
        assert got.dtype is torch.int64 and got.shape == (n,) and asc.shape == (n,)
        assert torch.equal(got.cpu(), torch.from_numpy(want)), (N, n)
        assert torch.equal(asc.cpu(), torch.from_numpy(np.sort(want))), (N, n)
        assert torch.equal(asc, torch.sort(got).values)
        assert int(flag) == 0 and int(flag_a) == 0
        assert torch.equal(draw_rows(N, n, seed=SEED, device=hip_device), got)                       # repeated calls: the same bits
        assert torch.equal(draw_rows(N, n, seed=SEED, order="ascending", device=hip_device), asc)
    assert not torch.equal(draw_rows(N, N, seed=SEED + 1, device=hip_device), draw_rows(N, N, seed=SEED, device=hip_device)) or N < 255


def test_draw_rows_of_the_largest_row_count_needs_no_memory_per_row(hip_device):
    from splatfields_amd import draw_rows
    N, n = 2 ** 31 - 1, 4096
    torch.cuda.reset_peak_memory_stats(hip_device)
    before = torch.cuda.memory_allocated(hip_device)
    got, flag = draw_rows(N, n, seed=SEED, device=hip_device, return_flag=True)
    assert torch.cuda.max_memory_allocated(hip_device) - before < 1 << 20
    assert torch.equal(got.cpu(), torch.from_numpy(R.draw_rows(N, n, SEED))) and int(flag) == 0
    assert got.unique().numel() == n and got.max().item() > 2 ** 30


def test_draw_rows_launch_counts_and_seeding(hip_device):
    from splatfields_amd import draw_rows
    N, n = 100_000, 30_000
    lib, other, fills = _kernels(lambda: draw_rows(N, n, seed=1, device=hip_device))
    assert len(lib) == 1 and not other and not fills, (lib, other, fills)
    lib, other, fills = _kernels(lambda: draw_rows(N, n, seed=1, order="ascending", device=hip_device))
    assert len(lib) == 3 and not other and len(fills) <= 1, (lib, other, fills)
    torch.manual_seed(77)
    a = draw_rows(N, n, device=hip_device)
    b = draw_rows(N, n, device=hip_device)
    torch.manual_seed(77)
    assert torch.equal(draw_rows(N, n, device=hip_device), a) and not torch.equal(a, b)            # torch.manual_seed governs the draw
    g = torch.Generator().manual_seed(3)
    c = draw_rows(N, n, generator=g, device=hip_device)
    assert torch.equal(draw_rows(N, n, generator=torch.Generator().manual_seed(3), device=hip_device), c)


def _model(N, sh_degree, isotropic, dev):
    gs = R.StandInGaussians(N, sh_degree=sh_degree, isotropic=isotropic, device=dev, seed=3)
    return gs, [gs._xyz, gs._scaling, gs._features_dc, gs._features_rest]


@pytest.mark.parametrize("isotropic", [False, True])
@pytest.mark.parametrize("sh_degree", [3, 0])
def test_gather_rows_forward_and_backward(hip_device, isotropic, sh_degree):
    from splatfields_amd import draw_rows, gather_rows
    N, n = 1000, 300
    gs, params = _model(N, sh_degree, isotropic, hip_device)
    idx = draw_rows(N, n, seed=SEED, device=hip_device)
    op = "exp3" if isotropic else "exp"
    call = lambda: gather_rows(idx, gs._xyz, gs._scaling, (gs._features_dc, gs._features_rest), ops=("copy", op, "copy"))
    xyz, scaling, feats = call()
    assert xyz.shape == (n, 3) and scaling.shape == (n, 3) and feats.shape == (n, (sh_degree + 1) ** 2, 3)
    assert torch.equal(xyz, gs._xyz[idx]) and torch.equal(feats, gs.get_features[idx])
    s64 = torch.exp(gs._scaling.detach().double().cpu())
    s64 = (s64.repeat(1, 3) if isotropic else s64)[idx.cpu()]
    accuracy.within("gather_rows", f"exp iso={isotropic}", {"scaling": scaling}, {"scaling": s64}, {"scaling": gs.get_scaling.detach()[idx].cpu()})
    lib, other, fills = _kernels(call)
    assert len(lib) == 1 and not other and not fills, (lib, other, fills)

    g = torch.Generator().manual_seed(5)
    ups = [torch.randn(t.shape, generator=g).to(hip_device) for t in (xyz, scaling, feats)]
    ours = torch.autograd.grad([xyz, scaling, feats], params, ups, allow_unused=True)
    ref = torch.autograd.grad([gs._xyz[idx], gs.get_scaling[idx], gs.get_features[idx]], params, ups, allow_unused=True)
    for k in (0, 2, 3):                                                    # the copies: PyTorch's index backward, bit for bit
        assert torch.equal(ours[k], ref[k]), k
    up64, x64 = ups[1].double().cpu(), gs._scaling.detach().double().cpu()
    d64 = torch.zeros_like(x64)
    d64[idx.cpu()] = (up64.sum(dim=1, keepdim=True) if isotropic else up64) * torch.exp(x64[idx.cpu()])
    accuracy.within("gather_rows", f"exp backward iso={isotropic}", {"d_scaling": ours[1]}, {"d_scaling": d64}, {"d_scaling": ref[1].cpu()})
    assert torch.equal(torch.autograd.grad(call(), params, ups, allow_unused=True)[1], ours[1])          # repeats: the same bits
    outs = call()
    lib, other, fills = _kernels(lambda: torch.autograd.grad(outs, params, ups, allow_unused=True))
    assert len(lib) == 1 and not other and len(fills) <= 4, (lib, other, fills)
    # only the inputs that ask get a gradient, and a detached input gives a detached result
    a, b = gather_rows(idx, gs._xyz.detach(), gs._features_dc)
    assert not a.requires_grad and b.requires_grad


def test_gather_rows_flags_a_row_out_of_range_without_a_host_read(hip_device):
    from splatfields_amd import gather_rows
    N = 1000
    gs, _ = _model(N, 3, False, hip_device)
    idx = torch.tensor([5, N, 7, -1, 0], device=hip_device)
    call = lambda: gather_rows(idx, gs._xyz.detach(), gs._scaling.detach(), (gs._features_dc.detach(), gs._features_rest.detach()),
                               ops=("copy", "exp", "copy"), return_flag=True)
    lib, other, fills = _kernels(call)                                      # the flag's zero fill and one launch: no copy to the host
    assert len(lib) == 1 and not other and len(fills) == 1 and not [n for n in launches.device_records(call) if n.startswith("Memcpy")]
    xyz, scaling, feats, flag = call()
    assert int(flag) == 1
    for t in (xyz, scaling, feats):
        bad = torch.isnan(t.reshape(5, -1))
        assert bad[[1, 3]].all() and not bad[[0, 2, 4]].any()
    assert torch.equal(xyz[[0, 2, 4]], gs._xyz.detach()[[5, 7, 0]])
    assert int(gather_rows(idx[[0, 2, 4]], gs._xyz.detach(), return_flag=True)[1]) == 0


def _stats_case(dev, N=2000, n=500):
    g = torch.Generator().manual_seed(9)
    grad = torch.randn(n, 3, generator=g).to(dev)
    radii = (torch.randint(1, 40, (n,), generator=g, dtype=torch.int32) * (torch.rand(n, generator=g) < 0.5)).to(torch.int32).to(dev)
    accum, denom, maxr = torch.rand(N, 1, generator=g).to(dev), torch.randint(0, 5, (N, 1), generator=g).float().to(dev), (30 * torch.rand(N, generator=g)).to(dev)
    return grad, radii, accum, denom, maxr


def _gather_update_scatter(grad, radii, idx, accum, denom, maxr):
    """the statistics through a row list with PyTorch indexing around the existing op: gather the drawn rows, run
    densification_stats on the copies, scatter them back"""
    from splatfields_amd import densification_stats
    copies = [t[idx].contiguous() for t in (accum, denom, maxr)]
    densification_stats(grad, radii, *copies)
    for t, c in zip((accum, denom, maxr), copies):
        t[idx] = c


def test_densification_stats_through_the_row_list(hip_device):
    from splatfields_amd import densification_stats, draw_rows
    N, n = 2000, 500
    grad, radii, accum, denom, maxr = _stats_case(hip_device, N, n)
    idx = draw_rows(N, n, seed=SEED, device=hip_device)
    assert 150 < int((radii > 0).sum()) < 350
    hidden, free = idx[radii == 0][0], int(torch.ones(N, dtype=torch.bool).index_fill_(0, idx.cpu(), False).nonzero()[0])
    maxr[hidden] = float("nan")                                            # a drawn row that is not visible, and a row that was not drawn
    maxr[free] = float("nan")
    before = [t.clone() for t in (accum, denom, maxr)]
    want = [t.clone() for t in before]
    _gather_update_scatter(grad, radii, idx, *want)
    call = lambda: densification_stats(grad, radii, accum, denom, maxr, idx=idx)
    lib, other, fills = _kernels(call)
    assert len(lib) == 1 and not other and not fills, (lib, other, fills)
    accum, denom, maxr = [t.clone() for t in before]
    call()
    as_bits = lambda t: t.view(torch.int32)
    for got, exp in zip((accum, denom, maxr), want):
        assert torch.equal(as_bits(got), as_bits(exp))
    keep = torch.ones(N, dtype=torch.bool, device=hip_device)
    keep[idx[radii > 0]] = False
    for got, old in zip((accum, denom, maxr), before):
        assert torch.equal(as_bits(got)[keep], as_bits(old)[keep])
    assert torch.isnan(maxr[hidden]) and torch.isnan(maxr[free])
    ref = [t.clone() for t in before]
    R.stats_through_idx(grad, radii, idx, *ref)                            # the reference's clone / mask / assign form: torch.norm rounds on its own
    assert torch.allclose(accum, ref[0], rtol=1e-6, atol=1e-7) and torch.equal(denom, ref[1]) and torch.equal(as_bits(maxr), as_bits(ref[2]))
    only = before[2].clone()
    densification_stats(grad, radii, None, None, only, idx=idx)            # any output may be missing
    assert torch.equal(as_bits(only), as_bits(maxr))


def _scene(dev, N=2000):
    from splatfields_amd.synthetic import make_camera, make_splats
    sp = make_splats(N, seed=21, mean_scale=0.05, device=dev)
    gs = R.StandInGaussians(N, device=dev)
    gs._xyz = sp["means3D"].clone().requires_grad_(True)
    gs._scaling = torch.log(sp["scales"]).requires_grad_(True)
    gs._features_dc = sp["shs"][:, :1].contiguous().requires_grad_(True)
    gs._features_rest = sp["shs"][:, 1:].contiguous().requires_grad_(True)
    cam = make_camera(1, 96, 80, device=dev)
    cam.fid = torch.tensor([0.25])
    return gs, cam


def test_subset_step_end_to_end(hip_device):
    """get_gaussian_dict -> render -> loss -> backward -> densification_stats(idx=) against the same step through the PyTorch
    restatement with the same rows"""
    from splatfields_amd import densification_stats, get_gaussian_dict, render
    N, n = 2000, 500
    gs, cam = _scene(hip_device, N)
    pipe, bg = types.SimpleNamespace(debug=False), torch.ones(3, device=hip_device)
    params = {"dc": gs._features_dc, "rest": gs._features_rest, "xyz": gs._xyz, "scaling": gs._scaling}

    def step(make_dict, stats):
        deform = R.StubDeform(None, device=hip_device)
        for p in params.values():
            p.grad = None
        d, over = make_dict(deform)
        pkg = render(cam, d, pipe, bg)
        loss = (pkg["render"] - 0.5).abs().mean() + 0.1 * pkg["opacity"].mean()
        loss.backward()
        g = _stats_case(hip_device, N, n)
        accum, denom, maxr = g[2], g[3], g[4]
        stats(pkg["viewspace_points"].grad, pkg["radii"], d["idx"], accum, denom, maxr)
        grads = {k: (None if p.grad is None else p.grad.clone()) for k, p in params.items()}
        grads["w"] = deform.w.grad.clone()
        return d, over, pkg, grads, (accum, denom, maxr)

    ours = step(lambda deform: get_gaussian_dict(cam, gs, deform, iteration=5, warm_up=2, n_splats=n, seed=SEED),
                lambda vg, radii, idx, *s: densification_stats(vg, radii, *s, idx=idx))
    idx = ours[0]["idx"]
    assert torch.equal(idx.cpu(), torch.from_numpy(R.draw_rows(N, n, SEED, order="ascending")))
    ref = step(lambda deform: R.get_gaussian_dict(cam, gs, deform, iteration=5, warm_up=2, n_splats=n, idx=idx),
               lambda vg, radii, idx, *s: _gather_update_scatter(vg, radii, idx, *s))
    assert set(ours[0]) == set(ref[0]) and set(ours[1]) == set(ref[1])
    for k in ("means3D", "gaussian_opacity", "gaussian_scales", "gaussian_rotations", "gaussian_features"):
        assert torch.equal(ours[0][k], ref[0][k]), k
    for k in ("f_dc", "f_rest", "xyz", "opacity", "scaling", "rotation"):
        assert torch.equal(ours[1][k], ref[1][k]), k
    for k in ("render", "depth", "opacity", "radii"):
        assert torch.equal(ours[2][k], ref[2][k]), k
    assert int((ours[2]["radii"] > 0).sum()) > 50
    assert torch.equal(ours[2]["viewspace_points"].grad, ref[2]["viewspace_points"].grad)
    for k in ("dc", "rest", "w"):                                          # what the restatement reaches through plain indexing
        assert torch.equal(ours[3][k], ref[3][k]), k
    assert ours[3]["xyz"] is None and ours[3]["scaling"] is None and ref[3]["xyz"] is None and ref[3]["scaling"] is None
    for a, b in zip(ours[4], ref[4]):
        assert torch.equal(a.view(torch.int32), b.view(torch.int32))
    # n_splats >= N and <= 0: the full step, idx None
    for n_splats in (N, -1):
        d, _ = get_gaussian_dict(cam, gs, R.StubDeform(None, device=hip_device), n_splats=n_splats)
        e, _ = R.get_gaussian_dict(cam, gs, R.StubDeform(None, device=hip_device), n_splats=n_splats)
        assert d["idx"] is None and torch.equal(d["means3D"], e["means3D"]) and torch.equal(d["gaussian_features"], e["gaussian_features"])


def _hull_inputs():
    masks, krt = np.zeros((2, 32, 32), np.uint8), np.zeros((2, 3, 4))
    masks[:, 4:28, 4:28] = 1
    for v, axes in enumerate(((0, 1), (1, 2))):                            # two orthographic-like views: u = 16 + 10 a, v = 16 + 10 b, h2 = 1
        krt[v, 0, axes[0]], krt[v, 0, 3] = 10.0, 16.0
        krt[v, 1, axes[1]], krt[v, 1, 3] = 10.0, 16.0
        krt[v, 2, 3] = 1.0
    return masks, krt


def test_initialisations_pick_with_the_keyed_draw(hip_device):
    from splatfields_amd import depth_points, visual_hull
    masks, krt = _hull_inputs()
    kw = dict(grid_resolution=24, aabb=(-1.5, 1.5), device=hip_device, return_indices=True)
    full, full_idx = visual_hull(masks, krt, **kw)
    M, k = full.shape[0], 200
    assert M > 2 * k
    xyz, idx = visual_hull(masks, krt, n_pts=k, draw="keyed", generator=torch.Generator().manual_seed(1), **kw)
    assert xyz.shape == (k, 3) and idx.unique().numel() == k
    at = torch.searchsorted(full_idx, idx)                                  # the full result is in grid order: indices ascend
    assert torch.equal(full_idx[at], idx) and torch.equal(full[at], xyz)
    again, _ = visual_hull(masks, krt, n_pts=k, draw="keyed", generator=torch.Generator().manual_seed(1), **kw)
    assert torch.equal(again, xyz)
    # the default: the permutation of the same generator, through the unchanged code path
    old, old_idx = visual_hull(masks, krt, n_pts=k, generator=torch.Generator().manual_seed(1), **kw)
    pick = torch.randperm(M, generator=torch.Generator().manual_seed(1))[:k].to(hip_device)
    assert torch.equal(old, full[pick]) and torch.equal(old_idx, full_idx[pick])
    both, _ = visual_hull(masks, krt, n_pts=k, draw="permutation", generator=torch.Generator().manual_seed(1), **kw)
    assert torch.equal(both, old)

    g = torch.Generator().manual_seed(4)
    depths = torch.rand(2, 20, 24, generator=g) * 3 - 0.8                    # about a quarter of the pixels are dropped
    kinv = torch.linalg.inv(torch.tensor([[30.0, 0, 12], [0, 30.0, 10], [0, 0, 1]])).expand(2, 3, 3)
    poses = torch.eye(4)[:3].expand(2, 3, 4).clone()
    poses[1, :, 3] = torch.tensor([0.5, 0.0, 0.1])
    dk = dict(device=hip_device, return_indices=True)
    cloud, _, cloud_idx = depth_points(depths, kinv, poses, **dk)
    M = cloud.shape[0]
    assert M > 2 * k
    xyz, _, idx = depth_points(depths, kinv, poses, n_pts=k, draw="keyed", generator=torch.Generator().manual_seed(2), **dk)
    assert xyz.shape == (k, 3) and idx.unique().numel() == k
    at = torch.searchsorted(cloud_idx, idx)
    assert torch.equal(cloud_idx[at], idx) and torch.equal(cloud[at], xyz)
    old, _, old_idx = depth_points(depths, kinv, poses, n_pts=k, generator=torch.Generator().manual_seed(2), **dk)
    pick = torch.randperm(M, generator=torch.Generator().manual_seed(2))[:k].to(hip_device)
    assert torch.equal(old, cloud[pick]) and torch.equal(old_idx, cloud_idx[pick])
