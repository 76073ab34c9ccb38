"""The restatements of tests/subset_reference.py, checked without a device: the keyed map is a bijection for every n_rows (what
ends the kernel's walk), the subsets it draws are uniform, and the PyTorch form of the reference's subset step agrees with itself
across its branches.  The GPU tests compare the kernels with exactly these functions."""
import math

import numpy as np
import pytest
import torch

import subset_reference as R

KEY_SEEDS = (0, 1, 0xDEADBEEF, 2 ** 63 + 12345, 2 ** 64 - 1)


def test_splitmix64_is_the_published_generator():
    # the first outputs for the seed 1234567, as printed by the public-domain reference implementation (Vigna, splitmix64.c)
    assert R.splitmix64(1234567, 3) == [6457827717110365317, 3203168211198807973, 9817491932198370423]
    assert R.keys_of(5) == R.splitmix64(5, R.ROUNDS) and len(R.keys_of(5)) == 8


def test_domain_is_the_smallest_power_of_two_and_below_twice_the_rows():
    for n in list(range(1, 70)) + [255, 256, 257, 65535, 65536, 65537, 2 ** 31 - 1]:
        lo, hi = R.halves(n)
        assert 0 <= hi - lo <= 1 and (1 << (lo + hi)) >= n and (n == 1 or (1 << (lo + hi)) < 2 * n), n
    assert R.halves(1) == (0, 0) and R.halves(2 ** 31 - 1) == (15, 16)


def test_map_is_a_bijection_for_every_row_count():
    """exhaustive for N = 1 .. 4097 and 65535, 65536, 65537, five key sets each: P hits every row once, P^-1 undoes it, and no walk
    is longer than 64 steps"""
    longest = 0
    sizes = list(range(1, 4098)) + [65535, 65536, 65537]
    for seed in KEY_SEEDS:
        keys = R.keys_of(seed)
        tables = {}
        for n in sizes:
            bits = sum(R.halves(n))
            if bits not in tables:
                fwd, inv = R.domain_table(n, keys), R.domain_table(n, keys, inverse=True)
                assert np.array_equal(np.sort(fwd), np.arange(1 << bits, dtype=np.uint64)), (seed, bits)     # F is a bijection of the domain
                assert np.array_equal(inv[fwd], np.arange(1 << bits, dtype=np.uint64)), (seed, bits)        # and the reversed rounds undo it
                tables[bits] = (fwd, inv)
            fwd, inv = tables[bits]
            rows = np.arange(n, dtype=np.uint64)
            p, walk = R.permute(rows, n, keys, table=fwd, return_walk=True)
            longest = max(longest, walk)
            assert p.min() >= 0 and np.array_equal(np.sort(p), np.arange(n)), (seed, n)
            back, walk = R.permute(p, n, keys, table=inv, return_walk=True)
            longest = max(longest, walk)
            assert np.array_equal(back, np.arange(n)), (seed, n)
    print(f"longest cycle walk over {len(sizes)} sizes x {len(KEY_SEEDS)} key sets: {longest} steps")
    assert longest <= 64


def test_table_lookup_is_the_network():
    """the exhaustive test walks through tables: the same values as the network evaluated per element"""
    for n in (1, 2, 3, 5, 1000, 4097, 65537):
        keys = R.keys_of(n)
        rows = np.arange(n, dtype=np.uint64)
        assert np.array_equal(R.permute(rows, n, keys), R.permute(rows, n, keys, table=R.domain_table(n, keys)))
        assert np.array_equal(R.permute(R.permute(rows, n, keys), n, keys, inverse=True), np.arange(n))


def test_large_row_counts_need_no_table():
    n = 2 ** 31 - 1
    idx = R.draw_rows(n, 4096, seed=3)
    assert idx.min() >= 0 and idx.max() < n and np.unique(idx).size == 4096
    assert np.array_equal(R.permute(idx, n, R.keys_of(3), inverse=True), np.arange(4096))
    assert np.array_equal(R.draw_rows(n, 4096, seed=3, order="ascending"), np.sort(idx))


def test_subsets_are_uniform():
    """N = 1000, n = 100, S = 4000 fixed seeds.  Under a uniform sampler a row's inclusion count is Binomial(S, n/N) and its count
    of appearances in position 0 is Binomial(S, 1/N); 6 sigma on either side is exceeded with probability < 2e-9 per row (normal
    tail; the binomial's is of the same order), < 1000 x 2e-9 for any row."""
    N, n, S = 1000, 100, 4000
    included, first = np.zeros(N, np.int64), np.zeros(N, np.int64)
    for seed in range(S):
        idx = R.draw_rows(N, n, seed=seed)
        assert np.unique(idx).size == n
        included[idx] += 1
        first[idx[0]] += 1
    for name, counts, p in (("inclusion", included, n / N), ("position 0", first, 1 / N)):
        mean, sigma = S * p, math.sqrt(S * p * (1 - p))
        worst = np.abs(counts - mean).max() / sigma
        print(f"{name}: mean {mean:.1f}, sigma {sigma:.2f}, worst deviation {worst:.2f} sigma (bound 6)")
        assert counts.sum() == S * (n if name == "inclusion" else 1)
        assert worst <= 6.0, (name, worst)


def _dict_equal(a, b):
    assert a.keys() == b.keys()
    for k in a:
        if torch.is_tensor(a[k]):
            assert torch.equal(a[k], b[k]), k
        elif callable(a[k]):
            dirs = torch.zeros(3)
            assert torch.equal(a[k](dirs), b[k](dirs)), k
        else:
            assert a[k] == b[k], k


@pytest.mark.parametrize("colour", [None, "features", "rgb", "rgb_fnc"])
@pytest.mark.parametrize("isotropic", [False, True])
def test_restated_get_gaussian_dict_agrees_with_itself(colour, isotropic):
    """the subset step through a row list equals the full step's rows, in every colour branch; n_splats >= N and <= 0 are the full
    step; the static / warm-up branch ignores the subset"""
    N, n = 50, 17
    gs = R.StandInGaussians(N, isotropic=isotropic)
    cam, deform = R.StandInCamera(), R.StubDeform(colour, gradient_error=colour == "rgb")
    idx = torch.from_numpy(R.draw_rows(N, n, seed=11, order="ascending"))
    full, over_full = R.get_gaussian_dict(cam, gs, deform)
    sub, over_sub = R.get_gaussian_dict(cam, gs, deform, n_splats=n, idx=idx)
    assert full["idx"] is None and torch.equal(sub["idx"], idx)
    want = {"idx", "means3D", "active_sh_degree", "gaussian_opacity", "gaussian_scales", "gaussian_rotations", "gradient_error",
            {None: "gaussian_features", "features": "gaussian_features", "rgb": "gaussian_rgb", "rgb_fnc": "gaussian_rgb_fnc"}[colour]}
    assert set(sub) == set(full) == want
    for k in ("means3D", "gaussian_opacity", "gaussian_scales", "gaussian_rotations", "gaussian_features", "gaussian_rgb"):
        if k in full:
            assert sub[k].shape[0] == n and torch.allclose(sub[k], full[k][idx], rtol=1e-6, atol=1e-7), k   # a row's values do not depend on its neighbours (up to the matmul's blocking)
    if colour is None:
        assert torch.equal(sub["gaussian_features"], gs.get_features[idx])
    assert torch.equal(sub["gaussian_scales"], over_sub["scaling"] + gs.get_scaling.detach()[idx])
    assert over_sub["f_dc"].shape == (N, 1, 3) and over_sub["f_rest"].shape == (N, 15, 3) and over_sub["xyz"] is sub["means3D"]
    for n_splats in (N, N + 1, 0, -1):
        again, _ = R.get_gaussian_dict(cam, gs, deform, n_splats=n_splats, idx=idx)
        _dict_equal(again, full)
    for kw in (dict(static=True), dict(iteration=3, warm_up=10)):
        warm, over = R.get_gaussian_dict(cam, gs, deform, n_splats=n, idx=idx, **kw)
        assert over is None and "idx" not in warm and warm["means3D"] is gs.get_xyz and warm["gaussian_scales"].shape == (N, 3)
    late, over = R.get_gaussian_dict(cam, gs, deform, iteration=10, warm_up=10, n_splats=n, idx=idx)
    assert over is not None and torch.equal(late["idx"], idx)


def test_restated_stats_touch_only_drawn_visible_rows():
    N, n = 40, 12
    g = torch.Generator().manual_seed(2)
    idx = torch.from_numpy(R.draw_rows(N, n, seed=4))
    grad, radii = torch.randn(n, 3, generator=g), torch.randint(0, 3, (n,), generator=g, dtype=torch.int32)
    accum, denom, maxr = torch.rand(N, 1, generator=g), torch.rand(N, 1, generator=g).round(), torch.rand(N, generator=g)
    maxr[idx[radii == 0][:1]] = float("nan")
    a0, d0, m0 = accum.clone(), denom.clone(), maxr.clone()
    R.stats_through_idx(grad, radii, idx, accum, denom, maxr)
    seen = idx[radii > 0]
    untouched = torch.ones(N, dtype=torch.bool)
    untouched[seen] = False
    for new, old in ((accum, a0), (denom, d0), (maxr, m0)):
        assert torch.equal(new[untouched].view(torch.int32), old[untouched].view(torch.int32))
    assert torch.equal(denom[seen], d0[seen] + 1) and torch.equal(accum[seen], a0[seen] + grad[radii > 0, :2].norm(dim=-1, keepdim=True))
    assert torch.equal(maxr[seen], torch.max(m0[seen], radii[radii > 0].float()))
