"""The depth-map initialisation on the GPU (splatfields_amd.init.depth_points and its companions, csrc/depth_init.hip) against the
float64 restatement (tests/depth_init_reference.py) and the reference's own outputs (tests/golden/depth_init_cases.npz).

Which pixels survive, their order, their pixel indices and their colours involve no rounding: they must be EQUAL to the
restatement's.  The kernel evaluates the restatement's expressions in double, in the same order, without fused multiply-adds, and
rounds to float32 once, so every coordinate must lie within R.coordinate_bound of the float64 value: half a float32 ulp of it plus
1e-12 of the largest coordinate (derived there, not measured)."""
import functools

import numpy as np
import pytest
import torch

from tests import depth_init_reference as R
from tests.launches import stage_counts
from tests.scan_round import BLOCK, SCAN_ROUND

pytestmark = pytest.mark.gpu


# ---- inputs ----------------------------------------------------------------------------------------------------------------
def cameras(B, H, W, seed):
    """generic cameras: (Kinv [B,3,3], pose [B,4,4]) float64 -- a pinhole with skew, seen from B poses around the origin"""
    rng = np.random.default_rng(seed)
    kinv, pose = [], []
    for _ in range(B):
        f = 1.2 * max(W, H, 4) * rng.uniform(0.9, 1.1)
        K = np.array([[f, rng.uniform(-0.5, 0.5), (W - 1) / 2 + rng.uniform(-1, 1)], [0.0, f * rng.uniform(0.95, 1.05), (H - 1) / 2 + rng.uniform(-1, 1)],
                      [0.0, 0.0, 1.0]])
        c = rng.normal(size=3)
        c = 3.0 * c / np.linalg.norm(c)
        z = -c / np.linalg.norm(c)
        x = np.cross(rng.normal(size=3), z)
        x /= np.linalg.norm(x)
        c2w = np.eye(4)
        c2w[:3, :3], c2w[:3, 3] = np.stack([x, np.cross(z, x), z]).T, c
        kinv.append(np.linalg.inv(K))
        pose.append(c2w)
    return np.stack(kinv), np.stack(pose)


@functools.lru_cache(maxsize=None)
def case(B, H, W, valid=0.4):
    """inputs and the restatement's outputs of one batch, made once: about `valid` of the depths are positive, the others 0 or -1"""
    rng = np.random.default_rng(1000 * B + 10 * H + W)
    kinv, pose = cameras(B, H, W, 7 * B + 3 * H + W)
    d = rng.uniform(2.2, 3.8, (B, H, W)).astype(np.float32)
    kind = rng.uniform(size=(B, H, W))
    d[kind > valid] = 0.0
    d[kind > valid + (1 - valid) / 2] = -1.0
    if B * H * W == 1:
        d[...] = 2.5
    images = rng.integers(0, 256, (B, H, W, 3), dtype=np.uint8)
    xyz, rgb, idx = R.back_project(d, kinv, pose, images=images)
    for a in (d, kinv, pose, images, xyz, rgb, idx):
        a.setflags(write=False)
    return dict(depths=d, kinv=kinv, pose=pose, images=images, xyz=xyz, rgb=rgb, idx=idx)


def run(c, **kw):
    import splatfields_amd as S
    kw.setdefault("images", c.get("images"))
    xyz, rgb, idx = S.depth_points(c["depths"], c["kinv"], c["pose"], return_indices=True, **kw)
    assert xyz.is_cuda and xyz.dtype is torch.float32 and xyz.dim() == 2 and xyz.shape[1] == 3
    assert idx.is_cuda and idx.dtype is torch.int64 and idx.shape == (xyz.shape[0],)
    assert rgb is None or (rgb.is_cuda and rgb.shape == xyz.shape)
    return xyz, rgb, idx


def assert_rows(got, want_xyz, want_rgb, want_idx):
    """indices and colours EQUAL, coordinates within the derived bound; returns the worst observed share of the bound"""
    xyz, rgb, idx = got
    assert np.array_equal(idx.cpu().numpy(), want_idx), (len(idx), len(want_idx))
    if want_rgb is not None:
        assert rgb.dtype is torch.from_numpy(want_rgb[:0].copy()).dtype and np.array_equal(rgb.cpu().numpy(), want_rgb)
    if not len(want_idx):
        assert xyz.shape == (0, 3)
        return 0.0
    err = np.abs(xyz.cpu().numpy().astype(np.float64) - want_xyz)
    share = float((err / R.coordinate_bound(want_xyz)).max())
    print(f"{len(want_idx)} rows, largest coordinate error {err.max():.3e}, {share:.3f} of the bound")
    assert share <= 1.0
    return share


def bounds_of(c, **kw):
    import splatfields_amd as S
    b = S.depth_points_bounds(c["depths"], c["kinv"], c["pose"], **kw)
    assert b.is_cuda and b.dtype is torch.float32 and b.shape == (2,)
    return b


# ---- every size at which the kernels take another path ---------------------------------------------------------------------
# B H W of 1, 63, 64, 65, 255, 256, 257 and 27 300 (a partial last workgroup and more than 100 workgroups); 1 x 9 and 9 x 1
# SCAN_ROUND and SCAN_ROUND + 1 images of 16 x 16 pixels, one workgroup each: k_depth_scan walks one count per workgroup (a full round
# of ordered_scan, and the first count of a second one)
SCAN_SHAPES = [(SCAN_ROUND, 16, 16), (SCAN_ROUND + 1, 16, 16)]
SHAPES = [(1, 1, 1), (1, 7, 9), (1, 8, 8), (1, 5, 13), (1, 15, 17), (1, 16, 16), (1, 1, 257), (3, 130, 70), (1, 1, 9), (1, 9, 1), (2, 9, 1)] + SCAN_SHAPES


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_cloud_and_bounds_equal_the_restatement(shape):
    c = case(*shape)
    assert len(c["idx"]) > 0
    got = run(c)
    assert_rows(got, c["xyz"], c["rgb"], c["idx"])
    bounds = bounds_of(c)
    assert torch.equal(bounds, torch.stack([got[0].min(), got[0].max()]))              # this path's own cloud, bit for bit
    top = np.abs(c["xyz"]).max()
    for value, want in ((float(bounds[0]), c["xyz"].min()), (float(bounds[1]), c["xyz"].max())):
        assert abs(value - want) <= 0.5 * R.ulp32(want) + 1e-12 * top


def test_all_none_and_exactly_one_valid_pixel():
    """2 x 9 x 17 = 306 pixels: two workgroups, the second partial"""
    base = case(2, 9, 17)
    n = 306
    everything = R.back_project(np.full((2, 9, 17), 3.0, np.float32), base["kinv"], base["pose"], images=base["images"])
    assert len(everything[2]) == n
    assert_rows(run(dict(base, depths=np.full((2, 9, 17), 3.0, np.float32))), *everything)
    for fill in (0.0, -1.0):
        c = dict(base, depths=np.full((2, 9, 17), fill, np.float32))
        xyz, rgb, idx = run(c)
        assert xyz.shape == (0, 3) and rgb.shape == (0, 3) and rgb.dtype is torch.uint8 and idx.shape == (0,)
        assert bounds_of(c).tolist() == [float("inf"), float("-inf")]
        xyz, rgb, idx = run(c, n_pts=5)
        assert xyz.shape == (0, 3) and idx.shape == (0,)
    for at in (0, n - 1, 63, 127, 255, 256):        # the first and the last pixel of the batch, the last bit of a word, of a workgroup
        d = np.full(n, -1.0, np.float32)
        d[at] = 2.75
        c = dict(base, depths=d.reshape(2, 9, 17))
        want = R.back_project(c["depths"], c["kinv"], c["pose"], images=c["images"])
        assert want[2].tolist() == [at]
        got = run(c)
        assert_rows(got, *want)
        assert torch.equal(bounds_of(c), torch.stack([got[0].min(), got[0].max()]))
        assert torch.equal(run(c, ranks=[0])[0], got[0])


def test_an_empty_batch():
    import splatfields_amd as S
    z = np.zeros((0, 4, 5), np.float32)
    xyz, rgb, idx = S.depth_points(z, np.zeros((0, 3, 3)), np.zeros((0, 3, 4)), images=np.zeros((0, 4, 5, 3), np.uint8), return_indices=True, device="cuda")
    assert xyz.shape == (0, 3) and rgb.shape == (0, 3) and idx.shape == (0,) and xyz.is_cuda
    assert S.depth_points_bounds(z, np.zeros((0, 3, 3)), np.zeros((0, 3, 4)), device="cuda").tolist() == [float("inf"), float("-inf")]


# ---- which depths survive ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_depth_values_are_kept_exactly_as_greater_than_zero_says(dtype):
    tiny = np.finfo(dtype).smallest_subnormal
    d = np.array([[[0.0, -0.0, -1.0, np.nan, np.inf, tiny, 1e30, 2.0, -np.inf]]], dtype)            # 1 x 9
    assert d[0, 0, 5] > 0
    kinv, pose = cameras(1, 1, 9, 77)
    want_xyz, _, want_idx = R.back_project(d, kinv, pose)
    assert want_idx.tolist() == [4, 5, 6, 7]
    xyz, _, idx = run(dict(depths=d, kinv=kinv, pose=pose))
    assert idx.tolist() == [4, 5, 6, 7]
    got = xyz.cpu().numpy()
    assert np.all(np.isinf(want_xyz[0])) and np.array_equal(got[0], want_xyz[0].astype(np.float32))   # +inf depth: signed infinities
    for row in (1, 2, 3):                                        # each against its own magnitude: the 1e30 row would hide the others
        assert np.all(np.abs(got[row].astype(np.float64) - want_xyz[row]) <= R.coordinate_bound(want_xyz[row])), row
    assert np.all(np.isfinite(got[2])) and np.abs(got[2]).max() > 1e29
    assert np.array_equal(got[1], pose[0, :3, 3].astype(np.float32))                                # the subnormal depth: the origin itself


def test_nan_coordinates_are_written_and_skipped_by_the_bounds():
    """identity cameras, pixel (0, 0): the ray is (0, 0, 1), so a depth of +inf gives the row (NaN, NaN, +inf) -- inf * 0.  The row
    is kept and written as it is; the bounds skip its NaN coordinates and take its infinite one"""
    eye = np.eye(4)[None]
    d = np.array([[[np.inf, 2.0, -1.0]]], np.float32)
    c = dict(depths=d, kinv=eye, pose=eye)
    xyz, _, idx = run(c)
    got = xyz.cpu().numpy()
    assert idx.tolist() == [0, 1] and np.isnan(got[0, 0]) and np.isnan(got[0, 1]) and got[0, 2] == np.inf
    want = R.back_project(d, eye, eye)[0]
    assert np.array_equal(got, want.astype(np.float32), equal_nan=True)
    assert bounds_of(c).tolist() == [float(np.nanmin(got)), float(np.nanmax(got))] == [0.0, float("inf")]
    c = dict(c, depths=np.array([[[np.inf, -1.0, -1.0]]], np.float32))
    assert bounds_of(c).tolist() == [float("inf"), float("inf")]


# ---- masks, depth dtypes, image dtypes --------------------------------------------------------------------------------------
def test_mask_dtypes_and_layouts_equal_pre_masked_depth():
    c = case(3, 130, 70)
    rng = np.random.default_rng(3)
    inside = rng.uniform(size=c["depths"].shape) < 0.6
    pre = np.where(inside, c["depths"], np.float32(-1.0))
    want = R.back_project(pre, c["kinv"], c["pose"], images=c["images"])
    assert 0 < len(want[2]) < len(c["idx"])
    ref = run(dict(c, depths=pre))
    assert_rows(ref, *want)
    masks = (inside, inside.astype(np.uint8) * 255, np.where(inside, 0.25, -3.0), np.where(inside, 1e-30, 0.0).astype(np.float32),
             torch.from_numpy(inside)[..., None].cuda(), inside.astype(np.int64)[..., None])
    for m in masks:
        got = run(c, masks=m)
        assert all(torch.equal(a, b) for a, b in zip(got, ref))
        assert torch.equal(bounds_of(c, masks=m), bounds_of(dict(c, depths=pre)))
    assert np.array_equal(R.back_project(c["depths"], c["kinv"], c["pose"], masks=masks[2])[2], want[2])


def test_float32_and_float64_depth_agree_and_tensors_are_accepted():
    c = case(1, 15, 17)
    ref = run(c)
    for depths in (c["depths"].astype(np.float64), torch.from_numpy(c["depths"].copy()).cuda(), torch.from_numpy(c["depths"].astype(np.float64))):
        got = run(dict(c, depths=depths, kinv=torch.from_numpy(c["kinv"].copy()), pose=torch.from_numpy(c["pose"][:, :3, :4].copy()).cuda()))
        assert all(torch.equal(a, b) for a, b in zip(got, ref))
    k4 = np.zeros((1, 4, 4))
    k4[:, :3, :3] = c["kinv"]
    assert torch.equal(run(dict(c, kinv=k4))[0], ref[0])
    d64 = c["depths"].astype(np.float64) * (1.0 + 2.0 ** -40)                     # not float32-representable: used as they are
    want = R.back_project(d64, c["kinv"], c["pose"])
    assert_rows(run(dict(c, depths=d64, images=None)), want[0], None, want[2])


@pytest.mark.parametrize("dtype", [np.uint8, np.float32, np.float64, np.int64, np.bool_])
def test_image_elements_of_1_4_and_8_bytes_are_copied_exactly(dtype):
    c = case(1, 5, 13)
    rng = np.random.default_rng(9)
    if np.issubdtype(dtype, np.floating):
        images = rng.normal(size=(1, 5, 13, 3)).astype(dtype)
        images[0, 0, :4, 0] = [np.inf, -0.0, np.finfo(dtype).smallest_subnormal, np.finfo(dtype).max]
    else:
        images = rng.integers(0, 2 if dtype is np.bool_ else 200, (1, 5, 13, 3)).astype(dtype)
    xyz, rgb, idx = run(c, images=images)
    assert rgb.cpu().numpy().dtype == dtype
    assert rgb.cpu().numpy().tobytes() == images.reshape(-1, 3)[c["idx"]].tobytes()
    xyz, rgb, idx = run(c, images=torch.from_numpy(images).cuda(), ranks=[len(c["idx"]) - 1, 0])
    assert rgb.cpu().numpy().tobytes() == images.reshape(-1, 3)[c["idx"][[-1, 0]]].tobytes()
    import splatfields_amd as S
    with pytest.raises(ValueError, match="element size"):
        S.depth_points(c["depths"], c["kinv"], c["pose"], images=np.zeros(images.shape, np.float16), device="cuda")


# ---- bounds into the hull -----------------------------------------------------------------------------------------------------
def test_bounds_as_the_box_of_the_hull():
    import splatfields_amd as S
    from tests.test_gpu_hull import blob_masks, pinhole_views
    c = case(3, 130, 70)
    aabb = S.depth_points_bounds(c["depths"], c["kinv"], c["pose"], as_aabb=True)
    assert isinstance(aabb, tuple) and all(isinstance(a, float) for a in aabb)
    cloud = run(c)[0].cpu().numpy()
    host = (float(cloud.min()), float(cloud.max()))
    assert aabb == host
    masks, krt = blob_masks(1, (40, 52), 3, fill=0.45), pinhole_views(3, 11, (40, 52), distance=9.0)
    a = S.visual_hull(masks, krt, grid_resolution=24, aabb=aabb, return_indices=True)
    b = S.visual_hull(masks, krt, grid_resolution=24, aabb=host, return_indices=True)
    assert a[0].shape[0] > 0 and torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])


# ---- select -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(3, 130, 70), (1, 5, 13), SCAN_SHAPES[1]], ids=["27300", "65", "scan_round_plus_one"])
def test_ranks_equal_rows_of_the_full_cloud(shape):
    c = case(*shape)
    full = run(c)
    m = len(c["idx"])
    rng = np.random.default_rng(5)
    some = np.sort(rng.choice(m, min(m, 300), replace=False))
    # the survivors of the first SCAN_ROUND workgroups (the first round of k_depth_scan): its last, and the first of the second round
    first_round = int(np.searchsorted(c["idx"], SCAN_ROUND * BLOCK))
    assert first_round == m or 0 < first_round < m
    across = [0, first_round - 1, min(first_round, m - 1), m - 1]
    for ranks in (np.arange(m), some, some[::-1].copy(), np.repeat(some[:7], 3), rng.integers(0, m, 500), [0], [m - 1], [m - 1, 0, 0, m - 1], across):
        got = run(c, ranks=ranks)
        pick = torch.as_tensor(np.asarray(ranks, np.int64)).cuda()
        assert all(torch.equal(a, b[pick]) for a, b in zip(got, full)), ranks
    got = run(c, ranks=torch.as_tensor(some).cuda())
    assert torch.equal(got[0], full[0][torch.as_tensor(some).cuda()])
    empty = run(c, ranks=np.zeros(0, np.int64))
    assert empty[0].shape == (0, 3) and empty[1].shape == (0, 3) and empty[2].shape == (0,)


def test_out_of_range_ranks_give_nan_rows_and_set_the_flag():
    """documented in include/splatraster.h: a rank outside [0, M) reads nothing and writes NaN coordinates, zero colour bytes and
    the index -1; the flag word becomes 1 and is left alone otherwise"""
    from splatfields_amd import init as I
    c = case(1, 5, 13)
    full = run(c)
    m = len(c["idx"])
    ranks = np.array([-1, m, 0, 2 ** 40, m - 1, -2 ** 62, 2 ** 31, 2 ** 32], np.int64)
    bad = np.array([1, 1, 0, 1, 0, 1, 1, 1], bool)
    xyz, rgb, idx = run(c, ranks=ranks)
    assert torch.isnan(xyz[bad]).all() and not rgb[bad].any() and (idx[bad] == -1).all()
    good = torch.as_tensor(ranks[~bad]).cuda()
    assert torch.equal(xyz[~bad], full[0][good]) and torch.equal(rgb[~bad], full[1][good]) and torch.equal(idx[~bad], full[2][good])
    dev = torch.device("cuda", torch.cuda.current_device())
    b = I._DepthBatch(c["depths"], c["kinv"], c["pose"], c["images"].astype(np.float64), None, dev)
    ws, count, _ = b.mark()
    assert int(count) == m
    out = b.select(ws, torch.as_tensor(ranks), True)
    assert int(out[3]) == 1 and torch.isnan(out[0][bad]).all() and not out[1][bad].any() and out[1].dtype is torch.float64
    assert int(b.select(ws, torch.as_tensor(ranks[~bad]), True)[3]) == 0


def test_return_flag_hands_the_report_to_the_caller_of_the_facade():
    import splatfields_amd as S
    c = case(1, 5, 13)
    m = len(c["idx"])
    call = lambda ranks, **kw: S.depth_points(c["depths"], c["kinv"], c["pose"], images=c["images"], ranks=ranks, return_flag=True, **kw)
    xyz, rgb, flag = call([0, m - 1])
    assert flag.is_cuda and flag.dtype is torch.int32 and flag.shape == (1,) and int(flag) == 0
    want = run(c, ranks=[0, m - 1])
    assert torch.equal(xyz, want[0]) and torch.equal(rgb, want[1])
    xyz, rgb, idx, flag = call([0, m], return_indices=True)
    assert int(flag) == 1 and torch.isnan(xyz[1]).all() and int(idx[1]) == -1 and torch.equal(xyz[0], want[0][0])
    assert int(call(np.zeros(0, np.int64))[2]) == 0
    with pytest.raises(ValueError, match="return_flag needs ranks"):
        S.depth_points(c["depths"], c["kinv"], c["pose"], return_flag=True)


def test_n_pts_draws_a_seeded_subset_without_repeats():
    c = case(3, 130, 70)
    full = run(c)
    draws = []
    for _ in range(2):
        gen = torch.Generator(device="cuda").manual_seed(31)
        xyz, rgb, idx = run(c, n_pts=500, generator=gen)
        assert xyz.shape == (500, 3)
        draws.append((xyz, rgb, idx))
    assert all(torch.equal(a, b) for a, b in zip(*draws))
    got = draws[0][2].cpu().numpy()
    assert len(np.unique(got)) == 500 and np.all(np.isin(got, c["idx"])) and not np.all(np.diff(got) > 0)
    rows = torch.as_tensor(np.searchsorted(c["idx"], got)).cuda()
    assert torch.equal(draws[0][0], full[0][rows]) and torch.equal(draws[0][1], full[1][rows])
    everything = run(c, n_pts=10 ** 9)                                         # more than there are: everything, in pixel order
    assert all(torch.equal(a, b) for a, b in zip(everything, full))


# ---- capacity, repeatability, launch counts -----------------------------------------------------------------------------------
def test_a_short_capacity_gives_the_ordered_prefix():
    from splatfields_amd import _lib, init as I
    c = case(1, 15, 17)
    full = run(c)
    m = len(c["idx"])
    for cap in (m + 5, m, m - 1, 1, 0):
        got = run(c, capacity=cap)
        assert all(torch.equal(a, b[:cap]) for a, b in zip(got, full)), cap
    # the C ABI itself: buffers of m rows, a capacity one short: the last row must stay untouched
    dev = torch.device("cuda", torch.cuda.current_device())
    b = I._DepthBatch(c["depths"], c["kinv"], c["pose"], c["images"], None, dev)
    ws, count, _ = b.mark()
    xyz = torch.full((m, 3), 9.0, device=dev)
    rgb = torch.full((m, 3), 77, dtype=torch.uint8, device=dev)
    idx = torch.full((m,), -5, dtype=torch.int64, device=dev)
    _lib.check(_lib.load().sr_depth_points_gather(*b.head(), I.ptr(b.images), 1, I.ptr(ws), m - 1, I.ptr(xyz), I.ptr(rgb), I.ptr(idx), _lib.stream(dev)))
    assert int(count) == m
    assert torch.equal(xyz[:-1], full[0][:-1]) and torch.equal(rgb[:-1], full[1][:-1]) and torch.equal(idx[:-1], full[2][:-1])
    assert xyz[-1].tolist() == [9.0, 9.0, 9.0] and rgb[-1].tolist() == [77, 77, 77] and int(idx[-1]) == -5


def test_same_call_twice_is_bit_identical():
    c = case(3, 130, 70)
    a, b = run(c), run(c)
    assert all(x.cpu().numpy().tobytes() == y.cpu().numpy().tobytes() for x, y in zip(a, b))
    assert torch.equal(bounds_of(c), bounds_of(c))
    r = np.random.default_rng(2).integers(0, len(c["idx"]), 1000)
    a, b = run(c, ranks=r), run(c, ranks=r)
    assert all(x.cpu().numpy().tobytes() == y.cpu().numpy().tobytes() for x, y in zip(a, b))


def library_launches(fn):
    return sum(stage_counts(fn)[1])


def test_launch_budget():
    """conditions of the design: mark, scan and gather or select for a cloud; mark and scan for the bounds"""
    c = case(3, 130, 70)
    assert library_launches(lambda: run(c)) == 3
    assert library_launches(lambda: run(c, ranks=[5, 1, 5])) == 3
    assert library_launches(lambda: run(c, n_pts=100, generator=torch.Generator(device="cuda").manual_seed(1))) == 3
    assert library_launches(lambda: bounds_of(c)) == 2
    assert library_launches(lambda: run(dict(c, depths=np.zeros_like(c["depths"])))) == 2      # nothing to gather


# ---- the reference's own outputs, and the drop-ins ----------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(R.golden_cases()))
def test_gen_3dpoints_against_the_committed_fixture(name):
    """the numpy drop-in with the reference's arguments: the fixture's shapes and dtypes, its colours, every coordinate within the
    derived bound of the reference's float64 run, and within 4 x the reference's own float32-against-float64 error on that tensor"""
    import splatfields_amd as S
    c = R.golden_cases()[name]
    H, W = int(c["H"]), int(c["W"])
    for k in (0, 2):
        args = (torch.from_numpy(c["kinv"]).float(), torch.from_numpy(c["pose"]).float(), torch.from_numpy(c["depths"]), torch.from_numpy(c["images"][k]))
        pts, rgb = S.gen_3dpoints(k, H, W, *args)
        want = c[f"pts64_{k}"]
        assert isinstance(pts, np.ndarray) and isinstance(rgb, np.ndarray)
        assert pts.dtype == c[f"pts32_{k}"].dtype == np.float32 and pts.shape == want.shape
        assert rgb.dtype == np.uint8 and np.array_equal(rgb, c[f"rgb32_{k}"])
        d = np.abs(pts.astype(np.float64) - want)
        # the reference's float64 run sums inside matmul: allow its own 1e-14 relative distance to the restatement on top
        assert np.all(d <= R.coordinate_bound(want) + 1e-14 * np.abs(want).max())
        r = max(np.abs(c[f"pts32_{k}"].astype(np.float64) - want).max(), float(R.ulp32(np.abs(want).max())))
        print(f"{name} img_idx {k}: d = {d.max():.3e}, r = {r:.3e}, d / 4r = {d.max() / (4 * r):.3f}")
        assert d.max() <= 4 * r
        pts_np, rgb_np = S.gen_3dpoints(k, H, W, c["kinv"], c["pose"], c["depths"], c["images"][k])       # numpy arguments
        assert np.array_equal(pts_np, pts) and np.array_equal(rgb_np, rgb)


def test_depth_point_cloud_feeds_splats_from_points():
    import splatfields_amd as S
    c = case(3, 130, 70)
    gen = torch.Generator(device="cuda").manual_seed(4)
    xyz, colors = S.depth_point_cloud(c["depths"], c["kinv"], c["pose"], c["images"], 700, generator=gen)
    assert xyz.shape == (700, 3) and colors.shape == (700, 3) and colors.dtype is torch.float32 and xyz.is_cuda and colors.is_cuda
    assert float(colors.min()) >= 0.0 and float(colors.max()) <= 1.0 and float(colors.max()) > 0.9
    t = S.splats_from_points(xyz, colors, sh_degree=3)
    shapes = {"_xyz": (700, 3), "_features_dc": (700, 1, 3), "_features_rest": (700, 15, 3), "_scaling": (700, 3), "_rotation": (700, 4),
              "_opacity": (700, 1), "max_radii2D": (700,)}
    for k, s in shapes.items():
        assert tuple(t[k].shape) == s and t[k].dtype is torch.float32 and t[k].is_cuda, k
    assert torch.equal(t["_xyz"], xyz) and torch.isfinite(t["_scaling"]).all()
    xyz, colors = S.depth_point_cloud(c["depths"], c["kinv"], c["pose"], c["images"], 10 ** 9)           # fewer than asked for: all of them
    assert xyz.shape == (len(c["idx"]), 3) and torch.equal(colors, torch.from_numpy(c["rgb"]).cuda().float() / 255.0)
