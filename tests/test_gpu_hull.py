"""The visual-hull initialisation on the GPU (splatfields_amd.init, csrc/hull.hip) against the float64 restatement
(tests/hull_reference.py) and the reference's own survivor sets (tests/golden/hull_cases.npz).

The kernel evaluates the restatement's expressions in double, in the same order, without fused multiply-adds, so wherever no pixel
coordinate lies within rounding distance of a boundary the survivor list must be EQUAL: every index, in order, and every float32
coordinate bit for bit.  Each case therefore first asserts, on the host, that no item has a margin below 1e-9 px (seven orders of
magnitude above double rounding at these image sizes; the seeds are chosen so that it holds -- at <= 48^3 voxels and <= 5 views
about 2e-3 of the seeds would not), and then requires equality.  The cases whose numbers are dyadic on purpose (a voxel exactly
on a half-pixel boundary, h2 == 0 exactly) are exempt from the margin requirement and say so: there every operation is exact, and
the boundary itself is what is tested."""
import functools

import numpy as np
import pytest
import torch

from tests import hull_reference as R
from tests.scan_round import BLOCK, SCAN_ROUND

pytestmark = pytest.mark.gpu
MARGIN = 1e-9


# ---- inputs ----------------------------------------------------------------------------------------------------------------
def look_at(center, up=(0.13, 0.31, 0.94)):
    z = -center / np.linalg.norm(center)
    x = np.cross(np.asarray(up), z)
    x /= np.linalg.norm(x)
    return np.stack([x, np.cross(z, x), z])


def pinhole_views(n, seed, sizes, distance=3.0, focal=1.1, target_spread=0.0):
    """n generic pinhole cameras (KRT [n,3,4]) on a sphere around the origin, looking at it; sizes: (H, W) or a list of them.
    focal is in units of the image width."""
    rng = np.random.default_rng(seed)
    sizes = [sizes] * n if isinstance(sizes[0], int) else sizes
    out = []
    for k in range(n):
        c = rng.normal(size=3)
        c = distance * c / np.linalg.norm(c)
        Rw = look_at(c - target_spread * rng.normal(size=3), up=rng.normal(size=3))
        H, W = sizes[k]
        K = np.array([[focal * W, 0.0, (W - 1) / 2 + rng.uniform(-1, 1)], [0.0, focal * W * rng.uniform(0.95, 1.05), (H - 1) / 2 + rng.uniform(-1, 1)],
                      [0.0, 0.0, 1.0]])
        out.append(K @ np.concatenate([Rw, (-Rw @ c)[:, None]], axis=1))
    return np.stack(out)


def blob_masks(seed, sizes, n, fill=0.36):
    """n elliptical silhouettes, one per size (uint8, 0 / 255)"""
    rng = np.random.default_rng(seed)
    sizes = [sizes] * n if isinstance(sizes[0], int) else sizes
    out = []
    for H, W in sizes:
        yy, xx = np.mgrid[:H, :W]
        cy, cx = (H - 1) / 2 + rng.uniform(-2, 2), (W - 1) / 2 + rng.uniform(-2, 2)
        out.append((255 * (((yy - cy) / (fill * H)) ** 2 + ((xx - cx) / (fill * W)) ** 2 <= 1.0)).astype(np.uint8))
    return out


@functools.lru_cache(maxsize=None)
def grid_case(name):
    """name -> dict(masks, matrices, convention, outside, G, aabb) of the grid cases below"""
    if name in ("samples_krt", "samples_list"):
        c = R.golden_cases()[name]
        return dict(masks=c["masks"], matrices=c["matrices"], convention=c["convention"], outside=c["outside"], G=c["G"], aabb=c["aabb"],
                    golden=c["indices"])
    sizes5 = [(40, 52), (31, 47), (52, 40), (33, 33), (48, 64)]
    specs = {
        # a partial last wavefront and a partial last workgroup: 35 937 = 140 * 256 + 97 = 561 * 64 + 33
        "g33": dict(masks=blob_masks(1, (40, 52), 4), matrices=pinhole_views(4, 11, (40, 52)), G=33),
        "g48_box": dict(masks=blob_masks(2, (44, 44), 3, fill=0.42), matrices=pinhole_views(3, 12, (44, 44)), G=48,
                        aabb=((-1.0, -0.5, -0.8), (0.7, 0.9, 1.1))),
        "v1": dict(masks=blob_masks(3, (36, 50), 1), matrices=pinhole_views(1, 13, (36, 50)), G=24),
        "v5_ragged_carve": dict(masks=blob_masks(4, sizes5, 5, fill=0.4), matrices=pinhole_views(5, 14, sizes5), G=32),
        "v5_ragged_keep": dict(masks=blob_masks(4, sizes5, 5, fill=0.3), matrices=pinhole_views(5, 14, sizes5, focal=1.9), G=32, outside="keep"),
        "v64_tiny": dict(masks=blob_masks(5, (8, 8), 64, fill=0.48), matrices=pinhole_views(64, 15, (8, 8), focal=0.8), G=16),
        "ndc_square": dict(masks=blob_masks(6, (40, 40), 3), matrices=ndc_views(3, 16), G=32, convention="ndc", aabb=(-1.3, 1.3)),
        # a camera inside the box: h2 of both signs, pixel coordinates of every magnitude
        "camera_inside": dict(masks=blob_masks(7, (40, 52), 2, fill=0.45), G=24,
                              matrices=np.concatenate([pinhole_views(1, 17, (40, 52), distance=0.37, focal=0.5, target_spread=0.3),
                                                       pinhole_views(1, 18, (40, 52), distance=2.5, focal=0.6)])),
    }
    s = dict(convention="krt", outside="carve", aabb=(-1.0, 1.0))
    s.update(specs[name])
    return s


def ndc_views(n, seed):
    """full_proj_transform [n,4,4] in the reference's transposed storage (clip = [p 1] @ M), perspective cameras around the origin"""
    rng = np.random.default_rng(seed)
    out = []
    for _ in range(n):
        c = rng.normal(size=3)
        c = 4.0 * c / np.linalg.norm(c)
        Rw = look_at(c, up=rng.normal(size=3))
        w2c = np.eye(4)
        w2c[:3, :3], w2c[:3, 3] = Rw, -Rw @ c
        t, zn, zf = np.tan(0.31), 0.01, 100.0
        P = np.zeros((4, 4))
        P[0, 0], P[1, 1], P[3, 2], P[2, 2], P[2, 3] = 1 / t, 1 / t, 1.0, zf / (zf - zn), -(zf * zn) / (zf - zn)
        out.append((P @ w2c).T)
    return np.stack(out)


@functools.lru_cache(maxsize=None)
def restated(name):
    c = grid_case(name)
    idx, margin = R.hull_grid(c["masks"], c["matrices"], c["aabb"], c["G"], c["convention"], c["outside"])
    return idx, margin


GRID_CASES = ("samples_krt", "samples_list", "g33", "g48_box", "v1", "v5_ragged_carve", "v5_ragged_keep", "v64_tiny", "ndc_square",
              "camera_inside")


def run_grid(c, **kw):
    import splatfields_amd as S
    xyz, idx = S.visual_hull(c["masks"], c["matrices"], convention=c["convention"], outside=c["outside"], grid_resolution=c["G"],
                             aabb=c["aabb"], return_indices=True, **kw)
    assert xyz.is_cuda and xyz.dtype is torch.float32 and idx.dtype is torch.int32 and xyz.shape == (idx.shape[0], 3)
    return xyz, idx


def assert_rows(xyz, idx, want, c):
    """the index list element for element, in order and in count, and the float32 coordinates bit for bit"""
    got = idx.cpu().numpy()
    assert got.shape == want.shape and np.array_equal(got, want), (len(got), len(want), np.setxor1d(got, want)[:10])
    coords = torch.from_numpy(R.grid_points(c["aabb"], c["G"], want).astype(np.float32))
    assert torch.equal(xyz.cpu(), coords)


# ---- grid mode -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", GRID_CASES)
def test_grid_cases_equal_the_restatement(name):
    c = grid_case(name)
    want, margin = restated(name)
    print(f"{name}: G = {c['G']}, {len(c['masks'])} views, {len(want)} survivors, smallest margin {margin.min():.3e} px")
    assert margin.min() >= MARGIN
    assert 0 < len(want) < c["G"] ** 3
    if "golden" in c:
        assert np.array_equal(want, c["golden"])                   # the reference's own set (float64 there too)
    if name == "camera_inside":
        h2 = R.grid_points(c["aabb"], c["G"]) @ R.rows_of(c["matrices"], "krt")[0, 2, :3] + c["matrices"][0, 2, 3]
        assert (h2 < 0).sum() > 500 and (h2 > 0).sum() > 500
    assert_rows(*run_grid(c), want, c)


def test_blender_fixture_against_the_stored_reference_indices():
    """256^3 voxels, the reference's float32 Blender branch: compared with the stored survivor set, not with a run-time restatement.
    A voxel decided the other way must lie within delta32 of a rounding boundary (evaluated through the restatement in points mode),
    and at most 1e-3 of the survivors may."""
    c = R.golden_cases()["blender_hull"]
    xyz, idx = run_grid(c)
    got, want = idx.cpu().numpy(), c["indices"]
    assert np.all(np.diff(got) > 0)
    differ = np.setxor1d(got, want)
    print(f"blender_hull: {len(want)} survivors stored, {len(got)} on the GPU, {len(differ)} differ")
    assert len(differ) <= 1e-3 * len(want)
    if len(differ):
        _, margin = R.hull_points(R.grid_points(c["aabb"], c["G"], differ), c["masks"], c["matrices"], "ndc", "carve")
        print(f"largest margin of a differing voxel {margin.max():.3e} px")
        assert np.all(margin < R.delta32(c["masks"][0].shape[0]))
    assert torch.equal(xyz.cpu(), torch.from_numpy(R.grid_points(c["aabb"], c["G"], got).astype(np.float32)))


def test_a_single_voxel():
    """G = 1: linspace gives the lower corner"""
    krt = pinhole_views(2, 21, (20, 24), distance=6.0, focal=0.7)
    ones = [np.ones((20, 24), np.uint8)] * 2
    c = dict(masks=ones, matrices=krt, convention="krt", outside="carve", G=1, aabb=(-1.0, 1.0))
    alive, margin = R.hull_points(R.grid_points(c["aabb"], 1), ones, krt)
    assert alive.tolist() == [True] and margin.min() >= MARGIN
    xyz, idx = run_grid(c)
    assert idx.tolist() == [0] and xyz.tolist() == [[-1.0, -1.0, -1.0]]
    xyz, idx = run_grid(dict(c, masks=[np.ones((20, 24), np.uint8), np.zeros((20, 24), np.uint8)]))
    assert idx.shape == (0,) and xyz.shape == (0, 3)


def test_all_ones_masks_full_count_and_a_capacity_one_short():
    """every voxel inside every image: count = G^3; with capacity G^3 everything is written, one short of it an ordered prefix
    is, and the count stays the true one"""
    from splatfields_amd import init as I
    G, sizes = 20, [(30, 36), (36, 30), (33, 33)]
    krt = pinhole_views(3, 22, sizes, distance=6.0, focal=0.7)
    masks = [np.full(s, 7, np.uint8) for s in sizes]
    c = dict(masks=masks, matrices=krt, convention="krt", outside="carve", G=G, aabb=(-1.0, 1.0))
    want, margin = R.hull_grid(masks, krt, c["aabb"], G)
    assert len(want) == G ** 3 and margin.min() >= MARGIN
    assert_rows(*run_grid(c), want, c)
    assert_rows(*run_grid(c, capacity=G ** 3), want, c)
    assert_rows(*run_grid(c, capacity=G ** 3 - 1), want[:-1], c)
    # the C ABI itself: buffers one row short plus a guard row that must stay untouched
    dev = torch.device("cuda")
    table, flat = I._view_table(masks, krt, "krt", "carve", dev)
    grid = torch.from_numpy(R.axis_tables(c["aabb"], G)).to(dev)
    ws, count = I._carve(table, flat, grid, G, None, G ** 3, dev)
    lib = I._lib.load()
    idx = torch.full((G ** 3,), -5, dtype=torch.int32, device=dev)
    xyz = torch.full((G ** 3, 3), 9.0, device=dev)
    I._lib.check(lib.sr_hull_gather(I.ptr(grid), G, None, 0, 0, I.ptr(ws), G ** 3 - 1, I.ptr(idx), I.ptr(xyz), I._lib.stream(dev)))
    assert int(count.item()) == G ** 3
    assert np.array_equal(idx.cpu().numpy()[:-1], want[:-1]) and int(idx[-1]) == -5 and xyz[-1].tolist() == [9.0, 9.0, 9.0]


def test_all_zero_masks_give_nothing():
    c = dict(grid_case("g33"), masks=[np.zeros((40, 52), np.float32)] * 4)
    xyz, idx = run_grid(c)
    assert idx.shape == (0,) and xyz.shape == (0, 3)


def test_mask_dtypes_and_layouts_are_equivalent():
    """[V,H,W] / [V,H,W,1], arrays / device tensors, any dtype: `> 0` is what counts"""
    c = grid_case("g33")
    want, _ = restated("g33")
    stack = np.stack(c["masks"])
    for masks in (stack.astype(np.float64) / 255.0, torch.from_numpy(stack)[..., None].cuda(), torch.from_numpy(stack > 0),
                  [torch.from_numpy(m).float() for m in c["masks"]]):
        assert_rows(*run_grid(dict(c, masks=masks)), want, c)


def test_half_pixel_boundaries_round_to_even_both_ways():
    """Dyadic numbers, an axis-aligned affine camera (h2 = 1): px = 4 x + 4.5 lands EXACTLY on k + 1/2 for the nine coordinates of a
    G = 9 grid over [-1, 1] (exempt from the margin requirement: every operation is exact, the boundary is the subject).  Halves to
    even: 0.5 -> 0, 1.5 -> 2, 2.5 -> 2, 3.5 -> 4, ...; the mask keeps the pixels whose x and y are multiples of 4, which separates
    half-to-even (k in {0, 3, 4, 7, 8}) from half-up ({3, 7}) and half-down ({0, 4, 8})."""
    G, aabb, keep = 9, (-1.0, 1.0), [0, 3, 4, 7, 8]
    want = np.array(sorted((iy * G + ix) * G + iz for iy in keep for ix in keep for iz in range(G)), np.int32)
    for convention, S, M in (("krt", 17, np.array([[[4.0, 0, 0, 4.5], [0, 4.0, 0, 4.5], [0, 0, 0, 1.0]]])),
                             ("ndc", 16, np.array([[[0.5, 0, 0, 0], [0, 0.5, 0, 0], [0, 0, 0, 0], [-0.375, -0.375, 1.0, 1.0]]]))):
        mask = np.zeros((1, S, S), np.uint8)
        mask[0, ::4, ::4] = 1
        got, margin = R.hull_grid(mask, M, aabb, G, convention)
        assert margin.max() == 0.0 and np.array_equal(got, want), convention
        c = dict(masks=mask, matrices=M, convention=convention, outside="carve", G=G, aabb=aabb)
        assert_rows(*run_grid(c), want, c)


def test_same_call_twice_is_bit_identical():
    c = grid_case("v5_ragged_carve")
    a, b = run_grid(c), run_grid(c)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])


def test_n_pts_draws_a_seeded_subset_without_repeats():
    c = grid_case("g33")
    want, _ = restated("g33")
    rows = []
    for _ in range(2):
        gen = torch.Generator(device="cuda").manual_seed(31)
        xyz, idx = run_grid(c, n_pts=500, generator=gen)
        assert xyz.shape == (500, 3)
        rows.append((xyz, idx))
    assert torch.equal(rows[0][0], rows[1][0]) and torch.equal(rows[0][1], rows[1][1])
    got = rows[0][1].cpu().numpy()
    assert len(np.unique(got)) == 500 and np.all(np.isin(got, want)) and not np.all(np.diff(got) > 0)
    assert torch.equal(rows[0][0].cpu(), torch.from_numpy(R.grid_points(c["aabb"], c["G"], got).astype(np.float32)))
    xyz, idx = run_grid(c, n_pts=10 ** 9)                               # more than there are: everything, in grid order
    assert np.array_equal(idx.cpu().numpy(), want)


def test_numpy_drop_ins_return_the_reference_rows():
    import splatfields_amd as S
    for name, fn in (("samples_krt", S.visual_hull_samples), ("samples_list", S.visual_hull_samples_list)):
        c = R.golden_cases()[name]
        masks = np.stack(c["masks"]).astype(np.float64) if name == "samples_krt" else [m.astype(np.float64) for m in c["masks"]]
        out = fn(masks, c["matrices"], 10 ** 9, c["G"], c["aabb"])
        assert isinstance(out, np.ndarray) and out.dtype == np.float64 and out.shape == (len(c["indices"]), 3)
        want = R.grid_points(c["aabb"], c["G"], c["indices"])
        order = np.lexsort(out.T[::-1])
        assert np.array_equal(out[order], want[np.lexsort(want.T[::-1])])       # the same rows (float64 grid positions), shuffled
        assert fn(masks, c["matrices"], 100, c["G"], c["aabb"]).shape == (100, 3)


# ---- points mode -----------------------------------------------------------------------------------------------------------
# SCAN_ROUND and SCAN_ROUND + 1 workgroups of points: k_hull_scan walks one count per workgroup (a full round of ordered_scan, and
# the first count of a second one); these two run the one-view case only
@pytest.mark.parametrize("n", [1, 65, 1000, SCAN_ROUND * BLOCK, SCAN_ROUND * BLOCK + 1])
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_hull_filter_equals_the_restatement(n, dtype):
    import splatfields_amd as S
    from splatfields_amd import init as I
    rng = np.random.default_rng(100 + n)
    pts = rng.uniform(-0.8, 0.8, (n, 3)).astype(dtype)
    if n == 1:
        pts[0] = [0.05, -0.1, 0.08]
    for name in ("g33", "v5_ragged_keep", "ndc_square") if n <= 1000 else ("v1",):
        c = grid_case(name)
        alive, margin = R.hull_points(pts.astype(np.float64), c["masks"], c["matrices"], c["convention"], c["outside"])
        assert margin.min() >= MARGIN
        keep = S.hull_filter(torch.from_numpy(pts), c["masks"], c["matrices"], convention=c["convention"], outside=c["outside"], device="cuda")
        assert keep.is_cuda and keep.dtype is torch.bool and keep.shape == (n,)
        assert np.array_equal(keep.cpu().numpy(), alive), name
        if n >= 1000:
            assert 0 < alive.sum() < n, name
        # the survivor list itself: the count, and every index in order
        dev = torch.device("cuda", torch.cuda.current_device())
        table, flat = I._view_table(c["masks"], c["matrices"], c["convention"], c["outside"], dev)
        on_dev = torch.from_numpy(pts).to(dev)
        ws, count = I._carve(table, flat, None, 0, on_dev, n, dev)
        assert int(count.item()) == int(alive.sum()), name
        idx, _ = I._gather(None, 0, on_dev, n, ws, int(count.item()), dev, want_points=False)
        assert np.array_equal(idx.cpu().numpy(), np.nonzero(alive)[0]), name


def test_blender_load_fixture():
    """the reference's `load` branch (float32 there): the stored rows, with the same allowance as the 256^3 case"""
    import splatfields_amd as S
    c = R.golden_cases()["blender_load"]
    keep = S.hull_filter(c["points"], c["masks"], c["matrices"], convention="ndc", outside="carve", device="cuda").cpu().numpy()
    differ = np.setxor1d(np.nonzero(keep)[0], c["indices"])
    print(f"blender_load: {len(c['indices'])} rows stored, {int(keep.sum())} on the GPU, {len(differ)} differ")
    assert len(differ) <= 1e-3 * len(c["indices"])
    assert S.hull_filter(np.zeros((0, 3)), c["masks"], c["matrices"], convention="ndc", device="cuda").shape == (0,)


def test_h2_zero_and_non_finite_coordinates_are_carved():
    """A camera in the plane z = 0.25 with dyadic entries (exact arithmetic, exempt from the margin requirement): points with
    h2 == 0 exactly give u = +-inf or 0 / 0 and are carved under both policies, a point behind the camera that projects into the
    mask survives (there is no test on the sign of h2), a point outside the image survives only under `keep`."""
    import splatfields_amd as S
    M = np.array([[[4.0, 0.0, 3.5, -0.875], [0.0, 4.0, 3.5, -0.875], [0.0, 0.0, 1.0, -0.25]]])      # u = 4 x / (z - 0.25) + 3.5
    mask = np.ones((1, 8, 8), np.uint8)
    pts = np.array([[0.5, 0.25, 0.25],      # h2 = 0, h0 = 2: +inf
                    [-0.5, 0.0, 0.25],      # h2 = 0, h0 = -2, h1 = 0: -inf and 0 / 0
                    [0.0, 0.0, 0.25],       # 0 / 0 on both axes
                    [0.25, 0.25, 1.25],     # in front: (4.5, 4.5) -> inside
                    [-0.25, -0.25, -0.75],  # behind: h2 = -1, u = 4.5 -> inside: survives
                    [3.0, 0.0, 1.25],       # (15.5, 3.5): outside the image
                    [0.25, 0.25, 0.25 + 2.0 ** -40]])   # h2 tiny: u ~ 1e12, finite, outside
    for outside, want in (("carve", [0, 0, 0, 1, 1, 0, 0]), ("keep", [0, 0, 0, 1, 1, 1, 1])):
        for dtype in (np.float32, np.float64):
            expect = [bool(w) for w in want]
            if dtype is np.float32:
                expect[6] = False                      # 0.25 + 2^-40 is 0.25 in float32: the point lies in the plane h2 = 0
            alive, _ = R.hull_points(pts.astype(dtype).astype(np.float64), mask, M, "krt", outside)
            assert alive.tolist() == expect, (outside, dtype)
            keep = S.hull_filter(pts.astype(dtype), mask, M, convention="krt", outside=outside, device="cuda")
            assert keep.cpu().tolist() == expect, (outside, dtype)
    # the same plane inside a grid: G = 17 over [-1, 1] has the coordinate 0.25 exactly (k = 10)
    c = dict(masks=mask, matrices=M, convention="krt", outside="keep", G=17, aabb=(-1.0, 1.0))
    want, _ = R.hull_grid(mask, M, c["aabb"], 17, "krt", "keep")
    assert not np.any(want % 17 == 10) and 0 < len(want) < 17 ** 3            # the whole plane iz = 10 is carved
    assert_rows(*run_grid(c), want, c)


# ---- the tensors behind create_from_pcd ------------------------------------------------------------------------------------
def test_splats_from_points():
    import splatfields_amd as S
    from simple_knn._C import distCUDA2
    gen = torch.Generator(device="cuda").manual_seed(5)
    pts = torch.rand(500, 3, device="cuda", generator=gen) * 2 - 1
    colors = torch.rand(500, 3, device="cuda", generator=gen)
    t = S.splats_from_points(pts, colors, sh_degree=3)
    assert sorted(t) == ["_features_dc", "_features_rest", "_opacity", "_rotation", "_scaling", "_xyz", "max_radii2D"]
    shapes = {"_xyz": (500, 3), "_features_dc": (500, 1, 3), "_features_rest": (500, 15, 3), "_scaling": (500, 3), "_rotation": (500, 4),
              "_opacity": (500, 1), "max_radii2D": (500,)}
    for k, s in shapes.items():
        assert tuple(t[k].shape) == s and t[k].dtype is torch.float32 and t[k].is_cuda and t[k].is_contiguous(), k
    assert torch.equal(t["_xyz"], pts)
    assert torch.allclose(t["_features_dc"][:, 0], (colors - 0.5) / 0.28209479177387814, atol=1e-6, rtol=0)
    assert not t["_features_rest"].any() and not t["max_radii2D"].any()
    assert torch.equal(t["_rotation"], torch.tensor([1.0, 0.0, 0.0, 0.0], device="cuda").expand(500, 4))
    assert torch.allclose(t["_opacity"], torch.full((500, 1), float(np.log(0.1 / 0.9)), device="cuda"), atol=1e-6, rtol=0)
    scales = torch.log(torch.sqrt(torch.clamp_min(distCUDA2(pts), 0.0000001)))[..., None]
    assert torch.allclose(t["_scaling"], scales.repeat(1, 3), atol=1e-6, rtol=0)
    iso = S.splats_from_points(pts.cpu().numpy(), None, sh_degree=1, isotropic=True, generator=torch.Generator(device="cuda").manual_seed(9))
    assert tuple(iso["_scaling"].shape) == (500, 1) and torch.allclose(iso["_scaling"], scales, atol=1e-6, rtol=0)
    assert tuple(iso["_features_rest"].shape) == (500, 3, 3)
    rgb = iso["_features_dc"][:, 0] * 0.28209479177387814 + 0.5                       # the reference's random / 255
    assert float(rgb.min()) >= -1e-6 and float(rgb.max()) <= 1.0 / 255.0 + 1e-6 and float(rgb.std()) > 1e-4
