"""The scenes of tests/boundary_scenes.py are what they claim -- by the oracles alone, no kernel involved:
  * every blend scene is flip-free (the float64 oracle's `fragile` map is all false) and its n_contrib takes exactly the designed
    values: the list length (B1, B4, B5), {p, p + 1} with both inside one quad (B2), p on every pixel (the all-dead scenes),
    early stops on the killed quads / sub-tiles only (B3);
  * every sort scene has one instance per splat, in its own tile, equal float depth keys inside a level, and the expected
    (level, splat index) order is the oracle's (float depth, splat index) order;
  * the (quad, entry) pair count of every B4 chunk, by the float64 alpha test per quad, is on the intended side of the slot
    caps of csrc/blend_bwd.hip (752, and 624 with a depth gradient)."""
import pytest
import torch

from oracle import c_oracle
from oracle import torch_oracle as O
from tests import boundary_scenes as B

BWD_CAP, BWD_CAP_DEPTH = 752, 624   # SR_BWD_CAP / SR_BWD_CAP_DEPTH of csrc/blend_bwd.hip


def oracle64(sc):
    d = {k: v.double() for k, v in sc.sp.items()}
    with torch.no_grad():
        return O.rasterize(d["means3D"], None, d["opacities"], shs=d["shs"] if sc.use_sh else None,
                           colors_precomp=None if sc.use_sh else d["colors_precomp"], scales=d["scales"], rotations=d["rotations"],
                           settings=sc.st)


def quad_ids(H, W):
    return (torch.arange(H)[:, None] // 4) * ((W + 3) // 4) + torch.arange(W)[None, :] // 4


@pytest.mark.parametrize("name", B.BLEND_NAMES)
def test_blend_scene_is_flip_free_and_on_its_boundary(name):
    sc = B.blend_scene(name)
    ref = oracle64(sc)
    H, W = sc.st.image_height, sc.st.image_width
    tiles = ((W + 15) // 16) * ((H + 15) // 16)
    assert not ref.fragile.any(), int(ref.fragile.sum())
    assert ref.num_rendered == sc.length * tiles            # every tile holds the whole list
    assert int((sc.pos > 0).sum()) == sc.length and int(ref.pre.visible.sum()) == sc.length
    nc = ref.n_contrib.long()
    assert int(nc.min()) == sc.nc_min and int(nc.max()) == sc.nc_max, (int(nc.min()), int(nc.max()))
    if sc.dead is not None:   # B3: the killed region stops inside the killers, per quad; everything else reaches the end
        assert (nc[~sc.dead] == sc.length).all() and (nc[sc.dead] <= sc.nc_dead).all() and (nc[sc.dead] >= 1).all()
        q = quad_ids(H, W)
        for k in q.unique():
            whole = sc.dead[q == k]
            assert whole.all() or not whole.any()            # killed regions are whole quads
    if sc.nc_max == sc.nc_min + 1:   # B2: the stop holds at p on some pixels and at p + 1 on others INSIDE one quad
        q = quad_ids(H, W)
        assert any(set(nc[q == k].tolist()) == {sc.nc_min, sc.nc_max} for k in q.unique())
        assert int((nc == sc.nc_max).sum()) >= 4
    if sc.behind.numel():
        assert int(sc.pos[sc.behind].min()) == sc.nc_max + 1 and sc.behind.numel() >= 300
    assert (sc.pos[sc.last] <= sc.nc_max).all() and (sc.pos[sc.last] >= sc.nc_min).all()


def test_the_families_cover_the_designed_boundaries():
    scenes = B.blend_scenes()
    one_tile = lambda s: s.st.image_width == 16 and s.st.image_height == 16
    assert sorted(s.length for s in scenes if s.family == "B1" and one_tile(s)) == B.B1_LENGTHS
    stops = sorted(s.nc_min for s in scenes if s.family == "B2" and one_tile(s))
    assert stops == B.B2_STOPS and {16, 17, 128, 129, 255, 256, 257, 511, 512, 513} <= set(stops) | {s + 1 for s in stops}
    assert any(s.st.image_width == 32 and s.st.image_height == 32 for s in scenes)
    assert sum(1 for s in scenes if s.st.image_width % 16 and s.st.image_height % 16) >= 2
    assert any(s.use_sh for s in scenes) and any(not s.use_sh for s in scenes)
    b3 = {s.name: s for s in scenes if s.family == "B3"}
    assert b3["B3_wave0_dead"].nc_dead < 256 and b3["B3_wave0_dead"].dead[:8, :8].all() and int(b3["B3_wave0_dead"].dead.sum()) == 64
    assert int(b3["B3_three_waves_dead"].dead.sum()) == 192 and not b3["B3_three_waves_dead"].dead[:8, :8].any()
    assert int(b3["B3_one_quad_dead"].dead.sum()) == 16
    for s in b3.values():   # the rest of the tile goes on through >= 3 more batches / chunks
        assert s.length - (s.nc_dead if s.dead is not None else s.nc_max) >= 3 * 256
    assert (b3["B3_all_dead_at_256"].nc_min, b3["B3_all_dead_at_256"].nc_max) == (256, 256)
    assert (b3["B3_all_dead_at_257"].nc_min, b3["B3_all_dead_at_257"].nc_max) == (257, 257)
    a, b = B.stale_pair()
    assert a.sp["means3D"].shape == b.sp["means3D"].shape and (a.length, b.nc_max) == (760, 256)
    assert int((b.pos == 0).sum()) == B.N_STALE - b.length > 0                     # culled filler


@pytest.mark.parametrize("name", [n for n in B.BLEND_NAMES if n.startswith("B4")])
def test_b4_pair_count_is_on_the_intended_side_of_the_slot_caps(name):
    sc = B.blend_scene(name)
    d = {k: v.double() for k, v in sc.sp.items()}
    pre = O.preprocess(d["means3D"], None, d["opacities"], None, d["colors_precomp"], d["scales"], d["rotations"], None, sc.st)
    ys, xs = torch.meshgrid(torch.arange(16, dtype=torch.float64), torch.arange(16, dtype=torch.float64), indexing="ij")
    dx = pre.pix[:, 0][:, None] - xs.reshape(1, -1)
    dy = pre.pix[:, 1][:, None] - ys.reshape(1, -1)
    power = -0.5 * (pre.conic[:, 0:1] * dx * dx + pre.conic[:, 2:3] * dy * dy) - pre.conic[:, 1:2] * dx * dy
    ok = (d["opacities"] * torch.exp(power) >= 1.0 / 255.0) & (power <= 0)            # [N, 256]
    q = quad_ids(16, 16).reshape(-1)
    reach = torch.stack([ok[:, q == k].any(dim=1) for k in range(16)], dim=1)       # [N, 16]
    pairs = int(reach.sum())
    per_entry = reach.sum(dim=1)
    assert pairs == sc.pairs and sc.length <= 256                                   # one chunk
    assert (per_entry[sc.groups["faint"]] == 16).all()
    if "single" in sc.groups:
        assert (per_entry[sc.groups["single"]] == 1).all()
        # ... and the support (alpha >= 1/255) of a single-quad entry stays inside its quad: the geometric reach test of the
        # kernels (quadmask.h) cannot count a second quad -- distance to the quad's border >= 1.4 px, support radius < 0.8 px
        s = sc.groups["single"]
        r2 = 2.0 * 0.3001 * torch.log(d["opacities"][s, 0] * 255.0)
        assert (r2.sqrt() < 0.8).all()
        fx, fy = pre.pix[s, 0] % 4.0, pre.pix[s, 1] % 4.0
        assert ((fx > 0.9) & (fx < 2.2) & (fy > 0.9) & (fy < 2.2)).all()
    a, s8 = sc.length - len(sc.groups.get("single", [])), len(sc.groups.get("single", []))
    want = {"B4_a37_s8": (1, 1), "B4_a38_s8": (1, 1), "B4_a39_s8": (1, 0), "B4_a40_s8": (1, 0), "B4_a41_s8": (1, 0),
            "B4_a45_s8": (1, 0), "B4_a46_s8": (1, 0), "B4_a47_s8": (0, 0), "B4_a48_s8": (0, 0), "B4_a49_s8": (0, 0),
            "B4_a39_s0": (1, 1), "B4_a39_s1": (1, 0), "B4_a47_s0": (1, 0), "B4_a47_s1": (0, 0), "B4_a256_s0": (0, 0)}[name]
    assert (pairs <= BWD_CAP, pairs <= BWD_CAP_DEPTH) == tuple(bool(w) for w in want), (a, s8, pairs)
    if name in ("B4_a47_s0", "B4_a47_s1"):
        assert pairs - BWD_CAP == int(name[-1])
    if name in ("B4_a39_s0", "B4_a39_s1"):
        assert pairs - BWD_CAP_DEPTH == int(name[-1])


SORT_LENGTHS = [0, 1, 2, 3, 255, 256, 257, 511, 512, 513, 1023, 1024, 1025, 1280, 1281, 1536, 1537, 2047, 2048, 2049, 3072, 3073,
                4095, 4096, 4097, 8191, 8192, 8193, 16384, 16385, 24577]


def test_sort_scenes_cover_every_boundary():
    scenes = B.sort_scenes()
    assert set(SORT_LENGTHS) <= {L for s in scenes for L in s.lengths}
    assert {2049, 4097, 8193} <= {max(s.lengths) for s in scenes}
    mixed = next(s for s in scenes if 24577 in s.lengths)
    assert {0, 2048, 2049, 4096, 4097, 8192, 8193} <= set(mixed.lengths)
    for s in scenes:
        assert sum(s.lengths) <= 60000 and len(s.lengths) <= 36
        assert any(k == 1 and L > 256 for k, L in zip(s.levels, s.lengths))            # a pure index sort
        assert any(k == L and L > 256 for k, L in zip(s.levels, s.lengths))            # distinct depths, reversed
        assert all(k <= 36 or k == L for k, L in zip(s.levels, s.lengths))


@pytest.mark.parametrize("name", B.SORT_NAMES)
def test_sort_scene_lists_are_the_oracles(name):
    sc = B.sort_scene_by_name(name)
    n, T = sc.sp["means3D"].shape[0], len(sc.lengths)
    assert n == sum(sc.lengths)
    _, _, nr = c_oracle.rasterize(sc.sp, sc.st, use_sh=True, threads=8)
    assert nr == n
    for dt in (torch.float64, torch.float32):
        d = {k: v.to(dt) for k, v in sc.sp.items()}
        pre = O.preprocess(d["means3D"], None, d["opacities"], d["shs"], None, d["scales"], d["rotations"], None, sc.st)
        assert pre.visible.all() and (pre.radii == 4).all() and (pre.radius_raw > 3.2).all() and (pre.radius_raw < 3.8).all()
        tile = torch.zeros(n, dtype=torch.int64)
        for t, e in enumerate(sc.expected):
            tile[e] = t
        want = torch.stack([tile, torch.zeros_like(tile), tile + 1, torch.ones_like(tile)], dim=1)
        assert torch.equal(pre.rect, want)                    # each splat's tile rectangle is its own tile
        # alpha >= 1/255 on the tile's centre pixels with a wide margin: exact-support culling drops nothing
        assert ((pre.pix[:, 0] - (16 * tile + 7.5)).abs() < 1e-3).all() and ((pre.pix[:, 1] - 7.5).abs() < 1e-3).all()
        a_centre = d["opacities"][:, 0] * torch.exp(-0.5 * (pre.conic[:, 0] + pre.conic[:, 2]) * 0.25 - pre.conic[:, 1].abs() * 0.25)
        assert (a_centre > 5.0 / 255.0).all()
    depth32 = pre.depth                                       # float32 preprocessing: the kernels' key is (float depth, index)
    ties = 0
    for t, e in enumerate(sc.expected):
        assert e.numel() == sc.lengths[t]
        if e.numel() < 2:
            continue
        dz = depth32[e]
        assert (dz[1:] >= dz[:-1]).all()
        same = dz[1:] == dz[:-1]
        assert (e[1:][same] > e[:-1][same]).all()
        ties += int(same.sum())
        assert int(dz.unique().numel()) == sc.levels[t]       # bit-identical means3D -> bit-identical keys
        assert int(sc.sp["means3D"][e].unique(dim=0).shape[0]) == sc.levels[t]
        rel = (dz[1:] - dz[:-1])[~same] / dz[:-1][~same]
        if sc.levels[t] <= 36 and rel.numel():
            assert rel.min() >= 1e-3                          # levels >= 1e-3 apart
        # the splat indices are a global shuffle: a list of several levels is not the tile's splats in index order
        if e.numel() > 16 and sc.levels[t] > 1:
            assert not (e[1:] > e[:-1]).all()
    assert ties > 0.8 * (n - sum(sc.levels))
