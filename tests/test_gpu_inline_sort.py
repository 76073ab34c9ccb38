"""The per-tile sort inside the forward blend's launch (csrc/render.hip: a workgroup sorts the list of its tile with the bodies
of csrc/sort_tile.h before it blends it -- lists of up to 2048 entries always, lists of 2049..4096 entries on views with at
most kInlineLongTiles = 8 tiles that long) against two independent statements of the same lists:

  host        every tile's list, read back whole through sr_debug_layout, equals a host sort of its own entries by the key
              (float bits of the view depth, splat index) -- the depths of a tile come in levels 2e-3 apart (relative), the splats
              of a level have bit-identical positions, so most neighbours in a list are depth ties and the order is exact;
  standalone  the same scene under the standalone-sort switch (set_sort_kernel("standalone"): k_sort_tiles_regs in a launch of
              its own, csrc/binning.hip): lists, images and every gradient tensor bit for bit.

Which path ran is asserted from the launch counters of the sort classes (sr_debug_sort_counters), never from timing.
Scenes: 64x64 pixels, 16 tiles, one list length per tile: every length at which the sort takes another path (1, 256/257,
512/513, 1024/1025, 2048/2049, 3072/3073, 4096/4097), a view with exactly the constant of long tiles and one with one more,
a forward launched on a wrong expectation, an empty tile, and a tile whose pixels all stop inside the first batch of a
2000-entry list."""
import ctypes as C

import numpy as np
import pytest
import torch

from oracle import torch_oracle as O
from splatfields_amd.synthetic import make_upstream_grads
from tests import boundary_scenes as B

pytestmark = pytest.mark.gpu

GX = GY = 4
Z0 = 3.0

# one tile each; 4097 takes the class of its own (4097..8192); the lengths around 2048 / 4096 are the launch boundaries
BOUNDARY_LENGTHS = [1, 256, 257, 512, 513, 1024, 1025, 2048, 2049, 3072, 3073, 4096, 4097, 0, 2047, 300]
# tile 5 = (1, 1), 2000 entries: 1880 behind 120 wide, nearly opaque splats that stop every pixel of the tile inside the first batch
# of 256 (they also reach the eight tiles around it); column 3 and row 3 are out of their reach: tile 15 stays empty
TINY_TILE, TINY_TAIL, TINY_BLOCKERS = 5, 1880, 120
TINY_LENGTHS = [40, 700, 3, 90, 1100, TINY_TAIL, 260, 1500, 5, 513, 64, 2048, 1024, 257, 33, 0]
# kInlineLongTiles (csrc/sort_tile.h) = 8 tiles of 2049..4096 entries, and one more.  The other tiles have at most 1024 entries:
# with a longest list of 4096 the coarse length classes of the launch order (k_scan_small: 255 - floor(255 len / longest)) put
# 2049 into class 128 and 1024 into class 192, so the kernel's count of "tiles that can hold a long list" is exact here
K_LONG = 8
FEW_LONG_LENGTHS = [2049, 2100, 2500, 3072, 3073, 3500, 4000, 4096, 1024, 513, 256, 1, 0, 700, 1000, 300]
MANY_LONG_LENGTHS = FEW_LONG_LENGTHS[:8] + [2300] + FEW_LONG_LENGTHS[9:]
# two long tiles, for the forward launched on the expectation of none
TWO_LONG_LENGTHS = [2300, 40, 2049, 3, 1024, 513, 256, 1, 0, 700, 1000, 300, 90, 64, 257, 33]
SCENES = {"boundaries": (BOUNDARY_LENGTHS, 31), "few_long": (FEW_LONG_LENGTHS, 33), "many_long": (MANY_LONG_LENGTHS, 34),
          "two_long": (TWO_LONG_LENGTHS, 35)}


def grid_scene(lengths, seed, blockers=0, blocker_tile=None):
    """Splats of tile t sit on the tile's centre pixel (sigma 1.1 px: radius 4 < 8, they reach no other tile) at one of up
    to 24 depth levels; splat indices are a random permutation, so index order and arrival order interleave.  `blockers`
    splats of sigma 6 px and opacity 0.95 sit in front of blocker_tile's list."""
    st = B.settings(16 * GX, 16 * GY)
    rng = np.random.default_rng(seed)
    tile = np.concatenate([np.full(L, t, dtype=np.int64) for t, L in enumerate(lengths)])
    level = np.concatenate([rng.integers(0, max(1, min(24, L // 8)), size=L) for L in lengths])
    z = Z0 * (1.0 + 2e-3 * level)
    sigma = np.full(tile.size, 1.1)
    opac = rng.uniform(0.04, 0.08, size=tile.size)
    if blockers:
        tile = np.concatenate([tile, np.full(blockers, blocker_tile, dtype=np.int64)])
        z = np.concatenate([z, np.full(blockers, Z0 * 0.95)])
        sigma = np.concatenate([sigma, np.full(blockers, 6.0)])
        opac = np.concatenate([opac, np.full(blockers, 0.95)])
    n = tile.size
    index_of = rng.permutation(n)   # record r is splat index_of[r]
    means_rec = B.unproject(st, 16.0 * (tile % GX) + 7.5, 16.0 * (tile // GX) + 7.5, z)
    s_rec = np.sqrt(sigma * sigma - O.COV2D_DILATION) * z / B.focal(st)
    idx = torch.from_numpy(index_of)
    means = torch.zeros(n, 3, dtype=torch.float64)
    scal, op = torch.zeros(n, dtype=torch.float64), torch.zeros(n, dtype=torch.float64)
    means[idx], scal[idx], op[idx] = means_rec, torch.from_numpy(s_rec), torch.from_numpy(opac)
    shs = torch.from_numpy(rng.uniform(-1.0, 1.5, size=(n, 16, 3))).float()
    shs[:, 1:, :] = torch.from_numpy(rng.normal(size=(n, 15, 3))).float() * 0.1
    rots = torch.zeros(n, 4)
    rots[:, 0] = 1.0
    sp = dict(means3D=means.float(), scales=scal.float()[:, None].expand(n, 3).contiguous(), rotations=rots,
              opacities=op.float()[:, None].contiguous(), shs=shs)
    return sp, st, idx, torch.from_numpy(tile)


def sort_counters(reset=False):
    from splatfields_amd import _lib
    out = (C.c_longlong * 4)()
    assert _lib.load().sr_debug_sort_counters(out, 1 if reset else 0) == 0
    return list(out)


_settings = {}


def raster_settings(st, dev):
    """One settings object (persistent camera tensors, as a training loop has them) per scene: the facade knows a camera again."""
    from diff_gaussian_rasterization import GaussianRasterizationSettings
    if id(st) not in _settings:
        _settings[id(st)] = (st, GaussianRasterizationSettings(
            image_height=st.image_height, image_width=st.image_width, tanfovx=st.tanfovx, tanfovy=st.tanfovy, bg=st.bg.to(dev),
            scale_modifier=st.scale_modifier, viewmatrix=st.viewmatrix.to(dev), projmatrix=st.projmatrix.to(dev),
            sh_degree=st.sh_degree, campos=st.campos.to(dev), prefiltered=False, debug=False))
    return _settings[id(st)][1]


def render(sp, st, dev):
    """Forward + backward through the facade; the tile lists are read back between the two.  Everything on the CPU."""
    from splatfields_amd import _lib, rasterizer as rz
    lib = _lib.load()
    leaf = {k: v.detach().to(dev).clone().requires_grad_(True) for k, v in sp.items()}
    means2D = torch.zeros_like(leaf["means3D"], requires_grad=True)
    rs = raster_settings(st, dev)
    sort_counters(reset=True)
    color, radii, depth, alpha = rz.rasterize_gaussians(leaf["means3D"], means2D, leaf["shs"], None, leaf["opacities"],
                                                        leaf["scales"], leaf["rotations"], None, rs)
    torch.cuda.synchronize()
    launched = sort_counters()
    fn = color.grad_fn
    geom, binning = fn.saved_tensors[8], fn.saved_tensors[9]
    n, H, W = leaf["means3D"].shape[0], st.image_height, st.image_width
    off = (C.c_size_t * 4)()
    assert lib.sr_debug_layout(n, H, W, int(fn.capacity), off) == 0
    i32 = lambda buf, o, cnt: buf[o:o + 4 * cnt].view(torch.int32).cpu().to(torch.int64)
    tile_start = i32(geom, off[0], GX * GY + 1)
    sorted_id = i32(binning, off[1], int(tile_start[-1]))
    gi, gd, ga = [g.to(dev) for g in make_upstream_grads(H, W)]
    ((color * gi).sum() + (depth * gd).sum() + (alpha * ga).sum()).backward()
    torch.cuda.synchronize()
    grads = {k: leaf[k].grad.detach().cpu() for k in leaf}
    grads["means2D"] = means2D.grad.detach().cpu()
    out = dict(color=color.detach().cpu(), depth=depth.detach().cpu(), alpha=alpha.detach().cpu(), radii=radii.cpu())
    return dict(tile_start=tile_start, sorted_id=sorted_id, out=out, grads=grads, launched=launched)


_runs = {}


def both_switches(name, dev):
    """(scene, render with the sort inside the forward blend, render under the standalone switch): once per scene."""
    if name not in _runs:
        from splatfields_amd.rasterizer import set_sort_kernel
        scene = grid_scene(*SCENES[name]) if name in SCENES else grid_scene(TINY_LENGTHS, 32, blockers=TINY_BLOCKERS, blocker_tile=TINY_TILE)
        sp, st = scene[0], scene[1]
        inline = render(sp, st, dev)
        try:
            assert set_sort_kernel("standalone") == "inline"
            alone = render(sp, st, dev)
        finally:
            set_sort_kernel(None)
        _runs[name] = (scene, inline, alone)
    return _runs[name]


def host_keys(sp, st):
    """(float bits of the view depth << 32) | splat index.  The depth is evaluated in float like the kernels do, possibly in
    another order of operations: levels are 2e-3 apart and the splats of a level have bit-identical positions, so the ORDER of
    the keys does not depend on it."""
    m, V = sp["means3D"].float(), st.viewmatrix.float()
    zv = m[:, 0] * V[0, 2] + m[:, 1] * V[1, 2] + m[:, 2] * V[2, 2] + V[3, 2]
    assert (zv > 0.2).all()
    return (zv.view(torch.int32).to(torch.int64) << 32) | torch.arange(m.shape[0], dtype=torch.int64)


def assert_lists_are_host_sorted(run, sp, st, tag):
    keys = host_keys(sp, st)
    ts, ids = run["tile_start"], run["sorted_id"]
    for t in range(GX * GY):
        got = ids[int(ts[t]):int(ts[t + 1])]
        assert got.unique().numel() == got.numel(), f"{tag}: tile {t} holds a splat twice"
        want = got[torch.argsort(keys[got])]   # keys are unique
        if not torch.equal(got, want):
            bad = int(torch.nonzero(got != want)[0])
            raise AssertionError(f"{tag}: tile {t} ({got.numel()} entries) is not in (depth, index) order from position {bad}")


def assert_bit_identical(a, b, tag):
    assert torch.equal(a["tile_start"], b["tile_start"]) and torch.equal(a["sorted_id"], b["sorted_id"]), f"{tag}: lists differ"
    for k in a["out"]:
        assert torch.equal(a["out"][k], b["out"][k]), f"{tag}: output {k} differs"
    for k in a["grads"]:
        assert torch.equal(a["grads"][k], b["grads"][k]), f"{tag}: gradient {k} differs"


def test_the_switch_selects_who_sorts_the_short_lists(hip_device):
    """Launch counters of one forward: [0] k_sort_tiles_regs, [1] lists 2049..4096, [2] 4097..8192, [3] longer."""
    _, inline, alone = both_switches("boundaries", hip_device)
    assert inline["launched"] == [0, 1, 1, 0]   # the longest list has 4097 entries: both merge classes, nothing for <= 2048
    assert alone["launched"] == [1, 1, 1, 0]
    _, inline, alone = both_switches("tiny", hip_device)
    assert inline["launched"] == [0, 0, 0, 0]   # longest list 2048: no separate sort launch at all
    assert alone["launched"] == [1, 0, 0, 0]


def test_every_length_boundary_gives_the_host_sorted_list(hip_device):
    (sp, st, idx, tile), inline, alone = both_switches("boundaries", hip_device)
    lengths = (inline["tile_start"][1:] - inline["tile_start"][:-1]).tolist()
    assert lengths == BOUNDARY_LENGTHS
    for t in range(GX * GY):   # membership: exactly the splats placed on the tile
        got = inline["sorted_id"][int(inline["tile_start"][t]):int(inline["tile_start"][t + 1])]
        assert torch.equal(got.sort().values, idx[tile == t].sort().values), t
    assert_lists_are_host_sorted(inline, sp, st, "inline")
    assert_lists_are_host_sorted(alone, sp, st, "standalone")
    assert torch.isfinite(inline["out"]["color"]).all()


def test_every_length_boundary_is_bit_identical_under_both_switches(hip_device):
    _, inline, alone = both_switches("boundaries", hip_device)
    assert_bit_identical(inline, alone, "boundaries")
    # (the splats are isotropic and sit on pixel centres: not every tensor has a gradient; these three must)
    assert all(float(inline["grads"][k].abs().max()) > 0 for k in ("means3D", "opacities", "shs"))


def test_an_unreached_tail_is_sorted_and_an_empty_tile_stays_empty(hip_device):
    (sp, st, idx, tile), inline, alone = both_switches("tiny", hip_device)
    ts = inline["tile_start"]
    lengths = (ts[1:] - ts[:-1]).tolist()
    assert lengths[15] == 0 and lengths[3] == TINY_LENGTHS[3] and lengths[12] == TINY_LENGTHS[12]
    n_tail = sum(TINY_LENGTHS)
    blockers = idx[n_tail:]                        # splat indices of the blockers
    tail = idx[:n_tail][tile[:n_tail] == TINY_TILE]
    got = inline["sorted_id"][int(ts[TINY_TILE]):int(ts[TINY_TILE + 1])]
    # the tile's list: all blockers (nearer: in front), then the whole tail
    assert got.numel() == TINY_BLOCKERS + TINY_TAIL == 2000
    assert torch.equal(got[:TINY_BLOCKERS], blockers.sort().values)
    assert torch.equal(got[TINY_BLOCKERS:].sort().values, tail.sort().values)
    assert_lists_are_host_sorted(inline, sp, st, "inline")
    assert_lists_are_host_sorted(alone, sp, st, "standalone")
    # every pixel of the tile stopped in front of the tail, i.e. inside the first batch of 256: no tail entry has a gradient
    # (exactly zero in every tensor), and the tile's transmittance is what a stop leaves: below 1e-4 / (1 - 0.95)
    for k, g in inline["grads"].items():
        assert (g[tail] == 0).all(), k
    assert float(inline["grads"]["opacities"][blockers].abs().max()) > 0
    ty, tx = divmod(TINY_TILE, GX)
    assert float(inline["out"]["alpha"][..., 16 * ty:16 * ty + 16, 16 * tx:16 * tx + 16].min()) > 1.0 - 2.1e-3
    assert_bit_identical(inline, alone, "tiny")


# ------------------------------------------------------------------------------------------------ the long-tile constant

def test_with_exactly_the_constant_of_long_tiles_the_forward_sorts_them(hip_device):
    assert sum(L > 2048 for L in FEW_LONG_LENGTHS) == K_LONG
    (sp, st, idx, tile), inline, alone = both_switches("few_long", hip_device)
    assert (inline["tile_start"][1:] - inline["tile_start"][:-1]).tolist() == FEW_LONG_LENGTHS
    assert inline["launched"] == [0, 0, 0, 0]      # no separate sort launch at all: the host knew the figures and left it out
    assert alone["launched"] == [1, 1, 0, 0]
    assert_lists_are_host_sorted(inline, sp, st, "inline")
    assert_lists_are_host_sorted(alone, sp, st, "standalone")
    assert_bit_identical(inline, alone, "few_long")


def test_with_one_long_tile_more_the_merge_launch_runs(hip_device):
    assert sum(L > 2048 for L in MANY_LONG_LENGTHS) == K_LONG + 1
    (sp, st, idx, tile), inline, alone = both_switches("many_long", hip_device)
    assert (inline["tile_start"][1:] - inline["tile_start"][:-1]).tolist() == MANY_LONG_LENGTHS
    assert inline["launched"] == [0, 1, 0, 0]      # lists up to 2048 in the forward, the nine long ones in the launch of their class
    assert alone["launched"] == [1, 1, 0, 0]
    assert_lists_are_host_sorted(inline, sp, st, "inline")
    assert_bit_identical(inline, alone, "many_long")


def test_the_short_only_switch_keeps_the_merge_launch(hip_device):
    from splatfields_amd.rasterizer import set_sort_kernel
    (sp, st, idx, tile), inline, alone = both_switches("few_long", hip_device)
    try:
        assert set_sort_kernel("short") == "inline"
        short = render(sp, st, hip_device)
    finally:
        set_sort_kernel(None)
    assert short["launched"] == [0, 1, 0, 0]
    assert_bit_identical(inline, short, "few_long, short-only switch")


def test_a_forward_launched_on_the_expectation_of_no_long_tile_sorts_the_two_it_meets(hip_device):
    """The camera's record says: longest list 2300 (so the launch covers lists up to 4096), no long tile.  The host leaves the
    merge launch out on that expectation; the view has two long tiles; the forward blend sorts them itself."""
    from splatfields_amd import rasterizer as rz
    (sp, st, idx, tile), inline, alone = both_switches("two_long", hip_device)   # waiting renders: the camera is known now
    assert inline["launched"] == [0, 0, 0, 0]
    n = sp["means3D"].shape[0]
    pack = rz._ViewPack.get(raster_settings(st, hip_device), hip_device, 16)
    key = (id(pack.seen), n)
    assert pack.seen[n][1] == 2300 and rz._ESTIMATES.long_tiles[key] == 2
    prev = rz.set_async_forward(True)
    try:
        rz._ESTIMATES.long_tiles[key] = 0                       # a stale expectation
        rz.host_sync_counters(reset=True)
        late = render(sp, st, hip_device)
        c = rz.host_sync_counters()
        assert c["forward_host_waits"] == 0 and c["async_forwards"] == 1, c
        assert late["launched"] == [0, 0, 0, 0]     # launched without the merge class ...
        assert rz._ESTIMATES.long_tiles[key] == 2               # ... and the ticket corrected the record
        assert_lists_are_host_sorted(late, sp, st, "async")
        assert_bit_identical(inline, late, "two_long, async on a stale expectation")
        # the record is right now: still no merge launch (two long tiles are few), same result
        again = render(sp, st, hip_device)
        assert again["launched"] == [0, 0, 0, 0] and rz.host_sync_counters()["async_forwards"] == 2
        assert_bit_identical(inline, again, "two_long, async")
        # ... and a record of many long tiles keeps the launch; its workgroups find few on the device and leave them to the forward
        rz._ESTIMATES.long_tiles[key] = 100
        many = render(sp, st, hip_device)
        assert many["launched"] == [0, 1, 0, 0]
        assert_bit_identical(inline, many, "two_long, async, merge class launched")
    finally:
        rz.set_async_forward(prev)
