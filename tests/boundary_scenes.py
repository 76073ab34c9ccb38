"""Deterministic scenes that put the rasterizer's hard-coded list-length boundaries exactly where a test wants them.

Every splat is placed on a chosen pixel at a chosen view depth by un-projecting through the test camera in float64 (the
oracle's pixel convention pix = ((ndc + 1) W - 1) / 2), so a tile's list, a pixel's stop and a chunk's (quad, entry) pair
count are DESIGNED, not met by chance.  CPU only; tests/test_boundary_scenes.py proves by the oracles alone that every scene
is what it claims, tests/test_gpu_list_boundaries.py runs the kernels on them.

A. Sort scenes (`sort_scenes`): a 16 T x 16 image, tile t holds exactly L_t one-tile splats (sigma 1.1 px on the tile centre),
   drawn from a few dozen depth levels that are each duplicated many times with bit-identical `means3D` (equal float depth
   keys: the order inside a level is the splat index alone), one tile of a single level, one tile of strictly distinct depths
   that DECREASE with the splat index.  Splat indices are a seeded global shuffle.

B. Blend scenes (`blend_scenes`): one 16x16 tile (one 2x2-tile and two ragged 24x20 images), "tile-wide" entries (sigma of tens
   of pixels, mildly anisotropic, randomly rotated) whose alpha varies by a few per cent over the tile:
   B1 no pixel stops, the list length is the boundary;  B2 a few strong entries make every pixel stop at list position p or
   p + 1, both inside one quad, with >= 300 entries behind;  B3 quads / sub-tiles (= wavefronts of the forward) stop early
   while the rest goes on for >= 3 batches, and tiles whose every pixel stops exactly at 256 / 257;  B4 the (quad, entry)
   pair count of a backward chunk sits on either side of the slot caps (752 / 624 with a depth gradient);  B5 groups of
   bit-identical positions with different colours: the image depends on the index order inside a tie.
   Opacities are TUNED here against the float64 alpha / transmittance arithmetic of the oracle (`_trace`), with three times
   the oracle's fragility margins, until the stop sits where it is wanted and no threshold decision is close.

Two places where the arithmetic forbids what one would like:
  * a transmittance stop cannot sit at list position 1 (or 2 without the 0.99 clamp): alpha <= 0.99 leaves T >= 0.01 after one
    entry and the second entry always passes T (1 - alpha) >= 1e-4.  The B2 family therefore starts at p = 3.
  * a FULL 256-entry chunk of `a` tile-wide and 256 - a single-quad entries has 15 a + 256 pairs: above both caps for every
    a >= 34.  The B4 sweeps a = 45..49 / 37..41 therefore use chunks of a + 8 entries (16 a + 8 pairs: the cap is crossed
    between a = 46 and 47 / 38 and 39 whatever a +-1 in a reach test does), two exact chunks on each cap (16 * 47 = 752 and
    753, 16 * 39 = 624 and 625) and one fully dense chunk of 256 tile-wide entries (4096 pairs).
"""
from __future__ import annotations

import math
from typing import NamedTuple, Optional

import numpy as np
import torch

from oracle import torch_oracle as O
from splatfields_amd.synthetic import make_camera, make_upstream_grads

ALPHA_MIN, T_STOP = 1.0 / 255.0, 1e-4
SAFETY = 3.0   # the scenes keep every decision this many oracle margins away from its threshold


def settings(W: int, H: int, sh_degree: int = 3, bg=(0.2, 0.5, 0.9), view: int = 1) -> O.OracleSettings:
    return O.settings_from_camera(make_camera(view, W, H), torch.tensor(bg, dtype=torch.float32), sh_degree)


def focal(st) -> float:
    return st.image_width / (2.0 * st.tanfovx)


def unproject(st, px, py, z) -> torch.Tensor:
    """World position (float64 [n,3]) of the point that lands on pixel (px, py) at view depth z.  Elementwise arithmetic only:
    equal inputs give bit-identical rows."""
    px, py, z = (torch.as_tensor(a, dtype=torch.float64) for a in (px, py, z))
    V = st.viewmatrix.double()
    xv = ((2.0 * px + 1.0) / st.image_width - 1.0) * st.tanfovx * (z + O.W_EPS)
    yv = ((2.0 * py + 1.0) / st.image_height - 1.0) * st.tanfovy * (z + O.W_EPS)
    pv = torch.stack([xv, yv, z], dim=1) - V[3, :3][None]
    Rinv = torch.linalg.inv(V[:3, :3])
    return pv[:, 0:1] * Rinv[0][None] + pv[:, 1:2] * Rinv[1][None] + pv[:, 2:3] * Rinv[2][None]


def _colours(rng, n):
    shs = torch.from_numpy(rng.uniform(-1.0, 1.5, size=(n, 16, 3))).float()
    shs[:, 1:, :] = torch.from_numpy(rng.normal(size=(n, 15, 3))).float() * 0.1
    return shs, torch.from_numpy(rng.uniform(0.05, 0.95, size=(n, 3))).float()


# ------------------------------------------------------------------------------------------------ A. sort scenes

class SortScene(NamedTuple):
    name: str
    sp: dict
    st: O.OracleSettings
    lengths: list
    expected: list     # per tile: int64 tensor of splat indices in (depth level, splat index) order
    levels: list       # per tile: number of distinct depths


Z_SORT = 3.0


def sort_scene(name: str, lengths, modes=None, *, seed: int, n_levels: int = 24) -> SortScene:
    """modes[t]: "levels" (default), "single" (one level: a pure index sort) or "reverse" (distinct depths decreasing with the
    splat index)."""
    T = len(lengths)
    modes = modes or {}
    st = settings(16 * T, 16)
    rng = np.random.default_rng(seed)
    tile = np.concatenate([np.full(L, t, dtype=np.int64) for t, L in enumerate(lengths)]) if sum(lengths) else np.zeros(0, np.int64)
    n = tile.size
    index_of = rng.permutation(n)            # record r is splat index_of[r]: index order interleaves with arrival order
    level = np.zeros(n, dtype=np.int64)
    zrel = np.zeros(n, dtype=np.float64)
    n_lev = []
    off = 0
    for t, L in enumerate(lengths):
        sl = slice(off, off + L)
        mode = modes.get(t, "levels")
        if mode == "reverse":
            rank = np.argsort(np.argsort(index_of[sl]))          # rank of the splat index inside the tile
            level[sl] = L - 1 - rank
            zrel[sl] = 0.1 * level[sl] / max(L, 1)                # >= 1.2e-5 apart (L <= 8193): far beyond a float ulp
            n_lev.append(L)
        else:
            K = 1 if mode == "single" else max(1, min(n_levels, L // 8))
            level[sl] = rng.integers(0, K, size=L)
            zrel[sl] = 2e-3 * level[sl]                           # levels >= 1e-3 apart (relative)
            n_lev.append(int(np.unique(level[sl]).size) if L else 0)
        off += L
    z = Z_SORT * (1.0 + zrel)
    means_rec = unproject(st, 16.0 * tile + 7.5, np.full(n, 7.5), z)
    s_rec = math.sqrt(1.1 * 1.1 - O.COV2D_DILATION) * z / focal(st)       # sigma 1.1 px (up to 6 % more off-axis): radius 4 < 8
    means = torch.zeros(n, 3, dtype=torch.float64)
    scal = torch.zeros(n, dtype=torch.float64)
    idx = torch.from_numpy(index_of)
    means[idx] = means_rec
    scal[idx] = torch.from_numpy(s_rec)
    shs, rgb = _colours(rng, n)
    rots = torch.zeros(n, 4)
    rots[:, 0] = 1.0
    sp = dict(means3D=means.float(), scales=scal.float()[:, None].expand(n, 3).contiguous(), rotations=rots,
              opacities=torch.from_numpy(rng.uniform(0.04, 0.08, size=(n, 1))).float(), shs=shs, colors_precomp=rgb)
    expected, off = [], 0
    for t, L in enumerate(lengths):
        order = np.lexsort((index_of[off:off + L], level[off:off + L]))
        expected.append(torch.from_numpy(index_of[off:off + L][order].astype(np.int64)))
        off += L
    return SortScene(name, sp, st, list(lengths), expected, n_lev)


# Every list-length boundary of csrc/binning.hip at least once; images whose LONGEST list is 2049, 4097, 8193 (the class of the
# longest list is the boundary class: head-of-order slot counts), one image that mixes a 24577-entry tile with both sides of
# every long class and empty tiles; no image above 60 k splats.  Every image has a single-level and a reversed tile.
_SORT_SPECS = {
    "longest2049": ([0, 1, 2, 3, 255, 256, 257, 511, 512, 513, 1023, 1024, 1025, 1280, 1281, 1536, 1537, 2047, 2048, 2049],
                    {9: "single", 12: "single", 14: "reverse", 17: "reverse"}, 11),
    "longest4097": ([3072, 0, 3073, 4095, 1025, 4096, 4097, 2049], {0: "reverse", 5: "single"}, 12),
    "longest8193": ([8191, 257, 8192, 0, 8193, 4097], {4: "reverse", 5: "single"}, 13),
    "mixed24577": ([2048, 0, 24577, 2049, 4096, 0, 4097, 8192, 8193], {6: "single", 3: "reverse"}, 14),
    "two_chunks": ([16384, 1, 16385, 0, 1024, 513], {4: "reverse", 5: "single"}, 15),
}
SORT_NAMES = list(_SORT_SPECS)
_sort_cache = {}


def sort_scene_by_name(name: str) -> SortScene:
    if name not in _sort_cache:
        lengths, modes, seed = _SORT_SPECS[name]
        _sort_cache[name] = sort_scene(name, lengths, modes, seed=seed)
    return _sort_cache[name]


def sort_scenes() -> list:
    return [sort_scene_by_name(n) for n in SORT_NAMES]


# ------------------------------------------------------------------------------------------------ B. blend scenes

class BlendScene(NamedTuple):
    name: str
    family: str
    sp: dict
    st: O.OracleSettings
    use_sh: bool
    length: int           # list length of every tile
    pos: torch.Tensor     # [N] 1-based list position of every splat (0: culled)
    groups: dict          # name -> int64 indices: the splat groups gradients are compared on
    nc_min: int           # designed min / max of n_contrib over the image ...
    nc_max: int
    dead: Optional[torch.Tensor]   # ... B3: [H,W] bool, pixels that stop early (n_contrib <= nc_dead); all others reach `length`
    nc_dead: int
    behind: torch.Tensor  # splats behind every pixel's stop: exactly zero gradient
    last: torch.Tensor    # splats at the designed last position(s): non-zero opacity gradient
    pairs: int = -1       # B4: designed (quad, entry) pair count of the one backward chunk


Z_BLEND = 2.5


class _Entries:
    """Entries of one tile list in front-to-back order; `finish` shuffles the splat indices."""

    def __init__(self, st, rng):
        self.st, self.rng = st, rng
        self.px, self.py, self.sc, self.rot, self.op, self.kind, self.zfix = [], [], [], [], [], [], []

    def wide(self, n, op, kind, *, sig=(34.0, 40.0), spread=3.0, centre=None):
        """n tile-wide entries: minor sigma in `sig` px, axis ratio 1.2 .. 2, random rotation, centre within `spread` px of
        `centre` (default the image centre) and at least a third of a pixel away from every pixel centre (power is never ~ 0)."""
        W, H, r = self.st.image_width, self.st.image_height, self.rng
        cx, cy = centre if centre is not None else ((W - 1) / 2.0, (H - 1) / 2.0)
        for i in range(n):
            self.px.append(math.floor(cx + r.uniform(-spread, spread)) + r.uniform(0.35, 0.65))
            self.py.append(math.floor(cy + r.uniform(-spread, spread)) + r.uniform(0.35, 0.65))
            s = r.uniform(*sig)
            self.sc.append([s, s * r.uniform(1.2, 2.0), s * r.uniform(1.0, 1.5)])
            q = r.normal(size=4)
            self.rot.append(q / np.linalg.norm(q))
            self.op.append(float(op[i]) if np.ndim(op) else float(op))
            self.kind.append(kind)
            self.zfix.append(None)

    def small(self, px, py, sigma2, op, kind):
        """One isotropic entry of 2D variance sigma2 (>= the 0.3 dilation) on (px, py)."""
        s = math.sqrt(max(sigma2 - O.COV2D_DILATION, 1e-4))
        self.px.append(px); self.py.append(py); self.sc.append([s, s, s])
        q = self.rng.normal(size=4)
        self.rot.append(q / np.linalg.norm(q))
        self.op.append(float(op)); self.kind.append(kind); self.zfix.append(None)

    def tie_with_previous(self):
        """The last entry shares the position (pixel and depth) of the one before it, bit for bit."""
        self.px[-1], self.py[-1] = self.px[-2], self.py[-2]
        self.zfix[-1] = len(self.px) - 2

    def __len__(self):
        return len(self.px)

    def finish(self, pad_to: int = 0):
        st, rng, L = self.st, self.rng, len(self)
        zi = np.arange(L, dtype=np.float64)
        for j, f in enumerate(self.zfix):
            if f is not None:
                zi[j] = zi[f]
        z = Z_BLEND * (1.0 + 2e-4 * zi)
        means = unproject(st, np.array(self.px), np.array(self.py), z)
        scales = torch.tensor(np.array(self.sc)) * torch.from_numpy(z)[:, None] / focal(st)
        n = max(L, pad_to)
        if n > L:   # culled filler: behind the camera
            k = n - L
            means = torch.cat([means, unproject(st, rng.uniform(0, 15, k), rng.uniform(0, 15, k), -rng.uniform(0.5, 2.0, k))])
            scales = torch.cat([scales, torch.full((k, 3), 0.05, dtype=torch.float64)])
        rot = torch.tensor(np.array(self.rot + [[1.0, 0.0, 0.0, 0.0]] * (n - L)))
        op = torch.tensor(self.op + [0.5] * (n - L), dtype=torch.float64)
        # splat indices: a shuffle that keeps tied entries in list order (a tie is ordered by index)
        index_of = rng.permutation(n)
        root = list(range(L))
        for j, f in enumerate(self.zfix):
            if f is not None:
                root[j] = root[f]
        for r in set(root):
            members = [j for j in range(L) if root[j] == r]
            index_of[members] = np.sort(index_of[members])
        idx = torch.from_numpy(index_of)
        shs, rgb = _colours(rng, n)
        out = {}
        for k, v in (("means3D", means), ("scales", scales), ("rotations", rot), ("opacities", op[:, None])):
            t = torch.zeros(n, v.shape[1], dtype=torch.float32)
            t[idx] = v.float()
            out[k] = t
        out["shs"], out["colors_precomp"] = shs, rgb
        pos = torch.zeros(n, dtype=torch.int64)
        pos[idx[:L]] = torch.arange(1, L + 1)
        kinds = np.array(self.kind)
        groups = {k: idx[:L][torch.from_numpy(np.nonzero(kinds == k)[0])] for k in dict.fromkeys(self.kind)}
        return out, pos, groups, idx[:L]


def _gauss(sp, st, order):
    """(G[P, L], power[P, L]): G = exp(power) of list entry j (splat order[j]) on pixel P of the image, float64, the oracle's own preprocessing."""
    d = {k: v.double() for k, v in sp.items()}
    pre = O.preprocess(d["means3D"], None, d["opacities"], None, d["colors_precomp"], d["scales"], d["rotations"], None, st)
    assert bool(pre.visible[order].all())
    ys, xs = torch.meshgrid(torch.arange(st.image_height, dtype=torch.float64), torch.arange(st.image_width, dtype=torch.float64), indexing="ij")
    dx = pre.pix[order, 0][None, :] - xs.reshape(-1, 1)
    dy = pre.pix[order, 1][None, :] - ys.reshape(-1, 1)
    A, B, C = pre.conic[order, 0][None], pre.conic[order, 1][None], pre.conic[order, 2][None]
    power = -0.5 * (A * dx * dx + C * dy * dy) - B * dx * dy
    assert bool((power <= 0).all())
    return torch.exp(power), power


def _trace(G, power, op, margin=SAFETY * 2e-4):
    """The oracle's blend decisions (oracle/torch_oracle.py rasterize) for opacities `op` in list order: n_contrib[P], a
    per-pixel `fragile` flag at `margin`, and the inclusive transmittance products Q[P, L] of the valid entries."""
    alpha = torch.clamp_max(op[None, :] * G, O.ALPHA_MAX)
    valid = alpha >= ALPHA_MIN
    Q = torch.cumprod(1.0 - torch.where(valid, alpha, torch.zeros_like(alpha)), dim=1)
    blended = valid & (Q >= T_STOP)
    pos = torch.arange(1, G.shape[1] + 1)[None, :].expand_as(blended)
    nc = torch.where(blended, pos, torch.zeros_like(pos)).max(dim=1).values
    reached = torch.cat([torch.ones_like(valid[:, :1]), Q[:, :-1] >= T_STOP * (1 - 50 * margin)], dim=1)
    frag = ((((alpha - ALPHA_MIN).abs() < margin * ALPHA_MIN) | (valid & ((Q - T_STOP).abs() < 50 * margin * T_STOP))
             | ((power.abs() < 3e-6) & (op[None, :] * G >= ALPHA_MIN))) & reached).any(dim=1)
    return nc, frag, Q


def _sig(W, H):
    """Minor sigma range of the faint tile-wide entries: alpha >= 1/255 with >= 10 % to spare in the image's corners."""
    k = max(W, H) / 16.0
    return (34.0 * k, 40.0 * k)


def _f32(x):
    return torch.as_tensor(x, dtype=torch.float64).float().double()


def _make(name, family, ent: _Entries, st, use_sh, *, nc_min=None, nc_max=None, dead=None, nc_dead=0, behind_from=None, last_pos=(),
          pad_to=0, pairs=-1):
    sp, pos, groups, order = ent.finish(pad_to)
    L = len(ent)
    behind = order[behind_from:] if behind_from is not None else order[:0]
    last = order[torch.tensor([p - 1 for p in last_pos], dtype=torch.int64)] if len(last_pos) else order[:0]
    return BlendScene(name, family, sp, st, use_sh, L, pos, groups, L if nc_min is None else nc_min, L if nc_max is None else nc_max,
                      dead, nc_dead, behind, last, pairs)


def _retune(sp, order, op_list):
    sp["opacities"][order, 0] = op_list.float()


def b1_scene(L: int, *, W=16, H=16, use_sh=True, seed=100) -> BlendScene:
    """L faint tile-wide entries (opacity 0.005 .. 0.006, alpha >= 1/255 with >= 10 % to spare on every pixel): nothing stops,
    n_contrib == L everywhere (1 - 0.994^760 leaves T ~ 0.015)."""
    st = settings(W, H)
    rng = np.random.default_rng(seed + L)
    ent = _Entries(st, rng)
    ent.wide(L, rng.uniform(0.005, 0.006, size=L), "faint", sig=_sig(W, H))
    sc = _make(f"B1_L{L}_{W}x{H}" + ("" if use_sh else "_rgb"), "B1", ent, st, use_sh, last_pos=(L,))
    _check(sc)
    return sc


def b2_scene(p: int, *, cutter=True, tail=300, W=16, H=16, use_sh=True, seed=200, pad_to=0, family="B2", name=None) -> BlendScene:
    """Every pixel's last contributor at list position p (and p + 1 on a ring of pixels when `cutter`):
        1 .. p - m        faint tile-wide entries
        p - m + 1 .. p    m strong tile-wide entries, ONE opacity tuned so that min over pixels of T after entry p = 1.3e-4
        p + 1             (cutter) a strong sigma-1.4 px entry near the tile centre: pixels near its centre fail the T test on it
                          and stop at p, a ring around them blends it and stops at p + 1, pixels it does not reach stop at p
        next              a closer (tile-wide, 0.95) that no pixel survives, then `tail` faint entries behind every stop."""
    for attempt in range(8):   # a geometry whose ring happens to graze a threshold on some pixel is redrawn
        try:
            return _b2_build(p, cutter, tail, W, H, use_sh, seed + 7919 * attempt, pad_to, family, name)
        except AssertionError:
            if attempt == 7:
                raise


def _b2_build(p, cutter, tail, W, H, use_sh, seed, pad_to, family, name) -> BlendScene:
    st = settings(W, H)
    rng = np.random.default_rng(seed + p + 1000 * int(cutter))
    ent = _Entries(st, rng)
    front_op = rng.uniform(0.005, 0.006, size=max(p, 1))
    Fest = np.cumprod(1.0 - 0.95 * front_op)
    m = 1
    while m < p and Fest[p - m - 1] * (1 - 0.8 * 0.97) ** m > 1.3e-4:   # strong entries needed at alpha ~ 0.78 each
        m += 1
    ent.wide(p - m, front_op[:p - m], "faint", sig=_sig(W, H))
    ent.wide(m, 0.8, "opaque", sig=(45.0, 55.0), spread=2.0)
    if cutter:
        ent.small(7.0 + rng.uniform(0.3, 0.7), 7.0 + rng.uniform(0.3, 0.7), 2.0, 0.8, "cutter")
    ent.wide(1, 0.95, "behind", sig=(45.0, 55.0), spread=2.0)
    ent.wide(tail, rng.uniform(0.005, 0.006, size=tail), "behind", sig=_sig(W, H))
    sc = _make(name or f"{family}_p{p}" + ("" if cutter else "_all") + f"_{W}x{H}", family, ent, st, use_sh, nc_min=p,
               nc_max=p + int(cutter), behind_from=p + int(cutter), last_pos=(p, p + 1) if cutter else (p,), pad_to=pad_to)
    order = sc.pos.argsort()[-sc.length:]
    G, power = _gauss(sc.sp, st, order)
    op = sc.sp["opacities"][order, 0].double()
    lo, hi = 0.3, 0.985
    for _ in range(60):   # bisection on the strong entries' opacity: min over pixels of Q_p -> 1.3e-4
        mid = 0.5 * (lo + hi)
        op[p - m:p] = _f32(mid)
        q = _trace(G, power, op)[2][:, p - 1].min().item()
        lo, hi = (mid, hi) if q > 1.3e-4 else (lo, mid)
    op[p - m:p] = _f32(lo)
    if cutter:
        quads = (torch.arange(H)[:, None] // 4 * ((W + 3) // 4) + torch.arange(W)[None, :] // 4).reshape(-1)
        for oc in np.linspace(0.9, 0.4, 101):
            op[p] = _f32(oc)
            nc, frag, _ = _trace(G, power, op)
            both = [q for q in quads.unique() if set(nc[quads == q].tolist()) == {p, p + 1}]
            if not frag.any() and set(nc.tolist()) == {p, p + 1} and both and int((nc == p + 1).sum()) >= 4:
                break
        else:
            raise AssertionError(f"{sc.name}: no cutter opacity leaves the scene flip-free")
    _retune(sc.sp, order, op)
    _check(sc)
    return sc


def b3_scene(regions, layers_hint=10, *, tail=900, seed=300, name="") -> BlendScene:
    """Strong small splats (2D variance 0.64, one per 2x2 pixel block and layer) kill the pixel regions `regions` -- rectangles
    (x0, y0, w, h) of whole quads / 8x8 sub-tiles (an 8x8 sub-tile is one wavefront of the forward) -- within the first entries
    of the list; every other pixel goes on through `tail` faint tile-wide entries (>= 3 forward batches / backward chunks)."""
    st = settings(16, 16)
    dead = torch.zeros(16, 16, dtype=torch.bool)
    for x0, y0, w, h in regions:
        dead[y0:y0 + h, x0:x0 + w] = True
    blocks = [(x0 + 2 * i + 0.5, y0 + 2 * j + 0.5) for x0, y0, w, h in regions for j in range(h // 2) for i in range(w // 2)]
    for layers in range(layers_hint, layers_hint + 8):
        for ok_op in np.linspace(0.97, 0.80, 35):
            rng = np.random.default_rng(seed)
            ent = _Entries(st, rng)
            for _ in range(layers):
                for bx, by in blocks:
                    ent.small(bx, by, 0.64, ok_op, "opaque")
            nk = len(ent)
            ent.wide(tail, rng.uniform(0.005, 0.0058, size=tail), "faint")
            sc = _make(name, "B3", ent, st, True, nc_min=0, nc_max=len(ent), dead=dead, nc_dead=nk, last_pos=(len(ent),))
            order = sc.pos.argsort()[-sc.length:]
            G, power = _gauss(sc.sp, st, order)
            nc, frag, _ = _trace(G, power, sc.sp["opacities"][order, 0].double())
            d = dead.reshape(-1)
            if not frag.any() and bool((nc[d] <= nk).all()) and bool((nc[d] >= 1).all()) and bool((nc[~d] == len(ent)).all()):
                return sc._replace(nc_min=int(nc.min()))
    raise AssertionError(f"{name}: no killer opacity leaves the scene flip-free")


def b4_scene(a: int, singles: int, *, seed=400) -> BlendScene:
    """ONE backward chunk (the whole list, nothing stops): `a` tile-wide entries (16 quads each) and `singles` faint entries of
    2D variance 0.3 + (support radius 0.5 px) 0.1 px off an interior pixel of a quad (one quad each): 16 a + singles pairs."""
    st = settings(16, 16)
    rng = np.random.default_rng(seed + 16 * a + singles)
    ent = _Entries(st, rng)
    slots = ["w"] * a + ["s"] * singles
    rng.shuffle(slots)
    if slots[-1] == "s":   # the list ends on a tile-wide entry: n_contrib == list length on every pixel
        i = slots.index("w")
        slots[i], slots[-1] = slots[-1], slots[i]
    qs = rng.permutation(16)
    k = 0
    for s in slots:
        if s == "w":
            ent.wide(1, rng.uniform(0.005, 0.006), "faint")
        else:
            q = int(qs[k % 16]); k += 1
            ent.small(4 * (q % 4) + 1 + int(rng.integers(0, 2)) + 0.1, 4 * (q // 4) + 1 + int(rng.integers(0, 2)) - 0.07, 0.3001,
                      rng.uniform(0.008, 0.01), "single")
    sc = _make(f"B4_a{a}_s{singles}", "B4", ent, st, True, last_pos=(len(ent),), pairs=16 * a + singles)
    _check(sc)
    return sc


def b5_scene(*, seed=500) -> BlendScene:
    """Ties in the blend: four groups of three bit-identical positions (pixel and depth) with different shapes, colours and
    opacities 0.3 .. 0.6, between faint entries: the image depends on the index order inside every tie.  Nothing stops
    (0.7^12 ~ 0.014)."""
    st = settings(16, 16)
    rng = np.random.default_rng(seed)
    ent = _Entries(st, rng)
    for g in range(4):
        ent.wide(5, rng.uniform(0.005, 0.006, size=5), "faint")
        ent.wide(1, rng.uniform(0.3, 0.6), "tie", sig=(40.0, 50.0))
        for _ in range(2):
            ent.wide(1, rng.uniform(0.3, 0.6), "tie", sig=(40.0, 50.0))
            ent.tie_with_previous()
    ent.wide(5, rng.uniform(0.005, 0.006, size=5), "faint")
    sc = _make("B5_ties", "B5", ent, st, False, last_pos=(len(ent),))
    _check(sc)
    return sc


def _check(sc: BlendScene):
    """The builder's own statement of the design (the CPU test repeats it with the oracles)."""
    order = sc.pos.argsort()[-sc.length:]
    G, power = _gauss(sc.sp, sc.st, order)
    nc, frag, _ = _trace(G, power, sc.sp["opacities"][order, 0].double())
    assert not frag.any(), (sc.name, int(frag.sum()))
    assert int(nc.min()) == sc.nc_min and int(nc.max()) == sc.nc_max, (sc.name, int(nc.min()), int(nc.max()))


B1_LENGTHS = [1, 2, 3, 15, 16, 17, 31, 32, 33, 127, 128, 129, 255, 256, 257, 511, 512, 513, 760]
B2_STOPS = [3, 16, 17, 128, 129, 255, 256, 257, 511, 512, 513]
B4_CASES = [(a, 8) for a in (37, 38, 39, 40, 41, 45, 46, 47, 48, 49)] + [(39, 0), (39, 1), (47, 0), (47, 1), (256, 0)]
N_STALE = 760

_cache = {}


def _specs() -> dict:
    """name -> builder of every blend scene (nothing is built until a test asks for the scene)."""
    d = {}
    for L in B1_LENGTHS:
        d[f"B1_L{L}"] = lambda L=L: b1_scene(L, use_sh=(L % 2 == 1))
    d["B1_L257_32x32"] = lambda: b1_scene(257, W=32, H=32, use_sh=False)
    d["B1_L513_24x20"] = lambda: b1_scene(513, W=24, H=20)
    for p in B2_STOPS:
        d[f"B2_p{p}"] = lambda p=p: b2_scene(p, use_sh=(p % 2 == 0))
    d["B2_p256_all_24x20"] = lambda: b2_scene(256, cutter=False, W=24, H=20)
    d["B3_wave0_dead"] = lambda: b3_scene([(0, 0, 8, 8)])
    d["B3_three_waves_dead"] = lambda: b3_scene([(8, 0, 8, 8), (0, 8, 8, 8), (8, 8, 8, 8)])
    d["B3_one_quad_dead"] = lambda: b3_scene([(4, 4, 4, 4)])
    d["B3_all_dead_at_256"] = lambda: b2_scene(256, cutter=False, tail=800, family="B3")
    d["B3_all_dead_at_257"] = lambda: b2_scene(257, cutter=False, tail=800, family="B3")
    for a, n1 in B4_CASES:
        d[f"B4_a{a}_s{n1}"] = lambda a=a, n1=n1: b4_scene(a, n1)
    d["B5_ties"] = b5_scene
    return d


BLEND_NAMES = list(_specs())


def blend_scene(name: str) -> BlendScene:
    if name not in _cache:
        _cache[name] = _specs()[name]()._replace(name=name)
    return _cache[name]


def blend_scenes() -> list:
    return [blend_scene(n) for n in BLEND_NAMES]


def stale_pair():
    """(the 760-entry B1 scene, an all-dead-at-256 scene padded with culled splats to the same N, H, W)."""
    if "stale" not in _cache:
        a = blend_scene(f"B1_L{N_STALE}")
        b = b2_scene(256, cutter=False, tail=400, pad_to=N_STALE, family="B3", name="B3_all_dead_at_256_padded")
        assert a.sp["means3D"].shape[0] == b.sp["means3D"].shape[0] == N_STALE
        _cache["stale"] = (a, b)
    return _cache["stale"]


def upstream(sc):
    return make_upstream_grads(sc.st.image_height, sc.st.image_width)
