"""Restatements for the subset step (csrc/subset.hip, splatfields_amd/subset.py).

numpy: the keyed bijection P of include/splatraster.h (`sr_draw_rows`), bit for bit: an alternating Feistel network over the
smallest power-of-two domain that holds n_rows, walked until it lands below n_rows; the keys come from one 64-bit seed through
splitmix64.  PyTorch: the reference's subset step in its own form -- `get_gaussian_dict` (train.py:36-101) with the row list
given instead of drawn, and the `_idx` clone / mask / assign updates of train.py:281-286 and scene/gaussian_model.py:431-438.
Imports numpy and torch only."""
import numpy as np
import torch

MASK64 = (1 << 64) - 1
ROUNDS = 8                    # splatfields_amd/subset.py: ROUNDS
MAX_WALK = 256                # include/splatraster.h: SR_DRAW_MAX_WALK


def splitmix64(seed: int, n: int) -> list:
    """the first n outputs of splitmix64 started at `seed`"""
    out, s = [], seed & MASK64
    for _ in range(n):
        s = (s + 0x9E3779B97F4A7C15) & MASK64
        z = s
        z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & MASK64
        z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & MASK64
        out.append(z ^ (z >> 31))
    return out


def keys_of(seed: int, rounds: int = ROUNDS) -> list:
    return splitmix64(seed, rounds)


def halves(n_rows: int):
    """(bits of the low half, bits of the high half) of the smallest power-of-two domain >= n_rows"""
    bits = 0
    while (1 << bits) < n_rows:
        bits += 1
    return bits // 2, bits - bits // 2


def mix(v, key: int):
    """uint32 arithmetic, carried in uint64 and masked after every product and sum"""
    m32 = np.uint64(0xFFFFFFFF)
    k_lo, k_hi = np.uint64(key & 0xFFFFFFFF), np.uint64(key >> 32)
    h = ((v + k_lo) & m32) * np.uint64(0x9E3779B1) & m32
    h ^= h >> np.uint64(15)
    h = ((h ^ k_hi) * np.uint64(0x85EBCA6B)) & m32
    h ^= h >> np.uint64(13)
    h = (h * np.uint64(0xC2B2AE35)) & m32
    h ^= h >> np.uint64(16)
    return h


def network(x, n_rows: int, keys, inverse: bool = False):
    """F (or F^-1) of every element of x (values below the domain's size), as uint64"""
    lo_bits, hi_bits = halves(n_rows)
    lo_mask, hi_mask = np.uint64((1 << lo_bits) - 1), np.uint64((1 << hi_bits) - 1)
    x = np.asarray(x, np.uint64)
    lo, hi = x & lo_mask, x >> np.uint64(lo_bits)
    order = range(len(keys) - 1, -1, -1) if inverse else range(len(keys))
    for r in order:
        if r & 1:
            hi = hi ^ (mix(lo, keys[r]) & hi_mask)
        else:
            lo = lo ^ (mix(hi, keys[r]) & lo_mask)
    return (hi << np.uint64(lo_bits)) | lo


def domain_table(n_rows: int, keys, inverse: bool = False):
    """F of the whole domain: every n_rows with the same number of bits shares it"""
    lo_bits, hi_bits = halves(n_rows)
    return network(np.arange(1 << (lo_bits + hi_bits), dtype=np.uint64), n_rows, keys, inverse)


def permute(j, n_rows: int, keys, inverse: bool = False, table=None, return_walk: bool = False):
    """P(j) (P^-1(j)) for an array of j < n_rows, int64; -1 where the walk did not end within MAX_WALK steps.  `table`: the
    domain_table of these keys, looked up instead of evaluating the network (the same values).  return_walk: also the longest
    walk."""
    y = np.asarray(j, np.uint64).copy()
    out = np.full(y.shape, -1, np.int64)
    todo = np.arange(y.size)
    longest = 0
    for step in range(1, MAX_WALK + 1):
        if todo.size == 0:
            break
        longest = step
        y = table[y] if table is not None else network(y, n_rows, keys, inverse)
        done = y < np.uint64(n_rows)
        out[todo[done]] = y[done].astype(np.int64)
        todo, y = todo[~done], y[~done]
    return (out, longest) if return_walk else out


def draw_rows(n_rows: int, n_pick: int, seed: int, order: str = "draw", rounds: int = ROUNDS):
    """what splatfields_amd.draw_rows(n_rows, n_pick, seed=seed, order=order) returns, as int64 numpy"""
    idx = permute(np.arange(n_pick, dtype=np.uint64), n_rows, keys_of(seed, rounds))
    return np.sort(idx) if order == "ascending" else idx


# ---- the reference's subset step in PyTorch ---------------------------------------------------------------------------------

class StandInGaussians:
    """the attributes of the reference GaussianModel that get_gaussian_dict reads (scene/gaussian_model.py:64-86)"""

    def __init__(self, n, sh_degree=3, isotropic=False, device="cpu", seed=0, requires_grad=True):
        g = torch.Generator().manual_seed(seed)
        mk = lambda *s, scale=1.0: (torch.randn(*s, generator=g) * scale).to(device).requires_grad_(requires_grad)
        self._xyz = mk(n, 3)
        self._scaling = mk(n, 1 if isotropic else 3, scale=0.5)
        self._features_dc = mk(n, 1, 3)
        self._features_rest = mk(n, (sh_degree + 1) ** 2 - 1, 3, scale=0.1)
        self._rotation = mk(n, 4)
        self._opacity = mk(n, 1)
        self.use_isotropic = isotropic
        self.active_sh_degree = sh_degree

    @property
    def get_xyz(self):
        return self._xyz

    @property
    def get_scaling(self):
        s = torch.exp(self._scaling)
        return s.repeat(1, 3) if self.use_isotropic else s

    @property
    def get_features(self):
        return torch.cat((self._features_dc, self._features_rest), dim=1)

    @property
    def get_rotation(self):
        return torch.nn.functional.normalize(self._rotation)

    @property
    def get_opacity(self):
        return torch.sigmoid(self._opacity)


class StandInCamera:
    def __init__(self, fid=0.25):
        self.fid = torch.tensor([fid])


class StubDeform:
    """a small deform.step: differentiable in its weights, with the colour branch of the reference network chosen by `colour`
    ("features", "rgb", "rgb_fnc" or None) and an optional gradient_error entry"""

    def __init__(self, colour=None, sh_coeffs=16, device="cpu", gradient_error=False):
        self.colour, self.sh_coeffs, self.gradient_error = colour, sh_coeffs, gradient_error
        g = torch.Generator().manual_seed(7)
        self.w = (torch.randn(4, 8, generator=g) * 0.1).to(device).requires_grad_(True)

    def step(self, xyz, time_input):
        h = torch.cat([xyz, time_input], dim=1) @ self.w                      # [n, 8]
        ret = {"means3D": xyz + 0.05 * h[:, :3], "opacity": torch.sigmoid(h[:, 3:4] + 1.0), "scales": 0.01 * h[:, 4:7],
               "rotations": torch.nn.functional.normalize(torch.cat([1.0 + h[:, 7:8], h[:, :3]], dim=1))}
        if self.colour == "features":
            ret["gaussian_features"] = (h[:, :1] * torch.ones(1, self.sh_coeffs * 3, device=xyz.device))
        elif self.colour == "rgb":
            ret["rgb"] = torch.sigmoid(h[:, :3])
        elif self.colour == "rgb_fnc":
            ret["rgb_fnc"] = lambda dirs, _h=h: torch.sigmoid(_h[:, :3] + dirs)
        if self.gradient_error:
            ret["gradient_error"] = h[:, :1].abs().mean()
        return ret


def get_gaussian_dict(viewpoint_cam, gaussians, deform, iteration=None, warm_up=None, static=False, n_splats=-1, idx=None):
    """reference train.py:36-101 with plain PyTorch indexing; the one change: the row list `idx` is GIVEN (int64 tensor) where the
    reference draws torch.randperm(N)[:n_splats] -- it is used iff the reference's condition 0 < n_splats < N holds"""
    fid = viewpoint_cam.fid.to(gaussians.get_xyz.device)
    if static:
        fid = 0 * fid
    if static or (iteration is not None and warm_up is not None and iteration < warm_up):
        return {"means3D": gaussians.get_xyz, "active_sh_degree": gaussians.active_sh_degree, "gaussian_opacity": gaussians.get_opacity,
                "gaussian_features": gaussians.get_features, "gaussian_scales": gaussians.get_scaling,
                "gaussian_rotations": gaussians.get_rotation}, None
    xyz, scaling, features = gaussians.get_xyz.detach(), gaussians.get_scaling.detach(), gaussians.get_features
    if 0 < n_splats < xyz.shape[0]:
        assert idx is not None and idx.numel() == n_splats
        xyz, scaling, features = xyz[idx], scaling[idx], features[idx]
    else:
        idx = None
    ret = deform.step(xyz, fid.detach().unsqueeze(0).expand(xyz.shape[0], -1))
    d = {"idx": idx, "means3D": ret["means3D"], "active_sh_degree": gaussians.active_sh_degree, "gaussian_opacity": ret["opacity"],
         "gaussian_scales": ret["scales"] + scaling, "gaussian_rotations": ret["rotations"], "gradient_error": ret.get("gradient_error", None)}
    if "gaussian_features" in ret:
        d["gaussian_features"] = ret["gaussian_features"].view(features.shape) * 0.1 + features
    elif "rgb" in ret:
        d["gaussian_rgb"] = ret["rgb"]
    elif "rgb_fnc" in ret:
        d["gaussian_rgb_fnc"] = ret["rgb_fnc"]
    else:
        d["gaussian_features"] = features
    f_dc, f_rest = gaussians.get_features.split([gaussians._features_dc.shape[1], gaussians._features_rest.shape[1]], dim=1)
    over = {"xyz": d["means3D"], "f_dc": f_dc, "f_rest": f_rest, "opacity": d["gaussian_opacity"], "scaling": ret["scales"],
            "rotation": d["gaussian_rotations"]}
    return d, over


def stats_through_idx(viewspace_grad, radii, idx, xyz_gradient_accum, denom, max_radii2D):
    """the `_idx` branch (train.py:281-286, scene/gaussian_model.py:431-438), in place, in the reference's clone / mask / assign
    form -- except that the drawn rows of max_radii2D start from their old values, not from torch.empty_like"""
    seen = radii > 0
    m = max_radii2D[idx].clone()
    m[seen] = torch.max(m[seen], radii[seen].to(m.dtype))
    max_radii2D[idx] = m
    a = xyz_gradient_accum[idx].clone().detach()
    a[seen] += torch.norm(viewspace_grad[seen, :2], dim=-1, keepdim=True)
    xyz_gradient_accum[idx] = a
    c = denom[idx].clone().detach()
    c[seen] += 1
    denom[idx] = c
