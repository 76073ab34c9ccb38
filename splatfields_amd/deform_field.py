"""Counterpart of the reference's `SplatFields` network (utils/time_utils.py:305-508) with its six `GeneralMLP`s on the fused
kernels (splatfields_amd/general_mlp.py).

Same constructor keywords, same `forward(xyz_in, t)` -> dict(scales, opacity, rotations, rgb | rgb_fnc, flow, means3D), same
parameter names (`mlp_deform.net.<i>...`, `mlp_refine_feat.<i>...`, `mlp_flow_head.branch_w...`), so the MLP / flow-head part of a
`deform.pth` checkpoint (reference scene/deform_model.py:36-47) loads with `load_state_dict`.  A default-config checkpoint also
carries the plane generator's weights (`encoder.subs.*`): they load, `strict=True`, when the network is built with the generator
-- `SplatFields(encoder_args={"generator": "decoder"})` (splatfields_amd/plane_generator.py) -- and `load_state_dict` says so
instead of failing on missing / unexpected keys when it was not.

The tri-plane feature encoder (reference scene/tripFields.py:383-436) is `splatfields_amd.triplane.TriPlaneSampler`: the
per-point lookup (three `grid_sample`s + cat) runs on HIP kernels, forward and backward.  With the reference's default
`encoder_type='VarTriPlaneEncoder'` and no `encoder=` argument the sampler owns its planes [3, out_ch, 16 noise_res,
16 noise_res] as a learnable parameter (a decoder-free tri-plane).  The reference GENERATES the planes with three CNN decoders
(`Tensorial2D`, :176-204): opt in with `encoder_args={"generator": "decoder", in_ch, out_ch, noise_res, fuse_mode}` (the
generator on HIP kernels, configured from `n_frames` / `layer_strategy` as utils/time_utils.py:316-327 does, and told the frame
of the step), pass a generator as `TriPlaneSampler(plane_source=...)`, or any module with the encoder's interface (`encoder(x[None]) -> [1, N, out_dim]`,
attribute `out_dim`, e.g. the reference's own `VarTriPlaneEncoder` instance) as `encoder=`.  An `encoder_type` outside the
reference's list runs without plane features (`feat_dim = 0`, utils/time_utils.py:333-334).  State-dict keys of the
decoder-free sampler are `encoder.planes`; a reference checkpoint's `encoder.subs.*` keys need the generator opt-in.

`FlowHead` (utils/time_utils.py:194-303): all seven flow models of the reference -- 'offset', 'se3' (default), 'se3Affine',
'se3Scaled', 'affine', 'dct' and 'dct_siren' -- with its parameter names; the SE(3) exponential is written out per point (no 4x4
batched matmuls), following the reference's formulas including its `w / theta + 1e-5` convention (a row with |w_raw| = 0 is
non-finite there and here).  `path="fused"` (opt-in: `SplatFields(flow_head="fused")`, `set_flow_head`, SPLATFIELDS_FLOW_HEAD) runs
the branch linears, the per-point epilogue and their backward on the kernels of csrc/flow_head.hip (splatfields_amd/flow_head.py).

`ViewColor` is `out["rgb_fnc"]` of a `use_view_dep_rgb` network (utils/time_utils.py:496): the reference's call, plus
`for_cameras(means3D, camera_centers)` for all views of a step.  `view_color="fused"` (opt-in: `SplatFields(view_color="fused")`,
`set_view_color`, SPLATFIELDS_VIEW_COLOR) runs it on the kernels of csrc/view_color.hip (splatfields_amd/view_color.py).
"""
from __future__ import annotations

import math
from typing import Optional

import torch
import torch.nn.functional as F
from torch import nn

from .fused_mlp import PointLinear
from .general_mlp import GeneralMLP, positional_encoding


def _se3_parts(w: torch.Tensor, v: torch.Tensor, theta: torch.Tensor):
    """rotation R [N, 3, 3] and translation p [N, 3] of exp of the screw (w, v) * theta (see se3_transform), in ~20 batched
    kernels: the cross products are `torch.linalg.cross` calls, [w] is minus the cross product of w with the three basis
    vectors (row j of cross(w, e_j) is column j of [w], and [w] is antisymmetric)."""
    n = w.shape[0]
    s, c = torch.sin(theta), torch.cos(theta)                    # [N, 1]
    eye = torch.eye(3, device=w.device, dtype=w.dtype)
    skew = -torch.linalg.cross(w[:, None, :].expand(n, 3, 3), eye.expand(n, 3, 3), dim=-1)
    ww = (w * w).sum(-1, keepdim=True)
    skew2 = w[:, :, None] * w[:, None, :] - ww[:, :, None] * eye
    omc = 1.0 - c
    R = eye + s[:, :, None] * skew + omc[:, :, None] * skew2
    wv = torch.linalg.cross(w, v, dim=-1)
    wwv = torch.linalg.cross(w, wv, dim=-1)
    p = theta * v + omc * wv + (theta - s) * wwv
    return R, p


def se3_transform(w: torch.Tensor, v: torch.Tensor, theta: torch.Tensor):
    """exp of the screw (w, v) * theta as the reference builds it (utils/rigid_utils.py:40-84; Modern Robotics 3.51 / 3.88),
    without assuming |w| = 1 (the reference adds 1e-5 to the normalised axis):  R = I + sin(theta) [w] + (1 - cos(theta)) [w]^2,
    p = (theta I + (1 - cos(theta)) [w] + (theta - sin(theta)) [w]^2) v, with [w]^2 = w w^T - |w|^2 I.  -> [N, 4, 4]."""
    R, p = _se3_parts(w, v, theta)
    bottom = torch.zeros(1, 1, 4, device=w.device, dtype=w.dtype)   # (device-side fill: no host -> device copy, safe under graph capture)
    bottom[..., 3] = 1.0
    return torch.cat([torch.cat([R, p[:, :, None]], dim=-1), bottom.expand(w.shape[0], 1, 4)], dim=1)


def dct_basis(num_basis: int, num_frames: int) -> torch.Tensor:
    """reference utils/time_utils.py:60-70: sqrt(2 / T) cos(pi / (2 T) (2 t + 1) k), k = 1..K"""
    t = torch.arange(num_frames, dtype=torch.float64)[:, None]
    k = torch.arange(1, num_basis + 1, dtype=torch.float64)[None, :]
    return (math.sqrt(2.0 / num_frames) * torch.cos(math.pi / (2.0 * num_frames) * (2 * t + 1) * k)).to(torch.float32)


class SirenMLP(nn.Module):
    """the reference's SIREN (utils/time_utils.py:76-121): linear layers with sin(30 x) between them, the first layer's weight
    uniform in +-1 / fan_in, the others' in +-sqrt(6 / fan_in) / 30; biases keep nn.Linear's initialisation"""

    def __init__(self, in_features: int, out_features: int, hidden_features: int, num_hidden_layers: int):
        super().__init__()
        dims = [in_features] + [hidden_features] * num_hidden_layers + [out_features]
        layers = []
        for i in range(len(dims) - 1):
            lin = nn.Linear(dims[i], dims[i + 1])
            bound = 1.0 / dims[i] if i == 0 else math.sqrt(6.0 / dims[i]) / 30.0
            with torch.no_grad():
                lin.weight.uniform_(-bound, bound)
            layers.append(lin)
        self.net = nn.Sequential(*layers)

    def forward(self, coords):
        x = coords
        for lin in self.net[:-1]:
            x = torch.sin(30 * lin(x))
        return self.net[-1](x)


FLOW_MODELS = ("offset", "se3", "se3Affine", "se3Scaled", "affine", "dct", "dct_siren")


class FlowHead(nn.Module):
    def __init__(self, W: int = 256, flow_model: str = "offset", num_basis: int = 4, n_frames: int = 100, path: Optional[str] = None):
        """`path`: "torch" (PyTorch ops), "fused" (csrc/flow_head.hip) or None = the process default at call time (set_flow_head)."""
        super().__init__()
        self.W, self.flow_model, self.n_frames, self.num_basis = W, flow_model, n_frames, num_basis
        if flow_model == "offset":
            self.gaussian_warp = PointLinear(W, 3)
        elif flow_model in ("se3", "se3Affine", "se3Scaled"):
            self.branch_w = PointLinear(W, 3)
            self.branch_v = PointLinear(W, 3)
            if flow_model == "se3Scaled":
                self.branch_scale = PointLinear(W, 1)
            if flow_model != "se3":
                self.branch_offset = PointLinear(W, 3)
        elif flow_model == "affine":
            self.branch_w = PointLinear(W, 9)
            self.branch_v = PointLinear(W, 3)
        elif flow_model in ("dct", "dct_siren"):
            self.branch_coeff = PointLinear(W, 3 * num_basis)
            nn.init.zeros_(self.branch_coeff.weight)
            nn.init.zeros_(self.branch_coeff.bias)
            if flow_model == "dct":
                self.trajectory_basis = nn.Parameter(dct_basis(num_basis, n_frames * 2))
            else:
                self.basis_net = SirenMLP(in_features=1, out_features=num_basis, hidden_features=128, num_hidden_layers=2)
        else:
            raise NotImplementedError(f"flow_model={flow_model!r}: expected one of {FLOW_MODELS}")
        from .flow_head import checked_flow_head, fused_shape_error, resolve_flow_head
        self.path = None if path is None else checked_flow_head(path)
        if resolve_flow_head(self.path) == "fused" and fused_shape_error(flow_model, W, num_basis):    # asked for here, or the process default
            raise ValueError("FlowHead on the fused path: " + fused_shape_error(flow_model, W, num_basis))

    def branches(self):
        """the branch linears in the order of the fused kernel's z layout (include/splatraster.h: sr_flow_head_forward)"""
        names = {"offset": ("gaussian_warp",), "se3": ("branch_w", "branch_v"), "se3Affine": ("branch_w", "branch_v", "branch_offset"),
                 "se3Scaled": ("branch_w", "branch_v", "branch_scale", "branch_offset"), "affine": ("branch_w", "branch_v"),
                 "dct": ("branch_coeff",), "dct_siren": ("branch_coeff",)}[self.flow_model]
        return [getattr(self, n) for n in names]

    def _bases(self, time_step, frame_id):
        """bases [K] of the fused path: a row of `trajectory_basis`, or the SIREN evaluated in float64 (one point, 17 k
        multiply-adds: the kernels compute in double, and sin(30 x) in float32 would be the largest error of the head)"""
        if self.flow_model == "dct":
            return self.trajectory_basis[frame_id.long() if torch.is_tensor(frame_id) else int(frame_id)]
        with torch.autocast(time_step.device.type, enabled=False):
            x = time_step.view(1, 1).double()
            layers = list(self.basis_net.net)
            for lin in layers[:-1]:
                x = torch.sin(30 * F.linear(x, lin.weight.double(), lin.bias.double()))
            return F.linear(x, layers[-1].weight.double(), layers[-1].bias.double()).view(-1)

    def forward(self, hidden, pts, time_step=None, frame_id=None):
        from .flow_head import fused_flow_head, resolve_flow_head
        if resolve_flow_head(self.path) == "fused":
            bases = self._bases(time_step, frame_id) if self.flow_model in ("dct", "dct_siren") else None
            lins = self.branches()
            return fused_flow_head(self.flow_model, hidden, pts, [l.weight for l in lins], [l.bias for l in lins], bases)
        if self.flow_model == "offset":
            flow = self.gaussian_warp(hidden)
            return flow, pts + flow
        if self.flow_model == "se3":
            w, v = self.branch_w(hidden), self.branch_v(hidden)
            theta = torch.norm(w, dim=-1, keepdim=True)
            w = w / theta + 1e-5
            v = v / theta + 1e-5
            flow = se3_transform(w, v, theta)
            means3D = (flow[:, :3, :3] * pts[:, None, :]).sum(-1) + flow[:, :3, 3]
            return flow, means3D
        if self.flow_model in ("se3Affine", "se3Scaled"):
            w, v = self.branch_w(hidden), self.branch_v(hidden)
            theta = torch.norm(w, dim=-1, keepdim=True)
            w = w / theta + 1e-5
            v = v / theta + 1e-5
            R, p = _se3_parts(w, v, theta)
            if self.flow_model == "se3Scaled":      # the rotation block is scaled, the translation is not
                R = F.softplus(self.branch_scale(hidden))[:, :, None] * R
            means3D = (R * pts[:, None, :]).sum(-1) + p + self.branch_offset(hidden)
            return means3D - pts, means3D
        if self.flow_model == "affine":
            A = self.branch_w(hidden).view(-1, 3, 3)
            means3D = (A * pts[:, None, :]).sum(-1) + self.branch_v(hidden)
            return means3D - pts, means3D
        coeff = self.branch_coeff(hidden).view(-1, 3, self.num_basis)
        if self.flow_model == "dct":
            bases = self.trajectory_basis[frame_id.long() if torch.is_tensor(frame_id) else int(frame_id)]
        else:
            bases = self.basis_net(time_step.view(1, 1))
        flow = (coeff * bases.view(1, 1, -1)).sum(-1)
        return flow, pts + flow


class ViewColor:
    """`out["rgb_fnc"]` of a view-dependent network: the reference's `lambda viewdir: mlp_rgb_viewdep(cat([rgb, viewdir]))`
    (utils/time_utils.py:496) as an object that can also evaluate every view of a step at once.

    fnc(viewdir [N, 3]) -> [N, 3]: the reference's call.  `path == "torch"`: the same PyTorch ops; "fused": the kernels of
    csrc/view_color.hip with the directions as given (splatfields_amd/view_color.py).
    fnc.for_cameras(means3D [N, 3], camera_centers [V, 3]) -> [V, N, 3]: what reference gaussian_renderer/__init__.py:44-46
    computes per view -- "torch": a loop over those expressions; "fused": one launch for all views."""

    def __init__(self, head: nn.Sequential, feature: torch.Tensor, path: str):
        self.head, self.feature, self.path = head, feature, path

    def __call__(self, viewdir):
        if self.path == "fused":
            from .view_color import fused_view_color
            return fused_view_color(self.feature, self.head[0].weight, self.head[0].bias, dirs=viewdir[None])[0]
        return self.head(torch.cat([self.feature, viewdir], dim=-1))

    def for_cameras(self, means3D, camera_centers):
        if self.path == "fused":
            from .view_color import fused_view_color
            return fused_view_color(self.feature, self.head[0].weight, self.head[0].bias, means3D=means3D, camera_centers=camera_centers)
        colours = []
        for centre in camera_centers:
            ray_d = means3D - centre[None]
            ray_d = ray_d / torch.norm(ray_d, dim=-1, keepdim=True)
            colours.append(self(ray_d))
        return torch.stack(colours)


class SplatFields(nn.Module):
    def __init__(self, radius=None, n_frames: int = 0, encoder: Optional[nn.Module] = None, mlp_precision: Optional[str] = None, **kwargs):
        """`mlp_precision`: "fp32", "bf16", "bf16x3" or None (the process default, splatfields_amd.set_mlp_precision) for the fused layer
        chains of every GeneralMLP built here.  `flow_head="torch" | "fused"` (a keyword, so it also arrives through
        `SplatFieldsModel`'s hyper_args): the path of the flow head, None = the process default (splatfields_amd.set_flow_head).
        `view_color="torch" | "fused"`, likewise: the path of the view-dependent colour head of `use_view_dep_rgb`
        (splatfields_amd.set_view_color).  `heads="separate" | "grouped"`, likewise: how the step runs the networks behind
        `mlp_deform` -- scale, opacity, rotation, rgb, flow, which all read (xyz_can, features, time).  "grouped" runs them through one
        autograd function, the networks of one width in one launch per phase (splatfields_amd.set_heads; general_mlp.HeadGroup).  A
        call whose inputs the grouped input kernel cannot take -- tensors that are not float32 on the device, a `t` that needs a
        gradient or is not one value per point (the branch that builds the time embedding with PyTorch ops), no points -- runs the
        separate path."""
        super().__init__()
        rank = kwargs.get("composition_rank", 0)
        self.n_frames = n_frames
        self.encoder_type = kwargs.get("encoder_type", "VarTriPlaneEncoder")
        if encoder is None and self.encoder_type in ["VarTriPlaneEncoder"] and (kwargs.get("encoder_args") or {}).get("generator") == "decoder":
            # opt-in: the reference's encoder with its plane generator (splatfields_amd/plane_generator.py), configured as the
            # reference does it (utils/time_utils.py:316-328)
            from .plane_generator import VarTriPlaneEncoder
            ea = kwargs["encoder_args"]
            unknown = sorted(k for k in ea if k not in ("generator", "in_ch", "out_ch", "noise_res", "fuse_mode", "attention"))
            if unknown:
                raise ValueError("SplatFields: encoder_args %s are not arguments of the plane generator (in_ch, out_ch, noise_res, fuse_mode, attention)" % unknown)
            encoder = VarTriPlaneEncoder({**{k: v for k, v in ea.items() if k != "generator"},
                                          "layer_kwargs": {"n_frames": n_frames, "strategy": kwargs.get("layer_strategy", "none")}})
        if encoder is None and self.encoder_type in ["VarTriPlaneEncoder"]:
            from .triplane import TriPlaneSampler
            ea = kwargs.get("encoder_args", {}) or {}
            ignored = sorted(k for k in ea if k not in ("out_ch", "noise_res", "fuse_mode", "plane_source"))
            if ignored:
                import warnings
                warnings.warn("SplatFields: encoder_args %s configure the reference's plane GENERATOR (scene/tripFields.py:176-204), which "
                              "is not part of this package -- they are ignored by the decoder-free TriPlaneSampler; pass the generator as "
                              "encoder_args['plane_source'] or a whole encoder as encoder=" % ignored, stacklevel=2)
            encoder = TriPlaneSampler(out_ch=ea.get("out_ch", 16), resolution=16 * ea.get("noise_res", 20),
                                      fuse_mode=ea.get("fuse_mode", "cat"), plane_source=ea.get("plane_source"))
        if encoder is not None:
            self.encoder = encoder
            self.feat_dim = int(encoder.out_dim)
            self.mlp_refine_feat = nn.Sequential(PointLinear(self.feat_dim, self.feat_dim), nn.ReLU(), PointLinear(self.feat_dim, self.feat_dim))
        else:
            self.feat_dim = 0
        if n_frames > 0:
            self.time_multires = kwargs.get("time_multires", 3)
            time_ch = 1 + 2 * self.time_multires
        else:
            self.time_multires, time_ch = 0, 0
        self.deform_weight = kwargs.get("deform_weight", 1.0)
        in_ch = 3 + self.feat_dim + time_ch

        def mlp(prefix, out, w, d, skips, multires, out_act, in_features=in_ch):
            return GeneralMLP(in_features=in_features, out_features=out, hidden_features=kwargs.get(prefix + "_w", w),
                              num_hidden_layers=kwargs.get(prefix + "_d", d), skips=kwargs.get(prefix + "_skips", skips),
                              multires=multires, out_activation=out_act, act="leaky_relu", composition_rank=rank, n_frames=n_frames,
                              precision=mlp_precision)

        self.mlp_deform = mlp("deform", 3, 128, 6, [3], kwargs.get("deform_multires", 6), "none")
        self.use_view_dep_rgb = kwargs.get("use_view_dep_rgb", False)
        self.mlp_rgb = mlp("rgb", kwargs.get("rgb_w", 128) if self.use_view_dep_rgb else 3, 128, 6, [3], kwargs.get("rgb_multires", 6),
                           "none" if self.use_view_dep_rgb else "sigmoid")
        if self.use_view_dep_rgb:
            self.mlp_rgb_viewdep = nn.Sequential(nn.Linear(3 + self.mlp_rgb.out_features, 3), nn.Sigmoid())
        from . import _lib
        from .view_color import checked_view_color, resolve_view_color
        self.view_color = None if kwargs.get("view_color") is None else checked_view_color(kwargs["view_color"])
        if self.use_view_dep_rgb and resolve_view_color(self.view_color) == "fused":      # asked for here, or the process default
            why = _lib.view_color_shape_error(self.mlp_rgb.out_features, 1)
            if why:
                raise ValueError("SplatFields: the fused view-colour head cannot run this network: " + why)
        self.geo_model_disable_pts = bool(kwargs.get("geo_model_disable_pts", False))
        geo_in = in_ch - (3 if self.geo_model_disable_pts else 0)
        off = self.geo_model_disable_pts
        self.mlp_scale = mlp("scale", 3, 64, 4, [2], 0 if off else kwargs.get("scale_multires", 4), "none", geo_in)
        self.mlp_opacity = mlp("opacity", 1, 64, 4, [2], 0 if off else kwargs.get("opacity_multires", 3), "sigmoid", geo_in)
        self.mlp_rotation = mlp("rotation", 4, 64, 3, [20], 0 if off else kwargs.get("rotation_multires", 3), "normalize", geo_in)
        if n_frames > 0:
            self.mlp_flow = mlp("flow", kwargs.get("flow_w", 128), 128, 6, [3], kwargs.get("flow_multires", 6), "none")
            self.mlp_flow_head = FlowHead(W=self.mlp_flow.out_features, flow_model=kwargs.get("flow_model", "se3"),
                                          num_basis=kwargs.get("dct_basis", 4), n_frames=n_frames, path=kwargs.get("flow_head"))

        from .fused_mlp import _checked_heads, resolve_heads
        self.heads = None if kwargs.get("heads") is None else _checked_heads(kwargs["heads"])
        self._head_group = None
        if resolve_heads(self.heads) == "grouped":      # asked for here, or the process default: refuse now what can never run grouped
            self._head_group = self._make_head_group()

    def _make_head_group(self):
        from .general_mlp import HeadGroup
        if self.geo_model_disable_pts:
            raise ValueError("SplatFields: heads='grouped' cannot run with geo_model_disable_pts=True (the geometry heads then read "
                             "other inputs than the colour and flow heads)")
        named = [("scales", self.mlp_scale), ("opacity", self.mlp_opacity), ("rotations", self.mlp_rotation), ("rgb", self.mlp_rgb)]
        if self.n_frames > 0:
            named.append(("flow", self.mlp_flow))
        return HeadGroup(named, self.time_multires)

    def load_state_dict(self, state_dict, strict: bool = True, assign: bool = False):
        """`nn.Module.load_state_dict`, plus one loud check: a reference default-config checkpoint holds the weights of its
        time-conditioned plane generators (`encoder.subs.*`, scene/tripFields.py:383-428).  The decoder-free sampler has no place
        for them, and silently training its own free planes instead would be a different model."""
        gen_keys = [k for k in state_dict if k.startswith("encoder.subs.")]
        own = getattr(self, "encoder", None)
        if gen_keys and own is not None and not any(k.startswith("encoder.subs.") for k in self.state_dict()):
            raise RuntimeError(
                "this checkpoint carries the reference's tri-plane GENERATOR (%d `encoder.subs.*` tensors, e.g. %r), but this SplatFields "
                "was built with the decoder-free TriPlaneSampler (planes are a free parameter, they ignore frame_id).  Build it with the "
                "reference's encoder -- SplatFields(encoder=<VarTriPlaneEncoder instance>) or encoder_args['plane_source'] -- to load it."
                % (len(gen_keys), gen_keys[0]))
        return super().load_state_dict(state_dict, strict=strict, assign=assign)

    def _time2frame_id(self, t):
        return torch.round(t * (self.n_frames - 1))

    def _encode(self, x, frame_id):
        """encoder features [N, feat_dim]; an encoder that generates its planes (plane_generator.VarTriPlaneEncoder) is told the
        frame: its per-frame convolution weights are the time conditioning of the planes"""
        if getattr(self.encoder, "takes_frame_id", False):
            return self.encoder(x[None], frame_id=frame_id).squeeze(0)
        return self.encoder(x[None]).squeeze(0)

    def extract_features(self, x, t):
        t_feat = positional_encoding(t, self.time_multires) if self.n_frames > 0 else None
        frame_id = self._time2frame_id(t.view(-1)[0]).long() if self.n_frames > 0 and torch.is_tensor(t) else None
        x_feat = self.mlp_refine_feat(self._encode(x, frame_id)) if self.feat_dim > 0 else None
        parts = [f for f in (x_feat, t_feat) if f is not None]
        return torch.cat(parts, dim=-1) if parts else None

    def _fuse_time(self, xyz_in, t) -> bool:
        return self.n_frames > 0 and torch.is_tensor(t) and t.is_cuda and t.dtype == torch.float32 and not t.requires_grad and \
            t.numel() == xyz_in.shape[0] and not self.geo_model_disable_pts

    def forward(self, xyz_in, t):
        out = {}
        time_step, frame_id = None, None
        if self.n_frames > 0:
            time_step = t.view(-1)[0]
            frame_id = self._time2frame_id(time_step).long()
        # features of every network: [refined tri-plane features | time embedding] (extract_features).  With one float32 time per
        # point that takes no gradient, the time embedding is written by the networks' input kernel instead of ~15 small kernels
        # and a concatenation per step.
        fuse_time = self._fuse_time(xyz_in, t)
        if fuse_time:
            feat = self.mlp_refine_feat(self._encode(xyz_in, frame_id)) if self.feat_dim > 0 else None
            tk = dict(time=t.reshape(-1), time_multires=self.time_multires)
        else:
            feat, tk = self.extract_features(xyz_in, t), {}
        if self.deform_weight > 0:
            xyz_can = torch.add(xyz_in, self.mlp_deform(xyz_in, feat, frame_id=frame_id, **tk), alpha=self.deform_weight)   # one kernel
        else:
            xyz_can = xyz_in
        from .fused_mlp import grouped_inputs_ok, resolve_heads
        grouped = None
        if resolve_heads(self.heads) == "grouped" and (fuse_time or self.n_frames == 0) and grouped_inputs_ok(xyz_can, feat, tk.get("time")):
            if self._head_group is None:       # the process default changed after construction
                self._head_group = self._make_head_group()
            grouped = self._head_group(xyz_can, feat, frame_id=frame_id, time=tk.get("time"))
        if grouped is not None:
            out["scales"], out["opacity"], out["rotations"], rgb = grouped["scales"], grouped["opacity"], grouped["rotations"], grouped["rgb"]
        else:
            geo_xyz, geo_feat = (feat, None) if self.geo_model_disable_pts else (xyz_can, feat)
            out["scales"] = self.mlp_scale(geo_xyz, geo_feat, frame_id=frame_id, **tk)
            out["opacity"] = self.mlp_opacity(geo_xyz, geo_feat, frame_id=frame_id, **tk)
            out["rotations"] = self.mlp_rotation(geo_xyz, geo_feat, frame_id=frame_id, **tk)
            rgb = self.mlp_rgb(xyz_can, feat, frame_id=frame_id, **tk)
        if self.use_view_dep_rgb:
            from .view_color import resolve_view_color
            out["rgb_fnc"] = ViewColor(self.mlp_rgb_viewdep, rgb, resolve_view_color(self.view_color))
        else:
            out["rgb"] = rgb
        if self.n_frames > 0:
            flow_feat = grouped["flow"] if grouped is not None else self.mlp_flow(xyz_can, feat, frame_id=frame_id, **tk)
            flow, means3D = self.mlp_flow_head(hidden=flow_feat, pts=xyz_can, time_step=time_step, frame_id=frame_id)
        else:
            flow, means3D = None, xyz_can
        out.update({"flow": flow, "means3D": means3D})
        return out


def expon_lr(step: int, lr_init: float, lr_final: float, lr_delay_steps: int = 0, lr_delay_mult: float = 1.0, max_steps: int = 1000000) -> float:
    """the reference's schedule (utils/general_utils.py:86-119): log-linear from lr_init to lr_final over max_steps, optionally
    eased in by lr_delay_mult + (1 - lr_delay_mult) sin(pi/2 clip(step / lr_delay_steps)); 0 for step < 0 or when both rates are 0."""
    if step < 0 or (lr_init == 0.0 and lr_final == 0.0):
        return 0.0
    delay = 1.0
    if lr_delay_steps > 0:
        delay = lr_delay_mult + (1.0 - lr_delay_mult) * math.sin(0.5 * math.pi * min(max(step / lr_delay_steps, 0.0), 1.0))
    t = min(max(step / max_steps, 0.0), 1.0)
    return delay * math.exp(math.log(lr_init) * (1.0 - t) + math.log(lr_final) * t)


class SplatFieldsModel:
    """Counterpart of reference scene/deform_model.py:9-54 around `SplatFields`: `step(xyz, time_emb)`, Adam over all network
    parameters at 5 x the position learning rate with the exponential schedule, `deform/iteration_<n>/deform.pth` checkpoints."""

    def __init__(self, hyper_args, radius=None, encoder: Optional[nn.Module] = None, device="cuda"):
        kwargs = dict(hyper_args.__dict__) if hasattr(hyper_args, "__dict__") else dict(hyper_args)
        self.deform = SplatFields(radius=radius, encoder=encoder, **kwargs).to(device)
        self.optimizer = None
        self.spatial_lr_scale = 5

    def step(self, xyz, time_emb):
        return self.deform(xyz, time_emb)

    def train_setting(self, training_args, optimizer: Optional[str] = None):
        """`optimizer`: "torch" (torch.optim.Adam, as the reference), "fused" (splatfields_amd.NetworkAdam: the same step in one
        launch per 480 tensors) or None = the process default at call time (set_network_optimizer, SPLATFIELDS_NETWORK_OPTIMIZER)."""
        from .network_optim import NetworkAdam, resolve_network_optimizer
        make = NetworkAdam if resolve_network_optimizer(optimizer) == "fused" else torch.optim.Adam
        lr0 = training_args.position_lr_init * self.spatial_lr_scale
        self.optimizer = make([{"params": list(self.deform.parameters()), "lr": lr0, "name": "deform"}], lr=0.0, eps=1e-15)
        self._schedule = dict(lr_init=lr0, lr_final=training_args.position_lr_final, lr_delay_mult=training_args.position_lr_delay_mult,
                              max_steps=training_args.deform_lr_max_steps)

    def update_learning_rate(self, iteration):
        for group in self.optimizer.param_groups:
            if group["name"] == "deform":
                group["lr"] = expon_lr(iteration, **self._schedule)
                return group["lr"]

    def save_weights(self, model_path, iteration):
        import os
        out = os.path.join(model_path, "deform/iteration_{}".format(iteration))
        os.makedirs(out, exist_ok=True)
        torch.save(self.deform.state_dict(), os.path.join(out, "deform.pth"))

    def load_weights(self, model_path, iteration=-1):
        import os
        if iteration == -1:
            iteration = max(int(name.split("_")[-1]) for name in os.listdir(os.path.join(model_path, "deform")))
        self.deform.load_state_dict(torch.load(os.path.join(model_path, "deform/iteration_{}/deform.pth".format(iteration))))
