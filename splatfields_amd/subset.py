"""Subset steps: the reference's ``--n_splats`` (train.py:56-60, :68, :281-286; scene/gaussian_model.py:431-438) on the device.

The reference draws ``torch.randperm(N)[:n_splats]`` on the host every iteration, indexes ``xyz``, ``scaling`` and the features
with it and writes the densification statistics back through it with clone / mask / assign sequences.  Here

  `draw_rows`          n distinct rows of [0, N) from a keyed bijection evaluated per output (csrc/subset.hip): cost and memory scale
                       with n, not with N (``order="draw"``), or one bit per row (``order="ascending"``); nothing waits;
  `gather_rows`        every tensor of the step through the row list in ONE launch, with the activations of
                       scene/gaussian_model.py:64-68 and the concatenation of :79-82 folded in; its backward is one launch too;
  `get_gaussian_dict`  the reference's function (train.py:36-101) on top of the two;
  `densification_stats(..., idx=)` (densify_stats.py) the scatter of the statistics.

There is no CPU path: a missing library or a CPU device is an error."""
from __future__ import annotations

import ctypes as C
from typing import Optional

import torch

from . import _lib
from ._lib import ptr

ROUNDS = 8                      # Feistel rounds = keys per draw
_MASK64 = (1 << 64) - 1
_OPS = {"copy": _lib.ROWS_COPY, "exp": _lib.ROWS_EXP, "exp3": _lib.ROWS_EXP_TO3}


def _splitmix64(seed: int, n: int) -> list:
    out, s = [], seed & _MASK64
    for _ in range(n):
        s = (s + 0x9E3779B97F4A7C15) & _MASK64
        z = s
        z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & _MASK64
        z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & _MASK64
        out.append(z ^ (z >> 31))
    return out


def _seed_of(seed, generator) -> int:
    if seed is not None:
        return int(seed) & _MASK64
    if generator is not None and generator.device.type != "cpu":
        raise ValueError("draw_rows takes its seed from a CPU generator (a device generator would make the host wait): pass seed=")
    hi, lo = torch.randint(0, 2 ** 32, (2,), generator=generator, dtype=torch.int64).tolist()    # torch's default CPU generator for None
    return (hi << 32) | lo


def draw_rows(n_rows: int, n_pick: int, *, seed: Optional[int] = None, generator: Optional[torch.Generator] = None, order: str = "draw",
              device=None, return_flag: bool = False):
    """``n_pick`` distinct rows of ``[0, n_rows)``: int64 [n_pick] on the device, a uniform subset -- in random order
    (``order="draw"``: one launch, no memory besides the result) or sorted (``order="ascending"``: three launches and a workspace
    of one bit per row; coalescing gathers, and a result that does not depend on the draw order).

    seed: 64 bits; None takes them from ``generator``, a CPU generator (None: torch's default one, so ``torch.manual_seed``
    governs the draw).  The same (seed, n_rows, n_pick, order) gives the same rows on every call and every machine: the rows are a
    function of these alone (include/splatraster.h: sr_draw_rows; tests/subset_reference.py restates it in numpy).  Nothing
    waits for the device.  return_flag: also an int32 [1] device tensor, 1 iff a lane gave up its walk (never, for a correct map)."""
    if order not in ("draw", "ascending"):
        raise ValueError(f"order must be 'draw' or 'ascending', not {order!r}")
    n_rows, n_pick = int(n_rows), int(n_pick)
    if not 0 <= n_rows <= 2 ** 31 - 1 or not 0 <= n_pick <= n_rows:
        raise ValueError("draw_rows needs 0 <= n_pick <= n_rows <= 2^31 - 1")
    dev = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
    if dev.type != "cuda":
        raise RuntimeError("draw_rows has no CPU path: the device must be a HIP ('cuda') device")
    lib = _lib.load()
    keys = (C.c_ulonglong * ROUNDS)(*_splitmix64(_seed_of(seed, generator), ROUNDS))
    with torch.cuda.device(dev):
        idx = torch.empty(n_pick, dtype=torch.int64, device=dev)
        flag = torch.zeros(1, dtype=torch.int32, device=dev) if return_flag else None
        if order == "draw":
            _lib.check(lib.sr_draw_rows(n_rows, n_pick, keys, ROUNDS, ptr(idx), ptr(flag), _lib.stream(dev)))
        else:
            ws = torch.empty(lib.sr_draw_rows_ascending_workspace_bytes(n_rows), dtype=torch.uint8, device=dev)
            _lib.check(lib.sr_draw_rows_ascending(n_rows, n_pick, keys, ROUNDS, ptr(ws), ptr(idx), ptr(flag), _lib.stream(dev)))
    return (idx, flag) if return_flag else idx


def _row_floats(shape) -> int:
    n = 1
    for d in shape[1:]:
        n *= int(d)
    return n


def _job_table(spec, src_shapes, src_ptrs, outs):
    """spec: per source (entry, op, first column inside the entry's row) -> the SrRowsJob array; outs: the result per entry"""
    jobs = (_lib.SrRowsJob * len(spec))()
    for k, (entry, op, col) in enumerate(spec):
        jobs[k].src, jobs[k].dst = src_ptrs[k], outs[entry].data_ptr()
        jobs[k].row_floats, jobs[k].op = _row_floats(src_shapes[k]), op
        jobs[k].dst_row_stride, jobs[k].dst_col_offset = _row_floats(outs[entry].shape), col
    return jobs


class _GatherRows(torch.autograd.Function):
    @staticmethod
    def forward(ctx, idx, spec, shapes, flag, *sources):
        lib = _lib.load()
        dev, n = idx.device, idx.numel()
        srcs = [_lib.f32c(s) for s in sources]
        n_rows = srcs[0].shape[0]
        outs = [torch.empty((n,) + tuple(s), dtype=torch.float32, device=dev) for s in shapes]
        jobs = _job_table(spec, [s.shape for s in srcs], [s.data_ptr() for s in srcs], outs)
        with torch.cuda.device(dev):
            _lib.check(lib.sr_rows_gather(len(spec), jobs, n, ptr(idx), n_rows, ptr(flag), _lib.stream(dev)))
        ctx.spec, ctx.n_rows, ctx.src_shapes = spec, n_rows, [tuple(s.shape) for s in srcs]
        ctx.save_for_backward(idx, *outs)                                    # the EXP jobs read their own output back
        live = {entry for j, (entry, _, _) in enumerate(spec) if ctx.needs_input_grad[4 + j]}
        ctx.mark_non_differentiable(*(o for e, o in enumerate(outs) if e not in live))   # a detached input gives a detached result
        return tuple(outs)

    @staticmethod
    def backward(ctx, *grads):
        lib = _lib.load()
        idx, *outs = ctx.saved_tensors
        dev, n, k = idx.device, idx.numel(), len(ctx.spec)
        gs = [None if g is None else _lib.f32c(g) for g in grads]
        d_src = [torch.zeros(shape, dtype=torch.float32, device=dev) if ctx.needs_input_grad[4 + j] and gs[ctx.spec[j][0]] is not None
                 else None for j, shape in enumerate(ctx.src_shapes)]
        if n and any(d is not None for d in d_src):
            jobs = _job_table(ctx.spec, ctx.src_shapes, [None] * k, outs)    # the scatter does not read job.src
            g_ptrs = (C.c_void_p * k)(*[None if gs[e] is None else gs[e].data_ptr() for e, _, _ in ctx.spec])
            d_ptrs = (C.c_void_p * k)(*[None if d is None else d.data_ptr() for d in d_src])
            with torch.cuda.device(dev):
                _lib.check(lib.sr_rows_scatter(k, jobs, g_ptrs, d_ptrs, n, ptr(idx), ctx.n_rows, None, _lib.stream(dev)))
        return (None, None, None, None, *d_src)


def gather_rows(idx: torch.Tensor, *tensors, ops=None, return_flag: bool = False):
    """Rows ``idx`` of every tensor, in one launch: a tuple with one float32 result per entry of ``tensors``.

    An entry is a tensor [N, ...], or a tuple of tensors whose rows are written side by side into ONE result, as ``torch.cat(...,
    dim=1)[idx]`` would give (``(_features_dc, _features_rest)`` -> [n, 16, 3], scene/gaussian_model.py:79-82 without the cat).
    ops: per entry "copy" (default), "exp" (``torch.exp(t)[idx]``) or "exp3" (t is [N,1]: ``torch.exp(t).repeat(1, 3)[idx]``, the
    isotropic scaling of scene/gaussian_model.py:66-67).  Gradients go to every input that requires one: a zero fill per such tensor
    and one launch.  PRECONDITION of the backward: the rows of ``idx`` are distinct, as `draw_rows` makes them -- there are no
    atomics, and with a repeated row one of its writers wins.  A row outside [0, N) gives NaN and (return_flag) sets the int32 [1]
    device flag that is then appended to the result; nothing is read back."""
    if not tensors:
        raise ValueError("gather_rows needs at least one tensor")
    ops = ["copy"] * len(tensors) if ops is None else list(ops)
    if len(ops) != len(tensors) or any(o not in _OPS for o in ops):
        raise ValueError("ops must name 'copy', 'exp' or 'exp3' for every entry")
    spec, shapes, sources = [], [], []
    for e, (entry, op) in enumerate(zip(tensors, ops)):
        parts = list(entry) if isinstance(entry, (tuple, list)) else [entry]
        col = 0
        for t in parts:
            if not torch.is_tensor(t) or not t.is_cuda or t.dim() < 1:
                raise RuntimeError("gather_rows has no CPU path: every tensor must be [N, ...] on a HIP ('cuda') device")
            row = int(torch.Size(t.shape[1:]).numel())
            if op == "exp3" and row != 1:
                raise ValueError("'exp3' reads rows of one float")
            spec.append((e, _OPS[op], col))
            sources.append(t)
            col += 3 * row if op == "exp3" else row
        if len(parts) == 1:
            shapes.append((3,) if op == "exp3" else tuple(parts[0].shape[1:]))
        else:
            if any(p.dim() < 2 or p.shape[2:] != parts[0].shape[2:] for p in parts) or op == "exp3":
                raise ValueError("the tensors of a tuple are concatenated along dim 1: the other dims must agree")
            shapes.append((sum(p.shape[1] for p in parts),) + tuple(parts[0].shape[2:]))
    if len(sources) > _lib.ROWS_MAX_JOBS:
        raise ValueError(f"at most {_lib.ROWS_MAX_JOBS} tensors per call")
    if any(s.shape[0] != sources[0].shape[0] or s.device != sources[0].device for s in sources):
        raise ValueError("every tensor must have the same number of rows, on one device")
    idx = idx.detach().to(sources[0].device, torch.int64).contiguous()
    flag = torch.zeros(1, dtype=torch.int32, device=idx.device) if return_flag else None
    out = _GatherRows.apply(idx, tuple(spec), tuple(shapes), flag, *sources)
    return out + (flag,) if return_flag else out


def get_gaussian_dict(viewpoint_cam, gaussians, deform, iteration=None, warm_up=None, static=False, n_splats=-1, *,
                      seed: Optional[int] = None, generator: Optional[torch.Generator] = None, order: str = "ascending"):
    """The reference's ``get_gaussian_dict`` (train.py:36-101) -> ``(gaussian_dict, overwrite_attributes)``, for any object with
    the reference ``GaussianModel``'s attributes (``_xyz``, ``_scaling``, ``_features_dc``, ``_features_rest``, ``use_isotropic``,
    ``active_sh_degree`` and the ``get_*`` accessors): the same keys, the same branches (static / warm-up; ``gaussian_features`` of
    the network times 0.1 plus the stored ones; ``rgb``; ``rgb_fnc``; ``gradient_error``) and the same condition ``0 < n_splats < N``
    for the subset.  The subset is drawn on the device (`draw_rows`: seed / generator / order as there) and gathered with one
    launch (`gather_rows`): the activation of the scaling and the concatenation of the features are applied to the drawn rows only.
    ``gaussian_dict['idx']`` is the device tensor, or None.  ``overwrite_attributes['f_dc' / 'f_rest']`` are the stored tensors
    themselves, which is what the reference's split of its concatenation holds."""
    xyz_all = gaussians.get_xyz
    fid = viewpoint_cam.fid.to(xyz_all.device)
    if static:
        fid = 0 * fid
    if static or (iteration is not None and warm_up is not None and iteration < warm_up):
        return {"means3D": xyz_all, "active_sh_degree": gaussians.active_sh_degree, "gaussian_opacity": gaussians.get_opacity,
                "gaussian_features": gaussians.get_features, "gaussian_scales": gaussians.get_scaling,
                "gaussian_rotations": gaussians.get_rotation}, None
    n_all = xyz_all.shape[0]
    if 0 < n_splats < n_all:
        idx = draw_rows(n_all, n_splats, seed=seed, generator=generator, order=order, device=xyz_all.device)
        xyz, scaling, features = gather_rows(idx, gaussians._xyz.detach(), gaussians._scaling.detach(),
                                             (gaussians._features_dc, gaussians._features_rest),
                                             ops=("copy", "exp3" if gaussians.use_isotropic else "exp", "copy"))
    else:
        idx = None
        xyz, scaling, features = xyz_all.detach(), gaussians.get_scaling.detach(), gaussians.get_features
    ret = deform.step(xyz, fid.detach().unsqueeze(0).expand(xyz.shape[0], -1))
    d = {"idx": idx, "means3D": ret["means3D"], "active_sh_degree": gaussians.active_sh_degree, "gaussian_opacity": ret["opacity"],
         "gaussian_scales": ret["scales"] + scaling, "gaussian_rotations": ret["rotations"],
         "gradient_error": ret.get("gradient_error", None)}
    if "gaussian_features" in ret:
        d["gaussian_features"] = ret["gaussian_features"].view(features.shape) * 0.1 + features
    elif "rgb" in ret:
        d["gaussian_rgb"] = ret["rgb"]
    elif "rgb_fnc" in ret:
        d["gaussian_rgb_fnc"] = ret["rgb_fnc"]
    else:
        d["gaussian_features"] = features
    over = {"xyz": d["means3D"], "f_dc": gaussians._features_dc, "f_rest": gaussians._features_rest, "opacity": d["gaussian_opacity"],
            "scaling": ret["scales"], "rotation": d["gaussian_rotations"]}
    return d, over
