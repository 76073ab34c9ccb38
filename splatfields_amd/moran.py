"""Moran's I regulariser on the device: the reference's ``query_nn`` / ``morans_measure`` / ``morans_loss``
(extract_geo.py:100-143) as drop-ins, and lines 203-215 of its train.py as one fused call.

The reference writes, per view,

    weights, nn_ix = query_nn(means3D)                      # pytorch3d.ops.knn.knn_points + cdist of the gathered points
    loss += lambda_corr * morans_loss(weights, scales[nn_ix]) ...            # four terms, [N, F, K, K] temporaries each

``moran_loss`` is the k-nearest-neighbour graph (``sr_knn_graph``), one kernel and a fixed-order reduction forward
(``sr_moran_forward``) and two kernels backward (``sr_moran_backward``: per-edge contributions, then their sum per row in a
fixed order): nothing of size N F K^2 exists, no host synchronisation, no floating-point atomics, bit-identical results from
call to call.  The loss does not depend on the view: evaluate it once per step, not once per rendered view.  There is no
CPU path."""
from __future__ import annotations

import ctypes as C
from typing import NamedTuple, Optional, Sequence

import torch

from . import _lib
from ._lib import f32c, ptr

MAX_NEIGHBORS = _lib.KNN_MAX_K
MAX_TENSORS = _lib.MORAN_MAX_TENSORS


def _pointer_array(tensors):
    return (C.c_void_p * len(tensors))(*[None if t is None else t.data_ptr() for t in tensors])


class KnnGraph(NamedTuple):
    """The K nearest points of every point (itself included, nearest first) and what the kernels walk it with."""
    nn_ix: torch.Tensor       # [N, K] int32
    order: torch.Tensor       # [N] int32: the points in grid-cell order
    rev_start: torch.Tensor   # [N + 1] int32: per point, where its incoming edges start in rev_edges
    rev_edges: torch.Tensor   # [N K] int32: edge ids p * K + slot, ascending per point


def _check_points(name, points, n_neighbors):
    if not isinstance(points, torch.Tensor) or points.dim() != 2 or points.shape[1] != 3 or not points.is_floating_point():
        raise RuntimeError(f"{name}: points must be a floating-point [N, 3] tensor")
    if not points.is_cuda:
        raise RuntimeError(f"{name} has no CPU path: tensors must be on a HIP ('cuda') device")
    if not 2 <= int(n_neighbors) <= MAX_NEIGHBORS:
        raise ValueError(f"{name}: n_neighbors must be 2 .. {MAX_NEIGHBORS}, got {n_neighbors}")
    if points.shape[0] < int(n_neighbors):
        raise RuntimeError(f"{name}: {points.shape[0]} points are fewer than n_neighbors = {n_neighbors}")


def knn_graph(points: torch.Tensor, n_neighbors: int = 5) -> KnnGraph:
    """Exact k-nearest-neighbour graph of ``points`` [N, 3] (``sr_knn_graph``); pass it to ``moran_loss`` to reuse the search."""
    _check_points("knn_graph", points, n_neighbors)
    lib = _lib.load()
    pts = f32c(points)
    n, k, dev = pts.shape[0], int(n_neighbors), pts.device
    with torch.cuda.device(dev):
        work = torch.empty(lib.sr_knn_graph_workspace_bytes(n, k), dtype=torch.uint8, device=dev)
        nn_ix = torch.empty((n, k), dtype=torch.int32, device=dev)
        order = torch.empty(n, dtype=torch.int32, device=dev)
        rev_start = torch.empty(n + 1, dtype=torch.int32, device=dev)
        rev_edges = torch.empty(n * k, dtype=torch.int32, device=dev)
        _lib.check(lib.sr_knn_graph(n, k, ptr(pts), ptr(nn_ix), ptr(order), ptr(rev_start), ptr(rev_edges), ptr(work), _lib.stream(dev)))
    return KnnGraph(nn_ix, order, rev_start, rev_edges)


def _run_forward(n, k, eps, pts, weight, graph, feats):
    """Enqueues sr_moran_forward; returns out = total | terms [T] | means [T] on the device."""
    lib = _lib.load()
    dev = feats[0].device
    widths = (C.c_int * len(feats))(*[f.shape[1] for f in feats])
    with torch.cuda.device(dev):
        work = torch.empty(lib.sr_moran_workspace_bytes(n, len(feats)), dtype=torch.uint8, device=dev)
        out = torch.empty(1 + 2 * len(feats), dtype=torch.float32, device=dev)
        _lib.check(lib.sr_moran_forward(n, k, eps, ptr(pts), ptr(weight), ptr(graph.nn_ix) if graph else None,
                                        ptr(graph.order) if graph else None, len(feats), _pointer_array(feats), widths, ptr(work),
                                        ptr(out), _lib.stream(dev)))
    return out


_TOTAL, _MEASURE = 0, 1


class _Moran(torch.autograd.Function):
    """source = points [N,3] with a graph, or weight [B,n,n] without one.  Differentiable output: the sum of the terms
    (_TOTAL) or the first tensor's mean (_MEASURE); the vector total | terms | means travels detached."""

    @staticmethod
    def forward(ctx, source, graph, eps, which, *features):
        src = f32c(source)
        k = graph.nn_ix.shape[1] if graph is not None else src.shape[-1]
        n = src.shape[0]
        feats = [f32c(f).reshape(-1, f.shape[-1]) if graph is None else f32c(f).reshape(n, -1) for f in features]
        pts, weight = (src, None) if graph is not None else (None, src)
        out = _run_forward(n, k, eps, pts, weight, graph, feats)
        ctx.save_for_backward(src, out, *feats)
        ctx.set_materialize_grads(False)
        ctx.graph, ctx.eps, ctx.which, ctx.k = graph, eps, which, k
        ctx.meta = [(t.shape, t.dtype) for t in (source,) + features]
        value = (out[0] if which == _TOTAL else out[1 + len(feats)]).to(source.dtype)
        ctx.mark_non_differentiable(out)
        return value, out

    @staticmethod
    def backward(ctx, g_value, g_out):
        none = (None,) * (4 + len(ctx.meta) - 1)
        if g_value is None:
            return none
        lib = _lib.load()
        src, out, *feats = ctx.saved_tensors
        graph, k, n, dev = ctx.graph, ctx.k, src.shape[0], src.device
        g = f32c(g_value).reshape(1)
        want_src = ctx.needs_input_grad[0]
        want = [ctx.needs_input_grad[4 + i] for i in range(len(feats))]
        widths = (C.c_int * len(feats))(*[f.shape[1] for f in feats])
        with torch.cuda.device(dev):
            # per-edge rows exist only for the tensors that get a gradient
            edges = torch.empty(lib.sr_moran_edges_bytes(n, k, sum(f.shape[1] for f, w in zip(feats, want) if w)), dtype=torch.uint8, device=dev)
            d_feats = [torch.empty_like(f) if w else None for f, w in zip(feats, want)]
            d_src = torch.empty_like(src) if want_src else None
            pts, weight = (src, None) if graph is not None else (None, src)
            _lib.check(lib.sr_moran_backward(n, k, ctx.eps, ptr(pts), ptr(weight), ptr(graph.nn_ix) if graph else None,
                                             ptr(graph.order) if graph else None, ptr(graph.rev_start) if graph else None,
                                             ptr(graph.rev_edges) if graph else None, len(feats), _pointer_array(feats), widths,
                                             ptr(out) if ctx.which == _TOTAL else None, ptr(g), ptr(edges), _pointer_array(d_feats),
                                             ptr(d_src) if graph is not None else None, ptr(d_src) if graph is None else None, _lib.stream(dev)))
        grads = [None if d is None else d.reshape(shape).to(dt) for d, (shape, dt) in zip([d_src] + d_feats, ctx.meta)]
        return (grads[0], None, None, None) + tuple(grads[1:])


def _call(source, graph, eps, which, features):
    tracked = torch.is_grad_enabled() and (source.requires_grad or any(f.requires_grad for f in features))
    if tracked:
        return _Moran.apply(source, graph, eps, which, *features)
    # nothing to differentiate: nothing is kept
    src = f32c(source)
    n = src.shape[0]
    feats = [f32c(f).reshape(-1, f.shape[-1]) if graph is None else f32c(f).reshape(n, -1) for f in features]
    pts, weight = (src, None) if graph is not None else (None, src)
    k = graph.nn_ix.shape[1] if graph is not None else src.shape[-1]
    out = _run_forward(n, k, eps, pts, weight, graph, feats)
    return (out[0] if which == _TOTAL else out[1 + len(feats)]).to(source.dtype), out


def moran_loss(points: torch.Tensor, features: Sequence[torch.Tensor], n_neighbors: int = 5, eps: float = 1e-5,
               graph: Optional[KnnGraph] = None, return_means: bool = False):
    """``sum_t morans_loss(query_nn(points, n_neighbors, eps)[0], features[t][nn_ix])`` (reference train.py:203-215) as one
    neighbour search, one forward and one backward.

    ``features``: a sequence of [N, ...] tensors, each flattened to [N, F_t].  Returns ``(total, terms)`` with ``terms`` the
    detached [T] tensor of the single ``1 - clamp(mean, 0, 1)`` (and the detached means with ``return_means``).  Gradients go
    to every feature tensor and to ``points`` where they require grad.  ``graph = knn_graph(points, n_neighbors)`` reuses a
    neighbour search."""
    _check_points("moran_loss", points, n_neighbors)
    features = list(features)
    if not 1 <= len(features) <= MAX_TENSORS:
        raise RuntimeError(f"moran_loss: 1 .. {MAX_TENSORS} feature tensors in one call, got {len(features)}")
    n = points.shape[0]
    for f in features:
        if not isinstance(f, torch.Tensor) or not f.is_floating_point() or f.dim() < 1 or f.shape[0] != n or f.numel() == 0:
            raise RuntimeError(f"moran_loss: every feature tensor must be floating-point [N, ...] with N = {n} rows")
        if not f.is_cuda or f.device != points.device:
            raise RuntimeError("moran_loss has no CPU path: every feature tensor must be on the points' HIP ('cuda') device")
    if graph is None:
        graph = knn_graph(points, n_neighbors)
    elif tuple(graph.nn_ix.shape) != (n, int(n_neighbors)) or graph.nn_ix.device != points.device:
        raise RuntimeError(f"moran_loss: the graph is [{graph.nn_ix.shape[0]}, {graph.nn_ix.shape[1]}] on {graph.nn_ix.device}, "
                           f"the call needs [{n}, {n_neighbors}] on {points.device}")
    total, out = _call(points, graph, float(eps), _TOTAL, features)
    t = len(features)
    terms, means = out[1:1 + t].to(points.dtype), out[1 + t:].to(points.dtype)
    return (total, terms, means) if return_means else (total, terms)


class _QueryWeights(torch.autograd.Function):
    @staticmethod
    def forward(ctx, points, graph, eps):
        lib = _lib.load()
        pts = f32c(points)
        n, k, dev = graph.nn_ix.shape[0], graph.nn_ix.shape[1], pts.device
        with torch.cuda.device(dev):
            weights = torch.empty((n, k, k), dtype=torch.float32, device=dev)
            _lib.check(lib.sr_moran_weights(n, k, eps, ptr(pts), ptr(graph.nn_ix), ptr(weights), _lib.stream(dev)))
        ctx.save_for_backward(pts)
        ctx.graph, ctx.eps, ctx.meta = graph, eps, (points.shape, points.dtype)
        return weights.to(points.dtype)

    @staticmethod
    def backward(ctx, g):
        lib = _lib.load()
        pts, = ctx.saved_tensors
        graph = ctx.graph
        n, k, dev = graph.nn_ix.shape[0], graph.nn_ix.shape[1], pts.device
        g = f32c(g)
        with torch.cuda.device(dev):
            edges = torch.empty(lib.sr_moran_edges_bytes(n, k, 0), dtype=torch.uint8, device=dev)
            d_pts = torch.empty_like(pts)
            _lib.check(lib.sr_moran_weights_backward(n, k, ctx.eps, ptr(pts), ptr(graph.nn_ix), ptr(graph.rev_start),
                                                     ptr(graph.rev_edges), ptr(g), ptr(edges), ptr(d_pts), _lib.stream(dev)))
        shape, dt = ctx.meta
        return d_pts.reshape(shape).to(dt), None, None


def query_nn(pts: torch.Tensor, n_neighbors: int = 5, eps: float = 1e-5):
    """The reference's ``query_nn`` (extract_geo.py:100-109): ``(weights [N,K,K], nn_ix [N,K] int64)``; ``weights`` is
    differentiable in ``pts``."""
    _check_points("query_nn", pts, n_neighbors)
    graph = knn_graph(pts, n_neighbors)
    return _QueryWeights.apply(pts, graph, float(eps)), graph.nn_ix.long()


def _check_pair(name, weight, feature):
    if not isinstance(weight, torch.Tensor) or not isinstance(feature, torch.Tensor):
        raise TypeError(f"{name} takes tensors")
    if not weight.is_cuda or not feature.is_cuda:
        raise RuntimeError(f"{name} has no CPU path: tensors must be on a HIP ('cuda') device")
    if weight.device != feature.device:
        raise RuntimeError(f"{name}: weight and feature must be on the same device")
    if weight.dim() != 3 or feature.dim() != 3 or weight.shape[1] != weight.shape[2] or feature.shape[:2] != weight.shape[:2] \
            or not 1 <= weight.shape[1] <= MAX_NEIGHBORS or weight.numel() == 0 or feature.numel() == 0:
        raise RuntimeError(f"{name}: expected weight [B,n,n] and feature [B,n,F] with n <= {MAX_NEIGHBORS}, got "
                           f"{tuple(weight.shape)} and {tuple(feature.shape)}")
    if not weight.is_floating_point() or not feature.is_floating_point():
        raise RuntimeError(f"{name}: floating-point tensors are required")


def morans_measure(weight: torch.Tensor, feature: torch.Tensor) -> torch.Tensor:
    """The reference's ``morans_measure`` (extract_geo.py:111-138) for weight [B,n,n], feature [B,n,F]; gradients go to both."""
    _check_pair("morans_measure", weight, feature)
    return _call(weight, None, 0.0, _MEASURE, [feature])[0]


def morans_loss(weight: torch.Tensor, feature: torch.Tensor) -> torch.Tensor:
    """The reference's ``morans_loss`` (extract_geo.py:140-143): ``1 - clamp(morans_measure(weight, feature), 0, 1)``."""
    _check_pair("morans_loss", weight, feature)
    return _call(weight, None, 0.0, _TOTAL, [feature])[0]
