"""The C ABI of the Moran's I regulariser (include/splatraster.h: sr_knn_graph*, sr_moran_*): exported and bound, its host-only
parts work without a GPU, and every bad call is refused on the host with a message before any launch."""
import ctypes as C
import os
import re

import pytest

import abi_text

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("sr_knn_graph_workspace_bytes", "sr_knn_graph", "sr_moran_workspace_bytes", "sr_moran_edges_bytes", "sr_moran_forward",
       "sr_moran_backward", "sr_moran_weights", "sr_moran_weights_backward")
# the grid build and the reverse adjacency count and place integers with these; nothing else in the two files may be atomic
ALLOWED_INTEGER_ATOMICS = ("atomicAdd(&count[", "atomicAdd(&cursor[")


@pytest.fixture(scope="module")
def lib():
    from splatfields_amd import build, _lib
    build.build_library()
    return _lib.load()


def test_symbols_are_declared_exported_and_bound(lib):
    from splatfields_amd import _lib, build
    header = open(os.path.join(ROOT, "include", "splatraster.h")).read()
    for name in NEW:
        assert name in _lib.SYMBOLS and hasattr(lib, name) and re.search(r"\b%s\s*\(" % name, header), name
    assert "moran.hip" in build.SOURCES and "knn.hip" in build.SOURCES
    assert lib.sr_version() == 4     # additions only: no existing struct or contract changed
    assert "extract_geo.py:100-143" in header and "train.py:203-215" in header      # the "replaces" map
    import splatfields_amd
    for name in ("moran_loss", "knn_graph", "query_nn", "morans_measure", "morans_loss"):
        assert callable(getattr(splatfields_amd, name)), name


def test_workspaces_grow_with_the_problem_and_are_256_byte_granular(lib):
    sizes = [lib.sr_knn_graph_workspace_bytes(n, 5) for n in (5, 1000, 100000, 300000)]
    assert all(s > 0 and s % 256 == 0 for s in sizes) and sizes == sorted(sizes) and len(set(sizes)) == 4
    assert lib.sr_knn_graph_workspace_bytes(1000, 8) > lib.sr_knn_graph_workspace_bytes(1000, 2)
    sizes = [lib.sr_moran_workspace_bytes(n, 4) for n in (1, 1000, 100000, 300000)]
    assert all(s > 0 and s % 256 == 0 for s in sizes) and sizes == sorted(sizes) and sizes[0] < sizes[2] < sizes[3]
    assert lib.sr_moran_workspace_bytes(300000, 8) > lib.sr_moran_workspace_bytes(300000, 1)
    sizes = [lib.sr_moran_edges_bytes(n, 5, 56) for n in (1, 1000, 100000, 300000)]
    assert all(s > 0 and s % 256 == 0 for s in sizes) and sizes == sorted(sizes) and len(set(sizes)) == 4
    assert lib.sr_moran_edges_bytes(300000, 5, 56) >= 300000 * 5 * (56 + 3) * 4      # one row per edge, and its point gradient
    assert lib.sr_moran_edges_bytes(1000, 5, 0) >= 1000 * 5 * 3 * 4 and lib.sr_moran_edges_bytes(1000, 8, 7) > lib.sr_moran_edges_bytes(1000, 5, 7)
    for bad in ((0, 5), (-1, 5), (10, 1), (10, 9)):
        assert lib.sr_knn_graph_workspace_bytes(*bad) == 0, bad
    for bad in ((0, 4), (10, 0), (10, 9)):
        assert lib.sr_moran_workspace_bytes(*bad) == 0, bad
    for bad in ((0, 5, 8), (10, 0, 8), (10, 9, 8), (10, 5, -1)):
        assert lib.sr_moran_edges_bytes(*bad) == 0, bad


def test_bad_calls_are_refused_on_the_host(lib):
    buf = (C.c_float * 1024)()
    p = C.c_void_p(C.addressof(buf))       # host memory: never dereferenced, every check comes before the launch
    err = lambda: lib.sr_last_error()
    ptrs = lambda *v: (C.c_void_p * len(v))(*[x.value if x is not None else None for x in v])
    ints = lambda *v: (C.c_int * len(v))(*v)

    def graph(n=10, k=5, points=p, nn=p, order=p, start=p, edges=p, work=p):
        return lib.sr_knn_graph(n, k, points, nn, order, start, edges, work, None)

    for kw, msg in ((dict(n=0), b"sizes must be positive"), (dict(k=1), b"k must be"), (dict(k=9), b"k must be"),
                    (dict(n=4), b"fewer points than neighbours"), (dict(n=1 << 30), b"too many points"), (dict(points=None), b"null pointer"),
                    (dict(nn=None), b"null pointer"), (dict(order=None), b"null pointer"), (dict(start=None), b"null pointer"),
                    (dict(edges=None), b"null pointer"), (dict(work=None), b"null pointer")):
        assert graph(**kw) != 0 and msg in err(), (kw, err())

    def fwd(n=10, k=5, points=p, weight=None, nn=p, order=None, t=2, feats=ptrs(p, p), widths=ints(3, 4), work=p, out=p):
        return lib.sr_moran_forward(n, k, 1e-5, points, weight, nn, order, t, feats, widths, work, out, None)

    def bwd(n=10, k=5, points=p, weight=None, nn=p, order=None, start=p, edges=p, t=2, feats=ptrs(p, p), widths=ints(3, 4), out=p, g=p,
            store=p, d_feats=ptrs(p, None), d_points=None, d_weight=None):
        return lib.sr_moran_backward(n, k, 1e-5, points, weight, nn, order, start, edges, t, feats, widths, out, g, store, d_feats,
                                     d_points, d_weight, None)

    for call in (fwd, bwd):
        for kw, msg in ((dict(n=0), b"sizes must be positive"), (dict(widths=ints(3, 0)), b"sizes must be positive"),
                        (dict(k=1), b"k must be"), (dict(k=9), b"k must be"), (dict(weight=p, points=None, k=0), b"k must be"),
                        (dict(n=4), b"fewer points than neighbours"), (dict(points=None), b"exactly one"), (dict(weight=p), b"exactly one"),
                        (dict(nn=None), b"points need nn_ix"), (dict(t=0), b"at least one feature tensor"),
                        (dict(t=9), b"at most 8 feature tensors"), (dict(feats=None), b"null pointer"), (dict(widths=None), b"null pointer"),
                        (dict(feats=ptrs(p, None)), b"null pointer"), (dict(n=1 << 30), b"too many"),
                        (dict(widths=ints(1 << 29, 4)), b"too many channels")):
            assert call(**kw) != 0 and msg in err(), (call.__name__, kw, err())
    for kw in (dict(work=None), dict(out=None)):
        assert fwd(**kw) != 0 and b"null pointer" in err(), kw
    for kw, msg in ((dict(g=None), b"null pointer"), (dict(store=None), b"null pointer"), (dict(d_feats=None), b"null pointer"),
                    (dict(d_weight=p), b"dL_dweight without weight"), (dict(points=None, weight=p, nn=None, start=None, edges=None, d_points=p), b"dL_dpoints without points"),
                    (dict(start=None), b"both or neither"), (dict(start=None, edges=None), b"needs the reverse adjacency"),
                    (dict(points=None, weight=p, nn=None), b"reverse adjacency without nn_ix")):
        assert bwd(**kw) != 0 and msg in err(), (kw, err())

    def wts(n=10, k=5, points=p, nn=p, out=p):
        return lib.sr_moran_weights(n, k, 1e-5, points, nn, out, None)

    def wts_bwd(n=10, k=5, points=p, nn=p, start=p, edges=p, dw=p, store=p, d_points=p):
        return lib.sr_moran_weights_backward(n, k, 1e-5, points, nn, start, edges, dw, store, d_points, None)

    for call, names in ((wts, ("points", "nn", "out")), (wts_bwd, ("points", "nn", "start", "edges", "dw", "store", "d_points"))):
        for kw, msg in ((dict(n=0), b"sizes must be positive"), (dict(k=1), b"k must be"), (dict(k=9), b"k must be"),
                        (dict(n=3), b"fewer points than neighbours"), (dict(n=1 << 30), b"too many points")):
            assert call(**kw) != 0 and msg in err(), (call.__name__, kw, err())
        for name in names:
            assert call(**{name: None}) != 0 and b"null pointer" in err(), (call.__name__, name)


def test_nothing_waits_for_the_device_and_no_float_is_added_atomically():
    from splatfields_amd.build import strip_comments
    moran = "\n".join(strip_comments(abi_text.source(f)) for f in ("moran.hip", "reduce.h"))   # with its sums
    knn = strip_comments(abi_text.source("knn.hip"))
    entries = "\n".join(abi_text.entry_point(name) for name in NEW + ("open_moran",))
    assert "sr_moran_backward" in entries and "k_moran_forward" in moran and "block_sum" in moran and "k_knn_search_k" in knn
    for word in ("hipDeviceSynchronize", "hipStreamSynchronize", "hipEventSynchronize", "hipMemcpy(", "hipMemcpyAsync"):
        assert word not in moran and word not in knn and word not in entries, word
    assert "atomic" not in moran and "atomic" not in entries
    rest = knn
    for allowed in ALLOWED_INTEGER_ATOMICS:
        rest = rest.replace(allowed, "")
    assert "atomic" not in rest, "an atomic in knn.hip that is not one of the integer counters / cursors"
    for target in ("count", "cursor"):       # ... and those are integers
        assert re.search(r"uint32_t\* __restrict__ %s\b" % target, knn), target
        assert not re.search(r"float\* (__restrict__ )?%s\b" % target, knn), target
    py = "\n".join(open(os.path.join(ROOT, "splatfields_amd", f)).read() for f in ("moran.py", "_lib.py"))   # with the shared call helpers
    for word in (".item()", ".cpu()", "synchronize", ".tolist()"):
        assert word not in py, word
