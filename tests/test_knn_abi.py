"""The C ABI of the distCUDA2 counterpart (include/splatraster.h: sr_knn_workspace_bytes, sr_knn3_mean_dist2): exported and
bound, the workspace size is a host-only function, and every bad call is refused on the host before any launch.  CPU only."""
import ctypes as C
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def lib():
    from splatfields_amd import build, _lib
    build.build_library()
    return _lib.load()


def test_symbols_are_declared_exported_and_bound(lib):
    from splatfields_amd import _lib, build
    header = open(os.path.join(ROOT, "include", "splatraster.h")).read()
    for name in ("sr_knn_workspace_bytes", "sr_knn3_mean_dist2"):
        assert name in _lib.SYMBOLS and hasattr(lib, name) and re.search(r"\b%s\s*\(" % name, header), name
    assert "knn.hip" in build.SOURCES and _lib.SYMBOLS["sr_knn_workspace_bytes"][0] is C.c_size_t
    from simple_knn._C import distCUDA2
    assert callable(distCUDA2)


def test_workspace_is_positive_256_byte_granular_and_monotone(lib):
    ns = (0, 1, 2, 3, 4, 5, 63, 64, 65, 1000, 100000, 300000, 1 << 24)
    sizes = [lib.sr_knn_workspace_bytes(n) for n in ns]
    assert all(s > 0 and s % 256 == 0 for s in sizes) and sizes == sorted(sizes)
    assert sizes[ns.index(1000)] < sizes[ns.index(100000)] < sizes[ns.index(300000)] < sizes[-1]
    for n, s in zip(ns, sizes):     # bounds, three arrays of n + 1 cells (n cells at the most), the points' order
        assert s >= 32 + 3 * 4 * (max(n, 2) + 1) + 4 * n, n
    assert lib.sr_knn_workspace_bytes(-5) == lib.sr_knn_workspace_bytes(0)


def test_workspace_sizes_follow_the_layout(lib):
    """csrc/knn.hip: carve_knn puts the bounds (8 floats), three arrays of max(n, 2) + 1 uint32 (cell counts, starts, cursors), the
    n points cell after cell (uint32; n = 0 is sized like n = 1) and, for the graph, its n k reverse edges (uint32), each part
    aligned to 256 bytes.  The sizes are written out here, not read from the library: this test is what pins the layout."""
    from tests.scan_round import SCAN_ROUND
    up = lambda v: (v + 255) // 256 * 256
    grid = (0, 1, 2, 255, 256, 257, 256 * SCAN_ROUND - 1, 256 * SCAN_ROUND, 256 * SCAN_ROUND + 1, 10 ** 6)
    for n in grid + (2 ** 31 - 1,):
        assert lib.sr_knn_workspace_bytes(n) == 256 + 3 * up(4 * (max(n, 2) + 1)) + up(4 * max(n, 1)), n
    for k in range(2, 9):
        for n in grid + (2 ** 31 - 1,):              # the size query takes any n > 0; sr_knn_graph itself stops at (2^31 - 1) / 24 points
            want = 0 if n == 0 else 256 + 3 * up(4 * (max(n, 2) + 1)) + up(4 * n) + up(4 * n * k)
            assert lib.sr_knn_graph_workspace_bytes(n, k) == want, (n, k)
    assert lib.sr_knn_graph_workspace_bytes(1000, 1) == lib.sr_knn_graph_workspace_bytes(1000, 9) == 0


def test_bad_calls_are_refused_on_the_host(lib):
    buf = (C.c_float * 1024)()
    p = C.c_void_p(C.addressof(buf))       # host memory: never dereferenced, every check comes before the launch

    def knn3(n=10, points=p, out=p, work=p):
        return lib.sr_knn3_mean_dist2(n, points, out, work, None)

    for kw in (dict(n=-1), dict(n=-(1 << 31)), dict(points=None), dict(out=None), dict(work=None)):
        assert knn3(**kw) != 0 and b"bad arguments to sr_knn3_mean_dist2" in lib.sr_last_error(), kw


def test_distcuda2_refuses_host_tensors_and_other_shapes():
    import torch
    from simple_knn._C import distCUDA2
    with pytest.raises(RuntimeError, match="no CPU path"):
        distCUDA2(torch.rand(10, 3))
