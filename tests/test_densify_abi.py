"""The C ABI of densify / prune (include/splatraster.h: sr_densify_*): exported and bound, its host-only part works without a
GPU, and every bad call is refused on the host with a message before any launch."""
import ctypes as C
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("sr_densify_workspace_bytes", "sr_densify_plan", "sr_densify_gather")
BLOCK = 256          # rows per workgroup (csrc/common.h: kBlock)


@pytest.fixture(scope="module")
def lib():
    from splatfields_amd import build, _lib
    build.build_library()
    return _lib.load()


def test_symbols_are_declared_exported_and_bound(lib):
    from splatfields_amd import _lib, build
    header = open(os.path.join(ROOT, "include", "splatraster.h")).read()
    for name in NAMES:
        assert name in _lib.SYMBOLS and hasattr(lib, name) and re.search(r"\b%s\s*\(" % name, header), name
    assert "densify.hip" in build.SOURCES
    assert lib.sr_version() == 4     # no struct or contract of the ABI changed


def test_workspace_is_the_layout_the_plan_carves(lib):
    """csrc/densify.hip: carve_densify puts flags [N] (one byte each), then counters [4][blocks] (uint32), then the totals,
    each part aligned to 256 bytes; N = 0 is sized like N = 1.  The sizes are written out here, not read from the library: this
    test is what pins the layout."""
    from tests.scan_round import SCAN_ROUND
    up = lambda v: (v + 255) // 256 * 256
    sizes = []
    for n in (0, 1, 2, 255, 256, 257, 256 * SCAN_ROUND - 1, 256 * SCAN_ROUND, 256 * SCAN_ROUND + 1, 10 ** 6, 2 ** 31 - 256, 2 ** 31 - 1):
        rows = max(n, 1)
        blocks = (rows + BLOCK - 1) // BLOCK
        assert lib.sr_densify_workspace_bytes(n) == up(rows) + up(16 * blocks) + 256, n
    for n in (0, 1, 255, 256, 257, 262_145):
        rows = max(n, 1)
        blocks = (rows + BLOCK - 1) // BLOCK
        flags, counters, totals = up(rows), up(4 * 4 * blocks), 256
        assert totals >= 5 * 4
        assert lib.sr_densify_workspace_bytes(n) == flags + counters + totals, n
        sizes.append(lib.sr_densify_workspace_bytes(n))
    assert sizes == sorted(sizes) and sizes[0] == sizes[1] == sizes[2] == sizes[3] < sizes[4] < sizes[5]
    assert all(lib.sr_densify_workspace_bytes(n) <= lib.sr_densify_workspace_bytes(n + 1) for n in range(0, 70_000, 97))
    assert lib.sr_densify_workspace_bytes(262_145) == 262_400 + 16_640 + 256       # 1025 workgroups: 16 400 bytes of counters


def test_bad_calls_are_refused_on_the_host(lib):
    buf = (C.c_float * 1024)()
    p = C.c_void_p(C.addressof(buf))       # host memory: never dereferenced, every check comes before the launch
    counts = (C.c_longlong * 5)()
    err = lambda: lib.sr_last_error()

    def plan(n=10, scales=p, cols=3, opacity=p, accum=p, denom=p, radii=p, work=p, dest=p, counts=counts):
        return lib.sr_densify_plan(n, scales, cols, opacity, accum, denom, radii, 0.0035, 0.1, 4.0, 0.01, 20.0, work, dest, counts, None)

    def gather(n=10, row=3, src=p, dst=p, dest=p, mode=0, scales=p, cols=3, rot=p, unit=p):
        return lib.sr_densify_gather(n, row, src, dst, dest, mode, scales, cols, rot, unit, None)

    for kw in (dict(n=-1), dict(cols=0), dict(cols=2), dict(cols=4), dict(cols=-3), dict(n=-1, scales=None), dict(cols=2, n=0)):
        assert plan(**kw) != 0 and b"bad arguments to sr_densify_plan" in err(), kw
    assert plan(counts=None) != 0 and b"null counts in sr_densify_plan" in err()
    assert plan(counts=None, n=0) != 0 and b"null counts in sr_densify_plan" in err()
    for name in ("scales", "opacity", "accum", "denom", "work", "dest"):
        for c in range(5):
            counts[c] = 7
        assert plan(**{name: None}) != 0 and b"null pointer in sr_densify_plan" in err(), name
        assert list(counts) == [0] * 5, name                                  # a refused call leaves no stale counts behind

    for kw in (dict(n=-1), dict(row=0), dict(row=-3), dict(mode=-1), dict(mode=4), dict(mode=4, n=0), dict(row=0, n=0)):
        assert gather(**kw) != 0 and b"bad arguments to sr_densify_gather" in err(), kw
    for mode in (0, 1, 3):
        for name in ("src", "dst", "dest"):
            assert gather(mode=mode, **{name: None}) != 0 and b"null pointer in sr_densify_gather" in err(), (mode, name)
    for kw in (dict(row=1), dict(row=4), dict(scales=None), dict(rot=None), dict(unit=None), dict(cols=2), dict(cols=0)):
        assert gather(mode=2, **kw) != 0 and b"mode 2 (positions) needs [N,3] rows" in err(), kw
    assert gather(mode=2, src=None) != 0 and b"null pointer in sr_densify_gather" in err()


def test_an_empty_cloud_succeeds_without_looking_at_the_pointers(lib):
    counts = (C.c_longlong * 5)(7, 7, 7, 7, 7)
    for cols in (1, 3):
        assert lib.sr_densify_plan(0, None, cols, None, None, None, None, 0.0035, 0.1, 4.0, 0.01, 20.0, None, None, counts, None) == 0
        assert list(counts) == [0] * 5
        counts[:] = [7] * 5
    for mode in range(4):
        assert lib.sr_densify_gather(0, 3, None, None, None, mode, None, 3, None, None, None) == 0, mode
