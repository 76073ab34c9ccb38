"""The C ABI of the tri-plane lookup (include/splatraster.h: sr_triplane_*): exported and bound, its host-only part works
without a GPU, and every bad call is refused on the host with a message before any launch."""
import ctypes as C
import os
import re

import pytest

import abi_text

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("sr_triplane_backward_workspace", "sr_triplane_forward", "sr_triplane_backward")
COPIES = 32          # counters per tile (csrc/triplane.hip: kTpCopies)


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
    assert "triplane.hip" in build.SOURCES
    assert lib.sr_version() == 4     # no struct or contract of the ABI changed


def test_workspace_is_zero_for_unsupported_sizes_and_grows_with_points_and_tiles(lib):
    ws = lib.sr_triplane_backward_workspace
    for bad in ((100, 0, 16, 16), (100, 6, 16, 16), (100, 132, 16, 16), (100, 16, 0, 16), (100, 16, 16, 0), (-1, 16, 16, 16), (100, -4, 16, 16)):
        assert ws(*bad) == 0, bad
    sizes = [ws(n, c, h, w) for n in (0, 1, 1000, 100_000) for c in (4, 12, 32, 36, 128) for h, w in ((1, 1), (16, 16), (17, 33), (320, 320))]
    assert all(s > 0 and s % 16 == 0 for s in sizes)
    # with N: the binned lists hold up to four tiles for each of a point's three planes
    by_n = [ws(n, 16, 64, 64) for n in (0, 1, 2, 1000, 4099, 100_000)]
    assert by_n[0] == by_n[1] < by_n[2] < by_n[3] < by_n[4] < by_n[5]
    assert ws(100_000, 16, 64, 64) - ws(1000, 16, 64, 64) == 12 * 4 * 99_000
    # with the tile count: a counter and a start per tile, plane and copy
    by_tiles = [ws(1000, 16, h, w) for h, w in ((16, 16), (17, 16), (17, 17), (64, 64), (320, 320))]
    assert by_tiles == sorted(set(by_tiles))
    assert ws(1000, 16, 17, 16) - ws(1000, 16, 16, 16) == 2 * 4 * 3 * COPIES
    assert ws(1000, 16, 1, 1) == ws(1000, 16, 16, 16) == ws(1000, 32, 16, 16)             # one 16 x 16 tile up to 32 channels
    # 8 x 8 tiles above 32 channels: four times the tiles on the same plane, so more counters
    assert ws(1000, 36, 16, 16) > ws(1000, 32, 16, 16)
    assert ws(1000, 36, 16, 16) - ws(1000, 32, 16, 16) == 2 * 4 * 3 * 3 * COPIES
    assert ws(1000, 36, 16, 16) == ws(1000, 128, 16, 16) and ws(1000, 36, 8, 8) == ws(1000, 32, 16, 16)


def test_bad_calls_are_refused_on_the_host(lib):
    buf = (C.c_float * 1024)()
    p = C.c_void_p(C.addressof(buf))       # host memory: never dereferenced, every check comes before the launch

    def fwd(n=10, c=8, h=4, w=4, planes=p, hwc=p, pts=p, out=p):
        return lib.sr_triplane_forward(n, c, h, w, planes, hwc, pts, out, None)

    def bwd(n=10, c=8, h=4, w=4, hwc=p, pts=p, g=p, d_planes=p, d_pts=p, work=p):
        return lib.sr_triplane_backward(n, c, h, w, hwc, pts, g, d_planes, d_pts, work, None)

    err = lambda: lib.sr_last_error()
    for kw in (dict(planes=None), dict(hwc=None), dict(pts=None), dict(out=None), dict(n=-1)):
        assert fwd(**kw) != 0 and b"bad arguments to sr_triplane_forward" in err(), kw
    for kw in (dict(c=0), dict(c=6), dict(c=-4), dict(h=0), dict(w=0), dict(h=1 << 16, w=1 << 15)):
        assert fwd(**kw) != 0 and b"sr_triplane_forward: channels must be a positive multiple of 4" in err(), kw
    for kw in (dict(hwc=None), dict(pts=None), dict(g=None), dict(n=-1), dict(n=-1, d_planes=None, work=None)):
        assert bwd(**kw) != 0 and b"bad arguments to sr_triplane_backward" in err(), kw
    for kw in (dict(c=0), dict(c=6), dict(c=6, d_planes=None, work=None), dict(h=0), dict(w=0), dict(h=1 << 16, w=1 << 15), dict(n=1 << 29)):
        assert bwd(**kw) != 0 and b"sr_triplane_backward: channels must be a positive multiple of 4" in err(), kw
    # more than 128 channels: the plane gradient has no tile for them; the message names the limit whether or not the caller
    # brought a workspace (sr_triplane_backward_workspace gave it 0 bytes)
    for kw in (dict(c=132), dict(c=132, work=None), dict(c=256, d_pts=None)):
        assert bwd(**kw) != 0 and b"4..128" in err(), kw
    assert bwd(work=None) != 0 and b"dL_dplanes needs a workspace" in err()
    assert bwd(c=128, work=None, d_pts=None) != 0 and b"dL_dplanes needs a workspace" in err()


def test_the_lookup_never_waits_for_the_device_and_has_no_float_atomics():
    from splatfields_amd.build import strip_comments
    text = strip_comments(abi_text.source("triplane.hip"))      # the kernels, their launchers and the entry points
    assert "sr_triplane_backward" in text and "k_tp_accumulate" in text
    for word in ("hipDeviceSynchronize", "hipStreamSynchronize", "hipEventSynchronize", "hipMemcpy(", "hipMemcpyAsync", "atomicAdd_f",
                 "unsafeAtomicAdd", "atomicAdd(float", "atomicExch"):
        assert word not in text, word
    # every atomic adds integers: the tile counters (uint32_t) and the 64-bit fixed-point accumulators in LDS
    for m in re.finditer(r"atomic\w+\(([^,]+),", text):
        assert m.group(1).strip() in ("word", "dst + j", "out_bits"), m.group(0)
    assert re.search(r"uint32_t\* word\b", text) and re.search(r"unsigned long long\* dst\b", text) and re.search(r"uint32_t\* __restrict__ out_bits", text)
    py = open(os.path.join(ROOT, "splatfields_amd", "triplane.py")).read()
    for word in (".item()", ".cpu()", "synchronize", ".tolist()"):
        assert word not in py, word
