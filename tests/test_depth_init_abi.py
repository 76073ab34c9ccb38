"""The C ABI of the depth-map initialisation (include/splatraster.h: sr_depth_points_*): declared, exported and bound with the
header's signatures, SR_VERSION still 4, the workspace is the layout the kernels carve, every bad call is refused on the host with
a message before anything is launched, and calls with nothing to do succeed without a device."""
import ctypes as C
import re

import pytest

import abi_text

NAMES = ("sr_depth_points_workspace_bytes", "sr_depth_points_mark", "sr_depth_points_gather", "sr_depth_points_select")
BLOCK, WAVE = 256, 64          # csrc/common.h: kBlock, kWave


@pytest.fixture(scope="module")
def lib():
    from splatfields_amd import build, _lib
    build.build_library()
    return _lib.load()


def test_symbols_are_declared_exported_and_bound(lib):
    from splatfields_amd import _lib, build
    for name in NAMES:                  # the signatures: test_c_abi.py::test_every_prototype_matches_the_binding
        assert name in abi_text.prototypes() and name in _lib.SYMBOLS and hasattr(lib, name), name
        assert abi_text.entry_point(name)                                  # defined once, in one of build.SOURCES
        assert name in abi_text.source("depth_init.hip"), name
    assert "depth_init.hip" in build.SOURCES and "ordered_scan.h" in build.HEADERS
    assert lib.sr_version() == 4 and _lib.SR_VERSION == 4 and re.search(r"#define\s+SR_VERSION\s+4\b", abi_text.header())


def test_camera_record_matches_the_header():
    from splatfields_amd import _lib
    assert abi_text.structs()["SrDepthCamera"] == [("double", "kinv", 9), ("double", "pose", 12)]
    V = _lib.SrDepthCamera
    assert [f[0] for f in V._fields_] == ["kinv", "pose"] and (V.kinv.offset, V.pose.offset, C.sizeof(V)) == (0, 72, 168)


def test_header_names_the_reference_ranges():
    import os
    text = open(os.path.join(abi_text.ROOT, "include", "splatraster.h")).read()
    block = text[text.index("Which upstream interface each entry replaces"):text.index("Conventions (SURVEY.md Appendix A)")]
    at = block.index("sr_depth_points_mark + sr_depth_points_gather / sr_depth_points_select")
    for span in (":1476-1491", ":1376", ":1463", ":1603-1613", ":1653-1658"):
        assert span in block[at:at + 600], span


def test_workspace_is_the_layout_the_kernels_carve(lib):
    """csrc/depth_init.hip carve_depth: one 64-bit survivor word per wavefront of whole workgroups, one uint32 count, one float
    minimum and one float maximum per workgroup, the total -- each part aligned to 256 bytes; 0 items are sized like 1"""
    up = lambda v: (v + 255) // 256 * 256
    sizes = []
    for n in (0, 1, 63, 64, 256, 257, 27300, 64 * 800 * 800, 2 ** 31 - 1):
        blocks = (max(n, 1) + BLOCK - 1) // BLOCK
        want = up(8 * blocks * (BLOCK // WAVE)) + 3 * up(4 * blocks) + 256
        assert lib.sr_depth_points_workspace_bytes(n) == want, n
        sizes.append(want)
    assert sizes == sorted(sizes)
    assert lib.sr_depth_points_workspace_bytes(-1) == 0 and lib.sr_depth_points_workspace_bytes(2 ** 31) == 0


def calls(lib):
    """the three entries with acceptable defaults: host memory that is never dereferenced (every check comes before the launch)"""
    from splatfields_amd import _lib
    buf = (C.c_double * 1024)()
    p = C.c_void_p(C.addressof(buf))
    cams = C.cast(p, C.POINTER(_lib.SrDepthCamera))

    def mark(B=2, H=4, W=5, cameras=cams, depths=p, dbl=0, masks=None, work=p, count=p, bounds=p):
        return lib.sr_depth_points_mark(B, H, W, cameras, depths, dbl, masks, work, count, bounds, None)

    def gather(B=2, H=4, W=5, cameras=cams, depths=p, dbl=0, images=p, cb=1, work=p, capacity=10, xyz=p, rgb=p, idx=p):
        return lib.sr_depth_points_gather(B, H, W, cameras, depths, dbl, images, cb, work, capacity, xyz, rgb, idx, None)

    def select(B=2, H=4, W=5, cameras=cams, depths=p, dbl=0, images=p, cb=1, work=p, ranks=p, n_ranks=3, xyz=p, rgb=p, idx=p, flag=p):
        return lib.sr_depth_points_select(B, H, W, cameras, depths, dbl, images, cb, work, ranks, n_ranks, xyz, rgb, idx, flag, None)

    return p, mark, gather, select


def test_bad_calls_are_refused_on_the_host(lib):
    from splatfields_amd import _lib
    p, mark, gather, select = calls(lib)
    err = lambda: lib.sr_last_error()
    odd = C.c_void_p(p.value + 1)
    no_cams = C.POINTER(_lib.SrDepthCamera)()
    for fn, name in ((mark, b"sr_depth_points_mark"), (gather, b"sr_depth_points_gather"), (select, b"sr_depth_points_select")):
        assert fn(B=-1) != 0 and name + b": B must not be negative" in err()
        for kw in (dict(H=0), dict(W=0), dict(H=-2), dict(W=-1)):
            assert fn(**kw) != 0 and name + b": H and W must be at least 1" in err(), kw
        for kw in (dict(B=2 ** 15, H=2 ** 8, W=2 ** 8), dict(B=1, H=2 ** 16, W=2 ** 16), dict(B=3, H=2 ** 15, W=2 ** 15)):    # 2^31, 2^32, 3 2^30
            assert fn(**kw) != 0 and name + b": B H W must not exceed 2^31 - 1" in err(), kw
        for flag in (2, -1):
            assert fn(dbl=flag) != 0 and name + b": depth_is_double must be 0 (float32) or 1 (float64)" in err()
        assert fn(cameras=no_cams) != 0 and b"null pointer in " + name in err()
        assert fn(depths=None) != 0 and b"null pointer in " + name in err()
        assert fn(work=None) != 0 and b"null" in err() and name in err()
        assert fn(depths=odd) != 0 and b"aligned" in err()
        assert fn(dbl=1, depths=C.c_void_p(p.value + 4)) != 0 and b"aligned" in err()
    assert mark(count=None, bounds=None) != 0 and b"null pointer in sr_depth_points_mark" in err()
    assert mark(count=odd) != 0 and b"aligned" in err()
    assert gather(capacity=-1) != 0 and b"sr_depth_points_gather: capacity must not be negative" in err()
    for fn, name in ((gather, b"sr_depth_points_gather"), (select, b"sr_depth_points_select")):
        for cb in (0, 2, 3, 16, -1):
            assert fn(cb=cb) != 0 and name + b": color_bytes must be 1, 4 or 8" in err(), cb
        assert fn(images=None) != 0 and b"colors_out needs images" in err()
        assert fn(cb=4, images=C.c_void_p(p.value + 2)) != 0 and b"aligned to color_bytes" in err()
        assert fn(xyz=odd) != 0 and b"aligned" in err()
        assert fn(idx=C.c_void_p(p.value + 4)) != 0 and b"aligned" in err()
    assert select(n_ranks=-1) != 0 and b"n_ranks must be in 0 .. 2^31 - 1" in err()
    assert select(n_ranks=2 ** 31) != 0 and b"n_ranks must be in 0 .. 2^31 - 1" in err()
    assert select(ranks=None) != 0 and b"null pointer in sr_depth_points_select" in err()
    assert select(flag=None) != 0 and b"null pointer in sr_depth_points_select" in err()
    assert select(ranks=C.c_void_p(p.value + 4)) != 0 and b"aligned" in err()
    assert select(B=0) != 0 and b"an empty batch has no row to select" in err()


def test_calls_with_nothing_to_do_succeed_without_a_launch(lib):
    p, mark, gather, select = calls(lib)
    assert mark(B=0) == 0 and mark(B=0, cameras=None, depths=None) == 0                   # an empty batch
    assert gather(B=0) == 0
    assert gather(capacity=0) == 0
    assert gather(xyz=None, rgb=None, idx=None, images=None, cb=0) == 0                    # no output asked for
    assert select(n_ranks=0) == 0 and select(n_ranks=0, ranks=None, flag=None) == 0
    assert select(xyz=None, rgb=None, idx=None) == 0
    assert select(B=0, n_ranks=0) == 0


def test_facade_exports_refuses_bad_arguments_and_has_no_cpu_path():
    import numpy as np
    import splatfields_amd as S
    for name in ("depth_points", "depth_points_bounds", "gen_3dpoints", "depth_point_cloud"):
        assert callable(getattr(S, name)), name
    d, k, p = np.ones((2, 4, 5), np.float32), np.eye(3)[None].repeat(2, 0), np.eye(4)[None].repeat(2, 0)
    with pytest.raises(RuntimeError, match="no CPU path"):
        S.depth_points(d, k, p, device="cpu")
    with pytest.raises(RuntimeError, match="no CPU path"):
        S.depth_points_bounds(d, k, p, device="cpu")
    with pytest.raises(RuntimeError, match="no CPU path"):
        S.depth_point_cloud(d, k, p, np.zeros((2, 4, 5, 3), np.uint8), 10, device="cpu")
