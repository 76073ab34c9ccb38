"""The C ABI of the visual-hull initialisation (include/splatraster.h: sr_hull_*): declared, exported and bound with the header's
signatures, SR_VERSION still 4 everywhere, the workspace is the layout the kernels carve, and every bad call is refused on the host
with a message before anything is launched or copied."""
import ctypes as C
import os
import re

import pytest

import abi_text

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("sr_hull_workspace_bytes", "sr_hull_carve", "sr_hull_gather")
BLOCK, WAVE = 256, 64          # csrc/common.h: kBlock, kWave


@pytest.fixture(scope="module")
def lib():
    from splatfields_amd import build, _lib
    build.build_library()
    return _lib.load()


def test_symbols_are_declared_exported_and_bound_with_the_headers_signatures(lib):
    from splatfields_amd import _lib, build
    for name in NAMES:                  # the signatures: test_c_abi.py::test_every_prototype_matches_the_binding
        assert name in abi_text.prototypes() and name in _lib.SYMBOLS and hasattr(lib, name), name
    assert "hull.hip" in build.SOURCES


def test_version_is_still_4_everywhere(lib):
    from splatfields_amd import _lib
    assert lib.sr_version() == 4 and _lib.SR_VERSION == 4
    assert re.search(r"#define\s+SR_VERSION\s+4\b", abi_text.header())


def test_view_record_and_constants_match_the_header():
    from splatfields_amd import _lib
    V = _lib.SrHullView
    text = abi_text.header()
    body = re.search(r"typedef struct SrHullView \{(.*?)\} SrHullView;", text, flags=re.S).group(1)
    fields = [f.strip() for f in body.split(";") if f.strip()]
    assert fields == ["double m[12]", "long long mask_offset", "int height, width", "int convention", "int outside"]
    assert [f[0] for f in V._fields_] == ["m", "mask_offset", "height", "width", "convention", "outside"]
    assert (V.m.offset, V.mask_offset.offset, V.height.offset, V.width.offset, V.convention.offset, V.outside.offset) == (0, 96, 104, 108, 112, 116)
    assert C.sizeof(V) == 120
    for name, value in (("SR_HULL_KRT", _lib.HULL_KRT), ("SR_HULL_NDC", _lib.HULL_NDC), ("SR_HULL_OUTSIDE_CARVE", _lib.HULL_OUTSIDE_CARVE),
                        ("SR_HULL_OUTSIDE_KEEP", _lib.HULL_OUTSIDE_KEEP), ("SR_HULL_MAX_VIEWS", _lib.HULL_MAX_VIEWS)):
        assert int(re.search(r"#define\s+%s\s+(\d+)" % name, text).group(1)) == value, name
    assert _lib.HULL_MAX_VIEWS >= 64


def test_header_names_the_four_reference_ranges():
    text = open(os.path.join(ROOT, "include", "splatraster.h")).read()
    block = text[text.index("Which upstream interface each entry replaces"):text.index("Conventions (SURVEY.md Appendix A)")]
    at = block.index("sr_hull_carve + sr_hull_gather")
    for span in (":1385-1417", ":1419-1458", ":605-644", ":544-588"):
        assert span in block[at:at + 700], span


def test_workspace_is_the_layout_the_kernels_carve(lib):
    """csrc/hull.hip carve_hull: the view table (SR_HULL_MAX_VIEWS records), one 64-bit survivor word per wavefront of whole
    workgroups, one uint32 count per workgroup, the total -- each part aligned to 256 bytes; 0 items are sized like 1."""
    from splatfields_amd import _lib
    up = lambda v: (v + 255) // 256 * 256
    sizes = []
    for n in (0, 1, 63, 64, 256, 257, 33 ** 3, 256 ** 3, 2 ** 31 - 1):
        blocks = (max(n, 1) + BLOCK - 1) // BLOCK
        want = up(120 * _lib.HULL_MAX_VIEWS) + up(8 * blocks * (BLOCK // WAVE)) + up(4 * blocks) + 256
        assert lib.sr_hull_workspace_bytes(n) == want, n
        sizes.append(want)
    assert sizes == sorted(sizes)
    assert lib.sr_hull_workspace_bytes(-1) == 0 and lib.sr_hull_workspace_bytes(2 ** 31) == 0


def test_bad_calls_are_refused_on_the_host(lib):
    from splatfields_amd import _lib
    buf = (C.c_double * 1024)()
    p = C.c_void_p(C.addressof(buf))       # host memory: never dereferenced, every check comes before the launch and the upload
    err = lambda: lib.sr_last_error()

    def views(n=2, H=8, W=8, convention=_lib.HULL_KRT, outside=_lib.HULL_OUTSIDE_CARVE, offset=None):
        t = (_lib.SrHullView * max(n, 1))()
        for k in range(max(n, 1)):
            t[k].height, t[k].width, t[k].convention, t[k].outside = H, W, convention, outside
            t[k].mask_offset = k * H * W if offset is None else offset
        return t

    def carve(n_views=2, table=None, masks=p, mask_bytes=128, grid=p, G=4, points=None, n_points=0, work=p, count=p):
        table = views(n_views) if table is None else table
        return lib.sr_hull_carve(n_views, table, masks, mask_bytes, grid, G, points, n_points, 0, work, count, None)

    def gather(grid=p, G=4, points=None, n_points=0, work=p, capacity=10, idx=p, xyz=p):
        return lib.sr_hull_gather(grid, G, points, n_points, 0, work, capacity, idx, xyz, None)

    for n in (0, -1, _lib.HULL_MAX_VIEWS + 1):
        assert carve(n_views=n) != 0 and b"n_views must be in 1 .. SR_HULL_MAX_VIEWS" in err(), n
    for kw in (dict(table=C.POINTER(_lib.SrHullView)()), dict(masks=None), dict(work=None), dict(count=None)):
        assert carve(**kw) != 0 and b"null pointer in sr_hull_carve" in err(), kw
    for fn, name in ((carve, b"sr_hull_carve"), (gather, b"sr_hull_gather")):
        assert fn(G=0) != 0 and name + b": G must be at least 1" in err()
        assert fn(G=-3) != 0 and name + b": G must be at least 1" in err()
        assert fn(G=1291) != 0 and name + b": G^3 must not exceed 2^31 - 1" in err()          # 1291^3 = 2 151 685 171
        assert fn(points=p, n_points=5) != 0 and name + b": exactly one of grid and points" in err()       # both
        assert fn(grid=None) != 0 and name + b": exactly one of grid and points" in err()                  # neither
        assert fn(grid=None, G=0, points=p, n_points=-1) != 0 and name + b": n_points must be in 0 .. 2^31 - 1" in err()
        assert fn(grid=None, G=0, points=p, n_points=2 ** 31) != 0 and name + b": n_points must be in 0 .. 2^31 - 1" in err()
    for kw in (dict(H=0), dict(W=0), dict(H=-2)):
        assert carve(table=views(**kw)) != 0 and b"H and W must be at least 1" in err(), kw
    assert carve(table=views(W=1)) != 0 and b"view 0: H or W of 1 divides by zero in the krt normalisation" in err()
    assert carve(table=views(H=1)) != 0 and b"divides by zero in the krt normalisation" in err()
    assert carve(table=views(convention=2)) != 0 and b"unknown pixel-mapping convention" in err()
    assert carve(table=views(outside=-1)) != 0 and b"unknown outside policy" in err()
    assert carve(mask_bytes=127) != 0 and b"view 1: the mask does not fit into mask_bytes" in err()
    assert carve(table=views(offset=-1)) != 0 and b"view 0: the mask does not fit into mask_bytes" in err()
    assert gather(capacity=-1) != 0 and b"capacity must not be negative" in err()
    assert gather(work=None) != 0 and b"null pointer in sr_hull_gather" in err()


def test_calls_with_nothing_to_write_succeed_without_a_launch(lib):
    buf = (C.c_double * 16)()
    p = C.c_void_p(C.addressof(buf))
    assert lib.sr_hull_gather(p, 4, None, 0, 0, p, 0, p, p, None) == 0            # capacity 0
    assert lib.sr_hull_gather(p, 4, None, 0, 0, p, 5, None, None, None) == 0      # no output asked for
    assert lib.sr_hull_gather(None, 0, p, 0, 1, p, 5, p, p, None) == 0            # an empty point list


def test_facade_refuses_bad_arguments_and_has_no_cpu_path():
    import numpy as np
    import torch
    import splatfields_amd as S
    for name in ("visual_hull", "hull_filter", "visual_hull_samples", "visual_hull_samples_list", "hull_matrices", "splats_from_points"):
        assert callable(getattr(S, name)), name
    masks, krt = np.ones((2, 8, 8), np.uint8), np.zeros((2, 3, 4))
    with pytest.raises(RuntimeError, match="no CPU path"):
        S.visual_hull(masks, krt, device="cpu")
    with pytest.raises(RuntimeError, match="no CPU path"):
        S.hull_filter(torch.zeros(4, 3), masks, krt, device="cpu")
    cams = [type("Cam", (), {"KRT": np.eye(3, 4) * (k + 1), "full_proj_transform": torch.eye(4) * (k + 1)})() for k in range(3)]
    assert S.hull_matrices(cams, "krt").shape == (3, 3, 4) and S.hull_matrices(cams, "ndc").shape == (3, 4, 4)
    assert S.hull_matrices(cams, "ndc").dtype == np.float64 and S.hull_matrices(cams, "ndc")[2, 1, 1] == 3.0
    with pytest.raises(ValueError, match="convention"):
        S.hull_matrices(cams, "colmap")
