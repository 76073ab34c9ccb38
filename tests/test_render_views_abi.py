"""The C ABI of the multi-view forward and of the view sum (include/splatraster.h: sr_forward_prepare_views / sr_forward_render_views /
sr_sum_views / SrSumJob): declared, exported and bound with the header's signatures, and every bad call is refused on the host with a
message before any launch."""
import ctypes as C
import re

import pytest

import abi_text


@pytest.fixture(scope="module")
def lib():
    from splatfields_amd import build, _lib
    build.build_library()
    return _lib.load()


ENTRIES = {
    "sr_forward_prepare_views": ["int n_views", "const SrView* views", "const SrSplats* splats", "void* const* geoms", "int* const* radii",
                                 "long long* instances_out", "long long* longest_out", "long long* long_tiles_out", "void* hip_stream"],
    "sr_forward_render_views": ["int n_views", "const SrView* views", "const SrSplats* splats", "void* const* geoms", "void* const* binnings",
                                "const long long* capacities", "const long long* longest", "const long long* long_tiles", "void* const* images",
                                "float* const* out_color", "float* const* out_depth", "float* const* out_alpha", "void* hip_stream"],
    "sr_sum_views": ["int n_jobs", "const SrSumJob* jobs", "int n_views", "void* hip_stream"],
}


def test_entries_parse_from_the_header_and_are_bound_with_those_signatures(lib):
    from splatfields_amd import _lib, build
    protos = abi_text.prototypes()
    P = C.POINTER
    tables = {"const SrView*": P(_lib.SrView), "const SrSplats*": P(_lib.SrSplats), "const SrSumJob*": P(_lib.SrSumJob), "int": C.c_int,
              "void* const*": P(C.c_void_p), "int* const*": P(C.c_void_p), "float* const*": P(C.c_void_p), "long long*": P(C.c_longlong),
              "const long long*": P(C.c_longlong), "void*": C.c_void_p}
    for name, args in ENTRIES.items():
        assert protos[name] == ("int", args), name
        restype, argtypes = _lib.SYMBOLS[name]
        assert restype is C.c_int and hasattr(lib, name)
        assert argtypes == [tables[a.rsplit(" ", 1)[0]] for a in args], name
        assert abi_text.entry_point(name)                      # defined once, in one of build.SOURCES
    assert "view_sum.hip" in build.SOURCES and "sr_sum_views" in abi_text.source("view_sum.hip")
    assert lib.sr_version() == 4                               # additions only: no existing struct or contract changed
    assert abi_text.structs()["SrSumJob"] == [("float*", "dst", None), ("const float*", "src", None), ("long long", "elems", None),
                                              ("long long", "view_stride", None)]
    assert C.sizeof(_lib.SrSumJob) == 32 and C.sizeof(_lib.SrSumJob) * _lib.SUM_MAX_JOBS < 4096   # the table is the kernel argument
    defs = abi_text.defines()
    assert int(defs["SR_SUM_MAX_JOBS"]) == _lib.SUM_MAX_JOBS and int(defs["SR_SUM_MAX_VIEWS"]) == _lib.SUM_MAX_VIEWS == 16


def _view_tables(n_views, h=64, w=64, count=0):
    from splatfields_amd import _lib
    fake = 4096   # never dereferenced: every check precedes the first launch
    views = (_lib.SrView * n_views)(*[_lib.SrView(h, w, 0.5, 0.5, 1.0, 0, 0, 0, 0, fake, fake, fake, fake) for _ in range(n_views)])
    some = fake if count else None   # means3D, opacities, scales, rotations, colors_precomp of a non-empty cloud
    splats = (_lib.SrSplats * n_views)(*[_lib.SrSplats(count, some, some, some, some, None, None, some, 0, None) for _ in range(n_views)])
    return views, splats


def test_prepare_views_refuses_bad_calls_on_the_host(lib):
    err = lib.sr_last_error
    views, splats = _view_tables(2)
    ptrs = (C.c_void_p * 2)(4096, 4096)
    out = [(C.c_longlong * 2)() for _ in range(3)]
    for n in (0, -3):
        assert lib.sr_forward_prepare_views(n, views, splats, ptrs, ptrs, *out, None) != 0 and b"n_views must be at least 1" in err()
    good = [views, splats, ptrs, ptrs, *out]
    for i in range(len(good)):
        args = list(good)
        args[i] = None
        assert lib.sr_forward_prepare_views(2, *args, None) != 0 and b"null table" in err(), i
    # the views of one call share the image size and the splat count
    other, _ = _view_tables(2, h=48)
    mixed = (type(views[0]) * 2)(views[0], other[1])
    assert lib.sr_forward_prepare_views(2, mixed, splats, ptrs, ptrs, *out, None) != 0 and b"share the image size" in err() and b"view 1" in err()
    _, more = _view_tables(2, count=7)
    uneven = (type(splats[0]) * 2)(splats[0], more[1])
    assert lib.sr_forward_prepare_views(2, views, uneven, ptrs, ptrs, *out, None) != 0 and b"share the image size and the splat count" in err()
    holes = (C.c_void_p * 2)(4096, None)
    assert lib.sr_forward_prepare_views(2, views, splats, holes, ptrs, *out, None) != 0 and b"null geom/radii" in err() and b"view 1" in err()
    # a view the one-view entries refuse is refused here with the same message
    bad, _ = _view_tables(1, w=65536)
    assert lib.sr_forward_prepare_views(1, bad, splats, ptrs, ptrs, *out, None) != 0 and b"image too large" in err()


def test_render_views_refuses_bad_calls_on_the_host(lib):
    err = lib.sr_last_error
    views, splats = _view_tables(2)
    ptrs = (C.c_void_p * 2)(4096, 4096)
    caps, longest, tiles = (C.c_longlong * 2)(1 << 16, 1 << 16), (C.c_longlong * 2)(10, 10), (C.c_longlong * 2)(0, 0)
    good = [views, splats, ptrs, ptrs, caps, longest, tiles, ptrs, ptrs, ptrs, ptrs]
    assert lib.sr_forward_render_views(0, *good, None) != 0 and b"n_views must be at least 1" in err()
    for i in range(len(good) - 1):                             # out_alpha, the last table, may be NULL
        args = list(good)
        args[i] = None
        assert lib.sr_forward_render_views(2, *args, None) != 0 and b"null table" in err(), i
    holes = (C.c_void_p * 2)(4096, None)
    for i in (2, 3, 7, 8, 9):
        args = list(good)
        args[i] = holes
        assert lib.sr_forward_render_views(2, *args, None) != 0 and b"null buffer" in err() and b"view 1" in err(), i
    for i, bad, word in ((4, (1 << 16, -1), b"capacity out of range"), (4, (1 << 16, 1 << 32), b"capacity out of range"),
                         (5, (10, -1), b"figures of sr_forward_prepare_views"), (6, (0, -1), b"figures of sr_forward_prepare_views")):
        args = list(good)
        args[i] = (C.c_longlong * 2)(*bad)
        assert lib.sr_forward_render_views(2, *args, None) != 0 and word in err() and b"view 1" in err(), (i, bad)


def _job(dst, src, elems=64, stride=64):
    from splatfields_amd import _lib
    return _lib.SrSumJob(dst, src, elems, stride)


def test_sum_views_refuses_bad_calls_on_the_host(lib):
    from splatfields_amd import _lib
    err = lib.sr_last_error
    buf = (C.c_float * 1024)()
    p = C.addressof(buf)

    def call(jobs, n_views=2, n=None):
        table = (_lib.SrSumJob * max(len(jobs), 1))(*jobs)
        return lib.sr_sum_views(len(jobs) if n is None else n, table, n_views, None)

    for v in (0, -1):
        assert call([_job(p, p + 2048)], n_views=v) != 0 and b"n_views must be at least 1" in err()
    assert call([], n=-1) != 0 and b"n_jobs must be 0 .. SR_SUM_MAX_JOBS" in err()
    assert call([_job(p, p + 2048)] * (_lib.SUM_MAX_JOBS + 1)) != 0 and b"n_jobs must be 0 .. SR_SUM_MAX_JOBS" in err()
    assert lib.sr_sum_views(1, None, 2, None) != 0 and b"null pointer" in err()
    assert call([_job(p, p + 2048), _job(None, p + 2048)]) != 0 and b"null pointer" in err() and b"job 1" in err()
    assert call([_job(p, None)]) != 0 and b"null pointer" in err()
    for dst, src in ((p + 2, p + 2048), (p, p + 2049)):        # a base off a 4-byte boundary
        assert call([_job(dst, src)]) != 0 and b"4-byte aligned" in err()
    assert call([_job(p, p + 2048, elems=-1)]) != 0 and b"negative element count" in err()
    assert call([_job(p, p + 2048, elems=1 << 31, stride=1 << 31)]) != 0 and b"too many elements" in err()
    assert call([_job(p, p + 2048, elems=64, stride=63)]) != 0 and b"view_stride must be at least elems" in err()


def test_sum_views_with_nothing_to_do_launches_nothing(lib):
    """no jobs, and jobs of zero elements, return before any HIP call: they succeed on a host without a device"""
    from splatfields_amd import _lib
    assert lib.sr_sum_views(0, None, 3, None) == 0
    table = (_lib.SrSumJob * 2)(_job(None, None, elems=0, stride=0), _job(None, None, elems=0, stride=5))
    assert lib.sr_sum_views(2, table, 17, None) == 0


def test_the_view_sum_never_waits_and_uses_no_lds_and_no_atomics():
    from splatfields_amd.build import strip_comments
    text = strip_comments(abi_text.source("view_sum.hip"))
    assert "k_sum_views" in text and "sr_sum_views" in text
    for word in ("hipDeviceSynchronize", "hipStreamSynchronize", "hipEventSynchronize", "hipMemcpy", "hipMalloc", "atomic", "__shared__",
                 "__syncthreads", "fmaf"):
        assert word not in text, word
    # sr_forward_render_views never waits: its body holds no synchronisation and hands launch_stage2 no status block
    body = strip_comments(abi_text.entry_point("sr_forward_render_views"))
    assert "Synchronize" not in body and "status_block_wait" not in body and re.search(r"launch_stage2\([^;]*nullptr,\s*longest\[v\], longest\[v\], long_tiles\[v\]", body)


def test_render_views_refuses_cameras_of_different_shapes_and_an_empty_list():
    import torch
    from splatfields_amd import render_views
    from splatfields_amd.synthetic import make_camera
    g = dict(means3D=torch.zeros(4, 3), active_sh_degree=0, gaussian_opacity=torch.ones(4, 1), gaussian_scales=torch.ones(4, 3),
             gaussian_rotations=torch.zeros(4, 4), gaussian_rgb=torch.zeros(4, 3))
    with pytest.raises(ValueError, match=r"share one image size.*\(40, 56\).*\(40, 48\)"):
        render_views([make_camera(0, 56, 40), make_camera(1, 48, 40)], g, None, torch.zeros(3))
    with pytest.raises(ValueError, match="at least one camera"):
        render_views([], g, None, torch.zeros(3))
    with pytest.raises(ValueError, match=r"bg_color must be \[3\] or \[V,3\]"):
        render_views([make_camera(0, 56, 40)], g, None, torch.zeros(2, 3))
    with pytest.raises(RuntimeError, match="no CPU path"):
        render_views([make_camera(0, 56, 40)], g, None, torch.zeros(3))
