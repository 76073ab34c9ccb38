"""The C ABI of the plane generator's kernels (include/splatraster.h: sr_groupnorm_*, sr_conv3x3_*): exported and bound with
the header's signatures, the workspace queries work without a GPU, and every bad call is refused on the host before any launch."""
import ctypes as C
import re

import pytest

import abi_text

NAMES = ("sr_groupnorm_stats_workspace", "sr_groupnorm_stats", "sr_conv3x3_forward", "sr_conv3x3_backward_data",
         "sr_groupnorm_silu_backward_workspace", "sr_groupnorm_silu_backward", "sr_conv3x3_weight_grad_workspace", "sr_conv3x3_weight_grad")


@pytest.fixture(scope="module")
def lib():
    from splatfields_amd import build, _lib
    build.build_library()
    return _lib.load()


def test_symbols_are_exported_with_the_headers_signatures(lib):
    from splatfields_amd import _lib, build
    header = abi_text.header()
    for name in NAMES:                  # the signatures: test_c_abi.py::test_every_prototype_matches_the_binding
        assert name in abi_text.prototypes() and name in _lib.SYMBOLS and hasattr(lib, name), name
    assert "planegen.hip" in build.SOURCES
    assert lib.sr_version() == 4 and re.search(r"#define SR_VERSION 4\b", header)


def test_job_struct_matches_the_header():
    from splatfields_amd import _lib
    fields = [f[1] for f in abi_text.structs()["SrPlaneJob"]]      # in the binding's order: test_c_abi.py
    assert C.sizeof(_lib.SrPlaneJob) == 8 * len(fields)
    assert _lib.PLANE_MAX_JOBS == int(re.search(r"#define SR_PLANE_MAX_JOBS (\d+)", abi_text.header()).group(1))
    for name, value in (("PROLOGUE", _lib.CONV_PROLOGUE), ("UPSAMPLE", _lib.CONV_UPSAMPLE), ("RESIDUAL", _lib.CONV_RESIDUAL), ("SILU_OUT", _lib.CONV_SILU_OUT)):
        assert value == int(re.search(r"#define SR_CONV_%s (\d+)" % name, abi_text.header()).group(1))


def test_workspaces_are_monotone_in_planes_and_size(lib):
    sizes = ((1, 2), (3, 5), (20, 20), (64, 64), (65, 64), (160, 160), (320, 320))
    for n0, n1 in ((1, 2), (2, 3), (3, 8)):
        for h, w in sizes:
            assert 0 < lib.sr_groupnorm_stats_workspace(n0, 32, 32, h, w) < lib.sr_groupnorm_stats_workspace(n1, 32, 32, h, w)
            assert 0 < lib.sr_groupnorm_silu_backward_workspace(n0, 32, h, w) < lib.sr_groupnorm_silu_backward_workspace(n1, 32, h, w)
            assert 0 < lib.sr_conv3x3_weight_grad_workspace(n0, 32, 32, h, w, 0) < lib.sr_conv3x3_weight_grad_workspace(n1, 32, 32, h, w, 0)
    for query in (lambda h, w: lib.sr_groupnorm_stats_workspace(3, 32, 1, h, w), lambda h, w: lib.sr_groupnorm_silu_backward_workspace(3, 32, h, w),
                  lambda h, w: lib.sr_conv3x3_weight_grad_workspace(3, 32, 32, h, w, 0), lambda h, w: lib.sr_conv3x3_weight_grad_workspace(3, 32, 32, h, w, 2)):
        got = [query(h, w) for h, w in sizes]
        assert got == sorted(got) and got[0] < got[-1], got
    # with the channel counts
    assert lib.sr_conv3x3_weight_grad_workspace(3, 8, 32, 20, 20, 0) < lib.sr_conv3x3_weight_grad_workspace(3, 32, 32, 20, 20, 0) < \
        lib.sr_conv3x3_weight_grad_workspace(3, 64, 64, 20, 20, 0)
    assert lib.sr_groupnorm_silu_backward_workspace(3, 16, 20, 20) < lib.sr_groupnorm_silu_backward_workspace(3, 32, 20, 20)
    # unsupported shapes have no workspace
    assert lib.sr_conv3x3_weight_grad_workspace(3, 12, 32, 20, 20, 0) == 0 and lib.sr_conv3x3_weight_grad_workspace(3, 32, 72, 20, 20, 0) == 0
    assert lib.sr_groupnorm_stats_workspace(3, 32, 5, 20, 20) == 0 and lib.sr_groupnorm_stats_workspace(0, 32, 4, 20, 20) == 0
    assert lib.sr_groupnorm_stats_workspace(9, 32, 4, 20, 20) == 0 and lib.sr_groupnorm_silu_backward_workspace(3, 32, 0, 20) == 0


def test_bad_calls_are_refused_on_the_host(lib):
    from splatfields_amd import _lib
    buf = (C.c_float * 1024)()
    p = C.addressof(buf)               # host memory: never dereferenced, every check comes before the launch
    jobs = (_lib.SrPlaneJob * 3)()
    for j in jobs:
        for name, _ in _lib.SrPlaneJob._fields_:
            setattr(j, name, p)
    ws = C.c_void_p(p)
    err = lambda: lib.sr_last_error()

    def fwd(n=3, jobs=jobs, cin=32, cout=32, h=4, w=4, groups=4, flags=1):
        return lib.sr_conv3x3_forward(n, jobs, cin, cout, h, w, groups, flags, None)

    def bwd(n=3, jobs=jobs, cin=32, cout=32, h=4, w=4, flags=0):
        return lib.sr_conv3x3_backward_data(n, jobs, cin, cout, h, w, flags, None)

    def wgrad(n=3, jobs=jobs, cin=32, cout=32, h=4, w=4, groups=4, flags=1, ws=ws):
        return lib.sr_conv3x3_weight_grad(n, jobs, cin, cout, h, w, groups, flags, ws, None)

    def stats(n=3, jobs=jobs, c=32, groups=4, h=4, w=4, ws=ws):
        return lib.sr_groupnorm_stats(n, jobs, c, groups, h, w, 1e-6, ws, None)

    def gnb(n=3, jobs=jobs, c=32, groups=4, h=4, w=4, ws=ws):
        return lib.sr_groupnorm_silu_backward(n, jobs, c, groups, h, w, 1e-6, ws, None)

    for fn in (fwd, bwd, wgrad):
        for kw in (dict(cin=12), dict(cout=72), dict(cin=0), dict(cout=4), dict(cin=68), dict(h=0), dict(w=-1), dict(flags=16)):
            assert fn(**kw) != 0 and b"multiples of 8 in 8..64" in err(), (fn.__name__, kw)
    for fn in (fwd, wgrad):
        for g in (0, 3, 5, 64):
            assert fn(groups=g) != 0 and b"groups must divide cin" in err(), (fn.__name__, g)
    for fn in (stats, gnb):
        for kw in (dict(groups=3), dict(groups=0), dict(c=0), dict(c=65), dict(h=0)):
            assert fn(**kw) != 0 and b"groups must divide channels" in err(), (fn.__name__, kw)
        assert fn(ws=None) != 0 and b"workspace" in err()
    assert wgrad(ws=None) != 0 and b"workspace" in err()
    for fn in (fwd, bwd, wgrad, stats, gnb):
        assert fn(jobs=None) != 0 and b"null pointer" in err() and b"jobs" in err(), fn.__name__
        for n in (0, -1, 9):
            assert fn(n=n) != 0 and b"n_planes" in err(), (fn.__name__, n)
    # a row that lacks a tensor the call needs
    jobs[1].weight = None
    assert fwd() != 0 and b"job 1" in err()
    jobs[1].weight = p
    jobs[2].stats = None
    assert fwd() != 0 and b"job 2" in err()
    assert stats() != 0 and b"job 2" in err()
