"""The C ABI of the stand-alone SH stage (include/splatraster.h: sr_sh_forward, sr_sh_forward_views, sr_sh_backward): exported and
bound, every bad call is refused on the host with a message before any launch, and the Python entry points
(splatfields_amd/sh.py) refuse tensors that the kernels would reach through a host or out-of-range pointer.  CPU only: nothing
here launches a kernel."""
import ctypes as C
import os
import re

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("sr_sh_forward", "sr_sh_forward_views", "sr_sh_backward")


@pytest.fixture(scope="module")
def lib():
    from splatfields_amd import build, _lib
    build.build_library()
    return _lib.load()


def test_symbols_are_declared_exported_and_bound(lib):
    from splatfields_amd import _lib, build
    header = open(os.path.join(ROOT, "include", "splatraster.h")).read()
    for name in NAMES:
        assert name in _lib.SYMBOLS and hasattr(lib, name) and re.search(r"\bint %s\s*\(" % name, header), name
    assert "sh.hip" in build.SOURCES
    assert len(_lib.SYMBOLS["sr_sh_forward"][1]) == 9 and len(_lib.SYMBOLS["sr_sh_forward_views"][1]) == 10
    assert len(_lib.SYMBOLS["sr_sh_backward"][1]) == 13 and _lib.SYMBOLS["sr_sh_backward"][1][8] is C.c_float


def test_bad_calls_are_refused_on_the_host(lib):
    buf = (C.c_float * 1024)()
    p = C.c_void_p(C.addressof(buf))       # host memory: never dereferenced, every check comes before the launch
    err = lambda: lib.sr_last_error()

    def fwd(n=10, k=16, deg=3, means=p, shs=p, campos=p, colors=p, clamped=p):
        return lib.sr_sh_forward(n, k, deg, means, shs, campos, colors, clamped, None)

    def views(n=10, k=16, deg=3, v=2, means=p, shs=p, campos=p, colors=p, keep=p):
        return lib.sr_sh_forward_views(n, k, deg, v, means, shs, campos, colors, keep, None)

    def bwd(n=10, k=16, deg=3, v=2, means=p, shs=p, campos=p, dcol=p, d_shs=p, d_means=p):
        return lib.sr_sh_backward(n, k, deg, v, means, shs, campos, dcol, 1.0, d_shs, d_means, 1, None)

    sizes = [dict(n=-1), dict(deg=-1), dict(deg=4), dict(k=15), dict(k=0, deg=0), dict(k=3, deg=1), dict(k=8, deg=2)]
    for call in (fwd, views, bwd):
        for kw in sizes + ([dict(v=-1)] if call is not fwd else []):
            assert call(**kw) != 0 and b"bad arguments to " + call_name(call) in err(), (call.__name__, kw, err())
    for call, names in ((fwd, ("means", "shs", "campos", "colors", "clamped")), (views, ("means", "shs", "campos", "colors")),
                        (bwd, ("means", "shs", "campos", "dcol"))):
        for name in names:
            assert call(**{name: None}) != 0 and b"null pointer in " + call_name(call) in err(), (call.__name__, name, err())


def call_name(call):
    return {"fwd": b"sr_sh_forward", "views": b"sr_sh_forward_views", "bwd": b"sr_sh_backward"}[call.__name__]


def test_python_entry_points_refuse_before_any_launch():
    """Every refusal below is raised from host-side checks on tensor metadata; the device is never touched (and there is none
    where this test runs)."""
    from splatfields_amd.sh import sh_backward, sh_forward, sh_forward_views, sh_to_rgb
    n, v = 10, 2
    means, shs, campos, dcol = torch.rand(n, 3), torch.rand(n, 16, 3), torch.rand(v, 3), torch.rand(v, n, 3)
    for call in (lambda: sh_forward(means, shs, campos[0], 3), lambda: sh_forward_views(means, shs, campos, 3),
                 lambda: sh_backward(means, shs, campos, dcol, 3), lambda: sh_backward(means, shs, campos, dcol, 3, want_shs=False),
                 lambda: sh_backward(means, shs, campos, dcol, 3, means_grad=torch.zeros(n, 3)),
                 lambda: sh_to_rgb(means.requires_grad_(True), shs, campos[0], 3)):
        with pytest.raises(RuntimeError, match="no CPU path"):
            call()
