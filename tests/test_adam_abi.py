"""The C ABI of the fused Adam step (include/splatraster.h: sr_adam_step / SrAdamJob / SR_ADAM_MAX_TENSORS): exported and bound,
every bad call is refused on the host with a message before any launch, the no-op cases launch nothing, and SplatAdam refuses
what it does not implement at construction."""
import ctypes as C
import os
import re

import pytest
import torch

import abi_text

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def lib():
    from splatfields_amd import build, _lib
    build.build_library()
    return _lib.load()


def make_job(p, count=16, row=4, **over):
    from splatfields_amd import _lib
    fields = dict(param=p, grad=p, exp_avg=p, exp_avg_sq=p, count=count, row=row, step_size=1e-3, bias_correction2_sqrt=0.03,
                  one_minus_beta1=0.1, one_minus_beta2=0.001, eps=1e-15)
    fields.update(over)
    return _lib.SrAdamJob(**fields)


def test_symbol_struct_and_constant_match_the_header(lib):
    from splatfields_amd import _lib, build
    header = abi_text.header()
    assert "sr_adam_step" in _lib.SYMBOLS and hasattr(lib, "sr_adam_step") and re.search(r"\bsr_adam_step\s*\(", header)
    assert int(re.search(r"#define\s+SR_ADAM_MAX_TENSORS\s+(\d+)", header).group(1)) == _lib.ADAM_MAX_TENSORS
    assert "adam.hip" in build.SOURCES
    assert lib.sr_version() == 4     # additions only: no existing struct or contract changed
    assert C.sizeof(_lib.SrAdamJob) == 4 * 8 + 8 + 4 + 5 * 4      # four pointers, count, row, five floats: no padding
    assert C.sizeof(_lib.SrAdamJob) * _lib.ADAM_MAX_TENSORS < 4096   # the table travels as a kernel argument


def test_bad_calls_are_refused_on_the_host(lib):
    from splatfields_amd import _lib
    buf = (C.c_float * 64)()
    p = C.addressof(buf)                   # host memory, 16-byte aligned or not: never dereferenced, every check precedes the launch
    err = lambda: lib.sr_last_error()

    def call(jobs, visible=None, rows=0, n=None):
        table = (_lib.SrAdamJob * max(len(jobs), 1))(*jobs)
        return lib.sr_adam_step(len(jobs) if n is None else n, table, visible, rows, None)

    assert call([], n=-1) != 0 and b"n_jobs must be 0 .. SR_ADAM_MAX_TENSORS" in err()
    assert call([make_job(p)] * (_lib.ADAM_MAX_TENSORS + 1)) != 0 and b"n_jobs must be 0 .. SR_ADAM_MAX_TENSORS" in err()
    assert lib.sr_adam_step(1, None, None, 0, None) != 0 and b"null pointer" in err()
    for name in ("param", "grad", "exp_avg", "exp_avg_sq"):
        assert call([make_job(p), make_job(p, **{name: None})]) != 0 and b"null pointer" in err() and b"job 1" in err(), name
        assert call([make_job(p, **{name: p + 2})]) != 0 and b"4-byte aligned" in err(), name
    assert call([make_job(p, count=-1)]) != 0 and b"negative element count" in err()
    assert call([make_job(p, count=1 << 31)]) != 0 and b"too many elements" in err()
    mask = C.c_void_p(p)
    assert call([make_job(p, count=16, row=4)], mask, rows=5) != 0 and b"count == rows * row" in err()
    assert call([make_job(p, count=16, row=4), make_job(p, count=12, row=4)], mask, rows=4) != 0 and b"job 1" in err()
    assert call([make_job(p, count=16, row=0)], mask, rows=4) != 0 and b"count == rows * row" in err()
    assert call([make_job(p, count=0, row=4)], mask, rows=4) != 0 and b"count == rows * row" in err()
    assert call([make_job(p, count=16, row=4)], mask, rows=-4) != 0 and b"negative row count" in err()


def test_nothing_to_do_launches_nothing(lib):
    """n_jobs == 0 and jobs of zero elements are valid and return before any HIP call: they succeed on a host without a device,
    where a launch would fail."""
    from splatfields_amd import _lib
    assert lib.sr_adam_step(0, None, None, 0, None) == 0
    table = (_lib.SrAdamJob * 3)(make_job(None, count=0), make_job(None, count=0, row=7), make_job(None, count=0))
    assert lib.sr_adam_step(3, table, None, 0, None) == 0
    mask = (C.c_ubyte * 4)()
    assert lib.sr_adam_step(1, table, C.c_void_p(C.addressof(mask)), 0, None) == 0      # 0 rows of 4 elements


def test_the_step_never_waits_and_uses_no_lds_and_no_atomics():
    from splatfields_amd.build import strip_comments
    text = strip_comments(abi_text.source("adam.hip"))        # the kernel, its launcher and sr_adam_step
    assert "k_adam" in text and "sr_adam_step" in text
    for word in ("hipDeviceSynchronize", "hipStreamSynchronize", "hipEventSynchronize", "hipMemcpy", "hipMalloc", "atomic", "__shared__",
                 "__syncthreads"):
        assert word not in text, word
    py = open(os.path.join(ROOT, "splatfields_amd", "optim.py")).read()
    for word in (".cpu()", "synchronize", ".tolist()", ".item()"):
        assert word not in py, word


def test_splat_adam_refuses_what_it_does_not_implement():
    from splatfields_amd import SplatAdam
    w = torch.nn.Parameter(torch.zeros(4, 3))
    with pytest.raises(ValueError, match="no CPU path"):
        SplatAdam([w], lr=1e-3)
    with pytest.raises(ValueError, match="no CPU path"):
        SplatAdam([{"params": [w], "lr": 1e-3, "name": "xyz"}], lr=0.0, eps=1e-15)
    # the options are refused before the parameters are looked at
    for kw in (dict(weight_decay=0.01), dict(amsgrad=True), dict(maximize=True), dict(capturable=True), dict(differentiable=True)):
        with pytest.raises(ValueError, match=next(iter(kw))):
            SplatAdam([w], lr=1e-3, **kw)
    with pytest.raises(ValueError, match="weight_decay"):
        SplatAdam([{"params": [w], "weight_decay": 0.1}], lr=1e-3)
    with pytest.raises(TypeError, match="unknown option"):
        SplatAdam([w], lr=1e-3, nesterov=True)
    with pytest.raises(ValueError, match="invalid lr"):
        SplatAdam([w], lr=-1.0)
    with pytest.raises(ValueError, match="invalid lr"):
        SplatAdam([w], lr=1e-3, betas=(0.9, 1.0))
    with pytest.raises(ValueError, match="lr must be a number"):
        SplatAdam([w], lr=torch.tensor(1e-3))


def test_splat_adam_refuses_float64_and_non_contiguous_parameters():
    from splatfields_amd import SplatAdam
    for bad, word in ((torch.zeros(4, 3, dtype=torch.float64), "float32"), (torch.zeros(3, 4).t(), "contiguous")):
        with pytest.raises(ValueError, match=word):
            SplatAdam([torch.nn.Parameter(bad)], lr=1e-3)


def test_defaults_are_torch_adams():
    """The group options are torch.optim.Adam's own, so a state_dict of either loads into the other."""
    from splatfields_amd.optim import _adam_defaults
    w = torch.nn.Parameter(torch.zeros(2))
    ref = torch.optim.Adam([w], lr=0.25, betas=(0.8, 0.9), eps=1e-15)
    mine = _adam_defaults()
    mine.update(lr=0.25, betas=(0.8, 0.9), eps=1e-15)
    assert mine == ref.defaults
