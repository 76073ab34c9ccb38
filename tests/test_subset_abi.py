"""The C ABI of the subset step (include/splatraster.h: sr_draw_rows*, sr_rows_gather / sr_rows_scatter,
sr_densification_stats_rows): declared, exported and bound with the header's signatures, SR_VERSION still 4, the job record laid
out as the binding lays it out, every bad call refused on the host with a message before anything is launched, and calls with
nothing to do succeed without a device."""
import ctypes as C
import re

import pytest

import abi_text
from test_c_abi import bound_as

NAMES = ("sr_draw_rows", "sr_draw_rows_ascending_workspace_bytes", "sr_draw_rows_ascending", "sr_rows_gather", "sr_rows_scatter",
         "sr_densification_stats_rows")
BLOCK, WAVE = 256, 64          # csrc/common.h: kBlock, kWave


@pytest.fixture(scope="module")
def lib():
    from splatfields_amd import build, _lib
    build.build_library()
    return _lib.load()


def test_symbols_are_declared_exported_and_bound(lib):
    from splatfields_amd import _lib, build
    protos = abi_text.prototypes()
    for name in NAMES:
        assert name in protos and name in _lib.SYMBOLS and hasattr(lib, name), name
        assert abi_text.entry_point(name)                                  # defined once, in one of build.SOURCES
        assert name in abi_text.source("subset.hip"), name
        ret, args = protos[name]
        restype, argtypes = _lib.SYMBOLS[name]
        assert restype in bound_as(ret)[:1] and len(argtypes) == len(args), name
        for arg, ctype in zip(args, argtypes):
            assert ctype in bound_as(arg), (name, arg, ctype)
    assert "subset.hip" in build.SOURCES and "ordered_scan.h" in build.HEADERS and "densify_stats.h" in build.HEADERS
    assert lib.sr_version() == 4 and _lib.SR_VERSION == 4 and re.search(r"#define\s+SR_VERSION\s+4\b", abi_text.header())


def test_job_record_matches_the_header():
    from splatfields_amd import _lib
    assert abi_text.structs()["SrRowsJob"] == [("const float*", "src", None), ("float*", "dst", None), ("int", "row_floats", None),
                                               ("int", "dst_row_stride", None), ("int", "dst_col_offset", None), ("int", "op", None)]
    J = _lib.SrRowsJob
    assert [f[0] for f in J._fields_] == ["src", "dst", "row_floats", "dst_row_stride", "dst_col_offset", "op"]
    assert (J.src.offset, J.dst.offset, J.row_floats.offset, J.dst_row_stride.offset, J.dst_col_offset.offset, J.op.offset,
            C.sizeof(J)) == (0, 8, 16, 20, 24, 28, 32)
    d = abi_text.defines()
    assert (int(d["SR_DRAW_MAX_KEYS"]), int(d["SR_DRAW_MAX_WALK"]), int(d["SR_ROWS_MAX_JOBS"])) == (_lib.DRAW_MAX_KEYS, _lib.DRAW_MAX_WALK,
                                                                                                  _lib.ROWS_MAX_JOBS) == (16, 256, 8)
    assert (int(d["SR_ROWS_COPY"]), int(d["SR_ROWS_EXP"]), int(d["SR_ROWS_EXP_TO3"])) == (_lib.ROWS_COPY, _lib.ROWS_EXP, _lib.ROWS_EXP_TO3)


def test_stats_share_one_device_function():
    """the per-row arithmetic of the two densification kernels is one function, called by both and defined once"""
    assert len(re.findall(r"void densification_stats_row\(", abi_text.source("densify_stats.h"))) == 1
    for f in ("preprocess.hip", "subset.hip"):
        text = abi_text.source(f)
        assert "densification_stats_row(" in text and "fmaxf(max_radii2D" not in text, f


def test_header_names_the_reference_ranges():
    import os
    text = open(os.path.join(abi_text.ROOT, "include", "splatraster.h")).read()
    block = text[text.index("Which upstream interface each entry replaces"):text.index("Conventions (SURVEY.md Appendix A)")]
    at = block.index("sr_draw_rows / sr_draw_rows_ascending, sr_rows_gather / sr_rows_scatter, sr_densification_stats_rows")
    for span in ("train.py:56-60", ":68", ":281-286", ":431-438"):
        assert span in block[at:at + 600], span


def test_workspace_is_the_layout_the_kernels_carve(lib):
    """csrc/subset.hip carve_draw: one 64-bit member word per wavefront of whole workgroups and one uint32 count per workgroup, each
    part aligned to 256 bytes; 0 rows are sized like 1: one bit per row and a little more"""
    up = lambda v: (v + 255) // 256 * 256
    for n in (0, 1, 63, 64, 256, 257, 27300, 14_300_000, 2 ** 31 - 1):
        blocks = (max(n, 1) + BLOCK - 1) // BLOCK
        assert lib.sr_draw_rows_ascending_workspace_bytes(n) == up(8 * blocks * (BLOCK // WAVE)) + up(4 * blocks), n
    assert lib.sr_draw_rows_ascending_workspace_bytes(-1) == 0 and lib.sr_draw_rows_ascending_workspace_bytes(2 ** 31) == 0


def calls(lib):
    """the entries with acceptable defaults: host memory that is never dereferenced on the device (every check comes before the launch)"""
    from splatfields_amd import _lib
    buf = (C.c_double * 1024)()
    p = C.c_void_p(C.addressof(buf))
    keys = (C.c_ulonglong * 8)(*range(1, 9))

    def job(**kw):
        j = _lib.SrRowsJob(p.value, p.value, 3, 3, 0, _lib.ROWS_COPY)
        for k, v in kw.items():
            setattr(j, k, v)
        return j

    def draw(n_rows=100, n_pick=10, keys=keys, n_keys=8, idx=p, flag=p):
        return lib.sr_draw_rows(n_rows, n_pick, keys, n_keys, idx, flag, None)

    def ascending(n_rows=100, n_pick=10, keys=keys, n_keys=8, work=p, idx=p, flag=p):
        return lib.sr_draw_rows_ascending(n_rows, n_pick, keys, n_keys, work, idx, flag, None)

    def gather(jobs=(job(),), n_pick=10, idx=p, n_rows=100, flag=p, n_jobs=None):
        table = (_lib.SrRowsJob * max(len(jobs), 1))(*jobs)
        return lib.sr_rows_gather(len(jobs) if n_jobs is None else n_jobs, table, n_pick, idx, n_rows, flag, None)

    def scatter(jobs=(job(),), n_pick=10, idx=p, n_rows=100, flag=p, g=(p.value,), d=(p.value,)):
        table = (_lib.SrRowsJob * max(len(jobs), 1))(*jobs)
        return lib.sr_rows_scatter(len(jobs), table, (C.c_void_p * len(g))(*g), (C.c_void_p * len(d))(*d), n_pick, idx, n_rows, flag, None)

    def stats(n_pick=10, idx=p, n_rows=100, g=p, radii=p, accum=p, denom=p, maxr=p, flag=p):
        return lib.sr_densification_stats_rows(n_pick, idx, n_rows, g, radii, accum, denom, maxr, flag, None)

    return p, job, draw, ascending, gather, scatter, stats


def test_bad_calls_are_refused_on_the_host(lib):
    p, job, draw, ascending, gather, scatter, stats = calls(lib)
    err = lambda: lib.sr_last_error()
    odd, half = C.c_void_p(p.value + 1), C.c_void_p(p.value + 4)
    no_keys = C.POINTER(C.c_ulonglong)()
    for fn, name in ((draw, b"sr_draw_rows"), (ascending, b"sr_draw_rows_ascending")):
        for kw in (dict(n_rows=-1), dict(n_rows=2 ** 31, n_pick=1)):
            assert fn(**kw) != 0 and name + b": n_rows must be in 0 .. 2^31 - 1" in err(), kw
        for kw in (dict(n_pick=-1), dict(n_pick=101), dict(n_rows=0, n_pick=1)):
            assert fn(**kw) != 0 and name + b": n_pick must be in 0 .. n_rows" in err(), kw
        for n_keys in (0, -1, 17):
            assert fn(n_keys=n_keys) != 0 and name + b": n_keys must be in 1 .. SR_DRAW_MAX_KEYS" in err()
        assert fn(keys=no_keys) != 0 and b"null pointer in " + name in err()
        assert fn(idx=None) != 0 and b"null pointer in " + name in err()
        assert fn(idx=half) != 0 and b"aligned" in err()
        assert fn(flag=odd) != 0 and b"aligned" in err()
    assert ascending(work=None) != 0 and b"null or misaligned workspace in sr_draw_rows_ascending" in err()
    assert ascending(work=half) != 0 and b"null or misaligned workspace in sr_draw_rows_ascending" in err()
    for fn, name in ((gather, b"sr_rows_gather"), (scatter, b"sr_rows_scatter")):
        assert fn(n_pick=-1) != 0 and name + b": n_pick must be in 0 .. 2^31 - 1" in err()
        assert fn(n_rows=2 ** 31) != 0 and name + b": n_rows must be in 0 .. 2^31 - 1" in err()
        assert fn(idx=None) != 0 and b"null pointer in " + name in err()
        assert fn(idx=half) != 0 and b"aligned" in err()
        assert fn(jobs=(job(op=3),)) != 0 and b"job 0: unknown op" in err()
        assert fn(jobs=(job(row_floats=-1),)) != 0 and b"row_floats must not be negative" in err()
        assert fn(jobs=(job(op=2, row_floats=3, dst_row_stride=9),)) != 0 and b"SR_ROWS_EXP_TO3 reads rows of 1 float" in err()
        assert fn(jobs=(job(dst_row_stride=2),)) != 0 and b"does not fit into dst_row_stride" in err()
        assert fn(jobs=(job(dst_col_offset=1),)) != 0 and b"does not fit into dst_row_stride" in err()
        assert fn(jobs=(job(op=2, row_floats=1, dst_row_stride=2),)) != 0 and b"does not fit into dst_row_stride" in err()
        assert fn(jobs=(job(dst=None),)) != 0 and b"null pointer in " + name + b", job 0" in err()
        assert fn(jobs=(job(dst=odd.value),)) != 0 and b"misaligned" in err()
    assert gather(n_jobs=9) != 0 and b"n_jobs must be in 0 .. SR_ROWS_MAX_JOBS" in err()
    assert gather(jobs=(job(src=None),)) != 0 and b"null pointer in sr_rows_gather, job 0" in err()
    assert scatter(g=(None,)) != 0 and b"null pointer in sr_rows_scatter, job 0" in err()
    assert scatter(g=(odd.value,)) != 0 and b"misaligned" in err()
    assert stats(n_pick=-1) != 0 and b"sr_densification_stats_rows: n_pick must be in 0 .. 2^31 - 1" in err()
    assert stats(n_rows=-1) != 0 and b"sr_densification_stats_rows: n_rows must be in 0 .. 2^31 - 1" in err()
    for kw in (dict(idx=None), dict(g=None), dict(radii=None)):
        assert stats(**kw) != 0 and b"null pointer in sr_densification_stats_rows" in err(), kw
    for kw in (dict(idx=half), dict(g=odd), dict(accum=odd), dict(flag=odd)):
        assert stats(**kw) != 0 and b"aligned" in err(), kw


def test_calls_with_nothing_to_do_succeed_without_a_launch(lib):
    p, job, draw, ascending, gather, scatter, stats = calls(lib)
    assert draw(n_pick=0) == 0 and draw(n_rows=0, n_pick=0, idx=None, flag=None) == 0
    assert ascending(n_pick=0) == 0 and ascending(n_pick=0, work=None, idx=None) == 0
    assert gather(n_pick=0) == 0 and gather(jobs=()) == 0
    assert gather(jobs=(job(row_floats=0, src=None, dst=None),)) == 0                      # SH degree 0: an empty _features_rest
    assert scatter(n_pick=0) == 0 and scatter(d=(None,)) == 0                             # no gradient asked for
    assert stats(n_pick=0) == 0 and stats(accum=None, denom=None, maxr=None) == 0


def test_facade_exports_refuses_bad_arguments_and_has_no_cpu_path():
    import torch
    import splatfields_amd as S
    for name in ("draw_rows", "gather_rows", "get_gaussian_dict", "densification_stats"):
        assert callable(getattr(S, name)), name
    with pytest.raises(RuntimeError, match="no CPU path"):
        S.draw_rows(10, 3, seed=1, device="cpu")
    with pytest.raises(RuntimeError, match="no CPU path"):
        S.gather_rows(torch.zeros(2, dtype=torch.int64), torch.zeros(4, 3))
    with pytest.raises(ValueError, match="order must be"):
        S.draw_rows(10, 3, seed=1, order="sorted", device="cuda")
    with pytest.raises(ValueError, match="n_pick <= n_rows"):
        S.draw_rows(3, 4, seed=1, device="cuda")
    with pytest.raises(ValueError, match="draw must be"):
        S.visual_hull(torch.ones(1, 4, 4), torch.zeros(1, 3, 4), draw="random", device="cuda")
    # the seed of a draw without one comes from torch's CPU generator: torch.manual_seed governs it
    from splatfields_amd import subset
    torch.manual_seed(5)
    a = subset._seed_of(None, None)
    torch.manual_seed(5)
    assert subset._seed_of(None, None) == a and 0 <= a < 2 ** 64 and subset._seed_of(7, None) == 7
    g = torch.Generator().manual_seed(9)
    assert subset._seed_of(None, g) != subset._seed_of(None, g)
    import subset_reference as R
    assert subset._splitmix64(123, 8) == R.keys_of(123) and subset.ROUNDS == R.ROUNDS
