"""The driver of the chunked weight-gradient launch (splatfields_amd/weight_grad.py) without a GPU: a stand-in library executes
the formula of include/splatraster.h (sr_mlp_weight_grad) on host memory, read through the jobs' own addresses, and records every
call.  Checked: the chunk limit against the four expressions the call sites held before the driver owned it, the chunks' point
counts and addresses, the accumulation in chunk order bit for bit, columns no job writes, two jobs writing one dw, an absent db,
the one failure path, and the fused MLP's job list through the driver."""
import contextlib
import ctypes as C

import numpy as np
import pytest
import torch

from splatfields_amd import _lib, weight_grad as wg

LIMIT = (1 << 31) - 1


def rows_at(address, rows, row, cols):
    """float32 [rows, cols] at `address` with a row stride of `row` floats; touches nothing behind the last row's `cols` floats"""
    flat = np.ctypeslib.as_array((C.c_float * ((rows - 1) * row + cols)).from_address(address))
    return np.lib.stride_tricks.as_strided(flat, shape=(rows, cols), strides=(4 * row, 4))


def contract(dz, x):
    """(dz^T x, column sums of dz) in float32, one point after the other: no library sum whose order could depend on alignment"""
    dw, db = np.zeros((dz.shape[1], x.shape[1]), np.float32), np.zeros(dz.shape[1], np.float32)
    for p in range(dz.shape[0]):
        dw += np.outer(dz[p], x[p])
        db += dz[p]
    return dw, db


class StandIn:
    """what weight_grad.run asks of the library"""

    def __init__(self, workspace=64, error=b"the stand-in refuses this list"):
        self.calls, self.workspace, self.error = [], workspace, error

    def sr_last_error(self):
        return self.error

    def sr_mlp_weight_grad_workspace(self, n_points, n_jobs, jobs):
        return self.workspace

    def sr_mlp_weight_grad(self, n_points, n_jobs, jobs, workspace, workspace_bytes, stream):
        self.calls.append((n_points, [{f: getattr(jobs[i], f) for f, _ in _lib.SrMlpGradJob._fields_} for i in range(n_jobs)]))
        for J in jobs[:n_jobs]:
            dw, db = contract(rows_at(J.dz, n_points, J.dz_row, J.m), rows_at(J.x, n_points, J.x_row, J.k))
            rows_at(J.dw + 4 * J.dw_col0, J.m, J.dw_row, J.k)[:] = dw
            if J.db:
                rows_at(J.db, 1, J.m, J.m)[0] = db
        return 0


@pytest.fixture
def lib(monkeypatch):
    stand_in = StandIn()

    class _Stream:
        cuda_stream = 0

    monkeypatch.setattr(_lib, "load", lambda: stand_in)
    monkeypatch.setattr(torch.cuda, "device", lambda d: contextlib.nullcontext())
    monkeypatch.setattr(torch.cuda, "current_stream", lambda d=None: _Stream())
    return stand_in


def chunked(monkeypatch, limit=64):
    monkeypatch.setattr(wg, "chunk_limit_override", limit)


def randn(*shape, seed=0):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed))


def in_chunk_order(dz, x, limit=64):
    """the float32 sums, in chunk order, of the stand-in's results on each row slice: (dw, db)"""
    total = None
    for lo in range(0, dz.shape[0], limit):
        part = contract(dz[lo:lo + limit].numpy(), x[lo:lo + limit].numpy())
        total = part if total is None else tuple(t + p for t, p in zip(total, part))
    return tuple(torch.from_numpy(t) for t in total)


def bits(t):
    return t.contiguous().view(torch.int32)


# ---- the limit: one function, against what each call site computed itself -----------------------------------------------------

def site_limit(row):
    return max(64, LIMIT // (4 * row) // 64 * 64)


def bound_holds(limit, row):
    return limit * row * 4 < 1 << 31 <= (limit + 64) * row * 4


def test_default_state():
    assert wg.chunk_limit_override is None


def test_limit_of_the_flow_head_and_of_view_colour_at_width_256():
    width = 256
    for dz_row in (4, 8, 12, 32):                                   # flow head: max(dz_row, width), one job per branch
        fields = [(dz_row, 3, width, width, width, 0)] * 2
        assert wg.chunk_limit(fields) == site_limit(max(dz_row, width)) == 2_097_088
    fields = [(4, 3, width, width, width + 3, 0)]                   # view colour: width alone (dz_row = 4 <= width always)
    assert wg.chunk_limit(fields) == site_limit(width) == 2_097_088
    assert bound_holds(2_097_088, width)
    for width in (4, 36, 128):
        assert wg.chunk_limit([(4, 3, width, width, width + 3, 0)]) == site_limit(width) and bound_holds(site_limit(width), width)


@pytest.mark.parametrize("d_in, hidden, out, widest", [(130, 128, 3, "mem_pad"), (27, 64, 3, "hidden"), (27, 64, 64, "out_pad"),
                                                       (75, 64, 33, "mem_pad")])
def test_limit_of_a_fused_mlp(d_in, hidden, out, widest):
    """max(mem_pad, out_pad, H) before; every network has a job of each stride (layer 0 reads the input and its dZ is H wide, the
    top layer's dZ is out_pad wide), so the jobs' own strides give the same row.  out_pad <= H always: it is the widest only tied."""
    from splatfields_amd import fused_mlp as fm
    dims = [(hidden, d_in), (hidden, hidden + d_in), (out, hidden)]
    shape = fm._Shape([torch.zeros(*d) for d in dims], d_in, skips=(0,))
    strides = {"mem_pad": shape.mem_pad, "hidden": shape.hidden, "out_pad": shape.out_pad}
    assert strides[widest] == max(strides.values())
    jobs = fm._grad_jobs(shape)[0]
    assert {s for f in jobs.fields for s in (f[0], f[2])} == set(strides.values())
    row = max(shape.mem_pad, shape.out_pad, shape.hidden)
    assert jobs.limit == wg.chunk_limit(jobs.fields) == site_limit(row) and bound_holds(jobs.limit, row)


@pytest.mark.parametrize("m, k", [(10, 8), (5, 48), (3, 4), (64 * 255, 64 * 255)])
def test_limit_of_point_linear(m, k):
    m_pad = (m + 3) // 4 * 4
    row = max(m_pad, k)
    got = wg.chunk_limit([(m_pad, m, k, k, k, 0)])
    assert got == site_limit(row) and bound_holds(got, row)


def test_limit_never_falls_below_one_slab():
    assert wg.chunk_limit([(1 << 24, 3, 4, 4, 4, 0)]) == 64


# ---- the chunks ---------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n, counts", [(64, (64,)), (65, (64, 1)), (200, (64, 64, 64, 8))])
def test_chunks_addresses_and_sums(lib, monkeypatch, n, counts):
    """two jobs of different strides; the second reads its dz from column 4 of a shared matrix (hence the extra row)"""
    chunked(monkeypatch)
    dz, x0, x1 = randn(wg.dz_rows(n), 12, seed=n), randn(n, 8, seed=n + 1), randn(n, 20, seed=n + 2)
    fields = ((12, 3, 8, 6, 6, 0), (12, 5, 20, 20, 20, 0))
    dw, db = [torch.empty(3, 6), torch.empty(5, 20)], [torch.empty(3), torch.empty(5)]
    starts = ([dz.data_ptr(), dz.data_ptr() + 16], [x0.data_ptr(), x1.data_ptr()])
    wg.run(n, torch.device("cpu"), wg.job_list(fields), *starts, dw, db)
    assert tuple(c[0] for c in lib.calls) == counts
    for c, (_, jobs) in enumerate(lib.calls):
        for i, J in enumerate(jobs):
            assert J["dz"] == starts[0][i] + 64 * c * 12 * 4 and J["x"] == starts[1][i] + 64 * c * fields[i][2] * 4
            assert tuple(J[f] for f in ("dz_row", "m", "x_row", "k", "dw_row", "dw_col0")) == fields[i]
            assert (J["dw"] == dw[i].data_ptr() and J["db"] == db[i].data_ptr()) == (c == 0)      # first chunk: the caller's tensors
    for i, (zs, xs) in enumerate(((dz[:n, 0:3], x0[:, :6]), (dz[:n, 4:9], x1))):
        want_w, want_b = in_chunk_order(zs, xs)
        assert torch.equal(bits(dw[i]), bits(want_w)) and torch.equal(bits(db[i]), bits(want_b)), i


def test_columns_no_job_writes_are_never_read_or_written(lib, monkeypatch):
    chunked(monkeypatch)
    n = 130
    dz, x = randn(n, 4, seed=1), randn(n, 4, seed=2)
    dw = torch.full((3, 7), float("nan"))
    before = bits(dw).clone()
    wg.run(n, torch.device("cpu"), wg.job_list(((4, 3, 4, 4, 7, 0),)), [dz.data_ptr()], [x.data_ptr()], [dw], [None])
    assert tuple(c[0] for c in lib.calls) == (64, 64, 2)
    assert torch.equal(bits(dw[:, 4:]), before[:, 4:]) and torch.isfinite(dw[:, :4]).all()
    assert torch.equal(bits(dw[:, :4]), bits(in_chunk_order(dz[:, :3], x)[0]))


def test_two_jobs_write_column_blocks_of_one_dw(lib, monkeypatch):
    chunked(monkeypatch)
    n = 150
    dz, xa, xb = randn(n, 8, seed=3), randn(n, 12, seed=4), randn(n, 64, seed=5)
    dw, db = torch.full((8, 76), float("nan")), torch.full((8,), float("nan"))
    fields = ((8, 8, 12, 12, 76, 0), (8, 8, 64, 64, 76, 12))
    wg.run(n, torch.device("cpu"), wg.job_list(fields), [dz.data_ptr()] * 2, [xa.data_ptr(), xb.data_ptr()], [dw, dw], [db, None])
    assert tuple(c[0] for c in lib.calls) == (64, 64, 22)
    for c, (_, jobs) in enumerate(lib.calls):
        assert jobs[0]["dw"] == jobs[1]["dw"] and (jobs[0]["dw"] == dw.data_ptr()) == (c == 0)      # one temporary per dw tensor
        assert jobs[0]["db"] and not jobs[1]["db"]                                                   # db = None: skipped
    want_a, want_b = in_chunk_order(dz, xa), in_chunk_order(dz, xb)
    assert torch.equal(bits(dw[:, :12]), bits(want_a[0])) and torch.equal(bits(dw[:, 12:]), bits(want_b[0]))
    assert torch.equal(bits(db), bits(want_a[1]))                                                    # a present db: in chunk order


def test_an_unsupported_list_is_one_error_and_no_launch(lib):
    lib.workspace = 0
    dz, x, dw = randn(8, 4), randn(8, 4), torch.empty(3, 4)
    with pytest.raises(ValueError, match="unsupported weight-gradient job list: the stand-in refuses this list"):
        wg.run(8, torch.device("cpu"), wg.job_list(((4, 3, 4, 4, 4, 0),)), [dz.data_ptr()], [x.data_ptr()], [dw], [None])
    lib.workspace = 64
    with pytest.raises(ValueError):      # fewer addresses than jobs
        wg.run(8, torch.device("cpu"), wg.job_list(((4, 3, 4, 4, 4, 0),) * 2), [dz.data_ptr()], [x.data_ptr()], [dw], [None])
    assert lib.calls == []
    with pytest.raises(ValueError):
        wg.JobList([(4, 3, 4, 4, 4, 0)] * (_lib.MLP_MAX_GRAD_JOBS + 1))


def test_job_lists_are_cached_and_a_call_leaves_the_lock_free(lib):
    jobs = wg.job_list(((4, 3, 4, 4, 4, 0),))
    dz, x, dw = randn(8, 4), randn(8, 4), torch.empty(3, 4)
    lib.workspace = 0
    with pytest.raises(ValueError):
        wg.run(8, torch.device("cpu"), jobs, [dz.data_ptr()], [x.data_ptr()], [dw], [None])
    lib.workspace = 64
    wg.run(8, torch.device("cpu"), jobs, [dz.data_ptr()], [x.data_ptr()], [dw], [None])
    assert wg.job_list(((4, 3, 4, 4, 4, 0),)) is jobs and not jobs.lock.locked() and len(lib.calls) == 1


# ---- a call site through the driver -------------------------------------------------------------------------------------------

@pytest.mark.parametrize("limit", [None, 64])
def test_fused_mlp_job_list_through_the_driver(lib, monkeypatch, limit):
    """fused_mlp._weight_grads (two layers and a skip: layer 1 writes two column blocks of its dW) at 200 points, whole and in
    chunks of 64, against the contraction in float64.  Bound: a float32 sum of n products, one after the other, is within
    n 2^-23 sum |dz| |x| of the exact one; three more additions join the chunks."""
    import heads_reference as hr
    from splatfields_amd import fused_mlp as fm
    chunked(monkeypatch, limit)
    n, d_in, H, out = 200, 27, 64, 3
    weights = [torch.zeros(H, d_in), torch.zeros(H, H + d_in), torch.zeros(out, H)]
    shape = fm._Shape(weights, d_in, skips=(0,))
    x0, acts, G, dz = randn(n, shape.mem_pad, seed=6), randn(2, n, H, seed=7), randn(n, shape.out_pad, seed=8), randn(2, n, H, seed=9)
    dWs, dbs = fm._weight_grads(shape, x0, acts, G, dz, weights)
    assert tuple(c[0] for c in lib.calls) == ((200,) if limit is None else (64, 64, 64, 8)) and len(lib.calls[0][1]) == 4
    refW, refb = hr.weight_grads(shape, x0.double(), acts.double(), G.double(), dz.double(), weights)
    absW, absb = hr.weight_grads(shape, x0.abs().double(), acts.abs().double(), G.abs().double(), dz.abs().double(), weights)
    eps = (n + 3) * 2.0 ** -23
    for got, ref, scale in zip(dWs + dbs, refW + refb, absW + absb):
        assert got.shape == ref.shape and bool(((got.double() - ref).abs() <= eps * scale).all())
