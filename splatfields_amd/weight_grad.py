"""The one caller of sr_mlp_weight_grad (include/splatraster.h; csrc/mlp.hip): dW = dZ^T X and db = sum dZ, contracted over the
points by the slab kernel, for a list of jobs in one launch.  A `JobList` holds what is static about a call: per job the header's
(dz_row, m, x_row, k, dw_row, dw_col0) as a filled SrMlpGradJob array, and the chunk limit that follows from the strides
(`job_list(fields)` caches one per field tuple).  `run` adds the addresses and the output tensors and owns the protocol:

* The kernel addresses its operands with 32-bit byte offsets and refuses n * row * 4 >= 2^31, so more than `chunk_limit` points
  are cut into chunks: chunk `lo` reads dz + 4 lo dz_row and x + 4 lo x_row.  The first chunk writes into the caller's tensors,
  later chunks into temporaries that are added in chunk order (deterministic) -- of dw only the block [:m, dw_col0:dw_col0 + k]
  of each job: several jobs may write column blocks of one dw tensor, and columns no job writes are never read.
* A job list the library refuses (workspace size 0) is a ValueError carrying sr_last_error; nothing is launched.
* A JobList's array is shared by every call with it: filling it and launching from it happen under the list's lock.
* The extra dz row (`dz_rows`).  A job whose dz address is not the first column of its matrix (the flow head's branches, the
  view-colour head's sums) still reads whole rows of dz_row floats from there on, so the last point's row ends beyond
  [N, dz_row]: whoever allocates such a matrix allocates one row more than points."""
from __future__ import annotations

import functools
import threading
from typing import Optional, Sequence, Tuple

import torch

from . import _lib

Fields = Tuple[int, int, int, int, int, int]      # dz_row, m, x_row, k, dw_row, dw_col0
chunk_limit_override: Optional[int] = None        # tests set it to force chunking at a few hundred points; nothing in the product does


def chunk_limit(fields: Sequence[Fields]) -> int:
    """the most points of one launch: the largest multiple of 64 (never below 64) with the widest dz or x matrix below 2^31 bytes"""
    row = max(max(f[0], f[2]) for f in fields)
    return max(64, ((1 << 31) - 1) // (4 * row) // 64 * 64)


def dz_rows(n_points: int) -> int:
    """rows to allocate for a dz matrix that a job reads from a column other than its first (the module docstring's last rule)"""
    return n_points + 1


class JobList:
    def __init__(self, fields: Sequence[Fields]):
        self.fields = tuple(tuple(int(v) for v in f) for f in fields)
        if not 1 <= len(self.fields) <= _lib.MLP_MAX_GRAD_JOBS:
            raise ValueError(f"one weight-gradient launch takes 1..{_lib.MLP_MAX_GRAD_JOBS} jobs, got {len(self.fields)}")
        self.array = (_lib.SrMlpGradJob * len(self.fields))()
        self.structs = list(self.array)          # views of the array's entries: no indexing per call
        for J, f in zip(self.structs, self.fields):
            J.dz_row, J.m, J.x_row, J.k, J.dw_row, J.dw_col0 = f
        self.steps = [(4 * f[0], 4 * f[2]) for f in self.fields]      # bytes per point of dz and of x
        self.limit = chunk_limit(self.fields)
        self.lock = threading.Lock()


@functools.lru_cache(maxsize=256)
def job_list(fields: Tuple[Fields, ...]) -> JobList:
    return JobList(fields)


def run(n_points: int, device, jobs: JobList, dz: Sequence[int], x: Sequence[int], dw: Sequence[torch.Tensor],
        db: Sequence[Optional[torch.Tensor]]) -> None:
    """dw[i][:m, dw_col0:dw_col0 + k] = dz_i^T x_i and db[i] = column sums of dz_i (where given) over `n_points` points, for
    every job i; dz[i], x[i]: the addresses of point 0."""
    lib = _lib.load()
    limit = chunk_limit_override or jobs.limit
    arr, n_jobs = jobs.array, len(jobs.fields)
    if not len(dz) == len(x) == len(dw) == len(db) == n_jobs:      # a shorter list would launch an earlier call's addresses
        raise ValueError(f"{n_jobs} jobs take {n_jobs} dz and x addresses and dw and db entries")
    out_dw, out_db = dw, db
    for lo in range(0, n_points, limit):
        cnt = min(limit, n_points - lo)
        if lo:
            fresh = {id(t): torch.empty_like(t) for t in out_dw}
            dw = [fresh[id(t)] for t in out_dw]
            db = [None if t is None else torch.empty_like(t) for t in out_db]
        with jobs.lock:
            for J, (dz_step, x_step), z, xx, w, b in zip(jobs.structs, jobs.steps, dz, x, dw, db):
                J.dz, J.x, J.dw, J.db = z + lo * dz_step, xx + lo * x_step, w.data_ptr(), (None if b is None else b.data_ptr())
            ws_bytes = lib.sr_mlp_weight_grad_workspace(cnt, n_jobs, arr)
            if ws_bytes == 0:
                raise ValueError("unsupported weight-gradient job list: " + lib.sr_last_error().decode("utf-8", "replace"))
            ws = torch.empty(ws_bytes // 4, dtype=torch.float32, device=device)
            with torch.cuda.device(device):
                _lib.check(lib.sr_mlp_weight_grad(cnt, n_jobs, arr, _lib.ptr(ws), ws_bytes, _lib.stream(device)))
        if lo:
            for i, (_, m, _, k, _, c0) in enumerate(jobs.fields):
                out_dw[i][:m, c0:c0 + k].add_(dw[i][:m, c0:c0 + k])
                if db[i] is not None:
                    out_db[i].add_(db[i])
