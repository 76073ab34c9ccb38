"""The collectives a view-parallel step issues, pinned: which collective, with which reduce op, dtype and element count, in which
order, and where every tensor sits inside a packed buffer.  Every rank must issue the same sequence, and with more than two
ranks the position of an element in a buffer can decide the order its contributions are summed in, so a change of this list is
a change of results.  A 1-rank gloo group with view_parallel.FORCE_COLLECTIVES runs the calls for real on the CPU (the steps
that need the rasterizer are pinned the same way in tests/test_gpu_rccl_single_rank.py)."""
import socket

import pytest
import torch
import torch.distributed as dist

from splatfields_amd import view_parallel as vp
from tests.helpers import record_collectives

F32, F64 = torch.float32, torch.float64


@pytest.fixture()
def forced_gloo_group():
    s = socket.socket(); s.bind(("127.0.0.1", 0)); port = s.getsockname()[1]; s.close()
    dist.init_process_group("gloo", init_method=f"tcp://127.0.0.1:{port}", rank=0, world_size=1)
    old = vp.FORCE_COLLECTIVES, vp.PACK_BELOW_BYTES
    vp.FORCE_COLLECTIVES, vp.PACK_BELOW_BYTES = True, 1024
    yield
    vp.FORCE_COLLECTIVES, vp.PACK_BELOW_BYTES = old
    dist.destroy_process_group()


def _is_segment(t: torch.Tensor, flat: torch.Tensor, offset: int) -> bool:
    """t is a view of flat[offset : offset + t.numel()]"""
    return t.untyped_storage().data_ptr() == flat.untyped_storage().data_ptr() and t.is_contiguous() \
        and t.storage_offset() == flat.storage_offset() + offset


def _params():
    """two tensors at or above the packing threshold (1024 B), small ones of two dtypes interleaved, one without a gradient, and
    an SH tensor of which only the 4 leading coefficients are active"""
    shapes = {"a": ((100, 3), F32), "b": ((10,), F32), "c": ((5,), F64), "d": ((4,), F32), "e": ((3,), F64), "big2": ((200, 3), F32),
              "shs": ((50, 16, 3), F32)}
    g = torch.Generator().manual_seed(5)
    p = {k: torch.nn.Parameter(torch.zeros(shape, dtype=dt)) for k, (shape, dt) in shapes.items()}
    for k, t in p.items():
        if k != "d":
            t.grad = torch.randn(t.shape, generator=g, dtype=F64).to(t.dtype)
    p["shs"].grad[:, 4:] = 0
    return p


@pytest.mark.parametrize("restore_none", [False, True])
def test_allreduce_gradients_sequence_and_layout(forced_gloo_group, restore_none):
    p = _params()
    before = {k: t.grad.clone() for k, t in p.items() if t.grad is not None}
    with record_collectives() as log:
        vp.allreduce_gradients(list(p.values()), 1, sh_param=p["shs"], sh_active_coeffs=4, restore_none=restore_none)
    # the large ones alone, largest first; the active SH bands; one packed buffer per dtype in first-seen order; the flags
    expected = [("all_reduce", "SUM", F32, 600), ("all_reduce", "SUM", F32, 300), ("all_reduce", "SUM", F32, 50 * 4 * 3),
                ("all_reduce", "SUM", F32, 10 + 4), ("all_reduce", "SUM", F64, 5 + 3)]
    if restore_none:
        expected.append(("all_reduce", "SUM", F32, 7))
    assert list(log) == expected
    assert log.tensors[0] is p["big2"].grad and log.tensors[1] is p["a"].grad          # in place, no packing copy
    flat32, flat64 = log.tensors[3], log.tensors[4]
    assert _is_segment(p["b"].grad, flat32, 0) and _is_segment(p["c"].grad, flat64, 0) and _is_segment(p["e"].grad, flat64, 5)
    if restore_none:
        assert p["d"].grad is None
        assert log.tensors[5].tolist() == [1.0, 1.0, 1.0, 0.0, 1.0, 1.0, 1.0]
    else:
        assert _is_segment(p["d"].grad, flat32, 10) and (p["d"].grad == 0).all()
    for k, g in before.items():   # the mean over one rank
        assert torch.equal(p[k].grad, g) and p[k].grad.shape == g.shape, k


def test_view_parallel_step_sequence_and_layout(forced_gloo_group):
    # p0 is at the threshold, p2 is not of the loss's dtype: both go alone; p1, p3 (unused: zeros) and the loss share a buffer
    params = [torch.ones(40, 4, dtype=F64).requires_grad_(True), torch.ones(6, dtype=F64).requires_grad_(True),
              torch.ones(5, dtype=F32).requires_grad_(True), torch.ones(2, dtype=F64).requires_grad_(True)]

    def render_loss(view):
        return (view + 1.0) * (params[0].sum() + 2.0 * params[1].sum() + 3.0 * params[2].double().sum())

    with record_collectives() as log:
        loss = vp.view_parallel_step(params, [0, 1], render_loss)
    assert list(log) == [("all_reduce", "SUM", F64, 160), ("all_reduce", "SUM", F32, 5), ("all_reduce", "SUM", F64, 6 + 2 + 1)]
    assert log.tensors[0] is params[0].grad and log.tensors[1] is params[2].grad
    flat = log.tensors[2]
    assert _is_segment(params[1].grad, flat, 0) and _is_segment(params[3].grad, flat, 6) and _is_segment(loss, flat, 8)
    assert loss.shape == () and loss.item() == 1.5 * (160 + 12 + 15)
    assert torch.equal(params[0].grad, torch.full((40, 4), 1.5, dtype=F64)) and torch.equal(params[1].grad, torch.full((6,), 3.0, dtype=F64))
    assert torch.equal(params[2].grad, torch.full((5,), 4.5)) and torch.equal(params[3].grad, torch.zeros(2, dtype=F64))


def test_field_view_parallel_step_sequence_and_layout(forced_gloo_group):
    w = torch.ones(3, dtype=F64, requires_grad=True)
    seen = {}

    def compute_splats():
        seen["out"] = {"means3D": w * torch.ones(7, 3, dtype=F64), "rgb": (w.sum() * torch.ones(7, 2, dtype=F64)).to(F32), "frame": 3}
        return seen["out"]

    def render_loss(s, view):
        assert s["frame"] == 3
        return (view + 1.0) * (s["means3D"].sum() + s["rgb"].double().sum())

    with record_collectives() as log:
        loss = vp.field_view_parallel_step(compute_splats, [0, 1], render_loss)
    # ONE buffer in the dtype of the first attribute: the attribute gradients in dict order, the loss last
    assert list(log) == [("all_reduce", "SUM", F64, 21 + 14 + 1)]
    assert _is_segment(loss, log.tensors[0], 35) and loss.item() == 1.5 * (21 + 3 * 14)
    assert torch.equal(log.tensors[0][:35], torch.full((35,), 1.5, dtype=F64))
    assert torch.equal(w.grad, torch.full((3,), 1.5 * 7 + 1.5 * 14, dtype=F64))
