"""The host-side bookkeeping of the rasterizer facade, without a device: what a launch is promised and what a finished forward
teaches (`rasterizer._Estimates`: plan / record), the ticket of an asynchronous launch (`_Pending.resolve` repeats its outcome)
and the render-redeem-render-again helper (`redeemed`).  The library is replaced by stubs: nothing is launched."""
from types import SimpleNamespace

import pytest

from splatfields_amd import rasterizer as rz

N, H, W = 30_000, 96, 160
KEY = (0, N, H, W)


def _view(**seen):
    return SimpleNamespace(seen=dict(seen))


def test_plan_and_record_rules(monkeypatch):
    monkeypatch.setattr(rz, "LAST_INSTANCES", 0)
    est, view = rz._Estimates(), _view()
    # unknown size, no ratio for this image size: four instances per splat, at least 65536; nothing to launch asynchronously on
    p = est.plan(0, N, H, W, view, may_async=True)
    assert p == rz._Promise(KEY, max(4 * N, 1 << 16)) and p.hint is None
    assert est.plan(0, 100, H, W, view, True).capacity == 1 << 16
    assert not est.capacity and not est.per_splat and not view.seen       # plan writes nothing

    # record: all four updates
    est.record(p, view, 210_000, 900)
    assert est.capacity == {KEY: rz._round_capacity(210_000)}
    assert est.per_splat == {(0, H, W): 7.0}
    assert view.seen == {N: (210_000, 900)}
    assert rz.LAST_INSTANCES == 210_000

    # known size: its stored capacity; the camera is known with this count: ticketed, list hint with 25 % headroom
    p = est.plan(0, N, H, W, view, may_async=True)
    assert p == rz._Promise(KEY, rz._round_capacity(210_000), hint=int(900 * 1.25) + 1, expected=900, covered=2048)
    # ... unless the caller may not launch asynchronously, or the camera has not been rendered with this count
    assert est.plan(0, N, H, W, view, may_async=False) == rz._Promise(KEY, rz._round_capacity(210_000))
    assert est.plan(0, N, H, W, _view(), may_async=True).hint is None
    # another device or image size knows nothing of it
    assert est.plan(1, N, H, W, view, True).capacity == 4 * N and est.plan(0, N, H, W + 16, view, True).capacity == 4 * N

    # unknown size with a ratio for this image size (the cloud was densified): ratio * n with the usual headroom
    n2 = 3 * N
    p2 = est.plan(0, n2, H, W, view, may_async=True)
    assert p2 == rz._Promise((0, n2, H, W), rz._round_capacity(int(7.0 * n2)))

    # estimates only grow; LAST_INSTANCES and the camera's record follow the latest forward
    est.record(p, view, 150_000, 700)
    assert est.capacity[KEY] == rz._round_capacity(210_000) and est.per_splat[(0, H, W)] == 7.0
    assert view.seen[N] == (150_000, 700) and rz.LAST_INSTANCES == 150_000
    est.record(p, view, 600_000, 3000)
    assert est.capacity[KEY] == rz._round_capacity(600_000) and est.per_splat[(0, H, W)] == 20.0
    p = est.plan(0, N, H, W, view, True)
    assert (p.hint, p.expected, p.covered) == (3751, 3000, 4096)
    # a forward that could not report its longest list (< 0) leaves the camera's record alone
    est.record(p, view, 630_000, -1)
    assert view.seen[N] == (600_000, 3000) and rz.LAST_INSTANCES == 630_000

    # stale `seen`: the camera's record needs more than the capacity the table holds for this size -> wait
    est.capacity[KEY] = rz._round_capacity(60_000)                        # "only a small cloud was ever seen"
    assert est.plan(0, N, H, W, view, True) == rz._Promise(KEY, rz._round_capacity(60_000))
    view.seen[N] = (60_000, 3000)
    assert est.plan(0, N, H, W, view, True).hint == 3751


def test_hint_to_covered_sort_classes():
    """the same mapping as csrc/api.hip: covered_by_hint (there -1 stands for "all")"""
    got = [rz._covered_by_hint(h) for h in (0, 1, 2048, 2049, 4096, 4097, 8192, 8193, 10 ** 9)]
    assert got == [2048, 2048, 2048, 4096, 4096, 8192, 8192, 1 << 62, 1 << 62]


def test_tables_stay_bounded(monkeypatch):
    monkeypatch.setattr(rz, "LAST_INSTANCES", 0)
    est, view = rz._Estimates(), _view()
    for n in range(1, 3 * est.CAPACITY_ROWS):                             # a long run: the splat count changes every few steps
        est.record(est.plan(0, n, H, W, view, True), view, 5 * n, 10)
        assert len(est.capacity) <= est.CAPACITY_ROWS and len(view.seen) <= est.SEEN_ROWS + 1
    assert view.seen[n] == (5 * n, 10)                                    # the latest record survives the pruning of `seen`
    assert len(est.per_splat) == 1


class _StubLib:
    """sr_ticket_wait / sr_ticket_release of a library that is not there: answers from a list, counts the calls."""

    def __init__(self, *answers):
        self.answers, self.waits, self.released = list(answers), 0, []

    def sr_ticket_wait(self, ticket, inst_ref, longest_ref):
        self.waits += 1
        rc, inst, longest = self.answers.pop(0)
        inst_ref._obj.value, longest_ref._obj.value = inst, longest
        return rc

    def sr_ticket_release(self, ticket):
        self.released.append(ticket)
        return 0


def _pending(lib, view, capacity=1 << 16, hint=1000, ticket=1):
    return rz._Pending(lib, ticket, rz._Promise(KEY, capacity, hint, 800, rz._covered_by_hint(hint)), view)


def test_resolve_repeats_a_failed_wait(monkeypatch):
    monkeypatch.setattr(rz, "_ESTIMATES", rz._Estimates())
    lib, view = _StubLib((1, 0, 0)), _view()
    p = _pending(lib, view)
    with pytest.raises(RuntimeError, match="libsplatraster") as first:
        p.resolve()
    with pytest.raises(RuntimeError) as second:                           # not `None` for an instance count
        p.resolve()
    assert second.value is first.value and not isinstance(first.value, rz.RasterizerOverflow)
    assert lib.waits == 1 and p.ticket is None                            # a ticket is redeemed once
    assert not rz._ESTIMATES.capacity and not view.seen                   # nothing was learned from it
    del p
    assert lib.released == []


def test_resolve_repeats_its_count_or_its_overflow(monkeypatch):
    monkeypatch.setattr(rz, "_ESTIMATES", rz._Estimates())
    monkeypatch.setattr(rz, "LAST_INSTANCES", 0)
    view = _view()
    lib = _StubLib((0, 40_000, 900))
    p = _pending(lib, view)
    assert p.resolve() == 40_000 and p.resolve() == 40_000 and lib.waits == 1
    assert view.seen[N] == (40_000, 900) and rz.LAST_INSTANCES == 40_000
    # more instances than the capacity promised
    lib = _StubLib((0, 300_000, 900))
    p = _pending(lib, view)
    with pytest.raises(rz.RasterizerOverflow, match="re-run the step") as first:
        p.resolve()
    with pytest.raises(rz.RasterizerOverflow, match="no result") as second:
        p.resolve()
    assert second.value is first.value and lib.waits == 1
    assert rz._ESTIMATES.capacity[KEY] == rz._round_capacity(300_000)     # corrected before it raised
    # a list longer than the launched sort classes cover
    lib = _StubLib((0, 40_000, 5000))
    with pytest.raises(rz.RasterizerOverflow, match="a list of 5000"):
        _pending(lib, view).resolve()
    assert view.seen[N] == (40_000, 5000)
    # a dropped forward hands its ticket back
    lib = _StubLib()
    p = _pending(lib, view, ticket=77)
    del p
    assert lib.released == [77]


def test_redeemed_renders_once_more_after_an_overflow(monkeypatch):
    monkeypatch.setattr(rz, "_ESTIMATES", rz._Estimates())
    prev = rz.set_async_forward(None)
    try:
        for scope in (True, False):
            view = _view()
            lib = _StubLib((0, 300_000, 900), (0, 300_000, 900))          # the first launch was promised 65536 instances
            calls, keep = [], []

            def render_fn():
                calls.append(rz.async_forward_enabled())
                capacity = rz._ESTIMATES.capacity.get(KEY, 1 << 16)
                keep.append(_pending(lib, view, capacity=capacity))       # (the autograd ctx holds it in a real forward)
                return len(calls)

            assert rz.redeemed(render_fn, scope=scope) == 2               # the second result
            assert calls == [scope, scope] and lib.waits == 2
            assert not rz.async_forward_enabled()
            monkeypatch.setattr(rz, "_ESTIMATES", rz._Estimates())
        # nothing overflows: one call
        calls = []
        assert rz.redeemed(lambda: calls.append(1) or "out") == "out" and calls == [1]
        # an overflow of the second render is the caller's to see
        lib, keep = _StubLib((0, 300_000, 900), (0, 600_000, 900)), []

        def always_short():
            keep.append(_pending(lib, _view()))
            return None

        with pytest.raises(rz.RasterizerOverflow):
            rz.redeemed(always_short)
        assert len(keep) == 2
    finally:
        rz.set_async_forward(prev)
        keep.clear()


def test_settings_from_camera_is_the_mapping_render_builds():
    """`settings_from_camera` is the one product-side mapping from a reference camera object to the settings tuple: field for
    field what `render.render` / `render_model` wrote out by hand (gaussian_renderer/__init__.py:59-72)."""
    import math
    import torch
    cam = SimpleNamespace(image_height=torch.tensor(96), image_width=160.0, FoVx=0.9, FoVy=0.6, world_view_transform=torch.eye(4),
                          full_proj_transform=torch.ones(4, 4), camera_center=torch.tensor([1.0, 2.0, 3.0]))
    bg = torch.ones(3)
    for kw, scale, debug in (({}, 1.0, False), ({"scale_modifier": 0.5, "debug": 1}, 0.5, True)):
        rs = rz.settings_from_camera(cam, bg, 2, **kw)
        by_hand = rz.GaussianRasterizationSettings(
            image_height=int(cam.image_height), image_width=int(cam.image_width), tanfovx=math.tan(cam.FoVx * 0.5),
            tanfovy=math.tan(cam.FoVy * 0.5), bg=bg, scale_modifier=scale, viewmatrix=cam.world_view_transform,
            projmatrix=cam.full_proj_transform, sh_degree=2, campos=cam.camera_center, prefiltered=False, debug=debug)
        assert rs._fields == by_hand._fields
        for name, a, b in zip(rs._fields, rs, by_hand):
            assert (a is b) if torch.is_tensor(b) else (type(a) is type(b) and a == b), name
