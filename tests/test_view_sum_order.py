"""The assumption sr_sum_views is built on, as a test: when V custom autograd nodes share one input, PyTorch runs the node created
last first, and the gradient the input ends up with is ((g[V-1] + g[V-2]) + ...) + g[0] bit for bit -- the left fold from the last
view to the first.  From V = 3 on that differs from the ascending fold, so the order is not a matter of taste.  CPU only."""
import pytest
import torch


class _View(torch.autograd.Function):
    """Stands for one view's rasterizer node: its output does not depend on the input's value, its backward hands the shared input a
    fixed gradient of its own and records when it ran."""

    @staticmethod
    def forward(ctx, x, grad, log, v):
        ctx.grad, ctx.log, ctx.v = grad, log, v
        return x.new_zeros(()) + float(v)

    @staticmethod
    def backward(ctx, upstream):
        ctx.log.append((ctx.v, upstream.detach().clone()))
        return ctx.grad * upstream, None, None, None


def _grads(V, n=4099, seed=0):
    g = torch.Generator().manual_seed(seed + V)
    # magnitudes spread over six decades: almost every element's sum depends on the association
    return [torch.randn(n, generator=g) * 10.0 ** torch.randint(-3, 4, (n,), generator=g).float() for _ in range(V)]


def descending_fold(grads):
    acc = grads[-1]
    for g in reversed(grads[:-1]):
        acc = acc + g
    return acc


def ascending_fold(grads):
    acc = grads[0]
    for g in grads[1:]:
        acc = acc + g
    return acc


@pytest.mark.parametrize("loss_form", ["sum_over_V", "stack_mean"])
@pytest.mark.parametrize("leaf", [True, False], ids=["leaf", "non_leaf"])
@pytest.mark.parametrize("V", [2, 3, 5, 8, 17])
def test_autograd_accumulates_the_views_last_to_first(V, leaf, loss_form):
    grads = _grads(V)
    base = torch.zeros(grads[0].numel(), requires_grad=True)
    x = base if leaf else base * 1.0
    if not leaf:
        x.retain_grad()
    log = []
    losses = [_View.apply(x, grads[v], log, v) for v in range(V)]
    loss = sum(losses) / V if loss_form == "sum_over_V" else torch.stack(losses).mean()
    loss.backward()
    assert [v for v, _ in log] == list(range(V - 1, -1, -1))    # the node created last ran first
    ups = [u for _, u in log]
    assert all(torch.equal(u, ups[0]) for u in ups) and abs(ups[0].item() * V - 1.0) < 1e-6   # every view got the same 1/V
    scaled = [g * ups[0] for g in grads]                        # what each node handed the shared input
    want = descending_fold(scaled)
    assert torch.equal(x.grad, want)
    if not leaf:
        assert torch.equal(base.grad, want)                     # `* 1.0` hands the sum on unchanged
    if V >= 3:
        assert not torch.equal(ascending_fold(scaled), want)    # the other order gives other bits


def test_descending_fold_in_chunks_of_sixteen_keeps_the_association():
    """what sr_sum_views does for more than SR_SUM_MAX_VIEWS views: the last 16 first, then the rest onto the partial sum"""
    grads = _grads(17)
    partial = descending_fold(grads[1:])
    assert torch.equal(partial + grads[0], descending_fold(grads))
    grads = _grads(40)
    acc = descending_fold(grads[24:])
    for lo, hi in ((8, 24), (0, 8)):
        for g in reversed(grads[lo:hi]):
            acc = acc + g
    assert torch.equal(acc, descending_fold(grads))
