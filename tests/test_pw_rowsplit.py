"""row_split(): (m[:, :a], m[:, a:]) whose backward receives both slice
gradients at once.  On the CPU only the concatenating fallback exists; it
must be indistinguishable from plain slicing."""

import pytest
import torch

from pvraft_amd.model.pointwise import _RowSplit, _SlabHolder, row_split


def _m(B=2, C=7, S=5, seed=0):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(B, C, S, dtype=torch.float64, generator=g).requires_grad_()


@pytest.mark.parametrize("a", [1, 3, 6])
def test_forward_is_slicing(a):
    m = _m()
    lo, hi = row_split(m, a)
    assert torch.equal(lo, m[:, :a]) and torch.equal(hi, m[:, a:])


@pytest.mark.parametrize("a", [1, 4])
def test_both_gradients_match_slicing(a):
    m = _m()
    w1 = torch.randn(2, a, 5, dtype=torch.float64)
    w2 = torch.randn(2, 7 - a, 5, dtype=torch.float64)

    def loss(lo, hi):
        return (lo * w1).sum() + (hi.sin() * w2).sum()

    (g_new,) = torch.autograd.grad(loss(*row_split(m, a)), m)
    (g_ref,) = torch.autograd.grad(loss(m[:, :a], m[:, a:]), m)
    assert torch.equal(g_new, g_ref)
    assert torch.autograd.gradcheck(lambda t: row_split(t, a), (m,))


@pytest.mark.parametrize("side", [0, 1])
def test_one_side_unused(side):
    a = 3
    m = _m()
    (g_new,) = torch.autograd.grad(row_split(m, a)[side].cos().sum(), m)
    ref = (m[:, :a], m[:, a:])[side]
    (g_ref,) = torch.autograd.grad(ref.cos().sum(), m)
    assert torch.equal(g_new, g_ref)
    assert torch.autograd.gradcheck(lambda t: row_split(t, a)[side], (m,))


def test_gradients_that_are_not_slab_views():
    # a holder whose buffer was never written by anyone: the gradients come
    # from elsewhere and must go through the cat, not be replaced by the
    # buffer
    a = 2
    m = _m()
    holder = _SlabHolder(m.shape[1])
    holder.buf = torch.full_like(m.detach(), 123.0)
    holder.filled = {0, a}
    lo, hi = _RowSplit.apply(m, a, holder)
    (g_new,) = torch.autograd.grad((lo * 2).sum() + (hi * 3).sum(), m)
    exp = torch.cat([torch.full((2, a, 5), 2.0), torch.full((2, 7 - a, 5), 3.0)], 1)
    assert torch.equal(g_new, exp.double())
    assert holder.buf is None and not holder.filled


def test_slab_views_return_the_buffer_itself():
    # the fast path's contract, exercised by hand: both incoming gradients
    # ARE the buffer's row blocks -> the buffer is the gradient
    a = 2
    m = _m()
    holder = _SlabHolder(m.shape[1])
    lo, hi = _RowSplit.apply(m, a, holder)
    buf, _ = holder.rows(0, torch.empty(2, a, 5, dtype=torch.float64))
    holder.rows(a, torch.empty(2, 7 - a, 5, dtype=torch.float64))
    buf.copy_(torch.arange(70, dtype=torch.float64).view(2, 7, 5))
    (g,) = torch.autograd.grad([lo, hi], m, [buf[:, :a], buf[:, a:]])
    assert g.data_ptr() == buf.data_ptr()
    assert torch.equal(g, torch.arange(70, dtype=torch.float64).view(2, 7, 5))
    # only one block written -> no fast path
    m2 = _m()
    h2 = _SlabHolder(7)
    lo2, hi2 = _RowSplit.apply(m2, a, h2)
    b2, _ = h2.rows(0, torch.empty(2, a, 5, dtype=torch.float64))
    b2.fill_(1.0)
    (g2,) = torch.autograd.grad([lo2, hi2], m2, [b2[:, :a], b2[:, a:] * 2])
    assert g2.data_ptr() != b2.data_ptr()
    assert torch.equal(g2[:, :a], torch.ones(2, a, 5).double())
    assert torch.equal(g2[:, a:], torch.full((2, 7 - a, 5), 2.0).double())


def test_double_use_in_one_graph():
    m = _m()

    def f(split):
        lo1, hi1 = split(m, 3)
        mid = torch.cat([hi1 * 2, lo1.exp()], dim=1)  # (B, 7, S) again
        lo2, hi2 = split(mid, 5)
        return (lo2.sin().sum() + (hi2 ** 2).sum() + lo1.sum())

    (g_new,) = torch.autograd.grad(f(row_split), m)
    (g_ref,) = torch.autograd.grad(f(lambda t, a: (t[:, :a], t[:, a:])), m)
    assert torch.equal(g_new, g_ref)

    def chain(t):
        lo1, hi1 = row_split(t, 3)
        mid = torch.cat([hi1 * 2, lo1.exp()], dim=1)
        return row_split(mid, 5)

    assert torch.autograd.gradcheck(chain, (m,))


def test_conv_gru_cpu_gradients_unchanged_by_row_split(monkeypatch):
    # the GRU cell on the CPU path: gradients with row_split equal those
    # with the two plain slices it replaced
    from pvraft_amd.model import pointwise
    from pvraft_amd.model import update

    torch.manual_seed(0)
    gru = update.ConvGRU(input_dim=10, hidden_dim=4).double()
    h = torch.randn(2, 4, 9, dtype=torch.float64, requires_grad=True)
    xs = [torch.randn(2, 6, 9, dtype=torch.float64, requires_grad=True),
          torch.randn(2, 4, 9, dtype=torch.float64, requires_grad=True)]

    def grads():
        out = gru.forward_parts(h, xs)
        return torch.autograd.grad(out.square().sum(), [h, *xs, *gru.parameters()])

    g_new = grads()
    monkeypatch.setattr(pointwise, "row_split",
                        lambda m, a: (m[:, :a], m[:, a:]))
    g_ref = grads()
    for x, y in zip(g_new, g_ref):
        assert torch.equal(x, y)
