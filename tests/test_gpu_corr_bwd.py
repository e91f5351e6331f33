"""Truncated-correlation backward without the composed chain
(csrc/corr_bwd.hip): corr_grad_expand, corr_gather_xyz, and _CorrTruncate
end to end against PVRAFT_CORR_BWD=classic.

corr_grad_expand and corr_gather_xyz only move and round values, so they
are held to torch.equal against the ATen composition.  fmap2.grad comes from
the same matrix bits through the same GEMM: torch.equal.  fmap1.grad comes
through a GEMM with another operand layout, so its summation order may
differ: both paths are compared with a float64 product of the same
bf16-rounded operands, and the new path's deviation may be at most twice the
classic path's largest on the same input, with a floor of one bf16 ulp of
the float64 value (both are bf16 roundings of fp32 sums).
"""

import math

import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = "cuda"

EXPAND_SHAPES = [
    (2, 70, 300, 64),     # rows not 16-byte aligned on odd n
    (1, 5, 301, 7),       # odd M
    (2, 33, 8192, 512),   # flagship row length, N no multiple of a row tile
    (1, 3, 96, 96),       # K = M, no zero survives
    (1, 4, 64, 1),        # K = 1
    (1, 2, 32768, 16),    # largest supported row (bf16 only)
]


def _C():
    from pvraft_amd import _C

    return _C


def _topk_idx(B, N, M, K):
    return torch.rand(B, N, M, device=DEV).topk(K, dim=2).indices.to(torch.int32)


def _scatter_ref(g, idx, scale, M, dt):
    B, N, _ = g.shape
    return torch.zeros(B, N, M, dtype=dt, device=g.device).scatter_(
        2, idx.long(), (g * scale).to(dt)
    )


def _bits(x):
    return x.view(torch.int16) if x.dtype == torch.bfloat16 else x.view(torch.int32)


@pytest.mark.parametrize(
    "B,N,M,K,dt",
    [s + (torch.bfloat16,) for s in EXPAND_SHAPES]
    # the row image is 64 KB: fp32 rows end at 16384
    + [s + (torch.float32,) for s in EXPAND_SHAPES if s[2] <= 16384],
)
def test_expand_matches_scatter(B, N, M, K, dt):
    idx = _topk_idx(B, N, M, K)
    g = torch.randn(B, N, K, device=DEV)
    scale = 1.0 / math.sqrt(128)
    out = _C().corr_grad_expand(g, idx, scale, M, dt == torch.bfloat16)
    ref = _scatter_ref(g, idx, scale, M, dt)
    assert out.dtype == dt and out.shape == ref.shape
    assert torch.equal(out, ref)
    assert torch.equal(_bits(out), _bits(ref))


@pytest.mark.parametrize("dt", [torch.bfloat16, torch.float32], ids=["bf16", "fp32"])
def test_expand_repeated_index(dt):
    """corr_topk pads with a repeated index when ties exceed its cap; both
    slots then carry the same value."""
    B, N, M, K = 1, 9, 520, 32
    idx = _topk_idx(B, N, M, K)
    g = torch.randn(B, N, K, device=DEV)
    idx[:, :, K - 1] = idx[:, :, 0]
    g[:, :, K - 1] = g[:, :, 0]
    idx[:, 3, 5] = idx[:, 3, 4]
    g[:, 3, 5] = g[:, 3, 4]
    scale = 1.0 / math.sqrt(64)
    out = _C().corr_grad_expand(g, idx, scale, M, dt == torch.bfloat16)
    assert torch.equal(out, _scatter_ref(g, idx, scale, M, dt))


@pytest.mark.parametrize("dt", [torch.bfloat16, torch.float32], ids=["bf16", "fp32"])
def test_expand_zero_row_is_plus_zero(dt):
    B, N, M, K = 1, 6, 1000, 40
    idx = _topk_idx(B, N, M, K)
    g = torch.randn(B, N, K, device=DEV)
    g[:, 2] = 0.0
    out = _C().corr_grad_expand(g, idx, 0.125, M, dt == torch.bfloat16)
    ref = _scatter_ref(g, idx, 0.125, M, dt)
    assert torch.equal(_bits(out), _bits(ref))
    assert bool((_bits(out[:, 2]) == 0).all())  # +0 in every element


def _offset_view(t, elems):
    """Contiguous copy of t whose storage starts `elems` elements into an
    allocation, so its base is not 16-byte aligned."""
    buf = torch.empty(t.numel() + elems, dtype=t.dtype, device=t.device)
    v = buf[elems:].view(t.shape)
    v.copy_(t)
    assert v.is_contiguous() and v.data_ptr() % 16 != 0
    return v


def test_unaligned_bases_take_the_narrow_loads():
    """g / idx given as contiguous views 4 and 8 bytes into an allocation:
    the 16-byte row loads must not be used, results stay equal."""
    B, N, M, K = 2, 7, 520, 64
    idx = _topk_idx(B, N, M, K)
    g = torch.randn(B, N, K, device=DEV)
    xyz2 = torch.randn(B, M, 3, device=DEV)
    ref = _scatter_ref(g, idx, 0.125, M, torch.bfloat16)
    ref_xyz = _C().corr_gather_xyz(idx, xyz2)
    for g_v, i_v in ((_offset_view(g, 1), idx), (g, _offset_view(idx, 2)),
                     (_offset_view(g, 3), _offset_view(idx, 1))):
        out = _C().corr_grad_expand(g_v, i_v, 0.125, M, True)
        assert torch.equal(_bits(out), _bits(ref))
    out_xyz = _C().corr_gather_xyz(_offset_view(idx, 1), _offset_view(xyz2, 1))
    assert torch.equal(out_xyz, ref_xyz)


def test_expand_rejects_rows_above_the_lds_image():
    idx = torch.zeros(1, 1, 4, dtype=torch.int32, device=DEV)
    g = torch.zeros(1, 1, 4, device=DEV)
    with pytest.raises(RuntimeError):
        _C().corr_grad_expand(g, idx, 1.0, 32769, True)
    with pytest.raises(RuntimeError):
        _C().corr_grad_expand(g, idx, 1.0, 16385, False)


def test_backward_above_row_limit_takes_classic_path(monkeypatch):
    """fp32 rows above 16384 do not fit the LDS image: the op must not
    launch corr_grad_expand there, must give what PVRAFT_CORR_BWD=classic
    gives, and both gradients must agree with a float64 product of the
    scattered gradient.  Bound: a g1 element sums K = 8 products and a g2
    element at most N = 4, each operand pair rounded once more by the
    `g * scale` in fp32, so 16 * 2^-24 * sum|a||b| covers an fp32
    accumulation in any order."""
    from pvraft_amd import ops

    B, N, M, C, K = 1, 4, 16392, 32, 8
    f1 = torch.randn(B, C, N, device=DEV)
    f2 = torch.randn(B, C, M, device=DEV)
    xyz2 = torch.randn(B, M, 3, device=DEV)
    g = torch.randn(B, N, K, device=DEV)

    def no_expand(*args, **kw):
        raise AssertionError("corr_grad_expand launched above the row limit")

    monkeypatch.setattr(_C(), "corr_grad_expand", no_expand)
    res = {}
    for mode in ("", "classic"):
        monkeypatch.setenv("PVRAFT_CORR_BWD", mode)
        a = f1.clone().requires_grad_(True)
        b = f2.clone().requires_grad_(True)
        corr, idx, txyz = ops.corr_truncate(a, b, xyz2, K)
        corr.backward(g)
        res[mode] = (corr.detach(), idx, txyz.detach(), a.grad, b.grad)
    for x, y in zip(res[""], res["classic"]):
        assert torch.equal(x, y)

    _, idx, _, g1, g2 = res[""]
    gfull = torch.zeros(B, N, M, dtype=torch.float64, device=DEV).scatter_(
        2, idx.long(), g.double() / math.sqrt(C)
    )
    f1d, f2d = f1.double(), f2.double()
    ref1 = torch.bmm(f2d, gfull.transpose(1, 2))
    ref2 = torch.bmm(f1d, gfull)
    tol1 = 16 * 2.0 ** -24 * torch.bmm(f2d.abs(), gfull.abs().transpose(1, 2))
    tol2 = 16 * 2.0 ** -24 * torch.bmm(f1d.abs(), gfull.abs())
    print(f"g1 max err {float((g1 - ref1).abs().max()):.3g}, "
          f"g2 max err {float((g2 - ref2).abs().max()):.3g}")
    assert bool(((g1 - ref1).abs() <= tol1).all())
    assert bool(((g2 - ref2).abs() <= tol2).all())


@pytest.mark.parametrize("B,N,M,K", [(2, 70, 300, 64), (1, 33, 8192, 512)])
def test_gather_xyz_matches_aten(B, N, M, K):
    idx = _topk_idx(B, N, M, K)
    xyz2 = torch.randn(B, M, 3, device=DEV)
    out = _C().corr_gather_xyz(idx, xyz2)
    ref = xyz2.gather(
        1, idx.long().reshape(B, N * K).unsqueeze(-1).expand(B, N * K, 3)
    ).view(B, N, K, 3)
    assert out.shape == ref.shape
    assert torch.equal(out, ref)


# --------------------------------------------------------------------------
# _CorrTruncate end to end
# --------------------------------------------------------------------------


def _e2e_inputs(B, N, M, C, K, seed):
    """h is a dense (B, N, M) gradient field: corr_topk hands out its set in
    no fixed slot order (it differs from call to call), so the gradient of a
    slot is taken from h at the slot's INDEX and every run of one input
    builds the same dense matrix."""
    gen = torch.Generator(device=DEV).manual_seed(seed)
    f1 = torch.randn(B, C, N, device=DEV, generator=gen).bfloat16()
    f2 = torch.randn(B, C, M, device=DEV, generator=gen).bfloat16()
    xyz2 = torch.randn(B, M, 3, device=DEV, generator=gen)
    h = torch.randn(B, N, M, device=DEV, generator=gen)
    return f1, f2, xyz2, h


def _by_index(corr, idx, txyz):
    """Slots of every row sorted by index (indices are distinct in a row)."""
    idx_s, order = idx.long().sort(dim=2)
    return (
        corr.gather(2, order),
        idx_s,
        txyz.gather(2, order.unsqueeze(-1).expand(-1, -1, -1, 3)),
    )


def _run_op(f1, f2, xyz2, h, K):
    from pvraft_amd import ops

    a = f1.clone().requires_grad_(True)
    b = f2.clone().requires_grad_(True)
    corr, idx, txyz = ops.corr_truncate(a, b, xyz2, K)
    assert idx.dtype == torch.int64
    corr.backward(h.gather(2, idx))
    return _by_index(corr.detach(), idx, txyz.detach()) + (a.grad, b.grad)


def _g1_float64(f2, h, idx, C):
    """float64 product of the bf16-rounded operands of the g1 GEMM."""
    M = h.shape[2]
    gfull = _scatter_ref(h.gather(2, idx), idx, 1.0 / math.sqrt(C), M, torch.bfloat16)
    return torch.bmm(f2.double(), gfull.double().transpose(1, 2))  # (B, C, N)


def _bf16_ulp(ref):
    e = torch.floor(torch.log2(ref.abs().clamp_min(2.0 ** -126)))
    return torch.exp2(e - 7)


def _check_g1(new, classic, ref, what):
    dev_new = (new.double() - ref).abs()
    dev_cls = float((classic.double() - ref).abs().max())
    print(f"{what}: max|g1 - f64| new {float(dev_new.max()):.6g} "
          f"classic {dev_cls:.6g} (max|f64| {float(ref.abs().max()):.4g})")
    bound = torch.maximum(torch.full_like(ref, 2.0 * dev_cls), _bf16_ulp(ref))
    bad = dev_new > bound
    assert not bool(bad.any()), (
        f"{what}: {int(bad.sum())} elements beyond the bound, "
        f"worst {float((dev_new - bound).max()):.6g}"
    )


E2E_SHAPES = [(1, 256, 300, 64, 64), (2, 512, 512, 128, 128)]


@pytest.mark.parametrize("B,N,M,C,K", E2E_SHAPES)
def test_corr_truncate_new_against_classic(B, N, M, C, K, monkeypatch):
    f1, f2, xyz2, h = _e2e_inputs(B, N, M, C, K, seed=11)
    monkeypatch.setenv("PVRAFT_CORR_BWD", "classic")
    c_corr, c_idx, c_txyz, c_g1, c_g2 = _run_op(f1, f2, xyz2, h, K)
    c_g2_again = _run_op(f1, f2, xyz2, h, K)[4]
    monkeypatch.delenv("PVRAFT_CORR_BWD")
    n_corr, n_idx, n_txyz, n_g1, n_g2 = _run_op(f1, f2, xyz2, h, K)

    assert torch.equal(n_idx, c_idx)
    assert torch.equal(n_corr, c_corr)
    assert torch.equal(n_txyz, c_txyz)
    # the parent's own GEMM, twice on the same matrix bits
    assert torch.equal(c_g2, c_g2_again), "classic bmm is not reproducible"
    assert torch.equal(n_g2, c_g2)
    ref = _g1_float64(f2, h, c_idx, C)
    _check_g1(n_g1, c_g1, ref, f"fmap1.grad {(B, N, M, C, K)}")


def test_corr_truncate_int32_index_keyword():
    from pvraft_amd import ops

    B, N, M, C, K = 1, 256, 300, 64, 64
    f1, f2, xyz2, _ = _e2e_inputs(B, N, M, C, K, seed=5)
    r64 = ops.corr_truncate(f1, f2, xyz2, K)
    r32 = ops.corr_truncate(f1, f2, xyz2, K, index_dtype=torch.int32)
    assert r64[1].dtype == torch.int64 and r32[1].dtype == torch.int32
    for x, y in zip(_by_index(*r64), _by_index(*r32)):
        assert torch.equal(x, y)


def test_corr_truncate_inside_graph(monkeypatch):
    """Forward and backward captured in one graph and replayed twice."""
    from pvraft_amd import ops

    B, N, M, C, K = E2E_SHAPES[0]
    f1, f2, xyz2, h = _e2e_inputs(B, N, M, C, K, seed=23)
    monkeypatch.setenv("PVRAFT_CORR_BWD", "classic")
    _, c_idx, _, c_g1, _ = _run_op(f1, f2, xyz2, h, K)
    monkeypatch.delenv("PVRAFT_CORR_BWD")
    e_corr, e_idx, e_txyz, e_g1, e_g2 = _run_op(f1, f2, xyz2, h, K)
    ref = _g1_float64(f2, h, c_idx, C)

    a = f1.clone().requires_grad_(True)
    b = f2.clone().requires_grad_(True)

    def step():
        corr, idx, txyz = ops.corr_truncate(a, b, xyz2, K)
        g1, g2 = torch.autograd.grad(corr, (a, b), h.gather(2, idx))
        return corr, idx, txyz, g1, g2

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        step()
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        outs = step()
    for replay in range(2):
        for o in outs:
            o.detach().zero_()
        graph.replay()
        torch.cuda.synchronize()
        corr, idx, txyz, g1, g2 = (o.detach().clone() for o in outs)
        corr, idx, txyz = _by_index(corr, idx, txyz)
        assert torch.equal(idx, e_idx)
        assert torch.equal(corr, e_corr) and torch.equal(txyz, e_txyz)
        assert torch.equal(g2, e_g2)
        print(f"replay {replay}: g1 bit-equal to eager: {torch.equal(g1, e_g1)}")
        _check_g1(g1, c_g1, ref, f"replay {replay} fmap1.grad")
