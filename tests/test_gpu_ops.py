"""GPU numerics tests: every HIP kernel against the pure-PyTorch fp32
reference (same inputs, fp32 tolerances).  Run with -m gpu on an MI355X."""

import os

import pytest
import torch

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    import pvraft_amd.ops as ops
    from pvraft_amd.ops import reference as R


@pytest.fixture(scope="module", autouse=True)
def _require_gpu_and_ext():
    if not torch.cuda.is_available():
        pytest.skip("needs GPU")
    import pvraft_amd.ops as ops

    assert ops.hip_available(), "HIP extension must be built on the GPU box"


def dev():
    return torch.device("cuda:0")


@pytest.mark.parametrize("B,N,k", [(2, 500, 16), (1, 8192, 32), (3, 127, 8)])
def test_knn_graph_matches_reference(B, N, k):
    xyz = torch.randn(B, N, 3, device=dev())
    got = ops.knn_graph(xyz, k)
    want = R.knn_idx(xyz, k)
    # neighbour SETS must match except where distance ties cross the k-boundary;
    # compare via distances, which are tie-insensitive
    sq = lambda idx: (
        (xyz.unsqueeze(2) - xyz.gather(1, idx.reshape(B, -1, 1).expand(B, N * k, 3).long()).view(B, N, k, 3)) ** 2
    ).sum(-1).sort(-1).values
    assert torch.allclose(sq(got), sq(want), atol=1e-4), (sq(got) - sq(want)).abs().max()


def test_gather_edge_concat_fwd_bwd():
    B, N, C, K = 2, 311, 35, 16
    xyz = torch.randn(B, N, 3, device=dev())
    idx = torch.randint(0, N, (B, N, K), device=dev())
    feats = torch.randn(B, N, C, device=dev(), requires_grad=True)
    feats_ref = feats.detach().clone().requires_grad_(True)

    out = ops.gather_edge_concat(feats, idx, xyz)
    out_ref = R.gather_edge_concat(feats_ref, idx, xyz)
    assert torch.allclose(out, out_ref, atol=1e-5)

    g = torch.randn_like(out)
    out.backward(g)
    out_ref.backward(g)
    assert torch.allclose(feats.grad, feats_ref.grad, atol=1e-3, rtol=1e-4)


@pytest.mark.parametrize("B,N,K,L", [(2, 257, 64, 3), (1, 1024, 512, 3), (1, 64, 33, 2)])
def test_voxel_corr_fwd_bwd(B, N, K, L):
    corr = torch.randn(B, N, K, device=dev(), requires_grad=True)
    coords = torch.randn(B, N, 3, device=dev())
    xyz = coords.unsqueeze(2) + torch.randn(B, N, K, 3, device=dev()) * 0.5
    corr_ref = corr.detach().clone().requires_grad_(True)

    out = ops.voxel_corr(corr, xyz, coords, 0.25, L)
    out_ref = R.voxel_corr(corr_ref, xyz, coords, 0.25, L)
    assert torch.allclose(out, out_ref, atol=1e-4), (out - out_ref).abs().max()

    g = torch.randn_like(out)
    out.backward(g)
    out_ref.backward(g)
    assert torch.allclose(corr.grad, corr_ref.grad, atol=1e-4), (corr.grad - corr_ref.grad).abs().max()


@pytest.mark.parametrize("B,N,K,k", [(2, 257, 64, 16), (1, 1024, 512, 32), (1, 50, 40, 32)])
def test_knn_corr_fwd_bwd(B, N, K, k):
    corr = torch.randn(B, N, K, device=dev(), requires_grad=True)
    coords = torch.randn(B, N, 3, device=dev())
    xyz = coords.unsqueeze(2) + torch.randn(B, N, K, 3, device=dev())
    corr_ref = corr.detach().clone().requires_grad_(True)

    out = ops.knn_corr(corr, xyz, coords, k)
    out_ref = R.knn_corr(corr_ref, xyz, coords, k)
    assert out.shape == (B, 4, k, N)
    # selections may differ on exact distance ties; compare sorted over k
    assert torch.allclose(
        out.sort(dim=2).values, out_ref.sort(dim=2).values, atol=1e-4
    ), (out.sort(dim=2).values - out_ref.sort(dim=2).values).abs().max()

    # backward: channel-0 grads scatter into corr at the selected slots
    out[:, 0].sum().backward()
    out_ref[:, 0].sum().backward()
    assert torch.allclose(corr.grad.sum(), corr_ref.grad.sum())
    assert corr.grad.max() == 1 and corr.grad.min() == 0


def test_knn_graph_excludes_nothing_and_includes_self():
    xyz = torch.randn(1, 300, 3, device=dev())
    idx = ops.knn_graph(xyz, 8)
    self_included = (idx == torch.arange(300, device=dev()).view(1, 300, 1)).any(-1)
    assert self_included.all()


def test_corr_truncate_gpu_matches_cpu():
    B, C, N, M, K = 2, 128, 513, 600, 128
    f1 = torch.randn(B, C, N, device=dev())
    f2 = torch.randn(B, C, M, device=dev())
    xyz2 = torch.randn(B, M, 3, device=dev())
    corr, idx, txyz = ops.corr_truncate(f1, f2, xyz2, K)
    corr_c, idx_c, txyz_c = R.corr_truncate(f1.cpu(), f2.cpu(), xyz2.cpu(), K)
    # top-K SET matches across devices (the GPU histogram-select kernel
    # returns the set unsorted -- every consumer is order-invariant -- and
    # GEMM rounding may swap near-equal entries), so compare sorted values
    assert torch.allclose(
        corr.sort(-1, descending=True).values.cpu(),
        corr_c.sort(-1, descending=True).values,
        atol=1e-3,
    ), (corr.sort(-1, descending=True).values.cpu() - corr_c.sort(-1, descending=True).values).abs().max()
    # internal consistency: txyz must be xyz2 gathered at the GPU's own idx
    want = xyz2.gather(1, idx.reshape(B, N * K).unsqueeze(-1).expand(B, N * K, 3).long()).view(B, N, K, 3)
    assert torch.equal(txyz, want)
    # and corr values must equal the dot products at those indices
    f2g = f2.transpose(1, 2).gather(1, idx.reshape(B, N * K).unsqueeze(-1).expand(B, N * K, C).long()).view(B, N, K, C)
    recomputed = torch.einsum("bcn,bnkc->bnk", f1, f2g) / (C ** 0.5)
    assert torch.allclose(corr, recomputed, atol=1e-3), (corr - recomputed).abs().max()


@pytest.mark.parametrize(
    "B,C,S,G,act,dtype",
    [
        (2, 96, 32 * 777, 8, "lrelu", torch.float32),
        (2, 128, 8192, 8, "none", torch.float32),
        (1, 64, 515, 8, "lrelu", torch.bfloat16),
        (4, 16, 100, 8, "none", torch.bfloat16),
    ],
)
def test_group_norm_act_fwd_bwd(B, C, S, G, act, dtype):
    import torch.nn.functional as F

    x = torch.randn(B, C, S, device=dev(), dtype=dtype, requires_grad=True)
    w = torch.randn(C, device=dev(), requires_grad=True)
    b = torch.randn(C, device=dev(), requires_grad=True)
    xr = x.detach().clone().requires_grad_(True)
    wr = w.detach().clone().requires_grad_(True)
    br = b.detach().clone().requires_grad_(True)

    y = ops.group_norm_act(x, G, w, b, 1e-5, act=act, slope=0.1)
    y_ref = F.group_norm(xr.float(), G, wr, br, 1e-5)
    if act == "lrelu":
        y_ref = F.leaky_relu(y_ref, 0.1)
    atol = 1e-4 if dtype == torch.float32 else 5e-2
    assert torch.allclose(y.float(), y_ref.to(y.dtype).float(), atol=atol), (
        (y.float() - y_ref.to(y.dtype).float()).abs().max()
    )

    g = torch.randn_like(y_ref)
    y.backward(g.to(dtype))
    y_ref.backward(g)
    gatol = 1e-3 if dtype == torch.float32 else 1e-1
    assert torch.allclose(x.grad.float(), xr.grad.float(), atol=gatol), (
        (x.grad.float() - xr.grad.float()).abs().max()
    )
    # weight/bias grads reduce over big spatial: compare with loose rel tol
    assert torch.allclose(w.grad, wr.grad, rtol=2e-2, atol=2e-1), (w.grad - wr.grad).abs().max()
    assert torch.allclose(b.grad, br.grad, rtol=2e-2, atol=2e-1), (b.grad - br.grad).abs().max()


def test_gather_edge_csr_backward_matches_atomic():
    from pvraft_amd.model.graph import Graph

    B, N, C, K = 2, 700, 35, 16
    xyz = torch.randn(B, N, 3, device=dev())
    g = Graph.build(xyz, K)
    feats = torch.randn(B, N, C, device=dev(), requires_grad=True)
    feats2 = feats.detach().clone().requires_grad_(True)
    feats3 = feats.detach().clone().requires_grad_(True)

    out_csr = ops.gather_edge_concat(feats, g.idx, g.xyz, csr=g.csr())
    out_atomic = ops.gather_edge_concat(feats2, g.idx, g.xyz, csr=None)
    out_ref = R.gather_edge_concat(feats3, g.idx, g.xyz)
    assert torch.allclose(out_csr, out_atomic)

    go = torch.randn_like(out_csr)
    out_csr.backward(go)
    out_atomic.backward(go)
    out_ref.backward(go)
    assert torch.allclose(feats.grad, feats3.grad, atol=1e-3), (feats.grad - feats3.grad).abs().max()
    assert torch.allclose(feats2.grad, feats3.grad, atol=1e-3)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_group_norm_act_maxpool_fwd_bwd(dtype):
    import torch.nn.functional as F

    B, C, K, N, G = 2, 96, 32, 555, 8
    x = torch.randn(B, C, K, N, device=dev(), dtype=dtype, requires_grad=True)
    w = torch.randn(C, device=dev(), requires_grad=True)
    b = torch.randn(C, device=dev(), requires_grad=True)
    xr = x.detach().clone().requires_grad_(True)
    wr = w.detach().clone().requires_grad_(True)
    br = b.detach().clone().requires_grad_(True)

    y = ops.group_norm_act_maxpool(x, G, w, b, 1e-5, act="lrelu", slope=0.1)
    y_ref = F.leaky_relu(F.group_norm(xr.float(), G, wr, br, 1e-5), 0.1).max(dim=2)[0]
    atol = 1e-4 if dtype == torch.float32 else 5e-2
    assert y.shape == (B, C, N)
    assert torch.allclose(y.float(), y_ref.to(y.dtype).float(), atol=atol), (
        (y.float() - y_ref.to(y.dtype).float()).abs().max()
    )

    g = torch.randn_like(y_ref)
    y.backward(g.to(dtype))
    y_ref.backward(g)
    gatol = 1e-3 if dtype == torch.float32 else 1e-1
    assert torch.allclose(x.grad.float(), xr.grad.float(), atol=gatol), (
        (x.grad.float() - xr.grad.float()).abs().max()
    )
    # bf16-saved xhat quantisation random-walks over the 17k-sample channel
    # reduction (the fp32 reference does not quantise): loose abs tolerance
    wtol = 2e-1 if dtype == torch.float32 else 1.5
    assert torch.allclose(w.grad, wr.grad, rtol=5e-2, atol=wtol), (w.grad - wr.grad).abs().max()
    assert torch.allclose(b.grad, br.grad, rtol=5e-2, atol=wtol), (b.grad - br.grad).abs().max()


@pytest.mark.parametrize("B,Co,Ci,S", [(2, 64, 192, 16384), (2, 61, 128, 8192), (1, 128, 131, 524288 // 4), (3, 16, 9, 1000)])
def test_pw_wgrad_mfma_matches_einsum(B, Co, Ci, S):
    from pvraft_amd import _C

    dy = torch.randn(B, Co, S, device=dev(), dtype=torch.bfloat16)
    x = torch.randn(B, Ci, S, device=dev(), dtype=torch.bfloat16)
    got, dbias = _C.pw_wgrad(dy, x, 0, True)
    want = torch.einsum("bos,bis->oi", dy.float(), x.float())
    # bf16 inputs, fp32 accumulation both sides; atomic split-K ordering
    err = (got - want).abs().max().item()
    denom = want.abs().max().item()
    assert err < 0.02 * max(denom, 1.0), (err, denom)
    want_b = dy.float().sum(dim=(0, 2))
    errb = (dbias - want_b).abs().max().item()
    assert errb < 0.02 * max(want_b.abs().max().item(), 1.0), errb


def test_knn_graph_degenerate_ties():
    """All-identical points: every distance ties; the kernel must still emit
    k valid indices per query (collect-buffer overflow with a collapsed
    threshold bracket: the tie-overflow path)."""
    xyz = torch.zeros(1, 300, 3, device=dev())
    idx = ops.knn_graph(xyz, 16)
    assert idx.shape == (1, 300, 16)
    assert (idx >= 0).all() and (idx < 300).all()

    # lattice: many exact ties at each shell
    g = torch.stack(torch.meshgrid(
        torch.arange(8.0), torch.arange(8.0), torch.arange(8.0), indexing="ij"
    ), -1).reshape(1, -1, 3).to(dev())
    idx = ops.knn_graph(g, 8)
    want = R.knn_idx(g, 8)
    B, N, k = idx.shape
    sq = lambda i: (
        (g.unsqueeze(2) - g.gather(1, i.reshape(B, -1, 1).expand(B, N * k, 3).long()).view(B, N, k, 3)) ** 2
    ).sum(-1).sort(-1).values
    assert torch.allclose(sq(idx), sq(want), atol=1e-4)


@pytest.mark.parametrize("B,N,K,L,k", [(2, 513, 512, 3, 32), (1, 200, 64, 2, 16)])
def test_pv_corr_fused_matches_separate(B, N, K, L, k):
    corr = torch.randn(B, N, K, device=dev(), requires_grad=True)
    coords = torch.randn(B, N, 3, device=dev())
    xyz = coords.unsqueeze(2) + torch.randn(B, N, K, 3, device=dev()) * 0.5
    corr2 = corr.detach().clone().requires_grad_(True)

    vox, knn = ops.pv_corr_lookup(corr, xyz, coords, 0.25, L, k)
    vox_ref = ops.voxel_corr(corr2, xyz, coords, 0.25, L)
    knn_ref = ops.knn_corr(corr2, xyz, coords, k)
    assert torch.allclose(vox, vox_ref, atol=1e-4), (vox - vox_ref).abs().max()
    assert torch.allclose(knn.sort(dim=2).values, knn_ref.sort(dim=2).values, atol=1e-4)

    gv = torch.randn_like(vox)
    gk = torch.randn_like(knn)
    (vox * gv).sum().backward(retain_graph=True)
    (vox_ref * gv).sum().backward(retain_graph=True)
    assert torch.allclose(corr.grad, corr2.grad, atol=1e-4), (corr.grad - corr2.grad).abs().max()
    corr.grad = None
    corr2.grad = None
    # knn channel 0 gradient (selection sets may differ on exact ties; use
    # a tie-free grad check: sum of channel 0 -> ones at selected slots)
    knn[:, 0].sum().backward()
    knn_ref[:, 0].sum().backward()
    assert torch.allclose(corr.grad.sum(), corr2.grad.sum())


@pytest.mark.parametrize("R,M,K", [(64, 8192, 512), (33, 1000, 100), (16, 512, 512), (8, 777, 32)])
def test_topk_rows_matches_torch(R, M, K):
    from pvraft_amd import _C

    vals = torch.randn(R, M, device=dev())
    got_v, got_i = _C.topk_rows(vals, K)
    want_v, want_i = vals.topk(K, dim=1)
    # set comparison (kernel output unsorted; ties may swap at the boundary)
    assert torch.allclose(got_v.sort(dim=1).values, want_v.sort(dim=1).values, atol=1e-5), (
        (got_v.sort(dim=1).values - want_v.sort(dim=1).values).abs().max()
    )
    # values must match the gathered indices exactly
    assert torch.equal(got_v, vals.gather(1, got_i.long()))


def test_topk_rows_degenerate_ties():
    from pvraft_amd import _C

    vals = torch.zeros(4, 2048, device=dev())
    got_v, got_i = _C.topk_rows(vals, 256)
    assert (got_v == 0).all()
    assert (got_i >= 0).all() and (got_i < 2048).all()


@pytest.mark.parametrize("dtype,N", [(torch.float32, 1024), (torch.float32, 515),
                                     (torch.bfloat16, 8192), (torch.bfloat16, 515)])
def test_gru_gates_fused_match_eager(dtype, N):
    """Fused GRU gate kernels vs the plain-torch formulation, fwd + grads."""
    B, H = 2, 64
    torch.manual_seed(0)
    pre_zr = torch.randn(B, 2 * H, N, device=dev(), dtype=dtype, requires_grad=True)
    pre_q = torch.randn(B, H, N, device=dev(), dtype=dtype, requires_grad=True)
    h = torch.randn(B, H, N, device=dev(), dtype=dtype, requires_grad=True)
    ref = [t.detach().clone().requires_grad_(True) for t in (pre_zr, pre_q, h)]

    z, rh = ops.gru_zr(pre_zr, h)
    out = ops.gru_q(pre_q, z, h)
    # weight rh into the loss so _GruZR's rh gradient path is exercised
    (out.float().square().sum() + rh.float().sum()).backward()

    zr_r = torch.sigmoid(ref[0])
    z_r, r_r = zr_r[:, :H], zr_r[:, H:]
    rh_r = r_r * ref[2]
    out_r = (1 - z_r) * ref[2] + z_r * torch.tanh(ref[1])
    (out_r.float().square().sum() + rh_r.float().sum()).backward()

    tol = 1e-5 if dtype == torch.float32 else 2e-2
    assert torch.allclose(out.float(), out_r.float(), atol=tol), (out.float() - out_r.float()).abs().max()
    assert torch.allclose(rh.float(), rh_r.float(), atol=tol)
    for got, want in zip((pre_zr, pre_q, h), ref):
        assert torch.allclose(got.grad.float(), want.grad.float(), atol=tol * 40), (
            (got.grad.float() - want.grad.float()).abs().max()
        )


def test_fused_sequence_loss_matches_eager():
    """Fused seq_loss kernel vs the eager masked-L1 formulation, fwd+grads."""
    from pvraft_amd.utils import loss as L

    torch.manual_seed(3)
    B, N, T = 2, 4097, 8
    gt = torch.randn(B, N, 3, device=dev())
    mask = (torch.rand(B, N, 1, device=dev()) > 0.3).float()
    batch = {"ground_truth": [mask, gt]}
    flows = [torch.randn(B, N, 3, device=dev(), requires_grad=True) for _ in range(T)]
    flows_r = [f.detach().clone().requires_grad_(True) for f in flows]

    fused = L.sequence_loss(flows, batch, gamma=0.8)
    eager = 0.0
    for i in range(T):
        eager = eager + (0.8 ** (T - i - 1)) * L._eager_loss(flows_r[i], batch)
    assert torch.allclose(fused, eager, atol=1e-5), (fused - eager).abs().max()
    fused.backward()
    eager.backward()
    for f, fr in zip(flows, flows_r):
        assert torch.allclose(f.grad, fr.grad, atol=1e-6), (f.grad - fr.grad).abs().max()

    # compute_loss (single flow) path
    one = torch.randn(B, N, 3, device=dev(), requires_grad=True)
    one_r = one.detach().clone().requires_grad_(True)
    lf = L.compute_loss(one, batch)
    le = L._eager_loss(one_r, batch)
    assert torch.allclose(lf, le, atol=1e-6)
    lf.backward()
    le.backward()
    assert torch.allclose(one.grad, one_r.grad, atol=1e-6)


def _edge_gnmp_reference(wg_t, idx, G, w, b, eps, slope=0.1):
    """Reference composition of the fused edge_gnmp op: explicit gather-diff
    edge tensor -> F.group_norm -> leaky_relu -> max over K (the reference
    SetConv stage-1 pipeline, gconv.py:64-75, on pre-multiplied Wg)."""
    B, N, M = wg_t.shape
    K = idx.shape[2]
    gathered = wg_t.gather(1, idx.reshape(B, N * K, 1).expand(B, N * K, M).long())
    edge = (gathered.view(B, N, K, M) - wg_t.unsqueeze(2)).permute(0, 3, 2, 1)  # (B,M,K,N)
    y = torch.nn.functional.group_norm(edge.contiguous(), G, w, b, eps)
    y = torch.nn.functional.leaky_relu(y, slope)
    y = y.max(dim=2)[0]  # (B, M, N)
    return y.transpose(1, 2)  # (B, N, M)


@pytest.mark.parametrize("B,N,K,M,G,dtype", [
    (2, 311, 16, 48, 8, torch.float32),
    (1, 1024, 32, 96, 8, torch.float32),
    (2, 500, 32, 16, 8, torch.float32),
    (1, 1024, 32, 64, 8, torch.bfloat16),
])
def test_edge_gnmp_matches_reference(B, N, K, M, G, dtype):
    from pvraft_amd.model.graph import Graph

    torch.manual_seed(0)
    wg = torch.randn(B, N, M, device=dev()).to(dtype).requires_grad_(True)
    wg_ref = wg.detach().float().clone().requires_grad_(True)
    idx = torch.randint(0, N, (B, N, K), device=dev(), dtype=torch.int64)
    graph = Graph(idx=idx, xyz=torch.randn(B, N, 3, device=dev()))
    w = torch.randn(M, device=dev(), requires_grad=True)
    b = torch.randn(M, device=dev(), requires_grad=True)
    w_ref = w.detach().clone().requires_grad_(True)
    b_ref = b.detach().clone().requires_grad_(True)

    y = ops.edge_gnmp(wg, graph.idx32, graph.csr(), G, w, b, 1e-5, act="lrelu", slope=0.1)
    y_ref = _edge_gnmp_reference(wg_ref, idx, G, w_ref, b_ref, 1e-5)

    tol = 5e-2 if dtype == torch.bfloat16 else 1e-4
    assert torch.allclose(y.float(), y_ref, atol=tol, rtol=tol), (y.float() - y_ref).abs().max()

    g = torch.randn_like(y_ref)
    y.backward(g.to(dtype))
    y_ref.backward(g)
    btol = 1e-1 if dtype == torch.bfloat16 else 1e-3
    assert torch.allclose(wg.grad.float(), wg_ref.grad, atol=btol, rtol=1e-2), (
        (wg.grad.float() - wg_ref.grad).abs().max()
    )
    # dgamma/dbeta are sums of ~N*K bf16-rounded terms: per-element noise
    # ~2^-8 accumulates to ~0.3% of the (large) sums, so scale the bf16
    # tolerance with the magnitude
    wtol = 5e-3 * w_ref.grad.abs().max().item() + btol
    assert torch.allclose(w.grad, w_ref.grad, atol=wtol, rtol=1e-2), (
        (w.grad - w_ref.grad).abs().max()
    )
    assert torch.allclose(b.grad, b_ref.grad, atol=wtol, rtol=1e-2), (
        (b.grad - b_ref.grad).abs().max()
    )


def test_setconv_fused_path_matches_reference_composition():
    """Whole SetConv module: fused GPU path vs the PVRAFT_REF_OPS
    composition on identical weights/inputs (fp32)."""
    from pvraft_amd.model.graph import Graph
    from pvraft_amd.model.setconv import SetConv

    torch.manual_seed(1)
    B, N, C = 2, 400, 32
    sc = SetConv(C, 64).to(dev())
    feats = torch.randn(B, C, N, device=dev()).transpose(1, 2).requires_grad_(True)
    xyz = torch.randn(B, N, 3, device=dev())
    graph = Graph(idx=torch.randint(0, N, (B, N, 32), device=dev()), xyz=xyz)

    out = sc(feats, graph)
    loss = (out ** 2).mean()
    loss.backward()
    grads = {n: p.grad.clone() for n, p in sc.named_parameters()}
    fgrad = feats.grad.clone()

    os.environ["PVRAFT_REF_OPS"] = "1"
    try:
        sc.zero_grad()
        feats2 = feats.detach().clone().requires_grad_(True)
        out_ref = sc(feats2, graph)
        (out_ref ** 2).mean().backward()
    finally:
        os.environ.pop("PVRAFT_REF_OPS", None)

    assert torch.allclose(out, out_ref, atol=1e-4, rtol=1e-4), (out - out_ref).abs().max()
    assert torch.allclose(fgrad, feats2.grad, atol=1e-4, rtol=1e-3), (fgrad - feats2.grad).abs().max()
    for n, p in sc.named_parameters():
        assert torch.allclose(grads[n], p.grad, atol=1e-3, rtol=1e-2), n


@pytest.mark.parametrize("B,N,M,C,K", [
    (2, 8192, 8192, 128, 512),   # flagship shape
    (1, 1000, 777, 64, 512),     # K > M/2, ragged sizes
    (2, 300, 4000, 32, 64),
    (1, 128, 100, 128, 100),     # K == M (everything selected)
])
def test_corr_topk_fused_matches_reference(B, N, M, C, K):
    """Fused MFMA corr GEMM + streaming top-K vs fp32 torch on the same
    bf16-rounded inputs (fp32 accumulate both sides; selection compared by
    value, tie-insensitive)."""
    torch.manual_seed(3)
    f1 = torch.randn(B, C, N, device=dev(), dtype=torch.bfloat16)
    f2 = torch.randn(B, C, M, device=dev(), dtype=torch.bfloat16)
    import pvraft_amd._C as _C

    f1t = _C.batched_transpose(f1.contiguous())
    f2t = _C.batched_transpose(f2.contiguous())
    v, i = _C.corr_topk(f1t, f2t, K)

    ref = torch.bmm(f1.float().transpose(1, 2), f2.float()) / (C ** 0.5)
    ref_v, _ = torch.topk(ref, K, dim=2)

    vs = v.sort(dim=2, descending=True).values
    assert torch.allclose(vs, ref_v, atol=2e-3, rtol=1e-3), (vs - ref_v).abs().max()

    # indices must be unique per row and consistent with their values
    ii = i.long()
    for b in range(B):
        rows = torch.randint(0, N, (8,))
        for n in rows:
            idx_row = ii[b, n]
            assert idx_row.unique().numel() == K
            gathered = ref[b, n].gather(0, idx_row)
            assert torch.allclose(gathered, v[b, n], atol=2e-3, rtol=1e-3)


def test_corr_topk_degenerate_ties():
    """All-equal feature rows -> all correlations tie; any K indices are a
    valid top-K set and values must all equal the tied value."""
    import pvraft_amd._C as _C

    B, N, M, C, K = 1, 64, 2048, 32, 512
    f1 = torch.ones(B, N, C, device=dev(), dtype=torch.bfloat16)
    f2 = torch.ones(B, M, C, device=dev(), dtype=torch.bfloat16)
    v, i = _C.corr_topk(f1, f2, K)
    expect = C / (C ** 0.5)
    assert torch.allclose(v, torch.full_like(v, expect), atol=1e-2)
    assert (i >= 0).all() and (i < M).all()


def test_corr_truncate_bf16_path_backward():
    """Autograd through the fused path: gradients flow to both fmaps."""
    B, N, M, C, K = 1, 256, 300, 64, 64
    f1 = torch.randn(B, C, N, device=dev(), dtype=torch.bfloat16, requires_grad=True)
    f2 = torch.randn(B, C, M, device=dev(), dtype=torch.bfloat16, requires_grad=True)
    xyz2 = torch.randn(B, M, 3, device=dev())
    corr, idx, txyz = ops.corr_truncate(f1, f2, xyz2, K)
    assert corr.shape == (B, N, K) and corr.dtype == torch.float32
    corr.sum().backward()
    assert f1.grad is not None and f1.grad.abs().sum() > 0
    assert f2.grad is not None and f2.grad.abs().sum() > 0


@pytest.mark.parametrize("parts,Co,S,act,with_bias,with_addend", [
    (1, 64, 2048, 0, True, False),
    (2, 61, 1000, 1, True, False),
    (3, 192, 4096, 0, False, True),
    (1, 128, 555, 1, False, False),
])
def test_pw_fwd_fused_matches_composed(parts, Co, S, act, with_bias, with_addend):
    """One-launch MFMA conv stack vs composed fp32 GEMMs (bf16-rounded
    inputs, fp32 accumulate both sides)."""
    import pvraft_amd._C as _C

    torch.manual_seed(7)
    B = 2
    cis = [64, 61, 37][:parts]
    ws = [torch.randn(Co, ci, device=dev(), dtype=torch.bfloat16) for ci in cis]
    xs = [torch.randn(B, ci, S, device=dev(), dtype=torch.bfloat16) for ci in cis]
    bias = torch.randn(Co, device=dev()) if with_bias else None
    add_full = torch.randn(B, Co + 32, S, device=dev(), dtype=torch.bfloat16)
    addend = add_full[:, 16:16 + Co] if with_addend else None

    y = _C.pw_fwd(ws, xs, bias, addend, act)

    ref = sum(torch.bmm(w.float().unsqueeze(0).expand(B, -1, -1), x.float())
              for w, x in zip(ws, xs))
    if bias is not None:
        ref = ref + bias.view(1, -1, 1)
    if addend is not None:
        ref = ref + addend.float()
    if act == 1:
        ref = torch.relu(ref)
    assert y.shape == (B, Co, S) and y.dtype == torch.bfloat16
    assert torch.allclose(y.float(), ref, atol=3e-2, rtol=2e-2), (
        (y.float() - ref).abs().max()
    )


def test_pw_fused_autograd_matches_fallback():
    """pw_fused under autocast (fused kernel) vs PVRAFT_NO_PWFWD=1
    (composed bmm path): same forward and same gradients within bf16
    tolerance."""
    from pvraft_amd.model.pointwise import pw_fused

    torch.manual_seed(11)
    B, Co, S = 2, 64, 3000
    w1 = torch.randn(Co, 64, device=dev(), requires_grad=True)
    w2 = torch.randn(Co, 61, device=dev(), requires_grad=True)
    x1 = torch.randn(B, 64, S, device=dev(), requires_grad=True)
    x2 = torch.randn(B, 61, S, device=dev(), requires_grad=True)
    bias = torch.randn(Co, device=dev(), requires_grad=True)
    leaves = [w1, w2, x1, x2, bias]
    clones = [t.detach().clone().requires_grad_(True) for t in leaves]

    with torch.autocast("cuda", dtype=torch.bfloat16):
        y = pw_fused([(w1, x1, None), (w2, x2, None)], bias=bias, act="relu")
    y.float().square().mean().backward()

    os.environ["PVRAFT_NO_PWFWD"] = "1"
    try:
        c1, c2, cx1, cx2, cb = clones
        with torch.autocast("cuda", dtype=torch.bfloat16):
            y2 = pw_fused([(c1, cx1, None), (c2, cx2, None)], bias=cb, act="relu")
        y2.float().square().mean().backward()
    finally:
        os.environ.pop("PVRAFT_NO_PWFWD", None)

    # the fallback rounds to bf16 after EACH part GEMM and again after the
    # bias add; the fused kernel keeps fp32 until the final store -- element
    # diffs up to a few bf16 ulps of the ACCUMULATED magnitude are expected
    # (the strict numerics test against fp32 is test_pw_fwd_fused_matches_
    # composed above)
    scale = y2.float().abs().max().item()
    assert torch.allclose(y.float(), y2.float(), atol=3e-2 * scale, rtol=5e-2), (
        (y.float() - y2.float()).abs().max(), scale
    )
    for a, b in zip(leaves, clones):
        gs = b.grad.abs().max().item() + 1e-6
        assert torch.allclose(a.grad, b.grad, atol=3e-2 * gs, rtol=5e-2), (
            (a.grad - b.grad).abs().max()
        )


@pytest.mark.parametrize("B,R,C,dtype", [
    (2, 8192, 96, torch.bfloat16),   # narrow-C fast path
    (2, 8191, 48, torch.bfloat16),   # narrow-C, ragged R
    (1, 513, 16, torch.float32),
    (2, 500, 35, torch.float32),     # narrow-scalar (C % W != 0)
    (2, 300, 128, torch.bfloat16),   # general tiled path
    (2, 48, 8192, torch.bfloat16),   # narrow-R fast path (wg direction)
    (2, 96, 8191, torch.bfloat16),   # narrow-R, ragged C
    (1, 16, 513, torch.float32),     # narrow-R fp32 (W=4)
    (2, 61, 8192, torch.bfloat16),   # R % W != 0: general kernel
])
def test_batched_transpose_shapes(B, R, C, dtype):
    import pvraft_amd._C as _C

    x = torch.randn(B, R, C, device=dev()).to(dtype)
    y = _C.batched_transpose(x.contiguous())
    assert torch.equal(y, x.transpose(1, 2).contiguous())

@pytest.mark.parametrize("B,N,K,C,G,autocast_on", [
    (2, 311, 32, 64, 8, False),
    (1, 1024, 16, 64, 8, True),
    (2, 500, 32, 32, 8, False),
])
def test_knn_gnmp_matches_reference(B, N, K, C, G, autocast_on):
    """Fused conv(4->C)+GN+PReLU+maxpool vs the explicit composition
    (reference model/corr.py:70-76 semantics)."""
    import torch.nn.functional as F

    torch.manual_seed(3)
    raw = torch.randn(B, 4, K, N, device=dev()).requires_grad_(True)
    w = torch.randn(C, 4, 1, 1, device=dev()).mul(0.2).requires_grad_(True)
    cb = torch.randn(C, device=dev()).mul(0.1).requires_grad_(True)
    ga = torch.rand(C, device=dev()).add(0.5).requires_grad_(True)
    be = torch.randn(C, device=dev()).mul(0.1).requires_grad_(True)
    sl = torch.tensor([0.25], device=dev()).requires_grad_(True)

    leaves = [raw, w, cb, ga, be, sl]
    clones = [t.detach().clone().requires_grad_(True) for t in leaves]
    raw2, w2, cb2, ga2, be2, sl2 = clones

    with torch.autocast("cuda", dtype=torch.bfloat16, enabled=autocast_on):
        y = ops.knn_gnmp(raw, w, cb, G, ga, be, 1e-5, sl)
    y.float().square().mean().backward()

    x = F.conv2d(raw2, w2, cb2)
    x = F.group_norm(x, G, ga2, be2, 1e-5)
    x = F.prelu(x, sl2)
    y_ref = x.max(dim=2).values  # (B, C, N)
    y_ref.square().mean().backward()

    tol = 3e-2 if autocast_on else 2e-3
    assert torch.allclose(y.float(), y_ref, atol=tol, rtol=1e-2), (
        (y.float() - y_ref).abs().max()
    )
    for a, b in zip(leaves, clones):
        scale = b.grad.abs().max().item() + 1e-6
        assert torch.allclose(a.grad.float(), b.grad, atol=0.03 * scale, rtol=5e-2), (
            (a.grad.float() - b.grad).abs().max(), scale
        )

def test_morton_order_valid_permutation():
    torch.manual_seed(5)
    xyz = torch.randn(3, 2048, 3, device=dev())
    perm, inv = ops.morton_order(xyz)
    B, N = perm.shape
    ar = torch.arange(N, device=dev())
    # perm and inv are permutations and mutual inverses
    assert torch.equal(perm.sort(1).values, ar.expand(B, N))
    assert torch.equal(inv.sort(1).values, ar.expand(B, N))
    assert torch.equal(perm.gather(1, inv), ar.expand(B, N))
    # gathering by perm sorts the Morton keys
    mn, mx = torch.aminmax(xyz, dim=1)
    inv_ext = (1023.0 / (mx - mn).clamp_min(1e-9)).contiguous()
    import pvraft_amd._C as _C
    keys = _C.morton_keys(xyz.contiguous(), mn.contiguous(), inv_ext)
    ks = keys.gather(1, perm)
    assert torch.all(ks[:, 1:] >= ks[:, :-1])


def test_multi_cast_bf16_matches_to():
    import pvraft_amd._C as _C

    torch.manual_seed(6)
    srcs = [torch.randn((i % 7) + 1, (i % 13) + 1, device=dev())
            for i in range(150)]
    dsts = [torch.empty_like(t, dtype=torch.bfloat16) for t in srcs]
    _C.multi_cast_bf16(srcs, dsts)
    torch.cuda.synchronize()
    for s_, d in zip(srcs, dsts):
        assert torch.equal(d, s_.to(torch.bfloat16))


def test_model_output_invariant_to_morton_relabel():
    """Morton relabeling permutes internals but must return flows in the
    caller's point order: compare a 16-iter forward (relabeling active)
    against PVRAFT_NO_MORTON on the same weights/inputs.  Not bitwise:
    kNN ties and fp32-atomic GN stats differ between labelings."""
    from pvraft_amd.model import PVRaft

    torch.manual_seed(11)
    model = PVRaft(truncate_k=256).to(dev())
    x1 = torch.randn(2, 2048, 3, device=dev())
    x2 = x1 + 0.05 * torch.randn_like(x1)
    with torch.no_grad(), torch.autocast("cuda", dtype=torch.bfloat16):
        f_m = model([x1, x2], num_iters=16)[-1].float()
    os.environ["PVRAFT_NO_MORTON"] = "1"
    try:
        with torch.no_grad(), torch.autocast("cuda", dtype=torch.bfloat16):
            f_p = model([x1, x2], num_iters=16)[-1].float()
    finally:
        os.environ.pop("PVRAFT_NO_MORTON", None)
    cos = torch.nn.functional.cosine_similarity(
        f_m.flatten(), f_p.flatten(), dim=0).item()
    assert cos > 0.98, cos
    scale = f_p.abs().max().item() + 1e-6
    assert (f_m - f_p).abs().median().item() < 0.05 * scale
