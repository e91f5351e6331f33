"""GPU tests of the fused kNN-interpolation kernel (csrc/knn_interp.hip)
against reference.knn_interpolate on the same device, and of
Predictor.predict_dense through the captured graph.  Run with -m gpu."""

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


def tile_pts():
    from pvraft_amd import _C

    return int(_C.KNN_INTERP_TILE)


def make_case(B, N, M, C):
    """randn*3 clouds; the first half of the queries are copies of support
    points."""
    g = torch.Generator().manual_seed(1000 * N + M)
    sup = torch.randn(B, N, 3, generator=g) * 3
    val = torch.randn(B, N, C, generator=g)
    qry = torch.randn(B, M, 3, generator=g) * 3
    half = M // 2
    src = torch.stack([torch.randint(0, N, (half,), generator=g) for _ in range(B)])
    qry[:, :half] = sup.gather(1, src.unsqueeze(-1).expand(B, half, 3))
    return sup.to(dev()), val.to(dev()), qry.to(dev())


def gather_rows(t, idx):
    """t (B, N, D), idx (B, M, k) -> (B, M, k, D)"""
    B, M, k = idx.shape
    D = t.shape[2]
    return t.gather(1, idx.reshape(B, M * k, 1).expand(B, M * k, D)).view(B, M, k, D)


def shapes():
    # the last case sweeps two full LDS tiles plus a remainder; M = 3001 is
    # no multiple of the 256-query block
    return [
        (2, 300, 1000, 3, 3),
        (1, 2, 7, 3, 3),
        (1, 1, 1, 1, 1),
        (2, 257, 513, 64, 16),
        (3, 127, 65, 3, 8),
        (1, "2*tile+77", 3001, 3, 3),
    ]


@pytest.mark.parametrize("B,N,M,C,k", shapes())
def test_knn_interpolate_matches_reference(B, N, M, C, k):
    if isinstance(N, str):
        N = 2 * tile_pts() + 77
    eps = 1e-8
    sup, val, qry = make_case(B, N, M, C)
    out, idx, w = ops.knn_interpolate(sup, val, qry, k=k, eps=eps)
    out_ref, idx_ref, _ = R.knn_interpolate(sup, val, qry, k=k, eps=eps)
    ke = min(k, N)
    assert out.shape == (B, M, C) and idx.shape == (B, M, ke) and w.shape == (B, M, ke)
    assert idx.dtype == torch.int64 and out.dtype == torch.float32

    # (b) in range, duplicate-free
    assert int(idx.min()) >= 0 and int(idx.max()) < N
    if ke > 1:
        assert (idx.sort(-1).values.diff(dim=-1) > 0).all()

    # (a) neighbour distances recomputed from the kernel's idx: ascending as
    # returned, and equal to the reference's (tie-insensitive comparison)
    d2 = lambda i: ((gather_rows(sup, i) - qry.unsqueeze(2)) ** 2).sum(-1)
    d_got, d_ref = d2(idx), d2(idx_ref)
    assert (d_got.diff(dim=-1) >= 0).all()
    err = (d_got.sort(-1).values - d_ref.sort(-1).values).abs().max().item()
    print(f"max neighbour-distance error = {err:.3e}")
    assert err <= 1e-4

    # (c) w and out follow the formula evaluated on the kernel's own idx
    w_want = 1.0 / (d_got + eps)
    w_want = w_want / w_want.sum(-1, keepdim=True)
    werr = (w - w_want).abs().max().item()
    out_want = (w_want.unsqueeze(-1) * gather_rows(val, idx)).sum(2)
    oerr = (out - out_want).abs().max().item()
    print(f"max |w - formula| = {werr:.3e}  max |out - formula| = {oerr:.3e}")
    assert werr <= 1e-4 and oerr <= 1e-4

    # (d) normalised weights
    assert (w.sum(-1) - 1).abs().max().item() <= 1e-5


@pytest.mark.parametrize("k", [3, 8, 16])
def test_constant_field_is_reproduced(k):
    sup, _, qry = make_case(2, 300, 1000, 3)
    val = torch.full((2, 300, 3), 2.5, device=dev())
    out, _, _ = ops.knn_interpolate(sup, val, qry, k=k)
    # fp32 worst case: k roundings in the weight sum, two in the
    # normalisation and k in the blend, (2k + 2) * 2^-24 * 2.5 = 5.1e-6 at
    # k = 16; the bound is that rounded up to 1e-5
    assert (out - 2.5).abs().max().item() <= 1e-5


def test_backward_to_values_matches_reference():
    B, N, M, C, k = 2, 300, 1000, 3, 3
    sup, val, qry = make_case(B, N, M, C)
    v_hip = val.clone().requires_grad_(True)
    v_ref = val.clone().requires_grad_(True)
    out, idx, _ = ops.knn_interpolate(sup, v_hip, qry, k=k)
    out_ref, idx_ref, _ = R.knn_interpolate(sup, v_ref, qry, k=k)
    g = torch.randn(B, M, C, generator=torch.Generator().manual_seed(2)).to(dev())
    out.backward(g)
    out_ref.backward(g)
    err = (v_hip.grad - v_ref.grad).abs().max().item()
    same = torch.equal(idx.sort(-1).values, idx_ref.sort(-1).values)
    print(f"max |dvalues - reference| = {err:.3e} (same neighbour sets: {same})")
    assert err <= 1e-4


def test_predict_dense_through_graph():
    from pvraft_amd.engine import Predictor
    from pvraft_amd.model import PVRaft

    torch.manual_seed(5)
    model = PVRaft(truncate_k=64).to(dev()).eval()
    pred = Predictor(model, points=512, batch=1, iters=2, use_graph=True)
    assert pred.use_graph

    graph = None
    for call, (n1, n2) in enumerate([(3000, 2500), (2777, 3100)]):
        g = torch.Generator().manual_seed(20 + call)
        pc1 = torch.randn(n1, 3, generator=g).to(dev())
        pc2 = (torch.randn(n2, 3, generator=g) * 0.05).to(dev()) + pc1[
            torch.randint(0, n1, (n2,), generator=g).to(dev())
        ]
        dense, idx1, flow_sub = pred.predict_dense(
            pc1, pc2, k=3, generator=torch.Generator().manual_seed(call), return_sparse=True
        )
        assert dense.shape == (n1, 3) and torch.isfinite(dense).all()
        err = (dense[idx1] - flow_sub).abs().max().item()
        print(f"call {call}: max |dense[idx1] - sparse| = {err:.3e}")
        assert err <= 1e-4
        # one capture serves both full-cloud sizes
        if call == 0:
            graph = pred._graph
            assert graph is not None
        else:
            assert pred._graph is graph
