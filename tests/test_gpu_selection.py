"""GPU tests of the three threshold-selection kernels on the inputs of
selection_cases.py: non-Gaussian families, coherent orders and stride-biased
orders that defeat the strided sample, so the retry, overflow and bracket
code runs.  Every query / row of every case is compared with the exact
float64 reference; nothing is sampled and no wrong row is tolerated.  Run
with -m gpu on an MI355X."""

import functools
import math

import pytest
import torch

import selection_cases as sc

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    import pvraft_amd.ops as ops


@pytest.fixture(scope="module", autouse=True)
def _require_gpu_and_ext():
    if not torch.cuda.is_available():
        pytest.skip("needs GPU")
    import pvraft_amd.ops as ops

    assert ops.hip_available(), "HIP extension must be built on the GPU box"


def dev():
    return torch.device("cuda:0")


def rows_distinct(idx):
    """(..., K) integer tensor -> (...) bool: no index twice in a row."""
    s = idx.sort(dim=-1).values
    return (s[..., 1:] != s[..., :-1]).all(-1)


# --------------------------------------------------------------------- kNN

@pytest.mark.parametrize("name", list(sc.KNN_CASES))
def test_knn_graph_exact_neighbour_sets(name):
    """The kernel forms d from three fp32 differences, three squares and two
    adds of the fp32 inputs: at most 6 roundings, a relative error below
    6 * 2^-24 = 3.6e-7 (no cancellation: all terms are >= 0).  It selects
    exactly on those d, so it can prefer a candidate at true distance t1 to
    one at t2 < t1 only if t1 / t2 <= (1 + 3.6e-7) / (1 - 3.6e-7) <
    1 + 1e-6.  Hence the sorted TRUE distances of the returned set match the
    k smallest true distances within rtol 1e-6, and atol 0."""
    xyz, k = sc.knn_case(name)
    xyz = xyz.to(dev())
    B, N, _ = xyz.shape
    idx = ops.knn_graph(xyz, k).long()
    assert idx.shape == (B, N, k)
    assert (idx >= 0).all() and (idx < N).all()
    distinct = rows_distinct(idx)
    assert distinct.all(), f"{(~distinct).sum().item()} of {B * N} queries repeat an index"
    has_self = (idx == torch.arange(N, device=dev()).view(1, N, 1)).any(-1)
    assert has_self.all(), f"{(~has_self).sum().item()} of {B * N} queries lack themselves"

    x = xyz.double()
    nb = x.gather(1, idx.reshape(B, N * k, 1).expand(B, N * k, 3)).view(B, N, k, 3)
    got = ((x.unsqueeze(2) - nb) ** 2).sum(-1).sort(dim=-1).values
    want = sc.knn_exact(xyz, k)
    bad = ((got - want).abs() > 1e-6 * want.abs()).any(-1)
    print(f"{name}: wrong neighbour sets {bad.sum().item()} of {B * N}")
    assert not bad.any(), f"{bad.sum().item()} of {B * N} neighbour sets are not the k nearest"


# ------------------------------------------------------ fused corr top-K

@functools.lru_cache(maxsize=None)
def _corr_inputs(name):
    f1t, f2t, K = sc.corr_case(name)
    f1t, f2t = f1t.to(dev()), f2t.to(dev())
    return f1t, f2t, K, sc.corr_exact(f1t, f2t), sc.corr_error_bound(f1t, f2t)


def check_corr_topk(name, v, i, ref, e, K):
    """e = C 2^-24 scale sum|f1||f2| bounds the fp32 result's distance from
    ref per entry (bf16 products are exact in fp32; C - 1 adds and the
    scaling round).  A kernel that selects exactly on its own values can
    take s and leave u only if ref[u] - e[u] <= ref[s] + e[s]."""
    B, N, M = ref.shape
    i = i.long()
    assert v.shape == (B, N, K) and i.shape == (B, N, K) and v.dtype == torch.float32
    assert (i >= 0).all() and (i < M).all()
    distinct = rows_distinct(i)
    assert distinct.all(), f"{name}: {(~distinct).sum().item()} of {B * N} rows repeat an index"
    off = (v.double() - ref.gather(2, i)).abs() - e.gather(2, i)
    assert (off <= 0).all(), f"{name}: value off by {off.max().item():.3e} beyond the bound"
    sel = torch.zeros(B, N, M, dtype=torch.bool, device=ref.device).scatter_(2, i, True)
    inf = torch.full_like(ref, math.inf)
    lo_sel = torch.where(sel, ref + e, inf).amin(-1)
    hi_uns = torch.where(sel, -inf, ref - e).amax(-1)
    bad = hi_uns > lo_sel
    print(f"{name}: wrong top-K sets {bad.sum().item()} of {B * N}")
    assert not bad.any(), f"{name}: {bad.sum().item()} of {B * N} rows are not a top-K set"


@pytest.mark.parametrize("name", list(sc.TOPK_CASES) + sc.CORR_TIE_CASES)
def test_corr_topk_exact_sets(name):
    from pvraft_amd import _C

    f1t, f2t, K, ref, e = _corr_inputs(name)
    v, i = _C.corr_topk(f1t, f2t, K)
    check_corr_topk(name, v, i, ref, e, K)


@pytest.mark.parametrize("name", [
    "gauss_1500_64", "gauss_8192_512_low1", "gauss_4096_256_low3",
    "gauss_8192_512_high10", "shelf_8192_512", "gauss_8192_1024",
    "lognormal_8192_1024", "tiedshelf_8192_512",
])
def test_corr_truncate_bf16_exact_sets(name):
    f1t, f2t, K, ref, e = _corr_inputs(name)
    M = f2t.shape[1]
    xyz2 = torch.randn(1, M, 3, device=dev(), generator=torch.Generator(dev()).manual_seed(5))
    corr, idx, txyz = ops.corr_truncate(
        f1t.transpose(1, 2).contiguous(), f2t.transpose(1, 2).contiguous(), xyz2, K)
    check_corr_topk(name, corr, idx, ref, e, K)
    N = f1t.shape[1]
    want = xyz2.gather(1, idx.reshape(1, N * K, 1).expand(1, N * K, 3).long()).view(1, N, K, 3)
    assert torch.equal(txyz, want)


# ------------------------------------------------------- fp32 row top-K

def check_rows_topk(name, vals, got_v, got_i, K):
    R, M = vals.shape
    got_i = got_i.long()
    assert got_v.shape == (R, K) and got_i.shape == (R, K)
    assert (got_i >= 0).all() and (got_i < M).all()
    assert torch.equal(got_v, vals.gather(1, got_i)), name
    distinct = rows_distinct(got_i)
    assert distinct.all(), f"{name}: {(~distinct).sum().item()} of {R} rows repeat an index"
    want_v, _ = sc.topk_exact(vals, K)
    bad = (got_v.sort(dim=1, descending=True).values != want_v).any(-1)
    print(f"{name}: wrong top-K sets {bad.sum().item()} of {R}")
    assert not bad.any(), f"{name}: {bad.sum().item()} of {R} rows are not the top K"


@pytest.mark.parametrize("name", list(sc.TOPK_CASES) + list(sc.TIE_CASES))
def test_topk_rows_exact_sets(name):
    from pvraft_amd import _C

    vals, K = sc.topk_rows_case(name)
    vals = vals.to(dev())
    got_v, got_i = _C.topk_rows(vals, K)
    check_rows_topk(name, vals, got_v, got_i, K)


@pytest.mark.parametrize("name", [
    "gauss_1000_256", "lognormal_8192_1024", "peaks300_1500_512",
    "gauss_8192_512_low10", "quantised_8192_512", "tiedshelf_8192_512",
])
def test_corr_truncate_fp32_exact_sets(name):
    """fp32 feature maps take the GEMM + topk_rows path.  With
    f1 = sqrt(C) I the product reproduces the rows bit for bit (one
    non-zero term per sum, sqrt(64) = 8 and the 1/8 scale are exact), so
    the checks stay exact."""
    vals, K = sc.topk_rows_case(name)
    vals = vals.to(dev())
    C, M = vals.shape
    assert C == 64
    f1 = (8.0 * torch.eye(C, device=dev())).unsqueeze(0)  # (1, C, N=C)
    xyz2 = torch.randn(1, M, 3, device=dev(), generator=torch.Generator(dev()).manual_seed(6))
    corr, idx, txyz = ops.corr_truncate(f1, vals.unsqueeze(0).contiguous(), xyz2, K)
    check_rows_topk(name, vals, corr[0], idx[0], K)
    want = xyz2.gather(1, idx.reshape(1, C * K, 1).expand(1, C * K, 3)).view(1, C, K, 3)
    assert torch.equal(txyz, want)
