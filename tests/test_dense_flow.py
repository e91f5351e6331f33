"""Dense scene flow on the CPU path: the kNN-interpolation reference op
against a brute-force float64 computation, its autograd, and the layers
built on it (Predictor.predict_dense, dataset "full" clouds, Batch,
test.py --dense)."""

import ast
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import pvraft_amd.ops as ops
from pvraft_amd.data import Batch, SyntheticSceneFlow
from pvraft_amd.ops import reference as R

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

SHAPES = [(2, 300, 1000, 3, 3), (1, 2, 7, 3, 3), (2, 257, 513, 64, 16)]


def make_case(B, N, M, C, device="cpu"):
    """randn*3 clouds; the first half of the queries are copies of support
    points (query j of batch b sits on support src[b, j])."""
    g = torch.Generator().manual_seed(1000 * N + M)
    sup = torch.randn(B, N, 3, generator=g) * 3
    val = torch.randn(B, N, C, generator=g)
    qry = torch.randn(B, M, 3, generator=g) * 3
    half = M // 2
    src = torch.stack([torch.randint(0, N, (half,), generator=g) for _ in range(B)])
    qry[:, :half] = sup.gather(1, src.unsqueeze(-1).expand(B, half, 3))
    return sup.to(device), val.to(device), qry.to(device), src.to(device)


def brute_force_f64(sup, val, qry, k, eps=1e-8):
    sup, val, qry = sup.double(), val.double(), qry.double()
    B, N, C = val.shape
    ke = min(k, N)
    d2 = ((qry.unsqueeze(2) - sup.unsqueeze(1)) ** 2).sum(-1)  # B, M, N
    d, i = d2.topk(ke, dim=-1, largest=False, sorted=True)
    w = 1.0 / (d + eps)
    w = w / w.sum(-1, keepdim=True)
    nb = torch.stack([val[b][i[b]] for b in range(B)])  # B, M, ke, C
    return (w.unsqueeze(-1) * nb).sum(2), i, w


@pytest.mark.parametrize("B,N,M,C,k", SHAPES)
def test_reference_matches_brute_force_float64(B, N, M, C, k):
    sup, val, qry, src = make_case(B, N, M, C)
    out, idx, w = R.knn_interpolate(sup, val, qry, k=k)
    want, widx, _ = brute_force_f64(sup, val, qry, k)
    ke = min(k, N)
    assert out.shape == (B, M, C) and idx.shape == (B, M, ke) and w.shape == (B, M, ke)
    assert idx.dtype == torch.int64
    assert torch.equal(idx.sort(-1).values, widx.sort(-1).values)
    err = (out.double() - want).abs().max().item()
    print(f"max |out - f64| = {err:.3e}")
    assert err <= 1e-4
    # ascending distance, distinct neighbours, normalised weights
    assert (w[..., :-1] >= w[..., 1:]).all()
    assert (idx.sort(-1).values.diff(dim=-1) > 0).all()
    assert torch.allclose(w.sum(-1), torch.ones(B, M), atol=1e-5)
    # a query sitting on a support point returns that point's value
    half = M // 2
    on_point = val.gather(1, src.unsqueeze(-1).expand(B, half, C))
    cerr = (out[:, :half] - on_point).abs().max().item()
    print(f"coincident-query error = {cerr:.3e}")
    assert cerr <= 2e-5


def test_chunking_does_not_change_the_result():
    sup, val, qry, _ = make_case(2, 300, 1000, 3)
    a = R.knn_interpolate(sup, val, qry, k=3, chunk=4096)
    b = R.knn_interpolate(sup, val, qry, k=3, chunk=97)
    assert torch.equal(a[1], b[1])
    assert torch.allclose(a[0], b[0], atol=1e-6)


def test_constant_field_is_reproduced():
    sup, _, qry, _ = make_case(2, 300, 1000, 3)
    val = torch.full((2, 300, 3), 2.5)
    for fn in (R.knn_interpolate, ops.knn_interpolate):
        out, _, _ = fn(sup, val, qry, k=5)
        assert (out - 2.5).abs().max().item() <= 1e-6


def test_fewer_support_points_than_k():
    sup, val, qry, _ = make_case(1, 2, 7, 3)
    out, idx, w = ops.knn_interpolate(sup, val, qry, k=3)
    assert idx.shape == (1, 7, 2) and w.shape == (1, 7, 2) and out.shape == (1, 7, 3)
    assert (idx.sort(-1).values == torch.tensor([0, 1])).all()


@pytest.mark.parametrize("k", [0, 17])
def test_k_out_of_range_raises(k):
    sup, val, qry, _ = make_case(1, 20, 15, 2)
    with pytest.raises(ValueError):
        R.knn_interpolate(sup, val, qry, k=k)
    with pytest.raises(ValueError):
        ops.knn_interpolate(sup, val, qry, k=k)


def test_op_upcasts_bf16_and_strided_inputs():
    sup, val, qry, _ = make_case(2, 64, 40, 4)
    want, widx, _ = ops.knn_interpolate(sup, val, qry, k=3)
    strided = torch.empty(2, 64, 8)[..., ::2]
    strided.copy_(val)
    assert not strided.is_contiguous()
    got, gidx, _ = ops.knn_interpolate(sup, strided, qry, k=3)
    assert torch.equal(gidx, widx) and torch.allclose(got, want)
    got, _, _ = ops.knn_interpolate(sup, val.bfloat16(), qry, k=3)
    assert got.dtype == torch.float32
    assert torch.allclose(got, ops.knn_interpolate(sup, val.bfloat16().float(), qry, k=3)[0])


def test_gradcheck_values_only():
    g = torch.Generator().manual_seed(3)
    sup = torch.randn(1, 20, 3, generator=g, dtype=torch.float64)
    qry = torch.randn(1, 15, 3, generator=g, dtype=torch.float64)
    val = torch.randn(1, 20, 2, generator=g, dtype=torch.float64, requires_grad=True)
    for fn in (R.knn_interpolate, ops.knn_interpolate):
        assert torch.autograd.gradcheck(lambda v: fn(sup, v, qry, k=3)[0], (val,))
    # coordinates get no gradient
    sup_g = sup.clone().requires_grad_(True)
    qry_g = qry.clone().requires_grad_(True)
    out, _, _ = ops.knn_interpolate(sup_g, val, qry_g, k=3)
    out.sum().backward()
    assert sup_g.grad is None and qry_g.grad is None and val.grad is not None


# ---------------------------------------------------------------------------
# Predictor.predict_dense
# ---------------------------------------------------------------------------


@pytest.fixture(scope="module")
def tiny_predictor():
    from pvraft_amd.engine import Predictor
    from pvraft_amd.model import PVRaft

    torch.manual_seed(11)
    model = PVRaft(truncate_k=16).eval()
    return Predictor(model, points=48, batch=1, iters=2)


def full_clouds(n1=200, n2=200, seed=4):
    g = torch.Generator().manual_seed(seed)
    pc1 = torch.randn(n1, 3, generator=g)
    pc2 = torch.randn(n2, 3, generator=g) * 0.05 + pc1[torch.randint(0, n1, (n2,), generator=g)]
    return pc1, pc2


def test_predict_dense_cpu(tiny_predictor):
    pc1, pc2 = full_clouds()
    gen = torch.Generator().manual_seed(9)
    dense, idx1, flow_sub = tiny_predictor.predict_dense(pc1, pc2, k=3, generator=gen, return_sparse=True)
    assert dense.shape == (200, 3) and dense.dtype == pc1.dtype
    assert idx1.shape == (48,) and flow_sub.shape == (48, 3)
    assert idx1.unique().numel() == 48
    assert torch.isfinite(dense).all()
    assert (dense[idx1] - flow_sub).abs().max().item() <= 1e-4

    again = tiny_predictor.predict_dense(pc1.unsqueeze(0), pc2.unsqueeze(0), k=3,
                                         generator=torch.Generator().manual_seed(9))
    assert torch.equal(again, dense)


def test_predict_dense_rejects_small_clouds_and_batches(tiny_predictor):
    from pvraft_amd.engine import Predictor

    pc1, pc2 = full_clouds()
    small, _ = full_clouds(n1=40, n2=40)
    with pytest.raises(ValueError, match=r"40\b.*\b48\b"):
        tiny_predictor.predict_dense(small, pc2)
    with pytest.raises(ValueError, match=r"40\b.*\b48\b"):
        tiny_predictor.predict_dense(pc1, small)
    two = Predictor(tiny_predictor.model, points=48, batch=2, iters=2)
    with pytest.raises(ValueError):
        two.predict_dense(pc1, pc2)


# ---------------------------------------------------------------------------
# dataset / Batch
# ---------------------------------------------------------------------------


def test_return_full_keeps_the_subsample():
    plain = SyntheticSceneFlow(nb_points=32, length=3, seed=5, full_points=100)
    withfull = SyntheticSceneFlow(nb_points=32, length=3, seed=5, full_points=100)
    withfull.return_full = True
    assert SyntheticSceneFlow.return_full is False
    np.random.seed(42)
    a = plain[1]
    np.random.seed(42)
    b = withfull[1]
    assert "full" not in a
    pc1_full, mask_full, flow_full = b["full"]
    assert pc1_full.shape == (1, 100, 3) and mask_full.shape == (1, 100, 1) and flow_full.shape == (1, 100, 3)
    for key in ("sequence", "ground_truth"):
        for x, y in zip(a[key], b[key]):
            assert torch.equal(x, y)
    assert b["sequence"][0].shape == (1, 32, 3)
    # every sampled point (and its ground truth) is a row of the full cloud
    match = (b["sequence"][0][0].unsqueeze(1) == pc1_full[0].unsqueeze(0)).all(-1)
    assert (match.sum(1) == 1).all()
    assert torch.equal(flow_full[0][match.float().argmax(1)], b["ground_truth"][1][0])


def test_full_points_none_is_the_historical_stream():
    a = SyntheticSceneFlow(nb_points=32, length=2, seed=3)
    b = SyntheticSceneFlow(nb_points=32, length=2, seed=3, full_points=None)
    for x, y in zip(a.load_sequence(1)[0], b.load_sequence(1)[0]):
        assert np.array_equal(x, y)
    assert a.load_sequence(0)[0][0].shape == (32, 3)


def test_batch_carries_full_for_one_sample_only():
    ds = SyntheticSceneFlow(nb_points=16, length=2, full_points=50)
    ds.return_full = True
    one = Batch([ds[0]]).to(torch.float64)
    assert len(one["full"]) == 3 and one["full"][0].shape == (1, 50, 3)
    assert all(t.dtype == torch.float64 for t in one["full"])
    with pytest.raises(ValueError):
        Batch([ds[0], ds[1]])
    ds.return_full = False
    with pytest.raises(KeyError):
        Batch([ds[0], ds[1]])["full"]


# ---------------------------------------------------------------------------
# test.py --dense
# ---------------------------------------------------------------------------

DENSE_KEYS = ("dense_epe", "dense_acc3d_strict", "dense_acc3d_relax", "dense_outlier")


def run_test_cli(tmp_path, extra):
    args = [
        sys.executable, os.path.join(REPO, "test.py"), "--root", str(tmp_path),
        "--dataset", "SYNTH", "--max_points", "48", "--truncate_k", "16", "--iters", "2",
        "--synth_len", "2", "--num_workers", "0", "--gpus", "", "--dump_results",
    ] + extra
    out = subprocess.run(args, capture_output=True, text=True, timeout=600, cwd=REPO)
    assert out.returncode == 0, f"--- stdout\n{out.stdout[-1500:]}\n--- stderr\n{out.stderr[-3000:]}"
    results = ast.literal_eval(out.stdout.strip().splitlines()[-1])
    return results, os.path.join(str(tmp_path), "result", "SYNTH", "0")


def test_cli_dense(tmp_path):
    results, dumped = run_test_cli(tmp_path, ["--dense"])
    for key in DENSE_KEYS + ("epe", "loss"):
        assert key in results and np.isfinite(results[key]), key
    flow_dense = np.load(os.path.join(dumped, "flow_dense.npy")).reshape(-1, 3)
    pc1_full = np.load(os.path.join(dumped, "pc1_full.npy")).reshape(-1, 3)
    assert flow_dense.shape == (4 * 48, 3) and pc1_full.shape == (4 * 48, 3)
    assert np.load(os.path.join(dumped, "flow.npy")).reshape(-1, 3).shape == (48, 3)

    out = subprocess.run(
        [sys.executable, os.path.join(REPO, "visual.py"), "--root", str(tmp_path),
         "--dataset", "SYNTH", "--index", "0"],
        capture_output=True, text=True, timeout=300, cwd=REPO,
    )
    assert out.returncode == 0, out.stderr[-2000:]
    assert os.path.exists(os.path.join(dumped, "view.png"))


def test_cli_without_dense_is_unchanged(tmp_path):
    results, dumped = run_test_cli(tmp_path, [])
    assert set(results) == {"loss", "epe", "acc3d_strict", "acc3d_relax", "outlier"}
    assert sorted(os.listdir(dumped)) == ["flow.npy", "pc1.npy", "pc2.npy"]
