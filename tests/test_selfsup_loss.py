"""CPU tests of the self-supervised loss: the reference ops against a dense
fp64 formula, gradcheck, self_supervised_loss behaviour, a descent sanity
check and the --self_supervised CLI."""

import os
import subprocess
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import pvraft_amd.ops as ops
from pvraft_amd.model.graph import Graph
from pvraft_amd.utils import self_supervised_loss
from selfsup_cases import dense_oracle, descent_epe, knn_dense, make_case

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = [(2, 300, 1000, 3), (1, 2, 7, 2), (1, 1, 1, 1)]
K = 9


def graph_of(pc1, k=K):
    return Graph(idx=knn_dense(pc1, k), xyz=pc1)


@pytest.mark.parametrize("B,N,M,T", SHAPES)
@pytest.mark.parametrize("dtype,rtol", [(torch.float32, 1e-6), (torch.float64, 1e-12)])
def test_reference_ops_match_dense_formula(B, N, M, T, dtype, rtol):
    pc1, flows, pc2 = (t.to(dtype) for t in make_case(B, N, M, T))
    graph = graph_of(pc1)
    want = dense_oracle(pc1, flows, pc2, graph.idx)

    for t in range(T):
        w = pc1 + flows[t]
        for (q, s, dk, ik) in ((w, pc2, "d1", "i1"), (pc2, w, "d2", "i2")):
            d, i = ops.chamfer_nn(q, s)
            assert d.dtype == dtype and i.dtype == torch.int64
            assert torch.equal(i, want[ik][t])
            torch.testing.assert_close(d.double(), want[dk][t], rtol=rtol, atol=0)

    cham = ops.chamfer_loss(pc1, flows, pc2)
    smooth = ops.flow_smoothness(flows, graph)
    assert cham.shape == (T,) and smooth.shape == (T,)
    assert cham.dtype == dtype and smooth.dtype == dtype
    print(f"chamfer rel err {((cham.double() - want['chamfer']) / want['chamfer']).abs().max():.2e}  "
          f"smooth rel err {((smooth.double() - want['smooth']).abs() / want['smooth'].clamp_min(1e-300)).max():.2e}")
    torch.testing.assert_close(cham.double(), want["chamfer"], rtol=rtol, atol=0)
    torch.testing.assert_close(smooth.double(), want["smooth"], rtol=rtol, atol=0)
    # a list of flows and a stacked tensor are the same thing
    assert torch.equal(ops.chamfer_loss(pc1, list(flows), pc2), cham)
    assert torch.equal(ops.flow_smoothness(list(flows), graph), smooth)


def test_ties_and_non_finite_rules():
    q = torch.tensor([[[0.0, 0.0, 0.0], [float("inf"), 0.0, 0.0], [5.0, 0.0, 0.0]]])
    s = torch.tensor([[[1.0, 0.0, 0.0], [float("nan"), 0.0, 0.0], [-1.0, 0.0, 0.0], [0.0, 1.0, 0.0]]])
    d, i = ops.chamfer_nn(q, s)
    assert i.tolist() == [[0, -1, 0]]  # three candidates tie for query 0
    assert d[0, 0] == 1.0 and d[0, 1] == float("inf") and d[0, 2] == 16.0
    flow = torch.zeros(1, 3, 3, requires_grad=True)
    loss = ops.chamfer_loss(q, flow, s)
    assert torch.isfinite(loss).all()
    loss.sum().backward()
    assert torch.isfinite(flow.grad).all() and (flow.grad[0, 1] == 0).all()


def test_gradcheck_fp64():
    B, N, M, T, k = 1, 6, 5, 2, 3
    pc1, flows, pc2 = (t.double() for t in make_case(B, N, M, T))
    graph = graph_of(pc1, k)
    f = flows.clone().requires_grad_(True)
    assert torch.autograd.gradcheck(lambda x: ops.chamfer_loss(pc1, x, pc2), (f,))
    assert torch.autograd.gradcheck(lambda x: ops.flow_smoothness(x, graph), (f,))
    # coordinates get no gradient
    p1 = pc1.clone().requires_grad_(True)
    p2 = pc2.clone().requires_grad_(True)
    ops.chamfer_loss(p1, f, p2).sum().backward()
    assert p1.grad is None and p2.grad is None and f.grad is not None


def test_self_supervised_loss_behaviour():
    B, N, M, T = 2, 300, 1000, 3
    pc1, flows, pc2 = make_case(B, N, M, T)
    gamma, cw, sw = 0.7, 1.5, 0.25
    batch = {"sequence": [pc1, pc2], "ground_truth": [torch.ones(B, N, 1), torch.zeros(B, N, 3)]}
    loss = self_supervised_loss(list(flows), batch, gamma=gamma, chamfer_weight=cw, smooth_weight=sw)
    assert loss.dim() == 0

    garbage = {"sequence": [pc1, pc2], "ground_truth": [torch.full((B, N, 1), float("nan")), "not a tensor"]}
    assert torch.equal(self_supervised_loss(list(flows), garbage, gamma=gamma, chamfer_weight=cw, smooth_weight=sw), loss)
    assert torch.equal(self_supervised_loss(list(flows), {"sequence": [pc1, pc2]}, gamma=gamma,
                                            chamfer_weight=cw, smooth_weight=sw), loss)

    graph = Graph.build(pc1, K)
    cham = ops.chamfer_loss(pc1, flows, pc2)
    smooth = ops.flow_smoothness(flows, graph)
    want = sum(gamma ** (T - 1 - t) * (cw * cham[t] + sw * smooth[t]) for t in range(T))
    torch.testing.assert_close(loss, want, rtol=1e-6, atol=0)
    assert torch.equal(
        self_supervised_loss(list(flows), batch, gamma=gamma, chamfer_weight=cw, smooth_weight=sw, graph=graph), loss
    )

    # a bare tensor is one flow, weight gamma^0
    single = self_supervised_loss(flows[1], batch)
    want1 = ops.chamfer_loss(pc1, flows[1], pc2)[0] + ops.flow_smoothness(flows[1], graph)[0]
    torch.testing.assert_close(single, want1, rtol=1e-6, atol=0)


def test_descent_recovers_a_rigid_shift():
    epe = descent_epe("cpu")
    print(f"final EPE {epe:.4f}")
    assert epe <= 0.027


def ss_flags(tmp_path):
    return [
        os.path.join(REPO, "train.py"), "--self_supervised", "--root", str(tmp_path), "--dataset", "SYNTH",
        "--max_points", "48", "--truncate_k", "16", "--iters", "2", "--synth_len", "4", "--batch_size", "2",
        "--num_epochs", "1", "--num_workers", "0", "--gpus", "",
    ]


def test_self_supervised_cli(tmp_path):
    cmd = [sys.executable] + ss_flags(tmp_path) + ["--exp_path", "ss_exp"]
    out = subprocess.run(cmd, capture_output=True, text=True, timeout=600, cwd=REPO)
    assert out.returncode == 0, f"--- stdout\n{out.stdout[-1500:]}\n--- stderr\n{out.stderr[-3000:]}"
    assert os.path.exists(
        os.path.join(str(tmp_path), "experiments", "ss_exp", "checkpoints", "best_checkpoint.params")
    )


def test_self_supervised_refine_is_rejected(tmp_path):
    cmd = [sys.executable] + ss_flags(tmp_path) + ["--refine"]
    out = subprocess.run(cmd, capture_output=True, text=True, timeout=120, cwd=REPO)
    assert out.returncode != 0
    assert "--self_supervised cannot be combined with --refine" in out.stderr
