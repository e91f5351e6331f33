"""GPU tests of the fused Chamfer (csrc/chamfer.hip) and flow-smoothness
(csrc/flow_smooth.hip) kernels against the dense fp64 oracle, and of one
eager SelfSupTrainer step.  Run with -m gpu."""

import argparse
import functools
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from selfsup_cases import dense_oracle, descent_epe, knn_dense, make_case

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    import pvraft_amd.ops as ops
    from pvraft_amd.model.graph import Graph
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

    return int(_C.CHAMFER_TILE)


def shapes():
    # N < M, N > M, single points, non-multiples of the 256-lane block,
    # T = 8, and two full LDS tiles plus a remainder
    return [
        (2, 300, 1000, 3),
        (2, 1000, 300, 2),
        (1, 2, 7, 2),
        (1, 1, 1, 1),
        (3, 127, 65, 1),
        (2, 257, 513, 8),
        (1, "2*tile+77", 3001, 2),
    ]


@functools.lru_cache(maxsize=None)
def gpu_case(B, N, M, T):
    """Inputs on the device, the graph (brute-force fp64 neighbours, so it
    does not depend on the kNN-graph kernel) and the dense fp64 oracle,
    computed once per shape and shared; nothing here is modified."""
    if isinstance(N, str):
        N = 2 * tile_pts() + 77
    pc1, flows, pc2 = (t.to(dev()) for t in make_case(B, N, M, T))
    graph = Graph(idx=knn_dense(pc1, 9), xyz=pc1)
    want = dense_oracle(pc1, flows, pc2, graph.idx)
    return pc1, flows, pc2, graph, want


def rows(t, idx):
    """t (B, S, 3), idx (T, B, Q) -> (T, B, Q, 3)"""
    T, B, Q = idx.shape
    return t.unsqueeze(0).expand(T, *t.shape).gather(2, idx.unsqueeze(-1).expand(T, B, Q, 3))


def chamfer_grad_formula(pc1, flows, pc2, i1, i2, g):
    """The closed-form flow gradient in fp64 on the given assignments."""
    T, B, N, _ = flows.shape
    M = pc2.shape[1]
    w = (pc1.unsqueeze(0) + flows).double()
    p2 = pc2.double()
    v1 = (i1 >= 0).unsqueeze(-1)
    out = 2.0 / (B * N) * torch.where(v1, w - rows(p2, i1.clamp_min(0)), torch.zeros_like(w))
    v2 = (i2 >= 0).unsqueeze(-1)
    tgt = i2.clamp_min(0).unsqueeze(-1).expand(T, B, M, 3)
    pull = torch.where(v2, w.gather(2, tgt) - p2.unsqueeze(0), torch.zeros(1, dtype=w.dtype, device=w.device))
    out = out + 2.0 / (B * M) * torch.zeros_like(w).scatter_add(2, tgt, pull)
    return g.double().view(T, 1, 1, 1) * out


def smooth_grad_formula(flows, idx, g):
    T, B, N, _ = flows.shape
    k = idx.shape[-1]
    f = flows.double()
    flat = idx.reshape(1, B, N * k, 1).expand(T, B, N * k, 3)
    e = f.unsqueeze(3).expand(T, B, N, k, 3).reshape(T, B, N * k, 3) - f.gather(2, flat)  # f_i - f_j per edge
    out = e.view(T, B, N, k, 3).sum(3) + torch.zeros_like(f).scatter_add(2, flat, -e)
    return g.double().view(T, 1, 1, 1) * 2.0 / (B * N * k) * out


@pytest.mark.parametrize("B,N,M,T", shapes())
def test_forward_matches_fp64_oracle(B, N, M, T):
    from pvraft_amd import _C

    pc1, flows, pc2, graph, want = gpu_case(B, N, M, T)
    cham, d1, i1, d2, i2 = _C.chamfer_fwd(pc1, flows, pc2)
    assert i1.dtype == torch.int32 and d1.shape == want["d1"].shape and d2.shape == want["d2"].shape
    assert torch.equal(i1.long(), want["i1"]) and torch.equal(i2.long(), want["i2"])
    e1 = (d1.double() - want["d1"]).abs().max().item()
    e2 = (d2.double() - want["d2"]).abs().max().item()
    print(f"max |d2 - fp64| = {e1:.3e} (warped->pc2)  {e2:.3e} (pc2->warped)")
    assert e1 <= 1e-4 and e2 <= 1e-4

    loss_c = ops.chamfer_loss(pc1, flows, pc2)
    loss_s = ops.flow_smoothness(flows, graph)
    assert torch.equal(loss_c, cham)
    rc = ((loss_c.double() - want["chamfer"]).abs() / want["chamfer"]).max().item()
    rs = ((loss_s.double() - want["smooth"]).abs() / want["smooth"].clamp_min(1e-300)).max().item()
    print(f"rel err chamfer {rc:.3e}  smooth {rs:.3e}")
    torch.testing.assert_close(loss_c.double(), want["chamfer"], rtol=2e-4, atol=0)
    torch.testing.assert_close(loss_s.double(), want["smooth"], rtol=2e-4, atol=0)

    # the one-direction primitive is the same sweep
    for t in range(flows.shape[0]):
        d, i = ops.chamfer_nn(pc1 + flows[t], pc2)
        assert i.dtype == torch.int64 and torch.equal(i, want["i1"][t])
        assert (d.double() - want["d1"][t]).abs().max().item() <= 1e-4


@pytest.mark.parametrize("B,N,M,T", shapes())
def test_backward_matches_closed_form_and_reference(B, N, M, T):
    from pvraft_amd import _C

    pc1, flows, pc2, graph, want = gpu_case(B, N, M, T)
    T = flows.shape[0]
    g = torch.randn(T, generator=torch.Generator().manual_seed(3)).to(dev())
    f = flows.clone().requires_grad_(True)
    (gc,) = torch.autograd.grad(ops.chamfer_loss(pc1, f, pc2), f, g)
    (gs,) = torch.autograd.grad(ops.flow_smoothness(f, graph), f, g)

    _, _, i1, _, i2 = _C.chamfer_fwd(pc1, flows, pc2)
    want_c = chamfer_grad_formula(pc1, flows, pc2, i1.long(), i2.long(), g)
    want_s = smooth_grad_formula(flows, graph.idx, g)

    f64 = flows.double().requires_grad_(True)
    (ref_c,) = torch.autograd.grad(R.chamfer_loss(pc1.double(), f64, pc2.double()), f64, g.double())
    (ref_s,) = torch.autograd.grad(R.flow_smoothness(f64, graph.idx), f64, g.double())

    for name, got, formula, ref in (("chamfer", gc, want_c, ref_c), ("smooth", gs, want_s, ref_s)):
        assert got.shape == flows.shape and got.dtype == torch.float32
        bound = 1e-5 * formula.abs().max().item()
        ef = (got.double() - formula).abs().max().item()
        er = (got.double() - ref).abs().max().item()
        print(f"{name}: max |grad - formula| = {ef:.3e}  max |grad - reference| = {er:.3e}  bound {bound:.3e}")
        assert ef <= bound and er <= bound


def test_two_calls_are_bit_identical():
    pc1, flows, pc2, graph, _ = gpu_case(2, 300, 1000, 3)
    g = torch.randn(3, generator=torch.Generator().manual_seed(4)).to(dev())

    def run():
        f = flows.clone().requires_grad_(True)
        c = ops.chamfer_loss(pc1, f, pc2)
        s = ops.flow_smoothness(f, graph)
        (gc,) = torch.autograd.grad(c, f, g)
        (gs,) = torch.autograd.grad(s, f, g)
        return c.detach(), s.detach(), gc, gs

    for a, b in zip(run(), run()):
        assert torch.equal(a, b)


def test_non_finite_points_never_win():
    from pvraft_amd import _C

    B, N, M, T = 2, 300, 1000, 3
    pc1, flows, pc2, _, _ = gpu_case(B, N, M, T)
    pc2 = pc2.clone()
    flows = flows.clone()
    pc2[1, 17] = float("nan")
    flows[2, 0, 5] = float("inf")
    f = flows.clone().requires_grad_(True)
    loss = ops.chamfer_loss(pc1, f, pc2)
    (grad,) = torch.autograd.grad(loss.sum(), f)
    cham, d1, i1, d2, i2 = _C.chamfer_fwd(pc1, flows, pc2)

    assert not (i1[:, 1] == 17).any()  # nobody's neighbour is the NaN row
    assert i1[2, 0, 5] == -1 and not (i2[2, 0] == 5).any()
    assert (i2[:, 1, 17] == -1).all()  # the NaN row finds no neighbour itself
    dead1 = torch.zeros_like(i1, dtype=torch.bool)
    dead1[2, 0, 5] = True
    dead2 = torch.zeros_like(i2, dtype=torch.bool)
    dead2[:, 1, 17] = True
    assert (i1[~dead1] >= 0).all() and (i2[~dead2] >= 0).all()
    assert torch.isfinite(d1[~dead1]).all() and torch.isfinite(d2[~dead2]).all()
    assert torch.isfinite(cham).all() and torch.isfinite(loss).all() and torch.equal(loss, cham)
    assert torch.isfinite(grad).all() and (grad[2, 0, 5] == 0).all()
    # the reference applies the same rules
    ref = R.chamfer_loss(pc1, flows, pc2)
    torch.testing.assert_close(loss, ref, rtol=2e-4, atol=0)


def test_chamfer_nn_agrees_with_knn_interpolate():
    pc1, flows, pc2, _, _ = gpu_case(2, 300, 1000, 3)
    q = pc1 + flows[0]
    d, i = ops.chamfer_nn(q, pc2)
    _, idx, _ = ops.knn_interpolate(pc2, pc2, q, k=1)
    assert torch.equal(i, idx[..., 0])


def test_eager_selfsup_train_step(tmp_path):
    from pvraft_amd.data import synthetic_batch
    from pvraft_amd.engine import SelfSupTrainer

    args = argparse.Namespace(
        root=str(tmp_path), exp_path="ss", dataset="SYNTH", max_points=256,
        corr_levels=3, base_scales=0.25, truncate_k=32, iters=2, gamma=0.8,
        batch_size=2, gpus="", num_epochs=1, weights=None, checkpoint_interval=5,
        refine=False, num_workers=0, amp=False, synth_len=4, hipgraph=True,
        self_supervised=True, chamfer_weight=1.0, smooth_weight=1.0, smooth_k=9,
    )
    t = SelfSupTrainer(args)
    assert t._graph_enabled()  # hipgraph is on: only the override keeps the step eager
    t.model.train()
    batch = synthetic_batch(2, 256, device=t.device, seed=11)
    loss, final = t.train_step(batch)
    assert torch.isfinite(loss) and final.shape == (2, 256, 3)
    assert getattr(t, "_graph_step", None) is None
    grads = [p.grad for p in t.model.parameters() if p.requires_grad]
    assert all(g is not None and torch.isfinite(g).all() for g in grads)
    assert any((g != 0).any() for g in grads)


def test_descent_through_hip_ops():
    epe = descent_epe(dev())
    print(f"final EPE {epe:.4f}")
    assert epe <= 0.027
