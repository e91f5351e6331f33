"""Self-supervised loss benchmark: fused HIP Chamfer + flow-smoothness
forward+backward vs the chunked pure-PyTorch reference forward+backward on
the same device, at the training shape (B=2, 8192 points, 8 GRU flows).

    python scripts/selfsup_loss_bench.py [--b 2] [--n 8192] [--m 8192] [--t 8] [--k 9]

Seeded synthetic inputs, no external files.  The kNN graph of pc1 and its
inverse adjacency are built once outside the timed region (a train step
builds them once per batch, whichever backend computes the loss).  Both
sides are warmed up, then timed with device events in alternating blocks
until each has accumulated --min_seconds of timed work.  Prints one JSON
line:

  op_ms            fused loss forward+backward per call
  ref_ms           torch reference forward+backward per call
  ref_over_op      their ratio
  dist_evals_per_s 2 * T * B * N * M / op time (both Chamfer directions)
  max_loss_diff    max |fused - reference| over the 2T loss terms
"""

import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch

import pvraft_amd.ops as ops
from pvraft_amd.model.graph import Graph
from pvraft_amd.ops import reference


def timed_block(fn, reps):
    start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(reps):
        fn()
    end.record()
    end.synchronize()
    return start.elapsed_time(end) * 1e-3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--b", type=int, default=2)
    ap.add_argument("--n", type=int, default=8192, help="points in pc1")
    ap.add_argument("--m", type=int, default=8192, help="points in pc2")
    ap.add_argument("--t", type=int, default=8, help="flows (GRU iterations)")
    ap.add_argument("--k", type=int, default=9, help="smoothness graph neighbours")
    ap.add_argument("--gamma", type=float, default=0.8)
    ap.add_argument("--min_seconds", type=float, default=1.0)
    ap.add_argument("--block_seconds", type=float, default=0.05)
    a = ap.parse_args()

    assert torch.cuda.is_available(), "selfsup_loss_bench needs a GPU"
    assert ops.hip_available(), "HIP extension is not built"
    dev = torch.device("cuda:0")
    g = torch.Generator().manual_seed(0)
    pc1 = ((torch.rand(a.b, a.n, 3, generator=g) - 0.5) * 10.0).to(dev)
    true_flow = 0.3 * torch.randn(a.b, a.n, 3, generator=g).to(dev)
    src = torch.randint(0, a.n, (a.b, a.m), generator=g).to(dev).unsqueeze(-1).expand(a.b, a.m, 3)
    pc2 = (pc1 + true_flow).gather(1, src) + 0.02 * torch.randn(a.b, a.m, 3, generator=g).to(dev)
    # a sequence of estimates approaching the true flow, as the GRU's are
    flows = torch.stack([
        true_flow * (t + 1) / a.t + 0.05 * torch.randn(a.b, a.n, 3, generator=g).to(dev) for t in range(a.t)
    ]).requires_grad_(True)
    weights = torch.tensor([a.gamma ** (a.t - 1 - t) for t in range(a.t)], device=dev)
    graph = Graph.build(pc1, a.k)
    graph.csr()

    def terms_hip():
        return ops.chamfer_loss(pc1, flows, pc2), ops.flow_smoothness(flows, graph)

    def terms_ref():
        return reference.chamfer_loss(pc1, flows, pc2), reference.flow_smoothness(flows, graph.idx)

    def step(terms):
        def run():
            cham, smooth = terms()
            flows.grad = None
            (weights * (cham + smooth)).sum().backward()
        return run

    hip, ref = step(terms_hip), step(terms_ref)

    # same answer on the timed inputs before any timing
    with torch.no_grad():
        ch, sh = terms_hip()
        cr, sr = terms_ref()
    max_diff = max((ch - cr).abs().max().item(), (sh - sr).abs().max().item())
    hip()
    grad_h = flows.grad.clone()
    ref()
    max_grad_diff = (grad_h - flows.grad).abs().max().item()

    est = {}
    for name, fn in (("hip", hip), ("ref", ref)):
        timed_block(fn, 3)  # warm-up
        est[name] = timed_block(fn, 3) / 3
    reps = {n: max(1, int(a.block_seconds / est[n])) for n in est}
    tot = {"hip": 0.0, "ref": 0.0}
    cnt = {"hip": 0, "ref": 0}
    while min(tot.values()) < a.min_seconds:
        for name, fn in (("hip", hip), ("ref", ref)):
            tot[name] += timed_block(fn, reps[name])
            cnt[name] += reps[name]
    op_s = tot["hip"] / cnt["hip"]
    ref_s = tot["ref"] / cnt["ref"]

    print(json.dumps({
        "shape": {"B": a.b, "N": a.n, "M": a.m, "T": a.t, "k": a.k},
        "op_ms": round(op_s * 1e3, 4),
        "op_calls": cnt["hip"],
        "ref_ms": round(ref_s * 1e3, 4),
        "ref_calls": cnt["ref"],
        "ref_over_op": round(ref_s / op_s, 2),
        "dist_evals_per_s": float(f"{2 * a.t * a.b * a.n * a.m / op_s:.4g}"),
        "max_loss_diff": max_diff,
        "max_grad_diff": max_grad_diff,
        "chamfer_last": ch[-1].item(),
        "smooth_last": sh[-1].item(),
    }))


if __name__ == "__main__":
    main()
