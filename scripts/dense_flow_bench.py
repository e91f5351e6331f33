"""Dense-flow interpolation benchmark: fused HIP kNN-interpolation op vs the
chunked pure-PyTorch reference on the same device, next to one Predictor
call, at the serving shape (8192 sampled points -> 131072-point scan).

    python scripts/dense_flow_bench.py [--n 8192] [--m 131072] [--k 3]

Seeded synthetic inputs, no external files.  Both ops are warmed up, then
timed with device events in alternating blocks until each has accumulated
--min_seconds of timed work.  Prints one JSON line:

  op_ms            fused op time per call
  ref_ms           torch reference time per call
  ref_over_op      their ratio
  predictor_ms     one --iters-iteration Predictor call at --n points
  op_share         op / (op + predictor call): share of a dense prediction
  dist_evals_per_s M * N / op time
"""

import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch

import pvraft_amd.ops as ops
from pvraft_amd.engine import Predictor
from pvraft_amd.model import PVRaft
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
    ap.add_argument("--n", type=int, default=8192, help="support (sampled) points")
    ap.add_argument("--m", type=int, default=131072, help="query (full-cloud) points")
    ap.add_argument("--c", type=int, default=3)
    ap.add_argument("--k", type=int, default=3)
    ap.add_argument("--iters", type=int, default=32)
    ap.add_argument("--truncate_k", type=int, default=512)
    ap.add_argument("--min_seconds", type=float, default=1.0)
    ap.add_argument("--block_seconds", type=float, default=0.05)
    ap.add_argument("--predictor_reps", type=int, default=10)
    ap.add_argument("--no-amp", dest="amp", action="store_false")
    a = ap.parse_args()

    assert torch.cuda.is_available(), "dense_flow_bench needs a GPU"
    assert ops.hip_available(), "HIP extension is not built"
    dev = torch.device("cuda:0")
    g = torch.Generator().manual_seed(0)
    # the full scan, and the network's sample of it as the support set
    full = ((torch.rand(1, a.m, 3, generator=g) - 0.5) * 10.0).to(dev)
    sel = torch.randperm(a.m, generator=g)[: a.n].to(dev)
    sup = full[:, sel].contiguous()
    val = torch.randn(1, a.n, a.c, generator=g).to(dev)

    hip = lambda: ops.knn_interpolate(sup, val, full, a.k)
    ref = lambda: reference.knn_interpolate(sup, val, full, a.k)

    # same answer on the timed inputs before any timing
    out_h, idx_h, _ = hip()
    out_r, idx_r, _ = ref()
    max_err = (out_h - out_r).abs().max().item()
    same_sets = (idx_h.sort(-1).values == idx_r.sort(-1).values).all(-1).float().mean().item()

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

    torch.manual_seed(0)
    model = PVRaft(truncate_k=a.truncate_k).to(dev).eval()
    pred = Predictor(model, points=a.n, batch=1, iters=a.iters, amp=a.amp)
    xyz1 = sup
    xyz2 = sup + 0.05 * torch.randn(1, a.n, 3, generator=g).to(dev)
    for _ in range(3):
        pred(xyz1, xyz2)
    torch.cuda.synchronize()
    calls = sorted(timed_block(lambda: pred(xyz1, xyz2), 1) for _ in range(a.predictor_reps))
    pred_s = calls[len(calls) // 2]

    print(json.dumps({
        "shape": {"B": 1, "N": a.n, "M": a.m, "C": a.c, "k": a.k},
        "op_ms": round(op_s * 1e3, 4),
        "op_calls": cnt["hip"],
        "ref_ms": round(ref_s * 1e3, 4),
        "ref_calls": cnt["ref"],
        "ref_over_op": round(ref_s / op_s, 2),
        "predictor_ms": round(pred_s * 1e3, 3),
        "predictor_iters": a.iters,
        "predictor_amp": a.amp,
        "predictor_graph": pred.use_graph,
        "op_share": round(op_s / (op_s + pred_s), 5),
        "dist_evals_per_s": float(f"{a.m * a.n / op_s:.4g}"),
        "max_abs_err_vs_ref": max_err,
        "same_neighbour_sets": same_sets,
    }))


if __name__ == "__main__":
    main()
