"""Ground-plane fit benchmark: the fused HIP path (csrc/plane_fit.hip, four
launches) vs the pure-PyTorch reference on the same device, and both against
one Predictor call.

    python scripts/ground_bench.py [--min_seconds 1.0] [--no_predictor]

Seeded synthetic LiDAR-like scenes, no external files: 40 % of the points on
a ground plane tilted 5 degrees (2 cm noise), 10 % on a vertical wall, the
rest 0.3-3 m above the ground.  N in {8192, 32768, 131072}, B = 1, 256
hypotheses, 3 refinement rounds.  All paths are warmed up, then timed with
device events in alternating blocks until each has accumulated --min_seconds
of timed work.  Prints one JSON line per N:

  op_ms         fused path, whole fit_plane call
  hyp_ms        fused path, hypotheses + scores only (plane_hypotheses)
  ref_ms        torch reference on the device, whole call
  ref_over_op   their ratio
  predictor_ms  one Predictor call (8192 points, 32 iterations, hipGraph)
  op_share      op_ms / predictor_ms
  same          best / count / rounds equal, plane within 1e-5
"""

import argparse
import json
import math
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np
import torch

import pvraft_amd.ops as ops
from pvraft_amd.ops import reference

SIZES = [8192, 32768, 131072]
HYPOTHESES = 256
ROUNDS = 3


def scene(N, seed):
    rng = np.random.default_rng(seed)
    t = math.radians(5.0)
    n = np.array([math.sin(t), math.cos(t), 0.0])
    d = 1.4 * n[1]
    xz = rng.uniform(-40.0, 40.0, size=(N, 2))
    n_g, n_w = int(0.4 * N), int(0.1 * N)
    y = -(d + n[0] * xz[:, 0] + n[2] * xz[:, 1]) / n[1]
    lift = rng.uniform(0.3, 3.0, size=N)
    lift[:n_g] = rng.normal(scale=0.02, size=n_g)
    pts = np.stack([xz[:, 0], y, xz[:, 1]], -1) + lift[:, None] * n
    pts[n_g:n_g + n_w, 0] = 8.0
    return torch.from_numpy(pts[rng.permutation(N)]).float().unsqueeze(0)


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
    ap.add_argument("--min_seconds", type=float, default=1.0)
    ap.add_argument("--block_seconds", type=float, default=0.05)
    ap.add_argument("--no_predictor", action="store_true")
    a = ap.parse_args()

    assert torch.cuda.is_available(), "ground_bench needs a GPU"
    assert ops.hip_available(), "HIP extension is not built"
    dev = torch.device("cuda:0")
    params = reference.plane_params(0.2, HYPOTHESES, (0.0, 1.0, 0.0), 20.0, ROUNDS, 0)
    thresh, thresh2, cos2, up32, H, iters, seed = params

    pred_call = None
    if not a.no_predictor:
        from pvraft_amd.engine import Predictor
        from pvraft_amd.model import PVRaft

        torch.manual_seed(0)
        pred = Predictor(PVRaft().to(dev).eval(), points=8192, batch=1, iters=32)
        p1 = scene(8192, seed=1).to(dev)
        p2 = p1 + torch.tensor([0.05, 0.0, 0.3], device=dev)
        pred_call = lambda: pred(p1, p2)

    for N in SIZES:
        x = scene(N, seed=N).to(dev)
        fns = {
            "hip": lambda: ops.fit_plane(x, hypotheses=HYPOTHESES, refine_iters=ROUNDS),
            "hyp": lambda: ops.plane_hypotheses(x, hypotheses=HYPOTHESES),
            "ref": lambda: reference.fit_plane(x, None, thresh, thresh2, cos2, up32, H, iters, seed),
        }
        if pred_call is not None:
            fns["pred"] = pred_call

        # same answer on the timed input before any timing
        got, want = fns["hip"](), ops.PlaneFit(*fns["ref"]())
        same = all(torch.equal(getattr(got, k), getattr(want, k)) for k in ("best", "count", "rounds", "ok"))
        same = same and (got.normal - want.normal).abs().max().item() <= 1e-5
        same = same and (got.offset - want.offset).abs().max().item() <= 1e-5

        est = {}
        for name, fn in fns.items():
            timed_block(fn, 3)  # warm-up
            est[name] = timed_block(fn, 3) / 3
        reps = {n: max(1, int(a.block_seconds / est[n])) for n in est}
        tot = {n: 0.0 for n in fns}
        cnt = {n: 0 for n in fns}
        while min(tot.values()) < a.min_seconds:
            for name, fn in fns.items():
                tot[name] += timed_block(fn, reps[name])
                cnt[name] += reps[name]
        ms = {n: tot[n] / cnt[n] * 1e3 for n in fns}
        line = {
            "shape": {"B": 1, "N": N, "hypotheses": HYPOTHESES, "refine_iters": ROUNDS},
            "op_ms": round(ms["hip"], 4),
            "op_calls": cnt["hip"],
            "hyp_ms": round(ms["hyp"], 4),
            "ref_ms": round(ms["ref"], 4),
            "ref_calls": cnt["ref"],
            "ref_over_op": round(ms["ref"] / ms["hip"], 2),
            "ground_ratio": round(got.ground.float().mean().item(), 4),
            "rounds": int(got.rounds[0]),
            "same": bool(same),
        }
        if pred_call is not None:
            line["predictor_ms"] = round(ms["pred"], 3)
            line["op_share"] = round(ms["hip"] / ms["pred"], 5)
        print(json.dumps(line), flush=True)


if __name__ == "__main__":
    main()
