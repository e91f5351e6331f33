"""Ego-motion fit benchmark: the fused HIP robust rigid fit (one launch for
the whole IRLS loop) vs the pure-PyTorch reference loop on the same device.

    python scripts/ego_motion_bench.py [--thresh 0.05] [--min_seconds 1.0]

Seeded synthetic driving-like scenes, no external files.  Shapes (B, N) =
(1, 8192), (4, 8192), (1, 131072), each at 0 and 10 reweighting rounds.  Both
paths are warmed up, then timed with device events in alternating blocks
until each has accumulated --min_seconds of timed work.  If the batched 3x3
SVD is not available on the device the reference is timed on the CPU (wall
clock) and the line says so.  Prints one JSON line per shape and round
count:

  op_ms        fused kernel time per call
  ref_ms       torch reference time per call
  ref_over_op  their ratio
  ref_device   where the reference ran
  max_abs_dev  largest |kernel - reference| over R, t and the residuals
"""

import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np
import torch

import pvraft_amd.ops as ops
from pvraft_amd.ops import reference

SHAPES = [(1, 8192), (4, 8192), (1, 131072)]
ROUNDS = [0, 10]


def scene(B, N, seed):
    """Box cloud 30 x 4 x 30 m around (0, 0, 20); 70 % of the points follow
    one small rigid motion with 5 mm noise, the rest move on their own."""
    rng = np.random.default_rng(seed)
    pc = (rng.random((B, N, 3)) - 0.5) * np.array([30.0, 4.0, 30.0]) + np.array([0.0, 0.0, 20.0])
    v = np.array([0.01, 0.03, -0.005])
    K = np.array([[0, -v[2], v[1]], [v[2], 0, -v[0]], [-v[1], v[0], 0]])
    th = np.linalg.norm(v)
    R = np.eye(3) + np.sin(th) / th * K + (1 - np.cos(th)) / th**2 * (K @ K)
    dst = pc @ R.T + np.array([0.1, -0.05, 1.0]) + rng.normal(scale=0.005, size=pc.shape)
    dst[:, : int(0.3 * N)] += np.array([1.2, 0.0, 0.4])
    return torch.from_numpy(pc).float(), torch.from_numpy(dst).float()


def timed_block_gpu(fn, reps):
    start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(reps):
        fn()
    end.record()
    end.synchronize()
    return start.elapsed_time(end) * 1e-3


def timed_block_cpu(fn, reps):
    t0 = time.perf_counter()
    for _ in range(reps):
        fn()
    return time.perf_counter() - t0


def device_svd_works(dev):
    try:
        torch.linalg.svd(torch.eye(3, device=dev).expand(2, 3, 3).contiguous())
        torch.cuda.synchronize()
        return True
    except RuntimeError:
        return False


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--thresh", type=float, default=0.05)
    ap.add_argument("--min_seconds", type=float, default=1.0)
    ap.add_argument("--block_seconds", type=float, default=0.05)
    a = ap.parse_args()

    assert torch.cuda.is_available(), "ego_motion_bench needs a GPU"
    assert ops.hip_available(), "HIP extension is not built"
    dev = torch.device("cuda:0")
    ref_on_gpu = device_svd_works(dev)

    for B, N in SHAPES:
        src_c, dst_c = scene(B, N, seed=N + B)
        src, dst = src_c.to(dev), dst_c.to(dev)
        for iters in ROUNDS:
            hip = lambda: ops.rigid_fit(src, dst, None, a.thresh, iters)
            if ref_on_gpu:
                ref = lambda: reference.rigid_fit(src, dst, None, a.thresh, iters)
                timers = {"hip": timed_block_gpu, "ref": timed_block_gpu}
            else:
                ref = lambda: reference.rigid_fit(src_c, dst_c, None, a.thresh, iters)
                timers = {"hip": timed_block_gpu, "ref": timed_block_cpu}
            fns = {"hip": hip, "ref": ref}

            # same answer on the timed inputs before any timing
            got, want = hip(), ref()
            dev_max = max((g.cpu() - w.cpu()).abs().max().item() for g, w in zip(got[:3], want[:3]))

            est = {}
            for name in fns:
                timers[name](fns[name], 3)  # warm-up
                est[name] = timers[name](fns[name], 3) / 3
            reps = {n: max(1, int(a.block_seconds / est[n])) for n in est}
            tot = {"hip": 0.0, "ref": 0.0}
            cnt = {"hip": 0, "ref": 0}
            while min(tot.values()) < a.min_seconds:
                for name in fns:
                    tot[name] += timers[name](fns[name], reps[name])
                    cnt[name] += reps[name]
            op_s = tot["hip"] / cnt["hip"]
            ref_s = tot["ref"] / cnt["ref"]
            print(json.dumps({
                "shape": {"B": B, "N": N, "iters": iters, "thresh": a.thresh},
                "op_ms": round(op_s * 1e3, 4),
                "op_calls": cnt["hip"],
                "ref_ms": round(ref_s * 1e3, 4),
                "ref_calls": cnt["ref"],
                "ref_over_op": round(ref_s / op_s, 2),
                "ref_device": "gpu" if ref_on_gpu else "cpu (no device SVD)",
                "points_in_registers": N <= int(ops._load_ext().RIGID_FIT_REG_POINTS),
                "ok": bool(got[3].all().item()),
                "max_abs_dev": dev_max,
            }), flush=True)


if __name__ == "__main__":
    main()
