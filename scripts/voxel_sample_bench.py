"""Voxel-stratified sampling benchmark: the HIP path (csrc/voxel_sample.hip,
10 + levels launches) vs the sort-based torch reference on the same device vs
``torch.randperm(n)[:m]``, one ``Predictor.predict_dense`` call with each
sampler, and the coverage both samplers reach.

    python scripts/voxel_sample_bench.py [--min_seconds 1.0] [--no_predictor]

Seeded synthetic LiDAR-like clouds, no external files: radius 2 + 33 u^2,
uniform angle, height N(0, 0.6).  N in {8192, 32768, 131072}, B = 1, m = 8192,
voxel 0.1, 10 levels.  All paths are warmed up, then timed with device events
in alternating blocks until each has accumulated --min_seconds of timed work;
the spread is the min / max over the blocks.  Prints one JSON line per N:

  op_ms          HIP path, whole voxel_sample call (op_ms_min / op_ms_max: blocks)
  ref_ms         torch reference on the device, whole call
  ref_over_op    their ratio
  randperm_ms    torch.randperm(n, device)[:m]
  predictor_ms   one Predictor call (8192 points, 32 iterations, hipGraph)
  op_share       op_ms / predictor_ms
  dense_random_ms / dense_voxel_ms   one predict_dense call with each sampler
  same           HIP and reference outputs equal
  cut_level      l* of the sample; p95 / max: nearest-sample distance of every
                 point, voxel sample and a seeded uniform sample
"""

import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np
import torch

import pvraft_amd.ops as ops
from pvraft_amd.ops import reference

SIZES = [8192, 32768, 131072]
M = 8192
VOXEL = 0.1
LEVELS = 10


def lidar(N, seed):
    rng = np.random.default_rng(seed)
    r = 2.0 + 33.0 * rng.random(N) ** 2
    a = rng.uniform(0.0, 2.0 * np.pi, N)
    y = rng.normal(0.0, 0.6, N)
    return torch.from_numpy(np.stack([r * np.cos(a), y, r * np.sin(a)], -1).astype(np.float32)).unsqueeze(0)


def nn_distance(points, samples, chunk=4096):
    out = []
    for s in range(0, points.shape[0], chunk):
        out.append(torch.cdist(points[s:s + chunk].double(), samples.double()).min(1).values)
    return torch.cat(out)


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

    assert torch.cuda.is_available(), "voxel_sample_bench needs a GPU"
    assert ops.hip_available(), "HIP extension is not built"
    dev = torch.device("cuda:0")
    m, inv, levels, seed = reference.voxel_params(M, VOXEL, LEVELS, 0)

    pred = None
    if not a.no_predictor:
        from pvraft_amd.engine import Predictor
        from pvraft_amd.model import PVRaft

        torch.manual_seed(0)
        pred = Predictor(PVRaft().to(dev).eval(), points=M, batch=1, iters=32)
        p1 = lidar(M, seed=1).to(dev)
        p2 = p1 + torch.tensor([0.05, 0.0, 0.3], device=dev)

    for N in SIZES:
        x = lidar(N, seed=N).to(dev)
        x2 = x + torch.tensor([0.05, 0.0, 0.3], device=dev)
        fns = {
            "hip": lambda: ops.voxel_sample(x, M, voxel=VOXEL, levels=LEVELS),
            "ref": lambda: reference.voxel_sample(x, m, inv, levels, None, seed),
            "randperm": lambda: torch.randperm(N, device=dev)[:M],
        }
        if pred is not None:
            fns["pred"] = lambda: pred(p1, p2)
            fns["dense_random"] = lambda: pred.predict_dense(x[0], x2[0], sampling="random")
            fns["dense_voxel"] = lambda: pred.predict_dense(x[0], x2[0], sampling="voxel")

        # same answer on the timed input before any timing
        got, want = fns["hip"](), ops.VoxelSample(*fns["ref"]())
        same = all(torch.equal(g, w) for g, w in zip(got, want))

        est = {}
        for name, fn in fns.items():
            timed_block(fn, 3)  # warm-up
            est[name] = timed_block(fn, 3) / 3
        reps = {n: max(1, int(a.block_seconds / est[n])) for n in est}
        tot = {n: 0.0 for n in fns}
        cnt = {n: 0 for n in fns}
        lo = {n: float("inf") for n in fns}
        hi = {n: 0.0 for n in fns}
        while min(tot.values()) < a.min_seconds:
            for name, fn in fns.items():
                t = timed_block(fn, reps[name])
                tot[name] += t
                cnt[name] += reps[name]
                lo[name] = min(lo[name], t / reps[name])
                hi[name] = max(hi[name], t / reps[name])
        ms = {n: tot[n] / cnt[n] * 1e3 for n in fns}

        pts = x[0]
        rnd = torch.from_numpy(np.random.default_rng(1000 + N).permutation(N)[:M]).to(dev)
        d_vox = nn_distance(pts, pts[got.idx[0]])
        d_rnd = nn_distance(pts, pts[rnd])
        covered = (got.occupied[0] <= M).nonzero()
        line = {
            "shape": {"B": 1, "N": N, "m": M, "voxel": VOXEL, "levels": LEVELS},
            "op_ms": round(ms["hip"], 4),
            "op_ms_min": round(lo["hip"] * 1e3, 4),
            "op_ms_max": round(hi["hip"] * 1e3, 4),
            "op_calls": cnt["hip"],
            "ref_ms": round(ms["ref"], 4),
            "ref_ms_min": round(lo["ref"] * 1e3, 4),
            "ref_ms_max": round(hi["ref"] * 1e3, 4),
            "ref_calls": cnt["ref"],
            "ref_over_op": round(ms["ref"] / ms["hip"], 2),
            "randperm_ms": round(ms["randperm"], 4),
            "same": bool(same),
            "count": int(got.count[0]),
            "occupied": got.occupied[0].tolist(),
            "cut_level": int(covered[0]) if covered.numel() else None,
            "p95_voxel": round(torch.quantile(d_vox, 0.95).item(), 4),
            "p95_random": round(torch.quantile(d_rnd, 0.95).item(), 4),
            "max_voxel": round(d_vox.max().item(), 4),
            "max_random": round(d_rnd.max().item(), 4),
        }
        if pred is not None:
            line["predictor_ms"] = round(ms["pred"], 3)
            line["op_share"] = round(ms["hip"] / ms["pred"], 5)
            line["dense_random_ms"] = round(ms["dense_random"], 3)
            line["dense_voxel_ms"] = round(ms["dense_voxel"], 3)
        print(json.dumps(line), flush=True)


if __name__ == "__main__":
    main()
