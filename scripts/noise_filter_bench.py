"""Noise-filter benchmark: the HIP path (csrc/noise_filter.hip, 9 launches) vs
the brute-force torch reference on the same device vs one ``Predictor`` call,
and what the filter's mask does to the voxel sample.

    python scripts/noise_filter_bench.py [--min_seconds 1.0] [--no_predictor] [--no_reference]

Seeded synthetic clouds, no external files, N in {8192, 32768, 131072}, B = 1,
the op's defaults (radius 0.5, 4 neighbours, k = 8, 2 sigma):

  lidar    radius 2 + 33 u^2, uniform angle, height N(0, 0.6)
  patches  60 planar 2 m x 2 m patches with 1 cm noise in a 40 x 6 x 40 m
           volume, 1.1 % of the points isolated and uniform in it

The HIP path and the Predictor are warmed up, then timed with device events in
alternating blocks until each has accumulated --min_seconds of timed work; the
spread is the min / max over the blocks.  The reference sweeps all pairs, so
it gets one warm-up call and as many timed calls as fit in --min_seconds, at
least one.  Prints one JSON line per cloud and N:

  op_ms          HIP path, whole noise_filter call (op_ms_min / op_ms_max: blocks)
  ref_ms         torch reference on the device, whole call (ref_calls of them)
  ref_over_op    their ratio
  predictor_ms   one Predictor call (8192 points, 32 iterations, hipGraph)
  op_share       op_ms / predictor_ms
  same           count and mean_dist bit-equal to the reference, keep equal
  kept / sparse / far   shares of the points
  patches only, m = min(8192, N / 4) voxel samples:
  injected_in_sample / injected_in_masked_sample   injected points among them
                 without and with mask = keep; surface_flagged: surface points
                 the filter flags
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
POINTS = 8192


def lidar(N, seed):
    rng = np.random.default_rng(seed)
    r = 2.0 + 33.0 * rng.random(N) ** 2
    a = rng.uniform(0.0, 2.0 * np.pi, N)
    y = rng.normal(0.0, 0.6, N)
    return np.stack([r * np.cos(a), y, r * np.sin(a)], -1).astype(np.float32), None


def patches(N, seed, n_patches=60, noise_share=0.011):
    rng = np.random.default_rng(seed)
    lo, hi = np.array([-20.0, -2.0, -20.0]), np.array([20.0, 4.0, 20.0])
    n_noise = int(round(noise_share * N))
    n_surf = N - n_noise
    centre = rng.uniform(lo + 1.0, hi - 1.0, size=(n_patches, 3))
    normal = rng.normal(size=(n_patches, 3))
    normal /= np.linalg.norm(normal, axis=1, keepdims=True)
    u = np.cross(normal, rng.normal(size=(n_patches, 3)))
    u /= np.linalg.norm(u, axis=1, keepdims=True)
    v = np.cross(normal, u)
    pid = rng.integers(0, n_patches, n_surf)
    a, b = rng.uniform(-1.0, 1.0, (2, n_surf))
    surf = centre[pid] + a[:, None] * u[pid] + b[:, None] * v[pid] + rng.normal(0.0, 0.01, (n_surf, 1)) * normal[pid]
    p = np.concatenate([surf, rng.uniform(lo, hi, size=(n_noise, 3))]).astype(np.float32)
    injected = np.arange(N) >= n_surf
    order = rng.permutation(N)
    return p[order], injected[order]


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
    ap.add_argument("--no_reference", action="store_true")
    a = ap.parse_args()

    assert torch.cuda.is_available(), "noise_filter_bench needs a GPU"
    assert ops.hip_available(), "HIP extension is not built"
    dev = torch.device("cuda:0")
    inv, r2, min_nb, k, ratio = reference.noise_params(0.5, 4, 8, 2.0)

    pred = None
    if not a.no_predictor:
        from pvraft_amd.engine import Predictor
        from pvraft_amd.model import PVRaft

        torch.manual_seed(0)
        pred = Predictor(PVRaft().to(dev).eval(), points=POINTS, batch=1, iters=32)
        p1 = torch.from_numpy(lidar(POINTS, seed=1)[0]).unsqueeze(0).to(dev)
        p2 = p1 + torch.tensor([0.05, 0.0, 0.3], device=dev)

    for cloud, build in (("lidar", lidar), ("patches", patches)):
        for N in SIZES:
            pts, injected = build(N, seed=N)
            x = torch.from_numpy(pts).unsqueeze(0).to(dev)
            fns = {"hip": lambda: ops.noise_filter(x)}
            if pred is not None:
                fns["pred"] = lambda: pred(p1, p2)
            got = fns["hip"]()

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

            el = got.count[0] >= 0
            far = el & ((got.count[0] < k) | (got.mean_dist[0].double() > got.threshold[0]))
            line = {
                "cloud": cloud,
                "shape": {"B": 1, "N": N, "radius": 0.5, "min_neighbors": min_nb, "k": k, "std_ratio": ratio},
                "op_ms": round(ms["hip"], 4),
                "op_ms_min": round(lo["hip"] * 1e3, 4),
                "op_ms_max": round(hi["hip"] * 1e3, 4),
                "op_calls": cnt["hip"],
                "ok": bool(got.ok[0]),
                "kept": round(got.keep.float().mean().item(), 4),
                "sparse": round((el & (got.count[0] < min_nb)).float().mean().item(), 4),
                "far": round(far.float().mean().item(), 4),
                "mean_neighbours": round(got.count[0][el].float().mean().item(), 2),
            }
            if not a.no_reference:
                ref_fn = lambda: reference.noise_filter(x, inv, r2, min_nb, k, ratio, None)
                want = ref_fn()  # warm-up, and the comparison
                torch.cuda.synchronize()
                line["same"] = bool(torch.equal(got.count, want[1]) and torch.equal(got.mean_dist, want[2])
                                    and torch.equal(got.keep, want[0]))
                rt, rc = 0.0, 0
                while rc == 0 or rt < a.min_seconds:
                    rt += timed_block(ref_fn, 1)
                    rc += 1
                line.update(ref_ms=round(rt / rc * 1e3, 3), ref_calls=rc,
                            ref_over_op=round(rt / rc * 1e3 / ms["hip"], 1))
            if pred is not None:
                line["predictor_ms"] = round(ms["pred"], 3)
                line["op_share"] = round(ms["hip"] / ms["pred"], 5)
            if injected is not None:
                m = min(POINTS, N // 4)
                inj = torch.from_numpy(injected).to(dev)
                plain = ops.voxel_sample(x, m).idx[0]
                masked = ops.voxel_sample(x, m, mask=got.keep).idx[0]
                masked = masked[masked >= 0]
                line.update(m=m, injected=int(inj.sum()), injected_in_sample=int(inj[plain].sum()),
                            injected_in_masked_sample=int(inj[masked].sum()), masked_sample=int(masked.numel()),
                            surface_flagged=int((~got.keep[0] & ~inj).sum()), surface=int((~inj).sum()))
            print(json.dumps(line), flush=True)


if __name__ == "__main__":
    main()
