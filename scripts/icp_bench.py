"""Grid-search / ICP benchmark: the HIP paths (csrc/grid_nn.hip) vs the
brute-force torch reference on the same device vs one ``Predictor`` call, and
what the refinement does to a known motion.

    python scripts/icp_bench.py [--min_seconds 1.0] [--no_predictor] [--no_reference]

Seeded synthetic clouds, no external files, B = 1, the ops' defaults (1.0 m,
0.1 m, 10 rounds):

  lidar    radius 2 + 33 u^2, uniform angle, height N(0, 0.6); the support is
           one draw of M points, the queries another draw of Nq points
  patches  60 planar 4 m x 4 m patches in a 40 x 6 x 40 m volume: src = 8192
           samples, dst = 32768 OTHER samples moved by a known motion (rotvec
           (0.01, 0.03, -0.005), t = (0.1, -0.05, 1.0)); the start is that
           motion perturbed by rotvec (0.002, -0.001, 0.0015) and (0.05, -0.03,
           0.04) m

The HIP paths and the Predictor are warmed up, then timed with device events in
alternating blocks until each has accumulated --min_seconds of timed work; the
spread is the min / max over the blocks.  The reference sweeps all pairs, so it
gets one warm-up call (which is also the comparison) and as many timed calls as
fit in --min_seconds, at least one.  Prints one JSON line per size:

  nn_ms / icp_ms      HIP path, whole nearest_in_radius / icp_refine call
  *_ref_ms            torch reference on the device, whole call
  *_ref_over_op       their ratio
  chamfer_ms          ops.chamfer_nn, the brute-force LDS sweep (Nq = M = 131072 only)
  predictor_ms        one Predictor call (8192 points, 32 iterations, hipGraph)
  nn_share / icp_share   op / predictor_ms
  same                idx and d2 bit-equal to the reference
  matched             share of the queries with a match
and one line "accuracy" with the rotation (degrees) and translation (m) error
against the known motion before and after ``icp_refine`` on the patches pair.
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

SIZES = [(8192, 8192, True), (8192, 32768, True), (8192, 131072, True), (131072, 131072, False)]  # Nq, M, icp too
POINTS = 8192
RADIUS, THRESH, ITERS = 1.0, 0.1, 10
TRUE_ROTVEC, TRUE_T = (0.01, 0.03, -0.005), (0.1, -0.05, 1.0)
PERTURB_ROTVEC, PERTURB_T = (0.002, -0.001, 0.0015), (0.05, -0.03, 0.04)


def lidar(N, seed):
    rng = np.random.default_rng(seed)
    r = 2.0 + 33.0 * rng.random(N) ** 2
    a = rng.uniform(0.0, 2.0 * np.pi, N)
    y = rng.normal(0.0, 0.6, N)
    return np.stack([r * np.cos(a), y, r * np.sin(a)], -1).astype(np.float32)


def rotvec_matrix(v):
    v = np.asarray(v, dtype=np.float64)
    th = np.linalg.norm(v)
    k = v / th
    K = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
    return np.eye(3) + np.sin(th) * K + (1 - np.cos(th)) * (K @ K)


def patch_pair(n_src, n_dst, seed, n_patches=60):
    rng = np.random.default_rng(seed)
    lo, hi = np.array([-20.0, -2.0, -20.0]), np.array([20.0, 4.0, 20.0])
    centre = rng.uniform(lo + 2.0, hi - 2.0, size=(n_patches, 3))
    normal = rng.normal(size=(n_patches, 3))
    normal /= np.linalg.norm(normal, axis=1, keepdims=True)
    u = np.cross(normal, rng.normal(size=(n_patches, 3)))
    u /= np.linalg.norm(u, axis=1, keepdims=True)
    v = np.cross(normal, u)

    def sample(n):
        pid = rng.integers(0, n_patches, n)
        a, b = rng.uniform(-2.0, 2.0, (2, n))
        return centre[pid] + a[:, None] * u[pid] + b[:, None] * v[pid]

    R, t = rotvec_matrix(TRUE_ROTVEC), np.array(TRUE_T)
    return sample(n_src).astype(np.float32), (sample(n_dst) @ R.T + t).astype(np.float32), R, t


def rot_err_deg(Ra, Rb):
    rel = np.asarray(Ra, dtype=np.float64) @ np.asarray(Rb, dtype=np.float64).T
    ax = 0.5 * np.array([rel[2, 1] - rel[1, 2], rel[0, 2] - rel[2, 0], rel[1, 0] - rel[0, 1]])
    return float(np.degrees(np.arctan2(np.linalg.norm(ax), (np.trace(rel) - 1) / 2)))


def timed_block(fn, reps):
    start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(reps):
        fn()
    end.record()
    end.synchronize()
    return start.elapsed_time(end) * 1e-3


def alternate(fns, min_seconds, block_seconds):
    """ms per call, min / max over the blocks and the number of calls, per name."""
    est = {}
    for name, fn in fns.items():
        timed_block(fn, 3)  # warm-up
        est[name] = timed_block(fn, 3) / 3
    reps = {n: max(1, int(block_seconds / est[n])) for n in est}
    tot = {n: 0.0 for n in fns}
    cnt = {n: 0 for n in fns}
    lo = {n: float("inf") for n in fns}
    hi = {n: 0.0 for n in fns}
    while min(tot.values()) < min_seconds:
        for name, fn in fns.items():
            t = timed_block(fn, reps[name])
            tot[name] += t
            cnt[name] += reps[name]
            lo[name] = min(lo[name], t / reps[name])
            hi[name] = max(hi[name], t / reps[name])
    return {n: (tot[n] / cnt[n] * 1e3, lo[n] * 1e3, hi[n] * 1e3, cnt[n]) for n in fns}


def time_reference(fn, min_seconds):
    rt, rc = 0.0, 0
    while rc == 0 or rt < min_seconds:
        rt += timed_block(fn, 1)
        rc += 1
    return rt / rc * 1e3, rc


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--min_seconds", type=float, default=1.0)
    ap.add_argument("--block_seconds", type=float, default=0.05)
    ap.add_argument("--no_predictor", action="store_true")
    ap.add_argument("--no_reference", action="store_true")
    a = ap.parse_args()

    assert torch.cuda.is_available(), "icp_bench needs a GPU"
    assert ops.hip_available(), "HIP extension is not built"
    dev = torch.device("cuda:0")
    inv, r2 = reference.radius_params("icp_bench", RADIUS)
    _, th2 = reference.radius_params("icp_bench", THRESH)
    R_true, t_true = rotvec_matrix(TRUE_ROTVEC), np.array(TRUE_T)
    R0 = torch.from_numpy(rotvec_matrix(PERTURB_ROTVEC) @ R_true).float().unsqueeze(0).to(dev)
    t0 = torch.from_numpy(t_true + np.array(PERTURB_T)).float().unsqueeze(0).to(dev)

    pred = None
    if not a.no_predictor:
        from pvraft_amd.engine import Predictor
        from pvraft_amd.model import PVRaft

        torch.manual_seed(0)
        pred = Predictor(PVRaft().to(dev).eval(), points=POINTS, batch=1, iters=32)
        p1 = torch.from_numpy(lidar(POINTS, seed=1)).unsqueeze(0).to(dev)
        p2 = p1 + torch.tensor([0.05, 0.0, 0.3], device=dev)

    for Nq, M, with_icp in SIZES:
        q = torch.from_numpy(lidar(Nq, seed=Nq + 1)).unsqueeze(0).to(dev)
        s = torch.from_numpy(lidar(M, seed=M)).unsqueeze(0).to(dev)
        # the ICP target: the support moved by the known motion, so that the start is near it
        d = s @ torch.from_numpy(R_true).float().to(dev).T + torch.from_numpy(t_true).float().to(dev)
        fns = {"nn": lambda: ops.nearest_in_radius(q, s, RADIUS)}
        if with_icp:
            fns["icp"] = lambda: ops.icp_refine(q, d, R0=R0, t0=t0, max_dist=RADIUS, thresh=THRESH, iters=ITERS)
        else:
            fns["chamfer"] = lambda: ops.chamfer_nn(q, s)
        if pred is not None:
            fns["pred"] = lambda: pred(p1, p2)
        got = fns["nn"]()
        res = alternate(fns, a.min_seconds, a.block_seconds)
        line = {
            "shape": {"B": 1, "Nq": Nq, "M": M, "radius": RADIUS, "thresh": THRESH, "iters": ITERS},
            "nn_ms": round(res["nn"][0], 4), "nn_ms_min": round(res["nn"][1], 4), "nn_ms_max": round(res["nn"][2], 4),
            "nn_calls": res["nn"][3], "ok": bool(got.ok[0]),
            "matched": round((got.idx >= 0).float().mean().item(), 4),
        }
        if with_icp:
            icp = fns["icp"]()
            line.update(icp_ms=round(res["icp"][0], 4), icp_ms_min=round(res["icp"][1], 4),
                        icp_ms_max=round(res["icp"][2], 4), icp_calls=res["icp"][3],
                        icp_rounds=int(icp.rounds[0]), icp_ok=bool(icp.ok[0]),
                        icp_matched=round(int(icp.matched[0]) / Nq, 4))
        else:
            line.update(chamfer_ms=round(res["chamfer"][0], 4), chamfer_calls=res["chamfer"][3],
                        chamfer_over_nn=round(res["chamfer"][0] / res["nn"][0], 1))
        if not a.no_reference:
            ref_fn = lambda: reference.nearest_in_radius(q, s, inv, r2)
            want = ref_fn()  # warm-up, and the comparison
            torch.cuda.synchronize()
            line["same"] = bool(torch.equal(got.idx, want[0]) and torch.equal(got.d2, want[1]))
            ms, calls = time_reference(ref_fn, a.min_seconds)
            line.update(nn_ref_ms=round(ms, 3), nn_ref_calls=calls, nn_ref_over_op=round(ms / res["nn"][0], 1))
            if with_icp:
                ref_fn = lambda: reference.icp_refine(q, d, inv, r2, th2, ITERS, None, None, R0, t0)
                want = ref_fn()
                torch.cuda.synchronize()
                line["icp_same_idx"] = bool(torch.equal(icp.idx, want[2]))
                ms, calls = time_reference(ref_fn, a.min_seconds)
                line.update(icp_ref_ms=round(ms, 3), icp_ref_calls=calls,
                            icp_ref_over_op=round(ms / res["icp"][0], 1))
        if pred is not None:
            line["predictor_ms"] = round(res["pred"][0], 3)
            line["nn_share"] = round(res["nn"][0] / res["pred"][0], 5)
            if with_icp:
                line["icp_share"] = round(res["icp"][0] / res["pred"][0], 5)
        print(json.dumps(line), flush=True)

    src, dst, R, t = patch_pair(8192, 32768, seed=3)
    src, dst = torch.from_numpy(src).unsqueeze(0).to(dev), torch.from_numpy(dst).unsqueeze(0).to(dev)
    icp = ops.icp_refine(src, dst, R0=R0, t0=t0, max_dist=RADIUS, thresh=THRESH, iters=ITERS)
    line = {
        "accuracy": "patches", "shape": {"B": 1, "N": 8192, "M": 32768},
        "rot_err_deg_before": round(rot_err_deg(R0[0].cpu().numpy(), R), 5),
        "rot_err_deg_after": round(rot_err_deg(icp.R[0].cpu().numpy(), R), 5),
        "trans_err_before": round(float(np.linalg.norm(t0[0].cpu().numpy() - t)), 5),
        "trans_err_after": round(float(np.linalg.norm(icp.t[0].cpu().double().numpy() - t)), 5),
        "matched": round(int(icp.matched[0]) / 8192, 4), "rounds": int(icp.rounds[0]), "ok": bool(icp.ok[0]),
        "rmse": round(float(icp.d2[icp.idx >= 0].double().mean().sqrt()), 5),
    }
    print(json.dumps(line), flush=True)


if __name__ == "__main__":
    main()
