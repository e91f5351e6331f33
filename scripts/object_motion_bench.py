"""Moving-object segmentation benchmark: the HIP clustering and segmented
rigid fit vs the pure-PyTorch reference on the same device, vs the batched
``ops.rigid_fit`` call that did the per-object fits before there was a
segmented fit, next to one Predictor call for scale.

    python scripts/object_motion_bench.py [--min_seconds 1.0]

Seeded synthetic driving-like scenes, no external files: N = 8192 points at
B = 1 and 2, about 30 % of them dynamic in 10 rigid lattice boxes of 240
points plus 60 isolated clutter points, the rest static under one ego-motion;
bounded noise on every flow.  Every path is warmed up, then timed with device
events in alternating blocks until each has accumulated --min_seconds of
timed work (the protocol of ego_motion_bench.py).  Prints one JSON line per
batch size:

  cluster_ms            ops.cluster_points (five launches)
  segfit_ms             ops.segmented_rigid_fit, M = 32 segments, one launch
  object_motion_ms      ops.object_motion: ego fit + clustering + fits + flow
  ref_cluster_ms        reference.cluster_points on the device
  ref_segfit_ms         reference.segmented_rigid_fit on the device
  ref_object_motion_ms  ops.object_motion under PVRAFT_REF_OPS=1
  batched_fit_ms        one ops.rigid_fit call on (B*M, N) inputs with the
                        membership of object m as weights of row m, inputs
                        built beforehand
  batched_fit_setup_ms  the same including building the (B*M, N) inputs
  predictor_ms          one Predictor call, 8192 points, --iters iterations
"""

import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np
import torch

import pvraft_amd.ops as ops
from pvraft_amd.engine import Predictor
from pvraft_amd.model import PVRaft
from pvraft_amd.ops import reference

N = 8192
BOX = (6, 5, 8)
N_BOXES = 10
N_CLUTTER = 60
SPACING = 0.2
MAX_OBJECTS = 32
FIT_ITERS = 5


def rotation(v):
    v = np.asarray(v, dtype=np.float64)
    th = np.linalg.norm(v)
    K = np.array([[0, -v[2], v[1]], [v[2], 0, -v[0]], [-v[1], v[0], 0]])
    return np.eye(3) + np.sin(th) / th * K + (1 - np.cos(th)) / th**2 * (K @ K)


def scene(B, seed):
    """Static points of a 30 x 4 x 30 m box follow one small rigid motion;
    ten lattice boxes on a 5 x 2 grid move with extra translations of 0.6 m
    and more; clutter points move alone.  Uniform noise of +-5 mm per
    component on every flow."""
    rng = np.random.default_rng(seed)
    R, t = rotation([0.01, 0.03, -0.005]), np.array([0.1, -0.05, 1.0])
    g = np.stack(np.meshgrid(*[np.arange(d) for d in BOX], indexing="ij"), -1).reshape(-1, 3) * SPACING
    pcs, flows = [], []
    for _ in range(B):
        pts, extra = [], []
        for k in range(N_BOXES):
            pts.append(np.array([-12.0 + 6.0 * (k % 5), -1.5, 10.0 + 12.0 * (k // 5)]) + g)
            shift = np.array([0.6 + 0.3 * (k % 5), 0.0, -0.9 + 0.45 * (k // 5) * (k % 3)])
            extra.append(np.tile(shift, (len(g), 1)))
        n_dyn = N_BOXES * len(g) + N_CLUTTER
        pts.append(np.stack([rng.uniform(-14, 14, N_CLUTTER), np.full(N_CLUTTER, 1.8),
                             rng.uniform(6, 34, N_CLUTTER)], -1))
        extra.append(rng.uniform(0.5, 1.5, (N_CLUTTER, 3)))
        pts.append((rng.random((N - n_dyn, 3)) - 0.5) * np.array([30.0, 4.0, 30.0]) + np.array([0.0, 0.0, 20.0]))
        extra.append(np.zeros((N - n_dyn, 3)))
        pts, extra = np.concatenate(pts), np.concatenate(extra)
        flow = pts @ R.T + t - pts + extra + (rng.random(pts.shape) - 0.5) * 0.01
        perm = rng.permutation(N)
        pcs.append(pts[perm])
        flows.append(flow[perm])
    return torch.from_numpy(np.stack(pcs)).float(), torch.from_numpy(np.stack(flows)).float()


def timed_block(fn, reps):
    start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(reps):
        fn()
    end.record()
    end.synchronize()
    return start.elapsed_time(end) * 1e-3


def with_reference_ops(fn):
    def run():
        os.environ["PVRAFT_REF_OPS"] = "1"
        try:
            return fn()
        finally:
            del os.environ["PVRAFT_REF_OPS"]
    return run


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--min_seconds", type=float, default=1.0)
    ap.add_argument("--block_seconds", type=float, default=0.05)
    ap.add_argument("--iters", type=int, default=32, help="GRU iterations of the Predictor call")
    ap.add_argument("--truncate_k", type=int, default=512)
    ap.add_argument("--predictor_reps", type=int, default=10)
    a = ap.parse_args()

    assert torch.cuda.is_available(), "object_motion_bench needs a GPU"
    assert ops.hip_available(), "HIP extension is not built"
    dev = torch.device("cuda:0")

    for B in (1, 2):
        pc_c, flow_c = scene(B, seed=100 + B)
        pc, flow = pc_c.to(dev), flow_c.to(dev)
        dst = pc + flow
        ego = ops.ego_motion(pc, flow)
        mask = ~ego.static
        labels, count, nobj = ops.cluster_points(pc, flow, mask, max_objects=MAX_OBJECTS)
        M = MAX_OBJECTS

        def batched_inputs():
            src_r = pc.unsqueeze(1).expand(B, M, N, 3).reshape(B * M, N, 3)
            dst_r = dst.unsqueeze(1).expand(B, M, N, 3).reshape(B * M, N, 3)
            w = (labels.unsqueeze(1) == torch.arange(M, device=dev, dtype=labels.dtype).view(1, M, 1)).float()
            return src_r, dst_r, w.reshape(B * M, N)

        src_r, dst_r, w_r = batched_inputs()
        fns = {
            "cluster": lambda: ops.cluster_points(pc, flow, mask, max_objects=M),
            "segfit": lambda: ops.segmented_rigid_fit(pc, dst, labels, M, None, 0.05, FIT_ITERS),
            "object_motion": lambda: ops.object_motion(pc, flow, max_objects=M, iters=FIT_ITERS),
            "ref_cluster": lambda: reference.cluster_points(pc, flow, mask, 0.5, 0.1, 8, M),
            "ref_segfit": lambda: reference.segmented_rigid_fit(pc, dst, labels, M, None, 0.05, FIT_ITERS),
            "ref_object_motion": with_reference_ops(
                lambda: ops.object_motion(pc, flow, max_objects=M, iters=FIT_ITERS)),
            "batched_fit": lambda: ops.rigid_fit(src_r, dst_r, w_r, 0.05, FIT_ITERS),
            "batched_fit_setup": lambda: ops.rigid_fit(*batched_inputs(), 0.05, FIT_ITERS),
        }

        # same answers on the timed inputs before any timing
        ref_labels = fns["ref_cluster"]()[0]
        seg = fns["segfit"]()
        old = fns["batched_fit"]()
        found = int(nobj.max().item())
        fit_dev = max(
            (seg[0][:, :found] - old[0].view(B, M, 3, 3)[:, :found]).abs().max().item(),
            (seg[1][:, :found] - old[1].view(B, M, 3)[:, :found]).abs().max().item(),
        )

        est = {}
        for name, fn in fns.items():
            timed_block(fn, 2)  # warm-up
            est[name] = timed_block(fn, 2) / 2
        reps = {n: max(1, int(a.block_seconds / est[n])) for n in est}
        tot = {n: 0.0 for n in fns}
        cnt = {n: 0 for n in fns}
        while min(tot.values()) < a.min_seconds:
            for name, fn in fns.items():
                if tot[name] < a.min_seconds:
                    tot[name] += timed_block(fn, reps[name])
                    cnt[name] += reps[name]
        ms = {n: tot[n] / cnt[n] * 1e3 for n in fns}

        torch.manual_seed(0)
        model = PVRaft(truncate_k=a.truncate_k).to(dev).eval()
        pred = Predictor(model, points=N, batch=B, iters=a.iters)
        xyz2 = pc + flow
        for _ in range(3):
            pred(pc, xyz2)
        torch.cuda.synchronize()
        calls = sorted(timed_block(lambda: pred(pc, xyz2), 1) for _ in range(a.predictor_reps))
        pred_ms = calls[len(calls) // 2] * 1e3
        del pred, model

        line = {"shape": {"B": B, "N": N, "max_objects": M, "fit_iters": FIT_ITERS},
                "dynamic_ratio": round(mask.float().mean().item(), 4),
                "objects_found": nobj.cpu().tolist(),
                "largest_object": int(count.max().item()),
                "labels_equal_reference": bool(torch.equal(labels, ref_labels)),
                "segfit_vs_batched_max_abs_dev": fit_dev}
        line.update({f"{n}_ms": round(v, 4) for n, v in ms.items()})
        line.update({f"{n}_calls": cnt[n] for n in fns})
        line.update({
            "batched_over_segfit": round(ms["batched_fit"] / ms["segfit"], 2),
            "ref_over_op_object_motion": round(ms["ref_object_motion"] / ms["object_motion"], 2),
            "predictor_ms": round(pred_ms, 3),
            "predictor_iters": a.iters,
            "object_motion_share": round(ms["object_motion"] / (ms["object_motion"] + pred_ms), 5),
        })
        print(json.dumps(line), flush=True)


if __name__ == "__main__":
    main()
