#!/usr/bin/env python3
"""Evaluation CLI (same flag surface as reference test.py:20-67).

python test.py --dataset=FT3D --weights=experiments/pvraft/checkpoints/best_checkpoint.params ...
Runs 32 GRU iterations per pair (reference test.py:120) and prints mean
EPE3D / Acc3DS / Acc3DR / Outlier.
"""

import argparse
import os

from pvraft_amd.cli import add_common_args
from pvraft_amd.engine.evaluator import evaluate


def parse_args():
    parser = argparse.ArgumentParser(description="Testing Argument")
    add_common_args(parser, training=False)
    parser.add_argument("--gamma", help="exponential weights", default=0.8, type=float)
    parser.add_argument("--dump_results", help="write result/<dataset>/<i>/{pc1,pc2,flow}.npy for visual.py", action="store_true")
    parser.add_argument("--dense", help="also interpolate the flow onto the full-resolution pc1 and report dense_* metrics", action="store_true")
    parser.add_argument("--dense_k", help="neighbours for the dense interpolation", default=3, type=int)
    parser.add_argument("--ego_motion", help="also fit the ego-motion of the predicted flow and report ego_* / rigid_* metrics", action="store_true")
    parser.add_argument("--ego_thresh", help="static/dynamic residual threshold of the ego-motion fit (m)", default=0.05, type=float)
    parser.add_argument("--ego_iters", help="reweighting rounds of the ego-motion fit", default=10, type=int)
    parser.add_argument("--object_motion", help="also segment the moving objects of the predicted flow (implies the ego-motion fit) and report obj_* / objrigid_* metrics", action="store_true")
    parser.add_argument("--obj_eps", help="spatial link radius of the object clustering (m)", default=0.5, type=float)
    parser.add_argument("--obj_flow_eps", help="flow link radius of the object clustering (m)", default=0.1, type=float)
    parser.add_argument("--obj_min_points", help="smallest object, in points", default=8, type=int)
    parser.add_argument("--obj_max_objects", help="objects kept per sample, largest first", default=32, type=int)
    parser.add_argument("--obj_iters", help="reweighting rounds of the per-object fits", default=5, type=int)
    parser.add_argument("--ground_fit", help="also fit the ground plane of every pc1 and report ground_* / ng_* metrics", action="store_true")
    parser.add_argument("--ground_thresh", help="point-to-plane distance of a ground point (m)", default=0.2, type=float)
    parser.add_argument("--ground_hyp", help="plane hypotheses of the ground fit", default=256, type=int)
    parser.add_argument("--ground_tilt", help="largest angle between the ground normal and +y (degrees)", default=20.0, type=float)
    parser.add_argument("--ground_iters", help="refinement rounds of the ground fit", default=3, type=int)
    parser.add_argument("--keep_ground", help="KITTI: keep the y < -1.4 points the loader removes by default", action="store_true")
    parser.add_argument("--sample", help="how the max_points inputs are drawn: the loader's uniform subsample, or ops.voxel_sample on both full clouds (adds sample_cut_* to the report)", default="random", choices=["random", "voxel"])
    parser.add_argument("--sample_voxel", help="finest cell edge of the voxel sampler (m)", default=0.1, type=float)
    parser.add_argument("--sample_levels", help="nested grid levels of the voxel sampler", default=10, type=int)
    parser.add_argument("--sample_seed", help="seed of the voxel sampler's tie-breaking hash", default=0, type=int)
    parser.add_argument("--noise_filter", help="with --sample voxel: filter both full clouds with ops.noise_filter, keep isolated points out of the sample and report noise_* metrics", action="store_true")
    parser.add_argument("--noise_radius", help="neighbour radius of the noise filter (m)", default=0.5, type=float)
    parser.add_argument("--noise_min_neighbors", help="a point with fewer neighbours within the radius is noise", default=4, type=int)
    parser.add_argument("--noise_k", help="nearest neighbours in the mean-distance statistic of the noise filter (0 disables it)", default=8, type=int)
    parser.add_argument("--noise_std_ratio", help="a point whose mean distance exceeds mean + ratio * std is noise", default=2.0, type=float)
    parser.add_argument("--ego_icp", help="with --ego_motion: refine the fitted motion by ICP of the static points against the full second scan (ops.icp_refine) and report icp_* / icprigid_* metrics", action="store_true")
    parser.add_argument("--icp_max_dist", help="largest correspondence distance of the ICP refinement (m)", default=1.0, type=float)
    parser.add_argument("--icp_thresh", help="Cauchy scale of the ICP weights (m)", default=0.1, type=float)
    parser.add_argument("--icp_iters", help="rounds of the ICP refinement", default=10, type=int)
    return parser.parse_args()


if __name__ == "__main__":
    args = parse_args()
    gpus = [g for g in str(args.gpus).split(",") if g != ""]
    if gpus and "RANK" not in os.environ:
        os.environ.setdefault("HIP_VISIBLE_DEVICES", gpus[0])
    results = evaluate(args)
    print(results)
