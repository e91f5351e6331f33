"""Standalone evaluation (reference test.py:70-156).

Builds the FT3D test split or KITTI, runs the (optionally refined) model
with 32 GRU iterations (test.py:120 hard-codes 32 regardless of --iters)
and reports mean EPE3D / Acc3DS / Acc3DR / Outlier.

On GPU the forward is served by the hipGraph Predictor (fixed shapes); it
exposes every per-iteration flow, so the logged loss is the same
gamma-weighted sequence loss the reference's test.py computes
(test.py:122).  Disable with --no_hipgraph for the eager path.

--dense (absent in the reference, whose evaluation is subset-only) also
interpolates the final flow from the sampled pc1 onto the full-resolution
cloud (ops.knn_interpolate, --dense_k neighbours) and reports dense_*
metrics over every masked point; the sparse path and its metrics are
untouched.

--ego_motion (also beyond the reference) fits the rigid motion that explains
the static part of the predicted flow (ops.ego_motion, --ego_thresh,
--ego_iters) and the same for the ground-truth flow with the ground-truth
mask as prior weights -- the dataset's own ego-motion.  It reports the
rotation / translation error between the two fits, the share of points
classified static, and rigid_* metrics of the flow whose static points are
snapped onto the fitted motion.

--object_motion (beyond the reference too) goes one step further with
ops.object_motion: the points the ego fit leaves over are clustered into
objects (--obj_eps, --obj_flow_eps, --obj_min_points, --obj_max_objects),
every object gets its own rigid fit (--obj_iters) and its points the flow
that fit induces.  It reports the mean number of objects, the share of
points in objects and objrigid_* metrics of the piecewise-rigid flow.  It
uses --ego_thresh / --ego_iters for its ego fit and adds no ego_* keys
unless --ego_motion is given as well.

--ground_fit (beyond the reference as well) fits the ground plane of every
sampled pc1 (ops.fit_plane, --ground_thresh, --ground_hyp, --ground_tilt,
--ground_iters) after the forward, like --ego_motion.  It reports
ground_ratio (share of points within the threshold of the plane),
ground_below_ratio (share further below it), ground_tilt_deg (angle between
the normal and +y), ground_height (height of the origin above the plane) and
ng_* metrics: the usual ones with every ground point (on or below the plane)
masked out through ground_truth[0].  --keep_ground makes the KITTI loader
keep its y < -1.4 points; ground_iou then compares the fitted ground with
that rule on pc1.  SYNTH puts 30 % of its points on a ground plane when the
flag is on.  The sparse path and its metrics are untouched.

--sample voxel (beyond the reference too) replaces the loader's uniform
subsample: both full-resolution clouds travel with the item ("full", "full2"),
max_points indices are drawn from each with ops.voxel_sample on the device
(--sample_voxel, --sample_levels, --sample_seed), mask and ground-truth flow
are taken at pc1's indices, and the usual forward and metrics follow, with
--dense, --ego_motion, --object_motion and --ground_fit on top as before.  It
also reports sample_cut_level, the mean over the samples of l* (the finest
grid level with at most max_points occupied cells in pc1, every cell of which
holds a sample; ``levels`` when there is none), and sample_cut_radius, the mean
of sqrt(3) * voxel * 2**l*.  SYNTH builds its clouds with 4 * max_points
points, as under --dense.  Without the flag nothing changes.

--noise_filter (beyond the reference too) keeps isolated points out of the
voxel sample: both full clouds get ops.noise_filter (--noise_radius,
--noise_min_neighbors, --noise_k, --noise_std_ratio) and its keep mask goes
into ops.voxel_sample as ``mask``.  It needs the full clouds, so it requires
--sample voxel and raises ValueError otherwise.  It reports noise_ratio (share
of pc1's points that are not kept), noise_sparse_ratio (share with fewer than
min_neighbors neighbours), noise_far_ratio (share whose mean distance to the k
nearest is above the threshold, or that have fewer than k neighbours) and
noise_mean_dist (the filter's ``mean`` of pc1), averaged over the set;
--dump_results also writes noise_mask.npy (~keep of the full pc1).  SYNTH
replaces 2 % of its points by uniform noise when the flag is on.

--ego_icp (beyond the reference too) refines the ego-motion fit by point-to-point
ICP: the points the fit calls static are registered against the FULL second
scan (the loader's "full2" cloud, which the network never sees whole) with
ops.icp_refine started from the fitted motion (--icp_max_dist, --icp_thresh,
--icp_iters).  It builds on the ego fit, so it requires --ego_motion and raises
ValueError otherwise.  It reports icp_rot_err_deg and icp_trans_err (the
formulas of the ego_* keys against the same ground-truth fit), icp_match_ratio
(matched share of the static points), icp_rmse (root of the mean matched
squared distance under the refined motion, a residual that needs no ground
truth) and icprigid_* metrics of the flow whose static points are snapped onto
the refined motion; --dump_results also writes icp_R.npy, icp_t.npy, icp_idx.npy
and icp_d2.npy.  Without the flag nothing changes.
"""

from __future__ import annotations

import os

import torch
from torch.utils.data import DataLoader

from pvraft_amd.data import FT3D, Batch, Kitti, SyntheticSceneFlow
from pvraft_amd.model import build_model
from pvraft_amd.utils import (
    compute_epe,
    compute_loss,
    load_checkpoint,
    sequence_loss,
    setup_logger,
)

TEST_ITERS = 32  # reference test.py:120


def build_eval_dataset(args):
    if args.dataset == "FT3D":
        ddir = os.path.join(args.root, "data", "FlyingThings3D_subset_processed_35m")
        return FT3D(ddir, args.max_points, "test")
    if args.dataset == "KITTI":
        ddir = os.path.join(args.root, "data", "kitti_processed")
        ds = Kitti(ddir, args.max_points)
        if getattr(args, "keep_ground", False):
            ds.keep_ground = True
        return ds
    if args.dataset == "SYNTH":
        voxel = getattr(args, "sample", "random") == "voxel"
        full = 4 * args.max_points if getattr(args, "dense", False) or voxel else None
        return SyntheticSceneFlow(args.max_points, length=getattr(args, "synth_len", 32), seed=7,
                                  full_points=full,
                                  ground_fraction=0.3 if getattr(args, "ground_fit", False) else 0.0,
                                  noise_fraction=0.02 if getattr(args, "noise_filter", False) else 0.0)
    raise ValueError(f"Unknown dataset {args.dataset!r}")


@torch.no_grad()
def evaluate(args):
    log = setup_logger(args.root, args.exp_path or "test", f"TestAlone_{args.dataset}")
    device = torch.device("cuda:0") if torch.cuda.is_available() else torch.device("cpu")

    dataset = build_eval_dataset(args)
    dense = bool(getattr(args, "dense", False))
    dense_k = int(getattr(args, "dense_k", 3))
    ego = bool(getattr(args, "ego_motion", False))
    ego_thresh = float(getattr(args, "ego_thresh", 0.05))
    ego_iters = int(getattr(args, "ego_iters", 10))
    obj = bool(getattr(args, "object_motion", False))
    obj_kw = dict(
        eps=float(getattr(args, "obj_eps", 0.5)),
        flow_eps=float(getattr(args, "obj_flow_eps", 0.1)),
        min_points=int(getattr(args, "obj_min_points", 8)),
        max_objects=int(getattr(args, "obj_max_objects", 32)),
        iters=int(getattr(args, "obj_iters", 5)),
    )
    ground = bool(getattr(args, "ground_fit", False))
    ground_kw = dict(
        thresh=float(getattr(args, "ground_thresh", 0.2)),
        hypotheses=int(getattr(args, "ground_hyp", 256)),
        max_tilt_deg=float(getattr(args, "ground_tilt", 20.0)),
        refine_iters=int(getattr(args, "ground_iters", 3)),
    )
    ground_iou = ground and args.dataset == "KITTI" and bool(getattr(args, "keep_ground", False))
    sample = str(getattr(args, "sample", "random"))
    if sample not in ("random", "voxel"):
        raise ValueError(f'--sample must be "random" or "voxel", got {sample!r}')
    voxel = sample == "voxel"
    sample_kw = dict(
        voxel=float(getattr(args, "sample_voxel", 0.1)),
        levels=int(getattr(args, "sample_levels", 10)),
        seed=int(getattr(args, "sample_seed", 0)),
    )
    denoise = bool(getattr(args, "noise_filter", False))
    if denoise and not voxel:
        raise ValueError("--noise_filter filters the full clouds: it requires --sample voxel")
    noise_kw = dict(
        radius=float(getattr(args, "noise_radius", 0.5)),
        min_neighbors=int(getattr(args, "noise_min_neighbors", 4)),
        k=int(getattr(args, "noise_k", 8)),
        std_ratio=float(getattr(args, "noise_std_ratio", 2.0)),
    )
    ego_icp = bool(getattr(args, "ego_icp", False))
    if ego_icp and not ego:
        raise ValueError("--ego_icp refines the ego-motion fit: it requires --ego_motion")
    icp_kw = dict(
        max_dist=float(getattr(args, "icp_max_dist", 1.0)),
        thresh=float(getattr(args, "icp_thresh", 0.1)),
        iters=int(getattr(args, "icp_iters", 10)),
    )
    if dense or ego or obj or ground or voxel:
        from pvraft_amd import ops
    if dense or voxel:
        dataset.return_full = True
    if voxel or ego_icp:
        dataset.return_full2 = True
    loader = DataLoader(
        dataset,
        batch_size=1,
        shuffle=False,
        num_workers=getattr(args, "num_workers", 8),
        collate_fn=Batch,
        pin_memory=device.type == "cuda",
    )

    model = build_model(args).to(device)
    if args.weights:
        path = args.weights
        if not os.path.isfile(path):
            path = os.path.join(args.root, "experiments", args.weights, "checkpoints", "best_checkpoint.params")
        load_checkpoint(path, model, strict=True)
        log.info(f"Loaded weights from {path}")
    model.eval()

    dump = bool(getattr(args, "dump_results", False))
    # hipGraph-captured inference (fixed bs=1 x max_points shapes)
    predictor = None
    if device.type == "cuda" and getattr(args, "hipgraph", True):
        from .predictor import Predictor

        predictor = Predictor(model, points=args.max_points, batch=1, iters=TEST_ITERS,
                              amp=bool(getattr(args, "amp", False)))
    sums = [0.0] * 5
    dense_sums = [0.0] * 4
    ego_sums = [0.0] * 7
    obj_sums = [0.0] * 6
    ground_sums = [0.0] * 9
    sample_sums = [0.0] * 2
    noise_sums = [0.0] * 4
    icp_sums = [0.0] * 8
    n_ng = 0
    n = 0
    for batch in loader:
        batch = batch.to(device, non_blocking=True)
        if voxel:
            # the loader's own subsample is replaced: same shapes, other points.
            # The loader still draws it (one permutation and gather per item,
            # wasted here): skipping it would change the numpy draws that a
            # run without the flag makes, and the datasets stay untouched
            pc1_all, mask_all, flow_all = batch["full"]
            pc2_all = batch["full2"][0]
            keep1 = keep2 = None
            if denoise:
                nf1 = ops.noise_filter(pc1_all, **noise_kw)
                nf2 = ops.noise_filter(pc2_all, **noise_kw)
                keep1, keep2 = nf1.keep, nf2.keep
                el = nf1.count >= 0
                far = el & (nf1.count < noise_kw["k"])
                if noise_kw["k"] >= 1:
                    far = far | (el & (nf1.mean_dist.double() > nf1.threshold.unsqueeze(1)))
                noise_sums[0] += (~keep1).float().mean().item()
                noise_sums[1] += (el & (nf1.count < noise_kw["min_neighbors"])).float().mean().item()
                noise_sums[2] += far.float().mean().item()
                noise_sums[3] += nf1.mean.mean().item()
            vs1 = ops.voxel_sample(pc1_all, args.max_points, mask=keep1, **sample_kw)
            vs2 = ops.voxel_sample(pc2_all, args.max_points, mask=keep2, **sample_kw)
            for name, vs in (("pc1", vs1), ("pc2", vs2)):
                if int(vs.count[0]) < args.max_points:
                    raise ValueError(
                        f"sample {n}: {name} has {int(vs.count[0])} points the voxel sampler can use, "
                        f"fewer than max_points = {args.max_points}"
                    )
            sample_idx1, sample_idx2 = vs1.idx[0], vs2.idx[0]
            batch.data["sequence"] = [pc1_all[:, sample_idx1], pc2_all[:, sample_idx2]]
            batch.data["ground_truth"] = [mask_all[:, sample_idx1], flow_all[:, sample_idx1]]
            covered = (vs1.occupied[0] <= args.max_points).nonzero()
            cut = int(covered[0]) if covered.numel() else sample_kw["levels"]
            sample_sums[0] += cut
            sample_sums[1] += 3.0 ** 0.5 * sample_kw["voxel"] * 2.0 ** cut
        if predictor is not None and batch["sequence"][0].shape[1] == args.max_points:
            final = predictor(batch["sequence"][0], batch["sequence"][1])
            flows = predictor.last_flows
            # reference test.py:122 logs the gamma-weighted sequence loss
            # for the stage-1 model (single refined flow -> plain loss)
            if len(flows) > 1:
                loss = sequence_loss(flows, batch, gamma=args.gamma if hasattr(args, "gamma") else 0.8)
            else:
                loss = compute_loss(final, batch)
        else:
            est_flow = model(batch["sequence"], num_iters=TEST_ITERS)
            if isinstance(est_flow, (list, tuple)):
                loss = sequence_loss(est_flow, batch, gamma=args.gamma if hasattr(args, "gamma") else 0.8)
                final = est_flow[-1]
            else:
                loss = compute_loss(est_flow, batch)
                final = est_flow
        epe3d, accs, accr, outl = compute_epe(final.float(), batch)
        for j, v in enumerate((loss.item(), epe3d, accs, accr, outl)):
            sums[j] += v
        if dense:
            pc1_full, mask_full, flow_full = batch["full"]
            flow_dense, _, _ = ops.knn_interpolate(
                batch["sequence"][0], final.float(), pc1_full, dense_k
            )
            dense_m = compute_epe(flow_dense, {"ground_truth": [mask_full, flow_full]})
            for j, v in enumerate(dense_m):
                dense_sums[j] += v
        if ego:
            pc1 = batch["sequence"][0].float()
            gt_mask, gt_flow = batch["ground_truth"]
            fit = ops.ego_motion(pc1, final.float(), thresh=ego_thresh, iters=ego_iters)
            gt_fit = ops.ego_motion(pc1, gt_flow.float(), thresh=ego_thresh, iters=ego_iters,
                                    weights=gt_mask[..., 0].float())
            rel = fit.R @ gt_fit.R.transpose(1, 2)
            cos = ((rel.diagonal(dim1=1, dim2=2).sum(-1) - 1) / 2).clamp(-1, 1)
            rot_err = torch.rad2deg(torch.acos(cos)).mean().item()
            trans_err = (fit.t - gt_fit.t).norm(dim=-1).mean().item()
            flow_rigid = torch.where(fit.static.unsqueeze(-1), fit.rigid_flow, final.float())
            rigid_m = compute_epe(flow_rigid, batch)
            for j, v in enumerate((rot_err, trans_err, fit.static.float().mean().item()) + tuple(rigid_m)):
                ego_sums[j] += v
            if ego_icp:
                icp = ops.icp_refine(pc1, batch["full2"][0].float(), R0=fit.R, t0=fit.t, src_mask=fit.static,
                                     **icp_kw)
                rel = icp.R @ gt_fit.R.transpose(1, 2)
                cos = ((rel.diagonal(dim1=1, dim2=2).sum(-1) - 1) / 2).clamp(-1, 1)
                icp_rot_err = torch.rad2deg(torch.acos(cos)).mean().item()
                icp_trans_err = (icp.t - gt_fit.t).norm(dim=-1).mean().item()
                found = icp.idx >= 0
                n_static = fit.static.sum().item()
                n_found = found.sum().item()
                match_ratio = n_found / n_static if n_static else 0.0
                rmse = (icp.d2[found].double().mean().sqrt().item()) if n_found else 0.0
                icp_flow = pc1 @ icp.R.transpose(1, 2) + icp.t.unsqueeze(1) - pc1
                flow_icprigid = torch.where(fit.static.unsqueeze(-1), icp_flow, final.float())
                icprigid_m = compute_epe(flow_icprigid, batch)
                for j, v in enumerate((icp_rot_err, icp_trans_err, match_ratio, rmse) + tuple(icprigid_m)):
                    icp_sums[j] += v
        if obj:
            pc1 = batch["sequence"][0].float()
            om = ops.object_motion(pc1, final.float(), ego=fit if ego else None, ego_thresh=ego_thresh,
                                   ego_iters=ego_iters, **obj_kw)
            objrigid_m = compute_epe(om.rigid_flow, batch)
            head = (om.num_objects.float().mean().item(), (om.labels >= 0).float().mean().item())
            for j, v in enumerate(head + tuple(objrigid_m)):
                obj_sums[j] += v
        if ground:
            pc1 = batch["sequence"][0].float()
            gfit = ops.fit_plane(pc1, **ground_kw)
            gt_mask, gt_flow = batch["ground_truth"]
            up = torch.tensor([0.0, 1.0, 0.0], device=pc1.device)
            tilt = torch.rad2deg(torch.atan2(torch.linalg.cross(gfit.normal, up.expand_as(gfit.normal)).norm(dim=-1),
                                             gfit.normal @ up)).mean().item()
            iou = 0.0
            if ground_iou:
                from pvraft_amd.data.kitti import GROUND_Y

                rule = pc1[..., 1] < GROUND_Y
                union = (rule | gfit.ground).sum().item()
                iou = (rule & gfit.ground).sum().item() / union if union else 1.0
            head = (gfit.inlier.float().mean().item(), (gfit.ground & ~gfit.inlier).float().mean().item(), tilt,
                    gfit.offset.mean().item(), iou)
            ng_mask = gt_mask * (~gfit.ground).unsqueeze(-1).to(gt_mask.dtype)
            ng_m = (0.0,) * 4
            if ng_mask.sum().item() > 0:  # a sample that is all ground adds nothing to ng_*
                ng_m = compute_epe(final.float(), {"ground_truth": [ng_mask, gt_flow]})
                n_ng += 1
            for j, v in enumerate(head + tuple(ng_m)):
                ground_sums[j] += v
        if dump:
            import numpy as np

            d = os.path.join(args.root, "result", args.dataset, str(n))
            os.makedirs(d, exist_ok=True)
            np.save(os.path.join(d, "pc1.npy"), batch["sequence"][0].cpu().numpy())
            np.save(os.path.join(d, "pc2.npy"), batch["sequence"][1].cpu().numpy())
            np.save(os.path.join(d, "flow.npy"), final.cpu().numpy())
            if voxel:
                np.save(os.path.join(d, "sample_idx1.npy"), sample_idx1.cpu().numpy())
            if denoise:
                np.save(os.path.join(d, "noise_mask.npy"), (~keep1[0]).cpu().numpy())
            if dense:
                np.save(os.path.join(d, "pc1_full.npy"), pc1_full.cpu().numpy())
                np.save(os.path.join(d, "flow_dense.npy"), flow_dense.cpu().numpy())
            if ego:
                np.save(os.path.join(d, "ego_R.npy"), fit.R.cpu().numpy())
                np.save(os.path.join(d, "ego_t.npy"), fit.t.cpu().numpy())
                np.save(os.path.join(d, "static_mask.npy"), fit.static.cpu().numpy())
                np.save(os.path.join(d, "flow_rigid.npy"), flow_rigid.cpu().numpy())
            if ego_icp:
                np.save(os.path.join(d, "icp_R.npy"), icp.R.cpu().numpy())
                np.save(os.path.join(d, "icp_t.npy"), icp.t.cpu().numpy())
                np.save(os.path.join(d, "icp_idx.npy"), icp.idx.cpu().numpy())
                np.save(os.path.join(d, "icp_d2.npy"), icp.d2.cpu().numpy())
            if obj:
                np.save(os.path.join(d, "object_labels.npy"), om.labels.cpu().numpy())
                np.save(os.path.join(d, "obj_R.npy"), om.R.cpu().numpy())
                np.save(os.path.join(d, "obj_t.npy"), om.t.cpu().numpy())
                np.save(os.path.join(d, "flow_objrigid.npy"), om.rigid_flow.cpu().numpy())
            if ground:
                np.save(os.path.join(d, "ground_mask.npy"), gfit.ground.cpu().numpy())
                np.save(os.path.join(d, "ground_plane.npy"),
                        torch.cat([gfit.normal, gfit.offset.unsqueeze(-1)], -1).cpu().numpy())
        n += 1
    means = [s / max(n, 1) for s in sums]
    log.info(
        f"[test {args.dataset}] loss={means[0]:.4f} EPE3D={means[1]:.4f} "
        f"Acc3DS={means[2]:.4f} Acc3DR={means[3]:.4f} Outlier={means[4]:.4f}"
    )
    results = {
        "loss": means[0],
        "epe": means[1],
        "acc3d_strict": means[2],
        "acc3d_relax": means[3],
        "outlier": means[4],
    }
    if dense:
        dmeans = [s / max(n, 1) for s in dense_sums]
        log.info(
            f"[test {args.dataset} dense k={dense_k}] EPE3D={dmeans[0]:.4f} "
            f"Acc3DS={dmeans[1]:.4f} Acc3DR={dmeans[2]:.4f} Outlier={dmeans[3]:.4f}"
        )
        results.update(
            dense_epe=dmeans[0],
            dense_acc3d_strict=dmeans[1],
            dense_acc3d_relax=dmeans[2],
            dense_outlier=dmeans[3],
        )
    if ego:
        emeans = [s / max(n, 1) for s in ego_sums]
        log.info(
            f"[test {args.dataset} ego thresh={ego_thresh} iters={ego_iters}] "
            f"rot_err={emeans[0]:.4f}deg trans_err={emeans[1]:.4f} static={emeans[2]:.4f} "
            f"rigid EPE3D={emeans[3]:.4f} Acc3DS={emeans[4]:.4f} Acc3DR={emeans[5]:.4f} "
            f"Outlier={emeans[6]:.4f}"
        )
        results.update(
            ego_rot_err_deg=emeans[0],
            ego_trans_err=emeans[1],
            ego_static_ratio=emeans[2],
            rigid_epe=emeans[3],
            rigid_acc3d_strict=emeans[4],
            rigid_acc3d_relax=emeans[5],
            rigid_outlier=emeans[6],
        )
    if ego_icp:
        imeans = [s / max(n, 1) for s in icp_sums]
        log.info(
            f"[test {args.dataset} icp max_dist={icp_kw['max_dist']} thresh={icp_kw['thresh']} "
            f"iters={icp_kw['iters']}] rot_err={imeans[0]:.4f}deg trans_err={imeans[1]:.4f} "
            f"match={imeans[2]:.4f} rmse={imeans[3]:.4f} "
            f"icprigid EPE3D={imeans[4]:.4f} Acc3DS={imeans[5]:.4f} Acc3DR={imeans[6]:.4f} "
            f"Outlier={imeans[7]:.4f}"
        )
        results.update(
            icp_rot_err_deg=imeans[0],
            icp_trans_err=imeans[1],
            icp_match_ratio=imeans[2],
            icp_rmse=imeans[3],
            icprigid_epe=imeans[4],
            icprigid_acc3d_strict=imeans[5],
            icprigid_acc3d_relax=imeans[6],
            icprigid_outlier=imeans[7],
        )
    if obj:
        omeans = [s / max(n, 1) for s in obj_sums]
        log.info(
            f"[test {args.dataset} objects eps={obj_kw['eps']} flow_eps={obj_kw['flow_eps']} "
            f"min_points={obj_kw['min_points']} iters={obj_kw['iters']}] "
            f"count={omeans[0]:.2f} point_ratio={omeans[1]:.4f} "
            f"objrigid EPE3D={omeans[2]:.4f} Acc3DS={omeans[3]:.4f} Acc3DR={omeans[4]:.4f} "
            f"Outlier={omeans[5]:.4f}"
        )
        results.update(
            obj_count=omeans[0],
            obj_point_ratio=omeans[1],
            objrigid_epe=omeans[2],
            objrigid_acc3d_strict=omeans[3],
            objrigid_acc3d_relax=omeans[4],
            objrigid_outlier=omeans[5],
        )
    if ground:
        gmeans = [v / max(n, 1) for v in ground_sums[:5]] + [v / max(n_ng, 1) for v in ground_sums[5:]]
        log.info(
            f"[test {args.dataset} ground thresh={ground_kw['thresh']} hyp={ground_kw['hypotheses']} "
            f"tilt={ground_kw['max_tilt_deg']} iters={ground_kw['refine_iters']}] "
            f"ratio={gmeans[0]:.4f} below={gmeans[1]:.4f} tilt={gmeans[2]:.3f}deg height={gmeans[3]:.3f} "
            f"ng EPE3D={gmeans[5]:.4f} Acc3DS={gmeans[6]:.4f} Acc3DR={gmeans[7]:.4f} Outlier={gmeans[8]:.4f}"
        )
        results.update(
            ground_ratio=gmeans[0],
            ground_below_ratio=gmeans[1],
            ground_tilt_deg=gmeans[2],
            ground_height=gmeans[3],
            ng_epe=gmeans[5],
            ng_acc3d_strict=gmeans[6],
            ng_acc3d_relax=gmeans[7],
            ng_outlier=gmeans[8],
        )
        if ground_iou:
            results["ground_iou"] = gmeans[4]
    if voxel:
        smeans = [v / max(n, 1) for v in sample_sums]
        log.info(
            f"[test {args.dataset} sample voxel={sample_kw['voxel']} levels={sample_kw['levels']} "
            f"seed={sample_kw['seed']}] cut_level={smeans[0]:.3f} cut_radius={smeans[1]:.4f}"
        )
        results.update(sample_cut_level=smeans[0], sample_cut_radius=smeans[1])
    if denoise:
        nmeans = [v / max(n, 1) for v in noise_sums]
        log.info(
            f"[test {args.dataset} noise radius={noise_kw['radius']} min_neighbors={noise_kw['min_neighbors']} "
            f"k={noise_kw['k']} std_ratio={noise_kw['std_ratio']}] ratio={nmeans[0]:.4f} "
            f"sparse={nmeans[1]:.4f} far={nmeans[2]:.4f} mean_dist={nmeans[3]:.4f}"
        )
        results.update(noise_ratio=nmeans[0], noise_sparse_ratio=nmeans[1], noise_far_ratio=nmeans[2],
                       noise_mean_dist=nmeans[3])
    return results
