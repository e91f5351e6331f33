"""``test.py --ego_motion --ego_icp`` on synthetic data (subprocess, CPU), the
flag without ``--ego_motion``, and the report without the flag."""

import ast
import os
import subprocess
import sys

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

BASE = ["--dataset", "SYNTH", "--max_points", "128", "--truncate_k", "16", "--iters", "2",
        "--synth_len", "2", "--num_workers", "0", "--gpus", ""]
METRICS = ("loss", "epe", "acc3d_strict", "acc3d_relax", "outlier")
EGO = ("ego_rot_err_deg", "ego_trans_err", "ego_static_ratio", "rigid_epe",
       "rigid_acc3d_strict", "rigid_acc3d_relax", "rigid_outlier")
ICP = ("icp_rot_err_deg", "icp_trans_err", "icp_match_ratio", "icp_rmse", "icprigid_epe",
       "icprigid_acc3d_strict", "icprigid_acc3d_relax", "icprigid_outlier")


def run_cli(tmp_path, *extra, ok=True):
    args = [sys.executable, os.path.join(REPO, "test.py"), "--root", str(tmp_path)] + BASE + list(extra)
    out = subprocess.run(args, capture_output=True, text=True, timeout=600, cwd=REPO)
    if not ok:
        return out
    assert out.returncode == 0, f"--- stdout\n{out.stdout[-1500:]}\n--- stderr\n{out.stderr[-3000:]}"
    return ast.literal_eval(out.stdout.strip().splitlines()[-1])


def test_cli_ego_icp(tmp_path):
    import pvraft_amd.ops as ops
    from pvraft_amd.data import SyntheticSceneFlow

    # --dense makes SYNTH build 4 * max_points points per cloud: the full second scan is
    # larger than the sample the network sees.  An untrained model's flow is noise: a loose
    # threshold keeps static points to refine
    results = run_cli(tmp_path, "--dump_results", "--dense", "--ego_motion", "--ego_thresh", "5.0", "--ego_icp",
                      "--icp_max_dist", "2.5", "--icp_thresh", "0.5", "--icp_iters", "3")
    for key in METRICS + EGO + ICP:
        assert key in results and np.isfinite(results[key]), key
    assert 0.0 <= results["icp_match_ratio"] <= 1.0 and results["icp_rmse"] >= 0.0
    ds = SyntheticSceneFlow(128, length=2, seed=7, full_points=512)
    ratios, rmses = [], []
    for i in range(2):
        d = os.path.join(str(tmp_path), "result", "SYNTH", str(i))
        pc1 = torch.from_numpy(np.load(os.path.join(d, "pc1.npy")))
        pc2 = torch.from_numpy(ds.load_sequence(i)[0][1]).float().unsqueeze(0)
        assert pc2.shape == (1, 512, 3)
        static = torch.from_numpy(np.load(os.path.join(d, "static_mask.npy")))
        R0 = torch.from_numpy(np.load(os.path.join(d, "ego_R.npy")))
        t0 = torch.from_numpy(np.load(os.path.join(d, "ego_t.npy")))
        want = ops.icp_refine(pc1, pc2, R0=R0, t0=t0, src_mask=static, max_dist=2.5, thresh=0.5, iters=3)
        got = {k: np.load(os.path.join(d, f"icp_{k}.npy")) for k in ("R", "t", "idx", "d2")}
        assert got["R"].shape == (1, 3, 3) and got["t"].shape == (1, 3) and got["idx"].shape == (1, 128)
        assert got["idx"].dtype == np.int32 and got["d2"].dtype == np.float32
        assert np.array_equal(got["R"], want.R.numpy()) and np.array_equal(got["t"], want.t.numpy())
        assert np.array_equal(got["d2"], want.d2.numpy()) and np.array_equal(got["idx"], want.idx.numpy())
        found = got["idx"][0] >= 0
        assert (got["idx"][0][~static[0].numpy()] == -1).all() and got["idx"].max() < 512
        ratios.append(found.sum() / max(int(static.sum()), 1))
        rmses.append(float(np.sqrt(got["d2"][0][found].astype(np.float64).mean())) if found.any() else 0.0)
    assert abs(results["icp_match_ratio"] - np.mean(ratios)) <= 1e-9
    assert abs(results["icp_rmse"] - np.mean(rmses)) <= 1e-9
    assert results["icp_match_ratio"] > 0


def test_cli_ego_icp_needs_the_ego_fit(tmp_path):
    out = run_cli(tmp_path, "--ego_icp", ok=False)
    assert out.returncode != 0 and "ValueError" in out.stderr and "--ego_motion" in out.stderr
    # and without the flag the report has exactly the keys it had
    plain = run_cli(tmp_path, "--ego_motion")
    assert set(plain) == set(METRICS + EGO)
    assert not os.path.exists(os.path.join(str(tmp_path), "result"))
