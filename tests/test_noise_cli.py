"""``test.py --noise_filter`` on synthetic data (subprocess, CPU) and the flag
without ``--sample voxel``."""

import ast
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

BASE = ["--dataset", "SYNTH", "--max_points", "128", "--truncate_k", "16", "--iters", "2",
        "--synth_len", "2", "--num_workers", "0", "--gpus", ""]
METRICS = ("loss", "epe", "acc3d_strict", "acc3d_relax", "outlier")
NOISE = ("noise_ratio", "noise_sparse_ratio", "noise_far_ratio", "noise_mean_dist")


def run_cli(tmp_path, *extra, ok=True):
    args = [sys.executable, os.path.join(REPO, "test.py"), "--root", str(tmp_path)] + BASE + list(extra)
    out = subprocess.run(args, capture_output=True, text=True, timeout=600, cwd=REPO)
    if not ok:
        return out
    assert out.returncode == 0, f"--- stdout\n{out.stdout[-1500:]}\n--- stderr\n{out.stderr[-3000:]}"
    return ast.literal_eval(out.stdout.strip().splitlines()[-1])


def test_cli_noise_filter(tmp_path):
    import pvraft_amd.ops as ops
    from pvraft_amd.data import SyntheticSceneFlow

    # 512 points in a 10 m cube: a 2.5 m radius gives every inner point neighbours
    kw = {"radius": 2.5, "min_neighbors": 6, "k": 4, "std_ratio": 1.5}
    results = run_cli(tmp_path, "--dump_results", "--sample", "voxel", "--sample_voxel", "0.25", "--noise_filter",
                      "--noise_radius", "2.5", "--noise_min_neighbors", "6", "--noise_k", "4",
                      "--noise_std_ratio", "1.5")
    for key in METRICS + NOISE + ("sample_cut_level",):
        assert key in results and np.isfinite(results[key]), key
    # the evaluator's dataset: 4 * max_points points per cloud, 2 % of them noise
    ds = SyntheticSceneFlow(128, length=2, seed=7, full_points=512, noise_fraction=0.02)
    want = {k: [] for k in NOISE}
    for i in range(2):
        (pc1, pc2), (mask, flow) = ds.load_sequence(i)
        assert int((mask[:, 0] == 0).sum()) == 10
        nf = ops.noise_filter(torch.from_numpy(pc1).unsqueeze(0), **kw)
        keep = nf.keep[0].numpy()
        d = os.path.join(str(tmp_path), "result", "SYNTH", str(i))
        noise = np.load(os.path.join(d, "noise_mask.npy"))
        assert noise.dtype == np.bool_ and np.array_equal(noise, ~keep) and noise.any() and not noise.all()
        idx1 = np.load(os.path.join(d, "sample_idx1.npy"))
        vs = ops.voxel_sample(torch.from_numpy(pc1).unsqueeze(0), 128, voxel=0.25, mask=nf.keep)
        assert np.array_equal(idx1, vs.idx[0].numpy()) and not noise[idx1].any()
        nf2 = ops.noise_filter(torch.from_numpy(pc2).unsqueeze(0), **kw)
        vs2 = ops.voxel_sample(torch.from_numpy(pc2).unsqueeze(0), 128, voxel=0.25, mask=nf2.keep)
        assert np.array_equal(np.load(os.path.join(d, "pc2.npy"))[0], pc2[vs2.idx[0].numpy()])
        count, md = nf.count[0].numpy(), nf.mean_dist[0].numpy().astype(np.float64)
        want["noise_ratio"].append((~keep).mean())
        want["noise_sparse_ratio"].append((count < 6).mean())
        want["noise_far_ratio"].append(((count < 4) | (md > float(nf.threshold[0]))).mean())
        want["noise_mean_dist"].append(float(nf.mean[0]))
    for key in NOISE:
        assert results[key] == pytest.approx(np.mean(want[key]), rel=1e-6, abs=1e-9), key


def test_cli_noise_filter_needs_the_voxel_sampler(tmp_path):
    out = run_cli(tmp_path, "--noise_filter", ok=False)
    assert out.returncode != 0 and "ValueError" in out.stderr and "--sample voxel" in out.stderr
    # and without the flag the report has none of the new keys
    plain = run_cli(tmp_path, "--sample", "voxel")
    assert not any(k in plain for k in NOISE)
    assert not os.path.exists(os.path.join(str(tmp_path), "result"))
