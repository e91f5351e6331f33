"""``test.py --ground_fit`` on synthetic data (subprocess, CPU)."""

import ast
import os
import subprocess
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

GROUND_KEYS = ("ground_ratio", "ground_below_ratio", "ground_tilt_deg", "ground_height",
               "ng_epe", "ng_acc3d_strict", "ng_acc3d_relax", "ng_outlier")


def test_cli_ground_fit(tmp_path):
    args = [
        sys.executable, os.path.join(REPO, "test.py"), "--root", str(tmp_path),
        "--dataset", "SYNTH", "--max_points", "128", "--truncate_k", "16", "--iters", "2",
        "--synth_len", "2", "--num_workers", "0", "--gpus", "", "--dump_results",
        "--ground_fit", "--ground_hyp", "128", "--ground_iters", "2",
    ]
    out = subprocess.run(args, capture_output=True, text=True, timeout=600, cwd=REPO)
    assert out.returncode == 0, f"--- stdout\n{out.stdout[-1500:]}\n--- stderr\n{out.stderr[-3000:]}"
    results = ast.literal_eval(out.stdout.strip().splitlines()[-1])
    for key in GROUND_KEYS + ("epe", "loss"):
        assert key in results and np.isfinite(results[key]), key
    assert "ground_iou" not in results  # KITTI with --keep_ground only
    # 30 % of the synthetic points lie on y = -1.4; the rest fill a 10 m cube,
    # of which a 0.4 m slab holds 4 %
    assert abs(results["ground_ratio"] - 0.33) < 0.06
    assert results["ground_tilt_deg"] < 2.0 and abs(results["ground_height"] - 1.4) < 0.05
    dumped = os.path.join(str(tmp_path), "result", "SYNTH", "0")
    mask = np.load(os.path.join(dumped, "ground_mask.npy"))
    plane = np.load(os.path.join(dumped, "ground_plane.npy"))
    pc1 = np.load(os.path.join(dumped, "pc1.npy"))
    assert mask.shape == (1, 128) and mask.dtype == bool and plane.shape == (1, 4)
    h = pc1[0] @ plane[0, :3] + plane[0, 3]
    assert np.array_equal(mask[0][np.abs(h - 0.2) > 1e-3], (h <= 0.2)[np.abs(h - 0.2) > 1e-3])
