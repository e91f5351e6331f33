"""``test.py --sample voxel`` on synthetic data (subprocess, CPU), the
unchanged default path, and ``Batch`` with "full2"."""

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


def run_cli(tmp_path, *extra):
    args = [sys.executable, os.path.join(REPO, "test.py"), "--root", str(tmp_path)] + BASE + list(extra)
    out = subprocess.run(args, capture_output=True, text=True, timeout=600, cwd=REPO)
    assert out.returncode == 0, f"--- stdout\n{out.stdout[-1500:]}\n--- stderr\n{out.stderr[-3000:]}"
    return ast.literal_eval(out.stdout.strip().splitlines()[-1])


def test_cli_sample_voxel(tmp_path):
    import pvraft_amd.ops as ops
    from pvraft_amd.data import SyntheticSceneFlow

    kw = {"voxel": 0.25, "levels": 8, "seed": 2}
    results = run_cli(tmp_path, "--dump_results", "--sample", "voxel", "--sample_voxel", "0.25",
                      "--sample_levels", "8", "--sample_seed", "2", "--dense", "--ground_fit", "--ground_hyp", "64")
    for key in METRICS + ("sample_cut_level", "sample_cut_radius", "dense_epe", "ground_ratio"):
        assert key in results and np.isfinite(results[key]), key
    # the evaluator's dataset: 4 * max_points points per cloud, 30 % ground under --ground_fit
    ds = SyntheticSceneFlow(128, length=2, seed=7, full_points=512, ground_fraction=0.3)
    levels, radii = [], []
    for i in range(2):
        (pc1, pc2), (mask, flow) = ds.load_sequence(i)
        vs = ops.voxel_sample(torch.from_numpy(pc1).unsqueeze(0), 128, **kw)
        d = os.path.join(str(tmp_path), "result", "SYNTH", str(i))
        idx1 = np.load(os.path.join(d, "sample_idx1.npy"))
        assert idx1.dtype == np.int64 and np.array_equal(idx1, vs.idx[0].numpy())
        assert np.array_equal(np.load(os.path.join(d, "pc1.npy"))[0], pc1[idx1])
        vs2 = ops.voxel_sample(torch.from_numpy(pc2).unsqueeze(0), 128, **kw)
        assert np.array_equal(np.load(os.path.join(d, "pc2.npy"))[0], pc2[vs2.idx[0].numpy()])
        assert np.load(os.path.join(d, "pc1_full.npy")).shape == (1, 512, 3)
        ls = int((vs.occupied[0] <= 128).nonzero()[0])
        levels.append(ls)
        radii.append(3.0 ** 0.5 * 0.25 * 2.0 ** ls)
    assert results["sample_cut_level"] == pytest.approx(np.mean(levels), abs=1e-9)
    assert results["sample_cut_radius"] == pytest.approx(np.mean(radii), rel=1e-9)


def test_cli_default_is_unchanged(tmp_path):
    """Without --sample voxel: no new keys, and the metrics of the run equal
    those of evaluate() called with a namespace that has none of the new
    attributes (the parent commit's argument surface) and never calls
    ``ops.voxel_sample``, same seed."""
    # test.py has no seed flag (the weights are random without --weights, the
    # loader subsamples with numpy's global generator): seed in the child
    seeded = (
        "import sys, runpy; sys.argv = ['test.py'] + sys.argv[1:]\n"
        "import numpy, torch; torch.manual_seed(0); numpy.random.seed(0)\n"
    )

    def run_seeded(code, root, *extra):
        args = [sys.executable, "-c", seeded + code, "--root", str(root)] + BASE + list(extra)
        out = subprocess.run(args, capture_output=True, text=True, timeout=600, cwd=REPO)
        assert out.returncode == 0, out.stderr[-3000:]
        return out.stdout.strip().splitlines()

    main = "runpy.run_path('test.py', run_name='__main__')\n"
    default = ast.literal_eval(run_seeded(main, tmp_path / "a")[-1])
    explicit = ast.literal_eval(run_seeded(main, tmp_path / "b", "--sample", "random", "--sample_voxel", "0.5",
                                           "--sample_seed", "9")[-1])
    assert "sample_cut_level" not in default and "sample_cut_radius" not in default
    assert not os.path.exists(os.path.join(str(tmp_path / "a"), "result"))
    for key in METRICS:
        assert default[key] == explicit[key], key
    assert set(default) == set(explicit) == set(METRICS)
    # a child that evaluates without the new flags and records whether the
    # sampler's op was ever called
    probe = (
        "import pvraft_amd.ops as ops\n"
        "calls = []\n"
        "orig = ops.voxel_sample\n"
        "ops.voxel_sample = lambda *a, **k: (calls.append(1), orig(*a, **k))[1]\n"
        "from test import parse_args\n"
        "from pvraft_amd.engine.evaluator import evaluate\n"
        "args = parse_args()\n"
        "for k in ('sample', 'sample_voxel', 'sample_levels', 'sample_seed'):\n"
        "    delattr(args, k)\n"
        "print(evaluate(args)); print(len(calls))\n"
    )
    lines = run_seeded(probe, tmp_path / "c")
    assert lines[-1] == "0"
    bare = ast.literal_eval(lines[-2])
    assert bare == default


def test_batch_full2_roundtrip_and_rejects_batching():
    from pvraft_amd.data import Batch, SyntheticSceneFlow

    ds = SyntheticSceneFlow(64, length=3, seed=1, full_points=200)
    plain = ds[0]
    assert "full2" not in plain and "full" not in plain
    ds.return_full2 = True
    np.random.seed(0)
    item = ds[0]
    assert "full" not in item and item["full2"][0].shape == (1, 200, 3)
    (pc1, pc2), _ = ds.load_sequence(0)
    assert np.array_equal(item["full2"][0][0].numpy(), pc2)
    # no extra RNG draw: the subsample is the one drawn without the option
    np.random.seed(0)
    ds.return_full2 = False
    again = ds[0]
    assert torch.equal(again["sequence"][0], item["sequence"][0]) and torch.equal(again["sequence"][1], item["sequence"][1])
    ds.return_full2 = True
    ds.return_full = True
    item = ds[1]
    b = Batch([item]).to(torch.float64)
    assert b["full2"][0].dtype == torch.float64 and b["full2"][0].shape == (1, 200, 3)
    assert b["full"][0].dtype == torch.float64 and b["sequence"][0].dtype == torch.float64
    assert torch.equal(b["full2"][0].float(), item["full2"][0])
    with pytest.raises(ValueError):
        Batch([ds[0], ds[1]])
    ds.return_full = False
    with pytest.raises(ValueError):
        Batch([ds[0], ds[1]])
