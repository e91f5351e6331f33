"""bench.py contract test (CPU plumbing config)."""

import json
import os
import subprocess
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_bench_emits_contract_json():
    out = subprocess.run(
        [
            sys.executable,
            os.path.join(REPO, "bench.py"),
            "--device", "cpu", "--points", "96", "--steps", "2", "--warmup", "1",
            "--batch", "1", "--truncate_k", "16", "--no-amp",
        ],
        capture_output=True,
        text=True,
        timeout=300,
        cwd=REPO,
    )
    assert out.returncode == 0, out.stderr[-2000:]
    lines = [l for l in out.stdout.strip().splitlines() if l.startswith("{")]
    assert lines, out.stdout
    rec = json.loads(lines[-1])
    for key in (
        "metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step",
        "higher_is_better", "scaling", "vs_baseline", "dtype", "data", "config",
    ):
        assert key in rec, key
    assert rec["metric"] == "train_pairs_per_sec"
    assert rec["value"] > 0
    assert rec["steps"] == 2 and rec["warmup"] == 1
    assert rec["scaling"] == "weak"
    assert rec["data"] == "synthetic"
    assert rec["config"]["gru_iters"] == 8


def test_bench_dump_outputs_repeatable_and_full(tmp_path):
    """--dump-outputs writes the last timed step's loss and final flow as
    float32 .npy, and the same arguments give the same inputs and initial
    weights: with one step and no warmup the dump is the forward of those
    weights, which two processes reproduce up to fp32 summation order
    (reductions over <= 96 points x 8 GRU iterations: ~1e-6 relative at
    worst, gated at 1e-4; another seed moves the O(1) flow by O(1)).
    --full is accepted and leaves the result line's meaning unchanged."""
    import numpy as np

    recs, dumps = [], []
    for name, extra in (("a", []), ("b", ["--full"])):
        d = tmp_path / name
        out = subprocess.run(
            [
                sys.executable, os.path.join(REPO, "bench.py"),
                "--device", "cpu", "--points", "96", "--steps", "1", "--warmup", "0",
                "--batch", "2", "--truncate_k", "16", "--no-amp",
                "--dump-outputs", str(d),
            ] + extra,
            capture_output=True, text=True, timeout=300, cwd=REPO,
        )
        assert out.returncode == 0, out.stderr[-2000:]
        lines = [l for l in out.stdout.strip().splitlines() if l.startswith("{")]
        recs.append(json.loads(lines[-1]))
        assert sorted(os.listdir(d)) == ["final_flow.npy", "loss.npy"]
        dumps.append({f[:-4]: np.load(d / f) for f in os.listdir(d)})
    for rec in recs:
        assert rec["steps"] == 1 and rec["warmup"] == 0 and rec["ms_per_step"] > 0
        assert rec["metric"] == "train_pairs_per_sec" and rec["unit"] == "pairs/s"
        assert rec["higher_is_better"] is True and rec["dtype"] == "fp32"
        assert abs(rec["value"] - 2 / (rec["ms_per_step"] * 1e-3)) < 1e-6 * rec["value"]
    assert set(recs[0]) == set(recs[1])
    a, b = dumps
    assert a["final_flow"].shape == (2, 96, 3) and a["loss"].shape == ()
    for k in a:
        assert a[k].dtype == np.float32 and np.isfinite(a[k]).all()
        assert np.allclose(a[k], b[k], rtol=1e-4, atol=1e-4), (
            k, np.abs(a[k] - b[k]).max())
    assert np.abs(a["final_flow"]).max() > 0.1  # an O(1) field, not zeros


def test_bench_two_ranks_cpu_gloo():
    """The distributed bench path (torchrun, gloo on CPU) emits aggregate
    whole-job throughput with n_gpus from the world size env."""
    env = dict(os.environ)
    env.pop("HIP_VISIBLE_DEVICES", None)
    env["CUDA_VISIBLE_DEVICES"] = ""  # force CPU so gloo is selected
    out = subprocess.run(
        [
            sys.executable, "-m", "torch.distributed.run", "--nnodes=1",
            "--nproc-per-node", "2", "--master-addr", "127.0.0.1",
            "--master-port", "29711", os.path.join(REPO, "bench.py"),
            "--device", "cpu", "--points", "64", "--steps", "2", "--warmup", "1",
            "--batch", "1", "--truncate_k", "16", "--no-amp", "--no-graph",
        ],
        capture_output=True, text=True, timeout=420, cwd=REPO, env=env,
    )
    assert out.returncode == 0, out.stderr[-3000:]
    lines = [l for l in out.stdout.strip().splitlines() if l.startswith("{")]
    rec = json.loads(lines[-1])
    assert rec["config"]["parallelism"] == "dp2"
    assert rec["config"]["global_batch"] == 2
