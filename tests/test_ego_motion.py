"""Ego-motion on the CPU path: the torch reference of the robust rigid fit
against an independent float64 oracle, its degenerate inputs, and the layers
built on it (ops.ego_motion, Predictor.predict_ego_motion, test.py
--ego_motion)."""

import ast
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import pvraft_amd.ops as ops
from ego_cases import (
    ROBUST_CASES,
    make_scene,
    oracle_fit,
    max_dev,
    rigid_pair,
    rot_angle_deg,
    rotvec_matrix,
)
from pvraft_amd.ops import reference as R

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
THRESH = 0.05
ROUNDS = 10


@pytest.fixture(scope="module")
def robust():
    """(scene, oracle) for every robust case, computed once."""
    out = {}
    for N, dyn, planar in ROBUST_CASES:
        sc = make_scene(1, N, dyn, seed=N + int(100 * dyn), planar=planar)
        dst = sc["pc1"] + sc["flow"]
        out[(N, dyn, planar)] = (sc, oracle_fit(sc["pc1"], dst, None, THRESH, ROUNDS))
    return out


@pytest.mark.parametrize("case", ROBUST_CASES)
def test_generator_and_oracle(robust, case):
    """What the GPU tests rely on: the oracle recovers the true motion, the
    classification is the true labelling with a margin, IRLS has converged."""
    sc, (Ro, to, ro, oko) = robust[case]
    assert oko.all()
    ang = rot_angle_deg(Ro[0], sc["R"]).item()
    terr = np.linalg.norm(to[0] - sc["t"])
    print(f"oracle vs truth: {ang:.4f} deg, {terr * 1e3:.2f} mm")
    assert ang <= 0.02 and terr <= 0.005
    assert np.array_equal(ro[0] < THRESH, sc["static"][0].numpy())
    assert np.abs(ro - THRESH).min() > 1e-3
    R9, t9, _, _ = oracle_fit(sc["pc1"], sc["pc1"] + sc["flow"], None, THRESH, ROUNDS - 1)
    assert np.abs(R9 - Ro).max() <= 1e-12 and np.abs(t9 - to).max() <= 1e-12


@pytest.mark.parametrize("case", ROBUST_CASES)
def test_reference_matches_oracle_float64(robust, case):
    sc, (Ro, to, ro, oko) = robust[case]
    src = sc["pc1"].double()
    dst = (sc["pc1"] + sc["flow"]).double()
    Rr, tr, rr, okr = R.rigid_fit(src, dst, None, THRESH, ROUNDS)
    assert Rr.dtype == tr.dtype == rr.dtype == torch.float64 and okr.dtype == torch.bool
    assert Rr.shape == (1, 3, 3) and tr.shape == (1, 3) and rr.shape == src.shape[:2] and okr.shape == (1,)
    errs = (max_dev(Rr, Ro), max_dev(tr, to), max_dev(rr, ro))
    print("max |ref64 - oracle| R %.2e t %.2e r %.2e" % errs)
    assert max(errs) <= 1e-9
    assert okr.all()


@pytest.mark.parametrize("case", ROBUST_CASES)
def test_robust_fit_beats_least_squares_and_classifies(robust, case):
    sc, _ = robust[case]
    ego = ops.ego_motion(sc["pc1"], sc["flow"], thresh=THRESH, iters=ROUNDS)
    ls = ops.ego_motion(sc["pc1"], sc["flow"], thresh=THRESH, iters=0)
    assert ego.R.dtype == torch.float32 and ego.static.dtype == torch.bool
    assert ego.rigid_flow.shape == sc["flow"].shape
    for name, fit in (("robust", ego), ("least squares", ls)):
        print(f"{name}: {rot_angle_deg(fit.R[0], sc['R']).item():.4f} deg, "
              f"{np.linalg.norm(fit.t[0].double().numpy() - sc['t']) * 1e3:.2f} mm")
    assert rot_angle_deg(ego.R[0], sc["R"]) < rot_angle_deg(ls.R[0], sc["R"])
    assert np.linalg.norm(ego.t[0].double().numpy() - sc["t"]) < np.linalg.norm(ls.t[0].double().numpy() - sc["t"])
    assert torch.equal(ego.static, sc["static"])
    assert ego.ok.all()
    want = sc["pc1"] @ ego.R[0].T + ego.t[0] - sc["pc1"]
    assert torch.allclose(ego.rigid_flow, want, atol=1e-5)


EXACT = [
    ("small", rotvec_matrix((0.01, 0.03, -0.005)), False),
    ("170deg", rotvec_matrix(np.deg2rad(170) * np.array([0.6, 0.0, 0.8])), False),
    ("planar", rotvec_matrix((0.2, -0.4, 0.1)), True),
]


@pytest.mark.parametrize("name,Rt,planar", EXACT, ids=[e[0] for e in EXACT])
def test_exact_recovery_float64(name, Rt, planar):
    """Noise-free rigid scene, plain fit: R and t to 1e-10, including a
    170 degree rotation and a planar cloud (whose unconstrained optimum is
    a reflection as good as the rotation)."""
    t = np.array([0.1, -0.05, 1.0])
    src, _ = rigid_pair(2, 65, seed=3, planar=planar)
    src = src.double()
    dst = src @ torch.from_numpy(Rt).T + torch.from_numpy(t)
    Rr, tr, rr, ok = R.rigid_fit(src, dst, iters=0)
    assert ok.all()
    assert (Rr - torch.from_numpy(Rt)).abs().max().item() <= 1e-10
    assert (tr - torch.from_numpy(t)).abs().max().item() <= 1e-10
    assert rr.max().item() <= 1e-9
    assert (torch.linalg.det(Rr) - 1).abs().max().item() <= 1e-10


def test_degenerate_inputs_are_not_errors():
    src, dst = rigid_pair(1, 8, seed=1)
    eye = torch.eye(3)
    for fn in (R.rigid_fit, ops.rigid_fit):
        # N = 1 and N = 2: R = I, t = mean displacement
        for n in (1, 2):
            Rr, tr, rr, ok = fn(src[:, :n], dst[:, :n], iters=3)
            assert not ok.any() and torch.equal(Rr[0], eye)
            assert torch.allclose(tr[0], (dst[:, :n] - src[:, :n]).mean(1)[0], atol=1e-6)
            assert torch.allclose(rr, (src[:, :n] + tr[:, None] - dst[:, :n]).norm(dim=-1), atol=1e-6)
        # weighted mean under the prior
        w = torch.tensor([[3.0, 1.0]])
        _, tr, _, ok = fn(src[:, :2], dst[:, :2], w)
        d = dst[:, :2] - src[:, :2]
        assert not ok.any() and torch.allclose(tr[0], (3 * d[0, 0] + d[0, 1]) / 4, atol=1e-6)
        # all weights zero: no usable point, t = 0, residual = |dst - src|
        Rr, tr, rr, ok = fn(src, dst, torch.zeros(1, 8), iters=2)
        assert not ok.any() and torch.equal(Rr[0], eye) and torch.equal(tr, torch.zeros(1, 3))
        assert torch.allclose(rr, (dst - src).norm(dim=-1), atol=1e-6)
        # all points NaN
        nan = torch.full_like(src, float("nan"))
        Rr, tr, rr, ok = fn(nan, dst, iters=2)
        assert not ok.any() and torch.equal(Rr[0], eye) and torch.equal(tr, torch.zeros(1, 3))
        assert torch.isinf(rr).all() and (rr > 0).all()


def test_nan_points_and_bad_weights_are_skipped():
    src, dst = rigid_pair(2, 40, seed=5, noise=0.005)
    w = torch.ones(2, 40)
    w[:, 3] = 0.0
    w[:, 4] = -2.0
    w[:, 5] = float("nan")
    keep = torch.ones(40, dtype=torch.bool)
    keep[[3, 4, 5, 7, 9]] = False
    want = R.rigid_fit(src[:, keep].double(), dst[:, keep].double(), iters=4)
    bad_src, bad_dst = src.clone(), dst.clone()
    bad_src[:, 7, 1] = float("nan")
    bad_dst[:, 9, 0] = float("inf")
    # the unweighted points are pushed away: they must not pull the fit
    bad_dst[:, 3:6] += 5.0
    for fn in (R.rigid_fit, ops.rigid_fit):
        Rr, tr, rr, ok = fn(bad_src, bad_dst, w, iters=4)
        assert ok.all()
        assert (Rr.double() - want[0]).abs().max().item() <= 1e-5
        assert (tr.double() - want[1]).abs().max().item() <= 1e-4
        assert torch.isinf(rr[:, [7, 9]]).all() and (rr[:, [7, 9]] > 0).all()
        assert torch.isfinite(rr[:, keep]).all() and (rr[:, 3:6] > 4.0).all()
        assert (rr[:, keep].double() - want[2]).abs().max().item() <= 1e-4
    ego = ops.ego_motion(bad_src, bad_dst - bad_src, weights=w, iters=4)
    assert not ego.static[:, [3, 4, 5, 7, 9]].any() and ego.static[:, keep].all()


def test_op_upcasts_and_takes_strided_inputs():
    src, dst = rigid_pair(1, 50, seed=8, noise=0.005)
    want = ops.rigid_fit(src, dst, iters=2)
    strided = torch.empty(1, 50, 6)[..., ::2]
    strided.copy_(src)
    assert not strided.is_contiguous()
    got = ops.rigid_fit(strided, dst, iters=2)
    for g, w in zip(got, want):
        assert torch.equal(g, w)
    half = ops.rigid_fit(src.bfloat16(), dst.bfloat16(), iters=2)
    assert half[0].dtype == torch.float32
    assert ops.rigid_fit(src.double(), dst.double())[0].dtype == torch.float64
    assert not any(x.requires_grad for x in ops.rigid_fit(src.requires_grad_(True), dst))


@pytest.mark.parametrize("kw", [{"iters": -1}, {"iters": 65}, {"thresh": 0.0}, {"thresh": -1.0}])
def test_bad_arguments_raise(kw):
    src, dst = rigid_pair(1, 10, seed=2)
    with pytest.raises(ValueError):
        R.rigid_fit(src, dst, **kw)
    with pytest.raises(ValueError):
        ops.rigid_fit(src, dst, **kw)


def test_predictor_ego_motion_cpu():
    from pvraft_amd.engine import Predictor
    from pvraft_amd.model import PVRaft

    torch.manual_seed(11)
    model = PVRaft(truncate_k=16).eval()
    pred = Predictor(model, points=48, batch=2, iters=2)
    g = torch.Generator().manual_seed(4)
    xyz1 = torch.randn(2, 48, 3, generator=g)
    xyz2 = xyz1 + 0.05 * torch.randn(2, 48, 3, generator=g)
    flow, ego = pred.predict_ego_motion(xyz1, xyz2, thresh=0.05, iters=3)
    assert torch.equal(flow, pred(xyz1, xyz2))
    assert isinstance(ego, ops.EgoMotion)
    assert ego.R.shape == (2, 3, 3) and ego.t.shape == (2, 3) and ego.ok.shape == (2,)
    assert ego.residual.shape == (2, 48) and ego.static.shape == (2, 48) and ego.rigid_flow.shape == (2, 48, 3)
    assert ego.ok.all() and ego.static.dtype == torch.bool
    assert torch.allclose(torch.linalg.det(ego.R), torch.ones(2), atol=1e-5)


EGO_KEYS = ("ego_rot_err_deg", "ego_trans_err", "ego_static_ratio", "rigid_epe",
            "rigid_acc3d_strict", "rigid_acc3d_relax", "rigid_outlier")


def test_cli_ego_motion(tmp_path):
    args = [
        sys.executable, os.path.join(REPO, "test.py"), "--root", str(tmp_path),
        "--dataset", "SYNTH", "--max_points", "48", "--truncate_k", "16", "--iters", "2",
        "--synth_len", "2", "--num_workers", "0", "--gpus", "", "--dump_results",
        "--ego_motion", "--ego_iters", "5",
    ]
    out = subprocess.run(args, capture_output=True, text=True, timeout=600, cwd=REPO)
    assert out.returncode == 0, f"--- stdout\n{out.stdout[-1500:]}\n--- stderr\n{out.stderr[-3000:]}"
    results = ast.literal_eval(out.stdout.strip().splitlines()[-1])
    for key in EGO_KEYS + ("epe", "loss"):
        assert key in results and np.isfinite(results[key]), key
    assert 0.0 <= results["ego_static_ratio"] <= 1.0
    dumped = os.path.join(str(tmp_path), "result", "SYNTH", "0")
    assert np.load(os.path.join(dumped, "ego_R.npy")).shape == (1, 3, 3)
    assert np.load(os.path.join(dumped, "ego_t.npy")).shape == (1, 3)
    mask = np.load(os.path.join(dumped, "static_mask.npy"))
    assert mask.shape == (1, 48) and mask.dtype == np.bool_
    assert np.load(os.path.join(dumped, "flow_rigid.npy")).shape == (1, 48, 3)
    assert sorted(os.listdir(dumped)) == [
        "ego_R.npy", "ego_t.npy", "flow.npy", "flow_rigid.npy", "pc1.npy", "pc2.npy", "static_mask.npy",
    ]
