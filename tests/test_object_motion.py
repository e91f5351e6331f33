"""CPU tests of the moving-object layer: the torch reference of
``cluster_points`` / ``segmented_rigid_fit`` against the independent numpy
oracle of object_cases.py, degenerate inputs, argument checks,
``ops.object_motion`` on a driving scene with three rigid boxes, the
Predictor method and the ``test.py --object_motion`` command line."""

import ast
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import pvraft_amd.ops as ops
from ego_cases import coord_scale, max_dev, rigid_pair, third_zero_weights
from object_cases import (
    SCENES,
    check_driving_scene,
    make_case,
    make_driving_scene,
    oracle_cluster,
    oracle_object_fits,
    segment_labels,
)
from pvraft_amd.ops import reference as R

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SCENE_N = {"blobs": 257, "chain": 300, "broken_chain": 300, "twin_chains": 301, "ties": 129, "overflow": 257}


def assert_partition(got, want):
    for g, w, name in zip(got, want, ("labels", "count", "num_objects")):
        assert g.dtype == torch.int32, name
        assert np.array_equal(g.cpu().numpy().astype(np.int64), w), name


@pytest.mark.parametrize("kind", SCENES)
def test_reference_clusters_match_oracle(kind):
    c = make_case(kind, 2, SCENE_N[kind], seed=3)
    want = oracle_cluster(c["xyz"], c["flow"], c["mask"], **c["kw"])
    assert want[2].min() >= 1 or kind == "blobs"
    assert_partition(ops.cluster_points(c["xyz"], c["flow"], c["mask"], **c["kw"]), want)
    assert_partition(ops.cluster_points(c["xyz"].double(), c["flow"].double(), c["mask"], **c["kw"]), want)


def test_scene_properties():
    """The scenes exercise what they are meant to."""
    c = make_case("broken_chain", 1, 300, seed=3)
    lab, cnt, n = oracle_cluster(c["xyz"], c["flow"], c["mask"], **c["kw"])
    assert n[0] == 2 and cnt[0, :2].tolist() == [200, 100]
    c = make_case("twin_chains", 1, 301, seed=3)
    assert oracle_cluster(c["xyz"], c["flow"], c["mask"], **c["kw"])[1][0, :3].tolist() == [151, 150, 0]
    kw = dict(c["kw"], flow_eps=float("inf"))
    want = oracle_cluster(c["xyz"], c["flow"], c["mask"], **kw)
    assert want[1][0, :2].tolist() == [301, 0]
    assert_partition(ops.cluster_points(c["xyz"], c["flow"], c["mask"], **kw), want)
    c = make_case("ties", 1, 129, seed=3)
    lab, cnt, n = oracle_cluster(c["xyz"], c["flow"], c["mask"], **c["kw"])
    assert n[0] == 6 and cnt[0, :6].tolist() == [12] * 6
    first = [int(np.nonzero(lab[0] == m)[0].min()) for m in range(6)]
    assert first == sorted(first)
    c = make_case("overflow", 1, 257, seed=3)
    lab, cnt, n = oracle_cluster(c["xyz"], c["flow"], c["mask"], **c["kw"])
    assert n[0] == 4 and cnt[0].tolist() == [30, 20, 14, 11]
    kw = dict(c["kw"], max_objects=32)
    assert oracle_cluster(c["xyz"], c["flow"], c["mask"], **kw)[1][0, :8].tolist() == [30, 20, 14, 11, 9, 9, 8, 0]


def test_degenerate_cluster_inputs():
    for n in (0, 1, 2):
        xyz = torch.zeros(2, n, 3)
        lab, cnt, num = ops.cluster_points(xyz, xyz, torch.ones(2, n, dtype=torch.bool), min_points=3, max_objects=4)
        assert lab.shape == (2, n) and cnt.shape == (2, 4) and num.shape == (2,)
        assert (lab == -1).all() and (cnt == 0).all() and (num == 0).all()
    c = make_case("blobs", 2, 129, seed=5)
    none = ops.cluster_points(c["xyz"], c["flow"], torch.zeros_like(c["mask"]), **c["kw"])
    assert (none[0] == -1).all() and (none[2] == 0).all()
    everything = torch.ones_like(c["mask"])
    # the unmasked filler points are random: only the oracle's eligibility
    # matters here, not their clearance
    lat = make_case("chain", 2, 129, seed=5)
    assert_partition(ops.cluster_points(lat["xyz"], lat["flow"], everything, **lat["kw"]),
                     oracle_cluster(lat["xyz"], lat["flow"], everything, **lat["kw"]))


def test_non_finite_points_are_excluded():
    c = make_case("blobs", 2, 257, seed=7)
    xyz, flow = c["xyz"].clone(), c["flow"].clone()
    base = oracle_cluster(xyz, flow, c["mask"], **c["kw"])
    hit = [int(np.nonzero(base[0][b] == 0)[0][k]) for b in range(2) for k in (0, 1, 2)]
    xyz[0, hit[0], 1] = float("nan")
    flow[0, hit[1], 0] = float("inf")
    xyz[1, hit[3], 2] = float("-inf")
    flow[1, hit[4], 2] = float("nan")
    want = oracle_cluster(xyz, flow, c["mask"], **c["kw"])
    assert want[0][0, hit[0]] == -1 and want[0][0, hit[1]] == -1 and want[0][1, hit[3]] == -1
    assert want[1][0, 0] == base[1][0, 0] - 2
    assert_partition(ops.cluster_points(xyz, flow, c["mask"], **c["kw"]), want)


@pytest.mark.parametrize("kw", [{"min_points": 2}, {"max_objects": 0}, {"max_objects": 257}, {"eps": -1.0},
                                {"flow_eps": float("nan")}])
def test_cluster_bad_arguments_raise(kw):
    c = make_case("blobs", 1, 64, seed=1)
    with pytest.raises(ValueError):
        ops.cluster_points(c["xyz"], c["flow"], c["mask"], **kw)


@pytest.mark.parametrize("kw", [{"iters": -1}, {"iters": 65}, {"thresh": 0.0}, {"num_segments": 0}])
def test_segmented_fit_bad_arguments_raise(kw):
    src, dst = rigid_pair(1, 10, seed=2)
    args = dict(num_segments=2, iters=0, thresh=0.05)
    args.update(kw)
    with pytest.raises(ValueError):
        ops.segmented_rigid_fit(src, dst, torch.zeros(1, 10, dtype=torch.int32), **args)
    with pytest.raises(ValueError):
        ops.segmented_rigid_fit(src, dst, torch.zeros(1, 10), 2)


SIZES = [40, 0, 1, 2, 3, 63, 17]


@pytest.mark.parametrize("iters", [0, 5])
def test_segmented_fit_matches_oracle(iters):
    """float64 tight; float32 within the tolerances test_ego_motion.py uses
    for the plain fit on the same box cloud (1e-5 for R, 1e-4 m for t and
    the residuals: rounding of 35 m coordinates times the lever arm)."""
    B, N = 2, 160
    src, dst = rigid_pair(B, N, seed=31, noise=0.005)
    labels = segment_labels(B, N, SIZES, seed=4)
    labels[0, labels[0] == -1] = torch.tensor([len(SIZES), -7, 99] * 12)[: int((labels[0] == -1).sum())].int()
    w = third_zero_weights(B, N, seed=9)
    for weights in (None, w):
        want = oracle_object_fits(src, dst, labels, len(SIZES), weights, 0.05, iters)
        got64 = ops.segmented_rigid_fit(src.double(), dst.double(), labels, len(SIZES),
                                        None if weights is None else weights.double(), 0.05, iters)
        got32 = ops.segmented_rigid_fit(src, dst, labels, len(SIZES), weights, 0.05, iters)
        assert got64[0].dtype == torch.float64 and got32[0].dtype == torch.float32
        # three random points determine R badly; R and t of such a segment are
        # compared through the residuals only
        firm = np.array([s >= 4 for s in SIZES])
        for got, tol in ((got64, (1e-9, 1e-8, 1e-8)), (got32, (1e-5, 1e-4, 1e-4))):
            assert np.array_equal(got[3].numpy(), want[3])
            if weights is None:
                assert got[3].numpy().tolist() == [[s >= 3 for s in SIZES]] * B
            assert max_dev(got[0][:, firm], want[0][:, firm]) <= tol[0]
            assert max_dev(got[1][:, firm], want[1][:, firm]) <= tol[1]
            assert max_dev(got[2], want[2]) <= tol[2]
            assert got[0].shape == (B, len(SIZES), 3, 3) and got[2].shape == (B, N)
        assert torch.isinf(got32[2][labels == -1]).all() and torch.isinf(got32[2][0][labels[0] >= len(SIZES)]).all()
        eye = torch.eye(3)
        for m in (1, 2, 3):
            assert torch.equal(got32[0][:, m], eye.expand(B, 3, 3))


def test_one_segment_is_the_plain_fit():
    src, dst = rigid_pair(2, 90, seed=12, noise=0.005)
    one = ops.segmented_rigid_fit(src, dst, torch.zeros(2, 90, dtype=torch.int64), 1, iters=4)
    plain = ops.rigid_fit(src, dst, iters=4)
    assert torch.equal(one[0][:, 0], plain[0]) and torch.equal(one[1][:, 0], plain[1])
    assert torch.equal(one[2], plain[2]) and torch.equal(one[3][:, 0], plain[3])


def test_ops_upcast_and_take_strided_inputs():
    c = make_case("blobs", 1, 129, seed=2)
    want = ops.cluster_points(c["xyz"], c["flow"], c["mask"], **c["kw"])
    strided = torch.empty(1, 129, 6)[..., ::2]
    strided.copy_(c["xyz"])
    assert not strided.is_contiguous()
    assert_partition(ops.cluster_points(strided, c["flow"], c["mask"], **c["kw"]), [w.numpy() for w in want])
    # bf16 rounds the coordinates: the call must work and return int32
    half = ops.cluster_points(c["xyz"].bfloat16(), c["flow"].bfloat16(), c["mask"], **c["kw"])
    assert half[0].dtype == torch.int32 and half[0].shape == (1, 129)
    src, dst = rigid_pair(1, 50, seed=8, noise=0.005)
    lab = segment_labels(1, 50, [20, 20], seed=1)
    fit = ops.segmented_rigid_fit(src, dst, lab, 2, iters=2)
    strided = torch.empty(1, 50, 6)[..., ::2]
    strided.copy_(src)
    for g, w in zip(ops.segmented_rigid_fit(strided, dst, lab.long(), 2, iters=2), fit):
        assert torch.equal(g, w)
    assert ops.segmented_rigid_fit(src.bfloat16(), dst.bfloat16(), lab, 2)[0].dtype == torch.float32
    assert not any(x.requires_grad for x in ops.segmented_rigid_fit(src.requires_grad_(True), dst, lab, 2))


def test_object_motion_driving_scene():
    """CPU float32 tolerances: a box of ~100 points 1 m across pins its
    rotation ~30x worse than the full cloud does (1e-4 instead of 1e-5 / 3),
    and t = c' - R c carries that error over the 35 m lever arm (3e-3 m);
    the residuals are taken in the pivot frame and stay at 1e-4 m."""
    sc = make_driving_scene(2, 1024, seed=40)
    om = ops.object_motion(sc["pc1"], sc["flow"], iters=5, **sc["kw"])
    assert isinstance(om, ops.ObjectMotion) and isinstance(om.ego, ops.EgoMotion)
    check_driving_scene(sc, om)
    # an ego fit handed in is used as it is
    again = ops.object_motion(sc["pc1"], sc["flow"], ego=om.ego, iters=5, **sc["kw"])
    assert again.ego is om.ego and torch.equal(again.labels, om.labels) and torch.equal(again.rigid_flow, om.rigid_flow)
    # rigid_flow: object flow in objects, ego flow on static points
    p = sc["pc1"]
    b, i = 0, int(np.nonzero(sc["labels"][0].numpy() == 1)[0][0])
    assert torch.allclose(om.rigid_flow[b, i], om.R[b, 1] @ p[b, i] + om.t[b, 1] - p[b, i], atol=1e-5)
    assert torch.equal(om.rigid_flow[sc["static"]], om.ego.rigid_flow[sc["static"]])
    assert torch.isinf(om.residual[sc["static"]]).all() and torch.isfinite(om.residual[~sc["static"]]).all()


def test_predictor_object_motion_cpu():
    from pvraft_amd.engine import Predictor
    from pvraft_amd.model import PVRaft

    torch.manual_seed(11)
    model = PVRaft(truncate_k=16).eval()
    pred = Predictor(model, points=48, batch=2, iters=2)
    g = torch.Generator().manual_seed(4)
    xyz1 = torch.randn(2, 48, 3, generator=g)
    xyz2 = xyz1 + 0.05 * torch.randn(2, 48, 3, generator=g)
    flow, om = pred.predict_object_motion(xyz1, xyz2, min_points=3, max_objects=5, ego_iters=3)
    assert torch.equal(flow, pred(xyz1, xyz2))
    assert isinstance(om, ops.ObjectMotion)
    assert om.labels.shape == (2, 48) and om.count.shape == (2, 5) and om.num_objects.shape == (2,)
    assert om.R.shape == (2, 5, 3, 3) and om.t.shape == (2, 5, 3) and om.ok.shape == (2, 5)
    assert om.residual.shape == (2, 48) and om.rigid_flow.shape == (2, 48, 3)
    want = ops.object_motion(xyz1, flow, min_points=3, max_objects=5, ego_iters=3)
    for a, b in zip(om[:-1], want[:-1]):
        assert torch.equal(a, b)


OBJ_KEYS = ("obj_count", "obj_point_ratio", "objrigid_epe", "objrigid_acc3d_strict", "objrigid_acc3d_relax",
            "objrigid_outlier")


def test_cli_object_motion(tmp_path):
    base = [
        sys.executable, os.path.join(REPO, "test.py"), "--root", str(tmp_path),
        "--dataset", "SYNTH", "--max_points", "48", "--truncate_k", "16", "--iters", "2",
        "--synth_len", "2", "--num_workers", "0", "--gpus", "",
    ]
    runs = {}
    for name, extra in (("plain", []), ("obj", ["--dump_results", "--object_motion", "--obj_min_points", "3",
                                                 "--obj_max_objects", "6", "--obj_iters", "2", "--ego_iters", "3"])):
        out = subprocess.run(base + extra, capture_output=True, text=True, timeout=600, cwd=REPO)
        assert out.returncode == 0, f"--- stdout\n{out.stdout[-1500:]}\n--- stderr\n{out.stderr[-3000:]}"
        runs[name] = ast.literal_eval(out.stdout.strip().splitlines()[-1])
    plain, results = runs["plain"], runs["obj"]
    for key in OBJ_KEYS:
        assert key in results and np.isfinite(results[key]), key
        assert key not in plain
    assert set(results) == set(plain) | set(OBJ_KEYS)
    # the old keys are the old keys (their values differ run to run: test.py
    # without --weights evaluates a randomly initialised model)
    assert set(plain) == {"loss", "epe", "acc3d_strict", "acc3d_relax", "outlier"}
    for key in plain:
        assert np.isfinite(results[key]), key
    assert 0.0 <= results["obj_point_ratio"] <= 1.0 and 0.0 <= results["obj_count"] <= 6.0
    dumped = os.path.join(str(tmp_path), "result", "SYNTH", "0")
    lab = np.load(os.path.join(dumped, "object_labels.npy"))
    assert lab.shape == (1, 48) and lab.dtype == np.int32
    assert np.load(os.path.join(dumped, "obj_R.npy")).shape == (1, 6, 3, 3)
    assert np.load(os.path.join(dumped, "obj_t.npy")).shape == (1, 6, 3)
    assert np.load(os.path.join(dumped, "flow_objrigid.npy")).shape == (1, 48, 3)
    assert sorted(os.listdir(dumped)) == [
        "flow.npy", "flow_objrigid.npy", "obj_R.npy", "obj_t.npy", "object_labels.npy", "pc1.npy", "pc2.npy",
    ]
