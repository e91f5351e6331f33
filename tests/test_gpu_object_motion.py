"""GPU tests of the clustering kernels (csrc/cluster.hip), the segmented
rigid fit (csrc/rigid_fit.hip) and the layers on them.  Partitions are
compared exactly with the numpy oracle of object_cases.py; fits with the
float64 oracle within ego_cases.bound (eight times the deviation of the fp32
CPU reference on the same input, floored at 16 ulp of the data).  Run with
-m gpu."""

import functools
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from ego_cases import bound, box_cloud, coord_scale, max_dev, oracle_fit, rigid_pair
from object_cases import (
    check_driving_scene,
    make_case,
    make_driving_scene,
    oracle_cluster,
    oracle_object_fits,
    segment_labels,
)

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    import pvraft_amd.ops as ops
    from pvraft_amd.ops import reference as R

THRESH = 0.05


@pytest.fixture(scope="module", autouse=True)
def _require_gpu_and_ext():
    if not torch.cuda.is_available():
        pytest.skip("needs GPU")
    import pvraft_amd.ops as ops

    assert ops.hip_available(), "HIP extension must be built on the GPU box"


def dev():
    return torch.device("cuda:0")


def ext_const(name, default):
    if not torch.cuda.is_available():
        return default
    from pvraft_amd import _C

    return int(getattr(_C, name))


def cluster_cases():
    T = ext_const("CLUSTER_TILE", 256)
    cases = [("blobs", b, n) for b, n in ((1, 1), (1, 2), (1, 3), (2, 63), (2, 64), (3, 65), (2, 257))]
    cases += [("blobs", 1, n) for n in (T - 1, T, T + 1, 2 * T + 1) if ("blobs", 1, n) not in cases]
    cases += [(k, 2, 1025) for k in ("chain", "broken_chain", "twin_chains")]
    cases += [("ties", 2, 257), ("overflow", 2, 257)]
    return cases


@functools.lru_cache(maxsize=None)
def case_and_oracle(kind, B, N):
    """Inputs and the oracle's answer, computed once and shared (read-only)."""
    c = make_case(kind, B, N, seed=11)
    return c, oracle_cluster(c["xyz"], c["flow"], c["mask"], **c["kw"])


def gpu_cluster(xyz, flow, mask, **kw):
    out = ops.cluster_points(xyz.to(dev()), flow.to(dev()), mask.to(dev()), **kw)
    torch.cuda.synchronize()
    return out


def assert_partition(got, want):
    for g, w, name in zip(got, want, ("labels", "count", "num_objects")):
        assert g.dtype == torch.int32 and g.is_cuda, name
        assert np.array_equal(g.cpu().numpy().astype(np.int64), w), name
    assert (got[2] >= 0).all(), "a retry cap was hit"


def pytest_generate_tests(metafunc):
    if "cluster_case" in metafunc.fixturenames:
        cs = cluster_cases()
        metafunc.parametrize("cluster_case", cs, ids=[f"{k}-{b}x{n}" for k, b, n in cs])


# ---------------------------------------------------------------------------
# 1. clustering kernels vs oracle
# ---------------------------------------------------------------------------


def test_cluster_matches_oracle(cluster_case):
    c, want = case_and_oracle(*cluster_case)
    got = gpu_cluster(c["xyz"], c["flow"], c["mask"], **c["kw"])
    assert got[0].shape == c["mask"].shape and got[1].shape == (c["mask"].shape[0], c["kw"]["max_objects"])
    assert_partition(got, want)


def test_cluster_without_flow_test():
    c, _ = case_and_oracle("twin_chains", 2, 1025)
    kw = dict(c["kw"], flow_eps=float("inf"))
    want = oracle_cluster(c["xyz"], c["flow"], c["mask"], **kw)
    assert want[1][:, :2].tolist() == [[1025, 0]] * 2
    assert_partition(gpu_cluster(c["xyz"], c["flow"], c["mask"], **kw), want)


def test_cluster_masks():
    c, _ = case_and_oracle("blobs", 2, 257)
    none = gpu_cluster(c["xyz"], c["flow"], torch.zeros_like(c["mask"]), **c["kw"])
    assert (none[0] == -1).all() and (none[1] == 0).all() and (none[2] == 0).all()
    lat, _ = case_and_oracle("chain", 2, 1025)
    everything = torch.ones_like(lat["mask"])
    assert_partition(gpu_cluster(lat["xyz"], lat["flow"], everything, **lat["kw"]),
                     oracle_cluster(lat["xyz"], lat["flow"], everything, **lat["kw"]))


def test_cluster_skips_non_finite_points():
    c, base = case_and_oracle("blobs", 2, 257)
    xyz, flow = c["xyz"].clone(), c["flow"].clone()
    hit = [int(np.nonzero(base[0][b] == 0)[0][k]) for b in range(2) for k in (0, 1, 2)]
    xyz[0, hit[0], 1] = float("nan")
    flow[0, hit[1], 0] = float("inf")
    xyz[1, hit[3], 2] = float("-inf")
    flow[1, hit[4], 2] = float("nan")
    want = oracle_cluster(xyz, flow, c["mask"], **c["kw"])
    assert want[0][0, hit[0]] == -1 and want[1][0, 0] == base[1][0, 0] - 2
    assert_partition(gpu_cluster(xyz, flow, c["mask"], **c["kw"]), want)


# ---------------------------------------------------------------------------
# 2. segmented fit vs oracle
# ---------------------------------------------------------------------------


def seg_sizes():
    return [0, 1, 2, 3, 63, 64, 65, 257, ext_const("SEGMENTED_FIT_CAPACITY", 1024) + 1]


@functools.lru_cache(maxsize=None)
def seg_inputs():
    sizes = seg_sizes()
    B, N = 2, sum(sizes) + 119
    src, dst = rigid_pair(B, N, seed=77, noise=0.005)
    labels = segment_labels(B, N, sizes, seed=5)
    free = np.nonzero(labels[0].numpy() == -1)[0]
    labels[0, free[:3]] = torch.tensor([len(sizes), -9, 2**30], dtype=torch.int32)  # out of range
    rng = np.random.default_rng(8)
    w = torch.from_numpy(rng.random((B, N)) + 0.1).float()
    w[:, ::5] = 0.0
    w[:, 1::31] = -1.5
    w[:, 2::37] = float("nan")
    return src, dst, labels, w, len(sizes)


def check_fit(got, want, ref, scale, label):
    bounds = {}
    for i, (name, sc) in enumerate((("R", 1.0), ("t", scale), ("residual", scale))):
        b = bound(ref[i], want[i], sc)
        e = max_dev(got[i], want[i])
        bounds[name] = b
        print(f"{label} {name}: |kernel - oracle| = {e:.3e}, |ref32 - oracle| = {max_dev(ref[i], want[i]):.3e}, "
              f"bound = {b:.3e}")
        assert e <= b, f"{name} off by {e:.3e} > {b:.3e}"
    assert np.array_equal(got[3].cpu().numpy(), want[3])
    assert got[3].dtype == torch.bool and all(x.dtype == torch.float32 for x in got[:3])
    return bounds


@pytest.mark.parametrize("iters", [0, 10])
@pytest.mark.parametrize("weighted", [False, True], ids=["unweighted", "weighted"])
def test_segmented_fit_matches_oracle(weighted, iters):
    src, dst, labels, w, M = seg_inputs()
    w = w if weighted else None
    want = oracle_object_fits(src, dst, labels, M, w, THRESH, iters)
    ref = R.segmented_rigid_fit(src, dst, labels, M, w, THRESH, iters)  # fp32 on the CPU
    got = ops.segmented_rigid_fit(src.to(dev()), dst.to(dev()), labels.to(dev()), M,
                                  None if w is None else w.to(dev()), THRESH, iters)
    torch.cuda.synchronize()
    assert got[0].shape == (2, M, 3, 3) and got[1].shape == (2, M, 3) and got[2].shape == src.shape[:2]
    check_fit(got, want, ref, coord_scale(src, dst), f"segments iters={iters} weighted={weighted}")
    if not weighted:
        assert got[3].cpu().tolist() == [[s >= 3 for s in seg_sizes()]] * 2
    outside = (labels < 0) | (labels >= M)
    assert torch.isinf(got[2].cpu()[outside]).all() and torch.isfinite(got[2].cpu()[~outside]).all()
    assert torch.equal(got[0].cpu()[:, :3], torch.eye(3).expand(2, 3, 3, 3))


def test_one_segment_agrees_with_rigid_fit():
    src, dst = rigid_pair(2, 300, seed=14, noise=0.005)
    want = oracle_fit(src, dst, None, THRESH, 10)
    ref = R.rigid_fit(src, dst, None, THRESH, 10)
    one = ops.segmented_rigid_fit(src.to(dev()), dst.to(dev()), torch.zeros(2, 300, dtype=torch.int32, device=dev()),
                                  1, None, THRESH, 10)
    plain = ops.rigid_fit(src.to(dev()), dst.to(dev()), None, THRESH, 10)
    torch.cuda.synchronize()
    squeezed = (one[0][:, 0], one[1][:, 0], one[2], one[3][:, 0])
    bounds = check_fit(squeezed, want, ref, coord_scale(src, dst), "one segment")
    for i, name in enumerate(("R", "t", "residual")):
        assert (squeezed[i] - plain[i]).abs().max().item() <= bounds[name]
    assert torch.equal(squeezed[3], plain[3])


# ---------------------------------------------------------------------------
# 3. / 4. determinism, dispatch
# ---------------------------------------------------------------------------


def test_bit_identical_runs():
    c, _ = case_and_oracle("chain", 2, 1025)
    for a, b in zip(gpu_cluster(c["xyz"], c["flow"], c["mask"], **c["kw"]),
                    gpu_cluster(c["xyz"], c["flow"], c["mask"], **c["kw"])):
        assert torch.equal(a, b)
    src, dst, labels, w, M = seg_inputs()
    args = (src.to(dev()), dst.to(dev()), labels.to(dev()), M, w.to(dev()), THRESH, 10)
    for a, b in zip(ops.segmented_rigid_fit(*args), ops.segmented_rigid_fit(*args)):
        assert torch.equal(a, b)
    sc = make_driving_scene(2, 1024, seed=40)
    one = ops.object_motion(sc["pc1"].to(dev()), sc["flow"].to(dev()), **sc["kw"])
    two = ops.object_motion(sc["pc1"].to(dev()), sc["flow"].to(dev()), **sc["kw"])
    for a, b in zip(tuple(one[:-1]) + tuple(one.ego), tuple(two[:-1]) + tuple(two.ego)):
        assert torch.equal(a, b)


def test_reference_dispatch_on_device(monkeypatch):
    c, want = case_and_oracle("blobs", 2, 257)
    src, dst = rigid_pair(2, 257, seed=3, noise=0.005)
    labels = torch.from_numpy(want[0]).int()
    M = c["kw"]["max_objects"]
    fit_want = oracle_object_fits(src, dst, labels, M, None, THRESH, 5)
    fit_ref = R.segmented_rigid_fit(src, dst, labels, M, None, THRESH, 5)
    got = ops.segmented_rigid_fit(src.to(dev()), dst.to(dev()), labels.to(dev()), M, None, THRESH, 5)
    bounds = check_fit(got, fit_want, fit_ref, coord_scale(src, dst), "dispatch")
    monkeypatch.setenv("PVRAFT_REF_OPS", "1")
    ref_part = ops.cluster_points(c["xyz"].to(dev()), c["flow"].to(dev()), c["mask"].to(dev()), **c["kw"])
    ref_fit = ops.segmented_rigid_fit(src.to(dev()), dst.to(dev()), labels.to(dev()), M, None, THRESH, 5)
    monkeypatch.delenv("PVRAFT_REF_OPS")
    assert ref_part[0].is_cuda and ref_fit[0].is_cuda
    assert_partition(ref_part, want)
    for a, b in zip(ref_part, gpu_cluster(c["xyz"], c["flow"], c["mask"], **c["kw"])):
        assert torch.equal(a, b)
    for i, name in enumerate(("R", "t", "residual")):
        fin = torch.isfinite(got[i])
        assert torch.equal(fin, torch.isfinite(ref_fit[i]))
        e = (ref_fit[i][fin] - got[i][fin]).abs().max().item()
        print(f"device reference vs kernel {name}: {e:.3e} (bound {bounds[name]:.3e})")
        assert e <= bounds[name]
    assert torch.equal(ref_fit[3], got[3])


def test_bad_arguments_raise_on_device():
    c, _ = case_and_oracle("blobs", 2, 64)
    x, f, m = c["xyz"].to(dev()), c["flow"].to(dev()), c["mask"].to(dev())
    for kw in ({"min_points": 2}, {"max_objects": 0}, {"max_objects": 257}, {"eps": -1.0}):
        with pytest.raises(ValueError):
            ops.cluster_points(x, f, m, **kw)
    lab = torch.zeros(2, 64, dtype=torch.int32, device=dev())
    for kw in ({"iters": 65}, {"thresh": 0.0}, {"num_segments": 0}):
        args = dict(num_segments=2)
        args.update(kw)
        with pytest.raises(ValueError):
            ops.segmented_rigid_fit(x, x + f, lab, **args)


# ---------------------------------------------------------------------------
# 5. driving scene, 6. Predictor
# ---------------------------------------------------------------------------


def driving_sizes():
    return [2048, ext_const("RIGID_FIT_REG_POINTS", 4096) + 1]


@pytest.mark.parametrize("which", [0, 1], ids=["2048", "reg_points+1"])
def test_object_motion_driving_scene(which):
    N = driving_sizes()[which]
    sc = make_driving_scene(2, N, seed=50 + which)
    om = ops.object_motion(sc["pc1"].to(dev()), sc["flow"].to(dev()), iters=5, **sc["kw"])
    torch.cuda.synchronize()
    assert isinstance(om, ops.ObjectMotion) and (om.num_objects >= 0).all()
    M = sc["kw"]["max_objects"]
    src, dst = sc["pc1"], sc["pc1"] + sc["flow"]
    want = oracle_object_fits(src, dst, sc["labels"], M, None, THRESH, 5)
    ref = R.segmented_rigid_fit(src, dst, sc["labels"], M, None, THRESH, 5)
    scale = coord_scale(src, dst)
    tol = {"R": bound(ref[0], want[0], 1.0), "t": bound(ref[1], want[1], scale),
           "residual": bound(ref[2], want[2], scale)}
    check_driving_scene(sc, om, tol)


def test_predictor_object_motion():
    from pvraft_amd.engine import Predictor
    from pvraft_amd.model import PVRaft

    torch.manual_seed(5)
    model = PVRaft(truncate_k=64).to(dev()).eval()
    pred = Predictor(model, points=256, batch=1, iters=2)
    pc, _ = box_cloud(1, 256, seed=9)
    xyz1 = torch.from_numpy(pc).float().to(dev())
    xyz2 = xyz1 + 0.05 * torch.randn(1, 256, 3, generator=torch.Generator().manual_seed(1)).to(dev())
    flow, om = pred.predict_object_motion(xyz1, xyz2, min_points=3, eps=2.0, flow_eps=float("inf"))
    assert flow.shape == (1, 256, 3) and torch.equal(flow, pred.last_flows[-1])
    want = ops.object_motion(xyz1, flow, min_points=3, eps=2.0, flow_eps=float("inf"))
    assert isinstance(om, ops.ObjectMotion)
    for g, w in zip(tuple(om[:-1]) + tuple(om.ego), tuple(want[:-1]) + tuple(want.ego)):
        assert torch.equal(g, w)
    assert om.labels.shape == (1, 256) and om.R.shape == (1, 32, 3, 3) and (om.num_objects >= 0).all()
