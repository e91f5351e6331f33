"""GPU tests of the fused robust rigid fit (csrc/rigid_fit.hip) and the
layers on it.  Every result is compared with the float64 oracle evaluated on
the CPU; the tolerance is eight times the deviation of the fp32 CPU
reference on the same input, floored at 16 ulp of the data
(ego_cases.bound).  Run with -m gpu."""

import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from ego_cases import (
    EPS32,
    bound,
    box_cloud,
    coord_scale,
    make_scene,
    max_dev,
    oracle_fit,
    rigid_pair,
    rotvec_matrix,
    third_zero_weights,
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


def reg_points():
    from pvraft_amd import _C

    return int(_C.RIGID_FIT_REG_POINTS)


def slot_boundaries():
    """Cloud sizes at which the kernel switches its points-per-lane
    template (1024 lanes x 1, 2, 4, ... slots), below the register limit."""
    out, n = [], 1024
    while n < reg_points():
        out.append(n)
        n *= 2
    return out


def shapes():
    reg = reg_points()
    s = [(1, 3), (1, 4), (2, 63), (2, 64), (3, 65), (2, 257), (1, reg - 1), (1, reg), (1, reg + 1)]
    for n in slot_boundaries():
        for m in (n - 1, n, n + 1):
            if (1, m) not in s:
                s.append((1, m))
    return s


def gpu_fit(src, dst, w=None, thresh=THRESH, iters=0):
    out = ops.rigid_fit(src.to(dev()), dst.to(dev()), None if w is None else w.to(dev()), thresh, iters)
    torch.cuda.synchronize()
    return out


def check_against_oracle(src, dst, w=None, thresh=THRESH, iters=0, compare=("R", "t", "residual"), label=""):
    """Kernel vs oracle within ego_cases.bound for R, t and residual; ok
    must agree.  Returns (kernel outputs, oracle outputs, bounds)."""
    want = oracle_fit(src, dst, w, thresh, iters)
    ref = R.rigid_fit(src, dst, w, thresh, iters)  # fp32 on the CPU
    got = gpu_fit(src, dst, w, thresh, iters)
    scale = coord_scale(src, dst)
    bounds = {}
    for i, (name, sc) in enumerate((("R", 1.0), ("t", scale), ("residual", scale))):
        if name not in compare:
            continue
        b = bound(ref[i], want[i], sc)
        e = max_dev(got[i], want[i])
        bounds[name] = b
        print(f"{label} {name}: |kernel - oracle| = {e:.3e}, |ref32 - oracle| = {max_dev(ref[i], want[i]):.3e}, "
              f"bound = {b:.3e}")
        assert e <= b, f"{name} off by {e:.3e} > {b:.3e}"
    assert np.array_equal(got[3].cpu().numpy(), want[3])
    assert got[0].shape == ref[0].shape and got[1].shape == ref[1].shape and got[2].shape == ref[2].shape
    assert got[3].dtype == torch.bool and all(x.dtype == torch.float32 for x in got[:3])
    return got, want, bounds


# ---------------------------------------------------------------------------
# 1. plain fit on every shape
# ---------------------------------------------------------------------------


def pytest_generate_tests(metafunc):
    if "plain_shape" in metafunc.fixturenames:
        s = shapes() if torch.cuda.is_available() else [(1, 3)]
        metafunc.parametrize("plain_shape", s, ids=[f"{b}x{n}" for b, n in s])


@pytest.mark.parametrize("kind", ["exact", "noisy", "weighted"])
def test_plain_fit(plain_shape, kind):
    B, N = plain_shape
    src, dst = rigid_pair(B, N, seed=10 * N + B, noise=0.0 if kind == "exact" else 0.005)
    w = third_zero_weights(B, N, seed=N) if kind == "weighted" else None
    check_against_oracle(src, dst, w, iters=0, label=f"{kind} {B}x{N}")


# ---------------------------------------------------------------------------
# 2. / 3. large angle, planar (reflection-prone) and collinear clouds
# ---------------------------------------------------------------------------


@pytest.mark.parametrize("planar", [False, True], ids=["170deg", "planar"])
def test_large_angle_and_planar(planar):
    Rt = rotvec_matrix((0.2, -0.4, 0.1)) if planar else rotvec_matrix(np.deg2rad(170) * np.array([0.6, 0.0, 0.8]))
    src, dst = rigid_pair(2, 65, seed=3, R=Rt, planar=planar)
    got, want, bounds = check_against_oracle(src, dst, iters=0, label="planar" if planar else "170deg")
    Rg = got[0].double().cpu()
    assert (torch.linalg.det(Rg) - 1).abs().max().item() <= bounds["R"]
    assert (Rg.transpose(1, 2) @ Rg - torch.eye(3, dtype=torch.float64)).abs().max().item() <= bounds["R"]
    assert np.abs(want[0] - Rt).max() <= 1e-5  # the oracle itself found the motion


def test_collinear_cloud():
    rng = np.random.default_rng(12)
    s = rng.random((2, 64, 1)) * 30.0 - 15.0
    line = np.array([0.0, 0.0, 20.0]) + s * np.array([0.6, 0.1, 0.79])
    Rt = rotvec_matrix((0.01, 0.03, -0.005))
    src = torch.from_numpy(line).float()
    dst = torch.from_numpy(line @ Rt.T + np.array([0.1, -0.05, 1.0])).float()
    # R (and with it t) is not unique on a line: the residuals are compared,
    # R only for being a rotation
    got, _, _ = check_against_oracle(src, dst, iters=0, compare=("residual",), label="collinear")
    Rg = got[0].double().cpu()
    tol = 16 * EPS32
    assert (torch.linalg.det(Rg) - 1).abs().max().item() <= tol
    assert (Rg.transpose(1, 2) @ Rg - torch.eye(3, dtype=torch.float64)).abs().max().item() <= tol
    assert got[3].all()


# ---------------------------------------------------------------------------
# 4. robust fit
# ---------------------------------------------------------------------------


def robust_cases():
    reg = reg_points() if torch.cuda.is_available() else 4096
    return [(2, 64, 0.25, False), (2, 300, 0.3, False), (1, reg + 1, 0.3, False), (1, 2048, 0.3, True)]


@pytest.mark.parametrize("i", range(4))
def test_robust_fit(i):
    B, N, dyn, planar = robust_cases()[i]
    sc = make_scene(B, N, dyn, seed=N + int(100 * dyn), planar=planar)
    src, dst = sc["pc1"], sc["pc1"] + sc["flow"]
    _, want, _ = check_against_oracle(src, dst, None, THRESH, 10, label=f"robust {B}x{N}")
    ego = ops.ego_motion(src.to(dev()), sc["flow"].to(dev()), thresh=THRESH, iters=10)
    near = np.abs(want[2] - THRESH) < 1e-4
    assert near.mean() <= 0.01, "too many points sit on the threshold"
    static = ego.static.cpu().numpy()
    assert np.array_equal(static[~near], (want[2] < THRESH)[~near])
    assert np.array_equal(static, sc["static"].numpy())
    assert ego.ok.all()
    rf = src.to(dev()) @ ego.R.transpose(1, 2) + ego.t.unsqueeze(1) - src.to(dev())
    assert torch.allclose(ego.rigid_flow, rf, atol=1e-6)


# ---------------------------------------------------------------------------
# 5. skipped points, degenerate clouds
# ---------------------------------------------------------------------------


def test_skipped_points():
    src, dst = rigid_pair(2, 300, seed=5, noise=0.005)
    w = third_zero_weights(2, 300, seed=5)
    w[:, 4] = -2.0
    w[:, 5] = float("nan")
    w[:, 6] = float("inf")
    src[:, 7, 1] = float("nan")
    dst[:, 9, 0] = float("inf")
    src[0, 11, 2] = float("-inf")
    dst[:, 4:7] += 5.0  # unweighted points far off the motion
    for iters in (0, 10):
        got, _, _ = check_against_oracle(src, dst, w, THRESH, iters, label=f"skipped iters={iters}")
        res = got[2].cpu()
        assert torch.isinf(res[:, [7, 9]]).all() and (res[:, [7, 9]] > 0).all() and torch.isinf(res[0, 11])
        assert torch.isfinite(res[:, 4:7]).all() and (res[:, 4:7] > 4.0).all()
        assert got[3].all()


def test_degenerate_clouds():
    src, dst = rigid_pair(2, 8, seed=1, noise=0.005)
    eye = torch.eye(3)
    for n in (1, 2):
        got, _, _ = check_against_oracle(src[:, :n].contiguous(), dst[:, :n].contiguous(), iters=3, label=f"N={n}")
        assert not got[3].any() and torch.equal(got[0].cpu(), eye.expand(2, 3, 3))
    got, _, _ = check_against_oracle(src, dst, torch.zeros(2, 8), iters=3, label="zero weights")
    assert not got[3].any() and torch.equal(got[1].cpu(), torch.zeros(2, 3))
    got, _, _ = check_against_oracle(torch.full_like(src, float("nan")), dst, iters=3, label="all NaN")
    assert not got[3].any() and torch.isinf(got[2]).all()
    # two positive weights among many points
    w = torch.zeros(2, 8)
    w[:, [2, 5]] = torch.tensor([3.0, 1.0])
    got, _, _ = check_against_oracle(src, dst, w, iters=3, label="two weights")
    assert not got[3].any()


# ---------------------------------------------------------------------------
# 6. / 7. determinism, dispatch
# ---------------------------------------------------------------------------


@pytest.mark.parametrize("path", ["registers", "streaming"])
def test_bit_identical_runs(path):
    N = 300 if path == "registers" else reg_points() + 1
    sc = make_scene(2, N, 0.3, seed=21)
    w = third_zero_weights(2, N, seed=3)
    a = gpu_fit(sc["pc1"], sc["pc1"] + sc["flow"], w, THRESH, 10)
    b = gpu_fit(sc["pc1"], sc["pc1"] + sc["flow"], w, THRESH, 10)
    for x, y in zip(a, b):
        assert torch.equal(x, y)


def test_reference_dispatch_on_device(monkeypatch):
    sc = make_scene(2, 300, 0.3, seed=330)
    src, dst = sc["pc1"], sc["pc1"] + sc["flow"]
    got, want, bounds = check_against_oracle(src, dst, None, THRESH, 10, label="dispatch")
    monkeypatch.setenv("PVRAFT_REF_OPS", "1")
    ref = ops.rigid_fit(src.to(dev()), dst.to(dev()), None, THRESH, 10)
    monkeypatch.delenv("PVRAFT_REF_OPS")
    assert ref[0].is_cuda
    for i, name in enumerate(("R", "t", "residual")):
        e = (ref[i] - got[i]).abs().max().item()
        print(f"device reference vs kernel {name}: {e:.3e} (bound {bounds[name]:.3e})")
        assert e <= bounds[name]
    assert torch.equal(ref[3], got[3])


def test_bad_arguments_raise_on_device():
    src, dst = rigid_pair(1, 10, seed=2)
    for kw in ({"iters": -1}, {"iters": 65}, {"thresh": 0.0}):
        with pytest.raises(ValueError):
            ops.rigid_fit(src.to(dev()), dst.to(dev()), **kw)


# ---------------------------------------------------------------------------
# 8. Predictor
# ---------------------------------------------------------------------------


def test_predictor_ego_motion():
    from pvraft_amd.engine import Predictor
    from pvraft_amd.model import PVRaft

    torch.manual_seed(5)
    model = PVRaft(truncate_k=64).to(dev()).eval()
    pred = Predictor(model, points=256, batch=1, iters=2)
    pc, _ = box_cloud(1, 256, seed=9)
    xyz1 = torch.from_numpy(pc).float().to(dev())
    xyz2 = xyz1 + 0.05 * torch.randn(1, 256, 3, generator=torch.Generator().manual_seed(1)).to(dev())
    flow, ego = pred.predict_ego_motion(xyz1, xyz2, thresh=0.05, iters=10)
    # the flow returned is the one this forward produced, bit for bit ...
    assert flow.shape == (1, 256, 3) and torch.equal(flow, pred.last_flows[-1])
    # ... and a second forward of the model agrees with it to rounding (the
    # model's forward is not bit-identical run to run)
    again = pred(xyz1, xyz2)
    assert (flow - again).abs().max().item() <= 1e-4
    want = ops.ego_motion(xyz1, flow, thresh=0.05, iters=10)
    assert isinstance(ego, ops.EgoMotion)
    for g, w in zip(ego, want):
        assert torch.equal(g, w)
    assert ego.R.shape == (1, 3, 3) and ego.static.shape == (1, 256) and ego.ok.all()
