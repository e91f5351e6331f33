"""GPU tests of the fused ground-plane fit (csrc/plane_fit.hip) and the
layers on it.  Every result is compared with the numpy oracle of
ground_cases evaluated on the CPU: hypotheses and counts bit-equal, the plane
and the heights within eight times the deviation of the fp32 CPU reference
on the same input, floored at 16 ulp of the data (ground_cases.bound), the
labels equal outside the near set.  Run with -m gpu."""

import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import ground_cases as gc

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    import pvraft_amd.ops as ops

HYPOTHESES = (1, 63, 64, 65, 256, 257)


@pytest.fixture(scope="module", autouse=True)
def _require_gpu_and_ext():
    if not torch.cuda.is_available():
        pytest.skip("needs GPU")
    import pvraft_amd.ops as ops

    assert ops.hip_available(), "HIP extension must be built on the GPU box"


def dev():
    return torch.device("cuda:0")


def tile():
    from pvraft_amd import _C

    assert int(_C.PLANE_SCORE_BLOCK) >= 64
    return int(_C.PLANE_SCORE_TILE)


def shapes():
    from pvraft_amd import _C

    t = tile()
    r = int(_C.PLANE_REFINE_BLOCK)  # lanes that stride over the points in a refinement round
    s = [(1, 3), (1, 4), (2, 63), (2, 64), (3, 65), (2, 257)]
    for n in (t - 1, t, t + 1, r - 1, r, r + 1):
        if n not in [m for _, m in s]:
            s.append((1, n))
    s.append((1, min(64 * t + 1, 16385)))  # many tiles, one point into the last
    return s


def pytest_generate_tests(metafunc):
    if "shape" in metafunc.fixturenames:
        s = shapes() if torch.cuda.is_available() else [(1, 3)]
        metafunc.parametrize("shape", s, ids=[f"{b}x{n}" for b, n in s])


_SCENES = {}


def scene(B, N):
    """One scene per shape, generated once and never modified."""
    if (B, N) not in _SCENES:
        _SCENES[(B, N)] = gc.make_scene(B, N, seed=7 * N + B)["xyz"]
    return _SCENES[(B, N)]


def gpu_fit(x, mask=None, **kw):
    out = ops.fit_plane(x.to(dev()), None if mask is None else mask.to(dev()), **kw)
    torch.cuda.synchronize()
    return out


def check_against_oracle(x, mask=None, label="", **kw):
    """plane_hypotheses bit-equal, fit_plane within ground_cases.check_fit."""
    m = None if mask is None else mask.numpy()
    hyp_kw = {k: v for k, v in kw.items() if k != "refine_iters"}
    want = gc.oracle_fit(x, mask=m, **kw)
    idx, count = ops.plane_hypotheses(x.to(dev()), None if mask is None else mask.to(dev()), **hyp_kw)
    assert idx.dtype == torch.int32 and count.dtype == torch.int32 and idx.is_cuda
    assert np.array_equal(idx.cpu().numpy(), want["idx"]), f"{label}: idx differs"
    assert np.array_equal(count.cpu().numpy(), want["hyp_count"]), f"{label}: count differs"
    ref = ops.fit_plane(x, mask, **kw)  # fp32 reference on the CPU
    got = gpu_fit(x, mask, **kw)
    assert isinstance(got, ops.PlaneFit) and got.height.is_cuda
    assert all(g.shape == r.shape and g.dtype == r.dtype for g, r in zip(got, ref))
    gc.check_fit(got, want, ref=ref, scale=gc.coord_scale(x), label=label)
    return got, want


# ---------------------------------------------------------------------------
# 1. every shape x every hypothesis count
# ---------------------------------------------------------------------------


@pytest.mark.parametrize("hyp", HYPOTHESES)
def test_fit_matches_oracle(shape, hyp):
    B, N = shape
    check_against_oracle(scene(B, N), hypotheses=hyp, label=f"{B}x{N} H={hyp}")


@pytest.mark.parametrize("iters", [0, 1, 16])
def test_refinement_rounds(iters):
    got, want = check_against_oracle(scene(2, 257), refine_iters=iters, label=f"iters={iters}")
    assert (got.rounds.cpu() <= iters).all()


def test_other_up_seed_thresh_and_tilt():
    x = scene(2, 257)[..., [0, 2, 1]].contiguous()  # z up
    check_against_oracle(x, up=(0.0, 0.0, 3.0), seed=12345, thresh=0.15, max_tilt_deg=12.0, label="z up")


def test_wall_larger_than_ground():
    sc = gc.make_scene(1, 1000, seed=11, ground=0.3, wall=0.5)
    got, _ = check_against_oracle(sc["xyz"], label="wall")
    assert gc.angle_deg(got.normal.cpu().numpy(), sc["normal"]).max() <= 0.1


# ---------------------------------------------------------------------------
# 2. masks, non-finite points, degenerate inputs
# ---------------------------------------------------------------------------


def test_mask_and_non_finite_points():
    sc = gc.make_scene(2, 300, seed=8)
    x = sc["xyz"].clone()
    x[:, 5, 0] = float("nan")
    x[:, 17, 1] = float("inf")
    x[0, 40, 2] = float("-inf")
    x[:, 100:160] = float("nan")
    got, _ = check_against_oracle(x, label="non-finite")
    bad = ~torch.isfinite(x).all(-1)
    h = got.height.cpu()
    assert (h[bad] == float("inf")).all() and torch.isfinite(h[~bad]).all()
    assert not got.ground.cpu()[bad].any() and not got.inlier.cpu()[bad].any()
    # fitting only what is not ground: the next valid plane, heights for all
    mask = ~sc["is_ground"]
    got, _ = check_against_oracle(x, mask=mask, label="masked")
    assert torch.isfinite(got.height.cpu()[~bad]).all()
    idx, _ = ops.plane_hypotheses(x.to(dev()), mask.to(dev()))
    idx = idx.cpu()
    for b in range(2):
        drawn = idx[b][idx[b] >= 0].long()
        assert mask[b][drawn].all() and not bad[b][drawn].any()


def test_degenerate_inputs():
    sc = gc.make_scene(2, 50, seed=2)["xyz"]
    cases = [
        ("N=1", sc[:, :1].contiguous(), None),
        ("N=2", sc[:, :2].contiguous(), None),
        ("all NaN", torch.full_like(sc, float("nan")), None),
        ("all masked", sc, torch.zeros(2, 50, dtype=torch.bool)),
        ("vertical", gc.vertical_cloud(2, 50, seed=4), None),
    ]
    for label, x, m in cases:
        got, want = check_against_oracle(x, mask=m, label=label)
        B, N = x.shape[:2]
        assert not want["ok"].any() and not got.ok.any()
        assert torch.equal(got.normal.cpu(), torch.tensor([0.0, 1.0, 0.0]).expand(B, 3))
        assert torch.equal(got.offset.cpu(), torch.zeros(B))
        assert (got.height == float("inf")).all() and not got.ground.any() and not got.inlier.any()
        assert (got.count == 0).all() and (got.best == -1).all() and (got.rounds == 0).all()


def test_collinear_inliers_accept_no_round():
    x = gc.collinear_cloud(2, 200, seed=6)
    got, want = check_against_oracle(x, label="collinear")
    assert want["ok"].all() and got.ok.all() and (got.rounds == 0).all()


# ---------------------------------------------------------------------------
# 3. determinism, dispatch, arguments
# ---------------------------------------------------------------------------


def test_bit_identical_runs():
    x = scene(1, min(64 * tile() + 1, 16385))
    m = torch.rand(x.shape[:2], generator=torch.Generator().manual_seed(3)) > 0.2
    a = gpu_fit(x, m, refine_iters=5)
    b = gpu_fit(x, m, refine_iters=5)
    for u, v in zip(a, b):
        assert torch.equal(u, v)
    assert a.ok.all() and (a.rounds > 0).all()


def test_reference_dispatch_on_device(monkeypatch):
    x = scene(2, 257)
    got, want = check_against_oracle(x, label="dispatch")
    monkeypatch.setenv("PVRAFT_REF_OPS", "1")
    ref = ops.fit_plane(x.to(dev()))
    ri, rc = ops.plane_hypotheses(x.to(dev()))
    monkeypatch.delenv("PVRAFT_REF_OPS")
    assert ref.height.is_cuda and ri.is_cuda
    assert np.array_equal(ri.cpu().numpy(), want["idx"]) and np.array_equal(rc.cpu().numpy(), want["hyp_count"])
    gc.check_fit(ref, want, scale=gc.coord_scale(x), label="device reference")
    for name in ("best", "count", "rounds", "ok"):
        assert torch.equal(getattr(ref, name), getattr(got, name))


def test_bad_arguments_raise_on_device():
    x = scene(1, 4).to(dev())
    for kw in ({"hypotheses": 0}, {"hypotheses": 4097}, {"refine_iters": -1}, {"refine_iters": 17},
               {"max_tilt_deg": 0.0}, {"max_tilt_deg": 90.0}, {"thresh": 0.0}, {"thresh": float("nan")},
               {"up": (0.0, 0.0, 0.0)}, {"up": (0.0, float("inf"), 0.0)}):
        with pytest.raises(ValueError):
            ops.fit_plane(x, **kw)
    with pytest.raises(ValueError):
        ops.fit_plane(x[0])
    with pytest.raises(ValueError):
        ops.fit_plane(x, mask=torch.ones(1, 3, dtype=torch.bool, device=dev()))


def test_largest_hypothesis_count():
    check_against_oracle(scene(2, 63), hypotheses=4096, label="H=4096")


# ---------------------------------------------------------------------------
# 4. Predictor
# ---------------------------------------------------------------------------


def test_predictor_remove_ground():
    from pvraft_amd.engine import Predictor
    from pvraft_amd.model import PVRaft

    torch.manual_seed(5)
    model = PVRaft(truncate_k=64).to(dev()).eval()
    pred = Predictor(model, points=256, batch=1, iters=2)
    sc = gc.make_scene(1, 1024, seed=21, ground=0.4)
    pc1 = sc["xyz"][0].to(dev())
    pc2 = pc1 + torch.tensor([0.05, 0.0, 0.3], device=dev())

    def gen():
        return torch.Generator().manual_seed(9)

    # the default call: what it returned before the option existed
    dense0, idx0, sub0 = pred.predict_dense(pc1, pc2, generator=gen(), return_sparse=True)
    g = gen()
    want_idx = torch.randperm(1024, generator=g)[:256]
    assert torch.equal(idx0.cpu(), want_idx) and dense0.shape == (1024, 3)
    out = pred.predict_dense(pc1, pc2, generator=gen(), return_sparse=True, remove_ground=False)
    assert len(out) == 3 and torch.equal(out[1], idx0)

    dense, idx, sub, ground = pred.predict_dense(pc1, pc2, generator=gen(), return_sparse=True, remove_ground=True)
    fit = ops.fit_plane(pc1.unsqueeze(0))
    assert ground.shape == (1024,) and ground.dtype == torch.bool and torch.equal(ground, fit.ground[0])
    assert abs(ground.float().mean().item() - 0.41) < 0.03  # 40 % ground, 1 % below it
    assert idx.shape == (256,) and not ground[idx].any() and idx.unique().numel() == 256
    assert dense.shape == (1024, 3) and torch.isfinite(dense).all() and sub.shape == (256, 3)
    # seeded generator: the same samples (the forward itself is not
    # bit-identical run to run, so the flow is compared to rounding)
    dense2, idx2, _, ground2 = pred.predict_dense(pc1, pc2, generator=gen(), return_sparse=True, remove_ground=True)
    assert torch.equal(idx, idx2) and torch.equal(ground, ground2)
    assert (dense - dense2).abs().max().item() <= 1e-4
    assert pred.predict_dense(pc1, pc2, generator=gen(), remove_ground=True).shape == (1024, 3)
    # keyword arguments reach the fit
    _, _, _, gk = pred.predict_dense(pc1, pc2, generator=gen(), return_sparse=True, remove_ground=True,
                                     ground_kw={"thresh": 0.1, "seed": 3})
    assert torch.equal(gk, ops.fit_plane(pc1.unsqueeze(0), thresh=0.1, seed=3).ground[0])
    with pytest.raises(ValueError):
        big = Predictor(model, points=700, batch=1, iters=2, use_graph=False)
        big.predict_dense(pc1, pc2, remove_ground=True)
