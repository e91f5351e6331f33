"""CPU tests of the ground-plane fit: the numpy oracle of ground_cases must
find the true plane by itself, ops.reference (reached through ops.fit_plane
on CPU tensors) must agree with the oracle, and the documented edge cases
hold.  The loader options that belong to the feature are tested here too."""

import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import ground_cases as gc

import pvraft_amd.ops as ops


@pytest.fixture(scope="module")
def scenes():
    """One scene and one oracle fit per size, shared by the tests below."""
    out = {}
    for n in gc.FIND_SIZES:
        sc = gc.make_scene(2, n, seed=n)
        out[n] = (sc, gc.oracle_fit(sc["xyz"]))
    return out


@pytest.mark.parametrize("n", gc.FIND_SIZES)
def test_oracle_finds_the_plane(scenes, n):
    sc, want = scenes[n]
    ang = gc.angle_deg(want["normal"], sc["normal"])
    off = np.abs(want["offset"] - sc["offset"])
    print(f"N={n}: angle {ang.max():.4f} deg, offset error {off.max() * 1e3:.2f} mm, rounds {want['rounds']}")
    assert want["ok"].all()
    assert (ang <= 0.1).all() and (off <= 0.02).all()
    assert (want["normal"] @ np.array([0.0, 1.0, 0.0]) > 0).all()
    near = gc.near_set(want["height"])
    assert near.mean() <= 0.01
    # the ground label covers the generated ground and the points below it
    truth = sc["is_ground"].numpy()
    assert (want["ground"][truth].mean() > 0.99) and want["inlier"][truth].mean() > 0.99


@pytest.mark.parametrize("n", gc.FIND_SIZES)
def test_reference_matches_oracle(scenes, n):
    sc, want = scenes[n]
    idx, count = ops.plane_hypotheses(sc["xyz"])
    assert idx.dtype == torch.int32 and count.dtype == torch.int32
    assert np.array_equal(idx.numpy(), want["idx"])
    assert np.array_equal(count.numpy(), want["hyp_count"])
    got = ops.fit_plane(sc["xyz"])
    assert isinstance(got, ops.PlaneFit)
    gc.check_fit(got, want, scale=gc.coord_scale(sc["xyz"]), label=f"N={n}")
    assert got.height.shape == (2, n) and got.normal.shape == (2, 3) and got.offset.shape == (2,)
    # the plane equation reproduces the heights
    h = (sc["xyz"].double() @ got.normal.double().unsqueeze(-1)).squeeze(-1) + got.offset.double().unsqueeze(1)
    assert (h - got.height.double()).abs().max().item() <= 1e-4


def test_ties_go_to_the_smallest_hypothesis(scenes):
    for n in (64, 300):
        _, want = scenes[n]
        for b in range(2):
            c = want["hyp_count"][b]
            assert want["best"][b] == np.nonzero(c == c.max())[0][0]
    # a tie at the top itself is needed to tell argmax conventions apart
    # (a noise-free level ground: many triples count exactly the same inliers)
    sc = gc.make_scene(1, 64, seed=5, ground=0.5)
    x = sc["xyz"].clone()
    x[0, :, 1] = torch.where(sc["is_ground"][0], torch.tensor(-1.4), x[0, :, 1])
    want = gc.oracle_fit(x, refine_iters=0)
    c = want["hyp_count"][0]
    assert (c == c.max()).sum() > 1, "this input is meant to produce a tie at the top"
    got = ops.fit_plane(x, refine_iters=0)
    assert int(got.best[0]) == int(np.nonzero(c == c.max())[0][0]) == int(want["best"][0])


def test_wall_larger_than_ground():
    sc = gc.make_scene(1, 1000, seed=11, ground=0.3, wall=0.5)
    want = gc.oracle_fit(sc["xyz"])
    got = ops.fit_plane(sc["xyz"])
    gc.check_fit(got, want, scale=gc.coord_scale(sc["xyz"]), label="wall")
    assert gc.angle_deg(got.normal.numpy(), sc["normal"]).max() <= 0.1
    # the wall is the larger plane: only the tilt limit keeps it from winning
    wall = ops.fit_plane(sc["xyz"], up=(1.0, 0.0, 0.0))
    assert gc.angle_deg(wall.normal.numpy(), np.array([1.0, 0.0, 0.0])).max() <= 0.1
    assert int(wall.count[0]) > int(got.count[0])


def test_mask_excludes_the_ground():
    sc = gc.make_scene(1, 600, seed=3, ground=0.4, wall=0.0)
    mask = ~sc["is_ground"]
    want = gc.oracle_fit(sc["xyz"], mask=mask.numpy())
    got = ops.fit_plane(sc["xyz"], mask=mask)
    gc.check_fit(got, want, scale=gc.coord_scale(sc["xyz"]), label="mask")
    # whatever plane was found, it was not fitted to the ground ...
    full = ops.fit_plane(sc["xyz"])
    assert int(got.count[0]) < int(full.count[0])
    # ... and unmasked points still get heights and labels
    assert torch.isfinite(got.height).all()
    i, _ = ops.plane_hypotheses(sc["xyz"], mask=mask)
    drawn = i[i >= 0].long()
    assert mask[0][drawn].all()
    # a mask that leaves two points: no plane
    m2 = torch.zeros_like(mask)
    m2[0, :2] = True
    none = ops.fit_plane(sc["xyz"], mask=m2)
    assert not none.ok.any()


def test_non_finite_points():
    sc = gc.make_scene(2, 300, seed=8)
    x = sc["xyz"].clone()
    x[:, 5, 0] = float("nan")
    x[:, 17, 1] = float("inf")
    x[0, 40, 2] = float("-inf")
    x[:, 100:160] = float("nan")
    want = gc.oracle_fit(x)
    got = ops.fit_plane(x)
    gc.check_fit(got, want, scale=gc.coord_scale(x), label="non-finite")
    bad = ~torch.isfinite(x).all(-1)
    assert (got.height[bad] == float("inf")).all()
    assert not got.ground[bad].any() and not got.inlier[bad].any()
    assert torch.isfinite(got.height[~bad]).all()
    idx, _ = ops.plane_hypotheses(x)
    for b in range(2):
        drawn = idx[b][idx[b] >= 0].long()
        assert not bad[b][drawn].any()


def _assert_not_ok(got, B, N, up=(0.0, 1.0, 0.0)):
    assert not got.ok.any()
    assert torch.equal(got.normal.cpu(), torch.tensor(up).expand(B, 3))
    assert torch.equal(got.offset.cpu(), torch.zeros(B))
    assert (got.height == float("inf")).all() and got.height.shape == (B, N)
    assert not got.ground.any() and not got.inlier.any()
    assert (got.count == 0).all() and (got.best == -1).all() and (got.rounds == 0).all()


def degenerate_inputs():
    sc = gc.make_scene(2, 50, seed=2)["xyz"]
    yield "N=1", sc[:, :1].contiguous(), None
    yield "N=2", sc[:, :2].contiguous(), None
    yield "all NaN", torch.full_like(sc, float("nan")), None
    yield "all masked", sc, torch.zeros(2, 50, dtype=torch.bool)
    yield "vertical", gc.vertical_cloud(2, 50, seed=4), None


def test_degenerate_inputs():
    for label, x, m in degenerate_inputs():
        got = ops.fit_plane(x, mask=m)
        _assert_not_ok(got, x.shape[0], x.shape[1])
        idx, count = ops.plane_hypotheses(x, mask=m)
        assert (idx == -1).all() and (count == -1).all(), label
        want = gc.oracle_fit(x, mask=None if m is None else m.numpy())
        assert not want["ok"].any(), label


def test_collinear_inliers_accept_no_round():
    x = gc.collinear_cloud(2, 200, seed=6)
    want = gc.oracle_fit(x)
    assert want["ok"].all(), "the collinear case is meant to have valid hypotheses"
    got = ops.fit_plane(x)
    assert got.ok.all() and (got.rounds == 0).all() and (want["rounds"] == 0).all()
    assert np.array_equal(got.best.numpy(), want["best"])
    assert np.array_equal(got.count.numpy(), want["count"])


def test_seeds_and_batch_elements():
    sc = gc.make_scene(1, 300, seed=1)
    x = sc["xyz"].expand(2, 300, 3).contiguous()  # two identical clouds
    a, ca = ops.plane_hypotheses(x, seed=7)
    b, cb = ops.plane_hypotheses(x, seed=7)
    assert torch.equal(a, b) and torch.equal(ca, cb)
    c, _ = ops.plane_hypotheses(x, seed=8)
    assert not torch.equal(a, c)
    assert not torch.equal(a[0], a[1])
    # seeds are taken modulo 2^32
    d, _ = ops.plane_hypotheses(x, seed=7 + (1 << 32))
    assert torch.equal(a, d)
    want_i, _ = gc.oracle_hypotheses(x, seed=7)
    assert np.array_equal(a.numpy(), want_i)


def test_other_up_axis():
    sc = gc.make_scene(1, 400, seed=12)
    x = sc["xyz"][..., [0, 2, 1]].contiguous()  # z up
    want = gc.oracle_fit(x, up=(0, 0, 2.0))
    got = ops.fit_plane(x, up=(0, 0, 2.0))
    gc.check_fit(got, want, scale=gc.coord_scale(x), label="z up")
    assert gc.angle_deg(got.normal.numpy(), sc["normal"][[0, 2, 1]]).max() <= 0.1
    y_up = ops.fit_plane(x)
    assert gc.angle_deg(y_up.normal.numpy(), sc["normal"][[0, 2, 1]]).max() > 45 or not y_up.ok.all()


BAD_ARGS = [
    {"hypotheses": 0}, {"hypotheses": 4097}, {"refine_iters": -1}, {"refine_iters": 17},
    {"max_tilt_deg": 0.0}, {"max_tilt_deg": 90.0}, {"max_tilt_deg": float("nan")},
    {"thresh": 0.0}, {"thresh": -1.0}, {"thresh": float("nan")}, {"thresh": float("inf")},
    {"up": (0.0, 0.0, 0.0)}, {"up": (0.0, float("nan"), 1.0)}, {"up": (0.0, float("inf"), 0.0)}, {"up": (1.0, 0.0)},
]


@pytest.mark.parametrize("kw", BAD_ARGS, ids=[str(k) for k in BAD_ARGS])
def test_bad_arguments(kw):
    x = gc.make_scene(1, 20, seed=0)["xyz"]
    with pytest.raises(ValueError):
        ops.fit_plane(x, **kw)
    if "refine_iters" not in kw:
        with pytest.raises(ValueError):
            ops.plane_hypotheses(x, **kw)


def test_bad_shapes():
    x = gc.make_scene(1, 20, seed=0)["xyz"]
    with pytest.raises(ValueError):
        ops.fit_plane(x[0])
    with pytest.raises(ValueError):
        ops.fit_plane(x, mask=torch.ones(1, 19, dtype=torch.bool))


# ---------------------------------------------------------------------------
# loaders
# ---------------------------------------------------------------------------


def test_synthetic_ground_fraction():
    from pvraft_amd.data import SyntheticSceneFlow

    a = SyntheticSceneFlow(nb_points=512, length=4, seed=3)
    b = SyntheticSceneFlow(nb_points=512, length=4, seed=3, ground_fraction=0.0)
    g = SyntheticSceneFlow(nb_points=512, length=4, seed=3, ground_fraction=0.3)
    for i in range(2):
        (sa, ga), (sb, gb), (sg, gg) = a.load_sequence(i), b.load_sequence(i), g.load_sequence(i)
        for x, y in zip(sa + ga, sb + gb):
            assert np.array_equal(x, y)
        pc1 = torch.from_numpy(sg[0])
        on = (pc1[:, 1] + 1.4).abs() < 0.1
        assert abs(on.float().mean().item() - 0.3) < 0.03
        # the ground follows the rigid motion: its flow is as smooth as the rest
        assert np.abs(gg[1] - (sg[1] - sg[0])).max() == 0 and np.abs(gg[1]).max() < 5
        fit = ops.fit_plane(pc1.unsqueeze(0))
        assert fit.ok.all() and abs(fit.inlier.float().mean().item() - 0.3) < 0.05
        assert gc.angle_deg(fit.normal.numpy(), np.array([0.0, 1.0, 0.0])).max() < 0.5
    with pytest.raises(ValueError):
        SyntheticSceneFlow(nb_points=128, length=4, ground_fraction=1.0)


# pc1.sum(), pc2.sum(), pc1[0, 0], pc2[-1, 2] of sample 0 of the default
# stream (nb_points = 8, seed = 0) as generated before ground_fraction existed
SYNTH_PINNED = [5.079913854598999, -10.08553458750248, 3.506242036819458, -5.580636024475098]


def test_synthetic_default_stream_pinned():
    """Any extra random draw in the default path would move these numbers."""
    from pvraft_amd.data import SyntheticSceneFlow

    (pc1, pc2), _ = SyntheticSceneFlow(nb_points=8, length=2, seed=0).load_sequence(0)
    got = [float(pc1.astype(np.float64).sum()), float(pc2.astype(np.float64).sum()), float(pc1[0, 0]),
           float(pc2[-1, 2])]
    assert got == pytest.approx(SYNTH_PINNED, abs=1e-6)


def test_kitti_keep_ground(tmp_path):
    from pvraft_amd.data import Kitti
    from pvraft_amd.data.base import SceneFlowDataset

    scene = tmp_path / "kitti" / "000000"
    scene.mkdir(parents=True)
    rng = np.random.default_rng(0)
    pc1 = rng.uniform(-3, 3, size=(400, 3)).astype(np.float32)
    pc1[:, 2] = rng.uniform(1, 30, size=400)
    pc2 = pc1 + np.float32(0.01)
    np.save(scene / "pc1.npy", pc1)
    np.save(scene / "pc2.npy", pc2)
    assert SceneFlowDataset.keep_ground is False and Kitti.keep_ground is False
    ds = Kitti(str(tmp_path / "kitti"), nb_points=64, mapping_file="", strict_sizes=False)
    is_ground = (pc1[:, 1] < -1.4) & (pc2[:, 1] < -1.4)
    assert 0 < is_ground.sum() < 400
    (a, _), (mask, flow) = ds.load_sequence(0)
    assert np.array_equal(a, pc1[~is_ground]) and flow.shape == a.shape and mask.shape == (a.shape[0], 1)
    ds.keep_ground = True
    (k, k2), (mask, flow) = ds.load_sequence(0)
    assert np.array_equal(k, pc1) and np.array_equal(k2, pc2) and flow.shape == pc1.shape
    assert Kitti.keep_ground is False  # set on the instance only
