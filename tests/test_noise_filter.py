"""CPU tests of ``ops.noise_filter`` (the torch reference behind the CPU
dispatch), compared with the numpy oracle of noise_cases: count, mean_dist and
ok bit for bit, the statistics within 1e-9 * radius, keep exactly.  Also the
layers above: ``Predictor.predict_dense(remove_noise=)``, the synthetic
dataset's ``noise_fraction`` and the filter's effect on the voxel sample."""

import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import noise_cases as nc
import pvraft_amd.ops as ops

SHAPES = [(1, 1), (1, 2), (2, 63), (2, 64), (3, 65), (1, 255), (1, 256), (1, 257), (1, 511), (1, 512), (1, 513)]


def run(x, mask=None, **kw):
    out = ops.noise_filter(x, mask=mask, **kw)
    assert isinstance(out, ops.NoiseFilter)
    return nc.as_numpy(out)


def full_check(key, x, mask=None, radius=0.5, min_neighbors=4, k=8, std_ratio=2.0):
    want = nc.scene_oracle(key, x, radius, min_neighbors, k, std_ratio, mask)
    got = run(x, mask, radius=radius, min_neighbors=min_neighbors, k=k, std_ratio=std_ratio)
    nc.check(got, want, radius, min_neighbors, k, str(key))
    return want


@pytest.mark.parametrize("shape", SHAPES, ids=[f"{b}x{n}" for b, n in SHAPES])
def test_matches_oracle(shape):
    B, N = shape
    want = full_check(("scene", B, N), nc.scene(B, N, seed=7 * N + B))
    if N >= 63:
        assert want["keep"].any() and want["sparse"].any() and want["far"].any()


def test_more_rows_than_one_chunk():
    from pvraft_amd.ops import reference

    n = 2049
    assert reference.NOISE_PAIR_BUDGET // n < n  # the reference takes several row chunks
    full_check(("scene", 1, n), nc.scene(1, n, seed=5))


def test_coincident_points():
    x = nc.coincident(1025)
    want = nc.oracle(x, k=16)
    assert (want["count"] == 1024).all() and (want["mean_dist"] == 0).all()
    got = run(x, k=16)
    nc.check_exact(got, want, "coincident")
    nc.check_sparse(got, want, 4, "coincident")


def test_lattice_ties_at_the_radius():
    x = nc.lattice(6, 0.5)  # d2 == r2 for the six axis neighbours
    for k in (0, 6, 8):
        want = nc.oracle(x, k=k)
        assert want["count"].max() == 6 and want["count"].min() == 3
        if k == 6:
            inner = want["count"] == 6
            assert (want["mean_dist"][inner] == 0.5).all() and np.isinf(want["mean_dist"][~inner]).all()
        got = run(x, k=k)
        nc.check_exact(got, want, f"lattice k={k}")
        nc.check_sparse(got, want, 4, f"lattice k={k}")
    up = nc.lattice(6, np.nextafter(np.float32(0.5), np.float32(1)))
    want = nc.oracle(up, k=0)
    assert (want["count"] == 0).all()
    got = run(up, k=0)
    nc.check(got, want, 0.5, 4, 0, "lattice one ulp above the radius")


def test_negative_coordinates_and_cell_faces():
    full_check(("negative", 1000), nc.negative(1000, seed=2))
    x = nc.faces(1000, seed=3)
    full_check(("faces", 1000), x)
    el, c = nc.cells(x[0].numpy(), 0.5)
    assert (c < 0).any() and (c >= 0).any() and (x[0] == 0).any() and (x[0, :, 1] == -0.5).any()


def test_stencil_condition_decides():
    x = nc.stencil_edges()
    want = full_check(("stencil",), x, radius=nc.STENCIL_RADIUS, min_neighbors=1, k=2)
    # the pair count is below the plain radius rule's
    p = x[0].numpy()
    d = p[:, None, :] - p[None, :, :]
    d2 = (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]
    r2 = np.float32(nc.STENCIL_RADIUS) * np.float32(nc.STENCIL_RADIUS)
    assert int(want["count"].sum()) < int((d2 <= r2).sum()) - len(p)


@pytest.mark.parametrize("k", [0, 1, 8, 16])
def test_k_and_counts_at_k(k):
    x = nc.exact_k(k, seed=3)
    want = nc.oracle(x, k=k, min_neighbors=0)
    counts = set(want["count"][0].tolist())
    assert {max(k - 1, 0), k, k + 1} <= counts
    if k >= 1:
        assert np.isinf(want["mean_dist"][want["count"] < k]).all() and np.isfinite(want["mean_dist"][want["count"] >= k]).all()
        assert not want["keep"][want["count"] < k].any()
    else:
        assert np.isinf(want["mean_dist"]).all() and want["keep"].all() and want["threshold"][0] == 0.0
    got = run(x, k=k, min_neighbors=0)
    nc.check(got, want, 0.5, 0, k, f"k={k}")
    full_check(("scene", 3, 65), nc.scene(3, 65, seed=7 * 65 + 3), k=k, min_neighbors=0)


def test_mask_removes_neighbours_and_judgement():
    x = nc.scene(2, 300, seed=9)
    mask = torch.rand(2, 300, generator=torch.Generator().manual_seed(3)) > 0.3
    want = full_check(("masked", 2, 300), x, mask=mask)
    m = mask.numpy()
    assert (want["count"][~m] == -1).all() and not want["keep"][~m].any() and np.isinf(want["mean_dist"][~m]).all()
    # the masked cloud equals the compacted cloud
    for b in range(2):
        sub = nc.oracle(x[b:b + 1, mask[b]])
        assert np.array_equal(sub["count"][0], want["count"][b][m[b]])
    none = run(x, torch.zeros(2, 300, dtype=torch.bool))
    assert (none["count"] == -1).all() and not none["keep"].any() and (none["threshold"] == 0).all() and none["ok"].all()


def test_non_finite_and_out_of_range_rows():
    x = nc.dirty(2, 300, seed=4)
    want = full_check(("dirty", 2, 300), x)
    assert (want["count"][:, nc.BAD_ROWS] == -1).all() and not want["keep"][:, nc.BAD_ROWS].any()
    assert (want["count"][:, 2] >= 1).all()  # the duplicate row


def test_clouds_do_not_see_each_other():
    x = nc.scene(3, 65, seed=7 * 65 + 3)
    want = nc.scene_oracle(("scene", 3, 65), x)
    for b in range(3):
        one = run(x[b:b + 1])
        assert np.array_equal(one["count"][0], want["count"][b])
        assert np.array_equal(nc.bits(one["mean_dist"][0]), nc.bits(want["mean_dist"][b]))
    same = run(x[:1].expand(3, 65, 3))
    assert np.array_equal(same["count"][0], same["count"][1]) and np.array_equal(same["keep"][0], same["keep"][2])


def test_permutation_equivariance_and_symmetry():
    x = nc.scene(1, 513, seed=7 * 513 + 1)
    want = nc.scene_oracle(("scene", 1, 513), x)
    perm = torch.randperm(513, generator=torch.Generator().manual_seed(1))
    got = run(x[:, perm])
    p = perm.numpy()
    assert np.array_equal(got["count"][0], want["count"][0][p])
    assert np.array_equal(nc.bits(got["mean_dist"][0]), nc.bits(want["mean_dist"][0][p]))
    assert np.array_equal(got["keep"][0], want["keep"][0][p])
    total = int(got["count"][got["count"] >= 0].sum())
    assert total % 2 == 0 and total == int(want["count"][want["count"] >= 0].sum())


def test_input_conversion_and_empty_shapes():
    x = nc.scene(2, 64, seed=7 * 64 + 2)
    want = nc.scene_oracle(("scene", 2, 64), x)
    xt = x.transpose(1, 2).contiguous().transpose(1, 2)
    assert not xt.is_contiguous()
    nc.check_exact(run(xt), want, "non-contiguous")
    nc.check_exact(run(x.double()), want, "fp64")
    for dt in (torch.float16, torch.bfloat16):
        xh = x.to(dt)
        nc.check_exact(run(xh), nc.oracle(xh.float()), str(dt))
    x.requires_grad_(True)
    assert not ops.noise_filter(x).mean_dist.requires_grad
    for shape in ((0, 5, 3), (2, 0, 3), (0, 0, 3)):
        out = ops.noise_filter(torch.zeros(shape))
        B, N = shape[:2]
        assert out.keep.shape == (B, N) and out.keep.dtype == torch.bool
        assert out.count.shape == (B, N) and out.count.dtype == torch.int32
        assert out.mean_dist.shape == (B, N) and out.mean_dist.dtype == torch.float32
        for t in (out.mean, out.std, out.threshold):
            assert t.shape == (B,) and t.dtype == torch.float64 and (t == 0).all()
        assert out.ok.shape == (B,) and out.ok.dtype == torch.bool and out.ok.all()


def test_bad_arguments_raise():
    x = nc.scene(1, 2, seed=1)
    for kw in ({"radius": 0.0}, {"radius": -1.0}, {"radius": float("nan")}, {"radius": float("inf")},
               {"min_neighbors": -1}, {"k": -1}, {"k": 17}, {"std_ratio": -0.5}, {"std_ratio": float("nan")},
               {"radius": "wide"}):
        with pytest.raises(ValueError):
            ops.noise_filter(x, **kw)
    with pytest.raises(ValueError):
        ops.noise_filter(x[0])
    with pytest.raises(ValueError):
        ops.noise_filter(torch.zeros(1, 4, 2))
    with pytest.raises(ValueError):
        ops.noise_filter(x, mask=torch.ones(1, 3, dtype=torch.bool))
    with pytest.raises(ValueError):  # N < 2**27, checked before any allocation
        ops.noise_filter(torch.zeros(1, 3).expand(1 << 27, 3).unsqueeze(0))


# ---------------------------------------------------------------------------
# effect
# ---------------------------------------------------------------------------


def test_effect_on_the_voxel_sample():
    """Patch-plus-noise scene, N = 8192, m = 2048, seed 11, with the radius
    rule of the defaults (radius 0.5, 4 neighbours, k = 0: the rule the
    motivating probe used).  Measured on the CPU for this seed: 87 of the 90
    injected points are in the unmasked voxel sample and 0 in the masked one,
    the rule keeps 1 injected point and flags 4 of 8102 surface points.  With
    the statistical rule on as well (k = 8, std_ratio = 2.0) a 2-sigma cut
    flags the tail of the surface's own distribution, 391 of 8102 (4.8 %)
    here, mostly at patch borders: printed, not asserted against the 1 %."""
    p, injected = nc.patches_with_noise(8192, seed=11)
    x = torch.from_numpy(p).unsqueeze(0)
    nf = ops.noise_filter(x, k=0)
    keep = nf.keep[0].numpy()
    plain = ops.voxel_sample(x, 2048).idx[0].numpy()
    masked = ops.voxel_sample(x, 2048, mask=nf.keep).idx[0].numpy()
    n_plain, n_masked = int(injected[plain].sum()), int(injected[masked].sum())
    flagged = int((~keep & ~injected).sum())
    both = ops.noise_filter(x).keep[0].numpy()
    print(f"injected {int(injected.sum())}: in the plain sample {n_plain}, in the masked one {n_masked}; surface "
          f"flagged {flagged} of {int((~injected).sum())}; with k = 8 as well {int((~both & ~injected).sum())}")
    assert n_plain >= 0.9 * injected.sum()  # the sampler's bias the filter is for
    assert (masked >= 0).all() and keep[masked].all()
    assert n_masked <= n_plain / 4
    assert flagged <= 0.01 * (~injected).sum()
    assert int((both & injected).sum()) <= int((keep & injected).sum())  # the second rule only removes


# ---------------------------------------------------------------------------
# layers
# ---------------------------------------------------------------------------


def test_synthetic_noise_fraction():
    from pvraft_amd.data import SyntheticSceneFlow

    for kw in ({}, {"full_points": 300}, {"ground_fraction": 0.3}):
        old = SyntheticSceneFlow(64, length=3, seed=1, **kw)
        new = SyntheticSceneFlow(64, length=3, seed=1, noise_fraction=0.0, **kw)
        for i in range(3):
            (a1, a2), (am, af) = old.load_sequence(i)
            (b1, b2), (bm, bf) = new.load_sequence(i)
            for u, v in ((a1, b1), (a2, b2), (am, bm), (af, bf)):
                assert u.dtype == v.dtype and np.array_equal(u, v)
    ds = SyntheticSceneFlow(64, length=2, seed=1, full_points=400, noise_fraction=0.05)
    base = SyntheticSceneFlow(64, length=2, seed=1, full_points=400)
    (p1, p2), (m, f) = ds.load_sequence(0)
    (q1, q2), _ = base.load_sequence(0)
    noise = m[:, 0] == 0
    assert noise.sum() == 20 and p1.dtype == np.float32 and p2.dtype == np.float32
    assert (f[noise] == 0).all() and np.array_equal(p1[~noise], q1[~noise]) and np.array_equal(p2[~noise], q2[~noise])
    assert not np.array_equal(p1[noise], q1[noise])
    lo, hi = np.minimum(q1.min(0), q2.min(0)), np.maximum(q1.max(0), q2.max(0))
    assert (p1[noise] >= lo).all() and (p1[noise] <= hi).all() and (p2[noise] >= lo).all() and (p2[noise] <= hi).all()
    with pytest.raises(ValueError):
        SyntheticSceneFlow(64, noise_fraction=1.0)


@pytest.fixture(scope="module")
def predictor():
    from pvraft_amd.engine import Predictor
    from pvraft_amd.model import PVRaft

    torch.manual_seed(5)
    return Predictor(PVRaft(truncate_k=16).eval(), points=128, batch=1, iters=1)


def _raw_scan():
    """600 surface points in clusters over a ground plane, 40 isolated ones."""
    rng = np.random.default_rng(4)
    obj = nc.clustered(360, seed=8, spread=0.15) * np.float32(0.5)
    obj[:, 1] = np.abs(obj[:, 1]) * 0.3 + 0.2
    ground = np.stack([rng.uniform(-4, 4, 240), rng.normal(-1.4, 0.01, 240), rng.uniform(-4, 4, 240)], -1)
    lone = rng.uniform(-30.0, 30.0, size=(40, 3)) + np.array([0.0, 40.0, 0.0])
    p = np.concatenate([obj, ground, lone]).astype(np.float32)
    return torch.from_numpy(p[rng.permutation(len(p))])


@pytest.mark.parametrize("sampling", ["random", "voxel"])
@pytest.mark.parametrize("remove_ground", [False, True])
def test_predict_dense_remove_noise(predictor, sampling, remove_ground):
    pc1 = _raw_scan()
    pc2 = pc1 + torch.tensor([0.05, 0.0, 0.1])
    kw = {"radius": 0.6, "min_neighbors": 3, "k": 4, "std_ratio": 3.0}
    gen = torch.Generator().manual_seed(3)
    out = predictor.predict_dense(pc1, pc2, generator=gen, return_sparse=True, sampling=sampling,
                                  remove_ground=remove_ground, remove_noise=True, noise_kw=kw,
                                  ground_kw={"hypotheses": 64}, sample_kw={"voxel": 0.2} if sampling == "voxel" else None)
    assert len(out) == (5 if remove_ground else 4)
    dense, idx1, sub, noise = out[0], out[1], out[2], out[-1]
    nf = ops.noise_filter(pc1.unsqueeze(0), **kw)
    assert noise.dtype == torch.bool and noise.shape == (640,) and torch.equal(noise, ~nf.keep[0])
    assert noise.any() and not noise[idx1].any()
    if remove_ground:
        ground = out[3]
        assert torch.equal(ground, ops.fit_plane(pc1.unsqueeze(0), hypotheses=64).ground[0])
        assert ground.any() and not ground[idx1].any()
    assert dense.shape == (640, 3) and torch.isfinite(dense).all() and sub.shape == (128, 3)
    assert idx1.shape == (128,) and idx1.unique().numel() == 128


def test_predict_dense_default_path_unchanged_and_count_error(predictor):
    pc1 = _raw_scan()
    pc2 = pc1 + torch.tensor([0.05, 0.0, 0.1])
    a = predictor.predict_dense(pc1, pc2, generator=torch.Generator().manual_seed(3), return_sparse=True)
    b = predictor.predict_dense(pc1, pc2, generator=torch.Generator().manual_seed(3), return_sparse=True,
                                remove_noise=False, noise_kw={"radius": 9.0})
    assert len(a) == len(b) == 3
    for u, v in zip(a, b):
        assert torch.equal(u, v)
    # the default draw is the plain permutation of the parent
    want = torch.randperm(640, generator=torch.Generator().manual_seed(3))[:128]
    assert torch.equal(a[1], want)
    tight = {"radius": 0.01, "min_neighbors": 50}
    for sampling in ("random", "voxel"):
        with pytest.raises(ValueError, match="fewer than the 128"):
            predictor.predict_dense(pc1, pc2, sampling=sampling, remove_noise=True, noise_kw=tight)
