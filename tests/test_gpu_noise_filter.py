"""GPU tests of the noise filter (csrc/noise_filter.hip) and the Predictor
option on it.  Every result is compared with the numpy oracle of noise_cases
evaluated on the CPU: count, mean_dist and ok bit for bit (every operation of
the definition is a single correctly rounded fp32 operation), the statistics
within 1e-9 * radius, keep exactly (no committed scene has a point in the near
set of its threshold; noise_cases asserts that).  Run with -m gpu."""

import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import noise_cases as nc

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    import pvraft_amd.ops as ops


@pytest.fixture(scope="module", autouse=True)
def _require_gpu_and_ext():
    if not torch.cuda.is_available():
        pytest.skip("needs GPU")
    import pvraft_amd.ops as ops

    assert ops.hip_available(), "HIP extension must be built on the GPU box"


def dev():
    return torch.device("cuda:0")


def shapes():
    from pvraft_amd import _C

    blk = int(_C.NOISE_FILTER_BLOCK)  # points, and table slots, per workgroup
    scan = int(_C.NOISE_FILTER_SCAN)  # run totals per step of the offset scan
    assert blk >= 64 and blk * scan + 1 <= 16385
    s = [(1, 1), (1, 2), (2, 63), (2, 64), (3, 65)]
    # the table of a cloud has the next power of two >= 2 N slots: 1024 -> 2048 at N = 513
    for n in (blk - 1, blk, blk + 1, 511, 512, 513):
        s.append((1, n))
    # the table has more than blk * scan slots from N = blk * scan / 2 + 1 on,
    # so the offset scan takes further steps; at blk * scan + 1 it doubles again
    s += [(1, blk * scan - 1), (1, blk * scan), (1, blk * scan + 1)]
    return s


def pytest_generate_tests(metafunc):
    if "shape" in metafunc.fixturenames:
        s = shapes() if torch.cuda.is_available() else [(1, 1)]
        metafunc.parametrize("shape", s, ids=[f"{b}x{n}" for b, n in s])


_SCENES = {}


def scene(B, N):
    """One scene per shape, generated once and never modified."""
    if (B, N) not in _SCENES:
        _SCENES[(B, N)] = nc.scene(B, N, seed=7 * N + B)
    return _SCENES[(B, N)]


def gpu_filter(x, mask=None, **kw):
    out = ops.noise_filter(x.to(dev()), mask=None if mask is None else mask.to(dev()), **kw)
    torch.cuda.synchronize()
    assert isinstance(out, ops.NoiseFilter) and all(t.is_cuda for t in out)
    return out


def full_check(key, x, mask=None, radius=0.5, min_neighbors=4, k=8, std_ratio=2.0):
    want = nc.scene_oracle(key, x, radius, min_neighbors, k, std_ratio, mask)
    got = nc.as_numpy(gpu_filter(x, mask, radius=radius, min_neighbors=min_neighbors, k=k, std_ratio=std_ratio))
    nc.check(got, want, radius, min_neighbors, k, str(key))
    return want


# ---------------------------------------------------------------------------
# 1. shapes and parameters
# ---------------------------------------------------------------------------


def test_matches_oracle(shape):
    B, N = shape
    full_check(("scene", B, N), scene(B, N))


@pytest.mark.parametrize("k", [0, 1, 8, 16])
def test_k_and_counts_at_k(k):
    x = nc.exact_k(k, seed=3)
    want = nc.oracle(x, k=k, min_neighbors=0)
    assert {max(k - 1, 0), k, k + 1} <= set(want["count"][0].tolist())
    got = nc.as_numpy(gpu_filter(x, k=k, min_neighbors=0))
    nc.check(got, want, 0.5, 0, k, f"k={k}")
    full_check(("scene", 3, 65), scene(3, 65), k=k, min_neighbors=0)
    full_check(("scene", 1, 513), scene(1, 513), k=k, min_neighbors=0 if k else 9, std_ratio=0.5)


# ---------------------------------------------------------------------------
# 2. contention, ties, signs, the stencil
# ---------------------------------------------------------------------------


def test_coincident_points_one_cell():
    x = nc.coincident(1025)
    want = nc.oracle(x, k=16)
    assert (want["count"] == 1024).all() and (want["mean_dist"] == 0).all()
    got = nc.as_numpy(gpu_filter(x, k=16))
    nc.check_exact(got, want, "coincident")
    nc.check_sparse(got, want, 4, "coincident")


def test_lattice_ties_at_the_radius():
    x = nc.lattice(6, 0.5)
    for k in (0, 6, 8):
        want = nc.oracle(x, k=k)
        assert want["count"].max() == 6
        got = nc.as_numpy(gpu_filter(x, k=k))
        nc.check_exact(got, want, f"lattice k={k}")
        nc.check_sparse(got, want, 4, f"lattice k={k}")
    big = nc.lattice(16, 0.5)  # 4096 points, arithmetic-progression keys
    got = nc.as_numpy(gpu_filter(big, k=0))
    nc.check(got, nc.oracle(big, k=0), 0.5, 4, 0, "lattice 16^3")
    up = nc.lattice(6, np.nextafter(np.float32(0.5), np.float32(1)))
    want = nc.oracle(up, k=0)
    assert (want["count"] == 0).all()
    nc.check(nc.as_numpy(gpu_filter(up, k=0)), want, 0.5, 4, 0, "lattice one ulp above the radius")


def test_negative_coordinates_and_cell_faces():
    full_check(("negative", 1000), nc.negative(1000, seed=2))
    full_check(("faces", 1000), nc.faces(1000, seed=3))


def test_stencil_condition_decides():
    full_check(("stencil",), nc.stencil_edges(), radius=nc.STENCIL_RADIUS, min_neighbors=1, k=2)


# ---------------------------------------------------------------------------
# 3. eligibility, batches
# ---------------------------------------------------------------------------


def test_mask_and_bad_rows():
    x = nc.dirty(2, 300, seed=4)
    want = full_check(("dirty", 2, 300), x)
    assert (want["count"][:, nc.BAD_ROWS] == -1).all()
    x = nc.scene(2, 300, seed=9)
    mask = torch.rand(2, 300, generator=torch.Generator().manual_seed(3)) > 0.3
    want = full_check(("masked", 2, 300), x, mask=mask)
    assert (want["count"][~mask.numpy()] == -1).all()
    none = nc.as_numpy(gpu_filter(x, torch.zeros(2, 300, dtype=torch.bool)))
    assert (none["count"] == -1).all() and not none["keep"].any() and np.isinf(none["mean_dist"]).all()
    assert (none["threshold"] == 0).all() and (none["mean"] == 0).all() and none["ok"].all()
    nan = nc.as_numpy(gpu_filter(torch.full((1, 70, 3), float("nan"))))
    assert (nan["count"] == -1).all() and not nan["keep"].any() and nan["ok"].all()


def test_clouds_do_not_see_each_other():
    x = scene(3, 65)
    want = nc.scene_oracle(("scene", 3, 65), x)
    for b in range(3):
        one = nc.as_numpy(gpu_filter(x[b:b + 1]))
        assert np.array_equal(one["count"][0], want["count"][b])
        assert np.array_equal(nc.bits(one["mean_dist"][0]), nc.bits(want["mean_dist"][b]))


# ---------------------------------------------------------------------------
# 4. invariants, dispatch, arguments
# ---------------------------------------------------------------------------


def test_bit_identical_runs_and_permutation():
    from pvraft_amd import _C

    n = int(_C.NOISE_FILTER_BLOCK) * int(_C.NOISE_FILTER_SCAN) + 1
    x = scene(1, n)
    want = nc.scene_oracle(("scene", 1, n), x)
    a = gpu_filter(x)
    b = gpu_filter(x)
    for u, v in zip(a, b):
        assert torch.equal(u, v)
    perm = torch.randperm(n, generator=torch.Generator().manual_seed(1))
    got = nc.as_numpy(gpu_filter(x[:, perm]))
    p = perm.numpy()
    assert np.array_equal(got["count"][0], want["count"][0][p])
    assert np.array_equal(nc.bits(got["mean_dist"][0]), nc.bits(want["mean_dist"][0][p]))
    assert np.array_equal(got["keep"][0], want["keep"][0][p])
    total = int(got["count"][got["count"] >= 0].sum())
    assert total % 2 == 0 and total == int(want["count"][want["count"] >= 0].sum())


def test_reference_dispatch_and_input_conversion(monkeypatch):
    x = scene(2, 64)
    want = nc.scene_oracle(("scene", 2, 64), x)
    monkeypatch.setenv("PVRAFT_REF_OPS", "1")
    ref = ops.noise_filter(x.to(dev()))
    monkeypatch.delenv("PVRAFT_REF_OPS")
    assert ref.keep.is_cuda
    nc.check(nc.as_numpy(ref), want, 0.5, 4, 8, "device reference")
    xt = x.to(dev()).transpose(1, 2).contiguous().transpose(1, 2)
    assert not xt.is_contiguous()
    nc.check_exact(nc.as_numpy(ops.noise_filter(xt)), want, "non-contiguous")
    nc.check_exact(nc.as_numpy(ops.noise_filter(x.double().to(dev()))), want, "fp64")
    xh = x.half()
    nc.check_exact(nc.as_numpy(ops.noise_filter(xh.to(dev()))), nc.oracle(xh.float()), "fp16")
    for shape in ((0, 5, 3), (2, 0, 3)):
        out = ops.noise_filter(torch.zeros(shape, device=dev()))
        assert out.keep.shape == shape[:2] and out.mean.shape == shape[:1] and out.keep.is_cuda


def test_bad_arguments_raise_on_device():
    x = scene(1, 2).to(dev())
    for kw in ({"radius": 0.0}, {"radius": -1.0}, {"radius": float("nan")}, {"min_neighbors": -1}, {"k": -1},
               {"k": 17}, {"std_ratio": -0.5}):
        with pytest.raises(ValueError):
            ops.noise_filter(x, **kw)
    with pytest.raises(ValueError):
        ops.noise_filter(x[0])
    with pytest.raises(ValueError):
        ops.noise_filter(x, mask=torch.ones(1, 3, dtype=torch.bool, device=dev()))


# ---------------------------------------------------------------------------
# 5. Predictor
# ---------------------------------------------------------------------------


def test_predictor_remove_noise():
    from pvraft_amd.engine import Predictor
    from pvraft_amd.model import PVRaft

    torch.manual_seed(5)
    model = PVRaft(truncate_k=64).to(dev()).eval()
    pred = Predictor(model, points=256, batch=1, iters=2)
    pc1 = scene(1, 1025)[0].to(dev())
    pc2 = pc1 + torch.tensor([0.05, 0.0, 0.3], device=dev())
    want = nc.scene_oracle(("scene", 1, 1025), scene(1, 1025), k=4, std_ratio=3.0)
    noise_kw = {"k": 4, "std_ratio": 3.0}
    for sampling in ("voxel", "random"):
        dense, idx1, sub, noise = pred.predict_dense(
            pc1, pc2, return_sparse=True, sampling=sampling, remove_noise=True, noise_kw=noise_kw,
            generator=torch.Generator().manual_seed(2))
        assert np.array_equal(noise.cpu().numpy(), ~want["keep"][0]) and noise.any()
        assert not noise[idx1].any() and idx1.unique().numel() == 256
        assert dense.shape == (1025, 3) and torch.isfinite(dense).all() and sub.shape == (256, 3)
    with pytest.raises(ValueError, match="fewer than the 256"):
        pred.predict_dense(pc1, pc2, sampling="voxel", remove_noise=True, noise_kw={"radius": 0.01})
