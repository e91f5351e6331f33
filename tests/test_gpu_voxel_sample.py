"""GPU tests of the voxel-stratified sampler (csrc/voxel_sample.hip) and the
Predictor option on it.  Every result is compared with the numpy oracle of
voxel_cases evaluated on the CPU, bit for bit in idx, count, rank and
occupied: the definition is integer after one fp32 multiply, and no test
coordinate makes that product a denormal.  Run with -m gpu."""

import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import voxel_cases as vc

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

    blk = int(_C.VOXEL_SAMPLE_BLOCK)  # points per workgroup
    scan = int(_C.VOXEL_SAMPLE_SCAN)  # workgroup counts per step of the offset scan
    assert blk >= 64 and blk * scan + 1 <= 16385
    s = [(1, 1), (1, 2), (2, 63), (2, 64), (3, 65)]
    # the table of a cloud has the next power of two >= 2 N slots: 1024 -> 2048 at N = 513
    for n in (blk - 1, blk, blk + 1, 511, 512, 513):
        s.append((1, n))
    # many workgroups; the offset scan takes a second step for the one
    # workgroup that holds the last point
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
        _SCENES[(B, N)] = vc.scene(B, N, seed=7 * N + B)
    return _SCENES[(B, N)]


def gpu_sample(x, m, mask=None, **kw):
    out = ops.voxel_sample(x.to(dev()), m, mask=None if mask is None else mask.to(dev()), **kw)
    torch.cuda.synchronize()
    assert isinstance(out, ops.VoxelSample) and all(t.is_cuda for t in out)
    return out


def check(x, m, mask=None, label="", **kw):
    want = vc.oracle(x, m, mask=mask, **kw)
    got = vc.as_numpy(gpu_sample(x, m, mask, **kw))
    vc.assert_equal(got, want, label)
    return want


# ---------------------------------------------------------------------------
# 1. shapes, m, levels, seeds
# ---------------------------------------------------------------------------


def test_matches_oracle(shape):
    B, N = shape
    x = scene(B, N)
    for m in sorted({1, max(1, N // 3), N}):
        check(x, m, label=f"{B}x{N} m={m}")


@pytest.mark.parametrize("levels", [1, 16])
@pytest.mark.parametrize("seed", [0, 1])
def test_levels_and_seeds(levels, seed):
    x = scene(3, 65)
    check(x, 20, levels=levels, seed=seed, label=f"3x65 L={levels} seed={seed}")
    x = scene(1, 513)
    check(x, 100, levels=levels, seed=seed, voxel=0.5, label=f"1x513 L={levels} seed={seed}")


def test_clouds_hash_differently():
    x = scene(1, 513).expand(3, 513, 3).contiguous()
    want = check(x, 64, label="same cloud three times")
    assert not np.array_equal(want["idx"][0], want["idx"][1]) and not np.array_equal(want["idx"][1], want["idx"][2])
    assert np.array_equal(want["occupied"][0], want["occupied"][1])


def test_padding_and_cut_at_level_boundaries():
    x = vc.dirty(1, 4097, seed=3)
    base = vc.oracle(x, 1)
    n_el = int(base["el"].sum())
    assert n_el < 4097
    want = check(x, n_el + 5, label="m = eligible + 5")
    assert want["count"][0] == n_el and (want["idx"][0, n_el:] == -1).all()
    occ = base["occupied"][0]
    lv = 4  # an interior level: the cut on, just below and just above its cell count
    assert occ[lv + 1] + 1 < occ[lv] - 1 and occ[lv] + 1 < occ[lv - 1]
    for m in (int(occ[lv]) - 1, int(occ[lv]), int(occ[lv]) + 1):
        check(x, m, label=f"m = occupied[{lv}] {m - int(occ[lv]):+d}")


# ---------------------------------------------------------------------------
# 2. contention, structured keys, signs
# ---------------------------------------------------------------------------


def test_identical_points_one_slot():
    want = check(vc.identical(4096), 7, label="identical")
    assert (want["occupied"] == 1).all() and want["count"][0] == 7


def test_all_points_in_distinct_cells():
    x = vc.distinct_cells(3000, seed=1)
    want = check(x, 500, label="distinct")
    assert want["occupied"][0, 0] == 3000


def test_integer_lattice_hits_no_cap():
    x = vc.lattice(32)
    for m in (1, 4096, 32768):
        want = check(x, m, voxel=1.0, label=f"lattice m={m}")
        assert (want["count"] >= 0).all()
    assert list(want["occupied"][0, :4]) == [32768, 4096, 512, 64]
    got = gpu_sample(x, 4096, voxel=1.0)
    assert (got.count >= 0).all()


def test_negative_and_straddling_coordinates():
    check(vc.negative(1000, seed=2), 100, label="negative")
    x = vc.straddle(1000, seed=3)
    want = check(x, 100, label="straddle")
    # floor, not truncate: the cells on either side of zero differ
    el, c = vc.cells(x[0].numpy(), 0.1)
    assert (c < 0).any() and (c >= 0).any() and want["occupied"][0, 0] == len(np.unique(c[el], axis=0))
    check(x, 100, levels=16, label="straddle L=16")


# ---------------------------------------------------------------------------
# 3. eligibility
# ---------------------------------------------------------------------------


def test_duplicates_non_finite_and_out_of_range_rows():
    x = vc.dirty(2, 300, seed=4)
    want = check(x, 300, label="dirty")
    bad = [5, 6, 7, 8, 9, 10]
    assert (want["rank"][:, bad] == -1).all() and (want["count"] == 294).all()
    assert not np.isin(want["idx"], bad).any()
    mask = torch.rand(2, 300, generator=torch.Generator().manual_seed(3)) > 0.3
    want = check(x, 50, mask=mask, label="dirty + mask")
    assert (want["rank"][~mask.numpy()] == -1).all()


def test_no_and_one_eligible_point():
    x = vc.dirty(2, 300, seed=4)
    mask = torch.zeros(2, 300, dtype=torch.bool)
    want = check(x, 5, mask=mask, label="nothing eligible")
    assert (want["count"] == 0).all() and (want["idx"] == -1).all() and (want["occupied"] == 0).all()
    check(torch.full((1, 70, 3), float("nan")), 3, label="all NaN")
    mask[0, 17] = True
    mask[1, 299] = True
    want = check(x, 5, mask=mask, label="one eligible")
    assert list(want["idx"][0]) == [17, -1, -1, -1, -1] and list(want["idx"][1]) == [299, -1, -1, -1, -1]
    assert (want["occupied"] == 1).all()


# ---------------------------------------------------------------------------
# 4. determinism, dispatch, arguments
# ---------------------------------------------------------------------------


def test_bit_identical_runs():
    from pvraft_amd import _C

    n = int(_C.VOXEL_SAMPLE_BLOCK) * int(_C.VOXEL_SAMPLE_SCAN) + 1
    x = scene(1, n)
    mask = torch.rand(1, n, generator=torch.Generator().manual_seed(3)) > 0.2
    a = gpu_sample(x, 2048, mask)
    b = gpu_sample(x, 2048, mask)
    for u, v in zip(a, b):
        assert torch.equal(u, v)
    assert a.count.item() == 2048
    vc.check_structure(vc.as_numpy(a), x, 2048, 0.1, 10, mask, 0, "structure on the GPU result")


def test_reference_dispatch_and_input_conversion(monkeypatch):
    x = scene(2, 64)
    want = check(x, 20, label="dispatch")
    monkeypatch.setenv("PVRAFT_REF_OPS", "1")
    ref = ops.voxel_sample(x.to(dev()), 20)
    monkeypatch.delenv("PVRAFT_REF_OPS")
    assert ref.idx.is_cuda
    vc.assert_equal(vc.as_numpy(ref), want, "device reference")
    # non-contiguous and half inputs are converted by the op
    xt = x.to(dev()).transpose(1, 2).contiguous().transpose(1, 2)
    assert not xt.is_contiguous()
    vc.assert_equal(vc.as_numpy(ops.voxel_sample(xt, 20)), want, "non-contiguous")
    xh = x.half()
    vc.assert_equal(vc.as_numpy(ops.voxel_sample(xh.to(dev()), 20)), vc.oracle(xh.float(), 20), "fp16")


def test_bad_arguments_raise_on_device():
    x = scene(1, 2).to(dev())
    for kw in ({"m": 0}, {"voxel": 0.0}, {"voxel": -1.0}, {"voxel": float("nan")}, {"levels": 0}, {"levels": 17}):
        args = {"m": 1, **kw}
        with pytest.raises(ValueError):
            ops.voxel_sample(x, **args)
    with pytest.raises(ValueError):
        ops.voxel_sample(x[0], 1)
    with pytest.raises(ValueError):
        ops.voxel_sample(x, 1, mask=torch.ones(1, 3, dtype=torch.bool, device=dev()))


# ---------------------------------------------------------------------------
# 5. Predictor
# ---------------------------------------------------------------------------


def test_predictor_voxel_sampling():
    from pvraft_amd.engine import Predictor
    from pvraft_amd.model import PVRaft

    torch.manual_seed(5)
    model = PVRaft(truncate_k=64).to(dev()).eval()
    pred = Predictor(model, points=256, batch=1, iters=2)
    pc1 = scene(1, 1025)[0].to(dev())
    pc2 = pc1 + torch.tensor([0.05, 0.0, 0.3], device=dev())
    kw = {"voxel": 0.2, "seed": 3}
    dense, idx1, sub = pred.predict_dense(pc1, pc2, return_sparse=True, sampling="voxel", sample_kw=kw)
    want = ops.voxel_sample(pc1.unsqueeze(0), 256, **kw)
    assert torch.equal(idx1, want.idx[0]) and idx1.dtype == torch.int64
    assert np.array_equal(idx1.cpu().numpy(), vc.oracle(pc1.cpu().unsqueeze(0), 256, **kw)["idx"][0])
    assert dense.shape == (1025, 3) and torch.isfinite(dense).all() and sub.shape == (256, 3)
    _, idx2, _ = pred.predict_dense(pc1, pc2, return_sparse=True, sampling="voxel", sample_kw=kw)
    assert torch.equal(idx1, idx2)
    with pytest.raises(ValueError):
        pred.predict_dense(pc1, pc2, sampling="fps")
