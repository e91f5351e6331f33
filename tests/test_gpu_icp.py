"""GPU tests of the grid search and the ICP refinement (csrc/grid_nn.hip) and
of the Predictor option on them.  The search is compared with the numpy oracle
of icp_cases bit for bit (every operation of the definition is a single
correctly rounded fp32 operation); the ICP loop with the float64 oracle under
the tolerance rule of ego_cases.  Run with -m gpu."""

import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import icp_cases as ic
from ego_cases import bound, box_cloud, coord_scale, max_dev

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    import pvraft_amd.ops as ops

INF = float("inf")
SHAPES = [(1, 1, 1), (2, 63, 65), (2, 64, 64), (1, 255, 257), (1, 256, 256), (2, 257, 1025), (1, 1025, 255)]


@pytest.fixture(scope="module", autouse=True)
def _require_gpu_and_ext():
    if not torch.cuda.is_available():
        pytest.skip("needs GPU")
    import pvraft_amd.ops as ops

    assert ops.hip_available(), "HIP extension must be built on the GPU box"


def dev():
    return torch.device("cuda:0")


def to_dev(x):
    return None if x is None else x.to(dev())


def gpu_search(q, s, radius, query_mask=None, support_mask=None, R=None, t=None):
    out = ops.nearest_in_radius(to_dev(q), to_dev(s), radius, to_dev(query_mask), to_dev(support_mask),
                                to_dev(R), to_dev(t))
    torch.cuda.synchronize()
    assert isinstance(out, ops.NearestInRadius) and all(x.is_cuda for x in out)
    assert out.idx.shape == q.shape[:2] and out.d2.shape == q.shape[:2] and out.ok.shape == q.shape[:1]
    return out


def gpu_icp(src, dst, **kw):
    out = ops.icp_refine(to_dev(src), to_dev(dst), **{k: to_dev(v) if torch.is_tensor(v) else v for k, v in kw.items()})
    torch.cuda.synchronize()
    assert isinstance(out, ops.IcpRefine) and all(x.is_cuda for x in out)
    return out


def exact(q, s, radius, label, **kw):
    want = ic.oracle_search(q, s, radius, **kw)
    ic.check_search(gpu_search(q, s, radius, **kw), want, label)
    return want


# ---------------------------------------------------------------------------
# 1. search, exact
# ---------------------------------------------------------------------------


@pytest.mark.parametrize("shape", SHAPES, ids=["x".join(map(str, s)) for s in SHAPES])
@pytest.mark.parametrize("moved", [False, True], ids=["plain", "Rt"])
def test_search_matches_the_oracle(shape, moved):
    B, Nq, M = shape
    q, s = ic.random_pair(B, Nq, M, seed=11 * Nq + M)
    kw = {}
    if moved:
        kw["R"], kw["t"] = ic.small_motion(B, seed=Nq)
    want = exact(q, s, 0.5, str(shape), **kw)
    if Nq > 1:
        assert (want[0] >= 0).any() and (want[0] < 0).any()


def test_search_on_the_resampled_scene():
    src, dst = ic.resampled_surface(seed=5)
    R0, t0 = ic.start_motion()
    assert src.shape == (1, 2048, 3) and dst.shape == (1, 16384, 3)
    want = exact(src, dst, 1.0, "resampled", R=R0, t=t0)
    assert (want[0] >= 0).mean() > 0.9


def test_every_support_point_in_one_cell():
    g = torch.Generator().manual_seed(3)
    s = 0.05 + 0.4 * torch.rand(1, 700, 3, generator=g)  # all in cell (0, 0, 0) of a 0.5 m grid
    q = torch.rand(1, 300, 3, generator=g) * 1.4 - 0.45
    want = exact(q, s, 0.5, "one cell")
    assert (want[0] >= 0).any() and (want[0] < 0).any()


def test_ties_go_to_the_smallest_index():
    # integer lattice queried at its cell centres: eight support points at the same d2
    g = np.stack(np.meshgrid(*[np.arange(-3, 4)] * 3, indexing="ij"), -1).reshape(1, -1, 3).astype(np.float32)
    for seed in (0, 1):  # two support orders: the sorted order inside a cell differs, idx must not
        perm = np.random.default_rng(seed).permutation(g.shape[1])
        s = torch.from_numpy(g[:, perm])
        q = torch.from_numpy(g + 0.5)
        want = exact(q, s, 1.0, "lattice midpoints")
        assert (want[2][want[0] >= 0] == 0).sum() > 100  # real ties
    # coincident support points, several copies of several places
    places = torch.tensor([[0.1, 0.2, 0.3], [0.1, 0.2, 0.3], [-0.7, 0.0, 0.2], [0.1, 0.2, 0.3], [-0.7, 0.0, 0.2]])
    s = places.repeat(40, 1)[None]
    q = torch.tensor([[[0.1, 0.2, 0.3], [-0.7, 0.0, 0.2], [0.0, 0.1, 0.25], [5.0, 5.0, 5.0]]])
    want = exact(q, s, 0.5, "coincident")
    assert want[0].tolist() == [[0, 2, 0, -1]]


def test_cell_faces_negative_coordinates_and_the_stencil_rule():
    p, radius, (i, j) = ic.stencil_scene()
    out = gpu_search(p[:, i : i + 1], p[:, j : j + 1], radius)  # closer than radius, two cells apart
    assert out.idx.tolist() == [[-1]] and out.d2.tolist() == [[INF]] and out.ok.all()
    exact(p, p[:, ::2], radius, "stencil")
    exact(p, p, radius, "stencil self")


def test_masks_bad_rows_and_batches():
    q, s = ic.random_pair(2, 300, 700, seed=3)
    q, s = q.clone(), s.clone()
    bad = (float("nan"), INF, -INF, 3e6, -3e6)
    for k, v in enumerate(bad):
        q[k % 2, 3 * k, k % 3] = v
        s[k % 2, 5 * k + 1, (k + 1) % 3] = v
    qm = torch.rand(2, 300, generator=torch.Generator().manual_seed(1)) > 0.3
    sm = torch.rand(2, 700, generator=torch.Generator().manual_seed(2)) > 0.3
    exact(q, s, 0.5, "bad rows")
    want = exact(q, s, 0.5, "bad rows, masked", query_mask=qm, support_mask=sm)
    assert (want[0][~qm.numpy()] == -1).all() and (want[0] >= 0).any()
    # an all-masked support (one cloud of the two): every idx of it is -1
    sm2 = sm.clone()
    sm2[1] = False
    none = exact(q, s, 0.5, "all masked", support_mask=sm2)
    assert (none[0][1] == -1).all() and (none[0][0] >= 0).any()
    # two batch elements must not see each other: cloud 1's support is cloud 0's query set
    q2 = torch.stack([q[0], q[0] + 50.0])
    s2 = torch.stack([q[0] + 50.0, q[0]])
    far = gpu_search(q2, s2, 0.5)
    assert (far.idx == -1).all() and (far.d2 == INF).all() and far.ok.all()


# ---------------------------------------------------------------------------
# 2. permutation and determinism
# ---------------------------------------------------------------------------


def test_permutation_and_determinism():
    q, s = ic.random_pair(1, 1500, 4000, seed=8)
    R, t = ic.small_motion(1, seed=2)
    base = gpu_search(q, s, 0.5, R=R, t=t)
    again = gpu_search(q, s, 0.5, R=R, t=t)
    assert torch.equal(base.idx, again.idx) and torch.equal(base.d2, again.d2)
    perm = torch.randperm(4000, generator=torch.Generator().manual_seed(4))
    moved = gpu_search(q, s[:, perm], 0.5, R=R, t=t)
    m = base.idx >= 0
    assert m.any() and torch.equal(m, moved.idx >= 0)
    assert torch.equal(perm.to(dev())[moved.idx[m].long()], base.idx[m].long())
    assert torch.equal(base.d2, moved.d2)
    qperm = torch.randperm(1500, generator=torch.Generator().manual_seed(5))
    qmoved = gpu_search(q[:, qperm], s, 0.5, R=R, t=t)
    assert torch.equal(qmoved.idx, base.idx[:, qperm.to(dev())]) and torch.equal(qmoved.d2, base.d2[:, qperm.to(dev())])


# ---------------------------------------------------------------------------
# 3. ICP on the paired lattice
# ---------------------------------------------------------------------------


@pytest.mark.parametrize("N", [257, 1024, 2048])
def test_icp_on_the_paired_lattice(N):
    src, dst, perm = ic.paired_lattice(N, seed=N)
    R0, t0 = ic.start_motion()
    want = ic.oracle_icp(src, dst, R0, t0, iters=10)
    # precondition: fp32 rounding moves a d2 by about 2 d ulp(40 m) ~ 1e-5 m^2
    # at d <= 1 m; a gap of 0.01 m^2 leaves a factor near 1000
    print(f"N={N}: smallest best / second-best gap over all rounds {want['min_gap']:.3f} m^2")
    assert want["min_gap"] >= ic.MIN_GAP
    ref = ops.icp_refine(src, dst, R0=R0, t0=t0, iters=10)  # fp32 on the CPU
    got = gpu_icp(src, dst, R0=R0, t0=t0, iters=10)
    assert np.array_equal(got.idx.cpu().numpy(), want["idx"]) and np.array_equal(want["idx"], perm.numpy())
    assert got.matched.tolist() == [N] and got.rounds.tolist() == [10] and got.ok.all()
    scale = coord_scale(src, dst)
    for name, sc in (("R", 1.0), ("t", scale), ("d2", scale)):
        b = bound(getattr(ref, name), want[name], sc)
        e = max_dev(getattr(got, name), want[name])
        print(f"N={N} {name}: |kernel - oracle| = {e:.3e}, |ref32 - oracle| = "
              f"{max_dev(getattr(ref, name), want[name]):.3e}, bound = {b:.3e}")
        assert e <= b, f"{name} off by {e:.3e} > {b:.3e}"


# ---------------------------------------------------------------------------
# 4. ICP on the resampled scene (ambiguous correspondences: no oracle for R, t)
# ---------------------------------------------------------------------------


def test_icp_on_the_resampled_scene():
    src, dst = ic.resampled_surface(seed=5)
    R0, t0 = ic.start_motion()
    first = gpu_icp(src, dst, R0=R0, t0=t0, iters=0)
    assert torch.equal(first.R.cpu(), R0) and torch.equal(first.t.cpu(), t0) and first.rounds.tolist() == [0]
    ic.check_search(ops.NearestInRadius(first.idx, first.d2, first.ok),
                    ic.oracle_search(src, dst, 1.0, R=R0, t=t0), "first round")
    one = gpu_icp(src, dst, R0=R0, t0=t0, iters=1)
    assert one.rounds.tolist() == [1] and one.ok.all()
    got = gpu_icp(src, dst, R0=R0, t0=t0, iters=10)
    nn = ops.nearest_in_radius(src.to(dev()), dst.to(dev()), 1.0, R=got.R, t=got.t)
    assert torch.equal(got.idx, nn.idx) and torch.equal(got.d2, nn.d2)
    assert got.ok.all() and got.rounds.tolist() == [10] and got.matched.tolist() == [int((nn.idx >= 0).sum())]
    again = gpu_icp(src, dst, R0=R0, t0=t0, iters=10)
    for a, b in zip(got, again):
        assert torch.equal(a, b)


# ---------------------------------------------------------------------------
# 5. degenerate
# ---------------------------------------------------------------------------


def test_icp_degenerate():
    src, dst, _ = ic.paired_lattice(300, seed=1, B=2)
    R0, t0 = ic.start_motion(2)
    far = dst.clone()
    far[1] += 100.0  # cloud 1 has no match; cloud 0 is unaffected
    got = gpu_icp(src, far, R0=R0, t0=t0, iters=4)
    assert got.ok.tolist() == [True, False] and got.rounds.tolist() == [4, 0] and got.matched.tolist() == [300, 0]
    assert torch.equal(got.R[1].cpu(), R0[1]) and torch.equal(got.t[1].cpu(), t0[1])
    assert (got.idx[1] == -1).all() and (got.d2[1] == INF).all()
    alone = gpu_icp(src[:1], dst[:1], R0=R0[:1], t0=t0[:1], iters=4)
    assert torch.equal(alone.R[0], got.R[0]) and torch.equal(alone.t[0], got.t[0]) and torch.equal(alone.idx[0], got.idx[0])
    # a src_mask that leaves two points
    mask = torch.zeros(2, 300, dtype=torch.bool)
    mask[:, :2] = True
    two = gpu_icp(src, dst, R0=R0, t0=t0, iters=4, src_mask=mask)
    assert not two.ok.any() and two.rounds.tolist() == [0, 0] and two.matched.tolist() == [2, 2]
    assert torch.equal(two.R.cpu(), R0) and torch.equal(two.t.cpu(), t0) and (two.idx[:, 2:] == -1).all()
    # iters = 0 with the default start: identity / zero, every point its own partner
    ident = gpu_icp(src, src, iters=0)
    assert torch.equal(ident.R.cpu(), torch.eye(3).expand(2, 3, 3)) and not ident.t.any() and ident.ok.all()
    assert torch.equal(ident.idx.cpu(), torch.arange(300, dtype=torch.int32).expand(2, 300)) and not ident.d2.any()


# ---------------------------------------------------------------------------
# 6. dispatch and arguments
# ---------------------------------------------------------------------------


def test_reference_dispatch_on_device(monkeypatch):
    q, s = ic.random_pair(2, 257, 1025, seed=21)
    R, t = ic.small_motion(2, seed=3)
    got = gpu_search(q, s, 0.5, R=R, t=t)
    src, dst, _ = ic.paired_lattice(257, seed=257)
    R0, t0 = ic.start_motion()
    icp = gpu_icp(src, dst, R0=R0, t0=t0, iters=3)
    monkeypatch.setenv("PVRAFT_REF_OPS", "1")
    ref = gpu_search(q, s, 0.5, R=R, t=t)
    ref_icp = gpu_icp(src, dst, R0=R0, t0=t0, iters=3)
    monkeypatch.delenv("PVRAFT_REF_OPS")
    assert torch.equal(ref.idx, got.idx) and torch.equal(ref.d2, got.d2) and torch.equal(ref.ok, got.ok)
    assert torch.equal(ref_icp.idx, icp.idx) and torch.equal(ref_icp.matched, icp.matched)
    assert torch.equal(ref_icp.rounds, icp.rounds) and torch.equal(ref_icp.ok, icp.ok)


def test_inputs_are_converted():
    q, s = ic.random_pair(1, 200, 500, seed=4)
    qb, sb = q.bfloat16(), s.bfloat16()
    want = ic.oracle_search(qb.float(), sb.float(), 0.5)
    ic.check_search(gpu_search(qb, sb, 0.5), want, "bf16")
    qt = q.to(dev()).transpose(1, 2).contiguous().transpose(1, 2)  # (1,200,3) view of a (1,3,200) buffer
    st = s.to(dev()).double()[:, ::2]
    assert not qt.is_contiguous() and not st.is_contiguous()
    out = ops.nearest_in_radius(qt, st, 0.5)
    ic.check_search(out, ic.oracle_search(q, s[:, ::2], 0.5), "strided")
    icp = ops.icp_refine(qt, st, iters=1)
    assert icp.idx.shape == (1, 200) and icp.R.dtype == torch.float32


def test_bad_arguments_raise_on_device():
    q, s = ic.random_pair(1, 8, 9, seed=1)
    q, s = q.to(dev()), s.to(dev())
    for kw in ({"radius": 0.0}, {"radius": -1.0}, {"radius": INF}):
        with pytest.raises(ValueError):
            ops.nearest_in_radius(q, s, **kw)
    for bad in ((q[0], s), (q, s[..., :2]), (q, s.repeat(2, 1, 1))):
        with pytest.raises(ValueError):
            ops.nearest_in_radius(*bad, 0.5)
        with pytest.raises(ValueError):
            ops.icp_refine(*bad)
    with pytest.raises(ValueError):
        ops.nearest_in_radius(q, s, 0.5, R=torch.eye(3, device=dev())[None])
    for kw in ({"iters": 65}, {"iters": -1}, {"max_dist": 0.0}, {"thresh": 0.0}):
        with pytest.raises(ValueError):
            ops.icp_refine(q, s, **kw)


# ---------------------------------------------------------------------------
# 7. Predictor
# ---------------------------------------------------------------------------


def test_predictor_ego_icp():
    from pvraft_amd.engine import Predictor
    from pvraft_amd.model import PVRaft

    torch.manual_seed(5)
    model = PVRaft(truncate_k=64).to(dev()).eval()
    pred = Predictor(model, points=256, batch=1, iters=2)
    pc, _ = box_cloud(1, 1024, seed=9)
    full = torch.from_numpy(pc).float().to(dev())
    xyz1 = full[:, :256].contiguous()
    xyz2 = full[:, 256:512].contiguous()
    flow, ego, icp = pred.predict_ego_motion(xyz1, xyz2, thresh=0.05, iters=10, icp=True,
                                             icp_kw={"iters": 2, "max_dist": 2.0}, target=full)
    assert torch.equal(flow, pred.last_flows[-1])
    want_ego = ops.ego_motion(xyz1, flow, thresh=0.05, iters=10)
    want = ops.icp_refine(xyz1, full, R0=want_ego.R, t0=want_ego.t, src_mask=want_ego.static, iters=2, max_dist=2.0)
    assert isinstance(ego, ops.EgoMotion) and isinstance(icp, ops.IcpRefine)
    for g, w in zip(ego, want_ego):
        assert torch.equal(g, w)
    for g, w in zip(icp, want):
        assert torch.equal(g, w)
    assert icp.idx.shape == (1, 256) and icp.R.shape == (1, 3, 3) and icp.matched.shape == (1,)
    # without icp the pair it always was
    assert len(pred.predict_ego_motion(xyz1, xyz2)) == 2
