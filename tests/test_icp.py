"""CPU tests of ``ops.nearest_in_radius`` and ``ops.icp_refine`` (the torch
reference path) against the numpy oracles of icp_cases, and of
``Predictor.predict_ego_motion(icp=True)``."""

import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import icp_cases as ic
import pvraft_amd.ops as ops
from ego_cases import EPS32, coord_scale, max_dev, rot_angle_deg

INF = float("inf")


def search(q, s, radius, **kw):
    out = ops.nearest_in_radius(q, s, radius, **kw)
    assert isinstance(out, ops.NearestInRadius)
    return out


@pytest.mark.parametrize("shape", [(1, 1, 1), (2, 63, 65), (1, 255, 257), (2, 257, 1025)], ids=str)
@pytest.mark.parametrize("moved", [False, True], ids=["plain", "Rt"])
def test_search_matches_the_oracle(shape, moved):
    B, Nq, M = shape
    q, s = ic.random_pair(B, Nq, M, seed=11 * Nq + M)
    kw = {}
    if moved:
        kw["R"], kw["t"] = ic.small_motion(B, seed=Nq)
    want = ic.oracle_search(q, s, 0.5, **kw)
    ic.check_search(search(q, s, 0.5, **kw), want, str(shape))
    if Nq > 1:
        assert (want[0] >= 0).any()


def test_search_ties_go_to_the_smallest_index():
    # integer lattice queried at its cell centres: eight support points at the same d2
    g = np.stack(np.meshgrid(*[np.arange(-2, 3)] * 3, indexing="ij"), -1).reshape(1, -1, 3).astype(np.float32)
    perm = np.random.default_rng(0).permutation(g.shape[1])
    s = torch.from_numpy(g[:, perm])
    q = torch.from_numpy(g[:, : 64] + 0.5)
    want = ic.oracle_search(q, s, 1.0)
    assert (want[2][want[0] >= 0] == 0).any()  # real ties
    ic.check_search(search(q, s, 1.0), want, "lattice")
    # coincident support points
    s2 = torch.zeros(1, 5, 3)
    out = search(torch.zeros(1, 1, 3), s2, 0.5)
    assert out.idx.tolist() == [[0]] and out.d2.tolist() == [[0.0]]


def test_search_edge_cases():
    # closer than the radius but two cells apart: not a match
    p, radius, (i, j) = ic.stencil_scene()
    out = search(p[:, i : i + 1], p[:, j : j + 1], radius)
    assert out.idx.tolist() == [[-1]] and out.d2.tolist() == [[INF]]
    # points on cell faces, negative coordinates: every second point as support
    ic.check_search(search(p, p[:, ::2], radius), ic.oracle_search(p, p[:, ::2], radius), "stencil")
    # masks, non-finite and out-of-range rows, on both sides
    q, s = ic.random_pair(2, 40, 90, seed=3)
    q, s = q.clone(), s.clone()
    q[0, 0, 1] = float("nan")
    q[0, 1, 0] = INF
    q[1, 2, 2] = 3e6
    s[0, 0, 0] = float("nan")
    s[1, 1, 1] = -INF
    s[1, 2, 2] = -3e6
    qm = torch.rand(2, 40, generator=torch.Generator().manual_seed(1)) > 0.3
    sm = torch.rand(2, 90, generator=torch.Generator().manual_seed(2)) > 0.3
    want = ic.oracle_search(q, s, 0.5, qm, sm)
    got = search(q, s, 0.5, query_mask=qm, support_mask=sm)
    ic.check_search(got, want, "masked")
    assert (got.idx[~qm] == -1).all() and got.idx[0, 0] == got.idx[0, 1] == got.idx[1, 2] == -1
    m = got.idx >= 0
    assert m.any() and sm[torch.arange(2)[:, None].expand_as(got.idx)[m], got.idx[m].long()].all()
    # an all-masked support
    none = search(q, s, 0.5, support_mask=torch.zeros(2, 90, dtype=torch.bool))
    assert (none.idx == -1).all() and (none.d2 == INF).all() and none.ok.all()
    # empty clouds
    e = search(torch.zeros(1, 0, 3), s[:1], 0.5)
    assert e.idx.shape == (1, 0) and e.d2.shape == (1, 0)
    e = search(q[:1], torch.zeros(1, 0, 3), 0.5)
    assert (e.idx == -1).all()


def test_search_permutation():
    q, s = ic.random_pair(1, 100, 300, seed=8)
    base = search(q, s, 0.5)
    perm = torch.randperm(300, generator=torch.Generator().manual_seed(4))
    moved = search(q, s[:, perm], 0.5)
    m = base.idx >= 0
    assert torch.equal(m, moved.idx >= 0) and torch.equal(perm[moved.idx[m].long()], base.idx[m].long())
    assert torch.equal(base.d2, moved.d2)


def test_bad_arguments():
    q, s = ic.random_pair(1, 8, 9, seed=1)
    for kw in ({"radius": 0.0}, {"radius": -1.0}, {"radius": INF}, {"radius": "x"}):
        with pytest.raises(ValueError):
            ops.nearest_in_radius(q, s, **kw)
    with pytest.raises(ValueError):
        ops.nearest_in_radius(q[0], s, 0.5)
    with pytest.raises(ValueError):
        ops.nearest_in_radius(q, torch.zeros(2, 9, 3), 0.5)
    with pytest.raises(ValueError):
        ops.nearest_in_radius(q, s, 0.5, query_mask=torch.ones(1, 9, dtype=torch.bool))
    with pytest.raises(ValueError):
        ops.nearest_in_radius(q, s, 0.5, R=torch.eye(3)[None])
    with pytest.raises(ValueError):
        ops.nearest_in_radius(q, s, 0.5, R=torch.eye(3), t=torch.zeros(1, 3))
    for kw in ({"iters": 65}, {"iters": -1}, {"max_dist": 0.0}, {"thresh": 0.0}, {"thresh": -1.0}):
        with pytest.raises(ValueError):
            ops.icp_refine(q, s, **kw)
    with pytest.raises(ValueError):
        ops.icp_refine(q, s[..., :2])
    with pytest.raises(ValueError):
        ops.icp_refine(q, s, R0=torch.eye(3)[None])


@pytest.mark.parametrize("N", [257, 1024])
def test_icp_on_the_paired_lattice(N):
    src, dst, perm = ic.paired_lattice(N, seed=N)
    R0, t0 = ic.start_motion()
    want = ic.oracle_icp(src, dst, R0, t0, iters=10)
    assert want["min_gap"] >= ic.MIN_GAP, want["min_gap"]
    got = ops.icp_refine(src, dst, R0=R0, t0=t0, iters=10)
    assert isinstance(got, ops.IcpRefine)
    assert np.array_equal(got.idx.numpy(), want["idx"]) and np.array_equal(want["idx"], perm.numpy())
    assert got.matched.tolist() == [N] and got.rounds.tolist() == [10] and got.ok.all() and want["ok"].all()
    assert got.idx.dtype == torch.int32 and got.matched.dtype == torch.int32 and got.rounds.dtype == torch.int32
    scale = coord_scale(src, dst)
    # fp32 data: the fit moves by a few ulp of the coordinates
    assert max_dev(got.R, want["R"]) <= 64 * EPS32
    assert max_dev(got.t, want["t"]) <= 64 * EPS32 * scale
    assert max_dev(got.d2, want["d2"]) <= 64 * EPS32 * scale
    # and ICP did its job: closer to the truth than the start
    Rt, tt = ic.true_motion()
    assert rot_angle_deg(got.R[0], Rt) < 0.1 * rot_angle_deg(R0[0], Rt)
    assert np.linalg.norm(got.t[0].double().numpy() - tt) < 0.1 * np.linalg.norm(t0[0].double().numpy() - tt)


def test_icp_correspondences_belong_to_the_returned_motion():
    src, dst = ic.resampled_surface(seed=5, n_src=256, n_dst=2048)
    R0, t0 = ic.start_motion()
    first = ops.icp_refine(src, dst, R0=R0, t0=t0, iters=0)
    assert torch.equal(first.R, R0) and torch.equal(first.t, t0) and first.rounds.tolist() == [0] and first.ok.all()
    ic.check_search(ops.NearestInRadius(first.idx, first.d2, first.ok), ic.oracle_search(src, dst, 1.0, R=R0, t=t0))
    got = ops.icp_refine(src, dst, R0=R0, t0=t0, iters=5)
    nn = ops.nearest_in_radius(src, dst, 1.0, R=got.R, t=got.t)
    assert torch.equal(got.idx, nn.idx) and torch.equal(got.d2, nn.d2) and got.ok.all()
    assert got.matched.tolist() == [int((nn.idx >= 0).sum())] and got.rounds.tolist() == [5]


def test_icp_degenerate():
    src, dst, _ = ic.paired_lattice(64, seed=1, B=2)
    R0, t0 = ic.start_motion(2)
    far = dst.clone()
    far[1] += 100.0  # cloud 1 has no match; cloud 0 is unaffected
    got = ops.icp_refine(src, far, R0=R0, t0=t0, iters=4)
    assert got.ok.tolist() == [True, False] and got.rounds.tolist() == [4, 0] and got.matched.tolist() == [64, 0]
    assert torch.equal(got.R[1], R0[1]) and torch.equal(got.t[1], t0[1]) and (got.idx[1] == -1).all()
    alone = ops.icp_refine(src[:1], dst[:1], R0=R0[:1], t0=t0[:1], iters=4)
    assert torch.equal(alone.R[0], got.R[0]) and torch.equal(alone.idx[0], got.idx[0])
    # a src_mask that leaves two points
    mask = torch.zeros(2, 64, dtype=torch.bool)
    mask[:, :2] = True
    two = ops.icp_refine(src, dst, R0=R0, t0=t0, iters=4, src_mask=mask)
    assert not two.ok.any() and two.rounds.tolist() == [0, 0] and two.matched.tolist() == [2, 2]
    assert torch.equal(two.R, R0) and torch.equal(two.t, t0) and (two.idx[:, 2:] == -1).all()
    # default start: identity / zero
    ident = ops.icp_refine(src, src, iters=0)
    assert torch.equal(ident.R, torch.eye(3).expand(2, 3, 3)) and not ident.t.any()
    assert torch.equal(ident.idx, torch.arange(64, dtype=torch.int32).expand(2, 64)) and not ident.d2.any()


def test_predictor_icp_on_cpu():
    from pvraft_amd.engine import Predictor
    from pvraft_amd.model import PVRaft

    torch.manual_seed(3)
    model = PVRaft(truncate_k=16).eval()
    pred = Predictor(model, points=64, batch=1, iters=2)
    src, full, _ = ic.paired_lattice(256, seed=2)
    xyz1, xyz2 = src[:, :64], full[:, :64]
    flow, ego = pred.predict_ego_motion(xyz1, xyz2, thresh=0.05, iters=3)
    out = pred.predict_ego_motion(xyz1, xyz2, thresh=0.05, iters=3, icp=True,
                                  icp_kw={"iters": 2, "max_dist": 1.5}, target=full)
    assert len(out) == 3 and isinstance(out[2], ops.IcpRefine)
    want_ego = ops.ego_motion(xyz1, out[0], thresh=0.05, iters=3)
    want = ops.icp_refine(xyz1, full, R0=want_ego.R, t0=want_ego.t, src_mask=want_ego.static, iters=2, max_dist=1.5)
    for g, w in zip(out[2], want):
        assert torch.equal(g, w)
    assert out[2].idx.shape == (1, 64)
    # without a target the second cloud of the forward is refined against
    again = pred.predict_ego_motion(xyz1, xyz2, thresh=0.05, iters=3, icp=True)
    want = ops.icp_refine(xyz1, xyz2, R0=again[1].R, t0=again[1].t, src_mask=again[1].static)
    for g, w in zip(again[2], want):
        assert torch.equal(g, w)
