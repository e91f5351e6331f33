"""Shared inputs and an independent float64 oracle for the moving-object
tests (CPU and GPU): lattice scene generators on which no pair of points sits
near a link threshold, a union-find over the explicit pair list in numpy
float64 with the canonical object order (NOT ops.reference.cluster_points),
and per-object fits through ego_cases.oracle_fit."""

import numpy as np
import torch

from ego_cases import DYN_SHIFTS, TRUE_ROTVEC, TRUE_T, box_cloud, max_dev, oracle_fit, rotvec_matrix

EPS = 0.5
FLOW_EPS = 0.1
CLEAR = 1e-4  # no pair within this relative distance of a squared threshold

SCENES = ("blobs", "chain", "broken_chain", "twin_chains", "ties", "overflow")


# ---------------------------------------------------------------------------
# oracle
# ---------------------------------------------------------------------------


def eligible(xyz, flow, mask):
    return mask & np.isfinite(xyz).all(-1) & np.isfinite(flow).all(-1)


def _pair_d2(x):
    d = x[:, None, :] - x[None, :, :]
    return (d * d).sum(-1)


def assert_clear(xyz, flow, mask, eps=EPS, flow_eps=FLOW_EPS):
    """Condition on the inputs: in float64, no pair of eligible points has
    |d^2 - eps^2| <= CLEAR * eps^2, in space or in flow.  Zero exceptions."""
    xyz = np.asarray(torch.as_tensor(xyz).double())
    flow = np.asarray(torch.as_tensor(flow).double())
    mask = np.asarray(torch.as_tensor(mask).bool())
    for b in range(xyz.shape[0]):
        el = eligible(xyz[b], flow[b], mask[b])
        iu = np.triu_indices(int(el.sum()), 1)
        for pts, e in ((xyz[b][el], eps), (flow[b][el], flow_eps)):
            if not np.isfinite(e):
                continue
            d2 = _pair_d2(pts)[iu]
            near = np.abs(d2 - e * e) <= CLEAR * e * e
            assert not near.any(), f"{int(near.sum())} pairs sit on the threshold {e}"


def oracle_cluster(xyz, flow, mask, eps=EPS, flow_eps=FLOW_EPS, min_points=8, max_objects=32):
    """labels (B,N), count (B,M), num_objects (B,) as int64 arrays: union-find
    over the explicit list of linked pairs, objects ordered by (size
    descending, smallest member ascending)."""
    xyz = np.asarray(torch.as_tensor(xyz).double())
    flow = np.asarray(torch.as_tensor(flow).double())
    mask = np.asarray(torch.as_tensor(mask).bool())
    B, N, _ = xyz.shape
    labels = np.full((B, N), -1, dtype=np.int64)
    count = np.zeros((B, max_objects), dtype=np.int64)
    nobj = np.zeros(B, dtype=np.int64)
    for b in range(B):
        el = eligible(xyz[b], flow[b], mask[b])
        ids = np.nonzero(el)[0]
        link = _pair_d2(xyz[b][ids]) <= eps * eps
        if np.isfinite(flow_eps):
            link &= _pair_d2(flow[b][ids]) <= flow_eps * flow_eps
        pi, pj = np.nonzero(np.triu(link, 1))
        parent = list(range(N))

        def find(x):
            while parent[x] != x:
                parent[x] = parent[parent[x]]
                x = parent[x]
            return x

        for i, j in zip(ids[pi].tolist(), ids[pj].tolist()):
            ri, rj = find(i), find(j)
            if ri != rj:
                parent[max(ri, rj)] = min(ri, rj)
        comps = {}
        for i in ids.tolist():
            comps.setdefault(find(i), []).append(i)
        objs = [m for m in comps.values() if len(m) >= min_points]
        objs.sort(key=lambda m: (-len(m), min(m)))
        for rank, members in enumerate(objs[:max_objects]):
            labels[b, members] = rank
            count[b, rank] = len(members)
        nobj[b] = min(len(objs), max_objects)
    return labels, count, nobj


def oracle_object_fits(src, dst, labels, num_segments, weights=None, thresh=0.05, iters=0):
    """R (B,M,3,3), t (B,M,3), residual (B,N), ok (B,M): ego_cases.oracle_fit
    on the members of every segment; labels outside [0, M) count as -1."""
    src = torch.as_tensor(src).double()
    dst = torch.as_tensor(dst).double()
    labels = np.asarray(torch.as_tensor(labels).long())
    B, N, _ = src.shape
    M = num_segments
    R = np.zeros((B, M, 3, 3))
    t = np.zeros((B, M, 3))
    ok = np.zeros((B, M), dtype=bool)
    res = np.full((B, N), np.inf)
    for b in range(B):
        for m in range(M):
            idx = np.nonzero(labels[b] == m)[0]
            w = None if weights is None else torch.as_tensor(weights)[b : b + 1, idx]
            Rm, tm, rm, okm = oracle_fit(src[b : b + 1, idx], dst[b : b + 1, idx], w, thresh, iters)
            R[b, m], t[b, m], ok[b, m] = Rm[0], tm[0], okm[0]
            res[b, idx] = rm[0]
    return R, t, res, ok


# ---------------------------------------------------------------------------
# lattice generators
# ---------------------------------------------------------------------------


def lattice_blob(n, origin, spacing):
    """First n points, in row-major order, of a 4 x 4 x k lattice: connected
    at link radius spacing / 0.8 for every n >= 1."""
    k = np.arange(n)
    ijk = np.stack([k % 4, (k // 4) % 4, k // 16], -1).astype(np.float64)
    return np.asarray(origin, dtype=np.float64) + spacing * ijk


def blob_origin(k):
    """Blob k of a scene: 8 m apart in x and y, so blobs of up to 16 layers
    keep gaps far above 2 eps."""
    return np.array([8.0 * (k % 6) - 20.0, 8.0 * (k // 6) - 8.0, 18.0])


def blob_flow(k, n, rng, flow_eps=FLOW_EPS):
    """Flow of blob k: a vector at least 2.5 flow_eps from every other blob's,
    plus a per-point offset of at most 0.35 flow_eps between any two points."""
    base = 2.5 * flow_eps * np.array([k % 5, (k // 5) % 5, k // 25], dtype=np.float64)
    return base + 0.2 * flow_eps * rng.integers(0, 2, size=(n, 3))


def _assemble(groups, N, rng, clutter=0):
    """groups: list of (xyz (n,3), flow (n,3)) of masked points.  Adds
    ``clutter`` isolated masked points, fills up to N with unmasked points in
    the middle of everything (they would link the blobs if the mask were
    ignored), shuffles the indices."""
    xyz = [g[0] for g in groups]
    flow = [g[1] for g in groups]
    n = sum(len(x) for x in xyz)
    clutter = max(0, min(clutter, N - n))
    if clutter:
        c = np.stack([3.0 * np.arange(clutter) - 20.0, np.full(clutter, -20.0), np.full(clutter, 18.0)], -1)
        xyz.append(c)
        flow.append(np.zeros((clutter, 3)))
    n += clutter
    assert n <= N, f"scene needs {n} points, N = {N}"
    mask = np.ones(N, dtype=bool)
    if N > n:
        xyz.append((rng.random((N - n, 3)) - 0.5) * np.array([50.0, 30.0, 8.0]) + np.array([0.0, 4.0, 20.0]))
        flow.append(np.zeros((N - n, 3)))
        mask[n:] = False
    xyz = np.concatenate(xyz) if xyz else np.zeros((0, 3))
    flow = np.concatenate(flow) if flow else np.zeros((0, 3))
    perm = rng.permutation(N)
    return xyz[perm], flow[perm], mask[perm]


def _sizes_blobs(N):
    if N <= 3:
        return [N]
    return [s for s in (int(0.35 * N), int(0.25 * N), int(0.12 * N), int(0.05 * N)) if s >= 1]


def _chain(n, y=0.0, x0=0.0, flow=(0.0, 0.0, 0.0)):
    xyz = np.stack([x0 + 0.9 * EPS * np.arange(n), np.full(n, y), np.full(n, 20.0)], -1)
    return xyz, np.tile(np.asarray(flow, dtype=np.float64), (n, 1))


def make_case(kind, B, N, seed=0):
    """One clustering case: float32 tensors xyz, flow (B,N,3), mask (B,N) and
    the op's keyword arguments.  The clearance assertion holds for every
    case by construction and is checked here."""
    kw = dict(eps=EPS, flow_eps=FLOW_EPS, min_points=8 if N >= 64 else 3, max_objects=32)
    out = []
    for b in range(B):
        rng = np.random.default_rng(1000 * seed + 17 * N + b)
        if kind == "blobs":
            groups = [(lattice_blob(n, blob_origin(k), 0.8 * EPS), blob_flow(k, n, rng))
                      for k, n in enumerate(_sizes_blobs(N))]
            out.append(_assemble(groups, N, rng, clutter=5 if N > 3 else 0))
        elif kind == "chain":
            out.append(_assemble([_chain(N)], N, rng))
        elif kind == "broken_chain":
            a = N // 3
            left, right = _chain(a), _chain(N - a, x0=0.9 * EPS * (a - 1) + 2.0 * EPS)
            out.append(_assemble([left, right], N, rng))
        elif kind == "twin_chains":
            a = (N + 1) // 2
            out.append(_assemble([_chain(a), _chain(N - a, y=0.1, flow=(2.0 * FLOW_EPS, 0.0, 0.0))], N, rng))
        elif kind == "ties":
            groups = [(lattice_blob(12, blob_origin(k), 0.8 * EPS), blob_flow(k, 12, rng)) for k in range(6)]
            out.append(_assemble(groups, N, rng, clutter=4))
        elif kind == "overflow":
            # seven objects for four slots, one blob at min_points, two just below
            kw.update(min_points=8, max_objects=4)
            sizes = [30, 9, 9, 20, 8, 7, 7, 14, 11]
            groups = [(lattice_blob(n, blob_origin(k), 0.8 * EPS), blob_flow(k, n, rng))
                      for k, n in enumerate(sizes)]
            out.append(_assemble(groups, N, rng, clutter=4))
        else:
            raise ValueError(kind)
    case = {
        "xyz": torch.from_numpy(np.stack([o[0] for o in out])).float(),
        "flow": torch.from_numpy(np.stack([o[1] for o in out])).float(),
        "mask": torch.from_numpy(np.stack([o[2] for o in out])),
        "kw": kw,
    }
    assert_clear(case["xyz"], case["flow"], case["mask"], kw["eps"], kw["flow_eps"])
    return case


# ---------------------------------------------------------------------------
# segmented-fit cases
# ---------------------------------------------------------------------------


def segment_labels(B, N, sizes, seed):
    """(B,N) int32 labels: segment m gets sizes[m] random points, the rest -1."""
    assert sum(sizes) <= N
    lab = np.full((B, N), -1, dtype=np.int32)
    for b in range(B):
        perm = np.random.default_rng(seed + b).permutation(N)
        o = 0
        for m, s in enumerate(sizes):
            lab[b, perm[o : o + s]] = m
            o += s
    return torch.from_numpy(lab)


# ---------------------------------------------------------------------------
# driving scene with three rigid boxes
# ---------------------------------------------------------------------------

BOX_DIMS = ((5, 5, 5), (6, 5, 4), (4, 4, 6))
BOX_ORIGINS = ((-9.0, -1.0, 12.0), (2.0, -0.5, 22.0), (8.0, -1.5, 30.0))
BOX_ROTVECS = ((0.0, 0.02, 0.0), (0.0, -0.015, 0.005), (0.01, 0.01, 0.0))
BOX_SPACING = 0.2
DRIVE_KW = dict(eps=EPS, flow_eps=0.25, min_points=8, max_objects=8)
NOISE = 0.005  # uniform, per component: bounded, so the clearance holds


def make_driving_scene(B, N, seed):
    """``ego_cases.make_scene``-like: static points of the box cloud follow
    the true ego-motion, the dynamic points are three rigid lattice boxes,
    each with its own motion on top (rotation about its centre, then one of
    DYN_SHIFTS).  Every flow carries bounded uniform noise.  Returns float32
    pc1, flow (noisy), clean_flow, static (B,N) bool, true labels (B,N)
    (boxes ranked by size as the op ranks them) and the true box motions
    R (3,3,3), t (3,3) as float64."""
    Re, te = rotvec_matrix(TRUE_ROTVEC), np.array(TRUE_T)
    boxes = []
    for dims, org in zip(BOX_DIMS, BOX_ORIGINS):
        g = np.stack(np.meshgrid(*[np.arange(d) for d in dims], indexing="ij"), -1).reshape(-1, 3)
        boxes.append(np.array(org) + BOX_SPACING * g)
    n_dyn = sum(len(x) for x in boxes)
    assert N > n_dyn + 16
    Rb, tb = [], []
    for x, rv, shift in zip(boxes, BOX_ROTVECS, DYN_SHIFTS):
        Ro, c = rotvec_matrix(rv), x.mean(0)
        # q = Ro (Re p + te - c') + c' + shift with c' = Re c + te
        c2 = Re @ c + te
        Rb.append(Ro @ Re)
        tb.append(Ro @ (te - c2) + c2 + np.array(shift))
    order = sorted(range(3), key=lambda k: -len(boxes[k]))
    pcs, flows, cleans, statics, labels = [], [], [], [], []
    for b in range(B):
        pc, rng = box_cloud(1, N - n_dyn, seed + b)
        pts = [pc[0]] + boxes
        lab = [np.full(N - n_dyn, -1)] + [np.full(len(boxes[k]), order.index(k)) for k in range(3)]
        clean = [pc[0] @ Re.T + te - pc[0]] + [x @ R.T + t - x for x, R, t in zip(boxes, Rb, tb)]
        pts, lab, clean = np.concatenate(pts), np.concatenate(lab), np.concatenate(clean)
        perm = rng.permutation(N)
        pts, lab, clean = pts[perm], lab[perm], clean[perm]
        pcs.append(pts)
        cleans.append(clean)
        flows.append(clean + (rng.random(clean.shape) - 0.5) * 2.0 * NOISE)
        labels.append(lab)
        statics.append(lab < 0)
    sc = {
        "pc1": torch.from_numpy(np.stack(pcs)).float(),
        "flow": torch.from_numpy(np.stack(flows)).float(),
        "clean_flow": torch.from_numpy(np.stack(cleans)).float(),
        "static": torch.from_numpy(np.stack(statics)),
        "labels": torch.from_numpy(np.stack(labels)),
        "R": np.stack([Rb[k] for k in order]),
        "t": np.stack([tb[k] for k in order]),
        "kw": dict(DRIVE_KW),
    }
    assert_clear(sc["pc1"], sc["flow"], ~sc["static"], DRIVE_KW["eps"], DRIVE_KW["flow_eps"])
    return sc


def check_driving_scene(sc, om, device_bound=None):
    """Assertions shared with the GPU test: true partition, each box's fit
    against the oracle fit of its points, lower EPE than the raw flow."""
    assert torch.equal(om.ego.static.cpu(), sc["static"])
    assert np.array_equal(om.labels.cpu().numpy(), sc["labels"].numpy())
    assert om.num_objects.cpu().tolist() == [3] * sc["pc1"].shape[0]
    M = sc["kw"]["max_objects"]
    assert om.count.cpu()[0].tolist() == [125, 120, 96] + [0] * (M - 3)
    assert om.ok.cpu()[:, :3].all() and not om.ok.cpu()[:, 3:].any()
    want = oracle_object_fits(sc["pc1"], sc["pc1"] + sc["flow"], sc["labels"], M, None, 0.05, 5)
    tol = device_bound if device_bound is not None else {"R": 1e-4, "t": 3e-3, "residual": 1e-4}
    errs = {"R": max_dev(om.R, want[0]), "t": max_dev(om.t, want[1]), "residual": max_dev(om.residual, want[2])}
    print("object fits vs oracle:", errs, "tolerance:", tol)
    for k in errs:
        assert errs[k] <= tol[k], (k, errs[k], tol[k])
    # the fits found the true box motions up to what the noise allows
    assert np.abs(want[0][:, :3] - sc["R"]).max() <= 5e-3
    clean = sc["clean_flow"]
    epe_raw = (sc["flow"] - clean).norm(dim=-1).mean().item()
    epe_rigid = (om.rigid_flow.cpu().float() - clean).norm(dim=-1).mean().item()
    print(f"EPE raw {epe_raw:.5f}  piecewise-rigid {epe_rigid:.5f}")
    assert epe_rigid < 0.5 * epe_raw
    return want
