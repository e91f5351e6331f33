"""Shared inputs and independent numpy oracles for the grid-search and ICP
tests (CPU and GPU); NOT ops.reference.

``oracle_search`` is the definition of ``ops.nearest_in_radius`` by brute
force in numpy float32 (every numpy float32 operation is a single correctly
rounded one), with the gap between the best and the second-best candidate.
``oracle_icp`` is the loop of ``ops.icp_refine`` in float64 with
``ego_cases._kabsch64`` fits and a float64 brute-force search; it also reports
the smallest best / second-best gap it met, the precondition under which an
fp32 loop must choose the same correspondences."""

import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from ego_cases import TRUE_ROTVEC, TRUE_T, _kabsch64, rotvec_matrix  # noqa: E402

RANGE = float(1 << 20)
F32 = np.float32
PERTURB_ROTVEC = (0.002, -0.001, 0.0015)
PERTURB_T = (0.05, -0.03, 0.04)
MIN_GAP = 0.01  # m^2, see test_gpu_icp


def _np(x, dtype=None):
    if x is None:
        return None
    a = torch.as_tensor(x).detach().cpu().numpy()
    return a if dtype is None else a.astype(dtype)


def map32(x, R, t):
    """x' = ((R00*x + R01*y) + R02*z) + t0 ... in float32, op by op."""
    if R is None:
        return x
    R, t = R.astype(F32), t.astype(F32)
    return np.stack([((R[a, 0] * x[:, 0] + R[a, 1] * x[:, 1]) + R[a, 2] * x[:, 2]) + t[a] for a in range(3)], -1)


def cells32(x, inv, mask):
    with np.errstate(invalid="ignore", over="ignore"):
        q = np.floor(x * inv)
        el = np.isfinite(x).all(-1) & (q >= -RANGE).all(-1) & (q < RANGE).all(-1)
    if mask is not None:
        el = el & mask
    return el, np.where(el[:, None], q, 0).astype(np.int64)


def oracle_search(query, support, radius, query_mask=None, support_mask=None, R=None, t=None, chunk=256):
    """idx (B,Nq) int32, d2 (B,Nq) float32, gap (B,Nq) float64 (second-best
    minus best candidate d2; +INF with fewer than two candidates)."""
    query, support = _np(query, F32), _np(support, F32)
    qm, sm = _np(query_mask, bool), _np(support_mask, bool)
    R, t = _np(R, F32), _np(t, F32)
    B, Nq, _ = query.shape
    M = support.shape[1]
    r32 = F32(radius)
    inv, r2 = F32(1) / r32, r32 * r32
    idx = np.full((B, Nq), -1, np.int32)
    best = np.full((B, Nq), np.inf, F32)
    gap = np.full((B, Nq), np.inf)
    for b in range(B):
        with np.errstate(invalid="ignore", over="ignore"):
            x = map32(query[b], None if R is None else R[b], None if t is None else t[b])
        elq, cq = cells32(x, inv, None if qm is None else qm[b])
        els, cs = cells32(support[b], inv, None if sm is None else sm[b])
        s = support[b]
        for lo in range(0, Nq, chunk):
            hi = min(Nq, lo + chunk)
            cand = elq[lo:hi, None] & els[None, :]
            cand &= (np.abs(cq[lo:hi, None, :] - cs[None, :, :]) <= 1).all(-1)
            with np.errstate(invalid="ignore", over="ignore"):
                dx = x[lo:hi, None, 0] - s[None, :, 0]
                dy = x[lo:hi, None, 1] - s[None, :, 1]
                dz = x[lo:hi, None, 2] - s[None, :, 2]
                d2 = (dx * dx + dy * dy) + dz * dz
                cand &= d2 <= r2
            d2 = np.where(cand, d2, F32(np.inf))
            if M == 0:
                continue
            j = np.argmin(d2, 1)  # numpy: the first of equal minima
            m = d2[np.arange(hi - lo), j]
            found = np.isfinite(m)
            idx[b, lo:hi] = np.where(found, j, -1)
            best[b, lo:hi] = np.where(found, m, np.inf)
            if M >= 2:
                two = np.partition(d2.astype(np.float64), 1, axis=1)[:, :2]
                with np.errstate(invalid="ignore"):
                    gap[b, lo:hi] = np.where(np.isfinite(two[:, 1]), two[:, 1] - two[:, 0], np.inf)
    return idx, best, gap


def search64(x, s, max_dist):
    """float64 brute force for one cloud: idx, d2 (inf without a match) and
    the gap to the second-nearest support point of all."""
    idx = np.full(len(x), -1, np.int64)
    d2 = np.full(len(x), np.inf)
    gap = np.full(len(x), np.inf)
    for lo in range(0, len(x), 512):
        d = ((x[lo:lo + 512, None, :] - s[None, :, :]) ** 2).sum(-1)
        j = np.argmin(d, 1)
        m = d[np.arange(len(j)), j]
        ok = m <= max_dist * max_dist
        idx[lo:lo + 512] = np.where(ok, j, -1)
        d2[lo:lo + 512] = np.where(ok, m, np.inf)
        if s.shape[0] >= 2:
            two = np.partition(d, 1, axis=1)[:, :2]
            gap[lo:lo + 512] = np.where(ok, two[:, 1] - two[:, 0], np.inf)
    return idx, d2, gap


def oracle_icp(src, dst, R0=None, t0=None, max_dist=1.0, thresh=0.1, iters=10, src_mask=None):
    """float64 loop of ``ops.icp_refine`` for finite clouds.  Returns a dict:
    R (B,3,3), t (B,3), idx (B,N), d2 (B,N), matched, rounds, ok, and min_gap,
    the smallest best / second-best gap over all searches and points."""
    src, dst = _np(src, np.float64), _np(dst, np.float64)
    B, N, _ = src.shape
    R0, t0, sm = _np(R0, np.float64), _np(t0, np.float64), _np(src_mask, bool)
    out = {k: [] for k in ("R", "t", "idx", "d2", "matched", "rounds", "ok")}
    min_gap = np.inf
    for b in range(B):
        R = np.eye(3) if R0 is None else R0[b]
        t = np.zeros(3) if t0 is None else t0[b]
        use = np.ones(N, bool) if sm is None else sm[b]
        rounds, ok = 0, True
        for k in range(iters + 1):
            idx, d2, gap = search64(src[b] @ R.T + t, dst[b], max_dist)
            idx, d2 = np.where(use, idx, -1), np.where(use, d2, np.inf)
            if use.any():
                min_gap = min(min_gap, gap[use].min())
            if k == iters:
                break
            f = idx >= 0
            if f.sum() < 3:
                ok = False
                break
            w = 1.0 / (1.0 + d2[f] / thresh ** 2)
            R, t = _kabsch64(src[b][f], dst[b][idx[f]], w)
            rounds += 1
        for name, v in zip(out, (R, t, idx, d2, int((idx >= 0).sum()), rounds, ok)):
            out[name].append(v)
    res = {k: np.stack(v) if k in ("R", "t", "idx", "d2") else np.array(v) for k, v in out.items()}
    res["min_gap"] = float(min_gap)
    return res


def true_motion():
    return rotvec_matrix(TRUE_ROTVEC), np.array(TRUE_T)


def start_motion(B=1):
    """The true motion perturbed by PERTURB_ROTVEC and PERTURB_T, float32
    tensors (B,3,3), (B,3)."""
    R, t = true_motion()
    R0 = rotvec_matrix(PERTURB_ROTVEC) @ R
    t0 = t + np.array(PERTURB_T)
    return (torch.from_numpy(np.repeat(R0[None], B, 0)).float(), torch.from_numpy(np.repeat(t0[None], B, 0)).float())


def paired_lattice(N, seed, B=1):
    """src: N nodes of a 1 m lattice in the 30 x 4 x 30 m box of ego_cases,
    jittered by +-0.2 m; dst = R src + t + 5 mm Gaussian noise, permuted.
    float32 tensors src (B,N,3), dst (B,N,3) and perm (B,N) with dst[perm[i]]
    the partner of src[i]."""
    rng = np.random.default_rng(seed)
    gx, gy, gz = np.meshgrid(np.arange(30), np.arange(4), np.arange(30), indexing="ij")
    nodes = np.stack([gx, gy, gz], -1).reshape(-1, 3) + 0.5 - np.array([15.0, 2.0, 15.0]) + np.array([0.0, 0.0, 20.0])
    assert N <= len(nodes)
    R, t = true_motion()
    srcs, dsts, perms = [], [], []
    for _ in range(B):
        p = nodes[rng.permutation(len(nodes))[:N]] + (rng.random((N, 3)) - 0.5) * 0.4
        q = p @ R.T + t + rng.normal(scale=0.005, size=p.shape)
        perm = rng.permutation(N)  # partner of src i sits at dst[perm[i]]
        d = np.empty_like(q)
        d[perm] = q
        srcs.append(p), dsts.append(d), perms.append(perm)
    return (torch.from_numpy(np.stack(srcs)).float(), torch.from_numpy(np.stack(dsts)).float(),
            torch.from_numpy(np.stack(perms)))


def resampled_surface(seed, n_src=2048, n_dst=16384, patches=20):
    """src: n_src samples of 20 planar 6 x 6 m patches in the box; dst: n_dst
    OTHER samples of the same patches moved by the true motion.  float32
    tensors (1,n,3)."""
    rng = np.random.default_rng(seed)
    R, t = true_motion()
    centre = (rng.random((patches, 3)) - 0.5) * np.array([30.0, 4.0, 30.0]) + np.array([0.0, 0.0, 20.0])
    u = rng.normal(size=(patches, 3))
    u /= np.linalg.norm(u, axis=1, keepdims=True)
    v = np.cross(u, rng.normal(size=(patches, 3)))
    v /= np.linalg.norm(v, axis=1, keepdims=True)

    def sample(n):
        k = rng.integers(0, patches, n)
        a = (rng.random((n, 2)) - 0.5) * 6.0
        return centre[k] + a[:, :1] * u[k] + a[:, 1:] * v[k]

    src = sample(n_src)
    dst = sample(n_dst) @ R.T + t
    return torch.from_numpy(src[None]).float(), torch.from_numpy(dst[None]).float()


def random_pair(B, Nq, M, seed, radius=0.5):
    """Uniform clouds in a cube that gives a cell of edge ``radius`` about one
    support point: most queries have a few candidates, some none."""
    rng = np.random.default_rng(seed)
    L = max(1.0, M ** (1.0 / 3.0)) * radius
    q = (rng.random((B, Nq, 3)) - 0.5) * L
    s = (rng.random((B, M, 3)) - 0.5) * L
    return torch.from_numpy(q).float(), torch.from_numpy(s).float()


def small_motion(B, seed):
    """A rotation of about 0.1 rad and a shift of a cell, float32 tensors."""
    rng = np.random.default_rng(seed)
    R = np.stack([rotvec_matrix(rng.normal(scale=0.06, size=3)) for _ in range(B)])
    t = rng.normal(scale=0.3, size=(B, 3))
    return torch.from_numpy(R).float(), torch.from_numpy(t).float()


def check_search(got, want, label=""):
    """got: an ops.NearestInRadius (any device); want: oracle_search output."""
    idx, d2 = got.idx.cpu().numpy(), got.d2.cpu().numpy()
    assert idx.dtype == np.int32 and d2.dtype == np.float32 and got.ok.dtype == torch.bool
    bad = np.flatnonzero((idx != want[0]).ravel())
    assert bad.size == 0, f"{label}: {bad.size} idx differ, first at {bad[:5]}: {idx.ravel()[bad[:5]]} vs {want[0].ravel()[bad[:5]]}"
    assert np.array_equal(d2.view(np.int32), want[1].view(np.int32)), f"{label}: d2 bits differ"
    assert bool(got.ok.all()), f"{label}: ok is False"


def stencil_scene():
    """``noise_cases.stencil_edges``: points a rounding error away from the
    cell faces and from ``radius`` of each other, negative coordinates
    included.  Returns (points (1,P,3), radius, (i, j)) with i, j one pair with
    d2 <= r2 in fp32 whose cells are two apart: it must NOT match."""
    import noise_cases as nc

    radius = nc.STENCIL_RADIUS
    p = nc.stencil_edges(radius)
    x = p[0].numpy()
    r32 = F32(radius)
    _, c = cells32(x, F32(1) / r32, None)
    d = x[:, None, :] - x[None, :, :]
    d2 = (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]
    apart = np.abs(c[:, None, :] - c[None, :, :]).max(-1) >= 2
    i, j = np.argwhere((d2 <= r32 * r32) & apart)[0]
    return p, radius, (int(i), int(j))
