"""Shared inputs and an independent float64 oracle for the ego-motion tests
(CPU and GPU): a driving-like scene generator, a few lines of
Kabsch-plus-Cauchy-IRLS in numpy float64 (NOT ops.reference.rigid_fit), and
the tolerance rule of the GPU tests."""

import numpy as np
import torch

TRUE_ROTVEC = (0.01, 0.03, -0.005)
TRUE_T = (0.1, -0.05, 1.0)
DYN_SHIFTS = ((1.2, 0.0, 0.4), (-0.8, 0.0, 0.9), (0.3, 0.1, -1.5))
EPS32 = float(np.finfo(np.float32).eps)

# (N, dyn, planar) of the robust-fit cases
ROBUST_CASES = [
    (64, 0.25, False), (300, 0.3, False), (2048, 0.3, False), (2048, 0.45, False),
    (8192, 0.3, False), (2048, 0.3, True),
]


def rotvec_matrix(v):
    """exp([v]x) by Rodrigues, float64 (3,3)."""
    v = np.asarray(v, dtype=np.float64)
    th = np.linalg.norm(v)
    if th == 0:
        return np.eye(3)
    k = v / th
    K = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
    return np.eye(3) + np.sin(th) * K + (1 - np.cos(th)) * (K @ K)


def rot_angle_deg(Ra, Rb):
    """Angle of Ra Rb^T in degrees; (3,3) or (B,3,3) arrays or tensors."""
    Ra = np.asarray(torch.as_tensor(Ra).double())
    Rb = np.asarray(torch.as_tensor(Rb).double())
    rel = Ra @ np.swapaxes(Rb, -1, -2)
    # atan2 of the skew part against the trace: accurate at small angles,
    # where acos of a rounded trace is not
    ax = 0.5 * np.stack([rel[..., 2, 1] - rel[..., 1, 2], rel[..., 0, 2] - rel[..., 2, 0],
                         rel[..., 1, 0] - rel[..., 0, 1]], -1)
    cos = (np.trace(rel, axis1=-2, axis2=-1) - 1) / 2
    return np.degrees(np.arctan2(np.linalg.norm(ax, axis=-1), cos))


def box_cloud(B, N, seed, planar=False):
    """Uniform points of a 30 x 4 x 30 m box centred at (0, 0, 20), float64."""
    rng = np.random.default_rng(seed)
    pc = (rng.random((B, N, 3)) - 0.5) * np.array([30.0, 4.0, 30.0]) + np.array([0.0, 0.0, 20.0])
    if planar:
        pc[..., 1] = 1.4
    return pc, rng


def make_scene(B, N, dyn, seed, planar=False):
    """One driving-like scene: static points follow the true motion with
    5 mm Gaussian noise, the first dyn * N points move in three groups with
    extra translations.  float32 tensors pc1, flow (B,N,3), static (B,N)
    bool, and the true motion R (3,3), t (3,) in float64."""
    pc, rng = box_cloud(B, N, seed, planar)
    R = rotvec_matrix(TRUE_ROTVEC)
    t = np.array(TRUE_T)
    flow = pc @ R.T + t - pc
    n_dyn = int(dyn * N)
    static = np.ones((B, N), dtype=bool)
    static[:, :n_dyn] = False
    flow += rng.normal(scale=0.005, size=flow.shape) * static[..., None]
    for g, shift in enumerate(DYN_SHIFTS):
        flow[:, g:n_dyn:3] += np.array(shift)
    return {
        "pc1": torch.from_numpy(pc).float(),
        "flow": torch.from_numpy(flow).float(),
        "static": torch.from_numpy(static),
        "R": R,
        "t": t,
    }


def rigid_pair(B, N, seed, R=None, t=None, noise=0.0, planar=False):
    """float32 (src, dst) with dst = R src + t (+ Gaussian noise) on the box
    cloud; R defaults to the true motion of ``make_scene``."""
    pc, rng = box_cloud(B, N, seed, planar)
    R = rotvec_matrix(TRUE_ROTVEC) if R is None else np.asarray(R, dtype=np.float64)
    t = np.array(TRUE_T) if t is None else np.asarray(t, dtype=np.float64)
    dst = pc @ R.T + t
    if noise:
        dst = dst + rng.normal(scale=noise, size=dst.shape)
    return torch.from_numpy(pc).float(), torch.from_numpy(dst).float()


def third_zero_weights(B, N, seed):
    """Random prior weights in (0.1, 1.1), a third of them zero."""
    rng = np.random.default_rng(seed + 77)
    w = rng.random((B, N)) + 0.1
    for b in range(B):
        w[b, rng.permutation(N)[: N // 3]] = 0.0
    return torch.from_numpy(w).float()


def _kabsch64(p, q, w):
    sw = w.sum()
    pm = (w[:, None] * p).sum(0) / sw
    qm = (w[:, None] * q).sum(0) / sw
    H = ((p - pm) * w[:, None]).T @ (q - qm)
    U, _, Vt = np.linalg.svd(H)
    D = np.diag([1.0, 1.0, np.sign(np.linalg.det(Vt.T @ U.T)) or 1.0])
    R = Vt.T @ D @ U.T
    return R, qm - R @ pm


def oracle_fit(src, dst, weights=None, thresh=0.05, iters=0):
    """float64 numpy oracle with the documented semantics of
    ``ops.rigid_fit``: returns R (B,3,3), t (B,3), residual (B,N), ok (B,)
    as float64 / bool arrays."""
    src = np.asarray(torch.as_tensor(src).double())
    dst = np.asarray(torch.as_tensor(dst).double())
    B, N, _ = src.shape
    prior = np.ones((B, N)) if weights is None else np.asarray(torch.as_tensor(weights).double())
    Rs, ts, rs, oks = [], [], [], []
    for b in range(B):
        fin = np.isfinite(src[b]).all(-1) & np.isfinite(dst[b]).all(-1)
        use = fin & np.isfinite(prior[b]) & (prior[b] > 0)
        p = np.where(fin[:, None], src[b], 0.0)
        q = np.where(fin[:, None], dst[b], 0.0)
        w0 = np.where(use, prior[b], 0.0)
        if use.sum() < 3:
            R = np.eye(3)
            t = (w0[:, None] * (q - p)).sum(0) / w0.sum() if use.any() else np.zeros(3)
            ok = False
        else:
            w = w0
            for k in range(iters + 1):
                R, t = _kabsch64(p, q, w)
                r = np.linalg.norm(p @ R.T + t - q, axis=-1)
                if k < iters:
                    w = w0 / (1.0 + (r / thresh) ** 2)
            ok = True
        r = np.linalg.norm(p @ R.T + t - q, axis=-1)
        Rs.append(R)
        ts.append(t)
        rs.append(np.where(fin, r, np.inf))
        oks.append(ok)
    return np.stack(Rs), np.stack(ts), np.stack(rs), np.array(oks)


def coord_scale(*tensors):
    """Largest finite |coordinate| of a case."""
    m = 0.0
    for x in tensors:
        x = torch.as_tensor(x).double()
        x = x[torch.isfinite(x)]
        if x.numel():
            m = max(m, x.abs().max().item())
    return m


def max_dev(got, want):
    """max |got - want| over the entries where ``want`` is finite; the
    non-finite entries must coincide."""
    got = np.asarray(torch.as_tensor(got).detach().cpu().double())
    want = np.asarray(want, dtype=np.float64)
    fin = np.isfinite(want)
    assert np.array_equal(fin, np.isfinite(got)), "finite / non-finite entries differ"
    assert np.array_equal(got[~fin], want[~fin]), "non-finite entries differ"
    return float(np.abs(got[fin] - want[fin]).max()) if fin.any() else 0.0


def bound(ref32, oracle, scale):
    """Tolerance of the GPU tests: eight times the deviation of the fp32 CPU
    reference from the oracle, floored at 16 ulp of the data."""
    return max(8.0 * max_dev(ref32, oracle), 16.0 * EPS32 * scale)
