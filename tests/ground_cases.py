"""Shared inputs and an independent numpy oracle for the ground-plane tests
(CPU and GPU): a LiDAR-like scene generator (tilted noisy ground, objects, a
vertical wall, a few points below the ground) and stages A-D of
``ops.fit_plane`` written out in numpy (NOT ops.reference): stages A and B
in np.uint64 / np.float32 elementwise arithmetic so the integers are exact,
stages C and D in float64 with np.linalg.eigh."""

import math

import numpy as np
import torch

EPS32 = float(np.finfo(np.float32).eps)
THRESH = 0.2
GAP = 1e-9  # documented eigenvalue separation of an accepted round
NEAR = 1e-4  # labels are compared outside |.| within NEAR of +-thresh

# N of the cases in which the oracle must find the true plane
FIND_SIZES = (64, 300, 1025, 4097)


def true_plane(tilt_deg, azimuth_deg=30.0, height=1.4):
    """Unit normal tilted ``tilt_deg`` off +y towards ``azimuth_deg`` and the
    offset of the plane that passes ``height`` below the origin."""
    t, a = math.radians(tilt_deg), math.radians(azimuth_deg)
    n = np.array([math.sin(t) * math.cos(a), math.cos(t), math.sin(t) * math.sin(a)])
    return n, height * n[1]  # n.(0,-height,0) + d = 0


def make_scene(B, N, seed, ground=0.4, wall=0.1, tilt_deg=None, below=0.01):
    """float32 xyz (B,N,3) plus the truth.  ``ground`` of the points lie on a
    plane tilted 3-8 degrees off +y with 2 cm Gaussian noise along the
    normal, ``wall`` on the vertical plane x = 8 (0-3 m above the ground),
    ``below`` 0.3-1 m under the ground, the rest on objects 0.3-3 m above it.
    Point order is shuffled.  Returns a dict with xyz, is_ground (B,N) bool,
    normal (3,), offset."""
    rng = np.random.default_rng(seed)
    tilt = float(rng.uniform(3.0, 8.0)) if tilt_deg is None else float(tilt_deg)
    n, d = true_plane(tilt, azimuth_deg=float(rng.uniform(0, 360)))
    n_g = int(round(ground * N))
    n_w = int(round(wall * N))
    n_b = int(round(below * N))
    n_o = N - n_g - n_w - n_b
    assert n_o >= 0
    out = np.empty((B, N, 3))
    is_ground = np.zeros((B, N), dtype=bool)
    for b in range(B):
        xz = rng.uniform(-20.0, 20.0, size=(N, 2))
        xz[n_g:n_g + n_w, 0] = 8.0
        # foot of every point on the plane: n.p + d = 0 solved for y
        y = -(d + n[0] * xz[:, 0] + n[2] * xz[:, 1]) / n[1]
        foot = np.stack([xz[:, 0], y, xz[:, 1]], -1)
        lift = np.empty(N)
        lift[:n_g] = rng.normal(scale=0.02, size=n_g)
        lift[n_g:n_g + n_w] = rng.uniform(0.0, 3.0, size=n_w)
        lift[n_g + n_w:n_g + n_w + n_b] = -rng.uniform(0.3, 1.0, size=n_b)
        lift[n_g + n_w + n_b:] = rng.uniform(0.3, 3.0, size=n_o)
        pts = foot + lift[:, None] * n
        pts[n_g:n_g + n_w, 0] = 8.0  # the wall is vertical: lift it along y only
        pts[n_g:n_g + n_w, 1] = y[n_g:n_g + n_w] + lift[n_g:n_g + n_w]
        pts[n_g:n_g + n_w, 2] = xz[n_g:n_g + n_w, 1]
        perm = rng.permutation(N)
        out[b] = pts[perm]
        is_ground[b] = perm < n_g
    return {
        "xyz": torch.from_numpy(out).float(),
        "is_ground": torch.from_numpy(is_ground),
        "normal": n,
        "offset": d,
    }


def collinear_cloud(B, N, seed):
    """Points of one horizontal line (y constant, general direction in the
    xz plane): the fp32 cross products of its triples are rounding noise along
    +-y, so some hypotheses are valid, every point is their inlier, and no
    refinement round can be accepted."""
    rng = np.random.default_rng(seed)
    s = rng.uniform(-15.0, 15.0, size=(B, N, 1))
    line = np.array([0.0, -1.4, 5.0]) + s * np.array([0.6, 0.0, 0.8])
    return torch.from_numpy(line).float()


def vertical_cloud(B, N, seed):
    """Only vertical structure: points of the wall x = 3."""
    rng = np.random.default_rng(seed)
    p = rng.uniform(-10.0, 10.0, size=(B, N, 3))
    p[..., 0] = 3.0
    return torch.from_numpy(p).float()


# ---------------------------------------------------------------------------
# oracle
# ---------------------------------------------------------------------------

_M32 = np.uint64(0xFFFFFFFF)


def _mix(x):
    x = np.asarray(x, dtype=np.uint64)
    x = x ^ (x >> np.uint64(16))
    x = (x * np.uint64(0x85EBCA6B)) & _M32
    x = x ^ (x >> np.uint64(13))
    x = (x * np.uint64(0xC2B2AE35)) & _M32
    return x ^ (x >> np.uint64(16))


def _params(thresh, up, max_tilt_deg):
    up = np.asarray(up, dtype=np.float64)
    up32 = (up / np.linalg.norm(up)).astype(np.float32)
    cos2 = np.float32(math.cos(math.radians(max_tilt_deg)) ** 2)
    thresh2 = np.float32(float(thresh) ** 2)
    return up32, cos2, thresh2


def _stage_ab(p, elig, H, seed, b, up32, cos2, thresh2):
    """One batch element: p (N,3) float32, elig (N,) bool -> idx (H,3),
    count (H,), n (H,3) f32, p0 (H,3) f32, nu (H,) f32."""
    N = p.shape[0]
    key = _mix(np.uint64(seed & 0xFFFFFFFF) ^ _mix((np.uint64(b) * np.uint64(0x9E3779B1) + np.uint64(1)) & _M32))
    idx = np.full((H, 3), -1, dtype=np.int64)
    valid = np.ones(H, dtype=bool)
    cand = (_mix(key ^ np.arange(H * 24, dtype=np.uint64)) % np.uint64(N)).astype(np.int64).reshape(H, 3, 8)
    for h in range(H):
        for j in range(3):
            for c in cand[h, j]:
                if elig[c]:
                    idx[h, j] = c
                    break
            if idx[h, j] < 0:
                valid[h] = False
        if len(set(idx[h])) < 3:
            valid[h] = False
    safe = np.where(valid[:, None], idx, 0)
    p0, p1, p2 = p[safe[:, 0]], p[safe[:, 1]], p[safe[:, 2]]
    u, v = p1 - p0, p2 - p0  # float32, one rounding per operation below
    nx = (u[:, 1] * v[:, 2]) - (u[:, 2] * v[:, 1])
    ny = (u[:, 2] * v[:, 0]) - (u[:, 0] * v[:, 2])
    nz = (u[:, 0] * v[:, 1]) - (u[:, 1] * v[:, 0])
    with np.errstate(all="ignore"):
        nn = (nx * nx + ny * ny) + nz * nz
        nu = (nx * up32[0] + ny * up32[1]) + nz * up32[2]
        valid &= np.isfinite(nn) & (nn > 0) & (nu * nu >= cos2 * nn)
        t2 = thresh2 * nn
        count = np.full(H, -1, dtype=np.int64)
        pe = p[elig]
        for h in np.nonzero(valid)[0]:
            e = ((pe[:, 0] - p0[h, 0]) * nx[h] + (pe[:, 1] - p0[h, 1]) * ny[h]) + (pe[:, 2] - p0[h, 2]) * nz[h]
            assert e.dtype == np.float32
            count[h] = int((e * e <= t2[h]).sum())
    idx[~valid] = -1
    return idx, count, np.stack([nx, ny, nz], -1), p0, nu


def oracle_hypotheses(xyz, mask=None, thresh=THRESH, hypotheses=256, up=(0.0, 1.0, 0.0), max_tilt_deg=20.0, seed=0):
    """idx (B,H,3), count (B,H) int64 arrays."""
    x = np.asarray(torch.as_tensor(xyz).float())
    up32, cos2, thresh2 = _params(thresh, up, max_tilt_deg)
    out_i, out_c = [], []
    for b in range(x.shape[0]):
        elig = np.isfinite(x[b]).all(-1)
        if mask is not None:
            elig &= np.asarray(mask[b]).astype(bool)
        i, c, _, _, _ = _stage_ab(x[b], elig, hypotheses, seed, b, up32, cos2, thresh2)
        out_i.append(i)
        out_c.append(c)
    return np.stack(out_i), np.stack(out_c)


def oracle_fit(xyz, mask=None, thresh=THRESH, hypotheses=256, up=(0.0, 1.0, 0.0), max_tilt_deg=20.0,
               refine_iters=3, seed=0):
    """float64 numpy oracle of ``ops.fit_plane``: a dict of arrays normal
    (B,3), offset (B,), height (B,N) float64 (unrounded), ground, inlier
    (B,N) bool from the float64 heights, count, best, rounds (B,) int, ok
    (B,) bool, idx (B,H,3), hyp_count (B,H)."""
    x = np.asarray(torch.as_tensor(xyz).float())
    B, N, _ = x.shape
    up32, cos2, thresh2 = _params(thresh, up, max_tilt_deg)
    upd = up32.astype(np.float64)
    res = {k: [] for k in ("normal", "offset", "height", "count", "best", "rounds", "ok", "idx", "hyp_count")}
    for b in range(B):
        fin = np.isfinite(x[b]).all(-1)
        elig = fin.copy()
        if mask is not None:
            elig &= np.asarray(mask[b]).astype(bool)
        idx, count, n32, p0, nu = _stage_ab(x[b], elig, hypotheses, seed, b, up32, cos2, thresh2)
        res["idx"].append(idx)
        res["hyp_count"].append(count)
        best = int(np.argmax(count))  # first maximum: the smallest h
        if count[best] < 0:
            res["normal"].append(upd.copy())
            res["offset"].append(0.0)
            res["height"].append(np.full(N, np.inf))
            res["count"].append(0)
            res["best"].append(-1)
            res["rounds"].append(0)
            res["ok"].append(False)
            continue
        n = n32[best].astype(np.float64)
        n = n / np.linalg.norm(n) * (-1.0 if nu[best] < 0 else 1.0)
        piv = p0[best].astype(np.float64)
        dp = 0.0
        q = np.where(fin[:, None], x[b], 0).astype(np.float64) - piv
        rounds = 0
        for _ in range(refine_iters):
            h = q @ n + dp
            w = np.where(elig & (np.abs(h) < thresh), (1.0 - (h / thresh) ** 2) ** 2, 0.0)
            W = w.sum()
            if (w > 0).sum() < 3 or not W > 0:
                break
            c = (w[:, None] * q).sum(0) / W
            qc = q - c
            C = (qc * w[:, None]).T @ qc
            lam, vec = np.linalg.eigh(C)
            m = vec[:, 0]
            if m @ upd < 0:
                m = -m
            if not (lam[1] - lam[0]) > GAP * lam[2]:
                break
            if (m @ upd) ** 2 < float(cos2):
                break
            n, dp = m, -(m @ c)
            rounds += 1
        h = q @ n + dp
        h = np.where(fin & np.isfinite(h), h, np.inf)
        res["normal"].append(n)
        res["offset"].append(dp - n @ piv)
        res["height"].append(h)
        res["count"].append(int(count[best]))
        res["best"].append(best)
        res["rounds"].append(rounds)
        res["ok"].append(True)
    out = {k: np.stack([np.asarray(v) for v in vals]) for k, vals in res.items()}
    out["ground"] = out["height"] <= thresh
    out["inlier"] = np.abs(out["height"]) <= thresh
    return out


def near_set(height, thresh=THRESH):
    """Points whose |height| lies within NEAR of the threshold: their labels
    may fall either way under rounding."""
    h = np.asarray(height, dtype=np.float64)
    with np.errstate(invalid="ignore"):
        return np.abs(np.abs(h) - thresh) < NEAR


def angle_deg(a, b):
    a = np.asarray(a, dtype=np.float64)
    b = np.asarray(b, dtype=np.float64)
    cr = np.linalg.norm(np.cross(a, b), axis=-1)
    return np.degrees(np.arctan2(cr, (a * b).sum(-1)))


def coord_scale(xyz):
    x = torch.as_tensor(xyz).double()
    x = x[torch.isfinite(x)]
    return float(x.abs().max()) if x.numel() else 0.0


def max_dev(got, want):
    """max |got - want| where ``want`` is finite; non-finite entries must
    coincide."""
    got = np.asarray(torch.as_tensor(got).detach().cpu().double())
    want = np.asarray(want, dtype=np.float64)
    fin = np.isfinite(want)
    assert np.array_equal(fin, np.isfinite(got)), "finite / non-finite entries differ"
    assert np.array_equal(got[~fin], want[~fin]), "non-finite entries differ"
    return float(np.abs(got[fin] - want[fin]).max()) if fin.any() else 0.0


def floor_bound(scale):
    """16 ulp of the data: what rounding an fp64 result to fp32 can cost."""
    return 16.0 * EPS32 * scale


def bound(ref32, oracle, scale):
    """Tolerance of the GPU tests: eight times the deviation of the fp32 CPU
    reference from the oracle, floored at 16 ulp of the data."""
    return max(8.0 * max_dev(ref32, oracle), floor_bound(scale))


def check_fit(got, want, ref=None, scale=1.0, label=""):
    """``got`` (a PlaneFit) against the oracle dict ``want``: integers equal,
    plane and heights within the bound (from ``ref``, the fp32 CPU reference,
    or the 16-ulp floor alone), labels equal outside the near set, which must
    hold at most 1 % of the points."""
    for name in ("best", "count", "rounds"):
        g = getattr(got, name).cpu().numpy()
        assert np.array_equal(g, want[name]), f"{label} {name}: {g} vs {want[name]}"
    assert np.array_equal(got.ok.cpu().numpy(), want["ok"]), f"{label} ok"
    for name, sc in (("normal", 1.0), ("offset", scale), ("height", scale)):
        b = floor_bound(sc) if ref is None else bound(getattr(ref, name), want[name], sc)
        e = max_dev(getattr(got, name), want[name])
        print(f"{label} {name}: |got - oracle| = {e:.3e}, bound = {b:.3e}")
        assert e <= b, f"{label} {name} off by {e:.3e} > {b:.3e}"
    near = near_set(want["height"])
    assert near.mean() <= 0.01, f"{label}: {near.mean():.3%} of the points sit on the threshold"
    for name in ("ground", "inlier"):
        g = getattr(got, name).cpu().numpy()
        assert g.dtype == bool and np.array_equal(g[~near], want[name][~near]), f"{label} {name}"
    assert got.height.dtype == torch.float32 and got.normal.dtype == torch.float32
    assert got.count.dtype == got.best.dtype == got.rounds.dtype == torch.int32
