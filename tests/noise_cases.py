"""Shared inputs and an independent numpy oracle for the noise-filter tests
(CPU and GPU): ``ops.noise_filter`` written out from its definition in numpy
(NOT ops.reference) -- np.float32 operations one by one for the cells and d2,
np.partition and np.sort for the k smallest, np.sqrt on float32 (correctly rounded), a
left-to-right float32 sum, float64 two-pass statistics -- plus scene builders
and the checks both suites share.

All test coordinates are exact zeros or have |x / radius| >= 2**-100, so no
product is a denormal fp32 number (unspecified in the definition)."""

import numpy as np
import torch

RANGE = 1 << 20
FIELDS = ("keep", "count", "mean_dist", "mean", "std", "threshold", "ok")


def cells(x, radius, mask=None):
    """Eligibility (N,) bool and cells (N,3) int64 of one cloud."""
    x = np.asarray(x, dtype=np.float32)
    inv = np.float32(1) / np.float32(radius)
    with np.errstate(invalid="ignore", over="ignore"):
        q = np.floor(x * inv)  # float32 product, rounded once
        el = np.isfinite(x).all(-1) & (q >= -RANGE).all(-1) & (q < RANGE).all(-1)
    if mask is not None:
        el = el & np.asarray(mask, dtype=bool)
    c = np.where(el[:, None], q, 0).astype(np.int64)
    return el, c


def _cloud(x, radius, k, mask, chunk_pairs=1 << 21):
    """count (N,) int32, mean_dist (N,) float32 and eligibility of one cloud."""
    x = np.asarray(x, dtype=np.float32)
    N = x.shape[0]
    el, c = cells(x, radius, mask)
    r32 = np.float32(radius)
    r2 = r32 * r32
    count = np.full(N, -1, dtype=np.int32)
    md = np.full(N, np.inf, dtype=np.float32)
    ar = np.arange(N)
    c32 = c.astype(np.int32)  # |c| <= 2**20: exact
    chunk = max(1, chunk_pairs // max(N, 1))
    for s in range(0, N, chunk):
        e = min(N, s + chunk)
        with np.errstate(invalid="ignore", over="ignore"):
            dx = x[s:e, None, 0] - x[None, :, 0]
            dy = x[s:e, None, 1] - x[None, :, 1]
            dz = x[s:e, None, 2] - x[None, :, 2]
            d2 = (dx * dx + dy * dy) + dz * dz
            assert d2.dtype == np.float32
            nb = el[s:e, None] & el[None, :] & (d2 <= r2) & (ar[s:e, None] != ar[None, :])
            for a in range(3):  # max |c_i - c_j| <= 1, axis by axis
                nb &= np.abs(c32[s:e, None, a] - c32[None, :, a]) <= 1
        n = nb.sum(1)
        count[s:e] = np.where(el[s:e], n, -1)
        if k >= 1:
            cand = np.where(nb, d2, np.float32(np.inf))
            if N < k:
                cand = np.concatenate([cand, np.full((e - s, k - N), np.inf, np.float32)], 1)
            # the k smallest as a multiset (partition), then ascending (sort)
            small = np.sort(np.partition(cand, k - 1, axis=1)[:, :k], axis=1)
            with np.errstate(invalid="ignore"):
                root = np.sqrt(small)
                tot = root[:, 0].copy()
                for j in range(1, k):
                    tot = tot + root[:, j]
                m = tot / np.float32(k)
            assert m.dtype == np.float32
            md[s:e] = np.where(el[s:e] & (n >= k), m, np.float32(np.inf))
    return count, md, el


def oracle(xyz, radius=0.5, min_neighbors=4, k=8, std_ratio=2.0, mask=None):
    """dict of the seven fields of ``NoiseFilter`` as numpy arrays, plus el
    (B,N) bool, sparse, far (B,N) bool, from the definition."""
    xyz = xyz.numpy() if isinstance(xyz, torch.Tensor) else np.asarray(xyz)
    if mask is not None and isinstance(mask, torch.Tensor):
        mask = mask.numpy()
    B, N, _ = xyz.shape
    out = {
        "keep": np.zeros((B, N), bool), "count": np.zeros((B, N), np.int32),
        "mean_dist": np.zeros((B, N), np.float32), "mean": np.zeros(B), "std": np.zeros(B),
        "threshold": np.zeros(B), "ok": np.ones(B, bool), "el": np.zeros((B, N), bool),
        "sparse": np.zeros((B, N), bool), "far": np.zeros((B, N), bool),
    }
    for b in range(B):
        count, md, el = _cloud(xyz[b], radius, k, None if mask is None else mask[b])
        fin = np.isfinite(md)
        if k >= 1 and fin.any():
            m64 = md[fin].astype(np.float64)
            mean = m64.sum() / len(m64)
            std = np.sqrt(((m64 - mean) ** 2).sum() / len(m64))
            out["mean"][b], out["std"][b], out["threshold"][b] = mean, std, mean + std_ratio * std
        far = np.zeros(N, bool)
        if k >= 1:
            far = (count < k) | (md.astype(np.float64) > out["threshold"][b])
        sparse = count < min_neighbors
        out["count"][b], out["mean_dist"][b], out["el"][b] = count, md, el
        out["sparse"][b], out["far"][b] = sparse & el, far & el
        out["keep"][b] = el & ~sparse & ~far
    return out


def near_set(md, threshold, radius):
    """Points whose float64(mean_dist) is within 2e-9 * radius of the threshold."""
    with np.errstate(invalid="ignore"):
        return np.abs(md.astype(np.float64) - np.asarray(threshold)[:, None]) <= 2e-9 * radius


_ORACLES = {}


def scene_oracle(key, x, radius=0.5, min_neighbors=4, k=8, std_ratio=2.0, mask=None):
    """Oracle of a committed scene, computed once per (key, parameters); asserts
    that no point of the scene sits in the near set of the threshold, so keep
    can be compared exactly."""
    full = (key, radius, min_neighbors, k, std_ratio, mask is not None)
    if full not in _ORACLES:
        want = oracle(x, radius, min_neighbors, k, std_ratio, mask)
        if k >= 1:
            assert not near_set(want["mean_dist"], want["threshold"], radius).any(), f"{key}: near set not empty"
        _ORACLES[full] = want
    return _ORACLES[full]


def as_numpy(nf):
    return {f: getattr(nf, f).cpu().numpy() for f in FIELDS}


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.int32)


def check_exact(got, want, label=""):
    """count, mean_dist and ok, bit for bit, with dtypes and shapes."""
    for f, dt in (("count", np.int32), ("mean_dist", np.float32), ("ok", np.bool_), ("keep", np.bool_)):
        assert got[f].dtype == dt, f"{label}: {f} dtype {got[f].dtype}"
        assert got[f].shape == want[f].shape, f"{label}: {f} shape {got[f].shape} vs {want[f].shape}"
    for f in ("mean", "std", "threshold"):
        assert got[f].dtype == np.float64 and got[f].shape == want[f].shape, f"{label}: {f}"
    assert np.array_equal(got["ok"], want["ok"]), f"{label}: ok"
    bad = np.nonzero(got["count"] != want["count"])
    assert len(bad[0]) == 0, f"{label}: count differs at {bad[0][:5]}, {bad[1][:5]}"
    bad = np.nonzero(bits(got["mean_dist"]) != bits(want["mean_dist"]))
    assert len(bad[0]) == 0, (
        f"{label}: mean_dist bits differ at {bad[0][:5]}, {bad[1][:5]}: "
        f"{got['mean_dist'][bad][:5]} vs {want['mean_dist'][bad][:5]}")


def check_sparse(got, want, min_neighbors, label=""):
    """The sparse rule alone, for inputs whose sigma is degenerate."""
    el = got["count"] >= 0
    assert np.array_equal(el, want["el"]), f"{label}: eligibility"
    assert not got["keep"][~el].any() and not got["keep"][got["count"] < min_neighbors].any(), f"{label}: sparse kept"


def check(got, want, radius, min_neighbors, k, label=""):
    """Everything: the exact fields, the statistics within 1e-9 * radius, keep
    equal to the rule applied to the returned threshold, and keep equal to the
    oracle's outside the near set of the oracle's threshold."""
    check_exact(got, want, label)
    for f in ("mean", "std", "threshold"):
        err = np.abs(got[f] - want[f]).max() if got[f].size else 0.0
        print(f"{label}: max |{f} - oracle| = {err:.3e} (bound {1e-9 * radius:.3e})")
        assert err <= 1e-9 * radius, f"{label}: {f} off by {err}"
    el = got["count"] >= 0
    far = np.zeros_like(el)
    if k >= 1:
        far = (got["count"] < k) | (got["mean_dist"].astype(np.float64) > got["threshold"][:, None])
    rule = el & (got["count"] >= min_neighbors) & ~far
    assert np.array_equal(got["keep"], rule), f"{label}: keep is not the rule at the returned threshold"
    clear = ~near_set(want["mean_dist"], want["threshold"], radius) if k >= 1 else np.ones_like(el)
    assert np.array_equal(got["keep"][clear], want["keep"][clear]), f"{label}: keep differs from the oracle"


# ---------------------------------------------------------------------------
# scenes
# ---------------------------------------------------------------------------


def clustered(N, seed, spread=0.2):
    """Clusters of about 20 points (sigma ``spread``) with centres uniform in a
    16 m cube, every 16th point uniform in it instead: counts on both sides
    of min_neighbors and k at every N."""
    rng = np.random.default_rng(seed)
    nc = max(1, N // 20)
    centres = rng.uniform(-8.0, 8.0, size=(nc, 3))
    p = centres[rng.integers(0, nc, N)] + rng.normal(0.0, spread, size=(N, 3))
    lone = np.arange(N) % 16 == 5
    p[lone] = rng.uniform(-8.0, 8.0, size=(int(lone.sum()), 3))
    return p.astype(np.float32)


def scene(B, N, seed):
    """(B,N,3) float32 tensor of clustered clouds."""
    return torch.from_numpy(np.stack([clustered(N, seed * 131 + b) for b in range(B)]))


def coincident(N):
    return torch.full((1, N, 3), 1.25, dtype=torch.float32)


def lattice(n, spacing):
    """n^3 lattice with fp32 ``spacing`` around the origin: with spacing ==
    radius every point is on a cell face and every axis neighbour a d2 == r2
    tie."""
    g = (np.arange(n, dtype=np.float32) - np.float32(n // 2)) * np.float32(spacing)
    p = np.stack(np.meshgrid(g, g, g, indexing="ij"), -1).reshape(1, -1, 3)
    return torch.from_numpy(np.ascontiguousarray(p.astype(np.float32)))


def negative(N, seed):
    return torch.from_numpy(clustered(N, seed) - np.float32(60.0)).unsqueeze(0)


def faces(N, seed, radius=0.5):
    """A dense cloud around the origin with exact zeros and coordinates on
    cell faces on both sides: floor, not truncation."""
    rng = np.random.default_rng(seed)
    p = rng.uniform(-1.2, 1.2, size=(N, 3)).astype(np.float32)
    p[::7] = np.round(p[::7] / radius) * radius
    p[::11, 0] = 0.0
    p[::13] = 0.0
    p[5::17, 1] = -radius
    return torch.from_numpy(p).unsqueeze(0)


STENCIL_RADIUS = 0.37  # 1 / 0.37 is inexact in fp32: products round across cell faces


def stencil_edges(radius=STENCIL_RADIUS):
    """Rows of points along each axis at fp32(radius * n) and one and two ulps
    (a relative 2**-23) on either side, n = -40 .. 40 and around +-1024 and
    +-2048: neighbours at n +- 1 are a rounding error away from ``radius`` and
    from a cell face, so both conditions are decided by single roundings.
    Asserts that the scene holds pairs with d2 <= r2 whose cells are two apart
    (the stencil condition excludes them)."""
    ns = list(range(-40, 41))
    for c in (1024, 2048):
        ns += list(range(c - 2, c + 3)) + list(range(-c - 2, -c + 3))
    vals = []
    for n in ns:
        base = np.float32(np.float64(radius) * n)
        if n == 0:
            vals.append(base)  # no denormal coordinates
            continue
        for j in range(-2, 3):
            vals.append(np.float32(base + np.float32(j) * np.spacing(base)))
    v = np.asarray(vals, dtype=np.float32)
    a, b = np.full_like(v, 0.01), np.full_like(v, 0.02)
    p = np.concatenate([np.stack([v, a, b], -1), np.stack([b, v, a], -1), np.stack([a, b, v], -1)])
    el, c = cells(p, radius)
    d = p[:, None, :] - p[None, :, :]
    d2 = (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]
    r2 = np.float32(radius) * np.float32(radius)
    apart = np.abs(c[:, None, :] - c[None, :, :]).max(-1) >= 2
    assert el.all() and ((d2 <= r2) & apart).sum() > 0, "no in-radius pair two cells apart"
    return torch.from_numpy(p).unsqueeze(0)


def exact_k(k, seed, radius=0.5):
    """Well separated groups of k + 2, k + 1 and k points, every group inside a
    ball of radius / 4: counts of exactly k + 1, k and k - 1."""
    rng = np.random.default_rng(seed)
    pts = []
    g = 0
    for size in (k + 2, k + 1, k, k + 1, k):
        if size <= 0:
            continue
        centre = np.array([4.0 * radius * g + 0.1, -3.0 * radius * g, 0.3])
        pts.append(centre + rng.uniform(-radius / 8, radius / 8, size=(size, 3)))
        g += 1
    p = np.concatenate(pts).astype(np.float32)
    return torch.from_numpy(p[rng.permutation(len(p))]).unsqueeze(0)


def dirty(B, N, seed, radius=0.5):
    """Clustered clouds with duplicates, NaN / +-Inf rows and rows outside the
    +-2**20 cell range."""
    x = scene(B, N, seed).clone()
    x[:, 3] = x[:, 2]
    x[:, N // 2:N // 2 + 4] = x[:, 1:2]
    x[:, 5, 0] = float("nan")
    x[:, 6, 1] = float("inf")
    x[:, 7, 2] = float("-inf")
    x[:, 8, 0] = radius * (2.0 ** 20) * 1.01
    x[:, 9, 1] = -radius * (2.0 ** 20) * 1.01
    x[:, 10, 2] = 3.0e38
    return x


BAD_ROWS = [5, 6, 7, 8, 9, 10]


def patches_with_noise(N, seed, patches=60, noise_share=0.011):
    """The effect scene: ``patches`` planar 2 m x 2 m patches with 1 cm noise
    in a 40 x 6 x 40 m volume and a share of isolated points uniform in it.
    Returns the (N,3) float32 cloud and the (N,) bool mask of injected points."""
    rng = np.random.default_rng(seed)
    lo, hi = np.array([-20.0, -2.0, -20.0]), np.array([20.0, 4.0, 20.0])
    n_noise = int(round(noise_share * N))
    n_surf = N - n_noise
    centre = rng.uniform(lo + 1.0, hi - 1.0, size=(patches, 3))
    normal = rng.normal(size=(patches, 3))
    normal /= np.linalg.norm(normal, axis=1, keepdims=True)
    u = np.cross(normal, rng.normal(size=(patches, 3)))
    u /= np.linalg.norm(u, axis=1, keepdims=True)
    v = np.cross(normal, u)
    pid = rng.integers(0, patches, n_surf)
    a, b = rng.uniform(-1.0, 1.0, (2, n_surf))
    surf = centre[pid] + a[:, None] * u[pid] + b[:, None] * v[pid] + rng.normal(0.0, 0.01, (n_surf, 1)) * normal[pid]
    noise = rng.uniform(lo, hi, size=(n_noise, 3))
    p = np.concatenate([surf, noise]).astype(np.float32)
    injected = np.arange(N) >= n_surf
    order = rng.permutation(N)
    return p[order], injected[order]
