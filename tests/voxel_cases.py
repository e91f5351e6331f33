"""Shared inputs and an independent numpy oracle for the voxel-sampling tests
(CPU and GPU): ``ops.voxel_sample`` written out from its definition in numpy
(NOT ops.reference) -- np.float32 for the one multiply, np.uint64 / np.int64
for everything after it, np.lexsort on (tag, key) per level -- plus scene
builders and the checks both suites share.

All test coordinates are exact zeros or have |x / voxel| >= 2**-100, so no
product is a denormal fp32 number (unspecified in the definition)."""

import numpy as np
import torch

RANGE = 1 << 20
M32 = np.uint64(0xFFFFFFFF)


def _mix32(x):
    x = x & M32
    x = x ^ (x >> np.uint64(16))
    x = (x * np.uint64(0x85EBCA6B)) & M32
    x = x ^ (x >> np.uint64(13))
    x = (x * np.uint64(0xC2B2AE35)) & M32
    return x ^ (x >> np.uint64(16))


def tags(b, N, seed):
    """uint64 tags (h << 32) | i of cloud b."""
    kb = _mix32(np.uint64(seed & 0xFFFFFFFF) ^ _mix32(np.uint64((b * 0x9E3779B1 + 1) & 0xFFFFFFFF)))
    i = np.arange(N, dtype=np.uint64)
    return (_mix32(kb ^ i) << np.uint64(32)) | i


def cells(x, voxel, mask=None):
    """Eligibility (N,) bool and level-0 cells (N,3) int64 of one cloud."""
    x = np.asarray(x, dtype=np.float32)
    inv = np.float32(1) / np.float32(voxel)
    with np.errstate(invalid="ignore", over="ignore"):
        q = np.floor(x * inv)  # float32 product, rounded once
        el = np.isfinite(x).all(-1) & (q >= -RANGE).all(-1) & (q < RANGE).all(-1)
    if mask is not None:
        el = el & np.asarray(mask, dtype=bool)
    c = np.where(el[:, None], q, 0).astype(np.int64)
    return el, c


def _key(c):
    return ((c[:, 0] + RANGE) << 42) | ((c[:, 1] + RANGE) << 21) | (c[:, 2] + RANGE)


def oracle(xyz, m, voxel=0.1, levels=10, mask=None, seed=0):
    """dict of idx (B,m) int64, count (B,) int32, rank (B,N) int32, occupied
    (B,levels) int32 plus el (B,N) bool, from the definition."""
    xyz = xyz.numpy() if isinstance(xyz, torch.Tensor) else np.asarray(xyz)
    if mask is not None and isinstance(mask, torch.Tensor):
        mask = mask.numpy()
    B, N, _ = xyz.shape
    idx = np.full((B, m), -1, dtype=np.int64)
    count = np.zeros(B, dtype=np.int32)
    rank = np.full((B, N), -1, dtype=np.int32)
    occ = np.zeros((B, levels), dtype=np.int32)
    els = np.zeros((B, N), dtype=bool)
    for b in range(B):
        el, c = cells(xyz[b], voxel, None if mask is None else mask[b])
        els[b] = el
        tag = tags(b, N, seed)
        rank[b, el] = 0
        alive = np.nonzero(el)[0]
        for lv in range(levels):
            key = _key(c[alive] >> lv)  # arithmetic shift: floors
            o = np.lexsort((tag[alive], key))  # by key, then by tag
            ks = key[o]
            first = np.ones(len(o), dtype=bool)
            first[1:] = ks[1:] != ks[:-1]
            alive = alive[o[first]]
            rank[b, alive] += 1
            occ[b, lv] = len(alive)
        ids = np.nonzero(el)[0]
        mp = min(m, len(ids))
        o = np.lexsort((tag[ids], -rank[b, ids].astype(np.int64)))
        idx[b, :mp] = np.sort(ids[o[:mp]])
        count[b] = mp
    return {"idx": idx, "count": count, "rank": rank, "occupied": occ, "el": els}


def cut_level(occupied, mp):
    """Smallest level l with occupied[l] <= m', or None."""
    for lv, o in enumerate(occupied):
        if o <= mp:
            return lv
    return None


def check_structure(got, xyz, m, voxel, levels, mask=None, seed=0, label=""):
    """Properties that follow from the definition, checked on ``got`` (numpy
    arrays under the four field names) without the oracle's selection."""
    xyz = xyz.numpy() if isinstance(xyz, torch.Tensor) else np.asarray(xyz)
    if mask is not None and isinstance(mask, torch.Tensor):
        mask = mask.numpy()
    B, N, _ = xyz.shape
    for b in range(B):
        el, c = cells(xyz[b], voxel, None if mask is None else mask[b])
        idx, cnt, rank, occ = got["idx"][b], int(got["count"][b]), got["rank"][b], got["occupied"][b]
        assert cnt == min(m, int(el.sum())), f"{label}: count"
        chosen = idx[:cnt]
        assert (idx[cnt:] == -1).all(), f"{label}: padding"
        assert (chosen >= 0).all() and (chosen < N).all() and (np.diff(chosen) > 0).all(), f"{label}: order"
        assert el[chosen].all(), f"{label}: ineligible point sampled"
        assert (rank[~el] == -1).all() and (rank[el] >= 0).all() and (rank <= levels).all(), f"{label}: rank range"
        assert (np.diff(occ) <= 0).all(), f"{label}: occupied increases"
        for lv in range(levels):
            assert occ[lv] == int((rank >= lv + 1).sum()), f"{label}: occupied[{lv}] vs rank histogram"
        # the guarantee, exactly: the representative of every eligible
        # point's level-l* cell is in idx
        ls = cut_level(occ, cnt)
        if ls is not None and cnt > 0:
            tag = tags(b, N, seed)
            ids = np.nonzero(el)[0]
            key = _key(c[ids] >> ls)
            o = np.lexsort((tag[ids], key))
            ks = key[o]
            first = np.ones(len(o), dtype=bool)
            first[1:] = ks[1:] != ks[:-1]
            reps = ids[o[first]]
            assert np.isin(reps, chosen).all(), f"{label}: a level-{ls} cell has no sample"
            assert (rank[reps] >= ls + 1).all(), f"{label}: representative rank"


def assert_equal(got, want, label=""):
    for k in ("idx", "count", "rank", "occupied"):
        g = got[k]
        g = g.cpu().numpy() if isinstance(g, torch.Tensor) else g
        assert g.dtype == want[k].dtype, f"{label}: {k} dtype {g.dtype}"
        assert g.shape == want[k].shape, f"{label}: {k} shape {g.shape} vs {want[k].shape}"
        assert np.array_equal(g, want[k]), f"{label}: {k} differs"


def as_numpy(vs):
    return {k: getattr(vs, k).cpu().numpy() for k in ("idx", "count", "rank", "occupied")}


# ---------------------------------------------------------------------------
# scenes
# ---------------------------------------------------------------------------


def lidar(N, seed):
    """LiDAR-like cloud: radius 2 + 33 u^2, uniform angle, height N(0, 0.6)."""
    rng = np.random.default_rng(seed)
    r = 2.0 + 33.0 * rng.random(N) ** 2
    a = rng.uniform(0.0, 2.0 * np.pi, N)
    y = rng.normal(0.0, 0.6, N)
    return np.stack([r * np.cos(a), y, r * np.sin(a)], -1).astype(np.float32)


def scene(B, N, seed):
    """(B,N,3) float32 tensor of LiDAR-like clouds."""
    return torch.from_numpy(np.stack([lidar(N, seed * 131 + b) for b in range(B)]))


def lattice(n=32):
    """n^3 integer lattice points (use with voxel = 1.0): structured keys,
    every point exactly on a cell boundary."""
    g = np.arange(n, dtype=np.float32) - n // 2
    p = np.stack(np.meshgrid(g, g, g, indexing="ij"), -1).reshape(1, -1, 3)
    return torch.from_numpy(np.ascontiguousarray(p))


def identical(N):
    return torch.full((1, N, 3), 1.25, dtype=torch.float32)


def distinct_cells(N, seed, voxel=0.1):
    """Every point in its own level-0 cell: a shuffled line of cell centres."""
    rng = np.random.default_rng(seed)
    i = rng.permutation(N).astype(np.float64) - N // 2
    p = np.stack([(i + 0.5) * voxel, np.full(N, 0.05), np.full(N, -0.05)], -1)
    return torch.from_numpy(p.astype(np.float32)).unsqueeze(0)


def straddle(N, seed):
    """A small cloud around the origin with exact zeros and cell-boundary
    values on both sides: floor, not truncate."""
    rng = np.random.default_rng(seed)
    p = rng.uniform(-0.45, 0.45, size=(N, 3)).astype(np.float32)
    p[::7] = np.round(p[::7] * 10) / 10  # near multiples of the voxel
    p[::11, 0] = 0.0
    p[::13] = 0.0
    p[5::17, 1] = -0.1
    return torch.from_numpy(p).unsqueeze(0)


def negative(N, seed):
    return torch.from_numpy(lidar(N, seed) - np.float32(60.0)).unsqueeze(0)


def dirty(B, N, seed, voxel=0.1):
    """LiDAR-like clouds with duplicates, NaN / +-Inf rows and rows outside
    the +-2**20 cell range."""
    x = scene(B, N, seed).clone()
    x[:, 3] = x[:, 2]
    x[:, N // 2:N // 2 + 4] = x[:, 1:2]
    x[:, 5, 0] = float("nan")
    x[:, 6, 1] = float("inf")
    x[:, 7, 2] = float("-inf")
    x[:, 8, 0] = voxel * (2.0 ** 20) * 1.01
    x[:, 9, 1] = -voxel * (2.0 ** 20) * 1.01
    x[:, 10, 2] = 3.0e38
    return x


def nn_distance(points, samples, chunk=2048):
    """Distance from every point to its nearest sample (float64)."""
    points = np.asarray(points, dtype=np.float64)
    samples = np.asarray(samples, dtype=np.float64)
    out = np.empty(len(points))
    s2 = (samples ** 2).sum(-1)
    for s in range(0, len(points), chunk):
        p = points[s:s + chunk]
        d2 = (p ** 2).sum(-1)[:, None] - 2.0 * p @ samples.T + s2[None]
        out[s:s + chunk] = np.sqrt(np.maximum(d2.min(1), 0.0))
    return out
