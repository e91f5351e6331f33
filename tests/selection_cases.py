"""Seeded inputs, exact float64 references and first-sweep witnesses for the
three threshold-selection kernels (kNN graph, fused correlation top-K, fp32
row top-K).  CPU only: nothing here touches the extension or a GPU, though
the references accept tensors on any device.

The kernels estimate a threshold (from a strided sample, or from histogram
rounds), collect against it into a fixed buffer and re-sweep when the count
comes out wrong.  On randn inputs in random order the first sweep always
lands; the cases here are built so that it does not: the points / columns
that the strided sample reads are displaced, so the sample misjudges the
rest of the data.  The witness functions replay only the documented sampling
rule on the exact reference and say how often, and on which side, the first
sweep misses its acceptance window."""

import math
import zlib

import numpy as np
import torch

# mirrors of csrc/knn_graph.hip: SAMP, CAP and the kp rule of knn_select_kernel
KNN_SAMP = 1024
KNN_CAP = 256
# mirrors of csrc/corr_topk.hip: CT_SAMP, CT_CAP and the rank rule of
# launch_corr_topk
CT_SAMP = 1024
CT_CAP = 704
# mirror of csrc/topk_rows.hip: TK_CAP (the smallest of the three buffers)
TK_CAP = 128
# no non-tie case may have a boundary tie group above this
MAX_TIE_GROUP = 64

TRANSLATION = (1000.0, -2000.0, 500.0)


def stride_of(n, samp=KNN_SAMP):
    return (n + samp - 1) // samp if n > samp else 1


# --------------------------------------------------------------- kNN clouds

def _family(rng, family, n):
    """(n, 3) float64 points of one distribution family."""
    if family == "gauss":
        return rng.standard_normal((n, 3))
    if family == "plane":
        p = rng.standard_normal((n, 3))
        p[:, 2] = 1e-3 * rng.standard_normal(n)
        return p
    if family == "line":
        t = rng.standard_normal(n)
        d = np.array([1.0, 2.0, 3.0]) / math.sqrt(14.0)
        return t[:, None] * d + 1e-5 * rng.standard_normal((n, 3))
    if family == "cluster":
        p = rng.random((n, 3))
        p[:600] = np.array([0.3, 0.6, 0.4]) + 1e-3 * rng.standard_normal((600, 3))
        return p[rng.permutation(n)]
    if family == "mixture":
        scales = np.array([1e-3, 1e-2, 1e-1, 1.0])
        centres = np.array([[0.0, 0.0, 0.0], [0.5, 0.0, 0.0], [0.0, -0.7, 0.2], [0.0, 0.0, 0.0]])
        which = rng.integers(0, 4, n)
        return centres[which] + scales[which, None] * rng.standard_normal((n, 3))
    raise ValueError(family)


def cloud(family, n, seed, order="random", translate=False):
    """One (n, 3) float32 cloud.  order: 'random', 'sorted' (by x, which makes
    point ids spatially coherent like a Morton relabel), 'far' (every st-th
    point, from index 0, replaced by a cluster at +100) or 'core' (every
    st-th point replaced by a dense core scaled by 1e-3)."""
    rng = np.random.default_rng(seed)
    p = _family(rng, family, n)
    if order == "sorted":
        p = p[np.argsort(p[:, 0], kind="stable")]
    elif order in ("far", "core"):
        st = stride_of(n)
        ns = len(range(0, n, st))
        if order == "far":
            p[::st] = 100.0 + rng.standard_normal((ns, 3))
        else:
            p[::st] = 1e-3 * rng.standard_normal((ns, 3))
    elif order != "random":
        raise ValueError(order)
    if translate:
        p = p + np.array(TRANSLATION)
    return torch.from_numpy(p.astype(np.float32))


# name -> (k, [(family, N, seed, order, translate) per batch element])
KNN_CASES = {
    # controls and unbiased orders
    "gauss_2048_random": (16, [("gauss", 2048, 1, "random", False)]),
    "gauss_4100_random": (32, [("gauss", 4100, 2, "random", False)]),
    "gauss_8192_random": (32, [("gauss", 8192, 3, "random", False)]),
    "gauss_2048_sorted": (32, [("gauss", 2048, 4, "sorted", False)]),
    "plane_8192_sorted": (32, [("plane", 8192, 5, "sorted", False)]),
    "line_4100_random": (16, [("line", 4100, 6, "random", False)]),
    "line_8192_sorted": (16, [("line", 8192, 7, "sorted", False)]),
    "cluster_8192_random": (32, [("cluster", 8192, 8, "random", False)]),
    "cluster_2048_sorted": (32, [("cluster", 2048, 9, "sorted", False)]),
    "mixture_8192_sorted": (32, [("mixture", 8192, 10, "sorted", False)]),
    "translated_8192_random": (32, [("gauss", 8192, 11, "random", True)]),
    "translated_4100_sorted": (16, [("gauss", 4100, 12, "sorted", True)]),
    "plane_mixture_2048_random": (32, [("plane", 2048, 13, "random", False),
                                       ("mixture", 2048, 14, "random", False)]),
    # stride-biased: the sampled points misrepresent the cloud
    "gauss_8192_far": (32, [("gauss", 8192, 20, "far", False)]),
    "gauss_8192_core": (32, [("gauss", 8192, 21, "core", False)]),
    "gauss_4100_far": (16, [("gauss", 4100, 22, "far", False)]),
    "plane_2048_far": (32, [("plane", 2048, 23, "far", False)]),
    "plane_4100_core": (32, [("plane", 4100, 24, "core", False)]),
    "line_4100_far": (32, [("line", 4100, 25, "far", False)]),
    "cluster_8192_far": (16, [("cluster", 8192, 26, "far", False)]),
    "cluster_8192_core": (16, [("cluster", 8192, 27, "core", False)]),
    "mixture_2048_far": (16, [("mixture", 2048, 28, "far", False)]),
    "mixture_4100_core": (32, [("mixture", 4100, 29, "core", False)]),
    "translated_8192_far": (32, [("gauss", 8192, 30, "far", True)]),
    "translated_4100_core": (32, [("gauss", 4100, 31, "core", True)]),
    "gauss_far_line_core_8192": (32, [("gauss", 8192, 32, "far", False),
                                      ("line", 8192, 33, "core", False)]),
}
KNN_CONTROLS = ["gauss_2048_random", "gauss_4100_random", "gauss_8192_random"]
KNN_BIASED = [n for n, (_, parts) in KNN_CASES.items()
              if all(p[3] in ("far", "core") for p in parts)]


def knn_case(name):
    """-> xyz (B, N, 3) float32, k."""
    k, parts = KNN_CASES[name]
    return torch.stack([cloud(*p[:4], translate=p[4]) for p in parts]), k


def sqdist_exact(xyz, q0, q1):
    """float64 squared distances of queries q0:q1 to every point, by explicit
    differences of the float32 inputs (no |a|^2+|b|^2-2ab, which cancels)."""
    x = xyz.double()
    return ((x[:, q0:q1, None, :] - x[:, None, :, :]) ** 2).sum(-1)


def knn_exact(xyz, k, chunk=512):
    """k smallest float64 squared distances per query, ascending: (B, N, k)."""
    n = xyz.shape[1]
    out = [sqdist_exact(xyz, s, min(s + chunk, n)).topk(k, dim=-1, largest=False).values
           for s in range(0, n, chunk)]
    return torch.cat(out, dim=1)


def knn_sample_rank(n, k):
    """Stride and sample rank of knn_select_kernel."""
    st = stride_of(n, KNN_SAMP)
    ns = (n + st - 1) // st
    kp = 2 * k if st == 1 else (4 * k + st - 1) // st
    return st, max(1, min(kp, ns))


def knn_witness(xyz, k, chunk=512):
    """First-sweep outcome of the kNN kernel from the exact distances: tau is
    the kp-th smallest distance to the strided sample, the window is
    k <= count(d <= tau) <= CAP.  Also the largest tie group at the k-th
    distance.  -> dict(under=frac, over=frac, max_tie=int)."""
    n = xyz.shape[1]
    st, kp = knn_sample_rank(n, k)
    under = over = 0
    max_tie = 0
    for s in range(0, n, chunk):
        d = sqdist_exact(xyz, s, min(s + chunk, n))
        tau = d[:, :, ::st].kthvalue(kp, dim=-1).values
        cnt = (d <= tau[..., None]).sum(-1)
        under += int((cnt < k).sum())
        over += int((cnt > KNN_CAP).sum())
        dk = d.kthvalue(k, dim=-1).values
        max_tie = max(max_tie, int((d == dk[..., None]).sum(-1).max()))
    tot = xyz.shape[0] * n
    return {"under": under / tot, "over": over / tot, "max_tie": max_tie}


# ------------------------------------------------------------- top-K rows

def _columns(rng, family, m):
    """Per-column magnitude s (m,) and shared additive offset o (m,), in
    units of the row sigma, of one row family."""
    s = np.ones(m)
    o = np.zeros(m)
    if family == "gauss" or family == "quantised":
        pass
    elif family == "lognormal":
        s = np.exp(3.0 * rng.standard_normal(m))
    elif family == "student":
        s = 1.0 / np.sqrt(rng.chisquare(2, m) / 2.0)
    elif family in ("peaks300", "peaks600"):
        s[:] = 0.01
        cols = rng.permutation(m)[: int(family[5:])]
        o[cols] = 5.0 + rng.standard_normal(len(cols))
    elif family == "block":
        a = m // 3
        o[a: a + 300] = 5.0
    elif family == "shelf":
        # 400 columns that the strided sample never reads, packed between
        # the two sample thresholds of a Gaussian row at M=8192, K=512
        # (P_lo ~ 1.33 sigma, P_hi ~ 1.77 sigma; sigma ~ 1.12 through the
        # GEMM): the band overflows while both thresholds are valid
        st = stride_of(m, CT_SAMP)
        cols = rng.permutation(np.flatnonzero(np.arange(m) % st == st // 2))[:400]
        s[cols] = 0.02
        o[cols] = 1.72
    elif family == "tiedshelf":
        # the same with 500 columns of ONE value (bitwise, also through the
        # GEMM: identical feature rows), placed where K=512 cuts the group
        # in most rows: a boundary tie group above half of CT_CAP that
        # still fits it
        st = stride_of(m, CT_SAMP)
        cols = rng.permutation(np.flatnonzero(np.arange(m) % st == st // 2))[:500]
        s[cols] = 0.0
        o[cols] = 1.8
    else:
        raise ValueError(family)
    return s, o


def _stride_shift(m, shift):
    """Offset of `shift` sigma on the columns the strided sample reads."""
    b = np.zeros(m)
    if shift:
        b[:: stride_of(m, CT_SAMP)] = shift
    return b


def rows(family, r, m, seed, shift=0.0):
    """(r, m) float32 rows for topk_rows: value = g * s_m + o_m + shift_m."""
    rng = np.random.default_rng(seed)
    s, o = _columns(rng, family, m)
    v = rng.standard_normal((r, m)) * s + o + _stride_shift(m, shift)
    if family == "quantised":
        # sigma 0.3 on a 1/16 grid: tie groups of about 200 at M=8192.  The
        # +0.0 turns -0.0 into +0.0, which the kernel's key order separates
        v = np.round(v * 0.3 * 16.0) / 16.0 + 0.0
    return torch.from_numpy(v.astype(np.float32))


def corr_features(family, n, m, c, seed, shift=0.0):
    """bf16 f1t (1, n, c), f2t (1, m, c) whose correlation rows follow
    `family`: f2[m] = g_m * s_m + 2 (o_m + shift_m) u with a shared unit
    direction u, f1[n] = h_n + a_n u with a_n = sqrt(c)/2 * U(0.95, 1.05), so
    f1[n].f2[m] / sqrt(c) = N(0, ~1.1) s_m + ~(o_m + shift_m): every row
    differs, all rows share the family and the stride bias."""
    rng = np.random.default_rng(seed)
    s, o = _columns(rng, family, m)
    u = rng.standard_normal(c)
    u /= np.linalg.norm(u)
    f2 = rng.standard_normal((m, c)) * s[:, None] + 2.0 * (o + _stride_shift(m, shift))[:, None] * u
    a = 0.5 * math.sqrt(c) * rng.uniform(0.95, 1.05, n)
    f1 = rng.standard_normal((n, c)) + a[:, None] * u
    to = lambda x: torch.from_numpy(x.astype(np.float32)).to(torch.bfloat16).unsqueeze(0)
    return to(f1), to(f2)


# name -> (family, M, K, shift in sigma on the sampled columns)
TOPK_CASES = {
    "gauss_8192_512": ("gauss", 8192, 512, 0.0),
    "gauss_1500_64": ("gauss", 1500, 64, 0.0),
    "gauss_1000_256": ("gauss", 1000, 256, 0.0),
    "gauss_4096_256": ("gauss", 4096, 256, 0.0),
    "gauss_8192_1024": ("gauss", 8192, 1024, 0.0),
    "lognormal_8192_1024": ("lognormal", 8192, 1024, 0.0),
    "lognormal_4096_256": ("lognormal", 4096, 256, 0.0),
    "student_8192_512": ("student", 8192, 512, 0.0),
    "peaks300_4096_256": ("peaks300", 4096, 256, 0.0),
    "peaks300_1500_512": ("peaks300", 1500, 512, 0.0),
    "peaks600_8192_512": ("peaks600", 8192, 512, 0.0),
    "block_4096_512": ("block", 4096, 512, 0.0),
    "gauss_8192_512_low1": ("gauss", 8192, 512, -1.0),
    "gauss_8192_512_low3": ("gauss", 8192, 512, -3.0),
    "gauss_8192_512_low10": ("gauss", 8192, 512, -10.0),
    "gauss_8192_512_high10": ("gauss", 8192, 512, 10.0),
    "gauss_4096_256_low3": ("gauss", 4096, 256, -3.0),
    "gauss_1500_64_low10": ("gauss", 1500, 64, -10.0),
    "gauss_1500_64_high10": ("gauss", 1500, 64, 10.0),
    "student_8192_512_low3": ("student", 8192, 512, -3.0),
}
# order-biased without a shift: see _columns
TOPK_CASES["shelf_8192_512"] = ("shelf", 8192, 512, 0.0)
# K <= 512 only: at K=1024 the expected band count is 616 +- 70 against a
# capacity of 704, so even randn rows overflow it now and then
TOPK_CONTROLS = ["gauss_8192_512", "gauss_1500_64", "gauss_1000_256", "gauss_4096_256"]
TOPK_BIASED = [n for n, c in TOPK_CASES.items() if c[3] != 0.0 or c[0] == "shelf"]
# explicit tie cases; a GEMM cannot realise a value grid, so only the tied
# shelf is also a correlation case
TIE_CASES = {
    "quantised_8192_512": ("quantised", 8192, 512, 0.0),
    "quantised_4096_256": ("quantised", 4096, 256, 0.0),
    "quantised_1500_64": ("quantised", 1500, 64, 0.0),
    "tiedshelf_8192_512": ("tiedshelf", 8192, 512, 0.0),
}
CORR_TIE_CASES = ["tiedshelf_8192_512"]
TOPK_ROWS_N = 64   # rows per fp32 case
CORR_ROWS_N = 96   # query rows per correlation case


def _case_seed(name):
    return zlib.crc32(name.encode())  # stable when cases are added


def topk_rows_case(name):
    """-> vals (R, M) float32, K."""
    family, m, k, shift = {**TOPK_CASES, **TIE_CASES}[name]
    return rows(family, TOPK_ROWS_N, m, _case_seed(name), shift), k


def corr_case(name):
    """-> f1t (1, N, C) bf16, f2t (1, M, C) bf16, K."""
    family, m, k, shift = {**TOPK_CASES, **TIE_CASES}[name]
    assert family != "quantised", "not realisable through a GEMM"
    c = 32 if m in (1500, 4096) else 128
    f1t, f2t = corr_features(family, CORR_ROWS_N, m, c, _case_seed(name), shift)
    return f1t, f2t, k


def corr_exact(f1t, f2t):
    """float64 product of the bf16 values times 1/sqrt(C): (B, N, M)."""
    c = f1t.shape[-1]
    return torch.bmm(f1t.double(), f2t.double().transpose(1, 2)) / math.sqrt(c)


def corr_error_bound(f1t, f2t):
    """Standard fp32 dot-product bound per entry: C 2^-24 scale sum|a||b|."""
    c = f1t.shape[-1]
    return torch.bmm(f1t.double().abs(), f2t.double().abs().transpose(1, 2)) * (
        c * 2.0 ** -24 / math.sqrt(c))


def topk_exact(vals, k):
    """K largest values per row, descending, and their indices."""
    return vals.topk(k, dim=-1)


def corr_sample_ranks(m, k):
    """Stride and the two sample ranks of launch_corr_topk."""
    st = stride_of(m, CT_SAMP)
    ns = (m + st - 1) // st
    if st == 1:
        return st, k, k
    q = k / st
    x = (-4.0 + math.sqrt(16.0 + 4.0 * q)) / 2.0
    kp_hi = int(x * x)
    x = (3.0 + math.sqrt(9.0 + 4.0 * q)) / 2.0
    kp_lo = int(x * x) + 1
    kp_hi = max(kp_hi, 1)
    if kp_lo <= kp_hi:
        kp_lo = kp_hi + 1
    kp_lo = min(kp_lo, ns)
    kp_hi = min(kp_hi, kp_lo)
    return st, kp_hi, kp_lo


def corr_witness(ref, k):
    """First-sweep outcome of the correlation kernel on exact rows (..., M):
    P_hi / P_lo are the kp_hi-th / kp_lo-th largest of the strided sample;
    the sweep fails over_hi when count(v > P_hi) > K, under when
    count(v >= P_lo) < K, over_bd when neither but the band
    count(P_lo <= v <= P_hi) exceeds CT_CAP.  Also the largest tie group at
    the K-th value.  -> dict of fractions and max_tie."""
    m = ref.shape[-1]
    r = ref.reshape(-1, m)
    st, kp_hi, kp_lo = corr_sample_ranks(m, k)
    samp = r[:, ::st].sort(dim=-1, descending=True).values
    p_hi = samp[:, kp_hi - 1: kp_hi]
    p_lo = samp[:, kp_lo - 1: kp_lo]
    chi = (r > p_hi).sum(-1)
    cov = (r >= p_lo).sum(-1)
    over_hi = chi > k
    under = ~over_hi & (cov < k)
    over_bd = ~over_hi & ~under & (cov - chi > CT_CAP)
    kth = r.topk(k, dim=-1).values[:, -1:]
    n = r.shape[0]
    return {"over_hi": int(over_hi.sum()) / n, "under": int(under.sum()) / n,
            "over_bd": int(over_bd.sum()) / n,
            "max_tie": int((r == kth).sum(-1).max())}
