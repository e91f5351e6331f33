"""GPU tests of the batched SetConv stage-1 kernels (csrc/edge_gnmp.hip):
_C.edge_gnmp_fwd then _C.edge_gnmp_bwd, called directly with a seeded dy,
against the plain torch composition (gather-diff -> group_norm -> act ->
pool over K) in float64 with autograd.  The reference pools with gather on
the op's own argmax, so near-ties cannot make the two sides pool different
elements, and it knows nothing of the closed forms or of the CSR walk.

Bound per tensor (the rule of tests/test_gpu_knn_gnmp_bwd.py):
max|kernel - ref64| <= max(8 * max|ref32 - ref64|, 16 * 2^-23 * max|ref64|)
where ref32 is the same composition in fp32 on the same inputs.  The op's
y and dwg come in the dtype of wg / dy; in the bf16 cases ref32 rounds
these two to bf16 as the op does (one rounding of the final value), so the
yardstick carries the output format's own error; the fp32 parameter
gradients are compared as they are.

Run with -m gpu (-s prints the largest deviations)."""

import functools

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

EPS = 1e-5
LRELU = 0.1
ACTS = {"none": 0, "lrelu": 1, "prelu": 2}
FWD_NAMES = ("y", "am", "vsel", "vsum", "mean", "rstd")


@pytest.fixture(scope="module", autouse=True)
def _require_gpu_and_ext():
    if not torch.cuda.is_available():
        pytest.skip("needs GPU")
    import pvraft_amd.ops as ops

    assert ops.hip_available(), "HIP extension must be built on the GPU box"


def dev():
    return torch.device("cuda:0")


def _graph(B, N, K, family, g):
    from pvraft_amd.model.graph import Graph

    xyz = torch.randn(B, N, 3, generator=g).to(dev())
    if family == "knn":
        return Graph.build(xyz, K)
    if family == "randint":  # duplicate slots inside a row
        idx = torch.randint(0, N, (B, N, K), generator=g)
    else:  # "hub": targets drawn from the lower half, so the upper half has
        # in-degree 0, except point N-1, which sits in slot 3 of every row
        # (in-degree N, far past the group size of the incoming walk)
        idx = torch.randint(0, N // 2, (B, N, K), generator=g)
        idx[:, :, 3] = N - 1
    return Graph(idx=idx.to(dev()), xyz=xyz)


def _reference(wg, idx, ga, be, sl, am, dy, G, act, dtype, out_dtype):
    """gather-diff -> group_norm -> act -> gather on am; autograd in
    ``dtype``, y and dwg rounded once to ``out_dtype``."""
    leaves = [t.detach().to(dtype).requires_grad_(True)
              for t in (wg, ga, be, sl)]
    w, g, b, s = leaves
    B, N, M = w.shape
    K = idx.shape[2]
    nb = w.gather(1, idx.reshape(B, N * K, 1).expand(B, N * K, M).long())
    edge = (nb.view(B, N, K, M) - w.unsqueeze(2)).permute(0, 3, 2, 1)
    x = F.group_norm(edge, G, g, b, EPS)  # (B, M, K, N)
    if act == "lrelu":
        x = F.leaky_relu(x, LRELU)
    elif act == "prelu":
        x = F.prelu(x, s)
    y = x.gather(2, am.permute(0, 2, 1).long().unsqueeze(2)).squeeze(2)
    y = y.transpose(1, 2)  # (B, N, M)
    y.backward(dy.to(dtype))
    rnd = lambda t: t.detach().to(out_dtype).double().reshape(-1)
    dsl = s.grad if s.grad is not None else torch.zeros_like(s)
    return {"y": rnd(y), "dwg": rnd(w.grad),
            "dgamma": g.grad.double().reshape(-1),
            "dbeta": b.grad.double().reshape(-1),
            "dslope": dsl.double().reshape(-1)}


@functools.lru_cache(maxsize=None)
def _case(B, N, K, M, G, act, family, dtype):
    """Everything one case needs, computed once and shared (read-only)."""
    import pvraft_amd._C as _C

    g = torch.Generator(device="cpu").manual_seed(
        1000 * N + 10 * K + M + len(act) + len(family)
        + (7 if dtype == torch.bfloat16 else 0))
    graph = _graph(B, N, K, family, g)
    idx = graph.idx32
    _order, offsets, order_n, order_j = graph.csr()
    wg = torch.randn(B, N, M, generator=g)
    if B > 1:
        wg[1] *= 3.0  # per-batch-element rstd must matter
    wg = wg.to(dev(), dtype)
    ga = torch.rand(M, generator=g) + 0.5
    ga[::3] *= -1  # negative gammas pool the lower extreme
    ga = ga.to(dev())
    be = (torch.randn(M, generator=g) * 0.1).to(dev())
    sl = torch.tensor([0.25]).to(dev())
    dy = torch.randn(B, N, M, generator=g).to(dev(), dtype)
    pre = [torch.randn(n, generator=g).to(dev()) for n in (M, M, 1)]
    a = ACTS[act]
    st = sl if a == 2 else None

    def fwd(classic):
        return _C.edge_gnmp_fwd(wg, idx, G, ga, be, EPS, a, LRELU, st, False,
                                classic)

    f = fwd(False)
    _y, am, vsel, vsum, mean, rstd = f

    def bwd(classic, targets=(None, None, None)):
        return _C.edge_gnmp_bwd(dy, wg, idx, am, vsel, vsum, offsets,
                                order_n, order_j, mean, rstd, G, ga, be, a,
                                LRELU, st, *targets, classic)

    out = {"fwd": f, "fwd_classic": fwd(True), "fwd_again": fwd(False),
           "bwd": bwd(False), "bwd_again": bwd(False),
           "bwd_classic": bwd(True)}
    targets = [p.clone() for p in pre]
    if a != 2:
        targets[2] = None
    out["acc"] = (bwd(False, targets), targets, pre)
    ref = lambda dt, odt: _reference(wg, idx, ga, be, sl, am, dy, G, act, dt,
                                     odt)
    out["ref64"] = ref(torch.float64, torch.float64)
    out["ref32"] = ref(torch.float32, dtype)
    torch.cuda.synchronize()
    return out


# (B, N, K, M, G): M = 48 and 96 give 12 and 24 threads per point (idle
# lanes in every block); no N is a multiple of the points per block; K = 20
# leaves a remainder after the groups of 8.  The last shape is not in the
# issue's list: K = 13 takes the forward's per-element index loads (rows of
# 13 ints are not 16-byte aligned) with one group and a remainder of 5.
SHAPES = [
    (2, 311, 16, 48, 8),
    (1, 257, 32, 96, 8),
    (2, 300, 32, 16, 8),
    (2, 311, 32, 64, 8),
    (1, 200, 20, 64, 8),
    (2, 67, 13, 16, 4),
]
FAMILIES = ["randint", "hub", "knn"]
DTYPES = [torch.float32, torch.bfloat16]

_params = lambda f: pytest.mark.parametrize("dtype", DTYPES, ids=["fp32", "bf16"])(
    pytest.mark.parametrize("family", FAMILIES)(
        pytest.mark.parametrize("act", list(ACTS))(
            pytest.mark.parametrize("B,N,K,M,G", SHAPES)(f))))


def _gathered(c, key, act):
    y = c["fwd"][0]
    dwg, dga, dbe, dsl = c[key]
    out = {"y": y, "dwg": dwg, "dgamma": dga, "dbeta": dbe}
    if act == "prelu":  # the slot is not written for the other two
        out["dslope"] = dsl
    return out


@_params
def test_matches_float64_autograd(B, N, K, M, G, act, family, dtype):
    c = _case(B, N, K, M, G, act, family, dtype)
    ref64, ref32 = c["ref64"], c["ref32"]
    fails = []
    for key in ("bwd", "bwd_classic"):
        for name, got in _gathered(c, key, act).items():
            r64, r32 = ref64[name], ref32[name]
            err = (got.double().reshape(-1) - r64).abs().max().item()
            ref_err = (r32 - r64).abs().max().item()
            scale = r64.abs().max().item()
            bound = max(8.0 * ref_err, 16.0 * 2.0 ** -23 * scale)
            print(f"  {key:11s} {name:6s} |kernel-ref64|={err:.3e}  "
                  f"|ref32-ref64|={ref_err:.3e}  max|ref64|={scale:.3e}  "
                  f"bound={bound:.3e}")
            assert torch.isfinite(got.float()).all(), name
            if not err <= bound:
                fails.append((key, name, err, bound))
    assert not fails, fails


@_params
def test_repeat_calls_are_bit_equal(B, N, K, M, G, act, family, dtype):
    c = _case(B, N, K, M, G, act, family, dtype)
    for name, a, b in zip(FWD_NAMES, c["fwd"], c["fwd_again"]):
        assert torch.equal(a, b), f"forward {name}: two calls differ"
    names = ("dwg", "dgamma", "dbeta", "dslope")
    for name, a, b in zip(names, c["bwd"], c["bwd_again"]):
        if name == "dslope" and act != "prelu":
            continue
        assert torch.equal(a, b), f"{name}: two calls differ"


@_params
def test_forward_equals_classic_bitwise(B, N, K, M, G, act, family, dtype):
    c = _case(B, N, K, M, G, act, family, dtype)
    for name, a, b in zip(FWD_NAMES, c["fwd"], c["fwd_classic"]):
        assert torch.equal(a, b), f"{name}: batched and classic differ"


@_params
def test_accumulate_targets(B, N, K, M, G, act, family, dtype):
    """Targets pre-filled with seeded values end as exactly the fp32 sum
    pre-fill + the returned-tensor mode's gradients."""
    c = _case(B, N, K, M, G, act, family, dtype)
    ret, targets, pre = c["acc"]
    assert len(ret) == 1
    assert torch.equal(ret[0], c["bwd"][0])
    for name, t, p, g in zip(("dgamma", "dbeta", "dslope"), targets, pre,
                             c["bwd"][1:]):
        if t is None:
            continue
        assert torch.equal(t, p + g.reshape(-1)), name


def test_env_toggle_selects_the_kernel_set(monkeypatch):
    """PVRAFT_EGNMP is read per call by the autograd wrapper; all settings
    give the same pooled output bit for bit and gradients within the
    accuracy bound's scale of each other."""
    import pvraft_amd.ops as ops

    B, N, K, M, G = 2, 311, 32, 64, 8
    g = torch.Generator(device="cpu").manual_seed(5)
    graph = _graph(B, N, K, "knn", g)
    wg0 = torch.randn(B, N, M, generator=g).to(dev())
    ga = (torch.rand(M, generator=g) + 0.5).to(dev())
    be = (torch.randn(M, generator=g) * 0.1).to(dev())
    dy = torch.randn(B, N, M, generator=g).to(dev())
    res = {}
    for mode, want in ((None, (False, False)), ("classic", (True, True)),
                       ("classic_fwd", (True, False)),
                       ("classic_bwd", (False, True))):
        if mode is None:
            monkeypatch.delenv("PVRAFT_EGNMP", raising=False)
        else:
            monkeypatch.setenv("PVRAFT_EGNMP", mode)
        assert ops.egnmp_classic() == want
        wg = wg0.clone().requires_grad_(True)
        y = ops.edge_gnmp(wg, graph.idx32, graph.csr(), G, ga, be, EPS,
                          act="lrelu", slope=LRELU)
        y.backward(dy)
        res[mode] = (y.detach(), wg.grad)
    for mode in ("classic", "classic_fwd", "classic_bwd"):
        assert torch.equal(res[mode][0], res[None][0]), mode
        scale = res[None][1].abs().max().item()
        err = (res[mode][1] - res[None][1]).abs().max().item()
        assert err <= 16.0 * 2.0 ** -23 * scale, (mode, err, scale)
