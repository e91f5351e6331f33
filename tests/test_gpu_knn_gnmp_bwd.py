"""GPU tests of the closed-form backward of the fused kNN-branch head
(csrc/knn_gnmp.hip): _C.knn_gnmp_fwd then _C.knn_gnmp_bwd, called directly
with a seeded dy, against the plain torch composition (conv -> group_norm
-> prelu) in float64 with autograd.  The reference pools with gather on the
op's own argmax, so near-ties cannot make the two sides pool different
elements, and it never uses the closed form.

Bound per gradient tensor (the rule of tests/test_gpu_ego_motion.py):
max|kernel - ref64| <= max(8 * max|ref32 - ref64|, 16 * 2^-23 * max|ref64|)
where ref32 is the same composition in fp32 on the same inputs.

Run with -m gpu (-s prints the largest deviations)."""

import functools

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

NAMES = ("d_raw", "dW", "dcb", "dgamma", "dbeta", "dslope")
EPS = 1e-5


@pytest.fixture(scope="module", autouse=True)
def _require_gpu_and_ext():
    if not torch.cuda.is_available():
        pytest.skip("needs GPU")
    import pvraft_amd.ops as ops

    assert ops.hip_available(), "HIP extension must be built on the GPU box"


def dev():
    return torch.device("cuda:0")


def _inputs(B, N, K, C, G, family, dy_dtype):
    g = torch.Generator(device="cpu").manual_seed(
        1000 * N + 10 * K + C + (7 if dy_dtype == torch.bfloat16 else 0))
    raw = torch.randn(B, 4, K, N, generator=g)
    if B > 1:
        raw[1] *= 3.0  # per-batch-element rstd must matter
    if family == "offset":
        raw += 5.0
    elif family == "row0x50":
        raw[:, 0] *= 50.0
    W = torch.randn(C, 4, generator=g) * 0.2
    cb = torch.randn(C, generator=g) * 0.1
    ga = torch.rand(C, generator=g) + 0.5
    be = torch.randn(C, generator=g) * 0.1
    sl = torch.tensor([0.25])
    dy = torch.randn(B, C, N, generator=g).to(dy_dtype)
    pre = [torch.randn(n, generator=g) for n in (C * 4, C, C, C, 1)]
    to = lambda t: t.to(dev()).contiguous()
    return (to(raw), to(W), to(cb), to(ga), to(be), to(sl), to(dy),
            [to(p) for p in pre])


def _reference(raw, W, cb, ga, be, sl, am, dy, G, dtype):
    """conv -> group_norm -> prelu -> gather on am; autograd in ``dtype``."""
    leaves = [t.detach().to(dtype).requires_grad_(True)
              for t in (raw, W, cb, ga, be, sl)]
    r, w, c, g, b, s = leaves
    x = F.conv2d(r, w.view(-1, 4, 1, 1), c)
    x = F.group_norm(x, G, g, b, EPS)
    x = F.prelu(x, s)
    idx = am.permute(0, 2, 1).long().unsqueeze(2)  # (B, C, 1, N)
    y = x.gather(2, idx).squeeze(2)
    y.backward(dy.to(dtype))
    return [t.grad.double().reshape(-1) for t in leaves]


@functools.lru_cache(maxsize=None)
def _case(B, N, K, C, G, family, dy_dtype):
    """Everything one case needs, computed once and shared (read-only)."""
    import pvraft_amd._C as _C

    raw, W, cb, ga, be, sl, dy_cm, pre = _inputs(B, N, K, C, G, family,
                                                 dy_dtype)
    _y, am, vsel, mean, rstd = _C.knn_gnmp_fwd(
        raw, W, cb, G, ga, be, EPS, sl, dy_dtype == torch.bfloat16, True)
    dy_pm = dy_cm.transpose(1, 2).contiguous()

    def bwd(dy, cm, targets=()):
        return _C.knn_gnmp_bwd(dy, raw, W, cb, am, vsel, mean, rstd, G, ga,
                               be, sl, EPS, cm, *targets)

    out = {
        "cm": bwd(dy_cm, True),
        "pm": bwd(dy_pm, False),
        "cm_again": bwd(dy_cm, True),
    }
    targets = [p.clone() for p in pre]
    out["acc"] = (bwd(dy_cm, True, targets), targets, pre)
    out["ref64"] = _reference(raw, W, cb, ga, be, sl, am, dy_cm, G,
                              torch.float64)
    out["ref32"] = _reference(raw, W, cb, ga, be, sl, am, dy_cm, G,
                              torch.float32)
    torch.cuda.synchronize()
    return out


# (B, N, K, C, G, input family): N in {1, 63, 65, 257, 311} (ragged tiles, a
# single point); K = 1 (every channel of a point lands in one slot), 5, 32
# and 255 (the largest the binding accepts); the minimum C and C/G = 4 and
# 8; B = 1 with N <= 256 is the shape at which equal-length workspaces
# aliased; B = 2 scales raw[1] by 3; "offset" (raw + 5) and "row0x50" probe
# the cancellation in the moment form.
CASES = [
    (2, 311, 32, 64, 8, "plain"),
    (1, 1, 5, 16, 2, "plain"),
    (2, 63, 1, 32, 8, "plain"),
    (1, 65, 255, 32, 8, "plain"),
    (1, 257, 5, 64, 8, "plain"),
    (2, 257, 32, 16, 2, "plain"),
    (1, 63, 32, 64, 8, "plain"),
    (2, 65, 5, 64, 8, "offset"),
    (2, 311, 32, 64, 8, "offset"),
    (2, 311, 32, 64, 8, "row0x50"),
    (1, 65, 255, 32, 8, "offset"),
]
DTYPES = [torch.float32, torch.bfloat16]


@pytest.mark.parametrize("dy_dtype", DTYPES, ids=["dy_fp32", "dy_bf16"])
@pytest.mark.parametrize("B,N,K,C,G,family", CASES)
def test_matches_float64_autograd(B, N, K, C, G, family, dy_dtype):
    """dslope is the delicate one: after the max-pool only a few hundred
    elements take the negative PReLU branch, so it is a small sum of terms
    near pre = 0 (0.02 in the row0x50 / bf16 case, bound 1.65e-07), where
    last-bit errors of the saved fp32 mean / rstd alone are 1.6e-07."""
    c = _case(B, N, K, C, G, family, dy_dtype)
    ref64, ref32 = c["ref64"], c["ref32"]
    fails = []
    for name, got, r64, r32 in zip(NAMES, c["cm"], ref64, ref32):
        err = (got.double().reshape(-1) - r64).abs().max().item()
        ref_err = (r32 - r64).abs().max().item()
        scale = r64.abs().max().item()
        bound = max(8.0 * ref_err, 16.0 * 2.0 ** -23 * scale)
        print(f"  {name:7s} |kernel-ref64|={err:.3e}  |ref32-ref64|="
              f"{ref_err:.3e}  max|ref64|={scale:.3e}  bound={bound:.3e}")
        assert torch.isfinite(got).all(), name
        if not err <= bound:
            fails.append((name, err, bound))
    assert not fails, fails


@pytest.mark.parametrize("dy_dtype", DTYPES, ids=["dy_fp32", "dy_bf16"])
@pytest.mark.parametrize("B,N,K,C,G,family", CASES)
def test_dy_layouts_and_repeat_calls_are_bit_equal(B, N, K, C, G, family,
                                                   dy_dtype):
    c = _case(B, N, K, C, G, family, dy_dtype)
    for name, a, b, again in zip(NAMES, c["cm"], c["pm"], c["cm_again"]):
        assert torch.equal(a, again), f"{name}: two calls differ"
        assert torch.equal(a, b), f"{name}: dy layouts differ"


@pytest.mark.parametrize("dy_dtype", DTYPES, ids=["dy_fp32", "dy_bf16"])
@pytest.mark.parametrize("B,N,K,C,G,family", CASES)
def test_accumulate_targets(B, N, K, C, G, family, dy_dtype):
    """Targets pre-filled with seeded values end as pre-fill + the
    returned-tensor mode's gradients, to one fp32 rounding of the sum."""
    c = _case(B, N, K, C, G, family, dy_dtype)
    ret, targets, pre = c["acc"]
    assert len(ret) == 1
    assert torch.equal(ret[0], c["cm"][0])
    for name, t, p, g in zip(NAMES[1:], targets, pre, c["cm"][1:]):
        want = p.double() + g.double().reshape(-1)
        err = (t.double() - want).abs()
        assert (err <= 2.0 ** -23 * want.abs()).all(), (name, err.max())
