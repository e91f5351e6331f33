"""pw_fused / PwConv1d / the GRU cell through autograd: the fused data
gradient (csrc/pw_bwd.hip) against PVRAFT_PW_BWD=classic, and the row-split
fast path against its concatenating fallback.

dx bound (see tests/test_gpu_pw_bwd.py):
    |dx - ref| <= 2^-7 |ref| + 2^-16 sum_o |W[o,c]| |dpre[o,s]|
with ref the float64 gradient on the bf16-rounded operands.
"""

import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = "cuda"


def _bound_ok(dx, w_bf, dpre, what):
    ref = torch.einsum("oc,bos->bcs", w_bf.double(), dpre.double())
    mag = torch.einsum("oc,bos->bcs", w_bf.double().abs(), dpre.double().abs())
    worst = ((dx.double() - ref).abs() - (2.0 ** -7 * ref.abs() + 2.0 ** -16 * mag)).max()
    assert worst.item() <= 0.0, f"{what}: over the bound by {worst.item():.3e}"


def _wgrad_partials(B, Co, Ci, S):
    """How many fp32 partial tiles pw_wgrad folds into one dW element with
    atomicAdd: B * schunks, schunks as launch_pw_wgrad (csrc/pw_wgrad.hip)
    picks it (64x64 output tiles, 32-wide K blocks, >= 4 K blocks a chunk)."""
    tiles = -(-Co // 64) * -(-Ci // 64)
    sc = max(1, min(512 // (tiles * B) + 1, S // (32 * 4)))
    return B * sc


def _wgrad_close(a, b, dpre, x, what, bias=False, ci=None):
    """Two pw_wgrad results on bit-equal operands.  The issue expected them
    exactly equal with deferral off; they are only where one partial makes
    up the sum.  Each partial tile is a fixed MFMA sum, but the P partials
    are folded with fp32 atomicAdd in whatever order the workgroups arrive
    (the bias sum folds 4 LDS partials per workgroup the same way: 4P).  A
    sum of P fp32 terms in any order is within (P-1) 2^-24 sum|terms| of the
    exact one, so two orders differ by at most twice that; sum|terms| <=
    sum|dpre||x| (1 + 2^-10, the partials' own rounding).  P = 1: equal."""
    B, Co, S = dpre.shape
    P = _wgrad_partials(B, Co, ci or x.shape[1], S) * (4 if bias else 1)
    if P == 1:
        assert torch.equal(a, b), f"{what}: one partial, must be exactly equal"
        return
    mag = torch.einsum("bos,bis->oi", dpre.double().abs(), x.double().abs())
    bound = 2 * (P - 1) * 2.0 ** -24 * (1 + 2.0 ** -10) * mag
    worst = ((a.double() - b.double()).abs() - bound).max().item()
    assert worst <= 0.0, f"{what}: wgrads differ by more than summation order ({worst:.3e})"


def _stack(cis, Co, B, S, seed, sliced):
    g = torch.Generator(device=DEV).manual_seed(seed)
    if sliced:
        wide = (torch.randn(Co, sum(cis), device=DEV, generator=g) * 0.2).requires_grad_()
        lo, ws = 0, []
        for ci in cis:
            ws.append(wide[:, lo : lo + ci])
            lo += ci
        params = [wide]
    else:
        ws = [(torch.randn(Co, ci, device=DEV, generator=g) * 0.2).requires_grad_()
              for ci in cis]
        params = ws
    xs = [torch.randn(B, ci, S, device=DEV, generator=g).bfloat16().float().requires_grad_()
          for ci in cis]
    bias = torch.randn(Co, device=DEV, generator=g).requires_grad_()
    addend = torch.randn(B, Co, S, device=DEV, generator=g).bfloat16().requires_grad_()
    return ws, params, xs, bias, addend


def _run_stack(monkeypatch, mode, cis, Co, B, S, act, pm, sliced, seed):
    from pvraft_amd.model import pointwise

    pointwise.clear_step_cache()
    if mode == "classic":
        monkeypatch.setenv("PVRAFT_PW_BWD", "classic")
    else:
        monkeypatch.delenv("PVRAFT_PW_BWD", raising=False)
    ws, params, xs, bias, addend = _stack(cis, Co, B, S, seed, sliced)
    # the last part's input needs no gradient (the detached-coords case)
    xs[-1] = xs[-1].detach()
    g = torch.Generator(device=DEV).manual_seed(seed + 1)
    shape = (B, S, Co) if pm else (B, Co, S)
    G = torch.randn(shape, device=DEV, generator=g).bfloat16()
    with torch.autocast("cuda", dtype=torch.bfloat16):
        y = pointwise.pw_fused(
            [(w, x, w) for w, x in zip(ws, xs)], bias=bias, bias_target=bias,
            addend=addend, act=act, out_point_major=pm)
    (y.float() * G.float()).sum().backward()
    return dict(y=y.detach(), G=G, ws=[w.detach() for w in ws],
                xs=xs, dxs=[x.grad for x in xs], dparams=[p.grad for p in params],
                dbias=bias.grad, daddend=addend.grad)


@pytest.mark.parametrize("sliced", [False, True], ids=["own", "slices"])
@pytest.mark.parametrize("act,pm", [("relu", False), ("none", False), ("none", True),
                                    ("relu", True)])
@pytest.mark.parametrize("cis,Co,B,S", [([64], 64, 2, 200), ([64, 61, 3], 61, 1, 555),
                                        ([81, 16], 128, 2, 1000)])
def test_pw_fused_backward_against_classic(monkeypatch, cis, Co, B, S, act, pm, sliced):
    new = _run_stack(monkeypatch, "new", cis, Co, B, S, act, pm, sliced, 3)
    old = _run_stack(monkeypatch, "classic", cis, Co, B, S, act, pm, sliced, 3)
    assert torch.equal(new["y"], old["y"])
    y = new["y"]
    dpre = new["G"] * (y > 0) if act == "relu" else new["G"]
    if pm:
        dpre = dpre.transpose(1, 2)
    assert new["dxs"][-1] is None and old["dxs"][-1] is None
    for i, w in enumerate(new["ws"][:-1]):
        _bound_ok(new["dxs"][i], w.bfloat16(), dpre, f"new dx{i}")
        _bound_ok(old["dxs"][i], w.bfloat16(), dpre, f"classic dx{i}")
    # dpre is bit-equal, so everything computed from it alone is too
    assert torch.equal(new["daddend"], old["daddend"])
    assert torch.equal(new["daddend"], dpre.to(torch.bfloat16))
    # weight / bias gradients: pw_wgrad on bit-equal dpre, equal up to the
    # order of its own fp32 atomics
    lo = 0
    for i, x in enumerate(new["xs"]):  # one pw_wgrad call per part
        ci = x.shape[1]
        if sliced:
            a, b = (d["dparams"][0][:, lo : lo + ci] for d in (new, old))
        else:
            a, b = new["dparams"][i], old["dparams"][i]
        _wgrad_close(a, b, dpre, x.detach(), f"dW{i}")
        lo += ci
    # the bias sum rides part 0's call
    x0 = new["xs"][0]
    _wgrad_close(new["dbias"].view(-1, 1), old["dbias"].view(-1, 1), dpre,
                 torch.ones_like(x0[:, :1]), "dbias", bias=True, ci=x0.shape[1])


@pytest.mark.parametrize("Ci,Co,S", [(64, 64, 200), (37, 3, 65), (224, 256, 1000)])
def test_pwconv1d_backward_against_classic(monkeypatch, Ci, Co, S):
    from pvraft_amd.model import pointwise

    res = {}
    for mode in ("new", "classic"):
        pointwise.clear_step_cache()
        if mode == "classic":
            monkeypatch.setenv("PVRAFT_PW_BWD", "classic")
        else:
            monkeypatch.delenv("PVRAFT_PW_BWD", raising=False)
        torch.manual_seed(0)
        conv = pointwise.PwConv1d(Ci, Co, 1).to(DEV)
        g = torch.Generator(device=DEV).manual_seed(1)
        x = torch.randn(2, Ci, S, device=DEV, generator=g).bfloat16().float().requires_grad_()
        G = torch.randn(2, Co, S, device=DEV, generator=g).bfloat16()
        with torch.autocast("cuda", dtype=torch.bfloat16):
            y = conv(x)
        (y.float() * G.float()).sum().backward()
        res[mode] = (y.detach(), x.grad, conv.weight.grad, conv.bias.grad,
                     conv.weight.detach().squeeze(-1).bfloat16(), G, x.detach())
    n, o = res["new"], res["classic"]
    assert torch.equal(n[0], o[0])
    _bound_ok(n[1], n[4], n[5], "new dx")
    _bound_ok(o[1], o[4], o[5], "classic dx")
    xb = res["new"][6]
    _wgrad_close(n[2].squeeze(-1), o[2].squeeze(-1), n[5], xb, "dW")
    _wgrad_close(n[3].view(-1, 1), o[3].view(-1, 1), n[5], torch.ones_like(xb[:, :1]),
                 "dbias", bias=True, ci=xb.shape[1])


def test_pw_matmul_backward_against_classic(monkeypatch):
    from pvraft_amd.model import pointwise

    res = {}
    for mode in ("new", "classic"):
        pointwise.clear_step_cache()
        if mode == "classic":
            monkeypatch.setenv("PVRAFT_PW_BWD", "classic")
        else:
            monkeypatch.delenv("PVRAFT_PW_BWD", raising=False)
        g = torch.Generator(device=DEV).manual_seed(2)
        w = (torch.randn(61, 37, device=DEV, generator=g) * 0.2).requires_grad_()
        x = torch.randn(2, 37, 555, device=DEV, generator=g).bfloat16().float().requires_grad_()
        G = torch.randn(2, 61, 555, device=DEV, generator=g).bfloat16()
        with torch.autocast("cuda", dtype=torch.bfloat16):
            y = pointwise.pw_matmul(w, x)
        (y.float() * G.float()).sum().backward()
        res[mode] = (y.detach(), x.grad, w.grad, w.detach().bfloat16(), G, x.detach())
    n, o = res["new"], res["classic"]
    assert torch.equal(n[0], o[0])
    _bound_ok(n[1], n[3], n[4], "new dx")
    _bound_ok(o[1], o[3], o[4], "classic dx")
    _wgrad_close(n[2], o[2], n[4], n[5], "dW")


@pytest.mark.parametrize("deferred", [False, True], ids=["eager-wgrad", "deferred"])
def test_gru_cell_row_split_fast_path_equals_fallback(monkeypatch, deferred):
    """H=16, N=200: the gradient of m assembled in place (both pw_bwd calls
    write their row block of one buffer) is bit-equal to the concatenated
    one, and so is every gradient downstream of it."""
    from pvraft_amd.model import pointwise, update

    H, N, B = 16, 200, 2
    res = {}
    for mode in ("fast", "classic"):
        pointwise.clear_step_cache()
        if mode == "classic":
            monkeypatch.setenv("PVRAFT_PW_ROWSPLIT", "classic")
        else:
            monkeypatch.delenv("PVRAFT_PW_ROWSPLIT", raising=False)
        torch.manual_seed(0)
        gru = update.ConvGRU(input_dim=24 + 3, hidden_dim=H).to(DEV)
        g = torch.Generator(device=DEV).manual_seed(1)
        h = torch.randn(B, H, N, device=DEV, generator=g).requires_grad_()
        xs = [torch.randn(B, 24, N, device=DEV, generator=g).requires_grad_(),
              torch.randn(B, 3, N, device=DEV, generator=g)]
        m_grads = []
        orig = pointwise.row_split

        def spy(m, a):
            m.register_hook(lambda gr: m_grads.append(gr.clone()))
            return orig(m, a)

        monkeypatch.setattr(pointwise, "row_split", spy)
        before = dict(pointwise.ROWSPLIT_STATS)
        if deferred:
            for p in gru.parameters():
                p.grad = torch.zeros_like(p)
            pointwise.wgrad_defer_begin()
        try:
            with torch.autocast("cuda", dtype=torch.bfloat16):
                out = gru.forward_parts(h, xs)
            out.float().square().sum().backward()
            if deferred:
                pointwise.wgrad_flush()
        finally:
            pointwise.wgrad_defer_end()
            monkeypatch.setattr(pointwise, "row_split", orig)
        torch.cuda.synchronize()
        took = {k: pointwise.ROWSPLIT_STATS[k] - before[k] for k in before}
        assert took == ({"fast": 1, "cat": 0} if mode == "fast" else {"fast": 0, "cat": 1})
        res[mode] = (out.detach(), m_grads[0], h.grad, xs[0].grad,
                     [p.grad.clone() for p in gru.parameters()])
    f, c = res["fast"], res["classic"]
    assert torch.equal(f[0], c[0])
    assert f[1].shape == (B, 3 * H, N)
    assert torch.equal(f[1].view(torch.int16), c[1].view(torch.int16))
    assert torch.equal(f[2], c[2]) and torch.equal(f[3], c[3])
    for a, b in zip(f[4], c[4]):
        assert torch.equal(a, b)
