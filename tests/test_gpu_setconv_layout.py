"""GPU tests of SetConv stage 1 without layout round-trips: the point-major
store of csrc/pw_fwd.hip, the channel-major output mode of the pick kernel
(csrc/edge_gnmp.hip, shared with csrc/knn_gnmp.hip), and the SetConv /
FlowHead composition built on them, each against the classic composition
(PVRAFT_SETCONV_LAYOUT=classic).  Run with -m gpu."""

import copy

import pytest
import torch

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", autouse=True)
def _require_gpu_and_ext():
    if not torch.cuda.is_available():
        pytest.skip("needs GPU")
    import pvraft_amd.ops as ops

    assert ops.hip_available(), "HIP extension must be built on the GPU box"


def dev():
    return torch.device("cuda:0")


# ------------------------------------------------------- pw_fwd point-major


@pytest.mark.parametrize(
    "cis,Co,B,S,bias_relu",
    [
        ([64, 3], 48, 2, 1000, False),
        ([64, 3], 64, 2, 8192, False),  # the 32-column tile
        ([3, 3], 16, 2, 257, False),
        ([64, 3], 96, 2, 16384, True),
        ([61], 61, 1, 555, False),  # Co % 4 != 0: per-element stores
    ],
)
def test_pw_fwd_point_major_store_is_the_transpose(cis, Co, B, S, bias_relu):
    from pvraft_amd import _C

    g = torch.Generator().manual_seed(11)
    ws = [torch.randn(Co, ci, generator=g).to(dev(), torch.bfloat16) for ci in cis]
    xs = [torch.randn(B, ci, S, generator=g).to(dev(), torch.bfloat16) for ci in cis]
    bias = torch.randn(Co, generator=g).to(dev()) if bias_relu else None
    act = 1 if bias_relu else 0
    y = _C.pw_fwd(ws, xs, bias, None, act)
    y_pm = _C.pw_fwd(ws, xs, bias, None, act, True)
    assert y.shape == (B, Co, S) and y_pm.shape == (B, S, Co)
    assert y_pm.is_contiguous()
    assert torch.equal(y_pm, y.transpose(1, 2))


def test_pw_fwd_takes_column_slices_of_a_wider_weight():
    from pvraft_amd import _C

    g = torch.Generator().manual_seed(12)
    Co, C, B, S = 48, 64, 2, 300
    w = torch.randn(Co, C + 3, generator=g).to(dev(), torch.bfloat16)
    f = torch.randn(B, C, S, generator=g).to(dev(), torch.bfloat16)
    x = torch.randn(B, 3, S, generator=g).to(dev(), torch.bfloat16)
    sliced = _C.pw_fwd([w[:, :C], w[:, C:]], [f, x], None, None, 0)
    copied = _C.pw_fwd([w[:, :C].contiguous(), w[:, C:].contiguous()], [f, x], None, None, 0)
    assert torch.equal(sliced, copied)


def test_batched_wgrad_accumulates_into_a_column_block():
    from pvraft_amd import _C

    g = torch.Generator().manual_seed(13)
    Co, C, B, S = 48, 64, 2, 777
    dy = torch.randn(B, Co, S, generator=g).to(dev(), torch.bfloat16)
    f = torch.randn(B, C, S, generator=g).to(dev(), torch.bfloat16)
    x = torch.randn(B, 3, S, generator=g).to(dev(), torch.bfloat16)
    empty = torch.empty(0)
    full = torch.zeros(Co, C + 3, device=dev())
    keep = _C.pw_wgrad_batched([dy, dy], [f, x], [full[:, :C], full[:, C:]], [empty, empty])
    want_f = torch.zeros(Co * C, device=dev())
    want_x = torch.zeros(Co * 3, device=dev())
    keep2 = _C.pw_wgrad_batched([dy, dy], [f, x], [want_f, want_x], [empty, empty])
    torch.cuda.synchronize()
    del keep, keep2
    # fp32 atomics: the two runs may sum the split-K partials in another order
    ref = torch.cat([want_f.view(Co, C), want_x.view(Co, 3)], dim=1)
    assert torch.allclose(full, ref, rtol=1e-4, atol=1e-3 * ref.abs().max().item())


# ------------------------------------------------------ channel-major pick


@pytest.mark.parametrize("M", [16, 48, 96])
def test_edge_gnmp_channel_major_output_is_the_transpose(M):
    import pvraft_amd.ops as ops
    from pvraft_amd import _C
    from pvraft_amd.model.graph import Graph

    B, N, K, G = 2, 500, 16, 8
    g = torch.Generator().manual_seed(20 + M)
    wg0 = torch.randn(B, N, M, generator=g).to(dev(), torch.bfloat16)
    graph = Graph.build(torch.randn(B, N, 3, generator=g).to(dev()), K)
    w = (torch.rand(M, generator=g) + 0.5).to(dev())
    b = (torch.randn(M, generator=g) * 0.1).to(dev())
    w[::3] *= -1  # negative gammas pick the lower extreme

    pm = _C.edge_gnmp_fwd(wg0, graph.idx32, G, w, b, 1e-5, 1, 0.1, None)
    cm = _C.edge_gnmp_fwd(wg0, graph.idx32, G, w, b, 1e-5, 1, 0.1, None, True)
    assert cm[0].shape == (B, M, N) and cm[0].is_contiguous()
    assert torch.equal(cm[0], pm[0].transpose(1, 2))
    assert torch.equal(cm[1], pm[1])  # am
    assert torch.equal(cm[2], pm[2])  # vsel

    dy = torch.randn(B, N, M, generator=g).to(dev(), torch.bfloat16)
    grads = []
    for channel_major in (False, True):
        wg = wg0.clone().requires_grad_(True)
        y = ops.edge_gnmp(wg, graph.idx32, graph.csr(), G, w, b, 1e-5, act="lrelu",
                          slope=0.1, channel_major_out=channel_major)
        y.backward(dy.transpose(1, 2).contiguous() if channel_major else dy)
        grads.append(wg.grad)
    assert torch.equal(grads[0], grads[1])


@pytest.mark.parametrize("C", [16, 48, 96])
def test_knn_gnmp_channel_major_output_is_the_transpose(C):
    import pvraft_amd.ops as ops

    B, N, K = 2, 500, 16
    G = 4 if C == 16 else 8  # the kernel needs C / G >= 4
    g = torch.Generator().manual_seed(40 + C)
    raw0 = torch.randn(B, 4, K, N, generator=g).to(dev())
    w = (torch.randn(C, 4, 1, 1, generator=g) * 0.2).to(dev())
    cb = (torch.randn(C, generator=g) * 0.1).to(dev())
    ga = (torch.rand(C, generator=g) + 0.5).to(dev())
    be = (torch.randn(C, generator=g) * 0.1).to(dev())
    sl = torch.tensor([0.25], device=dev())
    dy = torch.randn(B, C, N, generator=g).to(dev(), torch.bfloat16)
    outs, grads = [], []
    for channel_major in (False, True):
        raw = raw0.clone().requires_grad_(True)
        with torch.autocast("cuda", dtype=torch.bfloat16):
            y = ops.knn_gnmp(raw, w, cb, G, ga, be, 1e-5, sl,
                             channel_major_out=channel_major)
        assert y.shape == (B, C, N)
        y.backward(dy)
        outs.append(y.detach())
        grads.append(raw.grad)
    assert outs[1].is_contiguous()
    assert torch.equal(outs[0], outs[1])
    assert torch.equal(grads[0], grads[1])


# ------------------------------------------------------------ SetConv module


def _setconv_run(sc, feats0, graph, cot, monkeypatch, mode):
    """One forward + backward of ``sc``; mode in {'new', 'classic', 'ref'}.
    Returns (out, dfeats, {name: grad}) as fp32 clones."""
    from pvraft_amd.model import pointwise

    monkeypatch.delenv("PVRAFT_SETCONV_LAYOUT", raising=False)
    monkeypatch.delenv("PVRAFT_REF_OPS", raising=False)
    if mode == "classic":
        monkeypatch.setenv("PVRAFT_SETCONV_LAYOUT", "classic")
    if mode == "ref":
        monkeypatch.setenv("PVRAFT_REF_OPS", "1")
    pointwise.clear_step_cache()
    sc.zero_grad(set_to_none=True)
    feats = feats0.clone().requires_grad_(True)
    with torch.autocast("cuda", dtype=torch.bfloat16, enabled=mode != "ref"):
        out = sc(feats, graph)
    out.float().backward(cot)
    grads = {n: p.grad.float().clone() for n, p in sc.named_parameters()}
    return out.detach().float().clone(), feats.grad.float().clone(), grads


@pytest.mark.parametrize("cin,cout", [(64, 64), (3, 32)])
def test_setconv_new_layout_is_as_close_to_fp32_as_the_classic_one(cin, cout, monkeypatch):
    """Both paths against the fp32 PVRAFT_REF_OPS composition; the new one may
    be at most 2x as far off as the classic one (they differ only in the
    accumulation order of the fc1 GEMM).  Measured on one MI355X, max |err|
    / max |ref|, new == classic to the digits shown in every row:
    SetConv(64, 64) out 8.80e-3, dfeats 2.06e-1, fc1.weight 1.04e-1,
    fc2.weight 1.30e-1, fc3.weight 8.64e-2, gn weights/biases 2.6e-3..1.2e-1;
    SetConv(3, 32) out 8.15e-3, dfeats 2.39e-1, fc1.weight 1.16e-1,
    fc2.weight 1.04e-1, fc3.weight 9.02e-2, gn 7.0e-3..9.1e-2.  (The large
    gradient figures are max-pool argmax flips of bf16 against fp32.)"""
    from pvraft_amd.model.graph import Graph
    from pvraft_amd.model.setconv import SetConv

    B, N, k = 2, 700, 16
    g = torch.Generator().manual_seed(60 + cin)
    sc = SetConv(cin, cout).to(dev())
    feats0 = torch.randn(B, N, cin, generator=g).to(dev())
    graph = Graph.build(torch.randn(B, N, 3, generator=g).to(dev()), k)
    cot = torch.randn(B, N, cout, generator=g).to(dev())

    ref = _setconv_run(sc, feats0, graph, cot, monkeypatch, "ref")
    new = _setconv_run(sc, feats0, graph, cot, monkeypatch, "new")
    classic = _setconv_run(sc, feats0, graph, cot, monkeypatch, "classic")

    def flat(run):
        out, dfeats, grads = run
        return {"out": out, "dfeats": dfeats, **grads}

    ref, new, classic = flat(ref), flat(new), flat(classic)
    rows = []
    for name, r in ref.items():
        scale = r.abs().max().item()
        e_new = (new[name] - r).abs().max().item() / scale
        e_cls = (classic[name] - r).abs().max().item() / scale
        rows.append((name, e_new, e_cls))
        print(f"SetConv({cin},{cout}) {name}: new {e_new:.3e} classic {e_cls:.3e}")
    for name, e_new, e_cls in rows:
        assert e_new <= 2.0 * e_cls, (name, e_new, e_cls)


def test_model_runs_eagerly_under_both_layouts(monkeypatch):
    from pvraft_amd.data import synthetic_batch
    from pvraft_amd.model import PVRaft, pointwise
    from pvraft_amd.utils import sequence_loss

    model = PVRaft(truncate_k=64).to(dev())
    batch = synthetic_batch(1, 512, device=dev())
    got = {}
    for mode in ("classic", "new"):
        if mode == "classic":
            monkeypatch.setenv("PVRAFT_SETCONV_LAYOUT", "classic")
        else:
            monkeypatch.delenv("PVRAFT_SETCONV_LAYOUT", raising=False)
        pointwise.clear_step_cache()
        m = copy.deepcopy(model)
        with torch.autocast("cuda", dtype=torch.bfloat16):
            flows = m(batch["sequence"], num_iters=2)
            loss = sequence_loss(flows, batch, gamma=0.8)
        loss.backward()
        assert torch.isfinite(loss), mode
        got[mode] = {n for n, p in m.named_parameters() if p.grad is not None}
        assert all(
            torch.isfinite(p.grad).all() for p in m.parameters() if p.grad is not None
        ), mode
    assert got["classic"] <= got["new"], sorted(got["classic"] - got["new"])
