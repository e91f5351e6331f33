"""Fused data gradient of the 1x1-conv stacks (csrc/pw_bwd.hip).

    dpre = dy * (act == relu ? y > 0 : 1)        bit-equal to ATen
    dx_i = W_i^T @ dpre                          bf16 operands, fp32 sums

Oracle: float64 on the bf16-rounded inputs.  Bound per dx element (derived,
not tuned):

    |dx - ref| <= 2^-7 |ref| + 2^-16 sum_o |W[o,c]| |dpre[o,s]|

The first term is one bf16 ulp for the single rounding of the fp32 sum (its
worst case is half that); the second is K * 2^-24 with K <= 256 for an fp32
accumulation in any order.  The composed path (threshold_backward,
transpose, bmm) is held to the same bound on the same inputs, so a failure
of the bound itself shows.
"""

import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = "cuda"
CI_SETS = {
    "64": ([64], [True]),
    "64+64": ([64, 64], [True, True]),
    "61+3nw": ([61, 3], [True, False]),
    "81": ([81], [True]),
    "224+16+37+64": ([224, 16, 37, 64], [True, True, True, True]),
}


def _C():
    from pvraft_amd import _C

    return _C


def _inputs(B, S, Co, cis, pm, seed, w_offsets=None):
    g = torch.Generator(device=DEV).manual_seed(seed)
    shape = (B, S, Co) if pm else (B, Co, S)
    dy = torch.randn(shape, device=DEV, generator=g).bfloat16()
    y = torch.randn(shape, device=DEV, generator=g).relu().bfloat16()
    # exact zeros and negative zeros where the ReLU output is "off"
    flat = y.view(-1)
    flat[::7] = 0.0
    flat[3::11] = -0.0
    ws = []
    for i, ci in enumerate(cis):
        if w_offsets is None:
            ws.append((torch.randn(Co, ci, device=DEV, generator=g) * 0.2).bfloat16())
        else:
            off = w_offsets[i]
            wide = (torch.randn(Co, off + ci + 5, device=DEV, generator=g) * 0.2).bfloat16()
            ws.append(wide[:, off : off + ci])
    return dy, y, ws


def _dpre_ref(dy, y, act, pm):
    d = torch.ops.aten.threshold_backward(dy, y, 0) if act == 1 else dy
    return d.transpose(1, 2).contiguous() if pm else d


def _check_dx(dx, w, dpre, what):
    ref = torch.einsum("oc,bos->bcs", w.double(), dpre.double())
    mag = torch.einsum("oc,bos->bcs", w.double().abs(), dpre.double().abs())
    bound = 2.0 ** -7 * ref.abs() + 2.0 ** -16 * mag
    err = (dx.double() - ref).abs()
    worst = (err - bound).max().item()
    assert worst <= 0.0, f"{what}: error exceeds the bound by {worst:.3e}"


def _composed(ws, want, dpre):
    return [
        torch.bmm(w.t().unsqueeze(0).expand(dpre.shape[0], -1, -1), dpre) if k else None
        for w, k in zip(ws, want)
    ]


def _run(B, S, Co, cis, want, act, pm, seed=0, w_offsets=None):
    dy, y, ws = _inputs(B, S, Co, cis, pm, seed, w_offsets)
    outs = _C().pw_bwd(dy, y if act == 1 else None, ws, want, act, pm)
    assert len(outs) == sum(want) + 1
    dpre = outs[-1]
    dpre_ref = _dpre_ref(dy, y, act, pm)
    assert dpre.shape == (B, Co, S) and dpre.is_contiguous()
    assert torch.equal(dpre.view(torch.int16), dpre_ref.view(torch.int16))
    if act == 0 and not pm:
        assert dpre.data_ptr() == dy.data_ptr()  # nothing to write
    it = iter(outs[:-1])
    composed = _composed(ws, want, dpre_ref)
    for i, (w, k) in enumerate(zip(ws, want)):
        if not k:
            continue
        dx = next(it)
        assert dx.shape == (B, w.shape[1], S) and dx.is_contiguous()
        assert dx.dtype == torch.bfloat16
        _check_dx(dx, w, dpre_ref, f"pw_bwd part {i}")
        _check_dx(composed[i], w, dpre_ref, f"composed part {i}")
    return dy, y, ws, outs


@pytest.mark.parametrize("pm", [False, True], ids=["cm", "pm"])
@pytest.mark.parametrize("act", [0, 1])
@pytest.mark.parametrize("B", [1, 2])
@pytest.mark.parametrize("S", [1, 15, 64, 65, 555, 1000, 4104])
def test_ragged_and_tile_edge_columns(S, B, act, pm):
    _run(B, S, 64, [64], [True], act, pm, seed=S)


@pytest.mark.parametrize("pm", [False, True], ids=["cm", "pm"])
@pytest.mark.parametrize("ciset", list(CI_SETS))
@pytest.mark.parametrize("Co", [3, 61, 64, 128, 192, 256])
def test_channel_counts(Co, ciset, pm):
    cis, want = CI_SETS[ciset]
    # S=555: ragged, several tiles; S=1000 (8 | S): the aligned path with a
    # cut last tile
    for S, act in ((555, 1), (1000, 0)):
        _run(2, S, Co, cis, want, act, pm, seed=Co)


@pytest.mark.parametrize("pm", [False, True], ids=["cm", "pm"])
@pytest.mark.parametrize("S", [8192, 16384])  # TC=32 / TC=64 tile policies
@pytest.mark.parametrize(
    "Co,ciset,act", [(64, "64+64", 1), (192, "61+3nw", 0), (128, "81", 0)])
def test_flagship_tile_policies(S, Co, ciset, act, pm):
    cis, want = CI_SETS[ciset]
    _run(2, S, Co, cis, want, act, pm, seed=1)


@pytest.mark.parametrize("pm", [False, True], ids=["cm", "pm"])
@pytest.mark.parametrize("S", [64, 65, 1000])
@pytest.mark.parametrize("offs", [(0, 61), (61, 125), (125, 0)])
def test_weight_column_slices(offs, S, pm):
    # slices of a wider weight: offsets 61 and 125 leave rows off the
    # 16-byte grid (element path), 0 with an odd pitch likewise
    _run(2, S, 64, [64, 61], [True, True], 1, pm, seed=3, w_offsets=offs)
    # pitch a multiple of 8 at offset 0: the vector path on a pitched weight
    g = torch.Generator(device=DEV).manual_seed(5)
    wide = (torch.randn(64, 128, device=DEV, generator=g) * 0.2).bfloat16()
    dy, y, _ = _inputs(2, S, 64, [], pm, 4)
    ws = [wide[:, :64], wide[:, 64:]]
    outs = _C().pw_bwd(dy, y, ws, [True, True], 1, pm)
    dpre = _dpre_ref(dy, y, 1, pm)
    for dx, w in zip(outs[:-1], ws):
        _check_dx(dx, w, dpre, "pitched weight")
        same = _C().pw_bwd(dy, y, [w.contiguous()], [True], 1, pm)[0]
        assert torch.equal(dx, same)


@pytest.mark.parametrize("pm", [False, True], ids=["cm", "pm"])
@pytest.mark.parametrize("act", [0, 1])
def test_all_parts_unwanted_gives_only_dpre(act, pm):
    dy, y, ws, outs = _run(2, 555, 61, [64, 3], [False, False], act, pm)
    assert len(outs) == 1


@pytest.mark.parametrize("B", [1, 2])
@pytest.mark.parametrize("S", [15, 64, 1000, 4104])
@pytest.mark.parametrize("Co", [61, 64, 128])
def test_slab_rows(Co, S, B):
    dy, _y, ws = _inputs(B, S, Co, [64], False, 7)
    sentinel = -1.2345e5
    slab = torch.full((B, Co + 32, S), sentinel, device=DEV, dtype=torch.bfloat16)
    outs = _C().pw_bwd(dy, None, ws, [True], 0, False, slab, 16)
    assert outs[-1].data_ptr() == slab[:, 16:].data_ptr()
    assert torch.equal(outs[-1], dy) and torch.equal(slab[:, 16 : 16 + Co], dy)
    assert (slab[:, :16] == sentinel).all() and (slab[:, 16 + Co :] == sentinel).all()
    _check_dx(outs[0], ws[0], dy, "slab call")
    # a slab is refused where dpre is not dy
    with pytest.raises(RuntimeError):
        _C().pw_bwd(dy, dy, ws, [True], 1, False, slab, 16)
    with pytest.raises(RuntimeError):
        _C().pw_bwd(dy, None, ws, [True], 0, False, slab, 33)


@pytest.mark.parametrize("pm", [False, True], ids=["cm", "pm"])
def test_two_calls_are_bit_equal(pm):
    cis, want = CI_SETS["224+16+37+64"]
    dy, y, ws = _inputs(2, 4104, 192, cis, pm, 11)
    a = _C().pw_bwd(dy, y, ws, want, 1, pm)
    b = _C().pw_bwd(dy, y, ws, want, 1, pm)
    for x, z in zip(a, b):
        assert torch.equal(x.view(torch.int16), z.view(torch.int16))


def test_limits_are_errors():
    dy, y, ws = _inputs(1, 64, 64, [64], False, 0)
    with pytest.raises(RuntimeError):
        _C().pw_bwd(dy, None, ws, [True], 1, False)  # relu without y
    w_big = torch.zeros(64, 225, device=DEV, dtype=torch.bfloat16)
    with pytest.raises(RuntimeError):
        _C().pw_bwd(dy, None, [w_big], [True], 0, False)
    dy_big = torch.zeros(1, 257, 8, device=DEV, dtype=torch.bfloat16)
    with pytest.raises(RuntimeError):
        _C().pw_bwd(dy_big, None, [], [], 0, False)
