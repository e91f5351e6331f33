"""pw_fwd with the pw_stage.h operand staging (rows as stored + transposed
LDS read) is bit-equal to PVRAFT_PW_STAGE=classic (transpose with 2-byte LDS
stores on the way in): both feed every MFMA the same 32 products of the
same k block."""

import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = "cuda"


def _both(monkeypatch, ws, xs, bias, addend, act, pm):
    from pvraft_amd import _C

    monkeypatch.delenv("PVRAFT_PW_STAGE", raising=False)
    y_new = _C.pw_fwd(ws, xs, bias, addend, act, pm)
    monkeypatch.setenv("PVRAFT_PW_STAGE", "classic")
    y_old = _C.pw_fwd(ws, xs, bias, addend, act, pm)
    monkeypatch.delenv("PVRAFT_PW_STAGE", raising=False)
    torch.cuda.synchronize()
    assert y_new.shape == y_old.shape
    assert torch.equal(y_new.view(torch.int16), y_old.view(torch.int16)), (
        (y_new.float() - y_old.float()).abs().max().item())
    return y_new


def _case(monkeypatch, cis, Co, B, S, act, with_bias, with_addend, pm, slices=False):
    torch.manual_seed(7)
    if slices:
        wide = torch.randn(Co, sum(cis) + 3, device=DEV, dtype=torch.bfloat16)
        lo, ws = 0, []
        for ci in cis:
            ws.append(wide[:, lo : lo + ci])
            lo += ci
    else:
        ws = [torch.randn(Co, ci, device=DEV, dtype=torch.bfloat16) for ci in cis]
    xs = [torch.randn(B, ci, S, device=DEV, dtype=torch.bfloat16) for ci in cis]
    bias = torch.randn(Co, device=DEV) if with_bias else None
    add_full = torch.randn(B, Co + 32, S, device=DEV, dtype=torch.bfloat16)
    addend = add_full[:, 16 : 16 + Co] if with_addend else None
    y = _both(monkeypatch, ws, xs, bias, addend, act, pm)
    # and it is the right answer (the staging is not just equal, but
    # equally wrong, if both were broken the same way): float64 composition
    ref = sum(torch.bmm(w.double().unsqueeze(0).expand(B, -1, -1), x.double())
              for w, x in zip(ws, xs))
    if bias is not None:
        ref = ref + bias.view(1, -1, 1)
    if addend is not None:
        ref = ref + addend.double()
    if act == 1:
        ref = torch.relu(ref)
    if pm:
        ref = ref.transpose(1, 2)
    # one bf16 rounding (2^-8 relative) of an fp32 sum of <= 224*3 terms
    mag = sum(torch.bmm(w.double().abs().unsqueeze(0).expand(B, -1, -1), x.double().abs())
              for w, x in zip(ws, xs))
    if bias is not None:
        mag = mag + bias.abs().view(1, -1, 1)
    if addend is not None:
        mag = mag + addend.double().abs()
    if pm:
        mag = mag.transpose(1, 2)
    bound = 2.0 ** -7 * ref.abs() + 2.0 ** -15 * mag + 1e-30
    assert ((y.double() - ref).abs() <= bound).all()


@pytest.mark.parametrize("pm", [False, True], ids=["cm", "pm"])
@pytest.mark.parametrize("slices", [False, True], ids=["own", "slices"])
@pytest.mark.parametrize("parts,Co,S,act,with_bias,with_addend", [
    (1, 64, 2048, 0, True, False),
    (2, 61, 1000, 1, True, False),
    (3, 192, 4096, 0, False, True),
    (1, 128, 555, 1, False, False),
])
def test_new_staging_bit_equal_to_classic(monkeypatch, parts, Co, S, act,
                                          with_bias, with_addend, slices, pm):
    _case(monkeypatch, [64, 61, 37][:parts], Co, 2, S, act, with_bias,
          with_addend, pm, slices)


@pytest.mark.parametrize("pm", [False, True], ids=["cm", "pm"])
@pytest.mark.parametrize("S", [1, 15, 65, 555])
@pytest.mark.parametrize("ci", [3, 37, 61, 224])
def test_ragged_columns_and_channel_counts(monkeypatch, ci, S, pm):
    _case(monkeypatch, [ci, 64], 64, 2, S, 1, True, True, pm)
    _case(monkeypatch, [ci], 256, 1, S, 0, False, False, pm, slices=True)


@pytest.mark.parametrize("S", [8192, 16384])  # TC=32 / TC=64 policies
@pytest.mark.parametrize("Co", [64, 160, 192])  # 160: 10 row fragments
def test_flagship_tiles(monkeypatch, Co, S):
    _case(monkeypatch, [64, 61, 3], Co, 2, S, 1, True, True, False)
