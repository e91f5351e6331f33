"""CPU checks of tests/selection_cases.py: the generators are deterministic,
the exact references agree with torch, and -- by the first-sweep witnesses --
the control cases never leave the acceptance window while every
stride-biased case does, on every side the retry code has."""

import functools

import pytest
import torch

import selection_cases as sc


@functools.lru_cache(maxsize=None)
def knn_w(name):
    xyz, k = sc.knn_case(name)
    return sc.knn_witness(xyz, k)


@functools.lru_cache(maxsize=None)
def corr_w(name):
    f1t, f2t, k = sc.corr_case(name)
    return sc.corr_witness(sc.corr_exact(f1t, f2t), k)


@functools.lru_cache(maxsize=None)
def rows_w(name):
    vals, k = sc.topk_rows_case(name)
    return sc.corr_witness(vals.double(), k)


def test_generators_deterministic_and_finite():
    for name in sc.KNN_CASES:
        if "8192" in name and name not in ("gauss_8192_far", "gauss_far_line_core_8192"):
            continue  # same code path as the smaller clouds
        a, k = sc.knn_case(name)
        b, _ = sc.knn_case(name)
        assert a.dtype == torch.float32 and a.shape[-1] == 3 and k in (16, 32)
        assert torch.equal(a, b) and torch.isfinite(a).all(), name
    for name in list(sc.TOPK_CASES) + list(sc.TIE_CASES):
        a, k = sc.topk_rows_case(name)
        b, _ = sc.topk_rows_case(name)
        assert a.dtype == torch.float32 and k <= a.shape[1]
        assert torch.equal(a, b) and torch.isfinite(a).all(), name
    for name in list(sc.TOPK_CASES) + sc.CORR_TIE_CASES:
        f1, f2, k = sc.corr_case(name)
        g1, g2, _ = sc.corr_case(name)
        assert f1.dtype == torch.bfloat16 and f1.shape[-1] in (32, 128)
        assert 64 <= f1.shape[1] <= 128 and k <= f2.shape[1]
        assert torch.equal(f1, g1) and torch.equal(f2, g2), name
        assert torch.isfinite(f1.float()).all() and torch.isfinite(f2.float()).all(), name


def test_case_table_covers_the_strides():
    assert {sc.stride_of(p[1]) for _, parts in sc.KNN_CASES.values() for p in parts} == {2, 5, 8}
    assert {k for k, _ in sc.KNN_CASES.values()} == {16, 32}
    assert {sc.stride_of(c[1], sc.CT_SAMP) for c in sc.TOPK_CASES.values()} == {1, 2, 4, 8}
    assert {c[2] for c in sc.TOPK_CASES.values()} == {64, 256, 512, 1024}


@pytest.mark.parametrize("name", sc.KNN_CONTROLS)
def test_knn_controls_stay_inside_the_window(name):
    """Over ALL queries a randn cloud is not literally retry-free: the first
    sweep overflows when fewer than kp sampled points lie among the CAP
    nearest, a Binomial(CAP, 1/st) tail.  At N=8192, k=32 that is
    Binomial(256, 1/8) < 16, mean 32 and sd 5.3, about 1e-3 per query --
    a handful of queries per cloud, against at least half for a biased one.
    Underflow (kp or more sampled points among the k nearest) is out of
    reach."""
    w = knn_w(name)
    assert w["under"] == 0 and w["over"] <= 2e-3, w


@pytest.mark.parametrize("name", sc.TOPK_CONTROLS)
def test_topk_controls_stay_inside_the_window(name):
    for w in (corr_w(name), rows_w(name)):
        assert w["over_hi"] == 0 and w["under"] == 0 and w["over_bd"] == 0, w


@pytest.mark.parametrize("name", sc.KNN_BIASED)
def test_knn_biased_cases_leave_the_window(name):
    w = knn_w(name)
    assert w["under"] + w["over"] >= 0.5, w


@pytest.mark.parametrize("name", sc.TOPK_BIASED)
def test_corr_biased_cases_leave_the_window(name):
    w = corr_w(name)
    assert w["over_hi"] + w["under"] + w["over_bd"] >= 0.5, w


def test_retry_cases_reach_every_branch():
    """If CAP, SAMP or the sample ranks are retuned the cases must be
    regenerated, not left to decay into controls."""
    knn = [knn_w(n) for n in sc.KNN_BIASED]
    assert max(w["under"] for w in knn) >= 0.1
    assert max(w["over"] for w in knn) >= 0.5
    corr = [corr_w(n) for n in sc.TOPK_BIASED]
    for side in ("over_hi", "under", "over_bd"):
        assert max(w[side] for w in corr) >= 0.5, side


def test_boundary_tie_groups_are_small():
    """No case but the explicit tie cases has more than 64 equal values at
    its selection boundary (the smallest buffer holds 128), so a wrong
    result on them is never a tie artefact."""
    assert sc.MAX_TIE_GROUP * 2 <= min(sc.KNN_CAP, sc.CT_CAP, sc.TK_CAP)
    for name in sc.KNN_CASES:
        assert knn_w(name)["max_tie"] <= sc.MAX_TIE_GROUP, name
    for name in sc.TOPK_CASES:
        assert corr_w(name)["max_tie"] <= sc.MAX_TIE_GROUP, name
        assert rows_w(name)["max_tie"] <= sc.MAX_TIE_GROUP, name
    # and the tie cases do tie: more than the fp32 kernel's buffer holds
    assert max(rows_w(n)["max_tie"] for n in sc.TIE_CASES) > sc.TK_CAP
    # and the tied shelf cuts a group that only just fits the correlation band
    assert sc.CT_CAP // 2 < corr_w("tiedshelf_8192_512")["max_tie"] <= sc.CT_CAP


def test_exact_references_match_torch():
    g = torch.Generator().manual_seed(0)
    xyz = torch.randn(2, 200, 3, generator=g)
    want = torch.cdist(xyz.double(), xyz.double(), compute_mode="donot_use_mm_for_euclid_dist") ** 2
    want = want.topk(16, dim=-1, largest=False).values
    assert torch.allclose(sc.knn_exact(xyz, 16, chunk=64), want, rtol=1e-12, atol=1e-15)

    f1 = torch.randn(1, 200, 32, generator=g).to(torch.bfloat16)
    f2 = torch.randn(1, 150, 32, generator=g).to(torch.bfloat16)
    ref = sc.corr_exact(f1, f2)
    want = torch.einsum("bnc,bmc->bnm", f1.double(), f2.double()) / 32 ** 0.5
    assert ref.dtype == torch.float64 and torch.allclose(ref, want, rtol=1e-14, atol=1e-14)
    assert (sc.corr_error_bound(f1, f2) > 0).all()

    vals = torch.randn(5, 200, generator=g)
    v, i = sc.topk_exact(vals, 17)
    assert torch.equal(v, vals.sort(dim=1, descending=True).values[:, :17])
    assert torch.equal(v, vals.gather(1, i))
