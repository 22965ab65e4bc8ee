"""WaveMult without a GPU: the numpy restatement (tests/wavemult_ref.py) and the integer helpers of the Python mirror reproduce
every literal of the reference (tests/golden/wavemult_kats.json: test/wavemult.jl and the jldoctests of src/mod/wavemult/*.jl),
every `@test_throws AssertionError` of test/wavemult.jl raises AssertionError before anything reaches the library, and the closed
form of the stretch that the fill kernel uses equals stretchmatrix."""
import json
import os
import sys
import warnings

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import wavemult_ref as ref  # noqa: E402

from waveletsext_jl_amd import WT, wavelet  # noqa: E402

HAAR = wavelet(WT.haar).qmf                                  # Wavelets.jl's tabulated value (sqrt(2) / 2), not 1 / sqrt(2)


@pytest.fixture(scope="module")
def kats():
    with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "wavemult_kats.json")) as f:
        return json.load(f)


def _r4(a):
    return np.round(np.asarray(a, dtype=np.float64), 4)


def _eq4(a, lit):
    return np.abs(_r4(a) - np.asarray(lit, dtype=np.float64)).max() < 1e-9


# ---- integer helpers: restatement and Python mirror ------------------------------------------------------------------------------
def test_dyadlength(wx, kats):
    for n, J in kats["dyadlength"]["equal"]:
        with warnings.catch_warnings():
            warnings.simplefilter("error")
            assert wx.dyadlength(n) == wx.dyadlength(np.zeros(n)) == ref.dyadlength(n) == J
    for n, J in kats["dyadlength"]["warns"]:
        for fn in (wx.dyadlength, ref.dyadlength):
            with pytest.warns(UserWarning, match=kats["dyadlength"]["warning"].replace("^", r"\^")):
                assert fn(n) == J


def test_stretchmatrix_literal_and_assertions(wx, kats):
    k = kats["stretchmatrix"]
    for fn in (wx.stretchmatrix, ref.stretchmatrix):
        ie, je = fn(k["i"], k["j"], k["n"], k["L"])
        assert ie.tolist() == k["ie"] and je.tolist() == k["je"]
        for L in k["throws_L"]:
            with pytest.raises(AssertionError):
                fn(k["i"], k["j"], k["n"], L)


def test_ndyad_literal_and_assertions(wx, kats):
    for L, Lmax, g, lo, hi in kats["ndyad"]["values"]:
        r = wx.ndyad(L, Lmax, g)
        assert (r[0], r[-1], len(r)) == (lo, hi, hi - lo + 1)
        assert ref.ndyad(L, Lmax, g) == (lo, hi)
    for L, Lmax, g in kats["ndyad"]["throws"]:
        for fn in (wx.ndyad, ref.ndyad):
            with pytest.raises(AssertionError):
                fn(L, Lmax, g)


@pytest.mark.parametrize("n", [4, 8, 16, 32, 64, 128, 256])
def test_closed_form_of_the_stretch(wx, n):
    """every entry of a full n x n matrix lands where the closed form says, in the closed form's order (rows ascending inside a
    column), for every L"""
    jj, ii = np.meshgrid(np.arange(1, n + 1), np.arange(1, n + 1))
    ii, jj = ii.T.ravel(), jj.T.ravel()                                    # column by column, like findall
    for L in range(1, ref.maxtransformlevels(n) + 1):
        ie, je = ref.stretchmatrix(ii, jj, n, L)
        ie2, je2 = wx.stretchmatrix(ii, jj, n, L)
        assert np.array_equal(ie, ie2) and np.array_equal(je, je2)
        assert len(set(zip(ie.tolist(), je.tolist()))) == n * n               # no two entries collide
        src = {}                                                             # (ie, je) -> (i, j)
        for a, b, c, d in zip(ie.tolist(), je.tolist(), ii.tolist(), jj.tolist()):
            src[(a, b)] = (c, d)
        total = 0
        for c, (j, r0, r1, shift) in enumerate(ref.stretch_closed_form(n, L), start=1):
            col = sorted(a for (a, b) in src if b == c) if n <= 32 else None
            rows = list(range(r0, r1 + 1)) if j else []
            if col is not None:
                assert col == [r + shift for r in rows], (n, L, c)
            for r in rows:
                assert src[(r + shift, c)] == (r, j), (n, L, c, r)
            total += len(rows)
        assert total == n * n


# ---- the eight functions, restated -----------------------------------------------------------------------------------------------
def test_ns_dwt_literals(oracle, kats):
    k = kats["ns"]
    x = np.array(k["x"])
    assert _eq4(ref.ns_dwt(oracle, x, HAAR), k["ns_dwt_4"])
    assert _eq4(ref.ns_idwt(oracle, np.array(k["ns_dwt_4"], dtype=np.float64), HAAR), k["ns_idwt_of_rounded_4"])
    for L in k["throws_L"]:
        with pytest.raises(AssertionError):
            ref.ns_dwt(oracle, x, HAAR, L)
        with pytest.raises(AssertionError):
            ref.ns_idwt(oracle, np.array(k["ns_dwt_4"], dtype=np.float64), HAAR, L)


def test_ns_doctest_16_digits(oracle, kats):
    k = kats["ns_doctest"]
    nxw = ref.ns_dwt(oracle, np.array(k["x"]), HAAR)
    lit = np.array(k["nxw"])
    assert np.all(np.abs(nxw - lit)[2:] <= np.spacing(np.abs(lit))[2:])    # 1 ulp
    # the docstring prints 0.0 at position 1 although transforms.jl:68 copies s_L there, as test/wavemult.jl:28-30 has it
    assert nxw[0] == nxw[2] and nxw[1] == 0.0 and lit[0] == 0.0
    xh = ref.ns_idwt(oracle, lit, HAAR)
    lit = np.array(k["xhat"])
    assert np.all(np.abs(xh - lit) <= np.spacing(np.abs(lit)))
    assert not np.allclose(xh, k["x"])                                       # "Unlike standard dwt, x != x̂"


def test_sft_literals(oracle, kats):
    k = kats["sft"]
    x = np.array(k["x"])
    assert _eq4(ref.sft(oracle, x, HAAR), k["sft_4"])
    assert _eq4(ref.isft(oracle, np.array(k["sft_4"], dtype=np.float64), HAAR), k["x"])
    for L in k["throws_L"]:
        with pytest.raises(AssertionError):
            ref.sft(oracle, x, HAAR, L)
        with pytest.raises(AssertionError):
            ref.isft(oracle, x, HAAR, L)


def test_sparse_form_literals(oracle, kats):
    k = kats["sparse"]
    x = np.array(k["x"])
    for fn, key in ((ref.mat2sparseform_nonstd, "nonstd_4"), (ref.mat2sparseform_std, "std_4")):
        S = fn(oracle, x, HAAR)
        lit = np.array(k[key], dtype=np.float64)
        A = ref.todense(S)
        assert _eq4(A, lit)
        assert np.array_equal(A != 0, lit != 0)                              # pattern: exact zeros are never stored
        assert np.all(S[3] != 0) and S[1][-1] - 1 == S[2].size == np.count_nonzero(lit)
        with pytest.raises(AssertionError):
            fn(oracle, np.zeros(k["throws_shape"]), HAAR)


def test_product_literals(oracle, kats):
    k = kats["product"]
    M, x = ref.calderon(k["n"]), np.array(k["x"])
    assert _eq4(ref.nonstd_wavemult(oracle, M, x, HAAR), k["y_4"])
    assert _eq4(ref.std_wavemult(oracle, M, x, HAAR), k["y_4"])
    # the docstrings' claim for unseeded inputs: the dense-M form is the two-step form, bit for bit
    L = 2
    assert np.array_equal(ref.std_wavemult(oracle, ref.mat2sparseform_std(oracle, M, HAAR, L), x, HAAR, L),
                          ref.std_wavemult(oracle, M, x, HAAR, L))
    assert len(kats["wavemult_doctest_outputs"]["std"]) == len(kats["wavemult_doctest_outputs"]["nonstd"]) == 4


def test_both_forms_are_the_operator_at_eps_zero(oracle):
    """with eps = 0 nothing is dropped: both products equal M x up to rounding, for a filter that wraps (db4 at n = 8)"""
    rng = np.random.default_rng(5)
    db4 = wavelet(WT.db4).qmf
    for n, q in ((8, db4), (16, HAAR), (32, db4)):
        M = np.asfortranarray(rng.standard_normal((n, n)))
        x = rng.standard_normal(n)
        for L in (1, ref.maxtransformlevels(n)):
            for fn in (ref.std_wavemult, ref.nonstd_wavemult):
                y = fn(oracle, M, x, q, L, 0.0)
                assert np.abs(y - M @ x).max() <= 1e-12 * np.abs(M @ x).max() * n, (n, L, fn.__name__)


# ---- every @test_throws of test/wavemult.jl on the Python mirror: AssertionError before anything reaches the library -------------------
def test_mirror_assertions_need_no_device(wx, kats):
    wt = wx.wavelet(wx.WT.haar)
    x, y = np.array(kats["ns"]["x"]), np.array(kats["ns"]["ns_dwt_4"], dtype=np.float64)
    for L in kats["ns"]["throws_L"]:
        with pytest.raises(AssertionError):
            wx.ns_dwt(x, wt, L)
        with pytest.raises(AssertionError):
            wx.ns_idwt(y, wt, L)
    M = np.array(kats["sft"]["x"])
    for L in kats["sft"]["throws_L"]:
        with pytest.raises(AssertionError):
            wx.sft(M, wt, L)
        with pytest.raises(AssertionError):
            wx.isft(M, wt, L)
    bad = np.zeros(kats["sparse"]["throws_shape"])
    with pytest.raises(AssertionError):
        wx.mat2sparseform_nonstd(bad, wt)
    with pytest.raises(AssertionError):
        wx.mat2sparseform_std(bad, wt)
    with pytest.raises(AssertionError):
        wx.ns_dwt(np.zeros(12), wt)                                           # ispow2(n), transforms.jl:58


def test_sparse_matrix_class(wx):
    A = np.array([[1.0, 0, 2], [0, 0, 3], [4, 0, 0]])
    S = wx.SparseMatrixCSC.fromdense(A)
    assert (S.m, S.n, S.nnz) == (3, 3, 4)
    assert S.colptr.tolist() == [1, 3, 3, 5] and S.rowval.tolist() == [1, 3, 1, 2] and S.nzval.tolist() == [1.0, 4.0, 2.0, 3.0]
    assert S.colptr.dtype == S.rowval.dtype == np.int64
    assert np.array_equal(S.todense(), A)
