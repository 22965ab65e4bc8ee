"""WaveMult on the GPU against the numpy restatement of the reference (tests/wavemult_ref.py) and the reference's literals
(tests/golden/wavemult_kats.json): ns_dwtall / ns_idwtall, sft / isft, both sparse forms (exact pattern) and both products,
Float64 and Float32, host arrays and device tensors.

Tolerances: relerr <= TOL of tests/helpers.py (1e-10 / 1e-5).  The Float32 products take the larger of TOL and 4 x the distance
of the Float32 restatement from the Float64 restatement on the same inputs: the product sums a row in ascending column order with
fused multiply-adds, the reference adds column after column with a separate multiply and add.  Observed: profiles/wavemult.md.
"""
import ctypes
import json
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import wavemult_ref as ref  # noqa: E402
from helpers import TOL, relerr  # noqa: E402

pytestmark = pytest.mark.gpu

DTYPES = [np.float64, np.float32]
NS_LONG = 8192                       # the smallest n of the level-by-level ns_dwt / ns_idwt kernels (NS_LDS_MAX + 1 rounded to a power of two)


@pytest.fixture(scope="module")
def kats():
    with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "wavemult_kats.json")) as f:
        return json.load(f)


@pytest.fixture(scope="module")
def filt(wx):
    return {k: wx.wavelet(getattr(wx.WT, k)) for k in ("haar", "db4", "db8")}


def _levels(n):
    Lmax = ref.maxtransformlevels(n)
    return sorted({1, (Lmax + 1) // 2, Lmax})


def _both(wx, fn, *arrays):
    """fn on host arrays and on device tensors -> two host results"""
    h = fn(*[np.asfortranarray(a) for a in arrays])
    assert isinstance(h, np.ndarray)
    d = fn(*[wx.to_device(a, "cuda:0") for a in arrays])
    assert not isinstance(d, np.ndarray) and d.is_cuda
    return h, wx.to_numpy(d)


def _r4(a):
    return np.round(np.asarray(a, dtype=np.float64), 4)


# ------------------------------------------------------------------------------------------------------------------------------
# ns_dwtall / ns_idwtall
# ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("fname", ["haar", "db4", "db8"])
@pytest.mark.parametrize("n", [2, 4, 8, 64, 128, 1024, 4096, NS_LONG])
def test_ns_dwtall_and_ns_idwtall(wx, oracle, filt, n, fname, dtype):
    wt = filt[fname]
    rng = np.random.default_rng(n + len(fname))
    X = np.asfortranarray(rng.standard_normal((n, 65)).astype(dtype))
    W = np.asfortranarray(rng.standard_normal((2 * n, 65)).astype(dtype))
    for L in _levels(n):
        fwd = ref.columns(ref.ns_dwt, oracle, X, wt.qmf, L)
        inv = ref.columns(ref.ns_idwt, oracle, W, wt.qmf, L)
        m = n >> L
        for B in (1, 3, 65):
            for got in _both(wx, lambda a: wx.ns_dwtall(a, wt, L), X[:, :B]):
                assert got.shape == (2 * n, B) and got.dtype == dtype
                e = relerr(got, fwd[:, :B])
                print("ns_dwtall n=%d %s %s L=%d B=%d relerr %.2e" % (n, fname, np.dtype(dtype).name, L, B, e))
                assert e <= TOL[np.dtype(dtype)]
                assert np.all(got[m:2 * m] == 0.0) and np.all(fwd[m:2 * m] == 0.0)      # what the reference leaves at 0.0
            for got in _both(wx, lambda a: wx.ns_idwtall(a, wt, L), W[:, :B]):
                assert got.shape == (n, B) and got.dtype == dtype
                e = relerr(got, inv[:, :B])
                print("ns_idwtall n=%d %s %s L=%d B=%d relerr %.2e" % (n, fname, np.dtype(dtype).name, L, B, e))
                assert e <= TOL[np.dtype(dtype)]


def test_ns_doctest_to_one_ulp(wx, filt, kats):
    k = kats["ns_doctest"]
    wt = filt["haar"]
    for nxw in _both(wx, lambda a: wx.ns_dwt(a, wt), np.array(k["x"])):
        lit = np.array(k["nxw"])
        assert np.all(np.abs(nxw - lit)[2:] <= np.spacing(np.abs(lit))[2:]), nxw - lit
        # the docstring prints 0.0 at position 1 although transforms.jl:68 copies s_L there, as test/wavemult.jl:28-30 has it
        assert nxw[0] == nxw[2] and nxw[1] == 0.0
    for xh in _both(wx, lambda a: wx.ns_idwt(a, wt), np.array(k["nxw"])):
        lit = np.array(k["xhat"])
        assert np.all(np.abs(xh - lit) <= np.spacing(np.abs(lit))), xh - lit
    k = kats["ns"]
    assert np.array_equal(_r4(wx.ns_dwt(np.array(k["x"]), wt)), np.array(k["ns_dwt_4"]))
    assert np.array_equal(_r4(wx.ns_idwt(np.array(k["ns_dwt_4"], dtype=np.float64), wt)), np.array(k["ns_idwt_of_rounded_4"]))


# ------------------------------------------------------------------------------------------------------------------------------
# sft / isft
# ------------------------------------------------------------------------------------------------------------------------------
def test_sft_literal(wx, filt, kats):
    k = kats["sft"]
    for got in _both(wx, lambda a: wx.sft(a, filt["haar"]), np.array(k["x"])):
        assert np.abs(_r4(got) - np.array(k["sft_4"], dtype=np.float64)).max() < 1e-9
    for got in _both(wx, lambda a: wx.isft(a, filt["haar"]), np.array(k["sft_4"], dtype=np.float64)):
        assert np.abs(_r4(got) - np.array(k["x"])).max() < 1e-9


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("fname", ["haar", "db4"])
@pytest.mark.parametrize("shape", [(8, 8), (64, 64), (128, 32)])
def test_sft_isft(wx, oracle, filt, shape, fname, dtype):
    wt = filt[fname]
    rng = np.random.default_rng(shape[0] + shape[1])
    M = np.asfortranarray(rng.standard_normal(shape).astype(dtype))
    tol = TOL[np.dtype(dtype)]
    for L in sorted({1, ref.maxtransformlevels(min(shape))}):
        fwd, inv = ref.sft(oracle, M, wt.qmf, L), ref.isft(oracle, M, wt.qmf, L)
        for got in _both(wx, lambda a: wx.sft(a, wt, L), M):
            assert got.shape == shape and got.dtype == dtype
            assert relerr(got, fwd) <= tol
        for got in _both(wx, lambda a: wx.isft(a, wt, L), M):
            assert relerr(got, inv) <= tol
        back = wx.isft(wx.sft(M, wt, L), wt, L)
        assert relerr(back, M) <= tol


# ------------------------------------------------------------------------------------------------------------------------------
# sparse forms
# ------------------------------------------------------------------------------------------------------------------------------
def _same_sparse(S, R, dtype):
    """S: wx.SparseMatrixCSC, R: the restatement's tuple -- exact pattern, values within tolerance, rows ascending"""
    N, colptr, rowval, nzval = R
    assert (S.m, S.n) == (N, N)
    assert S.colptr.dtype == np.int64 and S.rowval.dtype == np.int64 and S.nzval.dtype == dtype
    assert np.array_equal(S.colptr, colptr), "colptr"
    assert np.array_equal(S.rowval, rowval), "rowval"
    for j in range(N):
        r = S.rowval[S.colptr[j] - 1:S.colptr[j + 1] - 1]
        assert np.all(np.diff(r) > 0)
    if nzval.size:
        assert relerr(S.nzval, nzval) <= TOL[np.dtype(dtype)]
    assert np.all(S.nzval != 0)


def _forms(wx, oracle, M, wt, L, eps, band):
    """both forms of M on host and device against the restatement, after the CPU check that no entry sits within `band` of the
    threshold (where the pattern could legitimately flip)"""
    dtype = M.dtype
    for std in (True, False):
        Mw = ref.sft(oracle, M, wt.qmf, L) if std else ref.dwt(oracle, M, wt.qmf, L)
        assert ref.near_threshold(Mw, eps, band) == 0, "an entry of the restatement lies in the band around the threshold"
        R = (ref.mat2sparseform_std if std else ref.mat2sparseform_nonstd)(oracle, M, wt.qmf, L, eps)
        fn = wx.mat2sparseform_std if std else wx.mat2sparseform_nonstd
        _same_sparse(fn(M, wt, L, eps), R, dtype)
        _same_sparse(fn(wx.to_device(M, "cuda:0"), wt, L, eps), R, dtype)


def test_sparse_form_literals(wx, filt, kats):
    k = kats["sparse"]
    x = np.asfortranarray(np.array(k["x"]))
    for fn, key in ((wx.mat2sparseform_nonstd, "nonstd_4"), (wx.mat2sparseform_std, "std_4")):
        lit = np.array(k[key], dtype=np.float64)
        for arg in (x, wx.to_device(x, "cuda:0")):
            S = fn(arg, filt["haar"])
            A = S.todense()
            assert np.abs(_r4(A) - lit).max() < 1e-9
            assert np.array_equal(A != 0, lit != 0) and S.nnz == np.count_nonzero(lit)


@pytest.mark.parametrize("eps", [1e-4, 1e-2])
@pytest.mark.parametrize("fname", ["haar", "db4"])
@pytest.mark.parametrize("n", [64, 256])
def test_sparse_forms_f64(wx, oracle, filt, n, fname, eps):
    M = ref.calderon(n)
    for L in (3, ref.maxtransformlevels(n)):
        _forms(wx, oracle, M, filt[fname], L, eps, 1e-9)


@pytest.mark.parametrize("fname", ["haar", "db4"])
def test_sparse_forms_f32(wx, oracle, filt, fname):
    M = ref.calderon(64, np.float32)
    for L in (3, 6):
        _forms(wx, oracle, M, filt[fname], L, 1e-2, 1e-3)


def _skewed(N, dtype=np.float64):
    """one dense row, one dense column and a diagonal"""
    rng = np.random.default_rng(N)
    A = np.zeros((N, N), dtype=dtype, order="F")
    A[np.arange(N), np.arange(N)] = rng.standard_normal(N)
    A[N // 3, :] = rng.standard_normal(N)
    A[:, 2 * N // 3] = rng.standard_normal(N)
    return A


@pytest.mark.parametrize("dtype", DTYPES)
def test_sparse_form_edge_cases(wx, oracle, filt, dtype):
    wt = filt["db4"]
    n = 64
    band = 1e-9 if dtype == np.float64 else 1e-3
    Z = np.zeros((n, n), dtype=dtype, order="F")
    X = np.asfortranarray(np.random.default_rng(1).standard_normal((n, 5)).astype(dtype))
    for fn, mul in ((wx.mat2sparseform_std, wx.std_wavemultall), (wx.mat2sparseform_nonstd, wx.nonstd_wavemultall)):
        S = fn(Z, wt)
        assert S.nnz == 0 and np.all(S.colptr == 1)
        Y = mul(S, X, wt)
        assert Y.shape == X.shape and np.all(Y == 0.0)
    # eps = 0 keeps every non-zero: the pattern is that of the restatement's transform
    M = np.asfortranarray(np.random.default_rng(2).standard_normal((n, n)).astype(dtype))
    _forms(wx, oracle, M, wt, 3, 0.0, 0.0)
    assert wx.mat2sparseform_std(M, wt, 3, 0.0).nnz == n * n
    # skewed rows and columns
    _forms(wx, oracle, _skewed(n, dtype), wt, 6, 1e-2, band)


# ------------------------------------------------------------------------------------------------------------------------------
# products
# ------------------------------------------------------------------------------------------------------------------------------
def _as_f64(S):
    return (S[0], S[1], S[2], S[3].astype(np.float64))


def _product_case(wx, oracle, wt, S, X, L, nonstd, batches):
    """wx.*_wavemultall with the restatement's sparse tuple S against the restatement, for every batch size, host and device"""
    dtype = X.dtype
    rmul = ref.nonstd_wavemultall if nonstd else ref.std_wavemultall
    mul = wx.nonstd_wavemultall if nonstd else wx.std_wavemultall
    want = rmul(oracle, S, X, wt.qmf, L)
    tol = TOL[np.dtype(dtype)]
    if dtype == np.float32:
        want64 = rmul(oracle, _as_f64(S), X.astype(np.float64), wt.qmf, L)
        own = relerr(want, want64)
        tol = max(tol, 4 * own)
        print("Float32 restatement vs Float64 restatement: %.2e -> tolerance %.2e" % (own, tol))
    SM = wx.SparseMatrixCSC(S[0], S[0], S[1], S[2], S[3])
    for B in batches:
        h, d = _both(wx, lambda a: mul(SM, a, wt, L), X[:, :B])
        for got in (h, d):
            assert got.shape == (X.shape[0], B) and got.dtype == dtype
            e = relerr(got, want[:, :B])
            print("%s n=%d B=%d %s relerr %.2e" % (mul.__name__, X.shape[0], B, np.dtype(dtype).name, e))
            assert e <= tol
        assert np.array_equal(h, d)                                          # host staging changes nothing
        again = mul(SM, np.asfortranarray(X[:, :B]), wt, L)
        assert np.array_equal(h, again)                                      # two applications of one plan: identical bits
    return SM


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("nonstd", [False, True], ids=["std", "nonstd"])
@pytest.mark.parametrize("n", [4, 64, 256, 1024])
def test_products_against_the_restatement(wx, oracle, filt, n, nonstd, dtype):
    wt = filt["haar"] if n == 4 else filt["db4"]
    M = ref.calderon(n, dtype)
    L = ref.maxtransformlevels(n)
    S = (ref.mat2sparseform_nonstd if nonstd else ref.mat2sparseform_std)(oracle, M, wt.qmf, L, 1e-4)
    X = np.asfortranarray(np.random.default_rng(n).standard_normal((n, 130)).astype(dtype))
    _product_case(wx, oracle, wt, S, X, L, nonstd, (1, 5, 64, 130))
    if n == 64:                                                              # fewer levels than the signal has
        S3 = (ref.mat2sparseform_nonstd if nonstd else ref.mat2sparseform_std)(oracle, M, wt.qmf, 3, 1e-4)
        _product_case(wx, oracle, wt, S3, X, 3, nonstd, (5,))


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("nonstd", [False, True], ids=["std", "nonstd"])
def test_products_with_skewed_rows(wx, oracle, filt, nonstd, dtype):
    """an operator with one dense row and one dense column: the dense row is cut into pieces that are added in a fixed order"""
    n = 256
    N = 2 * n if nonstd else n
    A = _skewed(N, dtype)
    jj, ii = np.nonzero(A.T)
    S = ref._sparse(ii + 1, jj + 1, A[ii, jj], N)
    X = np.asfortranarray(np.random.default_rng(3).standard_normal((n, 130)).astype(dtype))
    SM = _product_case(wx, oracle, filt["db4"], S, X, 8, nonstd, (1, 5, 64, 130))
    info = SM.plan_info()
    assert info["split_rows"] >= 1 and info["nnz"] == S[3].size


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("N", [1, 3, 64, 65, 200, 1024])
def test_sparse_product_alone(wx, N, dtype):
    """A * X of the product kernel against the dense product: sizes below, at and across a slice of 64 rows, tiles of 32 signals
    with a remainder, a matrix with empty rows and columns, rows cut into pieces"""
    rng = np.random.default_rng(N)
    A = _skewed(N, dtype) if N >= 64 else np.asfortranarray(rng.standard_normal((N, N)).astype(dtype))
    if N >= 64:
        A[5, :] = 0
        A[:, 7] = 0
    S = wx.SparseMatrixCSC.fromdense(A)
    for B in (1, 31, 32, 33, 130):
        X = np.asfortranarray(rng.standard_normal((N, B)).astype(dtype))
        want = A.astype(np.float64) @ X.astype(np.float64)
        h, d = _both(wx, S.matmul, X)
        assert h.shape == (N, B) and h.dtype == dtype and np.array_equal(h, d)
        assert relerr(h, want) <= (1e-13 if dtype == np.float64 else 1e-5)
        if N >= 64:
            assert np.all(h[5] == 0.0)
    assert np.array_equal(S.matmul(X[:, 0].copy()), h[:, 0])
    if N >= 200:
        assert S.plan_info()["split_rows"] >= 1


def test_product_literals(wx, filt, kats):
    k = kats["product"]
    M, x = ref.calderon(k["n"]), np.array(k["x"])
    for fn in (wx.nonstd_wavemult, wx.std_wavemult):
        for got in _both(wx, lambda m, v: fn(m, v, filt["haar"]), M, x):
            assert got.shape == (4,)
            assert np.abs(_r4(got) - np.array(k["y_4"])).max() < 1e-9


@pytest.mark.parametrize("n", [4, 64, 256])
def test_products_equal_the_dense_product_at_eps_zero(wx, filt, n):
    """needs no restatement: with nothing dropped both forms are M X"""
    rng = np.random.default_rng(n)
    M = np.asfortranarray(rng.standard_normal((n, n)))
    X = np.asfortranarray(rng.standard_normal((n, 37)))
    want = M @ X
    for wt in (filt["haar"], filt["db4"]):
        for L in sorted({1, ref.maxtransformlevels(n)}):
            for form, mul in ((wx.mat2sparseform_std, wx.std_wavemultall), (wx.mat2sparseform_nonstd, wx.nonstd_wavemultall)):
                S = form(M, wt, L, 0.0)
                assert relerr(mul(S, X, wt, L), want) <= 1e-10, (n, L, form.__name__)


@pytest.mark.parametrize("dtype", DTYPES)
def test_dense_forms_equal_the_two_step_forms(wx, filt, dtype):
    """wavemult.jl:58-65, 134-141: the docstrings' `y0 == y1`"""
    n, wt = 64, filt["db4"]
    M = ref.calderon(n, dtype)
    rng = np.random.default_rng(9)
    x = rng.standard_normal(n).astype(dtype)
    X = np.asfortranarray(rng.standard_normal((n, 5)).astype(dtype))
    for L, eps in ((6, 1e-4), (3, 1e-2)):
        for form, one, many in ((wx.mat2sparseform_std, wx.std_wavemult, wx.std_wavemultall),
                                (wx.mat2sparseform_nonstd, wx.nonstd_wavemult, wx.nonstd_wavemultall)):
            S = form(M, wt, L, eps)
            assert np.array_equal(one(S, x, wt, L), one(M, x, wt, L, eps))
            assert np.array_equal(many(S, X, wt, L), many(M, X, wt, L, eps))
            assert np.array_equal(one(S, X[:, 2].copy(), wt, L), many(S, X, wt, L)[:, 2])


# ------------------------------------------------------------------------------------------------------------------------------
# errors
# ------------------------------------------------------------------------------------------------------------------------------
def test_errors_python(wx, filt):
    wt = filt["db4"]
    x, M = np.zeros(16), np.zeros((16, 16), order="F")
    X = np.zeros((16, 3), order="F")
    S, NS = wx.mat2sparseform_std(M, wt), wx.mat2sparseform_nonstd(M, wt)
    for L in (0, 5):
        for call in (lambda: wx.ns_dwt(x, wt, L), lambda: wx.ns_idwt(np.zeros(32), wt, L), lambda: wx.ns_dwtall(X, wt, L),
                     lambda: wx.sft(M, wt, L), lambda: wx.isft(M, wt, L), lambda: wx.mat2sparseform_nonstd(M, wt, L),
                     lambda: wx.nonstd_wavemult(NS, x, wt, L), lambda: wx.nonstd_wavemultall(NS, X, wt, L)):
            with pytest.raises(AssertionError):
                call()
    with pytest.raises(AssertionError):
        wx.std_wavemult(S, x, wt, 5)
    with pytest.raises(AssertionError):
        wx.mat2sparseform_std(M, wt, 5)
    for call in (lambda: wx.mat2sparseform_std(np.zeros((16, 8)), wt), lambda: wx.mat2sparseform_nonstd(np.zeros((16, 8)), wt),
                 lambda: wx.ns_dwt(np.zeros(12), wt), lambda: wx.ns_dwtall(np.zeros((24, 2)), wt),
                 lambda: wx.std_wavemult(S, np.zeros(12), wt), lambda: wx.nonstd_wavemult(NS, np.zeros(12), wt),
                 lambda: wx.std_wavemult(NS, x, wt), lambda: wx.nonstd_wavemult(S, x, wt),            # a plan of the wrong size
                 lambda: wx.std_wavemultall(S, np.zeros((32, 2)), wt)):
        with pytest.raises(AssertionError):
            call()


def test_errors_c_abi(wx, filt):
    """the same refusals from the library itself: WX_EASSERT before anything is launched (the data pointers are never read)"""
    from waveletsext_jl_amd import _lib
    L = _lib.lib()
    q = np.ascontiguousarray(filt["db4"].qmf)
    qp, F = ctypes.c_void_p(q.ctypes.data), q.size
    x, y, w = np.zeros(16), np.zeros(16), np.zeros(32)
    M = np.zeros((16, 16), order="F")
    p = lambda a: ctypes.c_void_p(a.ctypes.data)      # noqa: E731
    E = _lib.WX_EASSERT
    for lv in (0, 5):
        assert L.wx_ns_dwt1d_f64(p(x), p(w), 16, lv, 1, qp, F, None) == E
        assert L.wx_ns_idwt1d_f64(p(w), p(x), 16, lv, 1, qp, F, None) == E
        assert L.wx_sft_f64(p(M), p(M.copy(order="F")), 16, 16, lv, 0, qp, F, None) == E
    assert L.wx_ns_dwt1d_f64(p(x), p(w), 12, 1, 1, qp, F, None) == E
    colptr = np.zeros(33, dtype=np.int64)
    thr = np.zeros(1)
    assert L.wx_sparseform_count_f64(p(M), 16, 5, 1e-4, p(colptr), p(thr), None) == E
    assert L.wx_sparseform_count_f64(p(np.zeros((12, 12), order="F")), 12, 1, 1e-4, p(colptr), p(thr), None) == E
    S, NS = wx.mat2sparseform_std(M, filt["db4"]), wx.mat2sparseform_nonstd(M, filt["db4"])
    assert L.wx_wavemult_apply_f64(S.plan(), 1, p(x), p(y), 16, 4, 1, qp, F, None) == E         # N = 16, needs 32
    assert L.wx_wavemult_apply_f64(NS.plan(), 0, p(x), p(y), 16, 4, 1, qp, F, None) == E
    assert L.wx_wavemult_apply_f64(NS.plan(), 1, p(x), p(y), 16, 0, 1, qp, F, None) == E
    assert L.wx_wavemult_apply_f64(S.plan(), 0, p(x), p(y), 16, 5, 1, qp, F, None) == E
    with pytest.raises(AssertionError):
        _lib.check(L.wx_wavemult_apply_f64(S.plan(), 0, p(x), p(y), 16, 5, 1, qp, F, None))
    # a plan survives wx_shutdown and still works
    wx.shutdown()
    assert L.wx_wavemult_apply_f64(S.plan(), 0, p(x), p(y), 16, 4, 1, qp, F, None) == 0
