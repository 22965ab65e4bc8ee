"""WaveMult: host-side mirror of the reference's `WaveMult` module (src/mod/WaveMult.jl, src/mod/wavemult/utils.jl,
transforms.jl, mat2sparse.jl, wavemult.jl) -- the Beylkin-Coifman-Rokhlin standard and non-standard forms of a matrix and the
products with them.  Same names, argument order, defaults and assertions; the `*all` drivers take a batch of vectors on the last
axis, which is what makes the product a GPU workload.  Integer helpers run here, everything else ends in the C ABI
(csrc/wx_wavemult.hip); there is no CPU path.
"""
import ctypes
import warnings

import numpy as np

from . import _lib
from ._arrays import Arg, qmf_arg
from .dwt import _call, dwt
from .util import maxtransformlevels


def _ispow2(n):
    return n >= 1 and (n & (n - 1)) == 0


# ---------------------------------------------------------------------------------------------
# utils.jl
# ---------------------------------------------------------------------------------------------
def dyadlength(x):
    """utils.jl:44-51: ceil(log2(n)), with a warning when n is not a power of two"""
    n = int(x) if isinstance(x, (int, np.integer)) else int(x.shape[0])
    J = (n - 1).bit_length()
    if (1 << J) != n:
        warnings.warn("Dyadlength n != 2^J")
    return J


def stretchmatrix(i, j, n, L):
    """utils.jl:98-114: 1-based (row, column) indices of an n x n matrix -> indices in the 2n x 2n non-standard form"""
    n, L = int(n), int(L)
    Lmax = maxtransformlevels(n)
    assert 1 <= L <= Lmax                                                    # utils.jl:101
    ie, je = np.array(i, dtype=np.int64), np.array(j, dtype=np.int64)
    for l in range(L):
        k = Lmax - l - 1
        cond = ((ie > (1 << k)) | (je > (1 << k))) & ((ie <= (1 << (k + 1))) & (je <= (1 << (k + 1))))
        ie[cond] += 1 << (k + 1)
        je[cond] += 1 << (k + 1)
    return ie, je


def ndyad(L, Lmax, gender):
    """utils.jl:146-155 -> 1-based inclusive range (python `range(lo, hi + 1)`); gender True = detail, False = approximation"""
    assert L <= Lmax                                                         # utils.jl:147
    assert L >= 1                                                            # utils.jl:148
    k = Lmax - L
    if gender:
        return range((1 << (k + 1)) + (1 << k) + 1, (1 << (k + 2)) + 1)
    return range((1 << (k + 1)) + 1, (1 << (k + 1)) + (1 << k) + 1)


# ---------------------------------------------------------------------------------------------
# SparseMatrixCSC{T,Int64}
# ---------------------------------------------------------------------------------------------
class SparseMatrixCSC:
    """The three arrays of Julia's SparseMatrixCSC{T,Int64}, 1-based, on the host: colptr (n + 1), rowval and nzval (nnz, rows
    ascending inside a column).  The device layout of the product (wx_wavemult_plan_create_*) is made on first use and lives as
    long as the object."""

    def __init__(self, m, n, colptr, rowval, nzval):
        self.m, self.n = int(m), int(n)
        self.colptr = np.ascontiguousarray(colptr, dtype=np.int64)
        self.rowval = np.ascontiguousarray(rowval, dtype=np.int64)
        self.nzval = np.ascontiguousarray(nzval)
        if self.nzval.dtype not in (np.float64, np.float32):
            raise TypeError("element type must be Float64 or Float32")
        assert self.colptr.size == self.n + 1 and self.rowval.size == self.nzval.size == self.colptr[-1] - 1
        self._plan = None

    @classmethod
    def fromdense(cls, A):
        """sparse(A): the non-zeros of a dense matrix, column by column"""
        A = np.asarray(A)
        cols, rows = np.nonzero(A.T)
        colptr = np.concatenate(([1], 1 + np.cumsum(np.bincount(cols, minlength=A.shape[1]))))
        return cls(A.shape[0], A.shape[1], colptr, rows + 1, A[rows, cols])

    @property
    def nnz(self):
        return int(self.nzval.size)

    @property
    def shape(self):
        return (self.m, self.n)

    def todense(self):
        A = np.zeros((self.m, self.n), dtype=self.nzval.dtype, order="F")
        cols = np.repeat(np.arange(self.n), np.diff(self.colptr))
        A[self.rowval - 1, cols] = self.nzval
        return A

    def plan(self, stream=None):
        if self._plan is None:
            assert self.m == self.n
            h = ctypes.c_void_p(0)
            suf = "_f64" if self.nzval.dtype == np.float64 else "_f32"
            _call("wx_wavemult_plan_create", suf, ctypes.c_void_p(self.colptr.ctypes.data), ctypes.c_void_p(self.rowval.ctypes.data),
                  ctypes.c_void_p(self.nzval.ctypes.data), self.n, ctypes.byref(h), stream or ctypes.c_void_p(0))
            self._plan = h
        return self._plan

    def matmul(self, X):
        """A * X for a vector or a batch of vectors X (n,) / (n, B) of the matrix's element type: the product kernel alone
        (wx_wavemult_product_*)"""
        X = Arg(X)
        assert self.m == self.n == X.shape[0]
        if X.dtype != self.nzval.dtype:
            raise TypeError("the sparse matrix and the vectors must have the same element type")
        Y = X.new(X.shape)
        _call("wx_wavemult_product", X.suffix, self.plan(), X.ptr, Y.ptr, int(np.prod(X.shape[1:], dtype=np.int64)), X.stream())
        return Y.arr

    def plan_info(self):
        """what the product reads: N, nnz, padded entries, slices, rows cut into pieces, longest piece, layout bytes, signals per
        workgroup (wx_wavemult_plan_info)"""
        info = np.zeros(8, dtype=np.int64)
        _lib.check(_lib.lib().wx_wavemult_plan_info(self.plan(), ctypes.c_void_p(info.ctypes.data)))
        return dict(zip(("N", "nnz", "padded", "slices", "split_rows", "cap", "layout_bytes", "tile"), info.tolist()))

    def __del__(self):
        h, self._plan = getattr(self, "_plan", None), None
        if h is not None:
            try:
                _lib.lib().wx_wavemult_plan_destroy(h)
            except Exception:       # interpreter shutdown
                pass


# ---------------------------------------------------------------------------------------------
# transforms.jl
# ---------------------------------------------------------------------------------------------
def _ns(name, x, wt, L, n, out_len, batched):
    Lmax = maxtransformlevels(n)
    L = Lmax if L is None else int(L)
    assert 1 <= L <= Lmax                                                    # transforms.jl:57,129
    assert _ispow2(n)                                                        # transforms.jl:58,130
    if batched:
        assert x.arr.ndim > 1
    else:
        assert x.arr.ndim == 1
    B = int(np.prod(x.shape[1:], dtype=np.int64))
    out = x.new((out_len,) + x.shape[1:])
    q, qp, F = qmf_arg(wt)
    _call(name, x.suffix, x.ptr, out.ptr, n, L, B, qp, F, x.stream())
    return out.arr


def ns_dwt(x, wt, L=None):
    """transforms.jl:52-70: x (n,) -> nxw (2n,)"""
    x = Arg(x)
    return _ns("wx_ns_dwt1d", x, wt, L, x.shape[0], 2 * x.shape[0], False)


def ns_idwt(nxw, wt, L=None):
    """transforms.jl:124-142: nxw (2n,) -> x (n,)"""
    nxw = Arg(nxw)
    return _ns("wx_ns_idwt1d", nxw, wt, L, nxw.shape[0] // 2, nxw.shape[0] // 2, False)


def ns_dwtall(x, wt, L=None):
    """ns_dwt of every column: x (n, B) -> (2n, B)"""
    x = Arg(x)
    return _ns("wx_ns_dwt1d", x, wt, L, x.shape[0], 2 * x.shape[0], True)


def ns_idwtall(nxw, wt, L=None):
    """ns_idwt of every column: nxw (2n, B) -> (n, B)"""
    nxw = Arg(nxw)
    return _ns("wx_ns_idwt1d", nxw, wt, L, nxw.shape[0] // 2, nxw.shape[0] // 2, True)


def _sft(M, wt, L, inverse):
    M = Arg(M)
    assert M.arr.ndim == 2
    Lmax = maxtransformlevels(int(min(M.shape)))
    L = Lmax if L is None else int(L)
    assert 1 <= L <= Lmax                                                    # transforms.jl:174,217
    out = M.new(M.shape)
    q, qp, F = qmf_arg(wt)
    _call("wx_sft", M.suffix, M.ptr, out.ptr, M.shape[0], M.shape[1], L, inverse, qp, F, M.stream())
    return out


def sft(M, wt, L=None):
    """transforms.jl:171-185"""
    return _sft(M, wt, L, 0).arr


def isft(Mw, wt, L=None):
    """transforms.jl:214-228"""
    return _sft(Mw, wt, L, 1).arr


# ---------------------------------------------------------------------------------------------
# mat2sparse.jl
# ---------------------------------------------------------------------------------------------
def _sparsify(Mw, L_nonstd, eps):
    """entries of Mw (an Arg, n x n) above eps * the largest column norm as a SparseMatrixCSC; L_nonstd >= 1 stretches"""
    n = Mw.shape[0]
    N = 2 * n if L_nonstd else n
    colptr = np.empty(N + 1, dtype=np.int64)
    thr = np.empty(1, dtype=Mw.dtype)
    _call("wx_sparseform_count", Mw.suffix, Mw.ptr, n, L_nonstd, float(eps), ctypes.c_void_p(colptr.ctypes.data),
          ctypes.c_void_p(thr.ctypes.data), Mw.stream())
    nnz = int(colptr[N]) - 1
    rowval = np.empty(nnz, dtype=np.int64)
    nzval = np.empty(nnz, dtype=Mw.dtype)
    _call("wx_sparseform_fill", Mw.suffix, Mw.ptr, n, L_nonstd, float(thr[0]), ctypes.c_void_p(colptr.ctypes.data),
          ctypes.c_void_p(rowval.ctypes.data), ctypes.c_void_p(nzval.ctypes.data), Mw.stream())
    return SparseMatrixCSC(N, N, colptr, rowval, nzval)


def mat2sparseform_nonstd(M, wt, L=None, eps=1e-4):
    """mat2sparse.jl:38-55 -> SparseMatrixCSC (2n, 2n)"""
    M = Arg(M)
    assert M.arr.ndim == 2 and M.shape[0] == M.shape[1]                      # mat2sparse.jl:42
    Lmax = maxtransformlevels(M.shape[0])
    L = Lmax if L is None else int(L)
    assert 1 <= L <= Lmax                                                    # dwt, then stretchmatrix (utils.jl:101)
    return _sparsify(Arg(dwt(M.arr, wt, L)), L, eps)


def mat2sparseform_std(M, wt, L=None, eps=1e-4):
    """mat2sparse.jl:89-100 -> SparseMatrixCSC (n, n)"""
    Ma = Arg(M)
    assert Ma.arr.ndim == 2 and Ma.shape[0] == Ma.shape[1]                   # mat2sparse.jl:93
    return _sparsify(_sft(Ma.arr, wt, L, 0), 0, eps)


# ---------------------------------------------------------------------------------------------
# wavemult.jl
# ---------------------------------------------------------------------------------------------
def _wavemult(A, x, wt, L, eps, nonstd, batched):
    x = Arg(x)
    assert x.arr.ndim > 1 if batched else x.arr.ndim == 1
    n = x.shape[0]
    Lmax = maxtransformlevels(n)
    L = Lmax if L is None else int(L)
    if not isinstance(A, SparseMatrixCSC):                                   # wavemult.jl:58-65, 134-141
        A = (mat2sparseform_nonstd if nonstd else mat2sparseform_std)(A, wt, L, eps)
    assert (1 if nonstd else 0) <= L <= Lmax                                 # ns_dwt transforms.jl:57 / dwt
    assert _ispow2(n)
    assert A.m == A.n == (2 * n if nonstd else n)
    if A.nzval.dtype != x.dtype:
        raise TypeError("the sparse matrix and the vectors must have the same element type")
    B = int(np.prod(x.shape[1:], dtype=np.int64))
    y = x.new(x.shape)
    q, qp, F = qmf_arg(wt)
    _call("wx_wavemult_apply", x.suffix, A.plan(), 1 if nonstd else 0, x.ptr, y.ptr, n, L, B, qp, F, x.stream())
    return y.arr


def nonstd_wavemult(M, x, wt, L=None, eps=1e-4):
    """wavemult.jl:58-76: M is a dense n x n matrix or the SparseMatrixCSC of mat2sparseform_nonstd; x (n,)"""
    return _wavemult(M, x, wt, L, eps, True, False)


def std_wavemult(M, x, wt, L=None, eps=1e-4):
    """wavemult.jl:134-152: M is a dense n x n matrix or the SparseMatrixCSC of mat2sparseform_std; x (n,)"""
    return _wavemult(M, x, wt, L, eps, False, False)


def nonstd_wavemultall(M, X, wt, L=None, eps=1e-4):
    """nonstd_wavemult of every column of X (n, B) with one compressed operator"""
    return _wavemult(M, X, wt, L, eps, True, True)


def std_wavemultall(M, X, wt, L=None, eps=1e-4):
    """std_wavemult of every column of X (n, B) with one compressed operator"""
    return _wavemult(M, X, wt, L, eps, False, True)
