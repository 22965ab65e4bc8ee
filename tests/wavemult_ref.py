"""numpy restatement of the reference's WaveMult module, the yardstick of tests/test_wavemult_cpu.py and
tests/test_gpu_wavemult.py.

The eight functions of src/mod/wavemult/{transforms,mat2sparse,wavemult}.jl and the three helpers of utils.jl in the reference's
loop order, on the CPU oracle's dwt_step / idwt_step / wpt / iwpt (`o` is the `oracle` fixture: Float32 inputs round at every
accumulate there).  Sparse matrices are (N, colptr, rowval, nzval) with Julia's 1-based Int64 arrays, what `sparse(...)` builds:
columns in order, rows ascending inside a column.  `norm` of a column is the square root of the Float64 sum of squares rounded to
the element type (Julia's own summation order is not pinned by any literal); the sparse product adds one column at a time with a
separate multiply and add in the element type, like SparseArrays' `*`.
"""
import warnings

import numpy as np


# ---- utils.jl ---------------------------------------------------------------------------------------------------------------
def maxtransformlevels(n):
    n, tl = int(n), 0
    if n < 2:
        return 0
    while n % 2 == 0:
        n //= 2
        tl += 1
    return tl


def dyadlength(n):
    """utils.jl:44-50"""
    J = int(np.ceil(np.log2(n)))
    if (1 << J) != n:
        warnings.warn("Dyadlength n != 2^J")
    return J


def stretchmatrix(i, j, n, L):
    """utils.jl:98-114"""
    Lmax = maxtransformlevels(n)
    assert 1 <= L <= Lmax
    ie, je = np.array(i, dtype=np.int64), np.array(j, dtype=np.int64)
    for l in range(0, L):
        k = Lmax - l - 1
        cond = ((ie > (1 << k)) | (je > (1 << k))) & ((ie <= (1 << (k + 1))) & (je <= (1 << (k + 1))))
        idx = np.nonzero(cond)[0]
        if idx.size:
            ie[idx] = ie[idx] + (1 << (k + 1))
            je[idx] = je[idx] + (1 << (k + 1))
    return ie, je


def ndyad(L, Lmax, gender):
    """utils.jl:146-155 -> (lo, hi), 1-based inclusive"""
    assert L <= Lmax
    assert L >= 1
    k = Lmax - L
    if gender:
        return (1 << (k + 1)) + (1 << k) + 1, 1 << (k + 2)
    return (1 << (k + 1)) + 1, (1 << (k + 1)) + (1 << k)


def stretch_closed_form(n, L):
    """The closed form of stretchmatrix that the fill kernel uses: for every output column c (1-based, 1 .. 2n) the source column
    (0 = empty), the first and last source row and the shift of the row indices."""
    Lmax = maxtransformlevels(n)
    assert 1 <= L <= Lmax
    K = Lmax - L
    out = []
    for c in range(1, 2 * n + 1):
        if c <= (1 << K):
            out.append((c, 1, 1 << K, 0))
        elif c <= (1 << (K + 1)):
            out.append((0, 1, 0, 0))
        else:
            k = (c - 1).bit_length() - 2                     # c in (2^(k+1), 2^(k+2)]
            j = c - (1 << (k + 1))
            out.append((j, 1 if j > (1 << k) else (1 << k) + 1, 1 << (k + 1), 1 << (k + 1)))
    return out


# ---- transforms.jl ----------------------------------------------------------------------------------------------------------
def _sl(rng):
    return slice(rng[0] - 1, rng[1])


def ns_dwt(o, x, qmf, L=None):
    """transforms.jl:52-70"""
    x = np.asarray(x)
    n = x.shape[0]
    Lmax = maxtransformlevels(n)
    L = Lmax if L is None else L
    assert 1 <= L <= Lmax
    assert n & (n - 1) == 0
    nxw = np.zeros(2 * n, dtype=x.dtype)
    g, h = o.makereverseqmfpair(qmf)
    for l in range(1, L + 1):
        v = x if l == 1 else nxw[_sl(ndyad(l - 1, Lmax, False))]
        w1, w2 = o.dwt_step(np.ascontiguousarray(v), h, g)
        nxw[_sl(ndyad(l, Lmax, False))] = w1
        nxw[_sl(ndyad(l, Lmax, True))] = w2
    nxw[:1 << (Lmax - L)] = nxw[_sl(ndyad(L, Lmax, False))]
    return nxw


def ns_idwt(o, nxw, qmf, L=None):
    """transforms.jl:124-142"""
    nxw = np.asarray(nxw)
    Lmax = maxtransformlevels(nxw.shape[0]) - 1
    n = nxw.shape[0] // 2
    L = Lmax if L is None else L
    assert 1 <= L <= Lmax
    assert n & (n - 1) == 0
    x = np.zeros(n, dtype=nxw.dtype)
    x[:1 << (Lmax - L)] = nxw[:1 << (Lmax - L)]
    g, h = o.makereverseqmfpair(qmf)
    for l in range(L, 0, -1):
        w1 = nxw[_sl(ndyad(l, Lmax, False))] + x[:1 << (Lmax - l)]
        w2 = nxw[_sl(ndyad(l, Lmax, True))]
        x[:1 << (Lmax - l + 1)] = o.idwt_step(np.ascontiguousarray(w1), np.ascontiguousarray(w2), h, g)
    return x


def dwt(o, x, qmf, L):
    """Wavelets.jl dwt of a vector or a square matrix: the packet transform along the :dwt tree (test/transforms.jl:42)"""
    x = np.asarray(x)
    if L == 0:
        return x.copy()
    tree = o.maketree1d(x.shape[0], L, "dwt") if x.ndim == 1 else o.maketree2d(x.shape[0], x.shape[1], L, "dwt")
    return o.wpt(x, qmf, tree)


def idwt(o, xw, qmf, L):
    xw = np.asarray(xw)
    if L == 0:
        return xw.copy()
    return o.iwpt(xw, qmf, o.maketree1d(xw.shape[0], L, "dwt"))


def sft(o, M, qmf, L=None):
    """transforms.jl:171-185"""
    M = np.asarray(M)
    Lmax = maxtransformlevels(min(M.shape))
    L = Lmax if L is None else L
    assert 1 <= L <= Lmax
    n, m = M.shape
    Mw = np.empty_like(M, order="F")
    for j in range(m):
        Mw[:, j] = dwt(o, np.ascontiguousarray(M[:, j]), qmf, L)
    for i in range(n):
        Mw[i, :] = dwt(o, np.ascontiguousarray(Mw[i, :]), qmf, L)
    return Mw


def isft(o, Mw, qmf, L=None):
    """transforms.jl:214-228"""
    Mw = np.asarray(Mw)
    Lmax = maxtransformlevels(min(Mw.shape))
    L = Lmax if L is None else L
    assert 1 <= L <= Lmax
    n, m = Mw.shape
    M = np.empty_like(Mw, order="F")
    for i in range(n):
        M[i, :] = idwt(o, np.ascontiguousarray(Mw[i, :]), qmf, L)
    for j in range(m):
        M[:, j] = idwt(o, np.ascontiguousarray(M[:, j]), qmf, L)
    return M


# ---- mat2sparse.jl ----------------------------------------------------------------------------------------------------------
def threshold_of(Mw, eps):
    """T(eps) * maximum column norm, in the element type (mat2sparse.jl:46-47, 96-97)"""
    T = Mw.dtype.type
    nrm = np.sqrt((Mw.astype(np.float64) ** 2).sum(axis=0)).astype(Mw.dtype)
    return T(T(eps) * nrm.max())


def _sparse(ie, je, vals, N):
    """sparse(ie, je, vals, N, N) for distinct (ie, je), 1-based"""
    order = np.lexsort((ie, je))
    ie, je, vals = ie[order], je[order], vals[order]
    colptr = np.concatenate(([1], 1 + np.cumsum(np.bincount(je - 1, minlength=N)))).astype(np.int64)
    return N, colptr, ie.astype(np.int64), vals


def _kept(Mw, eps):
    thr = threshold_of(Mw, eps)
    nil = Mw * (np.abs(Mw) > thr)
    jj, ii = np.nonzero(nil.T)                             # column by column, rows ascending: findall(!iszero, nilMw)
    return ii + 1, jj + 1, nil[ii, jj], thr


def near_threshold(Mw, eps, rel):
    """number of entries of Mw whose magnitude lies within a relative `rel` of the threshold"""
    thr = float(threshold_of(Mw, eps))
    return int((np.abs(np.abs(Mw.astype(np.float64)) - thr) <= rel * thr).sum()) if thr > 0 else 0


def mat2sparseform_std(o, M, qmf, L=None, eps=1e-4):
    """mat2sparse.jl:89-100"""
    M = np.asarray(M)
    assert M.shape[0] == M.shape[1]
    ii, jj, vals, _ = _kept(sft(o, M, qmf, L), eps)
    return _sparse(ii, jj, vals, M.shape[0])


def mat2sparseform_nonstd(o, M, qmf, L=None, eps=1e-4):
    """mat2sparse.jl:38-55"""
    M = np.asarray(M)
    assert M.shape[0] == M.shape[1]
    n = M.shape[0]
    L = maxtransformlevels(n) if L is None else L
    ii, jj, vals, _ = _kept(dwt(o, M, qmf, L), eps)
    ie, je = stretchmatrix(ii, jj, n, L)
    return _sparse(ie, je, vals, 2 * n)


def todense(S):
    N, colptr, rowval, nzval = S
    A = np.zeros((N, N), dtype=nzval.dtype, order="F")
    A[rowval - 1, np.repeat(np.arange(N), np.diff(colptr))] = nzval
    return A


def spmv(S, x):
    """SparseArrays' A * x: y[rowval[k]] += nzval[k] * x[j], column by column, in the element type; x (N,) or (N, B)"""
    N, colptr, rowval, nzval = S
    x = np.asarray(x)
    y = np.zeros((N,) + x.shape[1:], dtype=nzval.dtype)
    for j in range(N):
        lo, hi = colptr[j] - 1, colptr[j + 1] - 1
        if hi > lo:
            v = nzval[lo:hi]
            y[rowval[lo:hi] - 1] += (v * x[j]) if x.ndim == 1 else (v[:, None] * x[j][None, :])
    return y


# ---- wavemult.jl ------------------------------------------------------------------------------------------------------------
def std_wavemult(o, SM, x, qmf, L=None, eps=1e-4):
    """wavemult.jl:134-152; SM is a sparse tuple or a dense matrix"""
    x = np.asarray(x)
    L = maxtransformlevels(x.shape[0]) if L is None else L
    if not isinstance(SM, tuple):
        SM = mat2sparseform_std(o, SM, qmf, L, eps)
    return idwt(o, spmv(SM, dwt(o, x, qmf, L)), qmf, L)


def nonstd_wavemult(o, NM, x, qmf, L=None, eps=1e-4):
    """wavemult.jl:58-76"""
    x = np.asarray(x)
    L = maxtransformlevels(x.shape[0]) if L is None else L
    if not isinstance(NM, tuple):
        NM = mat2sparseform_nonstd(o, NM, qmf, L, eps)
    return ns_idwt(o, spmv(NM, ns_dwt(o, x, qmf, L)), qmf, L)


def columns(fn, o, X, qmf, *args):
    """fn(o, x, qmf, ...) over the columns of X"""
    X = np.asarray(X)
    return np.asfortranarray(np.stack([fn(o, np.ascontiguousarray(X[:, b]), qmf, *args) for b in range(X.shape[1])], axis=1))


def std_wavemultall(o, SM, X, qmf, L=None):
    """std_wavemult of every column of X with the sparse tuple SM (the product itself runs on the whole batch, same order)"""
    L = maxtransformlevels(X.shape[0]) if L is None else L
    return columns(idwt, o, spmv(SM, columns(dwt, o, X, qmf, L)), qmf, L)


def nonstd_wavemultall(o, NM, X, qmf, L=None):
    L = maxtransformlevels(X.shape[0]) if L is None else L
    return columns(ns_idwt, o, spmv(NM, columns(ns_dwt, o, X, qmf, L)), qmf, L)


def calderon(n, dtype=np.float64):
    """M[i, j] = 1 / |i - j|, zero diagonal (test/wavemult.jl:73-78)"""
    i = np.arange(n)
    d = np.abs(i[:, None] - i[None, :]).astype(np.float64)
    with np.errstate(divide="ignore"):
        M = np.where(d > 0, 1.0 / d, 0.0)
    return np.asfortranarray(M.astype(dtype))
