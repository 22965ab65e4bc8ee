"""Denoising: host-side mirror of the reference's `Denoising` module (src/mod/Denoising.jl:214-232, 483-712) for
the VisuShrink family.  The two data-parallel steps -- the MAD noise estimate of every signal and the thresholding
of the coefficient table -- run on the device between the batch transforms; `denoiseall` is one pipeline for the
whole batch instead of the reference's loop over signals.  SURVEY section 8(f) row 1.

Wavelets.jl (`Threshold.HardTH/SoftTH/SemiSoftTH/SteinTH`, `VisuShrink`, `mad!`) is not vendored in the reference
tree; those pieces are restated from its published source.  The threshold selection of SureShrink and
RelErrorShrink (Denoising.jl:146-166, 285-381) is one workgroup per signal on the device (csrc/wx_shrink.hip), so
`denoiseall(...; estnoise = relerrorthreshold)` (test/denoising.jl:59-83) is one pipeline as well."""
import ctypes

import numpy as np

from . import _lib
from ._arrays import Arg, is_torch, to_numpy
from .dwt import dwt, dwtall, idwt, idwtall, iwpt, iwptall
from .swt import isdwt, isdwtall, iswpd, iswpdall
from .acwt import iacdwt, iacdwtall, iacwpd, iacwpdall
from .util import (coarsestscalingrange, finestdetailrange, getleaf, isdyadic, maketree, maxtransformlevels,
                   nodelength)


class HardTH:
    kind = 0


class SoftTH:
    kind = 1


class SemiSoftTH:
    kind = 2


class SteinTH:
    kind = 3


class VisuShrink:
    """VisuShrink(n) / VisuShrink(n, th) (Denoising.jl:124-126: t = sqrt(2 log n)) or VisuShrink(th, t)"""

    def __init__(self, a, b=None):
        if isinstance(a, (int, np.integer)):
            self.th = HardTH() if b is None else b
            self.t = float(np.sqrt(2 * np.log(int(a))))
        else:
            self.th, self.t = a, float(b)


class RelErrorShrink:
    """RelErrorShrink(th = HardTH(), t = 1.0) Denoising.jl:41-48"""

    def __init__(self, th=None, t=1.0):
        self.th = HardTH() if th is None else th
        self.t = float(t)


class SureShrink:
    """SureShrink(th, t) Denoising.jl:60-66, or SureShrink(xw[, redundant, tree, th]) Denoising.jl:97-103: the
    threshold is surethreshold(xw, redundant, tree)"""

    def __init__(self, a, b=False, tree=None, th=None):
        if isinstance(a, (HardTH, SoftTH, SemiSoftTH, SteinTH)):
            self.th, self.t = a, float(b)
        else:
            self.th = HardTH() if th is None else th
            self.t = surethreshold(a, bool(b), tree)


INPUTTYPES = ("sig", "dwt", "wpt", "sdwt", "swpd", "acdwt", "acwpd")


def _select(xa, batched, redundant, tree, kind, elbows=2):
    """surethreshold (kind 0) / relerrorthreshold (kind 1) of every signal: the selected coefficients are all of them,
    or the leaf columns of a redundant packet table (Denoising.jl:150-157, 293-300)"""
    n = xa.shape[0]
    N = xa.shape[-1] if batched else 1
    nd = xa.arr.ndim - (1 if batched else 0)
    k = 1 if nd == 1 else xa.shape[1]
    cm = None
    if redundant and tree is not None:
        leaves = np.asarray(getleaf(np.asarray(tree, dtype=bool), "binary"), dtype=bool)
        assert not leaves[k:].any(), "tree has leaves below the last column of the table"
        cm = np.ascontiguousarray(leaves[:k].astype(np.uint8))
    out = np.empty(N, dtype=xa.dtype)
    cmp = ctypes.c_void_p(cm.ctypes.data) if cm is not None else ctypes.c_void_p(0)
    if kind == 0:
        fn = getattr(_lib.lib(), "wx_surethreshold" + xa.suffix)
        _lib.check(fn(xa.ptr, n, k, N, cmp, ctypes.c_void_p(out.ctypes.data), xa.stream()))
    else:
        assert elbows >= 1                                             # Denoising.jl:291
        fn = getattr(_lib.lib(), "wx_relerrorthreshold" + xa.suffix)
        _lib.check(fn(xa.ptr, n, k, N, cmp, int(elbows), ctypes.c_void_p(out.ctypes.data), xa.stream()))
    return out


def _select_trees(xa, trees, kind, elbows=2):
    """wx_surethreshold_trees_* (kind 0) / wx_relerrorthreshold_trees_* (kind 1): the threshold of every signal over the leaf columns of
    its own tree in its redundant packet table (csrc/wx_shrink_trees.hip); an Arg of the table's kind with N values, on the device for a
    device table (nothing is copied to the host, the call waits only for the 128 bytes of group sizes)"""
    from ._arrays import trees_arg
    if xa.arr.ndim != 3:
        raise _lib.WxError(_lib.WX_EUNSUPPORTED, "a tree matrix (one tree per signal) needs 1-D signals: an (n, ncols, N) packet table")
    n, k, N = xa.shape
    tb, tp, nt = trees_arg(trees, N, xa)
    out = xa.new((N,))
    if kind == 0:
        fn = getattr(_lib.lib(), "wx_surethreshold_trees" + xa.suffix)
        _lib.check(fn(xa.ptr, n, k, tp, nt, N, out.ptr, xa.stream()))
    else:
        fn = getattr(_lib.lib(), "wx_relerrorthreshold_trees" + xa.suffix)
        _lib.check(fn(xa.ptr, n, k, tp, nt, N, int(elbows), out.ptr, xa.stream()))
    return out


def surethreshold(coef, redundant, tree=None):
    """surethreshold(coef, redundant[, tree]) Denoising.jl:146-166 for one decomposed signal"""
    return float(_select(Arg(coef), False, redundant, tree, 0)[0])


def relerrorthreshold(coef, redundant=False, tree=None, elbows=2):
    """relerrorthreshold(coef[, redundant, tree, elbows]) Denoising.jl:285-327 for one decomposed signal (the plot of
    makeplot = true belongs to the reference's Visualizations, out of scope)"""
    return float(_select(Arg(coef), False, redundant, tree, 1, elbows)[0])


def surethresholdall(coef, redundant, tree=None):
    """surethreshold of every signal of a batch (last axis), one launch.  redundant with `tree` an (n - 1, N) matrix, host or device:
    coef is the (n, ncols, N) packet table of swpdall / acwpdall (numpy or a device tensor) and signal i is selected over the leaf
    columns of column i of `tree`; the N thresholds come back as the table's kind (a device tensor for a device table)"""
    if redundant and _is_tree_matrix(tree):
        return _select_trees(Arg(coef), tree, 0).arr
    return _select(Arg(coef), True, redundant, tree, 0)


def relerrorthresholdall(coef, redundant=False, tree=None, elbows=2):
    """relerrorthreshold of every signal of a batch (last axis), one launch: what denoiseall evaluates signal by
    signal when estnoise = relerrorthreshold (Denoising.jl:676-680).  redundant with `tree` an (n - 1, N) matrix: one tree per
    signal, as surethresholdall"""
    if redundant and _is_tree_matrix(tree):
        return _select_trees(Arg(coef), tree, 1, elbows).arr
    return _select(Arg(coef), True, redundant, tree, 1, elbows)


def _detail_range(n, k, inputtype, tree):
    """(row_lo, col) 0-based of the finest detail coefficients, as noisest picks them (Denoising.jl:221-230)"""
    if inputtype == "dwt":
        return n // 2, 0
    if inputtype == "wpt":
        return finestdetailrange(n, tree)[0] - 1, 0
    if inputtype in ("sdwt", "acdwt"):
        return 0, k - 1
    return 0, finestdetailrange(n, tree, True)[1] - 1


def _noisest(xa, batched, inputtype, tree, on_device=False):
    """sigma of every signal; on_device: an Arg of the input's kind (nothing is copied to the host, no synchronisation)"""
    n = xa.shape[0]
    assert isdyadic(n)                                                 # Denoising.jl:218
    N = xa.shape[-1] if batched else 1
    k = 1 if inputtype in ("dwt", "wpt") else xa.shape[1]
    lo, col = _detail_range(n, k, inputtype, tree)
    fn = getattr(_lib.lib(), "wx_noisest" + xa.suffix)
    if on_device:
        sig = xa.new((N,))
        _lib.check(fn(xa.ptr, n, k, N, lo, col, sig.ptr, xa.stream()))
        return sig
    sig = np.empty(N, dtype=xa.dtype)
    _lib.check(fn(xa.ptr, n, k, N, lo, col, ctypes.c_void_p(sig.ctypes.data), xa.stream()))
    return sig


def noisest(x, redundant, tree=None):
    """noisest(x, redundant[, tree]) Denoising.jl:214-232 for one decomposed signal"""
    xa = Arg(x)
    it = ("sdwt" if tree is None else "swpd") if redundant else ("dwt" if tree is None else "wpt")
    return float(_noisest(xa, False, it, None if tree is None else np.asarray(tree, dtype=bool))[0])


def _threshold(xa, out, batched, th, t, row_lo=0, colmask=None):
    """out = threshold(xa) on the selected rows / columns (out is xa: in place)"""
    n = xa.shape[0]
    N = xa.shape[-1] if batched else 1
    k = 1 if xa.arr.ndim - (1 if batched else 0) == 1 else xa.shape[1]
    tv = np.ascontiguousarray(np.atleast_1d(np.asarray(t, dtype=xa.dtype)))
    cm = None if colmask is None else np.ascontiguousarray(np.asarray(colmask, dtype=np.uint8))
    fn = getattr(_lib.lib(), "wx_threshold" + xa.suffix)
    _lib.check(fn(xa.ptr, out.ptr, n, k, N, th.kind, ctypes.c_void_p(tv.ctypes.data), tv.size, int(row_lo),
                  ctypes.c_void_p(cm.ctypes.data) if cm is not None else ctypes.c_void_p(0), xa.stream()))


def _iwpt_thresh(xa, wt, tree, batched, th, t, row_lo, scale=1.0):
    """threshold(x, th, scale * t) on rows [row_lo, n) followed by iwpt(x, wt, tree), in one pass (wx_iwpt1d_thresh_*);
    t: host values, or an Arg on the device (the noise estimates where wx_noisest_* left them)"""
    from ._arrays import qmf_arg, tree_arg
    n = xa.shape[0]
    N = xa.shape[-1] if batched else 1
    q, qp, F = qmf_arg(wt)
    tk, tp, nt = tree_arg(np.asarray(tree, dtype=bool))
    if isinstance(t, Arg):
        tptr, tn = t.ptr, int(np.prod(t.shape))
    else:
        tv = np.ascontiguousarray(np.atleast_1d(np.asarray(t, dtype=xa.dtype)))
        tptr, tn = ctypes.c_void_p(tv.ctypes.data), tv.size
    out = xa.new(xa.shape)
    fn = getattr(_lib.lib(), "wx_iwpt1d_thresh" + xa.suffix)
    _lib.check(fn(xa.ptr, out.ptr, n, 0, tp, nt, N, qp, F, th.kind, tptr, tn, int(row_lo), float(scale), xa.stream()))
    return out.arr


def threshold(x, th, t):
    """Wavelets.Threshold.threshold(x, TH, t): thresholded copy"""
    xa = Arg(x)
    out = xa.new(xa.shape)
    _threshold(xa, out, False, th, t)
    return out.arr


def _denoise_sig(xa, wt, L, dnt, smooth, batched, entry="wx_denoiseall_sig"):
    """denoise / denoiseall(x, :sig | :dwt, wt; L, dnt, smooth) with estnoise = noisest (Denoising.jl:483-599, 651-712): wx_denoiseall_sig_* /
    wx_denoiseall_dwt_*"""
    from ._arrays import qmf_arg
    n = xa.shape[0]
    N = xa.shape[-1] if batched else 1
    q, qp, F = qmf_arg(wt)
    out = xa.new(xa.shape)
    fn = getattr(_lib.lib(), entry + xa.suffix)
    _lib.check(fn(xa.ptr, out.ptr, n, int(L), N, qp, F, dnt.th.kind, float(dnt.t), 1 if smooth == "undersmooth" else 0,
                  ctypes.c_void_p(0), xa.stream()))
    return out.arr


def _is_tree_matrix(tree):
    """one tree per signal: an (n - 1, N) matrix, on the host or (bestbasistreeall(..., device=True)) on the device"""
    if is_torch(tree):
        return tree.dim() == 2
    return tree is not None and np.ndim(tree) == 2


def _thr_arg(thr, dtype):
    """(buffer kept alive, pointer, count) of the thresholds of a per-signal-tree entry: None, host values, or an Arg (a device pointer)"""
    if thr is None:
        return None, ctypes.c_void_p(0), 0
    if isinstance(thr, Arg):
        return thr, thr.ptr, int(np.prod(thr.shape))
    tv = np.ascontiguousarray(np.atleast_1d(np.asarray(thr, dtype=dtype)))
    return tv, ctypes.c_void_p(tv.ctypes.data), tv.size


def _trees_call(xa, N, wt, trees, th_kind, scale, thr, smooth, want_out, want_sigma, inputtype="wpt"):
    """wx_denoise_wpt1d_trees_* / wx_denoise_swpd1d_trees_* / wx_denoise_acwpd1d_trees_f64: (xhat | None, sigma | None) as Args of the input's
    kind; thr: None (the noise is estimated per signal, each on the finest detail node of its own tree), 1 / N host values, or an Arg on the
    device (what _select_trees left there): the thresholds before scaling.  A redundant table (n, ncols, N) gives (n, N) signals, or with :swpd and wt = None the thresholded table"""
    from ._arrays import qmf_arg, trees_arg
    null = ctypes.c_void_p(0)
    q, qp, F = (None, null, 0) if wt is None else qmf_arg(wt)
    tb, tp, nt = trees_arg(trees, N, xa)
    n = xa.shape[0]
    if inputtype == "wpt" or (inputtype == "swpd" and wt is None):
        oshape = tuple(xa.shape)
    else:
        oshape = (n,) + tuple(xa.shape[2:])                            # (n, ncols[, N]) -> (n[, N])
    out = xa.new(oshape) if want_out else None
    sig = xa.new((N,)) if want_sigma else None
    tv, tvp, tvn = _thr_arg(thr, xa.dtype)
    tail = (int(th_kind), float(scale), tvp, tvn, 1 if smooth == "undersmooth" else 0, sig.ptr if want_sigma else null, xa.stream())
    optr = out.ptr if want_out else null
    if inputtype == "wpt":
        fn = getattr(_lib.lib(), "wx_denoise_wpt1d_trees" + xa.suffix)
        _lib.check(fn(xa.ptr, optr, n, tp, nt, N, qp, F, *tail))
    elif inputtype == "swpd":
        fn = getattr(_lib.lib(), "wx_denoise_swpd1d_trees" + xa.suffix)
        _lib.check(fn(xa.ptr, optr, n, xa.shape[1], tp, nt, N, qp, F, *tail))
    else:
        if xa.suffix != "_f64":
            raise _lib.WxError(_lib.WX_EUNSUPPORTED, "the autocorrelation transforms are Float64 only")
        _lib.check(_lib.lib().wx_denoise_acwpd1d_trees_f64(xa.ptr, optr, n, xa.shape[1], tp, nt, N, *tail))
    return out, sig


# a packet table in host memory keeps the refusal it always had: the table is (2^(D+1) - 1) times the signals, its upload would be the
# call; the C entries take either
_RED_HOST = "a tree matrix (one tree per signal) on a redundant packet table needs the table on the device (host arrays: inputtype = :wpt)"


def _denoise_trees(xa, inputtype, wt, trees, dnt, estnoise, bestTH, smooth, batched):
    """denoise / denoiseall(x, :wpt | :swpd | :acwpd, wt; tree = M) with M an (n - 1, N) matrix: signal i in the basis of column i
    (csrc/wx_denoise_trees.hip; from a redundant packet table, a device tensor, csrc/wx_denoise_red_trees.hip).  estnoise =
    relerrorthreshold | surethreshold on a redundant table: every signal's threshold over the leaf columns of its own tree
    (csrc/wx_shrink_trees.hip), for a device table; a table in host memory keeps its refusal"""
    if inputtype not in ("wpt", "swpd", "acwpd"):
        raise _lib.WxError(_lib.WX_EUNSUPPORTED, "a tree matrix (one tree per signal) needs inputtype = :wpt, :swpd or :acwpd")
    red = inputtype != "wpt"
    if xa.arr.ndim != (2 if batched else 1) + (1 if red else 0):
        raise _lib.WxError(_lib.WX_EUNSUPPORTED, "a tree matrix (one tree per signal) needs 1-D signals")
    N = xa.shape[-1] if batched else 1
    if estnoise is None or estnoise is noisest:
        thr = None
    elif estnoise is relerrorthreshold or estnoise is surethreshold:
        kind = 1 if estnoise is relerrorthreshold else 0
        if red:
            if xa.kind != "torch":
                raise _lib.WxError(_lib.WX_EUNSUPPORTED, "relerrorthreshold / surethreshold with a tree matrix on a redundant table in host memory: "
                                                         "the per-signal leaf masks are built for a device table only")
            # the leaf columns of every signal's own tree (Denoising.jl:150-157, 293-300), elbows = 2: estnoise(x, true, tree); the N values
            # stay on the device
            thr = _select_trees(xa if batched else Arg(xa.arr[..., None]), trees, kind)
        else:
            # all coefficients of a non-redundant signal, whatever its tree (Denoising.jl:150-157, 293-300)
            thr = _select(xa, batched, False, None, kind)
    elif callable(estnoise):
        raise _lib.WxError(_lib.WX_EUNSUPPORTED,
                           "noise estimates on the device path: noisest, relerrorthreshold, surethreshold or precomputed values")
    else:
        thr = np.broadcast_to(np.asarray(estnoise, dtype=np.float64), (N,)).astype(xa.dtype)
    if red and xa.kind != "torch":
        raise _lib.WxError(_lib.WX_EUNSUPPORTED, _RED_HOST)
    if bestTH is not None:                                             # one summary threshold for the batch, Denoising.jl:697-700
        if thr is None:
            thr = to_numpy(_trees_call(xa, N, None, trees, dnt.th.kind, dnt.t, None, smooth, False, True, inputtype)[1].arr)
        elif isinstance(thr, Arg):
            thr = to_numpy(thr.arr)
        thr = np.full(1, bestTH(np.asarray(thr, dtype=np.float64)), dtype=xa.dtype)
    return _trees_call(xa, N, wt, trees, dnt.th.kind, dnt.t, thr, smooth, True, False, inputtype)[0].arr


def _red_sig_call(xa, wt, trees, L, transform, th_kind, scale, thr, smooth, want_out, want_sigma):
    """wx_denoise_swpd1d_sig_trees_* / wx_denoise_acwpd1d_sig_trees_f64: (xhat | None, sigma | None) as Args of the signals' kind"""
    from ._arrays import qmf_arg, trees_arg
    if transform not in ("swpd", "acwpd"):
        raise ValueError("transform: \"swpd\" or \"acwpd\"")
    if xa.arr.ndim != 2:
        raise _lib.WxError(_lib.WX_EUNSUPPORTED, "a tree matrix (one tree per signal) needs 1-D signals, (n, N)")
    null = ctypes.c_void_p(0)
    n, N = xa.shape
    L = maxtransformlevels(n) if L is None else int(L)
    q, qp, F = qmf_arg(wt)
    tb, tp, nt = trees_arg(trees, N, xa)
    out = xa.new((n, N)) if want_out else None
    sig = xa.new((N,)) if want_sigma else None
    tv, tvp, tvn = _thr_arg(thr, xa.dtype)
    name = ("wx_denoise_swpd1d_sig_trees" if transform == "swpd" else "wx_denoise_acwpd1d_sig_trees") + xa.suffix
    fn = getattr(_lib.lib(), name, None)
    if fn is None:
        raise _lib.WxError(_lib.WX_EUNSUPPORTED, "the autocorrelation transforms are Float64 only")
    _lib.check(fn(xa.ptr, out.ptr if want_out else null, n, L, tp, nt, N, qp, F, int(th_kind), float(scale),
                  tvp, tvn, 1 if smooth == "undersmooth" else 0, sig.ptr if want_sigma else null, xa.stream()))
    return out, sig


# the packet table of one chunk of signals in _red_chunks: the budget of route 2 of the from-the-signals entries
_RED_SELECT_BUDGET = 256 << 20


def _red_chunks(xa, wt, trees, L, transform, budget=None):
    """device signals (n, N) by chunks through swpdall / acwpdall(x, wt, L): (b0, b1, the chunk's packet table as an Arg, the chunk's columns
    of `trees`), a table of at most `budget` bytes (one signal's table where that is larger)"""
    from .swt import swpdall
    from .acwt import acwpdall
    if transform not in ("swpd", "acwpd"):
        raise ValueError("transform: \"swpd\" or \"acwpd\"")
    if xa.arr.ndim != 2:
        raise _lib.WxError(_lib.WX_EUNSUPPORTED, "a tree matrix (one tree per signal) needs 1-D signals, (n, N)")
    n, N = xa.shape
    L = maxtransformlevels(n) if L is None else int(L)
    tr = trees if is_torch(trees) else np.asarray(trees)
    assert tr.ndim == 2 and N == tr.shape[1]                           # Utils.jl:210
    budget = _RED_SELECT_BUDGET if budget is None else int(budget)
    per = max(1, budget // (n * ((2 << L) - 1) * xa.dtype.itemsize))
    for b0 in range(0, N, per):
        b1 = min(N, b0 + per)
        yield b0, b1, Arg((swpdall if transform == "swpd" else acwpdall)(xa.arr[:, b0:b1], wt, L)), tr[:, b0:b1]


def _red_select(xa, wt, trees, L, transform, kind, budget=None):
    """surethreshold (kind 0) / relerrorthreshold (kind 1) of device signals (n, N), each over the leaves of its own tree in swpdall /
    acwpdall(x, wt, L), chunk by chunk through _select_trees; an Arg with the N thresholds on the device"""
    out = xa.new((xa.shape[-1],))
    for b0, b1, table, tr in _red_chunks(xa, wt, trees, L, transform, budget):
        out.arr[b0:b1] = _select_trees(table, tr, kind).arr
    return out


def _red_denoise_selected(xa, wt, trees, L, dnt, kind, bestTH, smooth, transform, budget=None):
    """swpd_denoiseall / acwpd_denoiseall with estnoise = surethreshold (kind 0) / relerrorthreshold (kind 1) on device signals: the
    selections rank whole leaf columns, so a chunk's packet table has to exist; once it does, the chunk is denoised from it
    (_trees_call, the entries of denoiseall on a table) instead of being transformed a second time by the from-the-signals entry.  The
    result is therefore the table way's, byte for byte.  bestTH wants every threshold before the first signal is denoised: then the
    chunks are transformed twice."""
    n, N = xa.shape[0], xa.shape[-1]
    one = None
    if bestTH is not None:                                             # one summary threshold for the batch, Denoising.jl:697-700
        thr = to_numpy(_red_select(xa, wt, trees, L, transform, kind, budget).arr)
        one = np.full(1, bestTH(np.asarray(thr, dtype=np.float64)), dtype=xa.dtype)
    out = xa.new((n, N))
    for b0, b1, table, tr in _red_chunks(xa, wt, trees, L, transform, budget):
        thr = one if one is not None else _select_trees(table, tr, kind)
        out.arr[:, b0:b1] = _trees_call(table, b1 - b0, wt, tr, dnt.th.kind, dnt.t, thr, smooth, True, False, transform)[0].arr
    return out.arr


def _red_denoiseall(x, wt, trees, L, dnt, estnoise, bestTH, smooth, transform, select_budget=None):
    xa = Arg(x)
    dnt = VisuShrink(xa.shape[0]) if dnt is None else dnt
    if estnoise is None or estnoise is noisest:
        thr = None
    elif estnoise is relerrorthreshold or estnoise is surethreshold:
        if xa.kind != "torch":
            raise _lib.WxError(_lib.WX_EUNSUPPORTED, "relerrorthreshold / surethreshold with a tree matrix on a redundant basis of signals in host "
                                                     "memory: the per-signal leaf masks are built for device signals only")
        return _red_denoise_selected(xa, wt, trees, L, dnt, 1 if estnoise is relerrorthreshold else 0, bestTH, smooth, transform, select_budget)
    elif callable(estnoise):
        raise _lib.WxError(_lib.WX_EUNSUPPORTED,
                           "noise estimates on the device path: noisest, relerrorthreshold, surethreshold or precomputed values")
    else:
        thr = np.broadcast_to(np.asarray(estnoise, dtype=np.float64), (xa.shape[-1],)).astype(xa.dtype)
    if bestTH is not None:                                             # one summary threshold for the batch, Denoising.jl:697-700
        if thr is None:
            thr = to_numpy(_red_sig_call(xa, wt, trees, L, transform, dnt.th.kind, dnt.t, None, smooth, False, True)[1].arr)
        thr = np.full(1, bestTH(np.asarray(thr, dtype=np.float64)), dtype=xa.dtype)
    return _red_sig_call(xa, wt, trees, L, transform, dnt.th.kind, dnt.t, thr, smooth, True, False)[0].arr


def swpd_denoiseall(x, wt, trees, L=None, dnt=None, estnoise=None, bestTH=None, smooth="regular"):
    """denoiseall(swpdall(x, wt, L), "swpd", wt, tree=trees, ...) straight from the signals x (n, N), host or device, with the tree of
    signal i in column i of `trees` ((n - 1, N), host or device: what swpd_bestbasistreeall returns): the (n, 2^(L+1)-1, N) packet table
    is never written (csrc/wx_denoise_red_sig.hip).  No tree may decompose a node of depth >= L (IndexError).  dnt, estnoise (None /
    noisest / numbers), bestTH and smooth as denoiseall with a tree matrix.  estnoise = relerrorthreshold | surethreshold, for device
    signals only: the selections rank whole leaf columns, so chunks of the signals go through packet tables of at most 256 MiB; each
    chunk's thresholds are selected over the leaves of every signal's own tree (csrc/wx_shrink_trees.hip), stay on the device, and the
    chunk is denoised from the table it already has: byte for byte denoiseall on the table.  Signals in host memory are refused."""
    return _red_denoiseall(x, wt, trees, L, dnt, estnoise, bestTH, smooth, "swpd")


def acwpd_denoiseall(x, wt, trees, L=None, dnt=None, estnoise=None, bestTH=None, smooth="regular"):
    """swpd_denoiseall for the autocorrelation packet decomposition acwpdall(x, wt, L); Float64 only, like the transform"""
    return _red_denoiseall(x, wt, trees, L, dnt, estnoise, bestTH, smooth, "acwpd")


def red_noisestall(x, wt, trees, L=None, transform="swpd"):
    """noisestall(swpdall | acwpdall(x, wt, L), True, trees) straight from the signals: every signal's estimate from the finest detail node
    of its own tree, a chain of at most L high-pass steps"""
    return _red_sig_call(Arg(x), wt, trees, L, transform, 0, 1.0, None, "regular", False, True)[1].arr


def bestbasis_denoiseall(x, wt, L=None, transform="swpd", method=None, **denoise_kw):
    """swpd_denoiseall(x, wt, swpd_bestbasistreeall(x, wt, L, method), L, ...) (or the acwpd pair): every signal denoised in its own
    translation-invariant best basis.  With device signals the trees stay on the device."""
    from .bestbasis import swpd_bestbasistreeall, acwpd_bestbasistreeall
    if transform not in ("swpd", "acwpd"):
        raise ValueError("transform: \"swpd\" or \"acwpd\"")
    extra = set(denoise_kw) - {"dnt", "estnoise", "bestTH", "smooth"}
    if extra:
        raise TypeError("bestbasis_denoiseall: unexpected keyword arguments %s" % sorted(extra))
    dev = is_torch(x) and x.device.type != "cpu"
    trees = (swpd_bestbasistreeall if transform == "swpd" else acwpd_bestbasistreeall)(x, wt, L, method, device=dev)
    return _red_denoiseall(x, wt, trees, L, denoise_kw.get("dnt"), denoise_kw.get("estnoise"), denoise_kw.get("bestTH"),
                           denoise_kw.get("smooth", "regular"), transform)


def noisestall(x, redundant=False, tree=None):
    """noisest (Denoising.jl:214-232) of every signal of a batch (last axis): `tree` is None, one tree for all, or an (n - 1, N) matrix with
    the tree of signal i in column i (then each estimate comes from the finest detail node of its own tree; redundant: x is the
    (n, ncols, N) packet table of swpdall / acwpdall, a device tensor)"""
    xa = Arg(x)
    if _is_tree_matrix(tree):
        if xa.arr.ndim != (3 if redundant else 2):
            raise _lib.WxError(_lib.WX_EUNSUPPORTED, "a tree matrix (one tree per signal) needs 1-D signals")
        if redundant and xa.kind != "torch":
            raise _lib.WxError(_lib.WX_EUNSUPPORTED, _RED_HOST)
        # a redundant table: the column of the finest detail node, whichever transform filled it (the :swpd entry needs no filter for this)
        return _trees_call(xa, xa.shape[-1], None, tree, 0, 1.0, None, "regular", False, True, "swpd" if redundant else "wpt")[1].arr
    it = ("sdwt" if tree is None else "swpd") if redundant else ("dwt" if tree is None else "wpt")
    sig = _noisest(xa, True, it, None if tree is None else np.asarray(tree, dtype=bool), on_device=xa.kind == "torch")
    return sig.arr if isinstance(sig, Arg) else sig


def _denoise(x, inputtype, wt, L, tree, dnt, estnoise, bestTH, smooth, batched):
    assert smooth in ("undersmooth", "regular")                       # Denoising.jl:493
    assert inputtype in INPUTTYPES                                     # Denoising.jl:494
    if not isinstance(dnt, (VisuShrink, SureShrink, RelErrorShrink)):
        raise _lib.WxError(_lib.WX_EARG, "dnt must be a VisuShrink, SureShrink or RelErrorShrink")
    xa = Arg(x)
    if _is_tree_matrix(tree):
        return _denoise_trees(xa, inputtype, wt, tree, dnt, estnoise, bestTH, smooth, batched)
    n = xa.shape[0]
    L = maxtransformlevels(n) if L is None else int(L)
    tree = maketree(n, L, "dwt") if tree is None else np.asarray(tree, dtype=bool)
    if inputtype == "sig":
        if wt is None:
            raise ValueError("inputtype=:sig not supported with wt=nothing")    # Denoising.jl:498
        if bestTH is None and (estnoise is None or estnoise is noisest) and xa.arr.ndim == (2 if batched else 1) and isdyadic(n):
            # the whole pipeline behind one entry point: one pass over the signals where the lattice kernel applies (csrc/wx_lattice_dn.h),
            # else dwtall -> noisest -> threshold on the loads of idwtall inside the library
            return _denoise_sig(xa, wt, L, dnt, smooth, batched)
        xa = Arg(dwtall(xa.arr, wt, L) if batched else dwt(xa.arr, wt, L))
        inputtype = "dwt"
    elif (inputtype == "dwt" and wt is not None and bestTH is None and (estnoise is None or estnoise is noisest) and
          xa.arr.ndim == (2 if batched else 1) and isdyadic(n)):
        return _denoise_sig(xa, wt, L, dnt, smooth, batched, "wx_denoiseall_dwt")      # coefficients in, signals out: one pass where it applies
    if inputtype not in ("dwt", "wpt"):
        assert xa.arr.ndim > (2 if batched else 1)                     # @assert ndims(x) > 1
    N = xa.shape[-1] if batched else 1
    # noise estimation
    tr = None if inputtype in ("dwt", "sdwt", "acdwt") else tree
    noise_it = inputtype
    if bestTH is not None and inputtype == "acdwt":
        # denoiseall's summary-threshold branch estimates the noise of :acdwt input as estnoise(x, true, tree)
        # (Denoising.jl:683-690: only :dwt, :wpt and :sdwt have a case of their own), i.e. on the finest detail NODE of the
        # tree read as a column of a heap-ordered table, not on the last column
        tr, noise_it = tree, "acwpd"
    if (xa.kind == "torch" and bestTH is None and wt is not None and inputtype in ("dwt", "wpt") and
            xa.arr.ndim == (2 if batched else 1) and
            (estnoise is None or estnoise is noisest) and (inputtype == "wpt" or L >= 1)):
        # device-resident pipeline: MAD -> threshold riding on the inverse's loads; sigma never visits the host
        sig = _noisest(xa, batched, inputtype, tr, on_device=True)
        if inputtype == "dwt":
            return _iwpt_thresh(xa, wt, maketree(n, L, "dwt"), batched, dnt.th, sig,
                                nodelength(n, L) if smooth == "undersmooth" else 0, dnt.t)
        return _iwpt_thresh(xa, wt, tree, batched, dnt.th, sig,
                            coarsestscalingrange(n, tree)[-1] if smooth == "undersmooth" else 0, dnt.t)
    if estnoise is None or callable(estnoise):
        red = inputtype in ("sdwt", "swpd", "acdwt", "acwpd")
        if estnoise is None or estnoise is noisest:
            sigma = _noisest(xa, batched, noise_it, tr)
        elif estnoise is relerrorthreshold:                            # estnoise(x, redundant, tree), Denoising.jl:503-571
            sigma = _select(xa, batched, red, tr, 1)
        elif estnoise is surethreshold:
            sigma = _select(xa, batched, red, tr, 0)
        else:
            raise _lib.WxError(_lib.WX_EUNSUPPORTED,
                               "noise estimates on the device path: noisest, relerrorthreshold, surethreshold or precomputed values")
    else:
        sigma = np.broadcast_to(np.asarray(estnoise, dtype=np.float64), (N,)).astype(xa.dtype)
    if bestTH is not None:
        sigma = np.full(N, bestTH(sigma.astype(np.float64)), dtype=xa.dtype)     # Denoising.jl:697-700
    t = (sigma.astype(np.float64) * dnt.t).astype(xa.dtype)            # σ*dnt.t
    # thresholding + reconstruction
    if inputtype == "dwt":
        lo = nodelength(n, L) if smooth == "undersmooth" else 0
        if wt is not None and xa.arr.ndim == (2 if batched else 1) and L >= 1:      # threshold rides on the inverse's loads
            return _iwpt_thresh(xa, wt, maketree(n, L, "dwt"), batched, dnt.th, t, lo)
        xt = xa.new(xa.shape)          # thresholded copy (the reference leaves x alone)
        _threshold(xa, xt, batched, dnt.th, t, lo)
        if wt is None:
            return xt.arr
        return idwtall(xt.arr, wt, L) if batched else idwt(xt.arr, wt, L)
    if inputtype == "wpt":
        lo = coarsestscalingrange(n, tree)[-1] if smooth == "undersmooth" else 0
        if wt is not None and xa.arr.ndim == (2 if batched else 1):
            return _iwpt_thresh(xa, wt, tree, batched, dnt.th, t, lo)
        xt = xa.new(xa.shape)          # thresholded copy (the reference leaves x alone)
        _threshold(xa, xt, batched, dnt.th, t, lo)
        if wt is None:
            return xt.arr
        return iwptall(xt.arr, wt, tree) if batched else iwpt(xt.arr, wt, tree)
    xt = xa.new(xa.shape)
    k = xt.shape[1]
    if inputtype in ("sdwt", "acdwt"):
        mask = np.ones(k, dtype=np.uint8)
        if smooth == "undersmooth":
            mask[0] = 0
        _threshold(xa, xt, batched, dnt.th, t, 0, mask)
        if inputtype == "sdwt":
            if wt is None:
                return xt.arr
            return isdwtall(xt.arr, wt) if batched else isdwt(xt.arr, wt)
        return iacdwtall(xt.arr) if batched else iacdwt(xt.arr)
    leaves = np.asarray(getleaf(tree, "binary"), dtype=bool)
    assert not leaves[k:].any(), "tree has leaves below the last column of the table"
    mask = leaves[:k].astype(np.uint8)
    if smooth == "undersmooth":
        mask[coarsestscalingrange(n, tree, True)[1] - 1] = 0
    _threshold(xa, xt, batched, dnt.th, t, 0, mask)
    if inputtype == "swpd":
        if wt is None:
            return xt.arr
        return iswpdall(xt.arr, wt, tree) if batched else iswpd(xt.arr, wt, tree)
    return iacwpdall(xt.arr, tree) if batched else iacwpd(xt.arr, tree)


def denoise(x, inputtype, wt, L=None, tree=None, dnt=None, estnoise=None, smooth="regular"):
    """denoise(x, inputtype, wt; L, tree, dnt, estnoise, smooth) Denoising.jl:483-599 (one signal)"""
    xa = Arg(x)
    dnt = VisuShrink(xa.shape[0]) if dnt is None else dnt
    return _denoise(xa.arr, inputtype, wt, L, tree, dnt, estnoise, None, smooth, False)


def denoiseall(x, inputtype, wt, L=None, tree=None, dnt=None, estnoise=None, bestTH=None, smooth="regular"):
    """denoiseall(x, inputtype, wt; L, tree, dnt, estnoise, bestTH, smooth) Denoising.jl:651-712: the whole batch
    in one pipeline (transform, per-signal MAD, threshold, inverse) on the device"""
    xa = Arg(x)
    assert xa.arr.ndim > 1                                             # Denoising.jl:663
    dnt = VisuShrink(xa.shape[0]) if dnt is None else dnt
    return _denoise(xa.arr, inputtype, wt, L, tree, dnt, estnoise, bestTH, smooth, True)
