"""Best basis: host-side mirror of the reference's `BestBasis` module for the three best-basis types, JBB
(src/mod/BestBasis.jl:59-83,128-140,194-201; bestbasis/bestbasis_tree.jl:43-46,150-180; bestbasis/bestbasis_costs.jl:44-57,
127-132), BB (bestbasis_tree.jl:60-63, 210-258) and LSDB (bestbasis_tree.jl:24-27, 104-147; bestbasis_costs.jl:66, 135-164).
Moments, entropies and costs run on the GPU; the bottom-up tree selection is the library's tiny host routine."""
import ctypes

import numpy as np

from . import _lib
from ._lib import wpd_bb_route, red_bb_route  # noqa: F401
from ._arrays import Arg, is_torch, qmf_arg, to_numpy
from .dwt import _call
from .filters import ArgumentError
from .util import gettreelength, maxtransformlevels


class LoglpCost:
    """bestbasis_costs.jl:44-46"""

    def __init__(self, p=2):
        self.p = p


class NormCost:
    """bestbasis_costs.jl:55-57"""

    def __init__(self, p=1):
        self.p = p


class ShannonEntropyCost:
    """bestbasis_costs.jl:76"""


class LogEnergyEntropyCost:
    """bestbasis_costs.jl:86"""


class DifferentialEntropyCost:
    """bestbasis_costs.jl:66, the LSDB cost (coefcost :135-164)"""


class LSDB:
    """Least statistically dependent basis, bestbasis_tree.jl:24-27"""

    def __init__(self, cost=None, redundant=False):
        self.cost = DifferentialEntropyCost() if cost is None else cost
        if not isinstance(self.cost, DifferentialEntropyCost):
            raise TypeError("LSDB cost must be DifferentialEntropyCost")
        self.redundant = bool(redundant)


class BB:
    """Standard (per-signal) best basis, bestbasis_tree.jl:60-63"""

    def __init__(self, cost=None, redundant=False):
        self.cost = ShannonEntropyCost() if cost is None else cost
        if not isinstance(self.cost, (ShannonEntropyCost, LogEnergyEntropyCost)):
            raise TypeError("BB cost must be ShannonEntropyCost or LogEnergyEntropyCost")
        self.redundant = bool(redundant)


class JBB:
    """bestbasis_tree.jl:43-46"""

    def __init__(self, cost=None, redundant=False):
        self.cost = LoglpCost(2) if cost is None else cost
        if not isinstance(self.cost, (LoglpCost, NormCost)):
            raise TypeError("JBB cost must be LoglpCost or NormCost")
        self.redundant = bool(redundant)


def _cost_kind(cost):
    return (0, float(cost.p)) if isinstance(cost, LoglpCost) else (1, float(cost.p))


def jbb_moments(X, accumulate_into=None):
    """(sum, sumsq) over the signal (last) axis of a decomposition X (n, k, N) or (n, m, k, N)."""
    X = Arg(X)
    assert 3 <= X.arr.ndim <= 4
    shp, N = X.shape[:-1], X.shape[-1]
    if accumulate_into is None:
        s, q = X.new(shp), X.new(shp)
        acc = 0
    else:
        s, q = Arg(accumulate_into[0]), Arg(accumulate_into[1])
        acc = 1
    _call("wx_jbb_moments", X.suffix, X.ptr, s.ptr, q.ptr, int(np.prod(shp, dtype=np.int64)), N, acc, X.stream())
    return s.arr, q.arr


def costs_from_moments(s, q, Ntot, method=None):
    method = JBB() if method is None else method
    s, q = Arg(s), Arg(q)
    kind, p = _cost_kind(method.cost)
    if s.arr.ndim == 3:                                               # 2-D signals: (n, m, k)
        n, m, k = s.shape
        ncost = k if method.redundant else gettreelength(1 << k, 1 << k)
        costs = s.new((ncost,))
        _call("wx_jbb_costs2d", s.suffix, s.ptr, q.ptr, int(Ntot), n, m, k, int(method.redundant), kind, p, costs.ptr,
              s.stream())
        return costs.arr
    n, k = s.shape
    ncost = k if method.redundant else gettreelength(1 << k)
    costs = s.new((ncost,))
    _call("wx_jbb_costs", s.suffix, s.ptr, q.ptr, int(Ntot), n, k, int(method.redundant), kind, p, costs.ptr,
          s.stream())
    return costs.arr


def lsdb_entropy(X):
    """coefcost(X[e, :], DifferentialEntropyCost()) (bestbasis_costs.jl:135-155) of every row e of X seen as (nk, N), the
    signal axis last: Float64 array of shape X.shape[:-1], same kind as X."""
    Xa = Arg(X)
    shp, N = Xa.shape[:-1], Xa.shape[-1]
    E = Xa.new(shp, dtype=np.float64)
    _call("wx_lsdb_entropy", Xa.suffix, Xa.ptr, int(np.prod(shp, dtype=np.int64)), N, E.ptr, Xa.stream())
    return E.arr


def _lsdb_costs(Xa, method):
    """tree_costs(X, LSDB(...)) bestbasis_tree.jl:104-147: X (n, k, N) or (n, m, k, N) -> costs, same kind and type as X"""
    red = int(method.redundant)
    if Xa.arr.ndim == 4:
        n, m, k, N = Xa.shape
        ncost = k if red else gettreelength(1 << k, 1 << k)
        costs = Xa.new((ncost,))
        _call("wx_lsdb_costs2d", Xa.suffix, Xa.ptr, n, m, k, N, red, costs.ptr, Xa.stream())
    else:
        n, k, N = Xa.shape
        ncost = k if red else gettreelength(1 << k)
        costs = Xa.new((ncost,))
        _call("wx_lsdb_costs", Xa.suffix, Xa.ptr, n, k, N, red, costs.ptr, Xa.stream())
    return costs.arr


def _bb_costs(Xa, method, batched):
    """(ncost[, N]) costs of one signal (n, k) / (n, m, k) or of a batch (..., N) for BB"""
    nd = Xa.arr.ndim - (1 if batched else 0)
    assert 2 <= nd <= 3
    N = Xa.shape[-1] if batched else 1
    kind = 0 if isinstance(method.cost, ShannonEntropyCost) else 1
    if nd == 2:
        n, k = Xa.shape[:2]
        ncost = k if method.redundant else (1 << k) - 1
        costs = Xa.new((ncost, N) if batched else (ncost,))
        _call("wx_bb_costs", Xa.suffix, Xa.ptr, costs.ptr, n, k, N, int(method.redundant), kind, Xa.stream())
    else:
        n, m, k = Xa.shape[:3]
        ncost = k if method.redundant else gettreelength(1 << k, 1 << k)
        costs = Xa.new((ncost, N) if batched else (ncost,))
        _call("wx_bb_costs2d", Xa.suffix, Xa.ptr, costs.ptr, n, m, k, N, int(method.redundant), kind, Xa.stream())
    return costs


def _bb_trees(costs, sig, N, kind="min"):
    """bestbasis_treeselection for every column of costs (ncost, N) on the device -> uint8 (ntree, N)"""
    ncost = costs.shape[0]
    ntree = sig[0] - 1 if len(sig) == 1 else gettreelength(*sig)
    if costs.kind == "torch":
        import torch
        trees = torch.empty((N, ntree), dtype=torch.uint8, device=costs.device)
        tp, st = ctypes.c_void_p(trees.data_ptr()), costs.stream()
    else:
        trees = np.empty((N, ntree), dtype=np.uint8)
        tp, st = ctypes.c_void_p(trees.ctypes.data), ctypes.c_void_p(0)
    fn = getattr(_lib.lib(), "wx_treeselect_batch" + costs.suffix)
    _lib.check(fn(costs.ptr, ncost, sig[0], sig[1] if len(sig) == 2 else 0, 0 if kind == "min" else 1, N, tp, st))
    return trees


def bestbasistreeall(X, method=None, device=False):
    """bestbasistreeall(X, BB(...)) BestBasis.jl:253-262: X (n, k, N) or (n, m, k, N) -> BitMatrix (tree length, N);
    costs and the selection of all N trees run on the device.  device=True (X a device tensor): the selection's output itself, a
    column-major (tree length, N) torch.bool view on X's device -- no copy, no synchronisation; wptall / iwptall / iwpdall /
    getbasiscoefall take it as it is."""
    method = BB() if method is None else method
    if not isinstance(method, BB):
        raise TypeError("bestbasistreeall takes a BB method (BestBasis.jl:253)")
    if device and not (is_torch(X) and X.device.type != "cpu"):
        raise TypeError("bestbasistreeall(..., device=True) takes a device tensor")
    Xa = Arg(X)
    assert 3 <= Xa.arr.ndim <= 4                                      # BestBasis.jl:254
    sig = Xa.shape[:-2]
    costs = _bb_costs(Xa, method, True)
    trees = _bb_trees(costs, sig, Xa.shape[-1])
    if device:
        import torch
        return trees.T.view(torch.bool)                # (tree length, N) column-major; the selection writes bytes of 0 / 1
    if costs.kind == "torch":
        # device -> page-locked host memory (torch's caching host allocator) -> numpy view of it: .cpu() into pageable memory and a uint8 -> bool
        # copy were most of the call for short signals (19 MB of trees per GiB of table at 64 samples)
        import torch
        host = torch.empty(trees.shape, dtype=torch.uint8, pin_memory=True)
        host.copy_(trees, non_blocking=True)
        torch.cuda.current_stream(trees.device).synchronize()
        t = host.numpy()
    else:
        t = trees
    return t.T.view(np.bool_)                          # (tree length, N), column-major like the reference's BitMatrix; the bytes are 0 / 1


def tree_costs(X, method=None):
    """tree_costs(X::Array{T,3}, method::JBB) bestbasis_tree.jl:150-180; tree_costs(X, ::BB) :210-258 (one signal);
    tree_costs(X, ::LSDB) :104-147"""
    method = JBB() if method is None else method
    if isinstance(method, BB):
        Xa = Arg(X)
        assert 2 <= Xa.arr.ndim <= 3
        return _bb_costs(Xa, method, False).arr
    if isinstance(method, LSDB):
        Xa = Arg(X)
        assert 3 <= Xa.arr.ndim <= 4
        return _lsdb_costs(Xa, method)
    if not isinstance(method, JBB):
        raise _lib.WxError(_lib.WX_EUNSUPPORTED, "only the JBB best-basis type is on the device path")
    Xa = Arg(X)
    assert 3 <= Xa.arr.ndim <= 4
    s, q = jbb_moments(Xa.arr)
    costs = costs_from_moments(s, q, Xa.shape[-1], method)
    c = to_numpy(costs)
    assert not np.isnan(c).any()                                      # @assert all(sigma .>= 0) (:158)
    return costs


def bestbasis_treeselection(costs, n, *args, return_gap=False):
    """bestbasis_treeselection(costs, n[, type]) BestBasis.jl:59-83 and (costs, n, m[, type]) :85-110; `costs`
    (host copy) is mutated like the reference, returns the BitVector.  return_gap=True (1-D) also returns the margin of the
    closest split decision, min |cc - pc| / |pc| over the decisions taken (`wx_treeselect_gap_*`)."""
    args = list(args)
    kind = args.pop() if args and isinstance(args[-1], str) else "min"
    if kind not in ("min", "max"):
        raise ArgumentError("Unsupported type %s." % kind)
    c = np.array(to_numpy(costs), copy=True)
    if c.dtype not in (np.float32, np.float64):
        c = c.astype(np.float64)
    k = c.size
    if args:                                                          # quad tree
        m = int(args[0])
        assert k <= gettreelength(2 * n, 2 * m)                       # BestBasis.jl:90
        tree = np.zeros(gettreelength(n, m), dtype=np.uint8)
        fn = getattr(_lib.lib(), "wx_treeselect2d_f64" if c.dtype == np.float64 else "wx_treeselect2d_f32")
        _lib.check(fn(ctypes.c_void_p(c.ctypes.data), k, n, m, 0 if kind == "min" else 1,
                      ctypes.c_void_p(tree.ctypes.data)))
        return tree.astype(bool)
    assert k <= gettreelength(2 * n)                                  # BestBasis.jl:63
    tree = np.zeros(max(n - 1, 0), dtype=np.uint8)
    if return_gap:
        gap = ctypes.c_double(0.0)
        fn = getattr(_lib.lib(), "wx_treeselect_gap_f64" if c.dtype == np.float64 else "wx_treeselect_gap_f32")
        _lib.check(fn(ctypes.c_void_p(c.ctypes.data), k, n, 0 if kind == "min" else 1, ctypes.c_void_p(tree.ctypes.data),
                      ctypes.byref(gap)))
        return tree.astype(bool), float(gap.value)
    fn = getattr(_lib.lib(), "wx_treeselect_f64" if c.dtype == np.float64 else "wx_treeselect_f32")
    _lib.check(fn(ctypes.c_void_p(c.ctypes.data), k, n, 0 if kind == "min" else 1, ctypes.c_void_p(tree.ctypes.data)))
    return tree.astype(bool)


def bestbasistree(X, method=None):
    """bestbasistree(X, JBB(...)) BestBasis.jl:194-201 and bestbasistree(X, LSDB(...)) :185-192 (X is (n, k, N) or
    (n, m, k, N)); bestbasistree(X, BB(...)) :203-210 (one signal, X is (n, k) or (n, m, k))"""
    method = JBB() if method is None else method
    Xa = Arg(X)
    if isinstance(method, BB):
        assert 2 <= Xa.arr.ndim <= 3                                  # BestBasis.jl:205
        costs = _bb_costs(Xa, method, False)
        trees = _bb_trees(costs, Xa.shape[:-1], 1)
        t = trees.cpu().numpy() if costs.kind == "torch" else trees
        return t[0].astype(bool)
    assert 3 <= Xa.arr.ndim <= 4
    costs = tree_costs(Xa.arr, method)
    return bestbasis_treeselection(costs, *Xa.shape[:-2])


def acwpd_jbb_moments(x, wt, L=None, accumulate_into=None):
    """acwpdall + JBB moments fused on the device (the (n, 2^(L+1)-1, N) table is never returned):
    BASELINE config 5.  Returns (sum, sumsq), each (n, 2^(L+1)-1)."""
    x = Arg(x)
    assert x.arr.ndim == 2
    n, N = x.shape
    L = maxtransformlevels(n) if L is None else int(L)
    ncols = (1 << (L + 1)) - 1
    if accumulate_into is None:
        s, q = x.new((n, ncols)), x.new((n, ncols))
        acc = 0
    else:
        s, q = Arg(accumulate_into[0]), Arg(accumulate_into[1])
        acc = 1
        for a in (s, q):
            if a.shape != (n, ncols) or a.kind != x.kind:
                raise TypeError("accumulate_into must be two (n, 2^(L+1)-1) arrays of the same kind as x")
    # ACWT is Float64-only like the reference (acwt_one_level.jl:101-106): the suffix of every array selects the entry
    # point, so Float32 data raises WX_EUNSUPPORTED instead of being reinterpreted
    for a in (s, q):
        if a.suffix != x.suffix:
            raise TypeError("accumulate_into element type differs from x's")
    qq, qp, F = qmf_arg(wt)
    _call("wx_acwpd_jbb_moments", x.suffix, x.ptr, s.ptr, q.ptr, n, L, N, qp, F, acc, x.stream())
    return s.arr, q.arr


def _bbtrees_from_signals(entry, name, x, wt, L, method, device, return_costs):
    """wx_wpd_bbtrees_* / wx_swpd_bbtrees_* / wx_acwpd_bbtrees_f64 on the signals x (n, N): the trees as bestbasistreeall returns them
    (host matrix, or the device view with device=True), and the costs on request"""
    if device and not (is_torch(x) and x.device.type != "cpu"):
        raise TypeError("%s(..., device=True) takes a device tensor" % name)
    xa = Arg(x)
    assert xa.arr.ndim == 2
    n, N = xa.shape
    L = maxtransformlevels(n) if L is None else int(L)
    kind = 0 if isinstance(method.cost, ShannonEntropyCost) else 1
    ntree, ncost = max(n - 1, 0), (1 << (max(L, 0) + 1)) - 1
    costs = xa.new((ncost, N)) if return_costs else None
    if xa.kind == "torch":
        import torch
        trees = torch.empty((N, ntree), dtype=torch.uint8, device=xa.device)
        tp = ctypes.c_void_p(trees.data_ptr())
    else:
        trees = np.empty((N, ntree), dtype=np.uint8)
        tp = ctypes.c_void_p(trees.ctypes.data)
    q, qp, F = qmf_arg(wt)
    _call(entry, xa.suffix, xa.ptr, n, L, N, qp, F, kind, tp, costs.ptr if return_costs else ctypes.c_void_p(0), xa.stream())
    if device:
        t = trees.T.view(torch.bool)                   # (n-1, N) column-major; the kernel writes bytes of 0 / 1
    elif xa.kind == "torch":
        host = torch.empty(trees.shape, dtype=torch.uint8, pin_memory=True)
        host.copy_(trees, non_blocking=True)
        torch.cuda.current_stream(trees.device).synchronize()
        t = host.numpy().T.view(np.bool_)
    else:
        t = trees.T.view(np.bool_)
    return (t, costs.arr) if return_costs else t


def wpd_bestbasistreeall(x, wt, L=None, method=None, device=False, return_costs=False):
    """bestbasistreeall(wpdall(x, wt, L), BB(cost)) (BestBasis.jl:253-262, bestbasis_tree.jl:210-233) straight from the signals
    x (n, N): the (n, L+1, N) packet table is never written.  Returns what bestbasistreeall returns, a column-major boolean
    (n-1, N) matrix, or with device=True (x a device tensor) the torch.bool view that wptall / iwptall / denoiseall take as it
    is; return_costs=True adds the (2^(L+1)-1, N) costs, as tree_costs gives them for every signal."""
    method = BB() if method is None else method
    if not isinstance(method, BB):
        raise TypeError("wpd_bestbasistreeall takes a BB method (BestBasis.jl:253)")
    if method.redundant:
        raise TypeError("wpd_bestbasistreeall is the decimated transform: BB(redundant=True) goes with swpd_bestbasistreeall / acwpd_bestbasistreeall")
    return _bbtrees_from_signals("wx_wpd_bbtrees", "wpd_bestbasistreeall", x, wt, L, method, device, return_costs)


def _red_bestbasistreeall(entry, name, x, wt, L, method, device, return_costs):
    method = BB(redundant=True) if method is None else method
    if not isinstance(method, BB):
        raise TypeError("%s takes a BB method (BestBasis.jl:253)" % name)
    if not method.redundant:
        raise TypeError("%s: the table of a redundant transform takes BB(redundant=True) (bestbasis_tree.jl:215)" % name)
    return _bbtrees_from_signals(entry, name, x, wt, L, method, device, return_costs)


def swpd_bestbasistreeall(x, wt, L=None, method=None, device=False, return_costs=False):
    """bestbasistreeall(swpdall(x, wt, L), BB(cost, redundant=True)) (BestBasis.jl:253-262, bestbasis_tree.jl:210-233) straight from
    the signals x (n, N), host or device: the (n, 2^(L+1)-1, N) packet table is never written.  Returns what bestbasistreeall
    returns, a column-major boolean (n-1, N) matrix, or with device=True (x a device tensor) the torch.bool view that iswpdall and
    denoiseall(xw, "swpd", wt, tree=M) take as it is; return_costs=True adds the (2^(L+1)-1, N) costs, as tree_costs gives them
    for every signal.  method defaults to BB(redundant=True); red_bb_route() tells which way the call went."""
    return _red_bestbasistreeall("wx_swpd_bbtrees", "swpd_bestbasistreeall", x, wt, L, method, device, return_costs)


def acwpd_bestbasistreeall(x, wt, L=None, method=None, device=False, return_costs=False):
    """swpd_bestbasistreeall for the autocorrelation packet table acwpdall(x, wt, L); Float64 only, like the transform"""
    return _red_bestbasistreeall("wx_acwpd_bbtrees", "acwpd_bestbasistreeall", x, wt, L, method, device, return_costs)


def bestbasiscoefall(x, wt, L=None, method=None, device=False):
    """(wptall(x, wt, trees), trees) with trees = wpd_bestbasistreeall(x, wt, L, method, device): every signal's coefficients in its own
    best basis and the bases, without the packet table on either side"""
    from .dwt import wptall
    trees = wpd_bestbasistreeall(x, wt, L, method, device=device)
    return wptall(x, wt, trees), trees
