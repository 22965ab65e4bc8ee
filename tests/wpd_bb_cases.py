"""Seeded fixtures of the fused per-signal best basis (wpd_bestbasistreeall): signals, filters, the oracle's reference and the
checks on a returned tree matrix, shared by tests/test_wpd_bb_cpu.py (which guards the fixtures) and tests/test_gpu_wpd_bb.py.
Plain module: no pytest fixtures, no GPU.

Signals of length n: rng = default_rng(4100 + n), standard normal (n, COLS[n]), every third column replaced by its cumulative sum
so that the trees are non-trivial.  A case with fewer signals takes the leading columns, the batch-striding case repeats the
columns (the reference is computed once for the distinct ones).

Reference: the oracle on ITS OWN table, never the library's wpdall:
    T_o = oracle.bestbasistreeall_bb(oracle.wpdall(x, qmf, L), False, cost),  c_o = oracle.tree_costs_bb(...) per signal."""
import functools

import numpy as np

import qmf_family

COLS = {8: 200, 64: 200, 256: 33, 1024: 16, 4096: 6, 8192: 3}
GRID_SHORT = 256 * 16         # workgroups of a launch of 64-sample signals (wx_trees_grid: 16 per CU on 256 CUs); tests/test_wpd_bb_cpu.py asserts it against the launch code

# (n, filter, L (None = full depth), cost): every Float64 case of the GPU tests -- the margin guard of the CPU tests walks this list
F64_CASES = [
    (8, "db4", 3, "shannon"), (8, "db8", 3, "shannon"),
    (64, "db4", None, "shannon"), (64, "haar", None, "shannon"), (64, "db8", None, "shannon"), (64, "rand22", None, "shannon"),
    (256, "db4", 0, "shannon"), (256, "db4", 1, "shannon"), (256, "db4", 5, "shannon"), (256, "db4", 8, "shannon"),
    (256, "db4", 8, "logenergy"),
    (1024, "haar", None, "shannon"), (1024, "db4", None, "shannon"), (1024, "db8", None, "shannon"),
    (4096, "db4", 12, "shannon"),
    (8192, "db4", 13, "shannon"),
]

CTOL = {np.dtype(np.float64): 1e-10, np.dtype(np.float32): 1e-4}      # the cost tolerances of tests/test_gpu_bestbasis.py
MARGIN_MIN = 1e-8             # closest split decision of every Float64 fixture: what makes exact tree equality a fair demand
F32_MAX_DIFFERENT = 0.10      # Float32: share of a case's signals whose tree may differ from the oracle's at all


@functools.lru_cache(maxsize=None)
def signals(n):
    rng = np.random.default_rng(4100 + n)
    x = rng.standard_normal((n, COLS[n]))
    x[:, ::3] = np.cumsum(x[:, ::3], axis=0)
    x = np.asfortranarray(x)
    x.setflags(write=False)
    return x


def qmf(wx, name):
    if name == "rand22":                                # 22 taps: outside every LDS kernel's filter window
        return qmf_family.qmf_from_angles(qmf_family.angles_rand(22))
    return np.asarray(wx.wavelet(getattr(wx.WT, name)).qmf, dtype=np.float64)


def wavelet(wx, name):
    from waveletsext_jl_amd.filters import OrthoFilter
    return OrthoFilter(qmf(wx, name), name)


def cost_of(wx, cost):
    return wx.ShannonEntropyCost() if cost == "shannon" else wx.LogEnergyEntropyCost()


def full_depth(n):
    return int(np.log2(n))


_REF = {}


def reference(wx, oracle, n, filt, L, cost, dtype, x=None, key=None):
    """(T_o (n-1, B) bool, c_o (2^(L+1)-1, B)) of signals(n) as `dtype` (or of `x`, cached under `key`): computed once, shared, read-only"""
    L = full_depth(n) if L is None else L
    k = (n, filt, L, cost, np.dtype(dtype).str, key)
    if k not in _REF:
        xs = signals(n).astype(dtype) if x is None else x
        tab = oracle.wpdall(np.asfortranarray(xs), qmf(wx, filt), L)
        with np.errstate(all="ignore"):
            T = oracle.bestbasistreeall_bb(tab, False, cost)
            c = np.stack([oracle.tree_costs_bb(np.asfortranarray(tab[:, :, i]), False, cost) for i in range(tab.shape[-1])], axis=1)
        T.setflags(write=False)
        c.setflags(write=False)
        _REF[k] = (T, c)
    return _REF[k]


def leaf_cost(tree, c):
    """sum of c over the leaves of `tree` (heap order: node i is tree[i - 1], children 2i and 2i + 1), in Float64"""
    ncost = c.size
    dec = np.zeros(ncost + 1, dtype=bool)               # 1-based, decomposed
    m = min(tree.size, ncost)
    dec[1:m + 1] = tree[:m]
    reached = np.zeros(ncost + 1, dtype=bool)
    reached[1] = True
    for i in range(2, ncost + 1):
        reached[i] = reached[i >> 1] and dec[i >> 1]
    leaves = reached & ~dec
    return float(np.asarray(c, dtype=np.float64)[leaves[1:]].sum())


def check_trees(wx, trees, T_o, c_o, dtype, n):
    """the issue's contract on a returned tree matrix: Float64 equality; Float32 validity, leaf cost within 1e-4 relative of the
    oracle tree's, at most 10 % of the signals different"""
    trees = np.asarray(trees)
    assert trees.shape == T_o.shape and trees.dtype == np.bool_
    if np.dtype(dtype) == np.float64:
        bad = np.flatnonzero((trees != T_o).any(axis=0))
        assert bad.size == 0, "signals whose tree differs from the oracle's: %s" % bad[:10]
        return
    B = trees.shape[1]
    differ = 0
    probe = np.zeros(n)
    for i in range(B):
        if (trees[:, i] == T_o[:, i]).all():
            continue
        differ += 1
        assert wx.isvalidtree(probe, trees[:, i]), i
        got, exp = leaf_cost(trees[:, i], c_o[:, i]), leaf_cost(T_o[:, i], c_o[:, i])
        print("signal %d: leaf cost %.9g against the oracle tree's %.9g" % (i, got, exp))
        assert got - exp <= CTOL[np.dtype(np.float32)] * abs(exp), (i, got, exp)
    print("%d of %d Float32 trees differ from the oracle's" % (differ, B))
    assert differ <= F32_MAX_DIFFERENT * B, (differ, B)
