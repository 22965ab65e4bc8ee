"""Seeded fixtures of the redundant per-signal best basis straight from the signals (swpd_bestbasistreeall, acwpd_bestbasistreeall):
signals, filters and the oracle's reference, shared by tests/test_red_bb_cpu.py (which guards the fixtures) and
tests/test_gpu_red_bb.py.  Plain module: no pytest fixtures, no GPU.  The checks on a returned tree matrix, the cost tolerances and
the filters are those of tests/wpd_bb_cases.py.

Signals (n, B), seed = 7000 + n + L: three blocks of n / 16 samples at +-(20 .. 40) per signal under unit normal noise, so that the
trees are non-trivial and a noise estimate has something to separate.

Reference: the oracle on ITS OWN table, never the library's swpdall / acwpdall, per signal:
    tab = oracle.swpd | oracle.acwpd (x[:, i], qmf, L);  c_o = oracle.tree_costs_bb(tab, True, cost);  T_o = oracle.bestbasistree_bb(tab, True, cost)"""
import functools

import numpy as np

from wpd_bb_cases import CTOL, MARGIN_MIN, check_trees, cost_of, leaf_cost, qmf, wavelet  # noqa: F401

# (n, L, B)
SHAPES = [(8, 3, 24), (64, 6, 24), (256, 8, 12), (1024, 8, 4)]
SHAPE_F32 = (1024, 10, 4)                     # Float32 only: the deepest tree of the Float32 window at n = 1024


def _filters(n):
    return ["haar", "db4"] + (["db8"] if n == 256 else [])


# (n, L, B, filter, cost): every Float64 case of the GPU tests -- the guards of the CPU tests walk this list for both transforms
F64_CASES = [(n, L, B, f, "shannon") for n, L, B in SHAPES for f in _filters(n)] + [(256, 8, 12, "db4", "logenergy")]
F32_CASES = F64_CASES + [SHAPE_F32 + (f, "shannon") for f in _filters(1024)]
GRID_8 = 256 * 16             # workgroups of a launch of 8-sample signals (wx_trees_grid: 16 per CU on 256 CUs); tests/test_red_bb_cpu.py asserts it against the launch code


@functools.lru_cache(maxsize=None)
def signals(n, L, B):
    rng = np.random.default_rng(7000 + n + L)
    w = max(1, n // 16)
    x = np.zeros((n, B))
    for i in range(B):
        for s in rng.choice(n // w, size=3, replace=False):
            x[s * w:(s + 1) * w, i] = rng.choice([-1.0, 1.0]) * rng.uniform(20.0, 40.0)
    x += rng.standard_normal((n, B))
    x = np.asfortranarray(x)
    x.setflags(write=False)
    return x


def table(oracle, transform, xcol, q, L):
    return (oracle.swpd if transform == "swpd" else oracle.acwpd)(np.ascontiguousarray(xcol), q, L)


_REF = {}


def reference(wx, oracle, transform, n, L, B, filt, cost, dtype, x=None, key=None):
    """(T_o (n-1, B) bool, c_o (2^(L+1)-1, B)) of signals(n, L, B) as `dtype` (or of `x`, cached under `key`): computed once, shared,
    read-only"""
    k = (transform, n, L, B, filt, cost, np.dtype(dtype).str, key)
    if k not in _REF:
        xs = signals(n, L, B).astype(dtype) if x is None else x
        q = qmf(wx, filt)
        T, c = [], []
        with np.errstate(all="ignore"):
            for i in range(xs.shape[1]):
                if L == 0:
                    tab = np.asfortranarray(xs[:, i:i + 1])           # the one-column table
                else:
                    tab = table(oracle, transform, xs[:, i], q, L)
                c.append(oracle.tree_costs_bb(tab, True, cost))
                t = np.zeros(n - 1, dtype=bool)
                tt = np.asarray(oracle.bestbasistree_bb(tab, True, cost), dtype=bool)
                t[:tt.size] = tt[:n - 1]
                T.append(t)
                del tab
        T, c = np.stack(T, axis=1), np.stack(c, axis=1)
        T.setflags(write=False)
        c.setflags(write=False)
        _REF[k] = (T, c)
    return _REF[k]


def split_margin(c, L):
    """the closest split decision of the bottom-up selection on the costs c of a full tree of depth L: min |cc - pc| / max(|cc|, |pc|)
    over every node, with the folded children's costs (BestBasis.jl:59-83)"""
    c = np.array(c, dtype=np.float64)
    worst = np.inf
    for i in range((1 << L) - 1, 0, -1):
        pc, cc = c[i - 1], c[2 * i - 1] + c[2 * i]
        den = max(abs(cc), abs(pc))
        if den > 0:
            worst = min(worst, abs(cc - pc) / den)
        if cc < pc:
            c[i - 1] = cc
    return worst


def bb(wx, cost):
    return wx.BB(cost=cost_of(wx, cost), redundant=True)


def entry(wx, transform):
    return wx.swpd_bestbasistreeall if transform == "swpd" else wx.acwpd_bestbasistreeall
