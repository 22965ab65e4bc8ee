"""Times wptall / iwptall / iwpdall with one tree per signal (csrc/wx_wpt_trees.hip) against what they replace.

n = 4096, B = 16384 signals, Float64, db4, one random tree per signal (helpers.random_tree_1d's rule, p = 0.7), device tensors.
The per-signal entries take the tree matrix from host memory and wait for their stream before they return, so every row is the
wall-clock time of the whole call between two device synchronisations (2 warm-up calls, then the minimum and the median of 7):
  forward   wptall(x, wt, trees)  against  getbasiscoefall(wpdall(x, wt), trees), both calls timed;
  inverse   iwptall(y, wt, trees) and iwpdall(table, wt, trees): time, and the fraction of the 8 TB/s peak on 2 n values per signal
            plus the tree bytes; next to them the single-tree calls of the same batch along the first tree (the masked lattice
            kernels: the ceiling), and ONE batch-1 single-tree call (what each iteration of a host loop over the signals costs).
`--kernel-only` runs each per-signal call three times and nothing else, for a kernel trace to be taken around the process.

    python tools/wpt_trees_time.py [n [B]] [--kernel-only]
"""
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def random_trees(n, B, rng, p):
    """helpers.random_tree_1d for every column at once: the root with probability 0.95, a child under a decomposed parent with p"""
    t = np.zeros((n - 1, B), dtype=bool, order="F")
    t[0] = rng.random(B) < 0.95
    lo = 2
    while lo < n:
        idx = np.arange(lo, min(2 * lo, n))                            # the nodes of one level
        t[idx - 1] = t[idx // 2 - 1] & (rng.random((idx.size, B)) < p)
        lo *= 2
    return t


def wall(torch, fn, warm=2, reps=7):
    for _ in range(warm):
        fn()
    ts = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ts.append((time.perf_counter() - t0) * 1e3)
    ts.sort()
    return ts[0], ts[len(ts) // 2]


def main(n=4096, B=16384, kernel_only=False, p=0.7):
    import torch
    import waveletsext_jl_amd as wx
    wt = wx.wavelet(wx.WT.db4)
    rng = np.random.default_rng(7)
    trees = random_trees(n, B, rng, p)
    depth = np.array([0 if not trees[:, b].any() else int(np.flatnonzero(trees[:, b])[-1] + 1).bit_length() for b in range(min(B, 512))])
    x = wx.jl_empty((n, B), torch.float64, "cuda")
    x.normal_()
    print("n %d B %d Float64 db4, random trees p = %.1f (depth of the first %d: mean %.1f, max %d), %.0f MiB of signals, %.1f MiB of trees"
          % (n, B, p, depth.size, depth.mean(), depth.max(), n * B * 8 / 2 ** 20, trees.nbytes / 2 ** 20), flush=True)
    if kernel_only:
        table = wx.wpdall(x, wt)
        for _ in range(3):
            y = wx.wptall(x, wt, trees)
            wx.iwptall(y, wt, trees)
            wx.iwpdall(table, wt, trees)
        torch.cuda.synchronize()
        return
    model = (2 * n * 8 + (n - 1)) * B                                   # bytes that have to move: signal in, signal out, the trees

    def row(name, t, frac=True):
        extra = "  %.1f %% of 8 TB/s on %.0f MB" % (100 * model / (t[0] * 1e-3) / 8e12, model / 1e6) if frac else ""
        print("  %-46s min %8.3f ms  median %8.3f ms%s" % (name, t[0], t[1], extra), flush=True)

    y = wx.wptall(x, wt, trees)
    t_new = wall(torch, lambda: wx.wptall(x, wt, trees))
    row("wptall(x, wt, trees)", t_new)
    table = wx.wpdall(x, wt)
    t_wpd = wall(torch, lambda: wx.wpdall(x, wt))
    t_gat = wall(torch, lambda: wx.getbasiscoefall(table, trees))
    row("wpdall(x, wt)", t_wpd, False)
    row("getbasiscoefall(table, trees)", t_gat, False)
    print("  forward: table + gather %.3f ms / per-signal wptall %.3f ms = %.2f x" % (t_wpd[0] + t_gat[0], t_new[0], (t_wpd[0] + t_gat[0]) / t_new[0]))
    err = float((y - wx.getbasiscoefall(table, trees)).abs().max() / y.abs().max())
    print("  wptall against the gathered table: relative difference %.2e" % err)
    row("iwptall(y, wt, trees)", wall(torch, lambda: wx.iwptall(y, wt, trees)))
    row("iwpdall(table, wt, trees)", wall(torch, lambda: wx.iwpdall(table, wt, trees)))
    one = np.ascontiguousarray(trees[:, 0])
    row("iwptall(y, wt, trees[:, 0])   single tree", wall(torch, lambda: wx.iwptall(y, wt, one)))
    row("iwpdall(table, wt, trees[:, 0]) single tree", wall(torch, lambda: wx.iwpdall(table, wt, one)))
    y1 = wx.to_colmajor(y[:, :1].clone())
    row("iwptall of ONE signal (a host loop's iteration)", wall(torch, lambda: wx.iwptall(y1, wt, one)), False)
    back = wx.iwptall(y, wt, trees)
    print("  round trip: relative error %.2e" % float((back - x).abs().max() / x.abs().max()))


if __name__ == "__main__":
    nums = [int(v) for v in sys.argv[1:] if not v.startswith("--")]
    main(*nums[:2], kernel_only="--kernel-only" in sys.argv)
