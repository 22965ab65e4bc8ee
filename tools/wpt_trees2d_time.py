"""Times wptall / iwptall / iwpdall of images with one quad tree per image (csrc/wx_wpt_trees2d.hip) against what the library
could do for the same job before.

64 x 64 Float64 images, db4, one random quad tree per image (helpers.random_tree_2d's rule, p = 0.6), B = 32768 images (1 GiB),
device tensors.  Every figure is the minimum and the median of 12 timings between two device events after 3 warm-up calls:
  per-image calls   wptall / iwptall / iwpdall with `trees` a device tensor (prep launch + LDS kernel, one status read-back: the
                    whole call) and a numpy matrix (host check, packing and upload included), with the fraction of the 8 TB/s peak
                    on 2 m n values per image plus the tree bytes;
  forward before    getbasiscoefall(wpdall(x, wt), trees), both calls timed;
  host loop         what a reconstruction cost before: single-tree calls of ONE image each, timed on a slice of 256 images (wall
                    clock, and the time per image times B next to it);
  upper bound       the single-tree calls of the whole batch along the first tree (the masked 64 x 64 register kernels).
`--kernel-only` runs each per-image call three times with device trees and nothing else, for a kernel trace to be taken around
the process (the kernels alone).

    python tools/wpt_trees2d_time.py [m [B]] [--kernel-only]
"""
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def random_quad_trees(m, B, rng, p):
    """helpers.random_tree_2d for every column at once: the root always, a child under a decomposed parent with probability p"""
    L = int(m).bit_length() - 1
    nt = (4 ** L - 1) // 3
    t = np.zeros((nt, B), dtype=bool, order="F")
    t[0] = True
    lo = 2
    for d in range(1, L):
        idx = np.arange(lo, lo + 4 ** d)                               # the nodes of one level
        t[idx - 1] = t[(idx + 2) // 4 - 1] & (rng.random((idx.size, B)) < p)
        lo += 4 ** d
    return t


def events(torch, fn, warm=3, reps=12):
    for _ in range(warm):
        fn()
    ts = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        ts.append(a.elapsed_time(b))
    ts.sort()
    return ts[0], ts[len(ts) // 2]


def main(m=64, B=32768, kernel_only=False, p=0.6):
    import torch
    import waveletsext_jl_amd as wx
    wt = wx.wavelet(wx.WT.db4)
    rng = np.random.default_rng(7)
    trees = random_quad_trees(m, B, rng, p)
    nt = trees.shape[0]
    dtrees = wx.to_device(trees)
    x = wx.jl_empty((m, m, B), torch.float64, "cuda")
    x.normal_()
    leaves = trees.sum(axis=0)
    print("%d x %d x %d Float64 db4, random quad trees p = %.1f (decomposed nodes per tree: mean %.0f, max %d of %d), %.0f MiB of images, %.1f MiB of trees"
          % (m, m, B, p, leaves.mean(), leaves.max(), nt, m * m * B * 8 / 2 ** 20, trees.nbytes / 2 ** 20), flush=True)
    table = wx.wpdall(x, wt)
    y = wx.wptall(x, wt, dtrees)
    route = wx.wpt_trees_route()
    if kernel_only:
        for _ in range(3):
            wx.wptall(x, wt, dtrees)
            wx.iwptall(y, wt, dtrees)
            wx.iwpdall(table, wt, dtrees)
        torch.cuda.synchronize()
        return
    model = (2 * m * m * 8 + nt) * B                                   # bytes that have to move: image in, image out, the trees

    def row(name, t, frac=True):
        extra = "  %.1f %% of 8 TB/s on %.0f MB" % (100 * model / (t[0] * 1e-3) / 8e12, model / 1e6) if frac else ""
        print("  %-52s min %9.3f ms  median %9.3f ms%s" % (name, t[0], t[1], extra), flush=True)

    print("  route with device trees: %s" % route)
    t_new = events(torch, lambda: wx.wptall(x, wt, dtrees))
    row("wptall(x, wt, trees)              device trees", t_new)
    row("iwptall(y, wt, trees)             device trees", events(torch, lambda: wx.iwptall(y, wt, dtrees)))
    row("iwpdall(table, wt, trees)         device trees", events(torch, lambda: wx.iwpdall(table, wt, dtrees)))
    row("wptall(x, wt, trees)              host trees", events(torch, lambda: wx.wptall(x, wt, trees)))
    row("iwptall(y, wt, trees)             host trees", events(torch, lambda: wx.iwptall(y, wt, trees)))
    row("iwpdall(table, wt, trees)         host trees", events(torch, lambda: wx.iwpdall(table, wt, trees)))
    t_wpd = events(torch, lambda: wx.wpdall(x, wt))
    t_gat = events(torch, lambda: wx.getbasiscoefall(table, dtrees))
    row("wpdall(x, wt)", t_wpd, False)
    row("getbasiscoefall(table, trees)     device trees", t_gat, False)
    print("  forward: table + gather %.3f ms / per-image wptall %.3f ms = %.2f x" % (t_wpd[0] + t_gat[0], t_new[0], (t_wpd[0] + t_gat[0]) / t_new[0]))
    err = float((y - wx.getbasiscoefall(table, dtrees)).abs().max() / y.abs().max())
    print("  wptall against the gathered table: relative difference %.2e" % err)
    back = wx.iwptall(y, wt, dtrees)
    print("  round trip: relative error %.2e" % float((back - x).abs().max() / x.abs().max()))
    one = np.ascontiguousarray(trees[:, 0])
    row("wptall(x, wt, trees[:, 0])        single tree", events(torch, lambda: wx.wptall(x, wt, one)))
    row("iwptall(y, wt, trees[:, 0])       single tree", events(torch, lambda: wx.iwptall(y, wt, one)))
    row("iwpdall(table, wt, trees[:, 0])   single tree", events(torch, lambda: wx.iwpdall(table, wt, one)))
    S = min(256, B)                                                    # the host loop, on a SLICE of the batch
    xs = [wx.to_colmajor(x[:, :, b:b + 1].clone()) for b in range(S)]
    ys = [wx.to_colmajor(y[:, :, b:b + 1].clone()) for b in range(S)]
    cols = [np.ascontiguousarray(trees[:, b]) for b in range(S)]
    for name, fn, src in (("wptall", wx.wptall, xs), ("iwptall", wx.iwptall, ys)):
        for b in range(8):
            fn(src[b], wt, cols[b])
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for b in range(S):
            fn(src[b], wt, cols[b])
        torch.cuda.synchronize()
        dt = (time.perf_counter() - t0) * 1e3
        print("  host loop of single-tree %-8s %d images (a slice) %9.3f ms = %.4f ms per image; times %d images: %.0f ms"
              % (name + ":", S, dt, dt / S, B, dt / S * B), flush=True)


if __name__ == "__main__":
    nums = [int(v) for v in sys.argv[1:] if not v.startswith("--")]
    main(*nums[:2], kernel_only="--kernel-only" in sys.argv)
