"""Times the per-signal-tree calls with the tree matrix in device memory (csrc/wx_trees_prep.hip) against the same calls with the
matrix in host memory, in one process on one build.

The shape of profiles/wpt_trees.md: n = 4096, B = 16384 signals, Float64, db4, one random tree per signal (tools/wpt_trees_time.py's
random_trees, seed 7, p = 0.7), device data.  Every row is the wall-clock time of the whole call between two device
synchronisations (2 warm-up calls, then the minimum and the median of 7):
  wptall / iwptall / iwpdall / getbasiscoefall     with `trees` a numpy matrix (host route) and a device tensor (device route), and
                                                   the route each call reported (wx.wpt_trees_route());
  bestbasistreeall(table, BB()) -> wptall          with the default (trees to the host and back) and with device=True.
`--kernel-only` runs each device-tree call three times and nothing else, for a kernel trace to be taken around the process.

    python tools/wpt_trees_device_time.py [n [B]] [--kernel-only]
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from wpt_trees_time import random_trees, wall  # noqa: E402


def main(n=4096, B=16384, kernel_only=False, p=0.7):
    import torch
    import waveletsext_jl_amd as wx
    wt = wx.wavelet(wx.WT.db4)
    rng = np.random.default_rng(7)
    trees = random_trees(n, B, rng, p)
    x = wx.jl_empty((n, B), torch.float64, "cuda")
    x.normal_()
    dtrees = wx.to_device(trees)
    table = wx.wpdall(x, wt)
    y = wx.wptall(x, wt, dtrees)
    print("n %d B %d Float64 db4, random trees p = %.1f, %.0f MiB of signals, %.1f MiB of trees" % (n, B, p, n * B * 8 / 2 ** 20, trees.nbytes / 2 ** 20),
          flush=True)
    calls = [("wptall(x, wt, trees)", lambda t: wx.wptall(x, wt, t)), ("iwptall(y, wt, trees)", lambda t: wx.iwptall(y, wt, t)),
             ("iwpdall(table, wt, trees)", lambda t: wx.iwpdall(table, wt, t)), ("getbasiscoefall(table, trees)", lambda t: wx.getbasiscoefall(table, t))]
    if kernel_only:
        for _ in range(3):
            for _, fn in calls:
                fn(dtrees)
        torch.cuda.synchronize()
        return
    slower = []
    for name, fn in calls:
        h = wall(torch, lambda: fn(trees))
        hr = wx.wpt_trees_route()
        d = wall(torch, lambda: fn(dtrees))
        dr = wx.wpt_trees_route()
        same = bool((fn(trees) == fn(dtrees)).all())
        print("  %-30s host trees   min %8.3f ms  median %8.3f ms  [%s]" % (name, h[0], h[1], hr), flush=True)
        print("  %-30s device trees min %8.3f ms  median %8.3f ms  [%s]  %.1f x, results %s" % ("", d[0], d[1], dr, h[0] / d[0], "identical" if same else "DIFFER"),
              flush=True)
        if not d[0] < h[0]:
            slower.append(name)

    def chain(device):
        t = wx.bestbasistreeall(table, wx.BB(), device=device)
        return wx.wptall(x, wt, t)

    t_bb = wall(torch, lambda: wx.bestbasistreeall(table, wx.BB()))
    t_bbd = wall(torch, lambda: wx.bestbasistreeall(table, wx.BB(), device=True))
    h, d = wall(torch, lambda: chain(False)), wall(torch, lambda: chain(True))
    print("  bestbasistreeall(table, BB())               min %8.3f ms  median %8.3f ms" % t_bb)
    print("  bestbasistreeall(table, BB(), device=True)  min %8.3f ms  median %8.3f ms" % t_bbd)
    print("  best basis -> wptall, default               min %8.3f ms  median %8.3f ms" % h)
    print("  best basis -> wptall, device=True           min %8.3f ms  median %8.3f ms  %.1f x" % (d[0], d[1], h[0] / d[0]))
    print("  device trees slower than host trees: %s" % (", ".join(slower) if slower else "none"))
    return 1 if slower else 0


if __name__ == "__main__":
    nums = [int(v) for v in sys.argv[1:] if not v.startswith("--")]
    sys.exit(main(*nums[:2], kernel_only="--kernel-only" in sys.argv) or 0)
