"""Times denoiseall(y, "wpt", wt, tree=trees) with one tree per signal (csrc/wx_denoise_trees.hip) against what the library offered
before it, in one process on one build.

The shape of profiles/wpt_trees_device.md: n = 4096, B = 16384 signals, Float64, db4, one random tree per signal
(tools/wpt_trees_time.py's random_trees, seed 7, p = 0.7), device data, device trees.  Every row is the wall-clock time between two
device synchronisations (2 warm-up calls, then the minimum and the median of 7):
  (a) denoiseall(y, "wpt", wt, tree=trees)         the whole call: prep launch, status read-back, one kernel;
      noisestall(y, False, trees)                  its estimate-only mode;
  (b) iwptall(y, wt, trees) + wx_noisest_* on rows [n / 2, n)
                                                   the nearest pair of passes that existed before: the same inverse without a threshold,
                                                   and a noise estimate on one fixed range (both entries are untouched by this feature);
  (c) a loop of denoise(y[:, i], "wpt", wt, tree=trees[:, i]) over 256 signals, scaled to B.
`--kernel-only` runs (a) and (b) three times each and nothing else, for a kernel trace to be taken around the process.

    python tools/denoise_trees_time.py [n [B]] [--kernel-only]
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from wpt_trees_time import random_trees, wall  # noqa: E402


def main(n=4096, B=16384, kernel_only=False, p=0.7, loop=256):
    import torch
    import waveletsext_jl_amd as wx
    from waveletsext_jl_amd import denoising
    wt = wx.wavelet(wx.WT.db4)
    rng = np.random.default_rng(7)
    trees = random_trees(n, B, rng, p)
    x = wx.jl_empty((n, B), torch.float64, "cuda")
    x.normal_()
    dtrees = wx.to_device(trees)
    y = wx.wptall(x, wt, dtrees)
    print("n %d B %d Float64 db4, random trees p = %.1f, %.0f MiB of coefficients" % (n, B, p, n * B * 8 / 2 ** 20), flush=True)

    def a():
        return wx.denoiseall(y, "wpt", wt, tree=dtrees)

    def b():
        out = wx.iwptall(y, wt, dtrees)
        sig = denoising._noisest(wx._arrays.Arg(y), True, "dwt", None, on_device=True)
        return out, sig

    if kernel_only:
        for _ in range(3):
            a()
            b()
        torch.cuda.synchronize()
        return 0
    ta = wall(torch, a)
    route = wx.wpt_trees_route()
    ts = wall(torch, lambda: wx.noisestall(y, False, dtrees))
    tb = wall(torch, b)
    ti = wall(torch, lambda: wx.iwptall(y, wt, dtrees))
    m = min(loop, B)
    cols = [(y[:, i].contiguous(), trees[:, i].copy()) for i in range(m)]
    tc = wall(torch, lambda: [wx.denoise(c, "wpt", wt, tree=t) for c, t in cols])
    print("  (a) denoiseall(y, :wpt, wt; tree = trees)       min %9.3f ms  median %9.3f ms  [%s]" % (ta[0], ta[1], route))
    print("      noisestall(y, false, trees)                 min %9.3f ms  median %9.3f ms" % ts)
    print("  (b) iwptall(y, wt, trees) + noisest on [n/2, n) min %9.3f ms  median %9.3f ms  (iwptall alone min %.3f ms)" % (tb[0], tb[1], ti[0]))
    print("  (c) loop of denoise over %d signals             min %9.3f ms  median %9.3f ms  -> %.0f ms for %d signals, %.0f x (a)"
          % (m, tc[0], tc[1], tc[0] * B / m, B, tc[0] * B / m / ta[0]))
    print("  (a) / (b) = %.2f" % (ta[0] / tb[0]))
    return 0


if __name__ == "__main__":
    nums = [int(v) for v in sys.argv[1:] if not v.startswith("--")]
    sys.exit(main(*nums[:2], kernel_only="--kernel-only" in sys.argv) or 0)
