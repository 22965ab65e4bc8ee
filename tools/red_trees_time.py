"""Times iswpdall(xw, wt, M[, sm]) / iacwpdall(xw, M) with one tree per signal (csrc/wx_red_trees.hip) against what the library offered
before them, in one process on one build.

Shape: n = 256 samples, a table of depth 8 (511 columns), B = 4096 signals, Float64, db4: a 4 GiB table.  The signals are random walks,
the trees those of bestbasistreeall(swpdall(x, wt), BB(redundant = true), device = true) (for the autocorrelation rows: of
acwpdall(x, wt)), so they stay on the device.  Every row is the wall-clock time between two device synchronisations (2 warm-up calls,
then the minimum and the median of 7):
  (a) iswpdall(xw, wt, M)         average based            the whole call: prep launch, status read-back, one kernel
      iswpdall(xw, wt, M, 3)      shift based
      iacwpdall(xa, M)
  (b) a loop of iswpd(xw[:, :, i], wt, M[:, i]) / iacwpd(xa[:, :, i], M[:, i]) over 256 signals, scaled to B (an extrapolation)
  (c) iswpdall(xw, wt, M[:, 0])   the single-tree entry with column 0's tree for the whole batch: the bound
and the algorithmic bytes of (a): the leaf columns each tree reads, x written, the tree bytes.
`--kernel-only` runs the three calls of (a) three times each and nothing else, for a kernel trace to be taken around the process.

    python tools/red_trees_time.py [n [D [B]]] [--kernel-only]
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from wpt_trees_time import wall  # noqa: E402

PEAK = 8e12                                                           # HBM bytes per second


def leaves(M):
    """leaf nodes of every column: decomposed nodes + 1"""
    return M.sum(axis=0).astype(np.int64) + 1


def main(n=256, D=8, B=4096, kernel_only=False, loop=256):
    import torch
    import waveletsext_jl_amd as wx
    wt = wx.wavelet(wx.WT.db4)
    x = wx.to_device(np.asfortranarray(np.cumsum(np.random.default_rng(7).standard_normal((n, B)), axis=0)))   # random walks
    xw = wx.swpdall(x, wt, D)
    M = wx.bestbasistreeall(xw, wx.BB(redundant=True), device=True)
    Mh = M.cpu().numpy()
    print("n %d depth %d (%d columns) B %d Float64 db4, %.0f MiB per table; best-basis trees: %.1f leaves on average, %d distinct"
          % (n, D, xw.shape[1], B, xw.numel() * 8 / 2 ** 20, leaves(Mh).mean(), len({Mh[:, i].tobytes() for i in range(B)})), flush=True)
    calls = [("iswpdall(xw, wt, M)", lambda: wx.iswpdall(xw, wt, M), Mh),
             ("iswpdall(xw, wt, M, 3)", lambda: wx.iswpdall(xw, wt, M, 3), Mh)]
    if kernel_only:
        for _ in range(3):
            for _, fn, _ in calls:
                fn()
        del xw
        xa = wx.acwpdall(x, wt, D)
        Ma = wx.bestbasistreeall(xa, wx.BB(redundant=True), device=True)
        for _ in range(3):
            wx.iacwpdall(xa, Ma)
        torch.cuda.synchronize()
        return 0

    def report(name, t, route, Mx):
        nbytes = 8 * n * (int(leaves(Mx).sum()) + B) + Mx.size
        print("  (a) %-24s min %9.3f ms  median %9.3f ms  [%s]  %.1f MiB algorithmic, %.3f of 8 TB/s over the whole call"
              % (name, t[0], t[1], route, nbytes / 2 ** 20, nbytes / (t[0] * 1e-3) / PEAK), flush=True)

    m = min(loop, B)
    for name, fn, Mx in calls:
        t = wall(torch, fn)
        report(name, t, wx.wpt_trees_route(), Mx)
    e = float((wx.iswpdall(xw, wt, M) - x).abs().max() / x.abs().max())
    print("      round trip against x: %.2e" % e)
    for sm in (None, 3):
        cols = [(xw[:, :, i], Mh[:, i].copy()) for i in range(m)]
        tc = wall(torch, lambda: [wx.iswpd(c, wt, t, sm) for c, t in cols], warm=1, reps=3)
        print("  (b) loop of iswpd(sm = %s) over %d signals  min %9.3f ms -> %.0f ms for %d signals (extrapolated)"
              % (sm, m, tc[0], tc[0] * B / m, B), flush=True)
        del cols
    t0 = Mh[:, 0].copy()
    for sm in (None, 3):
        ts = wall(torch, lambda: wx.iswpdall(xw, wt, t0, sm))
        print("  (c) iswpdall(xw, wt, M[:, 0], sm = %s): one tree of %d leaves for the batch  min %9.3f ms  median %9.3f ms"
              % (sm, int(t0.sum()) + 1, ts[0], ts[1]), flush=True)
    del xw, M
    torch.cuda.empty_cache()
    xa = wx.acwpdall(x, wt, D)
    Ma = wx.bestbasistreeall(xa, wx.BB(redundant=True), device=True)
    Mah = Ma.cpu().numpy()
    print("autocorrelation table: %.1f leaves on average" % leaves(Mah).mean())
    t = wall(torch, lambda: wx.iacwpdall(xa, Ma))
    report("iacwpdall(xa, M)", t, wx.wpt_trees_route(), Mah)
    cols = [(xa[:, :, i], Mah[:, i].copy()) for i in range(m)]
    tc = wall(torch, lambda: [wx.iacwpd(c, t) for c, t in cols], warm=1, reps=3)
    print("  (b) loop of iacwpd over %d signals  min %9.3f ms -> %.0f ms for %d signals (extrapolated)" % (m, tc[0], tc[0] * B / m, B))
    t0 = Mah[:, 0].copy()
    ts = wall(torch, lambda: wx.iacwpdall(xa, t0))
    print("  (c) iacwpdall(xa, M[:, 0]): one tree of %d leaves for the batch  min %9.3f ms  median %9.3f ms" % (int(t0.sum()) + 1, ts[0], ts[1]))
    return 0


if __name__ == "__main__":
    nums = [int(v) for v in sys.argv[1:] if not v.startswith("--")]
    sys.exit(main(*nums[:3], kernel_only="--kernel-only" in sys.argv) or 0)
