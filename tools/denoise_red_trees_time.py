"""Times denoiseall(xw, :swpd | :acwpd, wt; tree = M) with one tree per signal (csrc/wx_denoise_red_trees.hip) against the walk it is
built on and against what a caller had to write before it, in one process on one build.

Shape: n = 256 samples, a table of depth 8 (511 columns), B = 4096 signals, Float64, db4: a 4 GiB table.  The signals are random walks
plus N(0, 1) noise, the trees those of bestbasistreeall(swpdall(x, wt), BB(redundant = true), device = true) (for the autocorrelation
rows: of acwpdall(x, wt)), so they stay on the device.  Every row is the wall-clock time between two device synchronisations (2 warm-up
calls, then the minimum and the median of 7):
  (a) denoiseall(xw, :swpd, wt; tree = M)      the whole call: prep launch, status read-back, one kernel
      denoiseall(xw, :swpd, nothing; tree = M) the thresholded table: prep, the estimate launch, the elementwise launch
      noisestall(xw, true, M)                  the estimates alone
      denoiseall(xa, :acwpd, wt; tree = M), noisestall(xa, true, M)
  (b) iswpdall(xw, wt, M) / iacwpdall(xa, M)   the same trees, no estimate, no threshold: the floor the walk sets
  (c) a loop of denoise(xw[:, :, i], :swpd | :acwpd, wt; tree = M[:, i]) over 256 signals, scaled to B (an extrapolation)
`--kernel-only` runs the calls of (a) and (b) three times each and nothing else, for a kernel trace to be taken around the process.

    python tools/denoise_red_trees_time.py [n [D [B]]] [--kernel-only]
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from wpt_trees_time import wall  # noqa: E402


def main(n=256, D=8, B=4096, kernel_only=False, loop=256):
    import torch
    import waveletsext_jl_amd as wx
    wt = wx.wavelet(wx.WT.db4)
    rng = np.random.default_rng(7)
    x = wx.to_device(np.asfortranarray(np.cumsum(rng.standard_normal((n, B)), axis=0) + rng.standard_normal((n, B))))
    m = min(loop, B)
    for kind in ("swpd", "acwpd"):
        xw = wx.swpdall(x, wt, D) if kind == "swpd" else wx.acwpdall(x, wt, D)
        M = wx.bestbasistreeall(xw, wx.BB(redundant=True), device=True)
        Mh = M.cpu().numpy()
        inv = (lambda: wx.iswpdall(xw, wt, M)) if kind == "swpd" else (lambda: wx.iacwpdall(xw, M))
        calls = [("denoiseall(xw, :%s, wt; tree = M)" % kind, lambda: wx.denoiseall(xw, kind, wt, tree=M)),
                 ("noisestall(xw, true, M)", lambda: wx.noisestall(xw, True, M)),
                 ("(b) %s with the same trees" % ("iswpdall(xw, wt, M)" if kind == "swpd" else "iacwpdall(xw, M)"), inv)]
        if kernel_only:
            for _ in range(3):
                for _, fn in calls:
                    fn()
            torch.cuda.synchronize()
            del xw, M
            torch.cuda.empty_cache()
            continue
        print("%s: n %d depth %d (%d columns) B %d Float64 db4, %.0f MiB per table; best-basis trees: %.1f leaves on average, %d distinct"
              % (kind, n, D, xw.shape[1], B, xw.numel() * 8 / 2 ** 20, Mh.sum(axis=0).mean() + 1, len({Mh[:, i].tobytes() for i in range(B)})),
              flush=True)
        res = {}
        for name, fn in calls:
            t = wall(torch, fn)
            res[name] = t
            print("  %s%-42s min %9.3f ms  median %9.3f ms  [%s]" % ("" if name.startswith("(b)") else "(a) ", name, t[0], t[1], wx.wpt_trees_route()),
                  flush=True)
        cols = [(xw[:, :, i], M[:, i:i + 1]) for i in range(m)]
        tc = wall(torch, lambda: [wx.denoise(c, kind, wt, tree=t) for c, t in cols], warm=1, reps=3)
        ta, tb = res[calls[0][0]][0], res[calls[2][0]][0]
        print("  (c) loop of denoise over %d signals            min %9.3f ms -> %.0f ms for %d signals (extrapolated), %.0f x (a)"
              % (m, tc[0], tc[0] * B / m, B, tc[0] * B / m / ta), flush=True)
        print("  (a) / (b) = %.2f" % (ta / tb), flush=True)
        del cols
        if kind == "swpd":
            t = wall(torch, lambda: wx.denoiseall(xw, "swpd", None, tree=M), warm=1, reps=3)
            print("  (a) %-42s min %9.3f ms  median %9.3f ms  [%s]" % ("denoiseall(xw, :swpd, nothing; tree = M)", t[0], t[1], wx.wpt_trees_route()),
                  flush=True)
        del xw, M
        torch.cuda.empty_cache()
    return 0


if __name__ == "__main__":
    nums = [int(v) for v in sys.argv[1:] if not v.startswith("--")]
    sys.exit(main(*nums[:3], kernel_only="--kernel-only" in sys.argv) or 0)
