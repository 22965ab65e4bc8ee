"""Times the per-signal-tree threshold selections (csrc/wx_shrink_trees.hip) on a redundant packet table in device memory, one process per
run:

    python tools/shrink_trees_time.py time swpd|acwpd [n [L [B]]] [--repeats R]
    python tools/shrink_trees_time.py once swpd|acwpd [n [L [B]]]                  one call of each selection (for a kernel trace)

Defaults: n = 256, L = 8, B = 4096, Float64, db4.  The trees are bestbasistreeall(table, BB(redundant=True), device=True); their leaf
counts (smallest, median, largest) are printed first, because the stationary and the autocorrelation bases differ by an order of magnitude.
Timed, each as the wall-clock time of the whole call between two device synchronisations (3 warm-up calls, the median and the minimum of
R = 25): surethresholdall and relerrorthresholdall(table, True, M); denoiseall(table, kind, wt, tree=M) with estnoise = noisest,
relerrorthreshold and surethreshold; and what a caller had to do before: a host loop of single-tree relerrorthresholdall(table[:, :, i:i+1],
True, M[:, i]) calls, timed once over the first 256 signals and EXTRAPOLATED to B.  One JSON line per figure.  profiles/shrink_trees.md
holds the numbers."""
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from red_bb_time import wall  # noqa: E402


def main(mode, kind, n=256, L=8, B=4096, reps=25):
    import torch
    import waveletsext_jl_amd as wx
    assert mode in ("time", "once") and kind in ("swpd", "acwpd")
    wt = wx.wavelet(wx.WT.db4)
    rng = np.random.default_rng(7)
    t = np.arange(n)[:, None]
    x = rng.standard_normal((n, B)) * np.exp(-t / (n / 8.0)) + 0.05 * rng.standard_normal((n, B))
    xd = wx.to_device(np.asfortranarray(x))
    td = (wx.swpdall if kind == "swpd" else wx.acwpdall)(xd, wt, L)
    M = wx.bestbasistreeall(td, wx.BB(redundant=True), device=True)
    leaves = (M.sum(dim=0) + 1).cpu().numpy()                          # a valid tree has popcount + 1 leaves
    npad = 2 ** np.ceil(np.log2(np.maximum(leaves * n, 2)))
    lds = 8192
    head = {"transform": kind, "n": n, "L": L, "B": B}
    print(json.dumps(dict(head, what="leaves", min=int(leaves.min()), median=float(np.median(leaves)), max=int(leaves.max()),
                          in_lds=int((npad <= lds).sum()), in_scratch=int((npad > lds).sum()),
                          classes=sorted({int(p) for p in npad}))), flush=True)
    sure = lambda: wx.surethresholdall(td, True, M)
    rel = lambda: wx.relerrorthresholdall(td, True, M)
    if mode == "once":
        sure()
        rel()
        torch.cuda.synchronize()
        return 0
    runs = [("surethresholdall", sure), ("relerrorthresholdall", rel),
            ("denoiseall noisest", lambda: wx.denoiseall(td, kind, wt, tree=M, dnt=wx.RelErrorShrink(wx.HardTH(), 0.3))),
            ("denoiseall relerrorthreshold", lambda: wx.denoiseall(td, kind, wt, tree=M, dnt=wx.RelErrorShrink(wx.HardTH(), 0.3),
                                                                   estnoise=wx.relerrorthreshold)),
            ("denoiseall surethreshold", lambda: wx.denoiseall(td, kind, wt, tree=M, dnt=wx.SureShrink(wx.HardTH(), 0.3),
                                                               estnoise=wx.surethreshold))]
    for name, fn in runs:
        med, mn = wall(torch, fn, reps=reps)
        print(json.dumps(dict(head, what=name, median_ms=round(med, 3), min_ms=round(mn, 3), route=wx.wpt_trees_route())), flush=True)
    # the loop a caller wrote before: a tree column to the host, a single-tree call, one value back, per signal
    S = min(256, B)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for i in range(S):
        wx.relerrorthresholdall(td[:, :, i:i + 1], True, M[:, i].cpu().numpy())
    torch.cuda.synchronize()
    dt = (time.perf_counter() - t0) * 1e3
    print(json.dumps(dict(head, what="host loop of single-tree relerrorthresholdall", signals_timed=S, ms=round(dt, 3),
                          extrapolated_ms=round(dt * B / S, 1))), flush=True)
    return 0


if __name__ == "__main__":
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    reps = int(sys.argv[sys.argv.index("--repeats") + 1]) if "--repeats" in sys.argv else 25
    if "--repeats" in sys.argv:
        args.remove(str(reps))
    sys.exit(main(args[0], args[1], *[int(v) for v in args[2:5]], reps=reps))
