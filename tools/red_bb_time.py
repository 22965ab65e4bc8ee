"""Times the redundant best bases and the denoising straight from the signals against the packet-table way, one process per run:

    python tools/red_bb_time.py signals swpd|acwpd [n [L [B]]] [--repeats R]     swpd_bestbasistreeall(x, wt, L, device=True), then
                                                                                  bestbasis_denoiseall(x, wt, L, transform)
    python tools/red_bb_time.py table   swpd|acwpd [n [L [B]]] [--repeats R]     M = bestbasistreeall(swpdall(x, wt, L), BB(redundant=True),
                                                                                  device=True), then that plus denoiseall(xw, kind, wt, tree=M)

Defaults: n = 256, L = 8, B = 4096, Float64, db4, device tensors.  Every figure is the wall-clock time of the whole call between two
device synchronisations: 3 warm-up calls, then the median (and the minimum) of R = 25.  The peak device memory is torch's
max_memory_allocated over the timed calls on top of the signals (the library's own scratch comes from the stream-ordered pool and is
not in it: the chunked route adds at most 256 MiB).  One JSON line per figure.  profiles/red_bb.md holds the numbers."""
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def wall(torch, fn, warm=3, reps=25):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ts.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(ts)), float(np.min(ts))


def main(way, kind, n=256, L=8, B=4096, reps=25):
    import torch
    import waveletsext_jl_amd as wx
    assert way in ("signals", "table") and kind in ("swpd", "acwpd")
    wt = wx.wavelet(wx.WT.db4)
    rng = np.random.default_rng(7)
    w = max(1, n // 16)
    x = np.zeros((n, B))
    for i in range(B):
        for s in rng.choice(n // w, size=3, replace=False):
            x[s * w:(s + 1) * w, i] = rng.choice([-1.0, 1.0]) * rng.uniform(20.0, 40.0)
    x = wx.to_device(np.asfortranarray(x + rng.standard_normal((n, B))))
    fwd = wx.swpdall if kind == "swpd" else wx.acwpdall
    bb = wx.BB(redundant=True)
    if way == "signals":
        trees = (lambda: (wx.swpd_bestbasistreeall if kind == "swpd" else wx.acwpd_bestbasistreeall)(x, wt, L, device=True))
        both = (lambda: wx.bestbasis_denoiseall(x, wt, L, kind))
    else:
        trees = (lambda: wx.bestbasistreeall(fwd(x, wt, L), bb, device=True))

        def both():
            xw = fwd(x, wt, L)
            return wx.denoiseall(xw, kind, wt, tree=wx.bestbasistreeall(xw, bb, device=True))
    for name, fn in (("trees", trees), ("trees + denoise", both)):
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        med, mn = wall(torch, fn, reps=reps)
        peak = (torch.cuda.max_memory_allocated() - base) / 2 ** 20
        print(json.dumps({"way": way, "transform": kind, "what": name, "n": n, "L": L, "B": B, "median_ms": round(med, 3), "min_ms": round(mn, 3),
                          "peak_MiB": round(peak, 1), "route": wx.red_bb_route() if way == "signals" else wx.wpt_trees_route()}), flush=True)
    return 0


if __name__ == "__main__":
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    reps = int(sys.argv[sys.argv.index("--repeats") + 1]) if "--repeats" in sys.argv else 25
    if "--repeats" in sys.argv:
        args.remove(str(reps))
    sys.exit(main(args[0], args[1], *[int(v) for v in args[2:5]], reps=reps))
