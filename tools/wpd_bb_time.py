"""Times the per-signal best basis of a batch of signals, whole calls on device tensors, one shape and one way per process:

    python tools/wpd_bb_time.py fused n B [--f32] [--repeats R]     wpd_bestbasistreeall(x, wt, device=True)        (csrc/wx_wpd_bb.hip)
    python tools/wpd_bb_time.py table n B [--f32] [--repeats R]     bestbasistreeall(wpdall(x, wt), BB(), device=True)

db4, Shannon entropy, full depth, standard normal signals with every third one replaced by its cumulative sum.  Three warm-up calls,
then R (default 25, at least 20) timed ones, each the wall-clock time between two device synchronisations; the line printed holds the
minimum and the median in ms, the route of the fused call, and the peak of torch's device allocations over the timed calls next to
the bytes of the signals and of the trees (both ways allocate their results through torch; the library's own scratch -- one norm
per signal on the table way, nothing in the fused kernel -- is not in that figure).  `table` uses nothing this feature added, so the
same command times the commit before it.  profiles/wpd_bb.md holds the numbers."""
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main(way, n, B, f32=False, repeats=25):
    import torch
    import waveletsext_jl_amd as wx
    assert way in ("fused", "table") and repeats >= 20
    wt = wx.wavelet(wx.WT.db4)
    dt = torch.float32 if f32 else torch.float64
    x = wx.jl_empty((n, B), dt, "cuda")
    torch.manual_seed(4100 + n)
    x.normal_()
    x[:, ::3] = torch.cumsum(x[:, ::3], dim=0)
    if way == "fused":
        def call():
            return wx.wpd_bestbasistreeall(x, wt, device=True)
    else:
        def call():
            return wx.bestbasistreeall(wx.wpdall(x, wt), wx.BB(), device=True)
    for _ in range(3):
        t = call()
    torch.cuda.synchronize()
    route = wx.wpd_bb_route() if way == "fused" else "-"
    ones = int(t.sum().item())
    del t
    torch.cuda.reset_peak_memory_stats()
    ms = []
    for _ in range(repeats):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        t = call()
        torch.cuda.synchronize()
        ms.append((time.perf_counter() - t0) * 1e3)
        del t
    peak = torch.cuda.max_memory_allocated()
    ms.sort()
    print("%-5s n %5d B %8d %s db4 shannon: min %8.3f ms  median %8.3f ms  (%d calls)  route %s  peak %9.1f MiB  signals %7.1f MiB  trees %6.1f MiB"
          "  decomposed nodes %d" % (way, n, B, "Float32" if f32 else "Float64", ms[0], ms[len(ms) // 2], repeats, route, peak / 2 ** 20,
                                     x.numel() * x.element_size() / 2 ** 20, (n - 1) * B / 2 ** 20, ones), flush=True)
    return 0


if __name__ == "__main__":
    import argparse
    ap = argparse.ArgumentParser(description="time the per-signal best basis of a batch of signals, one shape and one way per process")
    ap.add_argument("way", choices=("fused", "table"))
    ap.add_argument("n", type=int)
    ap.add_argument("B", type=int)
    ap.add_argument("--f32", action="store_true")
    ap.add_argument("--repeats", type=int, default=25)
    o = ap.parse_args()
    sys.exit(main(o.way, o.n, o.B, o.f32, o.repeats) or 0)
