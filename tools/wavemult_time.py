"""Times the batched wavelet-domain operator products against the dense product they replace.

M[i, j] = 1 / |i - j| (zero diagonal), n in {1024, 4096}, B = 4096 vectors, db4, L = maxtransformlevels(n), eps = 1e-4, Float64,
device tensors, hipEvents over 15 calls after warm-up (tools/floor_scan.py: timed).  Per n and form: nnz / n^2 of the sparse form,
the relative error of the product against M @ X, the whole call, its three stages (the product alone through
SparseMatrixCSC.matmul), the product's bytes per second on its own model -- layout bytes x signal tiles + the X and Y bytes --,
torch.matmul(M, X) on the same tensors, and dwtall + idwtall alone on the same batch.

    python tools/wavemult_time.py [n ...]
"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from floor_scan import timed  # noqa: E402


def main(lengths, B=4096, eps=1e-4):
    import torch
    import waveletsext_jl_amd as wx
    wt = wx.wavelet(wx.WT.db4)
    for n in lengths:
        L = wx.maxtransformlevels(n)
        i = torch.arange(n, device="cuda", dtype=torch.float64)
        d = (i[:, None] - i[None, :]).abs()
        M = wx.to_colmajor(torch.where(d > 0, 1.0 / d.clamp(min=1.0), torch.zeros_like(d)))
        X = wx.jl_empty((n, B), torch.float64, "cuda")
        X.normal_()
        dense = torch.matmul(M, X)
        t_dense = timed(torch, lambda: torch.matmul(M, X))
        t_pyr = timed(torch, lambda: wx.idwtall(wx.dwtall(X, wt, L), wt, L))
        print("n %5d B %d db4 L %d eps %g Float64: torch.matmul(M, X) %.3f ms; dwtall + idwtall alone %.3f ms" % (n, B, L, eps, t_dense, t_pyr),
              flush=True)
        for name, form, mul, fwd, inv in (("std", wx.mat2sparseform_std, wx.std_wavemultall, wx.dwtall, wx.idwtall),
                                          ("nonstd", wx.mat2sparseform_nonstd, wx.nonstd_wavemultall, wx.ns_dwtall, wx.ns_idwtall)):
            S = form(M, wt, L, eps)
            info = S.plan_info()
            Y = mul(S, X, wt, L)
            err = float((Y - dense).abs().max() / dense.abs().max())
            Xw = fwd(X, wt, L)
            Yw = S.matmul(Xw)
            t_all = timed(torch, lambda: mul(S, X, wt, L))
            t_fwd = timed(torch, lambda: fwd(X, wt, L))
            t_mul = timed(torch, lambda: S.matmul(Xw))
            t_inv = timed(torch, lambda: inv(Yw, wt, L))
            tiles = -(-B // info["tile"])
            model = info["layout_bytes"] * tiles + 2 * info["N"] * B * 8
            print("  %-6s nnz/n^2 %.4f (nnz %d, padded %d, slices %d, rows cut %d)  relerr vs M @ X %.2e" %
                  (name, info["nnz"] / float(n * n), info["nnz"], info["padded"], info["slices"], info["split_rows"], err))
            print("  %-6s whole call %.3f ms = analysis %.3f + product %.3f + synthesis %.3f (sum %.3f); product %.1f GB/s on %.1f MB "
                  "(layout %.2f MB x %d tiles + X, Y); dense / sparse path %.2f x" %
                  (name, t_all, t_fwd, t_mul, t_inv, t_fwd + t_mul + t_inv, model / (t_mul * 1e-3) / 1e9, model / 1e6,
                   info["layout_bytes"] / 1e6, tiles, t_dense / t_all), flush=True)
            del S, Xw, Yw, Y
        del M, X, dense
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main([int(v) for v in sys.argv[1:]] or [1024, 4096])
