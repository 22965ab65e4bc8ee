"""GPU parity of the noise estimate and the thresholds on non-finite and overflowing coefficients, against the numpy yardstick
tests/noisest_ref.py (Statistics.median! / mad! in the element type, the oracle's threshold rules).

Every kernel api_noisest (csrc/wx_denoise.hip) chooses by detail count is reached through the C entry with row_lo and col:
k_mad_wave (1, 2), k_mad_sort with 2 ... 16 signals per wavefront (3 ... 32) and one (33 ... 255), k_mad_count_rows (128, 256,
512), k_mad_count (1024 ... 4096), k_mad_count_wg (8192 ... 32768), k_mad (other counts up to 128 KiB of values) and k_mad_g
(more).  Each batch puts every case of noisest_ref.cases() between clean signals and ends on a ragged group; the estimates
must equal the yardstick bit for bit (NaN matching NaN), and the clean signals must equal those of the same batch without
the poisoned ones.  The one-pass kernels (k_lat_denoise_dwt_f64) are reached through wx_denoiseall_dwt_f64, the thresholds
through wx_threshold_* and the thresholding inverse (wx_iwpt1d_thresh_*) behind denoiseall."""
import ctypes

import numpy as np
import pytest

import noisest_ref as R
from helpers import relerr

pytestmark = pytest.mark.gpu

# detail counts per kernel of api_noisest with the default knobs (float32 reaches k_mad_g above 32768 values)
KERNEL_COUNTS = {
    "k_mad_wave": (1, 2),
    "k_mad_sort_PL": (3, 4, 5, 8, 13, 16, 17, 31, 32),
    "k_mad_sort_E": (33, 64, 100, 200, 255),
    "k_mad_count_rows": (128, 256, 512),
    "k_mad_count": (1024, 2048, 4096),
    "k_mad_count_wg": (8192, 16384, 32768),
    "k_mad": (300, 3000, 9000),
    "k_mad_g": (40000,),
}
TH = {"hard": "HardTH", "soft": "SoftTH", "semisoft": "SemiSoftTH", "stein": "SteinTH"}


def _lib():
    from waveletsext_jl_amd import _lib as L
    return L


def _noisest_c(X, row_lo, col):
    L = _lib()
    n, k, B = X.shape
    sig = np.empty(B, dtype=X.dtype)
    fn = getattr(L.lib(), "wx_noisest_f64" if X.dtype == np.float64 else "wx_noisest_f32")
    L.check(fn(ctypes.c_void_p(X.ctypes.data), n, k, B, row_lo, col, ctypes.c_void_p(sig.ctypes.data), None))
    return sig


def _batch(cnt, dtype, rng):
    """(details of every signal, the poisoned slots, the same batch with clean signals in those slots)"""
    cs = R.cases(cnt, dtype, rng)
    B = 2 * len(cs) + 1                              # 29: ragged for 2, 4, 8, 16 and 64 signals per group
    clean = rng.standard_normal((cnt, B)).astype(dtype)
    D = clean.copy()
    bad = []
    for j, v in enumerate(cs.values()):
        D[:, 2 * j + 1] = v
        bad.append(2 * j + 1)
    return D, bad, clean


def _embed(D, dtype):
    """the details as rows [row_lo, n) of column 1 of an (n, 2, B) table; column 0 and the rows above are NaN, so a kernel
    that reads outside the range gives NaN"""
    cnt, B = D.shape
    n = 1 << max(int(cnt - 1).bit_length(), 0)
    if n == cnt:
        n *= 2
    X = np.full((n, 2, B), np.nan, dtype=dtype, order="F")
    X[n - cnt:, 1, :] = D
    return X, n - cnt


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("kernel", list(KERNEL_COUNTS))
def test_noisest_every_kernel_nonfinite(wx, dtype, kernel):
    counts = KERNEL_COUNTS[kernel] + ((20000,) if kernel == "k_mad_g" and dtype == np.float64 else ())
    rng = np.random.default_rng(len(kernel) * 1009 + np.dtype(dtype).itemsize)
    for cnt in counts:
        D, bad, clean = _batch(cnt, dtype, rng)
        X, row_lo = _embed(D, dtype)
        sig = _noisest_c(X, row_lo, 1)
        for i in range(D.shape[1]):
            exp = R.noisest_range(D[:, i])
            assert R.same(sig[i:i + 1], np.array([exp], dtype=dtype)), (kernel, cnt, i, R.CASES[i // 2] if i in bad else "clean", sig[i], exp)
        Xc, _ = _embed(clean, dtype)
        sc = _noisest_c(Xc, row_lo, 1)
        keep = [i for i in range(D.shape[1]) if i not in bad]
        assert R.same(sig[keep], sc[keep]), (kernel, cnt)


def _dwt_c(xw, qmf, L, th_kind, t):
    lib = _lib()
    n, B = xw.shape
    y = np.empty_like(xw, order="F")
    sig = np.empty(B)
    q = np.ascontiguousarray(np.asarray(qmf, dtype=np.float64))
    lib.check(lib.lib().wx_denoiseall_dwt_f64(ctypes.c_void_p(xw.ctypes.data), ctypes.c_void_p(y.ctypes.data), n, L, B, ctypes.c_void_p(q.ctypes.data),
                                               len(q), th_kind, float(t), 0, ctypes.c_void_p(sig.ctypes.data), None))
    return y, sig


def _match_output(Y, exp, kept_finite, what, tol=1e-10):
    """the oracle's finite entries within tol, its non-finite entries non-finite.  When the thresholded table is finite
    (kept_finite) the non-finite positions are the same; a kept +-Inf / NaN coefficient may reach further through the
    lattice's rotations and lifting steps (Inf x 0 = NaN where the direct form has a zero tap), a difference by construction"""
    fy, fe = np.isfinite(Y), np.isfinite(exp)
    assert (fy <= fe).all(), what
    if kept_finite:
        assert (fy == fe).all(), what
    both = fy & fe
    if both.any():
        assert relerr(Y[both], exp[both]) <= tol, what


@pytest.mark.parametrize("n", [64, 128, 256, 512, 1024])
def test_onepass_dwt_nonfinite_details(wx, oracle, n):
    """k_lat_denoise_dwt_f64: 2^SH signals share a wavefront; sigma exact, the output as oracle.denoise(:dwt), the clean signals unchanged"""
    rng = np.random.default_rng(n + 77)
    wt = wx.wavelet(wx.WT.haar)
    L = wx.maxtransformlevels(n)
    B = max(3 * (4096 // n) + 5, 31)
    x = np.asfortranarray(rng.standard_normal((n, B)) + 3 * np.sin(np.arange(n) / 9.0)[:, None])
    xw0 = np.asfortranarray(wx.to_numpy(wx.dwtall(x, wt, L)))
    xw = xw0.copy(order="F")
    cs = R.cases(n // 2, np.float64, rng)
    bad = []
    for j, v in enumerate(cs.values()):
        xw[n // 2:, 2 * j + 1] = v
        bad.append(2 * j + 1)
    t = float(np.sqrt(2 * np.log(n)))
    for th_kind, th in enumerate(("hard", "soft", "semisoft")):
        y, sig = _dwt_c(xw, wt.qmf, L, th_kind, t)
        y0, sig0 = _dwt_c(xw0, wt.qmf, L, th_kind, t)
        for i in range(B):
            assert R.same(sig[i:i + 1], np.array([R.noisest_range(xw[n // 2:, i])])), (n, th, i, sig[i])
        for i in bad + [0, 2, B - 1]:
            exp = oracle.denoise(np.asfortranarray(xw[:, i]), "dwt", wt.qmf, L=L, th=th, t=t)
            kept = np.isfinite(oracle.threshold(xw[:, i], th, float(sig[i]) * t)).all()
            _match_output(y[:, i], exp, kept, (n, th, i))
        keep = [i for i in range(B) if i not in bad]
        assert R.same(sig[keep], sig0[keep]) and R.same(y[:, keep], y0[:, keep]), (n, th)


def _threshold_c(X, th_kind, t, inplace):
    lib = _lib()
    n, k, B = X.shape
    t = np.ascontiguousarray(np.atleast_1d(np.asarray(t, dtype=X.dtype)))
    Y = X if inplace else np.empty_like(X, order="F")
    fn = getattr(lib.lib(), "wx_threshold_f64" if X.dtype == np.float64 else "wx_threshold_f32")
    lib.check(fn(ctypes.c_void_p(X.ctypes.data), ctypes.c_void_p(Y.ctypes.data), n, k, B, th_kind, ctypes.c_void_p(t.ctypes.data), t.size, 0, None, None))
    return Y


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("th", ["hard", "soft", "semisoft", "stein"])
def test_threshold_nonfinite_bitexact(wx, oracle, dtype, th):
    """wx_threshold_*: +-0, subnormals, +-t, +-2t, huge, +-Inf, NaN with t = 0, finite, +Inf, NaN, huge -- in place and as a copy,
    one t and a t per signal, bit for bit as oracle.threshold"""
    T = np.dtype(dtype).type
    ts = [0.0, 0.7, np.inf, np.nan, float(R.big(dtype))]
    vals = np.concatenate([np.array([0.0, -0.0, 0.7, -0.7, 1.4, -1.4], dtype=dtype)] + [_vals(dtype, t) for t in ts])
    n = vals.size
    X = np.empty((n, 1, len(ts)), dtype=dtype, order="F")
    for b in range(len(ts)):
        X[:, 0, b] = np.roll(vals, 3 * b)
    kind = R.TH_KINDS[th]
    exp = np.stack([oracle.threshold(X[:, 0, b], th, T(ts[b])) for b in range(len(ts))], axis=1)
    for inplace in (False, True):
        Y = _threshold_c(X.copy(order="F"), kind, [T(v) for v in ts], inplace)
        assert R.same(Y[:, 0, :], exp), (th, inplace, "per signal")
        for b, tv in enumerate(ts):
            Y = _threshold_c(X.copy(order="F"), kind, [T(tv)], inplace)
            for c in range(len(ts)):
                assert R.same(Y[:, 0, c], oracle.threshold(X[:, 0, c], th, T(tv))), (th, inplace, tv, c)
    assert R.same(exp, np.stack([R.threshold(X[:, 0, b], th, ts[b]) for b in range(len(ts))], axis=1))


def _vals(dtype, t):
    tiny = np.finfo(dtype).smallest_subnormal
    huge = R.big(dtype)
    v = [tiny, -tiny, huge, -huge, np.inf, -np.inf, np.nan]
    if np.isfinite(t):
        v += [t, -t, 2 * t, -2 * t]
    with np.errstate(over="ignore"):
        return np.array(v, dtype=dtype)


def _poison_details(xw, rows, rng, dtype, which):
    """the finest details (rows) of the odd signals 1, 3, ... get the cases named in which"""
    cs = R.cases(len(rows), dtype, rng)
    bad = []
    for j, name in enumerate(which):
        xw[rows, 2 * j + 1] = cs[name]
        bad.append(2 * j + 1)
    return bad


def noisest_of(oracle, v, inputtype, tree):
    return oracle.noisest(v, False) if inputtype == "dwt" else oracle.noisest(v, False, tree)


# sigma +Inf (mad_inf), NaN (inf_half_p1, half_ninf_half_pinf, nan_inf), sigma * t above the largest finite value
INV_CASES = ("mad_inf", "inf_half_p1", "half_ninf_half_pinf", "nan_inf", "sigma_overflow", "pinf", "ninf")


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_thresholding_inverse_nonfinite_sigma(wx, oracle, dtype):
    """the threshold on the inverse's loads (wx_iwpt1d_thresh_*) with estimates of +Inf and NaN: denoiseall(:dwt) of 8192 samples (wx_noisest_*
    -> wx_iwpt1d_thresh_*) and denoiseall(:wpt) on device arrays, against oracle.denoise; the clean signals as without the poisoned ones"""
    import torch
    rng = np.random.default_rng(8192 + np.dtype(dtype).itemsize)
    wt = wx.wavelet(wx.WT.db4)
    tol = 1e-10 if dtype == np.float64 else 3e-4
    for inputtype, n, L in (("dwt", 8192, 5), ("wpt", 1024, 4)):
        B = 2 * len(INV_CASES) + 1
        x = np.asfortranarray((rng.standard_normal((n, B)) + 3 * np.sin(np.arange(n) / 40.0)[:, None]).astype(dtype))
        tree = wx.maketree(n, L, "full") if inputtype == "wpt" else None
        xw0 = np.asfortranarray(wx.to_numpy(wx.dwtall(x, wt, L) if inputtype == "dwt" else wx.wptall(x, wt, tree)))
        rows = np.arange(n // 2, n) if inputtype == "dwt" else np.arange(n - (n >> L), n)
        xw = xw0.copy(order="F")
        bad = _poison_details(xw, rows, rng, dtype, INV_CASES)
        for th in ("hard", "soft", "semisoft"):
            dnt = wx.VisuShrink(n, getattr(wx, TH[th])())
            kw = dict(L=L, dnt=dnt) if inputtype == "dwt" else dict(L=L, tree=tree, dnt=dnt)
            Y = wx.to_numpy(wx.denoiseall(torch.from_numpy(xw).cuda() if inputtype == "wpt" else xw, inputtype, wt, **kw))
            Y0 = wx.to_numpy(wx.denoiseall(torch.from_numpy(xw0).cuda() if inputtype == "wpt" else xw0, inputtype, wt, **kw))
            for i in bad + [0, B - 1]:
                okw = dict(L=L) if inputtype == "dwt" else dict(L=L, tree=tree)
                exp = oracle.denoise(np.asfortranarray(xw[:, i]), inputtype, wt.qmf, th=th, t=dnt.t, **okw)
                s_i = noisest_of(oracle, xw[:, i], inputtype, tree)
                kept = np.isfinite(oracle.threshold(xw[:, i], th, float(s_i) * dnt.t)).all()
                _match_output(Y[:, i], exp, kept, (inputtype, th, i), tol)
            keep = [i for i in range(B) if i not in bad]
            assert R.same(Y[:, keep], Y0[:, keep]), (inputtype, th)
