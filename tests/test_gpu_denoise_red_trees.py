"""denoiseall(xw, "swpd" | "acwpd", wt, tree=M) and noisestall(xw, True, M) with M an (n - 1, N) matrix -- one tree per signal, every signal
denoised from its redundant packet table in its own basis (csrc/wx_denoise_red_trees.hip) -- against the oracle called per signal with that
signal's table and column: the noise estimates bit for bit, the signals within 20 * helpers.TOL (the bound of tests/test_gpu_denoise.py for
the redundant input types), the thresholded table of wt = None byte for byte; host trees, bool and uint8 device trees and repeated calls byte
for byte; `wx.wpt_trees_route()` after every call; the input table unchanged.

The tables are the library's own swpdall / acwpdall of a seeded piecewise-constant signal (three bursts of height 20 .. 40 on a zero level)
plus N(0, 1) noise, copied to the host, so the library and the oracle see the same bits: with identical bits and an exact sigma no Hard
decision can flip.  Eleven trees of depth <= D per case (`_trees11` of tests/test_gpu_red_trees.py).  Shapes: n = 8, D = 3 (nodes shorter
than the filters: the wrap; the estimate pads its wavefront); n = 64, D = 6 (the detail column is one value per lane); n = 256, D = 8
(several wavefronts, a deep stack); n = 1024 with the deepest table the LDS window admits (D = 8 in Float64, D = 10 in Float32; the
estimate moved the window's bytes by 16 and capped n at 1024, neither of which moves these); n = 1024, D = 10 in Float64, outside it."""
import ctypes

import numpy as np
import pytest

import helpers
from test_gpu_red_trees import _bytes, _clip, _dev, _trees11

pytestmark = pytest.mark.gpu

LDS, SINGLE, COPIED, HOST = "device prep + lds kernel", "device prep + single tree", "device trees copied to host", "host trees"
RULES = ("hard", "soft", "semisoft", "stein")
SMOOTH = ("regular", "undersmooth")
P, L64, I, D64 = ctypes.c_void_p, ctypes.c_int64, ctypes.c_int, ctypes.c_double


def _window_depth(n, dtype):
    """the deepest table whose 2 D n values, 512 bytes of filter, tree bits and the estimate's 16 bytes fit 136 KiB"""
    D = int(n).bit_length() - 1
    while 512 + 2 * D * n * np.dtype(dtype).itemsize + 4 * max(1, n // 32) + 16 > 136 * 1024:
        D -= 1
    return D


def _signals(n, B, rng, dtype):
    """three bursts of n // 16 samples (at least one) of height +-(20 .. 40) on a zero level, plus N(0, 1): at most 3 / 16 of a signal is
    off the zero level (3 / 8 at n = 8), so the median absolute deviation of the signal itself stays that of the noise"""
    w = max(1, n // 16)
    x = np.zeros((n, B))
    for i in range(B):
        for s in rng.choice(n // w, size=3, replace=False):
            x[s * w:(s + 1) * w, i] = rng.choice([-1.0, 1.0]) * rng.uniform(20.0, 40.0)
    return np.asfortranarray((x + rng.standard_normal((n, B))).astype(dtype))


def _th(wx, rule):
    return {"hard": wx.HardTH, "soft": wx.SoftTH, "semisoft": wx.SemiSoftTH, "stein": wx.SteinTH}[rule]()


def _oracle_sigma(oracle, th, trees):
    return np.array([oracle.noisest(th[:, :, i], True, trees[:, i]) for i in range(trees.shape[1])], dtype=th.dtype)


def _oracle_denoise(oracle, th, kind, qmf, trees, rule, t, smooth, est=None):
    return np.stack([oracle.denoise(th[:, :, i], kind, qmf, tree=trees[:, i], th=rule, t=t, smooth=smooth,
                                    estnoise=None if est is None else float(est[i])) for i in range(trees.shape[1])], axis=-1)


def _same_sigma(got, want):
    """bit for bit, NaN matching NaN"""
    got, want = np.asarray(got), np.asarray(want)
    return got.dtype == want.dtype and got.shape == want.shape and bool(((got == want) | (np.isnan(got) & np.isnan(want))).all())


def _condition(oracle, th, trees, sigma):
    """on the oracle's result alone: at least 5 of the 11 estimates are non-zero (all of the columns when fewer are tried); for n >= 64 every
    such column has zeroed and kept leaf coefficients under HardTH with t = sqrt(2 log n) -- a case in which every decision goes one way
    would check no threshold; with undersmooth the coarsest scaling node's column is unchanged for every tree whose root is decomposed"""
    n, B = th.shape[0], trees.shape[1]
    t = float(np.sqrt(2 * np.log(n)))
    nz = np.flatnonzero(sigma != 0)
    assert nz.size >= min(5, B), sigma
    for i in range(B):
        leaves = np.flatnonzero(oracle.getleaf(trees[:, i], "binary"))
        leaves = leaves[leaves < th.shape[1]]
        if n >= 64 and i in nz:
            o = oracle.denoise(th[:, :, i], "swpd", None, tree=trees[:, i], th="hard", t=t, smooth="regular")
            assert (o[:, leaves] == 0).any() and (o[:, leaves] != 0).any(), i
        if trees[0, i]:
            u = oracle.denoise(th[:, :, i], "swpd", None, tree=trees[:, i], th="hard", t=t, smooth="undersmooth")
            c = oracle.coarsestscalingrange(n, trees[:, i], True) - 1
            assert c in leaves or n == 2
            assert u[:, c].tobytes() == th[:, c, i].tobytes(), i


def _abi(wx, kind, td, wt, dtrees, rule, t, smooth, thr=None):
    """the C entry with both outputs in device memory: (xhat, sigma) as tensors"""
    import torch
    n, ncols, B = td.shape
    dt = td.dtype
    out = torch.full((B, n), -7.25, dtype=dt, device=td.device)       # column-major (n, B)
    sig = torch.full((B,), -7.25, dtype=dt, device=td.device)
    q = np.ascontiguousarray(wt.qmf, dtype=np.float64)
    lib = wx._lib.lib()
    src = td.permute(2, 1, 0).contiguous()                            # column-major (n, ncols, B)
    tr = dtrees.t().contiguous()
    head = (P(src.data_ptr()), P(out.data_ptr()), L64(n), L64(ncols), P(tr.data_ptr()), L64(n - 1), L64(B))
    tail = (I(RULES.index(rule)), D64(t), P(0 if thr is None else thr.data_ptr()), L64(0 if thr is None else thr.numel()),
            I(1 if smooth == "undersmooth" else 0), P(sig.data_ptr()), P(torch.cuda.current_stream().cuda_stream))
    if kind == "acwpd":
        rc = lib.wx_denoise_acwpd1d_trees_f64(*head, *tail)
    else:
        fn = lib.wx_denoise_swpd1d_trees_f32 if dt == torch.float32 else lib.wx_denoise_swpd1d_trees_f64
        rc = fn(*head, P(q.ctypes.data), I(q.size), *tail)
    assert rc == 0, wx._lib.lib().wx_last_error()
    torch.cuda.synchronize()
    return out.cpu().numpy().T, sig.cpu().numpy()


def _check(wx, oracle, n, D, wname, dtype, inside=True, cols=None, full=False):
    import torch
    rng = np.random.default_rng(1000 * n + 10 * D + len(wname))
    wt = wx.wavelet(wname)
    tol = 20 * helpers.TOL[np.dtype(dtype)]
    trees = _trees11(wx, n, D, rng)
    if cols is not None:
        trees = np.asfortranarray(trees[:, cols])
    B = trees.shape[1]
    x = _signals(n, B, rng, dtype)
    xd = wx.to_device(x)
    t = float(np.sqrt(2 * np.log(n)))
    dtb, dtu = _dev(wx, trees), _dev(wx, trees, np.uint8)
    want_dev = LDS if inside else COPIED
    combos = [(r, s) for r in RULES for s in SMOOTH] if full else [(r, SMOOTH[i % 2]) for i, r in enumerate(RULES)]
    for kind in ("swpd", "acwpd") if dtype == np.float64 else ("swpd",):
        td = wx.swpdall(xd, wt, D) if kind == "swpd" else wx.acwpdall(xd, wt, D)
        th = wx.to_numpy(td)                                           # the same bits for the oracle
        assert th.shape == (n, (1 << (D + 1)) - 1, B) and th.dtype == np.dtype(dtype)
        sigma = _oracle_sigma(oracle, th, trees)
        _condition(oracle, th, trees, sigma)
        for tr, route in ((dtb, want_dev), (trees, HOST)):
            s = wx.noisestall(td, True, tr)
            assert wx.wpt_trees_route() == route, wx.wpt_trees_route()
            assert isinstance(s, torch.Tensor) and s.is_cuda and tuple(s.shape) == (B,)
            print(kind, "sigma", wx.to_numpy(s), sigma)
            assert _same_sigma(wx.to_numpy(s), sigma), (kind, route)
        for rule, smooth in combos:
            dnt = wx.VisuShrink(_th(wx, rule), t)
            d = wx.denoiseall(td, kind, wt, tree=dtb, dnt=dnt, smooth=smooth)
            assert wx.wpt_trees_route() == want_dev, wx.wpt_trees_route()
            assert isinstance(d, torch.Tensor) and d.is_cuda and tuple(d.shape) == (n, B)
            want = _oracle_denoise(oracle, th, kind, wt.qmf, trees, rule, t, smooth)
            g = wx.to_numpy(d)
            for i in range(B):
                e = helpers.relerr(g[:, i], want[:, i])
                assert e <= tol, (kind, rule, smooth, i, e)
            print(kind, rule, smooth, "against the oracle", helpers.relerr(g, want))
            h = wx.denoiseall(td, kind, wt, tree=trees, dnt=dnt, smooth=smooth)
            assert wx.wpt_trees_route() == HOST
            assert _bytes(wx, h) == g.tobytes(), (kind, rule, smooth, "device trees and host trees differ")
        # the last combination again: uint8 device trees, a repeated call, and the entry's own sigma output
        assert _bytes(wx, wx.denoiseall(td, kind, wt, tree=dtu, dnt=dnt, smooth=smooth)) == g.tobytes()
        assert wx.wpt_trees_route() == want_dev
        assert _bytes(wx, wx.denoiseall(td, kind, wt, tree=dtb, dnt=dnt, smooth=smooth)) == g.tobytes()
        with pytest.raises(wx.WxError) as err:                         # a table in host memory: the Python layer's refusal stands
            wx.denoiseall(th, kind, wt, tree=trees, dnt=dnt, smooth=smooth)
        assert err.value.code == wx._lib.WX_EUNSUPPORTED
        ga, sa = _abi(wx, kind, td, wt, dtb, rule, t, smooth)
        assert wx.wpt_trees_route() == want_dev
        assert _same_sigma(sa, sigma) and ga.tobytes() == g.tobytes(), kind
        # precomputed estimates, one per signal, and a summary threshold: the oracle with the same numbers
        est = (np.abs(sigma.astype(np.float64)) * 1.25 + 0.5).astype(dtype)
        d = wx.denoiseall(td, kind, wt, tree=dtb, dnt=wx.VisuShrink(wx.SoftTH(), t), estnoise=est, smooth="undersmooth")
        assert wx.wpt_trees_route() == want_dev
        want = _oracle_denoise(oracle, th, kind, wt.qmf, trees, "soft", t, "undersmooth", est)
        assert helpers.relerr(wx.to_numpy(d), want) <= tol, (kind, "estnoise")
        d = wx.denoiseall(td, kind, wt, tree=dtb, dnt=wx.VisuShrink(wx.HardTH(), t), bestTH=np.median)
        assert wx.wpt_trees_route() == want_dev
        med = np.full(B, np.median(sigma.astype(np.float64))).astype(dtype)
        want = _oracle_denoise(oracle, th, kind, wt.qmf, trees, "hard", t, "regular", med)
        assert helpers.relerr(wx.to_numpy(d), want) <= tol, (kind, "bestTH")
        if kind == "swpd":
            # wt = None: the thresholded table, the same bits, the same sigma, the same rounding
            for rule, smooth in (("hard", "undersmooth"), ("soft", "regular")):
                dnt = wx.VisuShrink(_th(wx, rule), t)
                tb = wx.denoiseall(td, "swpd", None, tree=dtb, dnt=dnt, smooth=smooth)
                assert wx.wpt_trees_route() == want_dev
                assert tuple(tb.shape) == tuple(td.shape)
                want = _oracle_denoise(oracle, th, "swpd", None, trees, rule, t, smooth)
                got = wx.to_numpy(tb)
                assert got.dtype == want.dtype and got.tobytes() == want.tobytes(), (rule, smooth)
                assert _bytes(wx, wx.denoiseall(td, "swpd", None, tree=trees, dnt=dnt, smooth=smooth)) == _bytes(wx, tb)
                assert wx.wpt_trees_route() == HOST
        assert _bytes(wx, td) == th.tobytes(), "the input table was modified"


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("wname", ["haar", "db4", "db10"])
@pytest.mark.parametrize("n,D", [(8, 3), (64, 6), (256, 8), (1024, "window")])
def test_parity_with_the_oracle_per_signal(wx, oracle, n, D, wname, dtype):
    """four rules x two smooth values at n = 64, the diagonal (rule i with smooth i mod 2) elsewhere"""
    if D == "window":
        D = _window_depth(n, dtype)
        assert D == (8 if dtype == np.float64 else 10)
    _check(wx, oracle, n, D, wname, dtype, full=n == 64)


def test_just_outside_the_window(wx, oracle):
    """n = 1024 with a table of depth 10 needs 160 KiB in Float64: the single-tree pipeline once per signal, a device matrix coming to the
    host first"""
    assert _window_depth(1024, np.float64) < 10
    _check(wx, oracle, 1024, 10, "db4", np.float64, inside=False, cols=[4, 7, 9])   # right-deep to 10 and two random trees


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_identical_columns_take_the_single_tree_pipeline(wx, oracle, dtype):
    n, D, B = 64, 5, 7
    rng = np.random.default_rng(9)
    wt = wx.wavelet(wx.WT.db4)
    tree = _clip(helpers.random_tree_1d(n, rng, 0.8), D)
    assert tree[0]
    M = np.asfortranarray(np.repeat(tree[:, None], B, axis=1))
    xd = wx.to_device(_signals(n, B, rng, dtype))
    t = float(np.sqrt(2 * np.log(n)))
    tol = 20 * helpers.TOL[np.dtype(dtype)]
    for kind in ("swpd", "acwpd") if dtype == np.float64 else ("swpd",):
        td = wx.swpdall(xd, wt, D) if kind == "swpd" else wx.acwpdall(xd, wt, D)
        th = wx.to_numpy(td)
        sigma = _oracle_sigma(oracle, th, M)
        assert _same_sigma(wx.to_numpy(wx.noisestall(td, True, _dev(wx, M))), sigma)
        assert wx.wpt_trees_route() == SINGLE
        for rule, smooth in (("hard", "undersmooth"), ("stein", "regular")):
            dnt = wx.VisuShrink(_th(wx, rule), t)
            d = wx.denoiseall(td, kind, wt, tree=_dev(wx, M), dnt=dnt, smooth=smooth)
            assert wx.wpt_trees_route() == SINGLE
            assert helpers.relerr(wx.to_numpy(d), _oracle_denoise(oracle, th, kind, wt.qmf, M, rule, t, smooth)) <= tol
            assert _bytes(wx, d) == _bytes(wx, wx.denoiseall(td, kind, wt, tree=tree, dnt=dnt, smooth=smooth))   # the single-tree call
            assert _bytes(wx, d) == _bytes(wx, wx.denoiseall(td, kind, wt, tree=M, dnt=dnt, smooth=smooth))
            assert wx.wpt_trees_route() == HOST
        assert _bytes(wx, td) == th.tobytes()


def test_single_signal_form_takes_a_one_column_matrix(wx, oracle):
    n, D = 64, 4
    rng = np.random.default_rng(3)
    wt = wx.wavelet(wx.WT.db4)
    tree = _clip(helpers.random_tree_1d(n, rng, 0.8), D)
    x = _signals(n, 1, rng, np.float64)[:, 0]
    t = float(np.sqrt(2 * np.log(n)))
    for kind in ("swpd", "acwpd"):
        tb = wx.swpd(wx.to_device(x), wt, D) if kind == "swpd" else wx.acwpd(wx.to_device(x), wt, D)
        th = wx.to_numpy(tb)
        d = wx.denoise(tb, kind, wt, tree=_dev(wx, tree[:, None]), dnt=wx.VisuShrink(wx.SoftTH(), t))
        assert tuple(d.shape) == (n,)
        want = oracle.denoise(th, kind, wt.qmf, tree=tree, th="soft", t=t)
        assert helpers.relerr(wx.to_numpy(d), want) <= 20 * helpers.TOL[np.dtype(np.float64)]


def test_non_finite_details(wx, oracle):
    """a NaN in one signal's finest detail column: its estimate is NaN, nothing of it is thresholded; +Inf in another's: the medians stay
    finite.  Every other signal as without them."""
    n, D = 64, 6
    rng = np.random.default_rng(11)
    wt = wx.wavelet(wx.WT.db4)
    trees = _trees11(wx, n, D, rng)
    B = trees.shape[1]
    th = np.array(wx.to_numpy(wx.swpdall(wx.to_device(_signals(n, B, rng, np.float64)), wt, D)), order="F")
    clean = _oracle_sigma(oracle, th, trees)
    inf = float("inf")
    for b, v in ((6, np.nan), (8, inf)):
        col = oracle.finestdetailrange(n, trees[:, b], True) - 1
        th[n // 3, col, b] = v
    sigma = _oracle_sigma(oracle, th, trees)
    assert np.isnan(sigma[6]) and np.isfinite(sigma[8]) and sigma[8] != 0
    assert (np.delete(sigma, [6, 8]) == np.delete(clean, [6, 8])).all()
    td, dtb = wx.to_device(th), _dev(wx, trees)
    for tr, route in ((dtb, LDS), (trees, HOST)):
        assert _same_sigma(wx.to_numpy(wx.noisestall(td, True, tr)), sigma)
        assert wx.wpt_trees_route() == route
    t = float(np.sqrt(2 * np.log(n)))
    for wtx in (wt, None):
        d, sa = _abi(wx, "swpd", td, wt, dtb, "hard", t, "regular") if wtx is not None else (None, None)
        g = wx.to_numpy(wx.denoiseall(td, "swpd", wtx, tree=dtb, dnt=wx.VisuShrink(wx.HardTH(), t)))
        assert wx.wpt_trees_route() == LDS
        want = _oracle_denoise(oracle, th, "swpd", None if wtx is None else wt.qmf, trees, "hard", t, "regular")
        fin = np.isfinite(want)
        assert (np.isnan(g) == np.isnan(want)).all() and (g[~fin & ~np.isnan(want)] == want[~fin & ~np.isnan(want)]).all()
        scale = np.abs(want[fin]).max()
        assert np.allclose(g, want, rtol=0, atol=20 * helpers.TOL[np.dtype(np.float64)] * scale, equal_nan=True)
        if wtx is not None:
            assert _same_sigma(sa, sigma) and np.array_equal(d, g, equal_nan=True)
            assert np.isnan(g[:, 6]).any() and not np.isnan(np.delete(g, [6, 8], axis=1)).any()
    assert _bytes(wx, td) == th.tobytes()
