"""swpd_denoiseall / acwpd_denoiseall / red_noisestall / bestbasis_denoiseall (wx_denoise_swpd1d_sig_trees_*,
wx_denoise_acwpd1d_sig_trees_f64, csrc/wx_denoise_red_sig.hip): every signal denoised in its own redundant basis straight from the
signals, against the oracle called per signal ON ITS OWN TABLE (oracle.swpd / oracle.acwpd, oracle.noisest, oracle.denoise), never the
library's.  Signals, filters and the oracle's best-basis trees are those of tests/red_bb_cases.py (tests/test_red_bb_cpu.py guards
them); four trees of fixed shape, clipped to depth L, follow them: the bare root, the full tree, the left-deep (:dwt) and the
right-deep one.

Bound: 20 * helpers.TOL by helpers.relerr, the project's bound for the redundant input types, for the signals and (relative) for
sigma.  sigma is not bit for bit: the coefficients come from an equivalent but different forward step."""
import numpy as np
import pytest

import helpers
import red_bb_cases as cases

pytestmark = pytest.mark.gpu

FUSED, CHUNKED, TRIVIAL = 1, 2, 3
RULES = ("hard", "soft", "semisoft", "stein")
SIG_CASES = [("swpd", c) for c in cases.F64_CASES if c[4] == "shannon"] + [("acwpd", c) for c in cases.F64_CASES if c[4] == "shannon"]


def _bound(dtype):
    return 20 * helpers.TOL[np.dtype(dtype)]


def _shapes(n, L):
    """bare root, full, left-deep (:dwt), right-deep: (n - 1, 4), no node of depth >= L decomposed"""
    t = np.zeros((n - 1, 4), dtype=bool)
    t[:(1 << L) - 1, 1] = True
    for d in range(L):
        t[(1 << d) - 1, 2] = True                                     # node 2^d
        t[(2 << d) - 2, 3] = True                                     # node 2^(d + 1) - 1
    return t


def _th(wx, rule):
    return {"hard": wx.HardTH, "soft": wx.SoftTH, "semisoft": wx.SemiSoftTH, "stein": wx.SteinTH}[rule]()


_CASE = {}


def _case(wx, oracle, transform, n, L, B, filt, dtype=np.float64):
    """(x (n, N), trees (n - 1, N), the oracle's tables): N = B + 4, the four fixed shapes on the first four signals again"""
    k = (transform, n, L, B, filt, np.dtype(dtype).str)
    if k not in _CASE:
        T_o, _ = cases.reference(wx, oracle, transform, n, L, B, filt, "shannon", dtype)
        x = cases.signals(n, L, B).astype(dtype)
        x = np.asfortranarray(np.concatenate([x, x[:, :4]], axis=1))
        trees = np.asfortranarray(np.concatenate([T_o, _shapes(n, L)], axis=1))
        q = cases.qmf(wx, filt)
        tabs = [cases.table(oracle, transform, x[:, i], q, L) if L > 0 else np.asfortranarray(x[:, i:i + 1]) for i in range(x.shape[1])]
        for a in (x, trees):
            a.setflags(write=False)
        _CASE[k] = (x, trees, tabs)
    return _CASE[k]


def _oracle(wx, oracle, transform, tabs, trees, filt, rule, t, smooth, est=None):
    q = cases.qmf(wx, filt)
    out = [oracle.denoise(tabs[i], transform, q, tree=trees[:, i], th=rule, t=t, smooth=smooth,
                          estnoise=None if est is None else float(np.atleast_1d(est)[i % np.size(est)])) for i in range(len(tabs))]
    return np.stack(out, axis=1)


def _sigma(oracle, tabs, trees):
    return np.array([oracle.noisest(tabs[i], True, trees[:, i]) for i in range(len(tabs))])


def _f(wx, transform):
    return wx.swpd_denoiseall if transform == "swpd" else wx.acwpd_denoiseall


def _check(wx, got, want, dtype, what):
    got = wx.to_numpy(got)
    assert got.shape == want.shape and got.dtype == np.dtype(dtype)
    err = max(helpers.relerr(got[:, i], want[:, i]) for i in range(want.shape[1]))
    print("%s: error %.3g" % (what, err))
    assert err <= _bound(dtype), (what, err)


@pytest.mark.parametrize("transform,case", SIG_CASES)
def test_float64_against_the_oracle(wx, oracle, transform, case):
    n, L, B, filt, _ = case
    x, trees, tabs = _case(wx, oracle, transform, n, L, B, filt)
    wt = cases.wavelet(wx, filt)
    t = float(np.sqrt(2 * np.log(n)))
    xd = wx.to_device(x, "cuda:0")
    sg = wx.to_numpy(wx.red_noisestall(xd, wt, trees, L, transform))
    assert wx.red_bb_route() == FUSED
    so = _sigma(oracle, tabs, trees)
    serr = np.abs(sg - so).max() / np.abs(so).max()
    print("%s n = %d L = %d %s: sigma error %.3g" % (transform, n, L, filt, serr))
    assert serr <= _bound(np.float64)
    rules = RULES if (n == 256 and filt == "db4") else RULES[:2]
    for rule in rules:
        for smooth in ("regular", "undersmooth"):
            got = _f(wx, transform)(xd, wt, trees, L, wx.VisuShrink(_th(wx, rule), t), smooth=smooth)
            assert wx.red_bb_route() == FUSED
            _check(wx, got, _oracle(wx, oracle, transform, tabs, trees, filt, rule, t, smooth), np.float64,
                   "%s n = %d L = %d %s %s %s" % (transform, n, L, filt, rule, smooth))
    assert wx.to_numpy(xd).tobytes() == x.tobytes()                   # the input is unchanged
    # undersmooth with every leaf zeroed: the inverse of the coarsest scaling column alone
    big = 1e30
    got = _f(wx, transform)(xd, wt, trees, L, wx.VisuShrink(wx.HardTH(), big), smooth="undersmooth")
    want = _oracle(wx, oracle, transform, tabs, trees, filt, "hard", big, "undersmooth")
    dec = np.flatnonzero(trees[0])
    assert dec.size
    _check(wx, wx.to_numpy(got)[:, dec], want[:, dec], np.float64, "%s n = %d every leaf zeroed" % (transform, n))


@pytest.mark.parametrize("case", [c for c in cases.F32_CASES if c[4] == "shannon"])
def test_float32_stationary_soft(wx, oracle, case):
    """SoftTH only: continuous in the coefficients"""
    n, L, B, filt, _ = case
    x, trees, tabs = _case(wx, oracle, "swpd", n, L, B, filt, np.float32)
    t = float(np.sqrt(2 * np.log(n)))
    for smooth in ("regular", "undersmooth"):
        got = wx.swpd_denoiseall(wx.to_device(x, "cuda:0"), cases.wavelet(wx, filt), trees, L, wx.VisuShrink(wx.SoftTH(), t), smooth=smooth)
        assert wx.red_bb_route() == FUSED
        _check(wx, got, _oracle(wx, oracle, "swpd", tabs, trees, filt, "soft", t, smooth), np.float32, "f32 n = %d L = %d %s %s" % (n, L, filt, smooth))


@pytest.mark.parametrize("transform", ["swpd", "acwpd"])
def test_thresholds_given_and_best_threshold(wx, oracle, transform):
    n, L, B, filt = 256, 8, 12, "db4"
    x, trees, tabs = _case(wx, oracle, transform, n, L, B, filt)
    wt = cases.wavelet(wx, filt)
    t = float(np.sqrt(2 * np.log(n)))
    dnt = wx.VisuShrink(wx.HardTH(), t)
    f = _f(wx, transform)
    xd = wx.to_device(x, "cuda:0")
    N = x.shape[1]
    for est in (0.9, np.linspace(0.7, 1.3, N)):
        got = f(xd, wt, trees, L, dnt, estnoise=est)
        assert wx.red_bb_route() == FUSED
        _check(wx, got, _oracle(wx, oracle, transform, tabs, trees, filt, "hard", t, "regular", est=est), np.float64, "%s thr given" % transform)
    sg = wx.to_numpy(wx.red_noisestall(xd, wt, trees, L, transform))
    by_hand = f(xd, wt, trees, L, dnt, estnoise=float(np.median(sg)))
    best = f(xd, wt, trees, L, dnt, bestTH=np.median)
    assert wx.to_numpy(best).tobytes() == wx.to_numpy(by_hand).tobytes()


@pytest.mark.parametrize("transform,dtype", [("swpd", np.float64), ("swpd", np.float32), ("acwpd", np.float64)])
def test_input_forms_and_repeats_are_byte_identical(wx, oracle, transform, dtype):
    import torch
    n, L, B, filt = 64, 6, 24, "db4"
    x, trees, _ = _case(wx, oracle, transform, n, L, B, filt, dtype)
    wt = cases.wavelet(wx, filt)
    f = _f(wx, transform)
    xd = wx.to_device(x, "cuda:0")
    ref = f(x, wt, trees, L)                                          # numpy signals, host trees
    assert isinstance(ref, np.ndarray) and wx.red_bb_route() == FUSED
    tb = torch.from_numpy(np.ascontiguousarray(trees)).to("cuda:0")
    for tr in (trees, tb, tb.to(torch.uint8), tb):
        got = f(xd, wt, tr, L)
        assert wx.red_bb_route() == FUSED
        assert wx.to_numpy(got).tobytes() == np.asfortranarray(ref).tobytes()
    sg = wx.red_noisestall(x, wt, trees, L, transform)
    assert wx.to_numpy(wx.red_noisestall(xd, wt, tb, L, transform)).tobytes() == np.asarray(sg).tobytes()


@pytest.mark.parametrize("transform", ["swpd", "acwpd"])
def test_bestbasis_denoiseall_is_the_composition(wx, transform):
    n, L, B = 256, 8, 12
    x = np.asfortranarray(cases.signals(n, L, B))
    wt = cases.wavelet(wx, "db4")
    xd = wx.to_device(x, "cuda:0")
    M = cases.entry(wx, transform)(xd, wt, L, device=True)
    by_hand = _f(wx, transform)(xd, wt, M, L, smooth="undersmooth")
    got = wx.bestbasis_denoiseall(xd, wt, L, transform, smooth="undersmooth")
    assert wx.to_numpy(got).tobytes() == wx.to_numpy(by_hand).tobytes()
    host = wx.bestbasis_denoiseall(x, wt, L, transform, smooth="undersmooth")          # numpy signals
    assert isinstance(host, np.ndarray) and np.asfortranarray(host).tobytes() == wx.to_numpy(got).tobytes()


@pytest.mark.parametrize("transform,n,L,B,filt", [("swpd", 64, 6, 24, "rand22"), ("acwpd", 64, 6, 24, "rand22"), ("swpd", 2048, 4, 4, "db4"),
                                                  ("swpd", 1024, 10, 4, "db4"), ("acwpd", 1024, 10, 4, "db4")])
def test_outside_the_window(wx, oracle, transform, n, L, B, filt):
    """22 taps, n = 2048 (the estimate's registers) and Float64 n = 1024 at depth 10 (20 columns of 8 KiB): chunks through the table
    entries, the same bound"""
    x, trees, tabs = _case(wx, oracle, transform, n, L, B, filt)
    t = float(np.sqrt(2 * np.log(n)))
    got = _f(wx, transform)(wx.to_device(x, "cuda:0"), cases.wavelet(wx, filt), trees, L, wx.VisuShrink(wx.SoftTH(), t))
    assert wx.red_bb_route() == CHUNKED
    _check(wx, got, _oracle(wx, oracle, transform, tabs, trees, filt, "soft", t, "regular"), np.float64, "%s n = %d L = %d %s route 2" % (transform, n, L, filt))
    sg = wx.to_numpy(wx.red_noisestall(x, cases.wavelet(wx, filt), trees, L, transform))
    so = _sigma(oracle, tabs, trees)
    assert np.abs(sg - so).max() / np.abs(so).max() <= _bound(np.float64)


@pytest.mark.parametrize("transform", ["swpd", "acwpd"])
def test_depth_zero_thresholds_the_signal(wx, oracle, transform):
    n, B = 64, 5
    x = np.asfortranarray(cases.signals(64, 6, 24)[:, :B])
    trees = np.zeros((n - 1, B), dtype=bool)
    t = float(np.sqrt(2 * np.log(n)))
    got = _f(wx, transform)(x, cases.wavelet(wx, "db4"), trees, 0, wx.VisuShrink(wx.HardTH(), t))
    assert wx.red_bb_route() == TRIVIAL
    want = np.stack([oracle.denoise(np.asfortranarray(x[:, i:i + 1]), transform, cases.qmf(wx, "db4"), tree=trees[:, i], th="hard", t=t)
                     for i in range(B)], axis=1)
    _check(wx, got, want, np.float64, "%s L = 0" % transform)


@pytest.mark.parametrize("transform", ["swpd", "acwpd"])
def test_a_tree_deeper_than_L_is_refused(wx, transform):
    import torch
    n, L, B = 64, 3, 6
    x = wx.to_device(np.asfortranarray(cases.signals(64, 6, 24)[:, :B]), "cuda:0")
    trees = np.repeat(_shapes(n, L)[:, 1:2], B, axis=1)
    trees[(1 << L) - 1, 4] = True                                     # node 2^L, depth L, decomposed in column 4
    wt = cases.wavelet(wx, "db4")
    for tr in (trees, torch.from_numpy(trees).to("cuda:0")):
        with pytest.raises(IndexError):
            _f(wx, transform)(x, wt, tr, L)
        assert wx.red_bb_route() == 0
    # through the C entry: nothing is written
    from waveletsext_jl_amd import _lib
    import ctypes
    out = torch.full((B, n), -7.25, dtype=torch.float64, device="cuda:0")
    sig = torch.full((B,), -7.25, dtype=torch.float64, device="cuda:0")
    q = np.ascontiguousarray(wt.qmf, dtype=np.float64)
    tb = np.asfortranarray(trees).view(np.uint8)
    P = ctypes.c_void_p
    fn = getattr(_lib.lib(), "wx_denoise_%s1d_sig_trees_f64" % transform)
    xs = x.t().contiguous()
    rc = fn(P(xs.data_ptr()), P(out.data_ptr()), n, L, P(tb.ctypes.data), n - 1, B, P(q.ctypes.data), q.size, 0, 1.0, P(0), 0, 0,
            P(sig.data_ptr()), P(0))
    torch.cuda.synchronize()
    assert rc == _lib.WX_EBOUNDS
    assert (out == -7.25).all() and (sig == -7.25).all()


@pytest.mark.parametrize("transform,dtype", [("swpd", np.float64), ("swpd", np.float32), ("acwpd", np.float64)])
def test_batch_striding(wx, oracle, transform, dtype):
    """n = 8: four full rounds of the launch grid plus one signal, the case's columns repeated: every repeat carries the same bytes,
    and the distinct columns are the oracle's"""
    from waveletsext_jl_amd import _lib
    n, L, B, filt = 8, 3, 24, "db4"
    x, trees, tabs = _case(wx, oracle, transform, n, L, B, filt, dtype)
    M = x.shape[1]
    grid = _lib.red_bb_grid(n, L, 8, np.dtype(dtype).itemsize, transform == "acwpd", 1, 10 ** 6)
    assert grid > 0
    N = 4 * grid + 1
    idx = np.arange(N) % M
    t = float(np.sqrt(2 * np.log(n)))
    got = _f(wx, transform)(wx.to_device(np.asfortranarray(x[:, idx]), "cuda:0"), cases.wavelet(wx, filt), np.asfortranarray(trees[:, idx]), L,
                            wx.VisuShrink(wx.SoftTH(), t))
    assert wx.red_bb_route() == FUSED
    got = wx.to_numpy(got)
    _check(wx, got[:, :M], _oracle(wx, oracle, transform, tabs, trees, filt, "soft", t, "regular"), dtype, "%s striding" % transform)
    assert np.asfortranarray(got).tobytes() == np.asfortranarray(got[:, idx]).tobytes()


def _abi(wx, transform, xd, trees, wt, L, rule, t, smooth="regular", thr=None, want_out=True, want_sigma=True):
    """the C entry with the signals, both outputs and the thresholds in device memory, host trees: (xhat | None, sigma | None, route)"""
    import ctypes

    import torch
    from waveletsext_jl_amd import _lib
    P = ctypes.c_void_p
    n, N = xd.shape
    dt = xd.dtype
    out = torch.full((N, n), -7.25, dtype=dt, device=xd.device)       # column-major (n, N)
    sig = torch.full((N,), -7.25, dtype=dt, device=xd.device)
    q = np.ascontiguousarray(wt.qmf, dtype=np.float64)
    tb = np.asfortranarray(trees).view(np.uint8)
    xs = xd.t().contiguous()
    fn = getattr(_lib.lib(), "wx_denoise_%s1d_sig_trees_%s" % (transform, "f32" if dt == torch.float32 else "f64"))
    rc = fn(P(xs.data_ptr()), P(out.data_ptr() if want_out else 0), n, L, P(tb.ctypes.data), n - 1, N, P(q.ctypes.data), q.size,
            RULES.index(rule), float(t), P(0 if thr is None else thr.data_ptr()), 0 if thr is None else thr.numel(),
            1 if smooth == "undersmooth" else 0, P(sig.data_ptr() if want_sigma else 0), P(torch.cuda.current_stream().cuda_stream))
    assert rc == 0, _lib.lib().wx_last_error()
    route = wx.red_bb_route()
    torch.cuda.synchronize()
    if not want_sigma:
        assert (sig == -7.25).all()
    return (out.cpu().numpy().T if want_out else None), (sig.cpu().numpy() if want_sigma else None), route


@pytest.mark.parametrize("transform,dtype,n,L,B,filt,route", [
    ("swpd", np.float64, 256, 8, 12, "db4", FUSED), ("swpd", np.float32, 256, 8, 12, "db4", FUSED), ("acwpd", np.float64, 256, 8, 12, "db4", FUSED),
    ("swpd", np.float64, 8, 3, 24, "db4", FUSED),
    ("swpd", np.float64, 64, 6, 24, "rand22", CHUNKED), ("swpd", np.float32, 64, 6, 24, "rand22", CHUNKED),
    ("acwpd", np.float64, 64, 6, 24, "rand22", CHUNKED), ("swpd", np.float64, 1024, 10, 4, "db4", CHUNKED)])
def test_xhat_and_sigma_in_one_call(wx, oracle, transform, dtype, n, L, B, filt, route):
    """out and sigma both given, through the C entry: sigma is red_noisestall's byte for byte, out is the call's without sigma; with the
    thresholds given (one, or one per signal) sigma receives them, and out is that of the call without sigma"""
    import torch
    x, trees, _ = _case(wx, oracle, transform, n, L, B, filt, dtype)
    wt = cases.wavelet(wx, filt)
    t = float(np.sqrt(2 * np.log(n)))
    xd = wx.to_device(x, "cuda:0")
    N = x.shape[1]
    alone = wx.to_numpy(wx.red_noisestall(xd, wt, trees, L, transform))
    assert wx.red_bb_route() == route and np.isfinite(alone).all() and (alone > 0).any()
    for smooth in ("regular", "undersmooth"):
        out, sig, r = _abi(wx, transform, xd, trees, wt, L, "hard", t, smooth)
        assert r == route
        assert sig.dtype == np.dtype(dtype) and sig.tobytes() == alone.tobytes()
        only, none, r = _abi(wx, transform, xd, trees, wt, L, "hard", t, smooth, want_sigma=False)
        assert r == route and none is None
        assert np.ascontiguousarray(out).tobytes() == np.ascontiguousarray(only).tobytes()
        py = wx.to_numpy(_f(wx, transform)(xd, wt, trees, L, wx.VisuShrink(wx.HardTH(), t), smooth=smooth))
        assert np.ascontiguousarray(out).tobytes() == np.ascontiguousarray(py).tobytes()
    nothing, sig, r = _abi(wx, transform, xd, trees, wt, L, "hard", t, want_out=False)
    assert r == route and nothing is None and sig.tobytes() == alone.tobytes()
    for thr in (np.array([0.9], dtype=dtype), np.linspace(0.7, 1.3, N).astype(dtype)):
        td = torch.from_numpy(thr).to("cuda:0")
        out, sig, r = _abi(wx, transform, xd, trees, wt, L, "soft", t, thr=td)
        assert r == route
        assert sig.tobytes() == np.broadcast_to(thr, (N,)).astype(dtype).tobytes()     # the thresholds used, before scaling
        only, _, r = _abi(wx, transform, xd, trees, wt, L, "soft", t, thr=td, want_sigma=False)
        assert np.ascontiguousarray(out).tobytes() == np.ascontiguousarray(only).tobytes()
        py = wx.to_numpy(_f(wx, transform)(xd, wt, trees, L, wx.VisuShrink(wx.SoftTH(), t), estnoise=thr if thr.size > 1 else float(thr[0])))
        assert np.ascontiguousarray(out).tobytes() == np.ascontiguousarray(py).tobytes()
