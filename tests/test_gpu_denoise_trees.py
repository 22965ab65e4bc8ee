"""denoiseall(xw, "wpt", wt, tree=M) with M an (n - 1, N) matrix -- one tree per signal, every signal denoised in its own basis
(csrc/wx_denoise_trees.hip) -- against the oracle called per signal with that signal's tree: the noise estimates bit for bit, the
output within the bound of tests/test_gpu_denoise.py; host trees and device trees byte for byte; `wx.wpt_trees_route()` after every call.

Coefficients: standard normal with max(2, n // 16) entries per column times 50, the same bits to the library and to the oracle.  With
identical bits and an exact sigma no Hard decision can flip.  Eleven trees per case (bare root, full, :dwt, left-deep L - 1, right-deep L,
six random ones); the column stride n - 1 is odd, so the columns start at every byte alignment.  Sizes: 8 (the smallest the kernel
takes), 64 (one wavefront's pairs, 256 lanes launched), 1024 (512 lanes), 8192 Float64 / 16384 Float32 (1024 lanes, the LDS limit)."""
import ctypes

import numpy as np
import pytest

import helpers

pytestmark = pytest.mark.gpu

LDS, SINGLE, COPIED, HOST = "device prep + lds kernel", "device prep + single tree", "device trees copied to host", "host trees"
RULES = ("hard", "soft", "semisoft", "stein")
SMOOTH = ("regular", "undersmooth")


def _log2(n):
    return int(n).bit_length() - 1


def _limit(dtype):
    return 8192 if dtype == np.float64 else 16384


def _deep(n, depth, right):
    """the chain root -> left (right) child -> ... decomposed `depth` times"""
    t = np.zeros(n - 1, dtype=bool)
    node = 1
    for _ in range(depth):
        t[node - 1] = True
        node = 2 * node + (1 if right else 0)
    return t


def _trees11(wx, n, rng, extra=6):
    """[bare root, full, :dwt, left-deep L - 1, right-deep L, random p = 0.3, 0.7, 0.9, 0.3, 0.7, 0.9 (, ...)], all different"""
    L = _log2(n)
    cols = [np.zeros(n - 1, dtype=bool), wx.maketree(n, L, "full"), wx.maketree(n, L, "dwt"), _deep(n, L - 1, False), _deep(n, L, True)]
    seen = {c.tobytes() for c in cols}
    for i in range(extra):
        p = (0.3, 0.7, 0.9)[i % 3]
        t = helpers.random_tree_1d(n, rng, p)
        while t.tobytes() in seen or not t[0]:
            t = helpers.random_tree_1d(n, rng, p)
        seen.add(t.tobytes())
        cols.append(t)
    trees = np.asfortranarray(np.stack(cols, axis=1))
    assert len({trees[:, i].tobytes() for i in range(trees.shape[1])}) == trees.shape[1]
    assert all(wx.isvalidtree(np.zeros(n), trees[:, i]) for i in range(trees.shape[1]))
    return trees


def _coefs(n, B, rng, dtype):
    c = rng.standard_normal((n, B))
    for i in range(B):
        c[rng.choice(n, size=max(2, n // 16), replace=False), i] *= 50.0
    return np.asfortranarray(c.astype(dtype))


def _dev(wx, trees, dtype=np.bool_):
    return wx.to_device(np.asfortranarray(trees.astype(dtype)))


def _bytes(wx, a):
    return wx.to_numpy(a).tobytes()


def _th(wx, rule):
    return {"hard": wx.HardTH, "soft": wx.SoftTH, "semisoft": wx.SemiSoftTH, "stein": wx.SteinTH}[rule]()


def _oracle_sigma(oracle, c, trees):
    return np.array([oracle.noisest(c[:, i], False, trees[:, i]) for i in range(trees.shape[1])], dtype=c.dtype)


def _oracle_denoise(oracle, c, qmf, trees, rule, t, smooth, est=None):
    return np.stack([oracle.denoise(c[:, i], "wpt", qmf, tree=trees[:, i], th=rule, t=t, smooth=smooth,
                                    estnoise=None if est is None else float(est[i])) for i in range(trees.shape[1])], axis=-1)


def _same_sigma(got, want):
    """bit for bit, NaN matching NaN"""
    got, want = np.asarray(got), np.asarray(want)
    return got.dtype == want.dtype and got.shape == want.shape and bool(((got == want) | (np.isnan(got) & np.isnan(want))).all())


def _condition(oracle, c, trees, sigma):
    """on the oracle's result alone: at least 5 of the 11 estimates are non-zero, and for n >= 64 every such column has zeroed and kept
    coefficients under HardTH with t = sqrt(2 log n) -- a case in which every decision goes one way would check no threshold"""
    n = c.shape[0]
    nz = np.flatnonzero(sigma != 0)
    assert nz.size >= 5, sigma
    if n >= 64:
        for i in nz:
            o = oracle.denoise(c[:, i], "wpt", None, tree=trees[:, i], th="hard", t=float(np.sqrt(2 * np.log(n))), smooth="regular")
            assert (o == 0).any() and (o != 0).any(), i


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("wname", ["haar", "db4", "db10"])
@pytest.mark.parametrize("n", [8, 64, 1024, "limit"])
def test_parity_with_the_oracle_per_signal(wx, oracle, n, wname, dtype):
    """four rules x two smooth values at n = 64, the diagonal (rule i with smooth i mod 2) elsewhere"""
    import torch
    n = _limit(dtype) if n == "limit" else n
    rng = np.random.default_rng(5 * n)
    trees = _trees11(wx, n, rng)
    B = trees.shape[1]
    assert B == 11
    c = _coefs(n, B, rng, dtype)
    wt = wx.wavelet(wname)
    tol = 20 * helpers.TOL[np.dtype(dtype)]
    sigma = _oracle_sigma(oracle, c, trees)
    _condition(oracle, c, trees, sigma)
    cd, td = wx.to_device(c), _dev(wx, trees)
    for tr, route in ((td, LDS), (trees, HOST)):
        s = wx.noisestall(cd, False, tr)
        assert wx.wpt_trees_route() == route
        assert isinstance(s, torch.Tensor) and s.is_cuda and tuple(s.shape) == (B,)
        got = wx.to_numpy(s)
        print("sigma", got, sigma)
        assert _same_sigma(got, sigma)
    t = float(np.sqrt(2 * np.log(n)))
    combos = [(r, s) for r in RULES for s in SMOOTH] if n == 64 else [(r, SMOOTH[i % 2]) for i, r in enumerate(RULES)]
    for rule, smooth in combos:
        dnt = wx.VisuShrink(_th(wx, rule), t)
        d = wx.denoiseall(cd, "wpt", wt, tree=td, dnt=dnt, smooth=smooth)
        assert wx.wpt_trees_route() == LDS
        h = wx.denoiseall(cd, "wpt", wt, tree=trees, dnt=dnt, smooth=smooth)
        assert wx.wpt_trees_route() == HOST
        assert isinstance(d, torch.Tensor) and d.is_cuda and tuple(d.shape) == (n, B)
        want = _oracle_denoise(oracle, c, wt.qmf, trees, rule, t, smooth)
        e = helpers.relerr(wx.to_numpy(d), want)
        print(rule, smooth, "against the oracle", e)
        assert e <= tol, (rule, smooth)
        assert _bytes(wx, d) == _bytes(wx, h), (rule, smooth, "device trees and host trees differ")
        if smooth == "undersmooth":                                    # the bare root: no scaling range to spare, nothing thresholded, no transform
            assert wx.to_numpy(d)[:, 0].tobytes() == c[:, 0].tobytes()
    assert _bytes(wx, cd) == c.tobytes()                               # the input is not modified


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_finest_nodes_of_one_and_two_samples_and_equal_details(wx, oracle, dtype):
    n, L = 64, 6
    rng = np.random.default_rng(6)
    wt = wx.wavelet(wx.WT.db4)
    cols = [_deep(n, L, True), _deep(n, L - 1, True), _deep(n, L - 2, True), wx.maketree(n, L, "dwt"), wx.maketree(n, 1, "full"),
            np.zeros(n - 1, dtype=bool)]
    trees = np.asfortranarray(np.stack(cols, axis=1))
    c = _coefs(n, trees.shape[1], rng, dtype)
    c[n // 2:, 3] = 3.0                                                # all details equal: the deviations are all zero
    c[:, 5] = -1.5                                                     # the whole signal is the detail range, and constant
    sigma = _oracle_sigma(oracle, c, trees)
    assert sigma[0] == 0 and sigma[1] != 0 and sigma[2] != 0 and sigma[3] == 0 and sigma[4] != 0 and sigma[5] == 0
    cd = wx.to_device(c)
    assert _same_sigma(wx.to_numpy(wx.noisestall(cd, False, _dev(wx, trees))), sigma)
    assert wx.wpt_trees_route() == LDS
    t = float(np.sqrt(2 * np.log(n)))
    for rule, smooth in ((r, s) for r in RULES for s in SMOOTH):
        d = wx.denoiseall(cd, "wpt", wt, tree=_dev(wx, trees), dnt=wx.VisuShrink(_th(wx, rule), t), smooth=smooth)
        assert wx.wpt_trees_route() == LDS
        want = _oracle_denoise(oracle, c, wt.qmf, trees, rule, t, smooth)
        assert helpers.relerr(wx.to_numpy(d), want) <= 20 * helpers.TOL[np.dtype(dtype)], (rule, smooth)


def test_a_nan_poisons_its_own_signal_only_on_a_workgroup_that_takes_several(wx, oracle):
    """the construction of test_workgroups_take_several_signals_in_turn (tests/test_gpu_wpt_trees_device.py): n = 64, 3 * 4096 + 5 signals,
    a different tree every turn of a workgroup -- the kernel's grid is 2048 here (eight workgroups of 256 lanes on each of the 256 CUs), six or
    seven turns each.  One NaN inside one signal's detail range: that signal's estimate is NaN, everything else as without it."""
    n, grid = 64, 4096
    B = 3 * grid + 5
    rng = np.random.default_rng(64)
    wt = wx.wavelet(wx.WT.db4)
    pool = _trees11(wx, n, rng, extra=56)
    assert pool.shape[1] == 61
    b = np.arange(B)
    which = (b + b // grid) % 61
    assert (which[:-grid] != which[grid:]).all() and (which[:-2048] != which[2048:]).all()
    trees = np.asfortranarray(pool[:, which])
    c = _coefs(n, B, rng, np.float64)
    b0 = grid + 2048 + 7
    lo = oracle.finestdetailrange(n, trees[:, b0]) - 1                 # 0-based start of the detail range
    cn = c.copy(order="F")
    cn[lo + (n - lo) // 2, b0] = np.nan
    td = _dev(wx, trees)
    t = float(np.sqrt(2 * np.log(n)))
    dnt = wx.VisuShrink(wx.HardTH(), t)
    clean_s = wx.to_numpy(wx.noisestall(wx.to_device(c), False, td))
    assert wx.wpt_trees_route() == LDS
    sigma = _oracle_sigma(oracle, c, trees)
    assert _same_sigma(clean_s, sigma)
    clean = wx.to_numpy(wx.denoiseall(wx.to_device(c), "wpt", wt, tree=td, dnt=dnt))
    assert wx.wpt_trees_route() == LDS
    pois_s = wx.to_numpy(wx.noisestall(wx.to_device(cn), False, td))
    pois = wx.to_numpy(wx.denoiseall(wx.to_device(cn), "wpt", wt, tree=td, dnt=dnt))
    assert np.isnan(pois_s[b0]) and np.isnan(oracle.noisest(cn[:, b0], False, trees[:, b0]))
    others = np.ones(B, dtype=bool)
    others[b0] = False
    assert (pois_s[others] == clean_s[others]).all()
    assert pois[:, others].tobytes() == clean[:, others].tobytes()
    pick = np.unique(np.concatenate([np.arange(0, B, 97), b0 + 2048 * np.arange(-3, 4), [B - 1]]))
    pick = pick[(pick >= 0) & (pick < B) & (pick != b0)]
    want = _oracle_denoise(oracle, c[:, pick], wt.qmf, trees[:, pick], "hard", t, "regular")
    assert helpers.relerr(clean[:, pick], want) <= 20 * helpers.TOL[np.dtype(np.float64)]
    host = wx.denoiseall(wx.to_device(c), "wpt", wt, tree=trees, dnt=dnt)
    assert wx.wpt_trees_route() == HOST
    assert wx.to_numpy(host).tobytes() == clean.tobytes()


# ---- estnoise and the options --------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_estnoise_forms_besth_and_no_filter(wx, oracle, dtype):
    n = 256
    rng = np.random.default_rng(5 * n)
    trees = _trees11(wx, n, rng)
    B = trees.shape[1]
    c = _coefs(n, B, rng, dtype)
    wt = wx.wavelet(wx.WT.db4)
    tol = 20 * helpers.TOL[np.dtype(dtype)]
    cd, td = wx.to_device(c), _dev(wx, trees)
    t = float(np.sqrt(2 * np.log(n)))
    sigma = _oracle_sigma(oracle, c, trees)
    # noisestall with a matrix is noisest per signal
    per = np.array([wx.noisest(c[:, i], False, trees[:, i]) for i in range(B)], dtype=dtype)
    assert _same_sigma(wx.to_numpy(wx.noisestall(cd, False, td)), per) and _same_sigma(per, sigma)
    assert _same_sigma(wx.noisestall(c, False, trees), sigma)          # host arrays in, host array out
    one = wx.to_numpy(wx.noisestall(cd, False, trees[:, 6]))           # a single tree goes where it went: wx_noisest_*
    assert _same_sigma(one, np.array([oracle.noisest(c[:, i], False, trees[:, 6]) for i in range(B)], dtype=dtype))
    for rule, smooth in (("soft", "regular"), ("hard", "undersmooth")):
        dnt = wx.VisuShrink(_th(wx, rule), t)
        # numbers, one per signal
        est = (0.5 + rng.random(B)).astype(dtype)
        d = wx.denoiseall(cd, "wpt", wt, tree=td, dnt=dnt, estnoise=est, smooth=smooth)
        assert wx.wpt_trees_route() == LDS
        assert helpers.relerr(wx.to_numpy(d), _oracle_denoise(oracle, c, wt.qmf, trees, rule, t, smooth, est)) <= tol
        # relerrorthreshold: all coefficients of the signal, whatever its tree
        thr = np.asarray(wx.relerrorthresholdall(cd), dtype=dtype)
        d = wx.denoiseall(cd, "wpt", wt, tree=td, dnt=dnt, estnoise=wx.relerrorthreshold, smooth=smooth)
        assert wx.wpt_trees_route() == LDS
        assert helpers.relerr(wx.to_numpy(d), _oracle_denoise(oracle, c, wt.qmf, trees, rule, t, smooth, thr)) <= tol
        # one summary threshold for the batch
        m = np.full(B, np.mean(sigma.astype(np.float64))).astype(dtype)
        d = wx.denoiseall(cd, "wpt", wt, tree=td, dnt=dnt, bestTH=np.mean, smooth=smooth)
        assert wx.wpt_trees_route() == LDS
        assert helpers.relerr(wx.to_numpy(d), _oracle_denoise(oracle, c, wt.qmf, trees, rule, t, smooth, m)) <= tol
        # wt = None: the thresholded coefficients, no transform -- the same arithmetic as the oracle's, element by element
        d = wx.denoiseall(cd, "wpt", None, tree=td, dnt=dnt, smooth=smooth)
        assert wx.wpt_trees_route() == LDS
        want = _oracle_denoise(oracle, c, None, trees, rule, t, smooth)
        assert helpers.relerr(wx.to_numpy(d), want) <= tol
        if rule == "hard":
            assert (wx.to_numpy(d) == want).all()
        # one signal, a matrix of one column
        one = wx.denoise(wx.to_device(c[:, 7].copy()), "wpt", wt, tree=_dev(wx, trees[:, 7:8]), dnt=dnt, smooth=smooth)
        assert helpers.relerr(wx.to_numpy(one), _oracle_denoise(oracle, c[:, 7:8], wt.qmf, trees[:, 7:8], rule, t, smooth)[:, 0]) <= tol


@pytest.mark.parametrize("same", [False, True])
def test_given_thresholds_in_device_memory_come_back_in_sigma(wx, same):
    """through the C ABI: thr as a device vector of 1 or B values, sigma receives the thresholds used before scaling -- from the kernel
    (different trees) and from the single-tree route (identical columns)"""
    import torch
    n, B = 64, 11
    rng = np.random.default_rng(65)
    wt = wx.wavelet(wx.WT.db4)
    trees = _trees11(wx, n, rng)
    if same:
        trees = np.asfortranarray(np.repeat(trees[:, 7:8], B, axis=1))
    td = _dev(wx, trees, np.uint8)
    cd = wx.to_device(_coefs(n, B, rng, np.float64))
    lib = wx._lib.lib()
    q = np.ascontiguousarray(wt.qmf, dtype=np.float64)
    P, L64, I, D = ctypes.c_void_p, ctypes.c_int64, ctypes.c_int, ctypes.c_double
    st = P(torch.cuda.current_stream().cuda_stream)
    dnt = wx.VisuShrink(wx.SoftTH(), 1.75)
    for nthr in (1, B):
        est = 0.5 + rng.random(nthr)
        thr = torch.from_numpy(est).to("cuda")
        out = wx.jl_empty((n, B), torch.float64, "cuda")
        sig = torch.full((B,), -7.25, dtype=torch.float64, device="cuda")
        rc = lib.wx_denoise_wpt1d_trees_f64(P(cd.data_ptr()), P(out.data_ptr()), L64(n), P(td.data_ptr()), L64(n - 1), L64(B), P(q.ctypes.data),
                                            I(q.size), I(1), D(1.75), P(thr.data_ptr()), L64(nthr), I(1), P(sig.data_ptr()), st)
        assert rc == 0 and wx.wpt_trees_route() == (SINGLE if same else LDS)
        assert (sig.cpu().numpy() == np.broadcast_to(est, (B,))).all()
        want = wx.denoiseall(cd, "wpt", wt, tree=td, dnt=dnt, estnoise=np.broadcast_to(est, (B,)), smooth="undersmooth")
        assert _bytes(wx, out) == _bytes(wx, want)


# ---- the other routes -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_identical_columns_equal_the_single_tree_call(wx, dtype):
    n, B = 256, 9
    rng = np.random.default_rng(9)
    wt = wx.wavelet(wx.WT.db4)
    tree = helpers.random_tree_1d(n, rng, 0.8)
    assert tree[0]
    M = np.asfortranarray(np.repeat(tree[:, None], B, axis=1))
    cd = wx.to_device(_coefs(n, B, rng, dtype))
    for smooth in SMOOTH:
        want = wx.denoiseall(cd, "wpt", wt, tree=tree, smooth=smooth)
        got = wx.denoiseall(cd, "wpt", wt, tree=_dev(wx, M), smooth=smooth)
        assert wx.wpt_trees_route() == SINGLE
        assert _bytes(wx, got) == _bytes(wx, want)
        got = wx.denoiseall(cd, "wpt", wt, tree=M, smooth=smooth)
        assert wx.wpt_trees_route() == HOST
        assert _bytes(wx, got) == _bytes(wx, want)
    assert _bytes(wx, wx.noisestall(cd, False, _dev(wx, M))) == _bytes(wx, wx.noisestall(cd, False, tree))
    assert wx.wpt_trees_route() == SINGLE


def test_outside_the_window(wx, oracle):
    """n = 16384 Float64 is longer than the LDS holds: the matrix is copied to the host once and the single-tree entries run per signal"""
    n, dtype = 16384, np.float64
    rng = np.random.default_rng(n)
    L = _log2(n)
    trees = np.asfortranarray(np.stack([helpers.random_tree_1d(n, rng, 0.8) | wx.maketree(n, 2, "full"), _deep(n, L - 1, False),
                                        _deep(n, L - 3, True)], axis=1))
    c = _coefs(n, 3, rng, dtype)
    wt = wx.wavelet(wx.WT.db4)
    cd = wx.to_device(c)
    t = float(np.sqrt(2 * np.log(n)))
    sigma = _oracle_sigma(oracle, c, trees)
    assert (sigma != 0).all()
    assert _same_sigma(wx.to_numpy(wx.noisestall(cd, False, _dev(wx, trees))), sigma)
    assert wx.wpt_trees_route() == COPIED
    for rule, smooth in (("hard", "undersmooth"), ("soft", "regular")):
        dnt = wx.VisuShrink(_th(wx, rule), t)
        d = wx.denoiseall(cd, "wpt", wt, tree=_dev(wx, trees), dnt=dnt, smooth=smooth)
        assert wx.wpt_trees_route() == COPIED
        h = wx.denoiseall(cd, "wpt", wt, tree=trees, dnt=dnt, smooth=smooth)
        assert wx.wpt_trees_route() == HOST
        assert _bytes(wx, d) == _bytes(wx, h)
        assert helpers.relerr(wx.to_numpy(d), _oracle_denoise(oracle, c, wt.qmf, trees, rule, t, smooth)) <= 20 * helpers.TOL[np.dtype(dtype)]


@pytest.mark.parametrize("where", ["device", "host"])
def test_an_invalid_tree_raises_and_leaves_the_outputs_untouched(wx, where):
    import torch
    n, B = 64, 9
    rng = np.random.default_rng(14)
    wt = wx.wavelet(wx.WT.db4)
    bad = np.asfortranarray(_trees11(wx, n, rng)[:, :B].copy())
    bad[:, 8] = False
    bad[0, 8] = True
    bad[62, 8] = True                                                  # node 63, the last byte of the matrix, under a cleared parent
    tr = _dev(wx, bad, np.uint8) if where == "device" else bad.astype(np.uint8, order="F")
    cd = wx.to_device(_coefs(n, B, rng, np.float64))
    with pytest.raises(AssertionError, match="isvalidtree"):
        wx.denoiseall(cd, "wpt", wt, tree=tr)
    assert wx.wpt_trees_route() == "none"
    with pytest.raises(AssertionError, match="isvalidtree"):
        wx.noisestall(cd, False, tr)
    lib = wx._lib.lib()
    q = np.ascontiguousarray(wt.qmf, dtype=np.float64)
    out = wx.jl_empty((n, B), torch.float64, "cuda")
    out.fill_(-7.25)
    sig = torch.full((B,), -7.25, dtype=torch.float64, device="cuda")
    P, L64, I, D = ctypes.c_void_p, ctypes.c_int64, ctypes.c_int, ctypes.c_double
    tp = P(tr.data_ptr()) if where == "device" else P(tr.ctypes.data)
    rc = lib.wx_denoise_wpt1d_trees_f64(P(cd.data_ptr()), P(out.data_ptr()), L64(n), tp, L64(n - 1), L64(B), P(q.ctypes.data), I(q.size), I(0),
                                        D(2.0), P(0), L64(0), I(0), P(sig.data_ptr()), P(torch.cuda.current_stream().cuda_stream))
    assert rc == -1 and lib.wx_wpt_trees_last_route() == 0
    torch.cuda.synchronize()
    assert bool((out == -7.25).all()) and bool((sig == -7.25).all())


# ---- the chain ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_best_basis_to_denoised_signals_stays_on_the_device(wx, oracle, dtype):
    import torch
    n, B = 256, 33
    rng = np.random.default_rng(256)
    wt = wx.wavelet(wx.WT.db4)
    x = np.cumsum(rng.standard_normal((n, B)), axis=0) + 0.5 * rng.standard_normal((n, B))    # random walks: trees of many shapes
    xd = wx.to_device(np.asfortranarray(x.astype(dtype)))
    table = wx.wpdall(xd, wt)
    t = wx.bestbasistreeall(table, wx.BB(), device=True)
    assert isinstance(t, torch.Tensor) and t.is_cuda and tuple(t.shape) == (n - 1, B)
    y = wx.wptall(xd, wt, t)
    assert wx.wpt_trees_route() == LDS
    out = wx.denoiseall(y, "wpt", wt, tree=t, smooth="undersmooth")
    assert wx.wpt_trees_route() == LDS
    assert isinstance(y, torch.Tensor) and y.is_cuda and isinstance(out, torch.Tensor) and out.is_cuda and tuple(out.shape) == (n, B)
    host = t.cpu().numpy()
    assert len({host[:, i].tobytes() for i in range(B)}) > 1
    assert _bytes(wx, out) == _bytes(wx, wx.denoiseall(y, "wpt", wt, tree=host, smooth="undersmooth"))
    c = wx.to_numpy(y)
    want = _oracle_denoise(oracle, c, wt.qmf, host, "hard", float(np.sqrt(2 * np.log(n))), "undersmooth")
    assert helpers.relerr(wx.to_numpy(out), want) <= 20 * helpers.TOL[np.dtype(dtype)]
