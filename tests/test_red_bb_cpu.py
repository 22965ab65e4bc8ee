"""Redundant per-signal best basis and denoising straight from the signals (wx_swpd_bbtrees_*, wx_acwpd_bbtrees_f64,
wx_denoise_swpd1d_sig_trees_*, wx_denoise_acwpd1d_sig_trees_f64; swpd_bestbasistreeall, acwpd_bestbasistreeall, swpd_denoiseall,
acwpd_denoiseall, red_noisestall, bestbasis_denoiseall), the part that needs no GPU: the argument checks of the C ABI happen before a device is needed, the Python
layer refuses what bestbasistreeall refuses, the launch geometry answers without a device, and the seeded fixtures of the GPU tests
(tests/red_bb_cases.py) keep every split decision far enough from a tie that exact tree equality is a fair demand on a kernel whose
coefficients differ from the oracle's in the last bits."""
import ctypes

import numpy as np
import pytest

import red_bb_cases as cases

WX_OK, WX_EASSERT, WX_EARG, WX_EUNSUPPORTED = 0, -1, -2, -11


def _p(a):
    return ctypes.c_void_p(a.ctypes.data)


NULL = ctypes.c_void_p(0)


@pytest.fixture()
def entry(wx):
    from waveletsext_jl_amd import _lib
    L = _lib.lib()
    q = np.ascontiguousarray(wx.wavelet(wx.WT.db4).qmf, dtype=np.float64)
    return L, q


@pytest.mark.parametrize("name,dtype", [("wx_swpd_bbtrees_f64", np.float64), ("wx_swpd_bbtrees_f32", np.float32),
                                        ("wx_acwpd_bbtrees_f64", np.float64)])
def test_argument_errors_before_any_device(entry, name, dtype):
    L, q = entry
    fn = getattr(L, name)
    n, B = 16, 3
    x = np.zeros((B, n), dtype=dtype)
    trees = np.full((B, n - 1), 7, dtype=np.uint8)
    costs = np.full((B, 31), 7, dtype=dtype)

    def call(x_=_p(x), n_=n, L_=4, B_=B, q_=_p(q), F_=q.size, kind=0, t_=_p(trees), c_=_p(costs)):
        return fn(x_, n_, L_, B_, q_, F_, kind, t_, c_, NULL)

    route = L.wx_red_bb_last_route
    assert call(B_=0) == WX_OK and (trees == 7).all()            # no signals: nothing written
    assert route() == 3
    assert call(n_=12, L_=2) == WX_EASSERT                       # not dyadic
    assert route() == 0                                          # a refused call leaves no route behind
    assert call(B_=0) == WX_OK and route() == 3
    assert call(L_=5) == WX_EASSERT and route() == 0             # deeper than maxtransformlevels(16) = 4
    assert call(L_=-1) == WX_EASSERT
    assert call(B_=0) == WX_OK and route() == 3
    assert call(n_=0) == WX_EARG and route() == 0                # bad dimensions
    assert call(B_=-1) == WX_EARG
    assert call(x_=NULL) == WX_EARG
    assert call(q_=NULL) == WX_EARG
    assert call(t_=NULL) == WX_EARG
    assert call(kind=2) == WX_EARG
    assert call(kind=-1) == WX_EARG
    assert call(F_=5) == WX_EARG                                 # odd filter length
    assert call(n_=1 << 30, L_=3) == WX_EUNSUPPORTED
    assert route() == 0
    assert (trees == 7).all() and (costs == 7).all()
    assert L.wx_last_error().decode()


def test_debug_grid_windows(wx):
    """wx_debug_red_bb_grid asks the functions the launch calls, without a device: non-zero for every shape that must take the kernel,
    zero outside its window"""
    from waveletsext_jl_amd import _lib
    g = _lib.red_bb_grid
    for ac in (0, 1):
        for F in (2, 8, 20):
            for log2n in range(3, 10):                                # Float64: every depth up to n = 512
                for L in range(1, log2n + 1):
                    assert g(1 << log2n, L, F, 8, ac, 0, 1000) > 0, (log2n, L, F, ac)
            assert g(1024, 8, F, 8, ac, 0, 1000) > 0                  # and depth 8 at n = 1024
        assert g(64, 6, 22, 8, ac, 0, 200) == 0                       # 22 taps: the chunked route
        assert g(4096, 12, 8, 8, ac, 0, 2) == 0                       # 25 columns of 32 KiB
        assert g(64, 0, 8, 8, ac, 0, 5) == 0                          # L = 0: nothing is launched
        assert g(64, 7, 8, 8, ac, 0, 5) == 0
        assert g(64, 6, 8, 8, ac, 0, 0) == 0
    assert g(1024, 10, 8, 4, 0, 0, 1000) > 0                          # Float32 at depth 10
    assert g(1024, 10, 8, 8, 0, 0, 1000) == 0                         # Float64 at depth 10: 21 columns of 8 KiB
    assert g(1024, 10, 8, 4, 1, 0, 1000) == 0                         # the autocorrelation family is Float64 only
    assert g(64, 6, 8, 8, 0, 5, 10) == 0                              # no such kernel
    assert g(64, 6, 8, 8, 0, 0, 5) == 5                               # never more workgroups than signals
    assert g(1024, 8, 8, 8, 0, 0, 10 ** 6) == 256                     # 141.6 KiB of LDS: one workgroup per CU


def test_batch_striding_case_is_tied_to_the_launch_grid(wx):
    """the GPU case `four rounds of the grid plus one signal` takes its batch from GRID_8: that must be the grid the launch of an
    8-sample signal really uses"""
    from waveletsext_jl_amd import _lib
    for esz, ac in ((8, 0), (4, 0), (8, 1)):
        assert _lib.red_bb_grid(8, 3, 8, esz, ac, 0, 4 * cases.GRID_8 + 1) == cases.GRID_8


@pytest.mark.parametrize("transform", ["swpd", "acwpd"])
def test_python_layer_errors(wx, transform):
    f = cases.entry(wx, transform)
    x = np.zeros((16, 2))
    wt = wx.wavelet(wx.WT.db4)
    with pytest.raises(TypeError):
        f(x, wt, method=wx.BB())                                  # a redundant table takes BB(redundant=True)
    with pytest.raises(TypeError):
        f(x, wt, method=wx.BB(redundant=False))
    with pytest.raises(TypeError):
        f(x, wt, method=wx.JBB())
    with pytest.raises(TypeError):
        f(x, wt, method=wx.LSDB())
    with pytest.raises(TypeError):
        f(x, wt, device=True)                                     # device=True takes a device tensor
    with pytest.raises(AssertionError):
        f(x, wt, L=5)                                             # WX_EASSERT, before a device is needed
    with pytest.raises(AssertionError):
        f(np.zeros((12, 2)), wt, L=2)
    assert wx.red_bb_route() == 0
    t = f(np.zeros((16, 0)), wt)                                  # no signals: an empty matrix, no device needed
    assert t.shape == (15, 0) and t.dtype == np.bool_
    assert wx.red_bb_route() == 3
    t, c = f(np.zeros((16, 0)), wt, L=2, method=wx.BB(cost=wx.LogEnergyEntropyCost(), redundant=True), return_costs=True)
    assert t.shape == (15, 0) and c.shape == (7, 0) and c.dtype == np.float64


def test_autocorrelation_is_float64_only(wx):
    from waveletsext_jl_amd import _lib
    with pytest.raises(wx.WxError) as e:
        wx.acwpd_bestbasistreeall(np.zeros((16, 2), dtype=np.float32), wx.wavelet(wx.WT.db4))
    assert e.value.code == _lib.WX_EUNSUPPORTED
    t = wx.swpd_bestbasistreeall(np.zeros((16, 0), dtype=np.float32), wx.wavelet(wx.WT.db4))
    assert t.shape == (15, 0)


def test_decimated_entry_still_refuses_redundant(wx):
    with pytest.raises(TypeError):
        wx.wpd_bestbasistreeall(np.zeros((16, 2)), wx.wavelet(wx.WT.db4), method=wx.BB(redundant=True))


@pytest.mark.parametrize("transform", ["swpd", "acwpd"])
@pytest.mark.parametrize("n,L,B,filt,cost", cases.F64_CASES)
def test_fixture_guards(wx, oracle, transform, n, L, B, filt, cost):
    """on the oracle alone: every signal's closest split decision |cc - pc| / max(|cc|, |pc|) is at least 1e-8, four orders above what
    the last bits of a Float64 table move a cost by, and at least half of a case's trees decompose the root.
    At n = 8 the second demand cannot be met by this generator: three spikes of 20 .. 40 among eight samples are sparser in time than in
    any stationary packet, and the oracle decomposes 5 (haar) and 1 (db4) of the 24 stationary roots, 20 and 11 of the autocorrelation
    ones; 20 other seeds gave 0 .. 7, 0 .. 4, 10 .. 20 and 5 .. 11.  There the guard is what it protects against, a case whose trees are
    all alike: both a decomposed and a bare root occur."""
    T_o, c_o = cases.reference(wx, oracle, transform, n, L, B, filt, cost, np.float64)
    assert T_o.shape == (n - 1, B) and c_o.shape == ((2 << L) - 1, B)
    worst = min(cases.split_margin(c_o[:, i], L) for i in range(B))
    probe = np.zeros(n)
    for i in range(B):
        assert wx.isvalidtree(probe, T_o[:, i])
        assert not T_o[(1 << L) - 1:, i].any()
    leaves = [int(T_o[:, i].sum()) + 1 for i in range(B)]
    print("%s n = %d L = %d %s %s: smallest margin %.3g, %d .. %d leaves, %d of %d roots decomposed"
          % (transform, n, L, filt, cost, worst, min(leaves), max(leaves), int(T_o[0].sum()), B))
    assert worst >= cases.MARGIN_MIN, worst
    if n >= 64:
        assert 2 * int(T_o[0].sum()) >= B
    else:
        assert 0 < int(T_o[0].sum()) < B


@pytest.mark.parametrize("name,dtype", [("wx_denoise_swpd1d_sig_trees_f64", np.float64), ("wx_denoise_swpd1d_sig_trees_f32", np.float32),
                                        ("wx_denoise_acwpd1d_sig_trees_f64", np.float64)])
def test_denoise_argument_errors_before_any_device(entry, name, dtype):
    WX_EBOUNDS = -3
    L, q = entry
    fn = getattr(L, name)
    n, B = 16, 3
    x = np.ones((B, n), dtype=dtype)
    out = np.full((B, n), 7, dtype=dtype)
    sig = np.full(B, 7, dtype=dtype)
    thr = np.ones(B, dtype=dtype)
    trees = np.zeros((B, n - 1), dtype=np.uint8)
    trees[:, 0] = 1                                              # the root decomposed: depth 1
    D = ctypes.c_double

    def call(x_=_p(x), o_=_p(out), n_=n, L_=4, t_=_p(trees), nt_=n - 1, B_=B, q_=_p(q), F_=q.size, kind=0, thr_=NULL, nthr=0, s_=_p(sig)):
        return fn(x_, o_, n_, L_, t_, nt_, B_, q_, F_, kind, D(1.0), thr_, nthr, 0, s_, NULL)

    route = L.wx_red_bb_last_route
    assert call(B_=0) == WX_OK and route() == 3                  # no signals: nothing written
    assert call(n_=0) == WX_EARG and route() == 0
    assert call(B_=0) == WX_OK and route() == 3
    assert call(B_=-1) == WX_EARG and route() == 0
    assert call(x_=NULL) == WX_EARG
    assert call(q_=NULL) == WX_EARG
    assert call(t_=NULL) == WX_EARG
    assert call(F_=5) == WX_EARG
    assert call(kind=4) == WX_EARG
    assert call(kind=-1) == WX_EARG
    assert call(thr_=_p(thr), nthr=2) == WX_EARG                 # not 0, 1 or batch
    assert call(thr_=_p(thr), nthr=0) == WX_EARG                 # thr and nthr disagree
    assert call(nthr=1) == WX_EARG
    assert call(o_=NULL, s_=NULL) == WX_EARG                     # neither xhat nor sigma
    assert call(o_=_p(x)) == WX_EARG                             # out == x
    assert call(n_=12, nt_=11, L_=2) == WX_EASSERT               # not dyadic
    assert call(L_=5) == WX_EASSERT
    assert call(L_=-1) == WX_EASSERT
    assert call(nt_=n) == WX_EASSERT
    bad = trees.copy()
    bad[1, 0], bad[1, 1] = 0, 1                                  # column 1: a decomposed node under a bare root
    assert call(t_=_p(bad)) == WX_EASSERT
    assert call(L_=0) == WX_EBOUNDS                              # every column decomposes the root, a node of depth 0 >= L
    deep = trees.copy()
    deep[2, 1] = 1                                               # column 2 decomposes node 2, depth 1
    assert call(t_=_p(deep), L_=1) == WX_EBOUNDS
    both = deep.copy()
    both[1, 0], both[1, 1] = 0, 1                                # the lowest offending column decides: column 1 is invalid
    assert call(t_=_p(both), L_=1) == WX_EASSERT
    assert call(n_=1 << 30, nt_=(1 << 30) - 1, L_=3) == WX_EUNSUPPORTED
    assert route() == 0
    assert (out == 7).all() and (sig == 7).all()
    assert L.wx_last_error().decode()


def test_denoise_debug_grid_windows(wx):
    from waveletsext_jl_amd import _lib
    g = _lib.red_bb_grid
    for ac in (0, 1):
        for F in (2, 8, 20):
            for log2n in range(3, 10):
                for L in range(1, log2n + 1):
                    assert g(1 << log2n, L, F, 8, ac, 1, 1000) > 0, (log2n, L, F, ac)
            assert g(1024, 8, F, 8, ac, 1, 1000) > 0
        assert g(64, 6, 22, 8, ac, 1, 200) == 0                       # 22 taps
        assert g(2048, 4, 8, 8, ac, 1, 2) == 0                        # the estimate's registers: n <= 1024
        assert g(1024, 10, 8, 8, ac, 1, 4) == 0                       # 20 columns of 8 KiB and the taps
        assert g(4096, 12, 8, 8, ac, 1, 2) == 0
    assert g(1024, 10, 8, 4, 0, 1, 1000) > 0                          # Float32 at depth 10
    assert g(2048, 4, 8, 4, 0, 1, 2) == 0


@pytest.mark.parametrize("transform", ["swpd", "acwpd"])
def test_denoise_python_layer_errors(wx, transform):
    from waveletsext_jl_amd import _lib
    f = wx.swpd_denoiseall if transform == "swpd" else wx.acwpd_denoiseall
    x = np.ones((16, 2))
    wt = wx.wavelet(wx.WT.db4)
    trees = np.zeros((15, 2), dtype=bool)
    for est in (wx.relerrorthreshold, wx.surethreshold, np.std):
        with pytest.raises(wx.WxError) as e:
            f(x, wt, trees, estnoise=est)
        assert e.value.code == _lib.WX_EUNSUPPORTED
    with pytest.raises(AssertionError):
        f(x, wt, trees, L=5)
    with pytest.raises(AssertionError):
        f(x, wt, np.zeros((15, 3), dtype=bool))                   # one column per signal (Utils.jl:210)
    deep = trees.copy()
    deep[0] = True
    with pytest.raises(IndexError):
        f(x, wt, deep, L=0)
    assert wx.red_bb_route() == 0
    with pytest.raises(ValueError):
        wx.red_noisestall(x, wt, trees, transform="wpt")
    with pytest.raises(ValueError):
        wx.bestbasis_denoiseall(x, wt, transform="wpt")
    with pytest.raises(TypeError):
        wx.bestbasis_denoiseall(x, wt, transform=transform, method=wx.BB())
    with pytest.raises(TypeError):
        wx.bestbasis_denoiseall(x, wt, transform=transform, tree=trees)
    out = f(np.ones((16, 0)), wt, np.zeros((15, 0), dtype=bool))  # no signals: nothing to do, no device needed
    assert out.shape == (16, 0) and wx.red_bb_route() == 3


def test_denoise_autocorrelation_is_float64_only(wx):
    from waveletsext_jl_amd import _lib
    with pytest.raises(wx.WxError) as e:
        wx.acwpd_denoiseall(np.ones((16, 2), dtype=np.float32), wx.wavelet(wx.WT.db4), np.zeros((15, 2), dtype=bool))
    assert e.value.code == _lib.WX_EUNSUPPORTED


@pytest.mark.parametrize("transform", ["swpd", "acwpd"])
@pytest.mark.parametrize("n,L,B,filt,cost", [c for c in cases.F64_CASES if c[4] == "shannon"])
def test_fixture_hard_threshold_guards(wx, oracle, transform, n, L, B, filt, cost):
    """on the oracle alone, over the leaf coefficients of every signal's chosen tree under HardTH with t = sqrt(2 ln n): the closest
    decision ||c| - sigma t| / (sigma t) is at least 1e-8 wherever sigma > 0 -- what makes a tolerance on sigma a fair demand -- and
    for n >= 64 every such signal has both zeroed and kept coefficients"""
    T_o, _ = cases.reference(wx, oracle, transform, n, L, B, filt, cost, np.float64)
    x = cases.signals(n, L, B)
    q = cases.qmf(wx, filt)
    t = float(np.sqrt(2 * np.log(n)))
    worst = np.inf
    for i in range(B):
        tab = cases.table(oracle, transform, x[:, i], q, L)
        sigma = float(oracle.noisest(tab, True, T_o[:, i]))
        if not sigma > 0:
            continue
        leaves = np.flatnonzero(oracle.getleaf(T_o[:, i], "binary"))
        c = np.abs(tab[:, leaves[leaves < tab.shape[1]]])
        worst = min(worst, float((np.abs(c - sigma * t) / (sigma * t)).min()))
        if n >= 64:
            assert (c <= sigma * t).any() and (c > sigma * t).any(), i
    print("%s n = %d L = %d %s: smallest Hard margin %.3g" % (transform, n, L, filt, worst))
    assert worst >= 1e-8, worst
