"""Fused per-signal best basis (wx_wpd_bbtrees_*, wpd_bestbasistreeall), the part that needs no GPU: the argument checks of the C
ABI happen before a device is needed, the Python layer refuses what bestbasistreeall refuses, and the seeded fixtures of the GPU
tests (tests/wpd_bb_cases.py) keep every split decision far enough from a tie that exact tree equality is a fair demand on a
kernel whose coefficients differ from the oracle's in the last bits."""
import ctypes

import numpy as np
import pytest

import wpd_bb_cases as cases

WX_OK, WX_EASSERT, WX_EARG = 0, -1, -2


def _p(a):
    return ctypes.c_void_p(a.ctypes.data)


NULL = ctypes.c_void_p(0)


@pytest.fixture()
def entry(wx):
    from waveletsext_jl_amd import _lib
    L = _lib.lib()
    q = np.ascontiguousarray(wx.wavelet(wx.WT.db4).qmf, dtype=np.float64)
    return L, q


@pytest.mark.parametrize("suffix,dtype", [("_f64", np.float64), ("_f32", np.float32)])
def test_argument_errors_before_any_device(entry, suffix, dtype):
    L, q = entry
    fn = getattr(L, "wx_wpd_bbtrees" + suffix)
    n, B = 16, 3
    x = np.zeros((B, n), dtype=dtype)
    trees = np.full((B, n - 1), 7, dtype=np.uint8)

    def call(x_=_p(x), n_=n, L_=4, B_=B, q_=_p(q), F_=q.size, kind=0, t_=_p(trees), c_=NULL):
        return fn(x_, n_, L_, B_, q_, F_, kind, t_, c_, NULL)

    route = L.wx_wpd_bb_last_route
    assert call(B_=0) == WX_OK and (trees == 7).all()            # no signals: nothing written
    assert route() == 3
    assert call(n_=12, L_=2) == WX_EASSERT                       # not dyadic
    assert route() == 0                                          # a refused call leaves no route behind
    assert call(B_=0) == WX_OK and route() == 3
    assert call(L_=5) == WX_EASSERT and route() == 0             # deeper than maxtransformlevels(16) = 4
    assert call(L_=-1) == WX_EASSERT
    assert call(x_=NULL) == WX_EARG
    assert call(q_=NULL) == WX_EARG
    assert call(t_=NULL) == WX_EARG
    assert call(kind=2) == WX_EARG
    assert call(kind=-1) == WX_EARG
    assert call(F_=5) == WX_EARG                                 # odd filter length
    assert route() == 0
    assert (trees == 7).all()
    msg = L.wx_last_error().decode()
    assert msg


def test_python_layer_type_errors(wx):
    x = np.zeros((16, 2))
    wt = wx.wavelet(wx.WT.db4)
    with pytest.raises(TypeError):
        wx.wpd_bestbasistreeall(x, wt, method=wx.BB(redundant=True))
    with pytest.raises(TypeError):
        wx.wpd_bestbasistreeall(x, wt, method=wx.JBB())
    with pytest.raises(TypeError):
        wx.wpd_bestbasistreeall(x, wt, method=wx.LSDB())
    with pytest.raises(TypeError):
        wx.wpd_bestbasistreeall(x, wt, device=True)               # device=True takes a device tensor
    with pytest.raises(TypeError):
        wx.bestbasiscoefall(x, wt, method=wx.BB(redundant=True))
    with pytest.raises(AssertionError):
        wx.wpd_bestbasistreeall(x, wt, L=5)                       # WX_EASSERT, before a device is needed
    with pytest.raises(AssertionError):
        wx.wpd_bestbasistreeall(np.zeros((12, 2)), wt, L=2)
    assert wx.wpd_bb_route() == 0
    t = wx.wpd_bestbasistreeall(np.zeros((16, 0)), wt)            # no signals: an empty matrix, no device needed
    assert t.shape == (15, 0) and t.dtype == np.bool_
    assert wx.wpd_bb_route() == 3
    t, c = wx.wpd_bestbasistreeall(np.zeros((16, 0), dtype=np.float32), wt, L=2, return_costs=True)
    assert t.shape == (15, 0) and c.shape == (7, 0) and c.dtype == np.float32


@pytest.mark.parametrize("n,filt,L,cost", cases.F64_CASES)
def test_fixture_margins(wx, oracle, n, filt, L, cost):
    """every signal's closest split decision, min |cc - pc| / |pc| (wx_treeselect_gap_f64 on the ORACLE's costs), is at least
    1e-8: four orders above what the last bits of a Float64 table move a cost by (1e-13 relative flipped no tree)"""
    T_o, c_o = cases.reference(wx, oracle, n, filt, L, cost, np.float64)
    if c_o.shape[0] == 1:
        assert not T_o.any()                                      # L = 0: no decision to take
        return
    worst = np.inf
    for i in range(c_o.shape[1]):
        tree, gap = wx.bestbasis_treeselection(c_o[:, i], n, return_gap=True)
        assert (tree == T_o[:, i]).all()                          # the library's host selection agrees with the oracle's
        worst = min(worst, gap)
    print("n = %d %s L = %s %s: smallest margin %.3g" % (n, filt, L, cost, worst))
    assert worst >= cases.MARGIN_MIN, worst


def test_leaf_cost_helper():
    # depth-2 heap: root decomposed, left child decomposed, right child a leaf -> leaves are nodes 4, 5, 3
    c = np.array([10.0, 20.0, 3.0, 4.0, 5.0, 6.0, 7.0])
    assert cases.leaf_cost(np.array([True, True, False]), c) == 4.0 + 5.0 + 3.0
    assert cases.leaf_cost(np.array([False, False, False]), c) == 10.0
    assert cases.leaf_cost(np.array([True, True, True]), c) == 4.0 + 5.0 + 6.0 + 7.0


def test_batch_striding_case_is_tied_to_the_launch_grid(wx):
    """the GPU case `four rounds of the grid plus one signal` takes its batch from GRID_SHORT: that must be the grid the launch of
    a 64-sample signal really uses (wx_debug_wpd_bb_grid asks the functions the launch calls; no device needed)"""
    from waveletsext_jl_amd import _lib
    for esz in (8, 4):
        assert _lib.wpd_bb_grid(64, 6, 8, esz, 4 * cases.GRID_SHORT + 1) == cases.GRID_SHORT
        assert _lib.wpd_bb_grid(64, 6, 8, esz, 5) == 5                # never more workgroups than signals
    assert _lib.wpd_bb_grid(4096, 12, 8, 8, 10 ** 6) == 256           # 137.6 KiB of LDS: one workgroup per CU
    assert _lib.wpd_bb_grid(8192, 13, 8, 8, 3) == 0                   # outside the Float64 window: the chunked route
    assert _lib.wpd_bb_grid(8192, 13, 8, 4, 3) == 3                   # inside the Float32 window
    assert _lib.wpd_bb_grid(64, 6, 22, 8, 200) == 0                   # 22 taps: outside
