"""GPU parity of the full-depth lattice inverse with its deepest levels folded into node matrices (csrc/wx_lattice_fold.h,
k_lat_iwpt12_f64 / k_lat_iwpt8k12_f64) against the CPU oracle and against the unfolded kernels (dispatch mode 3).  n = 4096 is
the only length these kernels take (8192 through the two-wavefront kernel)."""
import numpy as np
import pytest

from helpers import relerr

pytestmark = pytest.mark.gpu
FOLDED = ["db5", "db6", "db7", "db8", "db10"]
N = 4096
BIG = 2051                                                  # more than the 2048 resident wavefronts, and odd
ORACLE_COLS = [0, 1, 1023, 2047, 2048, 2049, 2050]          # columns of the big batch that carry oracle data


def _wt(wx, name):
    return wx.wavelet(getattr(wx.WT, name))


def _mode(wx, mode, f):
    wx.set_force_generic(mode)
    try:
        return f()
    finally:
        wx.set_force_generic(0)


_cache = {}


def _small(wx, oracle, wname):
    """three signals, their oracle coefficients and oracle packet table at depth 12: computed once per filter"""
    if wname not in _cache:
        wt = _wt(wx, wname)
        x = np.asfortranarray(np.random.default_rng(len(wname) + 7 * wt.qmf.size).standard_normal((N, 3)))
        _cache[wname] = (wt, x, oracle.wptall(x, wt.qmf, 12), oracle.wpdall(x, wt.qmf, 12))
    return _cache[wname]


@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("wname", FOLDED)
def test_folded_inverse_small_batches(wx, oracle, wname, B):
    wt, x, w, tab = _small(wx, oracle, wname)
    x, w, tab = (np.asfortranarray(a[..., :B]) for a in (x, w, tab))
    assert tab.shape == (N, 13, B)
    for what, run in (("iwptall", lambda: wx.iwptall(w, wt, 12)), ("iwpdall", lambda: wx.iwpdall(tab, wt, 12))):
        got = run()
        plain = _mode(wx, 3, run)
        e_or, e_pl = relerr(got, x), relerr(got, plain)
        print(wname, B, what, "vs oracle input %.2e" % e_or, "vs mode 3 %.2e" % e_pl)
        assert e_or <= 1e-12, what
        assert relerr(plain, x) <= 1e-12, what
        assert e_pl <= 1e-13, what
        assert not np.array_equal(got, plain), what            # the fold ran


@pytest.mark.parametrize("wname", FOLDED)
def test_folded_inverse_more_signals_than_resident_wavefronts(wx, oracle, wname):
    """2051 signals on the device: coefficients and tables from the forward kernels (which do not fold), the columns ORACLE_COLS
    replaced by the oracle's; every column against the signals and against mode 3"""
    import torch
    wt = _wt(wx, wname)
    x = np.asfortranarray(np.random.default_rng(2051).standard_normal((N, BIG)))
    xs = np.asfortranarray(x[:, ORACLE_COLS])
    xd = wx.to_device(x)
    w = wx.wptall(xd, wt, 12)
    w[:, ORACLE_COLS] = wx.to_device(oracle.wptall(xs, wt.qmf, 12))
    tab = wx.wpdall(xd, wt, 12)
    tab[:, :, ORACLE_COLS] = wx.to_device(oracle.wpdall(xs, wt.qmf, 12))
    for what, run in (("iwptall", lambda: wx.iwptall(w, wt, 12)), ("iwpdall", lambda: wx.iwpdall(tab, wt, 12))):
        got = wx.to_numpy(run())
        plain = wx.to_numpy(_mode(wx, 3, run))
        e_or, e_all, e_pl = relerr(got[:, ORACLE_COLS], xs), relerr(got, x), relerr(got, plain)
        print(wname, what, "oracle columns %.2e" % e_or, "all columns %.2e" % e_all, "vs mode 3 %.2e" % e_pl)
        assert e_or <= 1e-12 and e_all <= 1e-12, what
        assert e_pl <= 1e-13, what
        assert not np.array_equal(got, plain), what
    del xd, w, tab
    torch.cuda.empty_cache()


@pytest.mark.parametrize("L", [10, 11])
@pytest.mark.parametrize("wname", FOLDED)
def test_shallower_depths_keep_the_general_kernel(wx, oracle, wname, L):
    wt, x, _, _ = _small(wx, oracle, wname)
    w = oracle.wptall(x, wt.qmf, L)
    tab = oracle.wpdall(x, wt.qmf, L)
    for run in (lambda: wx.iwptall(w, wt, L), lambda: wx.iwpdall(tab, wt, L)):
        got = run()
        assert np.array_equal(got, _mode(wx, 3, run))
        assert relerr(got, x) <= 1e-12


@pytest.mark.parametrize("wname", ["haar", "db4"])
def test_short_filters_are_bit_identical_controls(wx, oracle, wname):
    wt, x, w, tab = _small(wx, oracle, wname)
    for run in (lambda: wx.iwptall(w, wt, 12), lambda: wx.iwpdall(tab, wt, 12), lambda: wx.wptall(x, wt, 12)):
        assert np.array_equal(run(), _mode(wx, 3, run))
    assert relerr(wx.iwptall(w, wt, 12), x) <= 1e-12


@pytest.mark.parametrize("wname", FOLDED)
def test_forward_does_not_fold(wx, oracle, wname):
    """the forward kernels are the parent's: wptall is bit-identical under mode 3 and matches the oracle"""
    wt, x, w, _ = _small(wx, oracle, wname)
    got = wx.wptall(x, wt, 12)
    assert np.array_equal(got, _mode(wx, 3, lambda: wx.wptall(x, wt, 12)))
    assert relerr(got, w) <= 1e-12


def test_8192_samples_full_depth(wx, oracle):
    """k_lat_iwpt8k12_f64: db8, depth 13, three signals"""
    wt = _wt(wx, "db8")
    x = np.asfortranarray(np.random.default_rng(8192).standard_normal((8192, 3)))
    w = oracle.wptall(x, wt.qmf, 13)
    run = lambda: wx.iwptall(w, wt, 13)
    got, plain = run(), _mode(wx, 3, run)
    print("8192: vs oracle input %.2e" % relerr(got, x), "vs mode 3 %.2e" % relerr(got, plain))
    assert relerr(got, x) <= 1e-12
    assert relerr(got, plain) <= 1e-13
    assert not np.array_equal(got, plain)
    run12 = lambda: wx.iwptall(oracle.wptall(x, wt.qmf, 12), wt, 12)
    assert np.array_equal(run12(), _mode(wx, 3, run12))


@pytest.mark.parametrize("wname", FOLDED)
def test_round_trip_energy(wx, oracle, wname):
    wt, x, _, _ = _small(wx, oracle, wname)
    back = wx.iwpdall(wx.wpdall(x, wt, 12), wt, 12)
    assert abs(float((back * back).sum() / (x * x).sum()) - 1.0) <= 1e-12
    assert relerr(back, x) <= 1e-12
