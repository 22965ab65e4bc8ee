"""GPU parity of the fused per-signal best basis: wpd_bestbasistreeall / bestbasiscoefall (wx_wpd_bbtrees_*, csrc/wx_wpd_bb.hip)
against the CPU oracle ON ITS OWN TABLE (tests/wpd_bb_cases.py), never against the library's wpdall + bestbasistreeall.

Float64 trees equal the oracle's for every signal (tests/test_wpd_bb_cpu.py guards the fixtures' margins); Float32 trees are
valid, cost at most 1e-4 relative more than the oracle's tree on the oracle's costs, and at most 10 % of a case's signals differ.
Costs: helpers.relerr <= 1e-10 / 1e-4, the tolerances of tests/test_gpu_bestbasis.py.  Shapes: the smallest at which the kernel can
go wrong -- nodes shorter than the filter, one wavefront per level, batch striding with a ragged last round, several wavefronts,
partial depth, sums across wavefronts, the edge of the LDS window, and both routes around it."""
import numpy as np
import pytest

import wpd_bb_cases as cases
from helpers import TOL, relerr

pytestmark = pytest.mark.gpu

DTYPES = [np.float64, np.float32]
FUSED, CHUNKED, TRIVIAL = 1, 2, 3


def _run(wx, oracle, n, filt, L, cost, dtype, route, B=None, device_input=False):
    x = cases.signals(n).astype(dtype)
    T_o, c_o = cases.reference(wx, oracle, n, filt, L, cost, dtype)
    if B is not None:
        idx = np.arange(B) % x.shape[1]
        x, T_o, c_o = x[:, idx], T_o[:, idx], c_o[:, idx]
    x = np.asfortranarray(x)
    arg = wx.to_device(x, "cuda:0") if device_input else x
    trees, costs = wx.wpd_bestbasistreeall(arg, cases.wavelet(wx, filt), L, wx.BB(cost=cases.cost_of(wx, cost)), return_costs=True)
    assert wx.wpd_bb_route() == route
    costs = wx.to_numpy(costs)
    assert costs.shape == c_o.shape and costs.dtype == np.dtype(dtype)
    err = relerr(costs, c_o)
    print("n = %d B = %d %s L = %s %s %s: cost error %.3g" % (n, x.shape[1], filt, L, cost, np.dtype(dtype).name, err))
    assert err <= cases.CTOL[np.dtype(dtype)], err
    cases.check_trees(wx, trees, T_o, c_o, dtype, n)
    # without the costs: the same trees
    t2 = wx.wpd_bestbasistreeall(arg, cases.wavelet(wx, filt), L, wx.BB(cost=cases.cost_of(wx, cost)))
    assert (np.asarray(t2) == np.asarray(trees)).all()
    return trees


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("filt", ["db4", "db8"])
def test_nodes_shorter_than_the_filter(wx, oracle, dtype, filt):
    """n = 8, L = 3: nodes of 4, 2 and 1 samples under 8 and 16 taps -- the wrap is a true modulo"""
    _run(wx, oracle, 8, filt, 3, "shannon", dtype, FUSED)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("B", [5, 4 * cases.GRID_SHORT + 1])
def test_one_wavefront_per_level_and_batch_striding(wx, oracle, dtype, B):
    """n = 64: one wavefront per signal; fewer signals than workgroups, and four full rounds of the grid plus one signal"""
    _run(wx, oracle, 64, "db4", None, "shannon", dtype, FUSED, B=B, device_input=B > 5)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("filt", ["haar", "db8"])
def test_short_signals_other_filters(wx, oracle, dtype, filt):
    _run(wx, oracle, 64, filt, None, "shannon", dtype, FUSED)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("L", [0, 1, 5, 8])
def test_partial_depth(wx, oracle, dtype, L):
    """n = 256: several wavefronts; L = 0 decomposes nothing -- all-false trees, the root's cost, route 3"""
    trees = _run(wx, oracle, 256, "db4", L, "shannon", dtype, TRIVIAL if L == 0 else FUSED)
    if L == 0:
        assert not np.asarray(trees).any()


@pytest.mark.parametrize("dtype", DTYPES)
def test_log_energy_cost(wx, oracle, dtype):
    _run(wx, oracle, 256, "db4", 8, "logenergy", dtype, FUSED)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("filt", ["haar", "db4", "db8"])
def test_sums_across_wavefronts(wx, oracle, dtype, filt):
    """n = 1024: nodes of 64 ... 1024 coefficients are summed over several wavefronts"""
    _run(wx, oracle, 1024, filt, None, "shannon", dtype, FUSED)


@pytest.mark.parametrize("dtype", DTYPES)
def test_edge_of_the_lds_window(wx, oracle, dtype):
    """n = 4096, L = 12: 137.6 KiB of LDS in Float64 -- must be the fused kernel"""
    _run(wx, oracle, 4096, "db4", 12, "shannon", dtype, FUSED)


@pytest.mark.parametrize("dtype", DTYPES)
def test_longer_than_the_window(wx, oracle, dtype):
    """n = 8192, L = 13: 128 KiB of Float64 level buffers and as much again of costs do not fit -- chunks through the table kernels, the same
    contract.  Float32 needs half of that and is the edge of ITS window (146.6 KiB): the fused kernel."""
    _run(wx, oracle, 8192, "db4", 13, "shannon", dtype, CHUNKED if dtype == np.float64 else FUSED)


@pytest.mark.parametrize("dtype", DTYPES)
def test_filter_outside_the_window(wx, oracle, dtype):
    """22 taps: no LDS kernel of the library takes them -- chunks through the table kernels"""
    _run(wx, oracle, 64, "rand22", None, "shannon", dtype, CHUNKED)


@pytest.mark.parametrize("dtype", DTYPES)
def test_zero_nan_and_inf_columns(wx, oracle, dtype):
    """nrm == 0 and non-finite input: an all-false tree in all three, like the oracle's"""
    n = 256
    x = np.array(cases.signals(n)[:, :7], dtype=dtype, order="F")
    x[:, 1] = 0.0
    x[17, 2] = np.nan
    x[200, 4] = np.inf
    T_o, c_o = cases.reference(wx, oracle, n, "db4", None, "shannon", dtype, x=x, key="special")
    for col in (1, 2, 4):
        assert not T_o[:, col].any()                              # what the reference does with them
    for arg in (x, wx.to_device(x, "cuda:0")):
        trees, costs = wx.wpd_bestbasistreeall(arg, cases.wavelet(wx, "db4"), return_costs=True)
        assert wx.wpd_bb_route() == FUSED
        trees, costs = np.asarray(trees), wx.to_numpy(costs)
        for col in (1, 2, 4):
            assert not trees[:, col].any(), col
        assert (costs[:, 1] == 0).all()                           # bestbasis_costs.jl:119
        fin = [0, 3, 5, 6]
        assert relerr(costs[:, fin], c_o[:, fin]) <= cases.CTOL[np.dtype(dtype)]
        cases.check_trees(wx, trees[:, fin], T_o[:, fin], c_o[:, fin], dtype, n)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("n,filt", [(1024, "db4"), (4096, "db4"), (64, "rand22")])
def test_host_device_and_repeated_calls_are_byte_identical(wx, dtype, n, filt):
    import torch
    x = np.asfortranarray(cases.signals(n).astype(dtype))
    wt = cases.wavelet(wx, filt)
    th, ch = wx.wpd_bestbasistreeall(x, wt, return_costs=True)
    xd = wx.to_device(x, "cuda:0")
    runs = [wx.wpd_bestbasistreeall(xd, wt, device=True, return_costs=True) for _ in range(2)]
    for td, cd in runs:
        assert isinstance(td, torch.Tensor) and td.dtype == torch.bool and td.shape == (n - 1, x.shape[1])
        assert td.stride() == (1, n - 1)                          # column-major, what wptall / iwptall / denoiseall take
        assert np.array_equal(td.cpu().numpy(), th)
        assert wx.to_numpy(cd).tobytes() == np.asfortranarray(ch).tobytes()
    tn = wx.wpd_bestbasistreeall(xd, wt)                          # device data, host trees
    assert isinstance(tn, np.ndarray) and np.array_equal(tn, th)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("n", [256, 1024])
def test_end_to_end_coefficients(wx, oracle, dtype, n):
    """bestbasiscoefall: every signal in its own basis and back; Float64 coefficients against the oracle's wpt along its own tree"""
    x = np.asfortranarray(cases.signals(n).astype(dtype))
    wt = cases.wavelet(wx, "db4")
    T_o, _ = cases.reference(wx, oracle, n, "db4", None, "shannon", dtype)
    for dev in (False, True):
        arg = wx.to_device(x, "cuda:0") if dev else x
        y, t = wx.bestbasiscoefall(arg, wt, device=dev)
        back = wx.to_numpy(wx.iwptall(y, wt, t))
        assert relerr(back, x) <= TOL[np.dtype(dtype)]
        y = wx.to_numpy(y)
        t = t.cpu().numpy() if dev else t
        if dtype == np.float64:
            assert (t == T_o).all()
            for i in range(x.shape[1]):
                assert relerr(y[:, i], oracle.wpt(x[:, i], wt.qmf, T_o[:, i])) <= TOL[np.dtype(dtype)], i
