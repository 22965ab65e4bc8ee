"""GPU parity of the redundant per-signal best basis straight from the signals: swpd_bestbasistreeall / acwpd_bestbasistreeall
(wx_swpd_bbtrees_*, wx_acwpd_bbtrees_f64, csrc/wx_red_bb.hip) against the CPU oracle ON ITS OWN TABLE (tests/red_bb_cases.py), never
against the library's swpdall / acwpdall + bestbasistreeall.

Float64 trees equal the oracle's for every signal (tests/test_red_bb_cpu.py guards the fixtures' margins); Float32 trees are valid,
cost at most 1e-4 relative more than the oracle's tree on the oracle's costs, and at most 10 % of a case's signals differ.  Costs:
helpers.relerr per column <= 1e-10 / 1e-4.  Shapes: the smallest at which the kernel can go wrong -- columns shorter than the filter, one
wavefront per column, several, sixteen; partial depth; the edge of the LDS window and both routes around it; batch striding with a
ragged last round."""
import numpy as np
import pytest

import red_bb_cases as cases
from helpers import relerr

pytestmark = pytest.mark.gpu

FUSED, CHUNKED, TRIVIAL = 1, 2, 3
TRANSFORMS = ["swpd", "acwpd"]


def _check(wx, trees, costs, T_o, c_o, dtype, n, what):
    costs = wx.to_numpy(costs)
    assert costs.shape == c_o.shape and costs.dtype == np.dtype(dtype)
    err = max(relerr(costs[:, i], c_o[:, i]) for i in range(c_o.shape[1]))
    print("%s %s: cost error %.3g" % (what, np.dtype(dtype).name, err))
    assert err <= cases.CTOL[np.dtype(dtype)], err
    cases.check_trees(wx, trees, T_o, c_o, dtype, n)


def _run(wx, oracle, transform, n, L, B, filt, cost, dtype, route, device_input=False):
    x = np.asfortranarray(cases.signals(n, L, B).astype(dtype))
    T_o, c_o = cases.reference(wx, oracle, transform, n, L, B, filt, cost, dtype)
    arg = wx.to_device(x, "cuda:0") if device_input else x
    f = cases.entry(wx, transform)
    trees, costs = f(arg, cases.wavelet(wx, filt), L, cases.bb(wx, cost), return_costs=True)
    assert wx.red_bb_route() == route
    _check(wx, trees, costs, T_o, c_o, dtype, n, "%s n = %d L = %d B = %d %s %s" % (transform, n, L, B, filt, cost))
    # without the costs: the same trees
    t2 = f(arg, cases.wavelet(wx, filt), L, cases.bb(wx, cost))
    assert np.asarray(t2).tobytes() == np.asarray(trees).tobytes()
    return np.asarray(trees)


@pytest.mark.parametrize("transform", TRANSFORMS)
@pytest.mark.parametrize("n,L,B,filt,cost", cases.F64_CASES)
def test_float64_cases(wx, oracle, transform, n, L, B, filt, cost):
    _run(wx, oracle, transform, n, L, B, filt, cost, np.float64, FUSED, device_input=n == 64)


@pytest.mark.parametrize("n,L,B,filt,cost", cases.F32_CASES)
def test_float32_stationary(wx, oracle, n, L, B, filt, cost):
    _run(wx, oracle, "swpd", n, L, B, filt, cost, np.float32, FUSED, device_input=n == 64)


@pytest.mark.parametrize("transform", TRANSFORMS)
@pytest.mark.parametrize("L", [1, 5])
def test_partial_depth(wx, oracle, transform, L):
    """n = 256: bytes above 2^L - 1 are zero"""
    trees = _run(wx, oracle, transform, 256, L, 12, "db4", "shannon", np.float64, FUSED)
    assert not trees[(1 << L) - 1:].any()
    assert trees.view(np.uint8).max() <= 1


@pytest.mark.parametrize("transform,dtype", [("swpd", np.float64), ("swpd", np.float32), ("acwpd", np.float64)])
def test_depth_zero(wx, oracle, transform, dtype):
    """L = 0 decomposes nothing: route 3, all-false trees, the root's cost of a one-column table"""
    trees = _run(wx, oracle, transform, 256, 0, 12, "db4", "shannon", dtype, TRIVIAL)
    assert not trees.any()


@pytest.mark.parametrize("transform,dtype", [("swpd", np.float64), ("swpd", np.float32), ("acwpd", np.float64)])
def test_zero_column(wx, oracle, transform, dtype):
    """nrm == 0 among others: an all-false tree and zero costs (bestbasis_costs.jl:119), the neighbours unchanged"""
    n, L, B = 64, 6, 24
    f = cases.entry(wx, transform)
    wt = cases.wavelet(wx, "db4")
    x = np.array(cases.signals(n, L, B).astype(dtype), order="F")
    t0, c0 = f(x, wt, L, return_costs=True)
    x[:, 5] = 0.0
    t1, c1 = f(x, wt, L, return_costs=True)
    assert wx.red_bb_route() == FUSED
    assert not t1[:, 5].any() and (c1[:, 5] == 0).all()
    rest = [i for i in range(B) if i != 5]
    assert t1[:, rest].tobytes() == t0[:, rest].tobytes()
    assert np.asfortranarray(c1[:, rest]).tobytes() == np.asfortranarray(c0[:, rest]).tobytes()


@pytest.mark.parametrize("transform,dtype", [("swpd", np.float64), ("swpd", np.float32), ("acwpd", np.float64)])
def test_filter_outside_the_window(wx, oracle, transform, dtype):
    """22 taps: no LDS kernel of the library takes them -- chunks of signals through the table kernels, the same contract"""
    _run(wx, oracle, transform, 64, 6, 24, "rand22", "shannon", dtype, CHUNKED)


@pytest.mark.parametrize("transform", TRANSFORMS)
def test_longer_than_the_window(wx, oracle, transform):
    """Float64 n = 4096, L = 12: 25 columns of 32 KiB do not fit; one signal's table (256 MiB) is a chunk"""
    _run(wx, oracle, transform, 4096, 12, 2, "db4", "shannon", np.float64, CHUNKED)


@pytest.mark.parametrize("transform,dtype", [("swpd", np.float64), ("swpd", np.float32), ("acwpd", np.float64)])
def test_batch_striding(wx, oracle, transform, dtype):
    """n = 8: four full rounds of the launch grid plus one signal, the fixture's columns repeated; every repeat carries the same bytes,
    and the distinct columns are the oracle's"""
    n, L, B = 8, 3, 24
    x = cases.signals(n, L, B).astype(dtype)
    T_o, c_o = cases.reference(wx, oracle, transform, n, L, B, "db4", "shannon", dtype)
    N = 4 * cases.GRID_8 + 1
    idx = np.arange(N) % B
    xd = wx.to_device(np.asfortranarray(x[:, idx]), "cuda:0")
    trees, costs = cases.entry(wx, transform)(xd, cases.wavelet(wx, "db4"), L, return_costs=True)
    assert wx.red_bb_route() == FUSED
    costs = wx.to_numpy(costs)
    _check(wx, trees[:, :B], costs[:, :B], T_o, c_o, dtype, n, "%s striding" % transform)
    assert (trees == trees[:, idx]).all()                             # column j carries the bytes of column j mod B
    assert np.asfortranarray(costs).tobytes() == np.asfortranarray(costs[:, idx]).tobytes()


@pytest.mark.parametrize("transform,dtype,n,L,B,filt", [("swpd", np.float64, 256, 8, 12, "db4"), ("swpd", np.float32, 1024, 10, 4, "db4"),
                                                        ("acwpd", np.float64, 1024, 8, 4, "haar"), ("swpd", np.float64, 64, 6, 24, "rand22")])
def test_host_device_and_repeated_calls_are_byte_identical(wx, transform, dtype, n, L, B, filt):
    import torch
    f = cases.entry(wx, transform)
    x = np.asfortranarray(cases.signals(n, L, B).astype(dtype))
    wt = cases.wavelet(wx, filt)
    th, ch = f(x, wt, L, return_costs=True)
    xd = wx.to_device(x, "cuda:0")
    for td, cd in [f(xd, wt, L, device=True, return_costs=True) for _ in range(2)]:
        assert isinstance(td, torch.Tensor) and td.dtype == torch.bool and td.shape == (n - 1, B)
        assert td.stride() == (1, n - 1)                              # column-major, what iswpdall / denoiseall take
        assert np.array_equal(td.cpu().numpy(), th)
        assert wx.to_numpy(cd).tobytes() == np.asfortranarray(ch).tobytes()
    tn = f(xd, wt, L)                                                 # device data, host trees, no costs
    assert isinstance(tn, np.ndarray) and tn.tobytes() == th.tobytes()


@pytest.mark.parametrize("transform,dtype", [("swpd", np.float64), ("swpd", np.float32), ("acwpd", np.float64)])
def test_non_finite_columns_stay_in_their_columns(wx, transform, dtype):
    """one column all NaN, one with a +Inf: the call returns, their trees are valid trees, every other column's bytes are those of
    a call without them"""
    n, L, B = 64, 6, 24
    f = cases.entry(wx, transform)
    wt = cases.wavelet(wx, "db4")
    x = np.array(cases.signals(n, L, B).astype(dtype), order="F")
    t0, c0 = f(x, wt, L, return_costs=True)
    x[:, 3] = np.nan
    x[40, 17] = np.inf
    t1, c1 = f(x, wt, L, return_costs=True)
    assert wx.red_bb_route() == FUSED
    probe = np.zeros(n)
    for col in (3, 17):
        assert t1.view(np.uint8)[:, col].max() <= 1
        assert wx.isvalidtree(probe, t1[:, col]), col
    rest = [i for i in range(B) if i not in (3, 17)]
    assert t1[:, rest].tobytes() == t0[:, rest].tobytes()
    assert np.asfortranarray(c1[:, rest]).tobytes() == np.asfortranarray(c0[:, rest]).tobytes()


@pytest.mark.parametrize("transform", TRANSFORMS)
def test_trees_feed_the_table_consumers(wx, oracle, transform):
    """the device tree matrix is what iswpdall / iacwpdall take: the signal comes back along its own basis"""
    n, L, B = 256, 8, 12
    x = np.asfortranarray(cases.signals(n, L, B))
    wt = cases.wavelet(wx, "db4")
    xd = wx.to_device(x, "cuda:0")
    M = cases.entry(wx, transform)(xd, wt, L, device=True)
    if transform == "swpd":
        back = wx.iswpdall(wx.swpdall(xd, wt, L), wt, M)
    else:
        back = wx.iacwpdall(wx.acwpdall(xd, wt, L), M)
    assert relerr(wx.to_numpy(back), x) <= 1e-10
