"""wptall / iwptall / iwpdall with one tree per signal (csrc/wx_wpt_trees.hip) against the oracle's wpt / iwpt / iwpd called per
signal with that signal's tree, within helpers.TOL.

Sizes, each for one way the kernel can go wrong: 8 and 16 (every node shorter than most filters: the modulo wrap goes round more
than once), 64 (32 items on 64 lanes: idle lanes), 1024 (512 items on 512 lanes, ten levels), 8192 Float64 / 16384 Float32 (the LDS
limit, several items per lane), 16384 Float64 / n = 4 / 22 taps (outside the window: the per-signal fallback)."""
import numpy as np
import pytest

import helpers

pytestmark = pytest.mark.gpu

FILTERS = ["haar", "db2", "db4", "db8", "db10"]                      # 2, 4, 8, 16 and 20 taps


def _log2(n):
    return int(n).bit_length() - 1


def _deep(n, depth, right):
    """the chain root -> left (right) child -> ... decomposed `depth` times"""
    t = np.zeros(n - 1, dtype=bool)
    node = 1
    for _ in range(depth):
        t[node - 1] = True
        node = 2 * node + (1 if right else 0)
    return t


def _tree_mix(wx, n, rng, extra=0):
    """the batch of trees every case runs, asserted below: [copy, full, :dwt, left-deep, right-deep, random p = 0.3, 0.7, 0.9, ...]"""
    L = _log2(n)
    cols = [np.zeros(n - 1, dtype=bool), wx.maketree(n, L, "full"), wx.maketree(n, L, "dwt"), _deep(n, L - 1, False), _deep(n, L, True)]
    seen = {c.tobytes() for c in cols}
    for i in range(3 + extra):
        p = (0.3, 0.7, 0.9)[i % 3]
        t = helpers.random_tree_1d(n, rng, p)
        while t.tobytes() in seen or not t[0]:                        # a new tree each time, never the bare root's copy
            t = helpers.random_tree_1d(n, rng, p)
        seen.add(t.tobytes())
        cols.append(t)
    trees = np.asfortranarray(np.stack(cols, axis=1))
    # the mix itself, whatever the seed gave
    assert not trees[:, 0].any() and trees[:, 1].all()
    assert (trees[:, 2] == wx.maketree(n, L, "dwt")).all()
    left, right = trees[:, 3], trees[:, 4]                            # adjacent columns: a tree kept from the previous signal shows
    assert left[[0, 1]].all() and not left[2] and right[[0, 2]].all() and not right[1]
    assert left.sum() == L - 1 and right.sum() == L
    assert len({trees[:, i].tobytes() for i in range(trees.shape[1])}) == trees.shape[1]
    assert all(wx.isvalidtree(np.zeros(n), trees[:, i]) for i in range(trees.shape[1]))
    return trees


def _per_signal(fn, a, qmf, trees):
    return np.stack([fn(a[..., i], qmf, trees[:, i]) for i in range(trees.shape[1])], axis=-1)


def _check_all(wx, oracle, dtype, n, wname, trees, rng):
    wt = wx.wavelet(wname)                                            # by name: "db11" (22 taps) is computed, not tabulated
    tol = helpers.TOL[np.dtype(dtype)]
    B = trees.shape[1]
    x = np.asfortranarray(rng.standard_normal((n, B)).astype(dtype))
    # forward: the leaves at their nodes' own ranges
    y = wx.wptall(x, wt, trees)
    assert y.dtype == dtype and y.shape == x.shape
    e = helpers.relerr(y, _per_signal(oracle.wpt, x, wt.qmf, trees))
    print("wpt", e)
    assert e <= tol
    table = wx.wpdall(x, wt)
    e = helpers.relerr(y, wx.getbasiscoefall(table, trees))
    print("wpt vs gather", e)
    assert e <= tol
    # inverse, from coefficients that no forward transform made and as a round trip
    c = np.asfortranarray(rng.standard_normal((n, B)).astype(dtype))
    e = helpers.relerr(wx.iwptall(c, wt, trees), _per_signal(oracle.iwpt, c, wt.qmf, trees))
    print("iwpt", e)
    assert e <= tol
    e = helpers.relerr(wx.iwptall(y, wt, trees), x)
    print("iwpt(wpt)", e)
    assert e <= tol
    # iwpd: the round trip through the table, and a table of random values
    e = helpers.relerr(wx.iwpdall(table, wt, trees), x)
    print("iwpd(wpd)", e)
    assert e <= tol
    rt = np.asfortranarray(rng.standard_normal(table.shape).astype(dtype))
    e = helpers.relerr(wx.iwpdall(rt, wt, trees), _per_signal(oracle.iwpd, rt, wt.qmf, trees))
    print("iwpd", e)
    assert e <= tol


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("wname", FILTERS)
@pytest.mark.parametrize("n", [8, 16, 64, 1024])
def test_three_families_against_the_oracle(wx, oracle, n, wname, dtype):
    rng = np.random.default_rng(1000 * n + len(wname) + ord(wname[-1]))
    trees = _tree_mix(wx, n, rng, extra=3)                             # 11 signals: an odd batch
    assert trees.shape[1] == 11
    _check_all(wx, oracle, dtype, n, wname, trees, rng)


@pytest.mark.parametrize("n,dtype,wname", [(8192, np.float64, "db4"), (8192, np.float64, "db10"), (16384, np.float32, "db4"),
                                           (16384, np.float32, "db10")])
def test_lds_limit(wx, oracle, n, dtype, wname):
    """the longest signals the kernel takes: the filter, both buffers and the tree's bits fill 129.5 KiB (Float64) / 130.5 KiB (Float32) of the 160"""
    rng = np.random.default_rng(n)
    mix = _tree_mix(wx, n, rng)
    trees = np.asfortranarray(mix[:, [7, 3, 4]])                       # random p = 0.9 (deep and bushy), left-deep, right-deep
    _check_all(wx, oracle, dtype, n, wname, trees, rng)


def test_table_with_more_columns_than_the_deepest_tree(wx, oracle):
    n, k, B = 64, 6, 5
    rng = np.random.default_rng(3)
    wt = wx.wavelet(wx.WT.db4)
    trees = np.asfortranarray(np.stack([wx.maketree(n, 3, "full"), wx.maketree(n, 2, "dwt"), np.zeros(n - 1, dtype=bool),
                                        _deep(n, 3, True), _deep(n, 1, False)], axis=1))    # depth <= 3 under a table of depth 5
    rt = np.asfortranarray(rng.standard_normal((n, k, B)))
    exp = _per_signal(oracle.iwpd, rt, wt.qmf, trees)
    assert helpers.relerr(wx.iwpdall(rt, wt, trees), exp) <= helpers.TOL[np.dtype(np.float64)]
    with pytest.raises(wx.ArgumentError):                              # Utils.jl:120: depth 3 needs four columns
        wx.iwpdall(rt[:, :3, :], wt, trees)


def test_workgroups_take_several_signals_in_turn(wx, oracle):
    """n = 64 Float64: 64 lanes and 512 + 2 * 64 * 8 + 8 = 1544 bytes of LDS per workgroup, so the launch puts 16 workgroups (its
    cap) on each of the 256 CUs: a grid of 4096.  3 * 4096 + 5 signals: workgroups 0 .. 4 take four signals in turn, all others
    three, every one with another tree than the turn before.  wpt and iwpt are checked on every signal, iwpd on a fixed sample
    with the first, the second and the last turns of the stride loop."""
    n, grid = 64, 4096
    B = 3 * grid + 5
    rng = np.random.default_rng(64)
    wt = wx.wavelet(wx.WT.db4)
    pool = _tree_mix(wx, n, rng, extra=53)                             # 61 distinct trees
    assert pool.shape[1] == 61
    b = np.arange(B)
    which = (b + b // grid) % 61                                       # the signals of one workgroup (b, b + 4096, ...) differ in their trees
    assert (which[:-grid] != which[grid:]).all()
    trees = np.asfortranarray(pool[:, which])
    x = np.asfortranarray(rng.standard_normal((n, B)))
    tol = helpers.TOL[np.dtype(np.float64)]
    y = wx.wptall(x, wt, trees)
    assert helpers.relerr(y, _per_signal(oracle.wpt, x, wt.qmf, trees)) <= tol
    assert helpers.relerr(wx.iwptall(y, wt, trees), x) <= tol
    c = np.asfortranarray(rng.standard_normal((n, B)))
    assert helpers.relerr(wx.iwptall(c, wt, trees), _per_signal(oracle.iwpt, c, wt.qmf, trees)) <= tol
    rt = np.asfortranarray(rng.standard_normal((n, 7, B)))
    got = wx.iwpdall(rt, wt, trees)
    last = np.r_[0:64, grid - 3:grid + 3, B - 2 * grid - 8:B - 2 * grid, B - 64:B]     # first, second and last turns of the stride loop
    exp = _per_signal(oracle.iwpd, rt[:, :, last], wt.qmf, trees[:, last])
    assert helpers.relerr(got[:, last], exp) <= tol


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_identical_columns_equal_the_single_tree_entry(wx, dtype):
    n, B = 256, 9
    rng = np.random.default_rng(9)
    wt = wx.wavelet(wx.WT.db4)
    tree = helpers.random_tree_1d(n, rng, 0.8)
    assert tree[0]
    trees = np.asfortranarray(np.repeat(tree[:, None], B, axis=1))
    x = np.asfortranarray(rng.standard_normal((n, B)).astype(dtype))
    assert (wx.wptall(x, wt, trees) == wx.wptall(x, wt, tree)).all()
    assert (wx.iwptall(x, wt, trees) == wx.iwptall(x, wt, tree)).all()
    table = wx.wpdall(x, wt)
    assert (wx.iwpdall(table, wt, trees) == wx.iwpdall(table, wt, tree)).all()


@pytest.mark.parametrize("n,dtype,wname", [(16384, np.float64, "db4"), (4, np.float64, "db2"), (64, np.float32, "db11")])
def test_fallback_outside_the_window(wx, oracle, n, dtype, wname):
    """longer than the LDS holds, shorter than 8, a filter of 22 taps: the single-tree path once per signal inside the library"""
    rng = np.random.default_rng(n)
    L = _log2(n)
    trees = np.asfortranarray(np.stack([helpers.random_tree_1d(n, rng, 0.8) | wx.maketree(n, 2, "full"), _deep(n, L - 1, False),
                                        _deep(n, L, True)], axis=1))
    assert len({trees[:, i].tobytes() for i in range(3)}) == 3
    _check_all(wx, oracle, dtype, n, wname, trees, rng)


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_host_and_device_calls_give_the_same_bits_twice(wx, dtype):
    n = 1024
    rng = np.random.default_rng(21)
    wt = wx.wavelet(wx.WT.db8)
    trees = _tree_mix(wx, n, rng, extra=3)
    B = trees.shape[1]
    x = np.asfortranarray(rng.standard_normal((n, B)).astype(dtype))
    table = wx.wpdall(x, wt)
    xd, td = wx.to_device(x), wx.to_device(table)
    for fn, host, dev in ((wx.wptall, x, xd), (wx.iwptall, x, xd), (wx.iwpdall, table, td)):
        h1 = fn(host, wt, trees)
        h2 = fn(host, wt, trees)
        d1 = wx.to_numpy(fn(dev, wt, trees))
        d2 = wx.to_numpy(fn(dev, wt, trees))
        assert h1.tobytes() == h2.tobytes() == d1.tobytes() == d2.tobytes()
        assert np.isfinite(h1).all() and np.abs(h1).max() > 0
