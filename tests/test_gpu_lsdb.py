"""LSDB best basis on the MI355X: per-row differential entropies, tree costs and trees against tests/lsdb_ref.py
(bestbasis_costs.jl:135-164, bestbasis_tree.jl:104-147, BestBasis.jl:185-192)."""
import numpy as np
import pytest

import lsdb_ref

pytestmark = pytest.mark.gpu
TOL = {np.float64: 1e-10, np.float32: 1e-5}


def _close(got, exp, dt, scale=None):
    # a sample at or past the last grid point has pdf 0 (the grid is one point short of (nbins + 1) mbins): an infinite
    # entropy, on both sides, for some heavy-tailed rows
    got, exp = np.asarray(got, dtype=np.float64), np.asarray(exp, dtype=np.float64)
    assert not np.isnan(got).any()
    fin = np.isfinite(exp)
    assert np.array_equal(np.isfinite(got), fin) and np.array_equal(got[~fin], exp[~fin])
    den = np.maximum(np.abs(exp), 1.0) if scale is None else np.broadcast_to(scale, exp.shape)
    err = float(np.max(np.abs(got[fin] - exp[fin]) / den[fin], initial=0.0))
    assert err <= TOL[dt], err


def _rows(kind, nk, N, rng):
    if kind == "gauss":
        return rng.standard_normal((nk, N))
    if kind == "cauchy":
        return rng.standard_cauchy((nk, N))
    # heavy ties: few distinct values (every row keeps at least two)
    X = rng.integers(0, 4, (nk, N)).astype(np.float64) * 0.5
    X[:, 0], X[:, -1] = 0.0, 1.5
    return X


def _cost_scale(X, redundant):
    """|cost| plus the sum of |row entropy| of its rows bounds the rounding of a node sum"""
    E = np.abs(lsdb_ref.row_entropy(X.reshape(-1, X.shape[-1], order="F"))).reshape(X.shape[:-1], order="F")
    return np.maximum(np.abs(lsdb_ref.node_costs(E, redundant)), 1.0)


@pytest.mark.parametrize("dt", [np.float64, np.float32])
@pytest.mark.parametrize("N", [2, 3, 7, 64, 257, 1000, 4096])
@pytest.mark.parametrize("kind", ["gauss", "cauchy", "ties"])
def test_row_entropy_matches_helper(wx, dt, N, kind):
    rng = np.random.default_rng(N * 7 + len(kind))
    X = _rows(kind, 70, N, rng).astype(dt)
    X = np.asfortranarray(X)
    if N == 2:
        X[:, 1] = X[:, 0] + np.where(X[:, 0] == 0, 1, X[:, 0])   # distinct pairs
    exp = lsdb_ref.row_entropy(X)
    got = wx.lsdb_entropy(X)
    assert got.dtype == np.float64 and got.shape == (70,)
    _close(got, exp, dt)


def test_row_entropy_values_on_bin_edges(wx):
    # rows of small integers with a power-of-two count or an exact standard deviation: the grid is the same to the bit on
    # both sides, and the values that fall on (within an ulp of) a bin edge are counted by the same rounding
    rows, edges = [], 0
    rng = np.random.default_rng(3)
    base = np.array([-1.0, -1.0, 0.0, 1.0, 1.0])                 # sigma = 1, 0 lies on an edge of the 68-point grid
    for s in (1.0, 2.0, 0.5, 4.0, 0.25):
        rows.append(base * s)
    X = np.array(rows)
    a, delta, length, _, _ = lsdb_ref.row_grid(X)
    t = (X - a[:, None]) / delta[:, None] + 1.5
    edges += int((np.abs(t - np.round(t)) < 1e-9).sum())
    assert edges >= 5
    _close(wx.lsdb_entropy(np.asfortranarray(X)), lsdb_ref.row_entropy(X), np.float64)
    Y = rng.integers(-3, 4, (64, 8)).astype(np.float64)           # 8 signals: sums and deviations exact
    Y[:, 0], Y[:, 1] = -3.0, 3.0
    _close(wx.lsdb_entropy(np.asfortranarray(Y)), lsdb_ref.row_entropy(Y), np.float64)


@pytest.mark.parametrize("dt", [np.float64, np.float32])
def test_split_signal_axis(wx, dt):
    # 130 rows x 100000 signals: three row tiles, the signal axis split over hundreds of workgroups
    rng = np.random.default_rng(11)
    X = np.asfortranarray(rng.standard_normal((130, 100000)).astype(dt))
    X[::3] *= 10.0
    got = wx.lsdb_entropy(wx.to_device(X, "cuda:0"))
    got = wx.to_numpy(got)
    sample = np.arange(0, 130, 13)
    _close(got[sample], lsdb_ref.row_entropy(X, rows=sample), dt)


@pytest.mark.parametrize("dt", [np.float64, np.float32])
@pytest.mark.parametrize("n,L,N", [(8, 3, 40), (64, 4, 100), (64, 6, 33), (1024, 5, 20), (4096, 3, 12)])
def test_tree_costs_wpd_1d(wx, dt, n, L, N):
    rng = np.random.default_rng(n + L)
    wt = wx.wavelet(wx.WT.db4)
    X = wx.to_numpy(wx.wpdall(np.asfortranarray(rng.standard_normal((n, N)).astype(dt)), wt, L))
    X = np.asfortranarray(X)
    exp = lsdb_ref.tree_costs(X)
    for inp in (X, wx.to_device(X, "cuda:0")):
        got = wx.to_numpy(wx.tree_costs(inp, wx.LSDB()))
        assert got.dtype == dt and got.shape == exp.shape
        _close(got, exp, dt, _cost_scale(X, False))


@pytest.mark.parametrize("tf,dt", [("swpdall", np.float64), ("swpdall", np.float32), ("acwpdall", np.float64)])
def test_tree_costs_redundant_1d(wx, dt, tf):                     # (ACWT is Float64-only like the reference)
    rng = np.random.default_rng(5)
    wt = wx.wavelet(wx.WT.haar)
    X = np.asfortranarray(wx.to_numpy(getattr(wx, tf)(np.asfortranarray(rng.standard_normal((64, 50)).astype(dt)), wt, 4)))
    exp = lsdb_ref.tree_costs(X, redundant=True)
    got = wx.to_numpy(wx.tree_costs(wx.to_device(X, "cuda:0"), wx.LSDB(redundant=True)))
    assert got.shape == (X.shape[1],)
    _close(got, exp, dt, _cost_scale(X, True))


@pytest.mark.parametrize("dt", [np.float64, np.float32])
@pytest.mark.parametrize("n", [16, 64])
def test_tree_costs_2d(wx, dt, n):
    rng = np.random.default_rng(n)
    wt = wx.wavelet(wx.WT.db2)
    x = np.asfortranarray(rng.standard_normal((n, n, 12)).astype(dt))
    X = np.asfortranarray(wx.to_numpy(wx.wpdall(x, wt, 3)))
    exp = lsdb_ref.tree_costs(X)
    got = wx.to_numpy(wx.tree_costs(wx.to_device(X, "cuda:0"), wx.LSDB()))
    _close(got, exp, dt, _cost_scale(X, False))
    Xs = np.asfortranarray(wx.to_numpy(wx.swpdall(x, wt, 2)))
    exp = lsdb_ref.tree_costs(Xs, redundant=True)
    got = wx.to_numpy(wx.tree_costs(Xs, wx.LSDB(redundant=True)))
    assert got.shape == (Xs.shape[2],)
    _close(got, exp, dt, _cost_scale(Xs, True))


def test_misaligned_device_view(wx):
    import torch
    rng = np.random.default_rng(2)
    X = np.asfortranarray(rng.standard_normal((32, 4, 50)))
    flat = torch.zeros(X.size + 1, dtype=torch.float64, device="cuda:0")
    flat[1:] = torch.from_numpy(X.reshape(-1, order="F")).to("cuda:0")
    view = flat[1:].view(50, 4, 32).permute(2, 1, 0)              # column-major (32, 4, 50) starting 8 bytes in
    got = wx.to_numpy(wx.tree_costs(view, wx.LSDB()))
    _close(got, lsdb_ref.tree_costs(X), np.float64, _cost_scale(X, False))


def test_trees_match_helper(wx):
    wt = wx.wavelet(wx.WT.db4)
    rng = np.random.default_rng(21)
    checked = 0
    for seed in range(6):
        r = np.random.default_rng(seed)
        x = np.cumsum(r.standard_normal((128, 60)), axis=0) + 3 * r.standard_normal((128, 60))
        X = np.asfortranarray(wx.to_numpy(wx.wpdall(np.asfortranarray(x), wt, 5)))
        exp = lsdb_ref.tree_costs(X)
        tree_h, gap = wx.bestbasis_treeselection(exp, 128, return_gap=True)
        if gap <= 1e-8:
            continue
        got = wx.bestbasistree(wx.to_device(X, "cuda:0"), wx.LSDB())
        assert np.array_equal(np.asarray(got), tree_h)
        assert wx.isvalidtree(np.zeros(128), np.asarray(got))
        checked += 1
    assert checked >= 3
    # 2-D: quad-tree selection of the helper's costs
    x = np.asfortranarray(rng.standard_normal((32, 32, 20)))
    X = np.asfortranarray(wx.to_numpy(wx.wpdall(x, wt, 3)))
    exp = lsdb_ref.tree_costs(X)
    got = wx.bestbasistree(X, wx.LSDB())
    assert np.array_equal(np.asarray(got), wx.bestbasis_treeselection(exp, 32, 32))


def test_reference_test_cases(wx):
    # test/bestbasis.jl:35-39 of the reference: Haar, 16-sample signals (5 of them), 16x16 images
    wt = wx.wavelet(wx.WT.haar)
    rng = np.random.default_rng(35)
    x = np.asfortranarray(rng.standard_normal((16, 5)))
    img = np.asfortranarray(rng.standard_normal((16, 16, 5)))
    cases = [(wx.wpdall(x, wt), False, (16,)), (wx.swpdall(x, wt), True, (16,)), (wx.acwpdall(x, wt), True, (16,)),
             (wx.wpdall(img, wt), False, (16, 16)), (wx.swpdall(img, wt), True, (16, 16))]
    for Xw, red, sig in cases:
        Xw = np.asfortranarray(wx.to_numpy(Xw))
        tree = np.asarray(wx.bestbasistree(Xw, wx.LSDB(redundant=red)))
        assert wx.isvalidtree(np.zeros(sig), tree)
        exp = lsdb_ref.tree_costs(Xw, redundant=red)
        assert np.array_equal(tree, wx.bestbasis_treeselection(exp, *sig))


def test_bit_reproducible(wx):
    rng = np.random.default_rng(4)
    X = wx.to_device(np.asfortranarray(rng.standard_normal((256, 7, 30000))), "cuda:0")
    a = wx.to_numpy(wx.tree_costs(X, wx.LSDB()))
    b = wx.to_numpy(wx.tree_costs(X, wx.LSDB()))
    assert a.tobytes() == b.tobytes()
    e1, e2 = wx.to_numpy(wx.lsdb_entropy(X)), wx.to_numpy(wx.lsdb_entropy(X))
    assert e1.tobytes() == e2.tobytes()


def test_argument_errors(wx):
    rng = np.random.default_rng(9)
    good = np.asfortranarray(rng.standard_normal((16, 3, 20)))
    ref = lsdb_ref.tree_costs(good)
    same = np.asfortranarray(np.repeat(rng.standard_normal((16, 3, 1)), 20, axis=2))     # identical signals
    one = np.asfortranarray(rng.standard_normal((16, 3, 1)))
    bad = []
    for v in (np.nan, np.inf, -np.inf):
        b = good.copy(order="F")
        b[5, 1, 7] = v
        bad.append(b)
    for X in [same, one] + bad:
        for inp in (X, wx.to_device(X, "cuda:0")):
            with pytest.raises(wx.ArgumentError) as e:
                wx.tree_costs(inp, wx.LSDB())
            assert "LSDB" in str(e.value)
        with pytest.raises(wx.ArgumentError):
            wx.bestbasistree(X, wx.LSDB())
        _close(wx.tree_costs(good, wx.LSDB()), ref, np.float64, _cost_scale(good, False))
    with pytest.raises(wx.ArgumentError) as e:
        wx.tree_costs(bad[0], wx.LSDB())
    assert "coefficient 6 of column 2" in str(e.value)


def test_one_gib_table(wx):
    import torch
    rng = np.random.default_rng(12)
    n, L, N = 4096, 12, 2520                                        # 4096 x 13 x 2520 Float64 = 1.0 GiB
    X = torch.empty((N, L + 1, n), dtype=torch.float64, device="cuda:0")
    g = torch.Generator(device="cuda:0").manual_seed(5)
    X.normal_(generator=g)
    Xv = X.permute(2, 1, 0)                                         # column-major (n, L + 1, N)
    costs = wx.to_numpy(wx.tree_costs(Xv, wx.LSDB()))
    assert costs.shape == ((1 << (L + 1)) - 1,) and np.isfinite(costs).all()
    E = wx.to_numpy(wx.lsdb_entropy(Xv)).reshape(n * (L + 1), order="F")
    sample = rng.choice(n * (L + 1), 24, replace=False)
    host = np.stack([X[:, int(e) // n, int(e) % n].cpu().numpy() for e in sample])
    _close(E[sample], lsdb_ref.row_entropy(host), np.float64)
    tree = wx.bestbasistree(Xv, wx.LSDB())
    assert wx.isvalidtree(np.zeros(n), np.asarray(tree))
