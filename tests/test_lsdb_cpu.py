"""LSDB best basis without a GPU: the numpy restatement in tests/lsdb_ref.py against the oracle's ASH, Base's range-length
rule on constructed cases, the Python types, and the C entry points in the header and the library."""
import ctypes
import os
import re

import numpy as np
import pytest

import lsdb_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LSDB_SYMBOLS = ["wx_lsdb_entropy_f64", "wx_lsdb_entropy_f32", "wx_lsdb_costs_f64", "wx_lsdb_costs_f32",
                "wx_lsdb_costs2d_f64", "wx_lsdb_costs2d_f32"]


@pytest.mark.parametrize("N", [2, 3, 7, 64, 257, 1000])
def test_helper_density_and_pdf_match_the_oracle(oracle, N):
    rng = np.random.default_rng(N)
    X = rng.standard_normal((3, N))
    _, mbins, _ = lsdb_ref.ash_params(N)
    a, delta, length, _, ok = lsdb_ref.row_grid(X)
    assert ok.all()
    for r in range(3):
        L = int(length[r])
        mine = lsdb_ref.ash_density(X[r], a[r], delta[r], L, mbins)
        ref = oracle.ash_density(X[r], a[r], delta[r], L, mbins)
        np.testing.assert_allclose(mine, ref, rtol=1e-12, atol=1e-14)
        assert abs(mine.sum() * delta[r] - 1.0) < 1e-12
        p = lsdb_ref.ash_pdf(mine, a[r], delta[r], X[r])
        pref = np.array([oracle.ash_pdf(ref, a[r], delta[r], v) for v in X[r]])
        np.testing.assert_allclose(p, pref, rtol=1e-12, atol=1e-14)
        assert (p > 0).all()


def test_ash_parameters():
    # M = 50 (bestbasis_costs.jl:138): the grid has at most 68 points up to 65536 signals and 86 below 4e6
    assert lsdb_ref.ash_params(64) == (5, 10, 60)
    assert lsdb_ref.ash_params(1) == (2, 25, 75)
    assert max(lsdb_ref.ash_params(N)[2] for N in range(2, 65537)) <= 68
    assert max(lsdb_ref.ash_params(N)[2] for N in np.unique(np.geomspace(2, 4e6 - 1, 4000).astype(int))) <= 86


def test_range_length_rule():
    # the fallback length is round(lf) + 1 unless that point overshoots stop; search seeded data for both kinds
    rng = np.random.default_rng(7)
    over = under = 0
    for _ in range(20000):
        start, step = rng.standard_normal(), 10.0 ** rng.uniform(-3, 0)
        n = int(rng.integers(2, 90))
        stop = start + (n - 1) * step * (1 + rng.choice([-1, 1]) * 1e-16 * rng.integers(0, 4))
        lf = (stop - start) / step
        naive = int(round(lf)) + 1
        got = lsdb_ref.range_length(start, step, stop)
        assert not lsdb_ref.rational_branch(start, step, stop)
        if got == naive - 1:
            over += 1
        else:
            assert got == naive
            under += 1
    assert over > 0 and under > 0
    # constructed: 0:0.1:0.3 -- lf = 2.9999999999999996, round + 1 = 4 points, 0 + 3 * 0.1 overshoots 0.3: 3 by the
    # fallback.  Base takes its rational branch here (1/10 is an exact small rational), which the helper reports.
    assert lsdb_ref.range_length(0.0, 0.1, 0.3) == 3
    assert lsdb_ref.rational_branch(0.0, 0.1, 0.3)
    assert lsdb_ref.range_length(0.0, 0.25, 1.0) == 5
    with pytest.raises(ValueError):
        lsdb_ref.range_length(0.0, 0.0, 1.0)


def test_helper_flags_what_the_reference_throws_for():
    X = np.ones((2, 16))
    X[1] = np.arange(16)
    with pytest.raises(lsdb_ref.Degenerate) as e:
        lsdb_ref.row_entropy(X)
    assert list(e.value.rows) == [0]
    for bad in (np.nan, np.inf, -np.inf):
        Y = np.random.default_rng(0).standard_normal((2, 9))
        Y[1, 4] = bad
        with pytest.raises(lsdb_ref.Degenerate):
            lsdb_ref.row_entropy(Y)
    with pytest.raises(lsdb_ref.Degenerate):
        lsdb_ref.row_entropy(np.ones((1, 1)))


def test_helper_node_sums():
    E = np.arange(1.0, 17.0).reshape(8, 2, order="F")          # (n = 8, k = 2)
    c = lsdb_ref.node_costs(E)
    assert c.tolist() == [E[:, 0].sum(), E[:4, 1].sum(), E[4:, 1].sum()]
    c = lsdb_ref.node_costs(E, redundant=True)
    assert c.tolist() == [E[:, 0].sum(), E[:, 1].sum() / 2]
    E2 = np.arange(1.0, 33.0).reshape(4, 4, 2, order="F")        # (n = 4, m = 4, k = 2)
    c = lsdb_ref.node_costs(E2)
    assert c.size == 5 and c[0] == E2[:, :, 0].sum()
    assert sorted(c[1:]) == sorted([E2[:2, :2, 1].sum(), E2[:2, 2:, 1].sum(), E2[2:, :2, 1].sum(), E2[2:, 2:, 1].sum()])
    assert c[1] == E2[:2, :2, 1].sum() and c[2] == E2[:2, 2:, 1].sum() and c[3] == E2[2:, :2, 1].sum()
    c = lsdb_ref.node_costs(E2, redundant=True)
    assert c.tolist() == [E2[:, :, 0].sum(), E2[:, :, 1].sum() / 4]


def test_lsdb_type(wx):
    m = wx.LSDB()
    assert isinstance(m.cost, wx.DifferentialEntropyCost) and m.redundant is False
    assert wx.LSDB(redundant=True).redundant is True
    assert isinstance(wx.LSDB(cost=wx.DifferentialEntropyCost()).cost, wx.DifferentialEntropyCost)
    for bad in (wx.ShannonEntropyCost(), wx.LogEnergyEntropyCost(), wx.LoglpCost(2), wx.NormCost(1)):
        with pytest.raises(TypeError):
            wx.LSDB(cost=bad)
    with pytest.raises(TypeError):                              # the reference has bestbasistreeall for BB only
        wx.bestbasistreeall(np.zeros((8, 4, 3)), wx.LSDB())


def test_lsdb_entry_points_are_declared_and_exported(wx):
    txt = open(os.path.join(ROOT, "include", "waveletsext_hip.h")).read()
    lib = ctypes.CDLL(wx.LIB_PATH)
    for s in LSDB_SYMBOLS:
        assert re.search(r"\bint %s\(" % s, txt), s
        assert hasattr(lib, s), s
