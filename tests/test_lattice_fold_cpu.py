"""CPU checks of the fold of the deepest lattice levels (csrc/wx_lattice_fold.h): the node matrices of the host routine and of
the emulation against the level recurrences they replace, and the folded emulation against the oracle."""
import numpy as np
import pytest

FILTERS = ["db5", "db6", "db7", "db8", "db10"]
KS = {2: (5,), 4: (5, 4), 8: (5, 4, 3)}                    # lat_level<K, 0, NS, .> that a node of NF registers is closed under


def _shears(wx, wname):
    from tools.lattice_emu import shear_coefs
    from tools.lattice_proto import lattice_factor
    q = np.asarray(wx.wavelet(getattr(wx.WT, wname)).qmf, dtype=np.float64)
    t, g1 = lattice_factor(q)
    return q, shear_coefs(t), g1


def _composite(sh, nf, inv, rng):
    """random registers of 3 lanes through the recurrences of tools/lattice_emu.py::level, in long double"""
    import tools.lattice_emu as E
    x = rng.standard_normal((64, 3)).astype(np.longdouble)
    y = x.copy()
    saved = E.LANES
    E.LANES = np.arange(3)
    try:
        for K in (KS[nf] if inv else KS[nf][::-1]):
            E.level(y, K, 0, (sh[0].astype(np.longdouble), sh[1].astype(np.longdouble)), inv)
    finally:
        E.LANES = saved
    return x, y


@pytest.mark.parametrize("inv", [True, False])
@pytest.mark.parametrize("nf", [2, 4, 8])
@pytest.mark.parametrize("wname", FILTERS)
def test_node_matrix_equals_the_level_recurrences(wx, wname, nf, inv):
    """the host routine (wx_lattice_fold_matrix through wx_debug_lattice_fold) and the emulation's fold_matrix: applied to the
    groups {s + (64 / NF) j} of random registers they give what the two or three lat_level recurrences give, to 1e-14"""
    from tools.lattice_emu import fold_matrix
    q, sh, _ = _shears(wx, wname)
    x, y = _composite(sh, nf, inv, np.random.default_rng(nf))
    G = 64 // nf
    for name, M in (("host", wx.lattice_fold_matrix(q, nf, inverse=inv)), ("emulation", fold_matrix(sh, nf, inv))):
        assert M is not None and M.shape == (nf, nf), name
        got = np.empty_like(x)
        for s in range(G):
            got[s::G] = M.astype(np.longdouble) @ x[s::G]
        err = float(np.abs(got - y).max() / np.abs(y).max())
        print(wname, nf, inv, name, "max |M| %.3g" % np.abs(M).max(), "err %.2e" % err)
        assert err <= 1e-14, (name, err)


@pytest.mark.parametrize("nf", [2, 4, 8])
@pytest.mark.parametrize("wname", FILTERS)
def test_folded_emulation_matches_oracle(wx, oracle, wname, nf):
    """iwpt_emu with the fold (the same matrix on the same register groups as k_lat_iwpt12_f64) at n = 4096, L = 12; wpt_emu has no
    fold to apply: the forward kernel does not fold (it spills at three wavefronts per SIMD)"""
    from tools.lattice_emu import iwpt_emu, wpt_emu
    q, sh, g1 = _shears(wx, wname)
    x = np.random.default_rng(12).standard_normal(4096)
    ref = oracle.wpt(x, q, 12)
    plain = iwpt_emu(ref, sh, g1, 12)
    folded = iwpt_emu(ref, sh, g1, 12, fold=nf)
    assert not np.array_equal(plain, folded)                           # the fold ran
    assert np.abs(folded - x).max() <= 1e-12 * np.abs(x).max()
    assert np.abs(wpt_emu(x, sh, g1, 12) - ref).max() <= 1e-12 * np.abs(ref).max()


def test_a_declined_fold_takes_the_unfolded_path(wx, oracle, monkeypatch):
    """filters of fewer than six rotations do not fold (host: no matrix; emulation: bit-identical to the unfolded run), depths
    below 12 neither, and a matrix the builder declines (an entry out of range) leaves the lattice levels in place"""
    import tools.lattice_emu as E
    for wname in ("haar", "db2", "db4"):
        q, sh, g1 = _shears(wx, wname)
        assert wx.lattice_fold_matrix(q, 8) is None and wx.lattice_fold_matrix(q, 4, inverse=False) is None
        w = np.random.default_rng(3).standard_normal(4096)
        assert np.array_equal(E.iwpt_emu(w, sh, g1, 12, fold=8), E.iwpt_emu(w, sh, g1, 12))
    q, sh, g1 = _shears(wx, "db8")
    w = np.random.default_rng(4).standard_normal(4096)
    assert np.array_equal(E.iwpt_emu(w, sh, g1, 11, fold=8), E.iwpt_emu(w, sh, g1, 11))
    assert not np.array_equal(E.iwpt_emu(w, sh, g1, 12, fold=8), E.iwpt_emu(w, sh, g1, 12))
    assert E.fold_matrix((sh[0] * 1e8, sh[1]), 8, True) is None       # entries beyond 1e30: declined
    monkeypatch.setattr(E, "fold_matrix", lambda t, NF, inv: None)
    assert np.array_equal(E.iwpt_emu(w, sh, g1, 12, fold=8), E.iwpt_emu(w, sh, g1, 12))
