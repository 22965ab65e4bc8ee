"""GPU parity of every launcher behind the lattice factorisation (csrc/wx_lattice.hip: wx_lattice_factor / wx_lattice_factor32) on
the QMF family of tests/qmf_family.py: filters the factorisation declines, filters next to each of its thresholds, ill-conditioned
ones (small gain g, large tangents) and inputs far from unit scale.  Each case is the smallest shape that reaches its launcher,
the batch a few signals off a multiple of the wavefront's signal count (sizes as in tests/test_gpu_lattice*.py).

Every case: the library against the oracle's direct form (C double, or Float32 for Float32 signals) within helpers.TOL, the
inverse of the oracle's coefficients back to x within the same bound, everything finite.  The verdict of wx.lattice_factor for
the case's (filter, L, type) is recorded; both verdicts occur in every launcher group, so the fall-back to the direct-form
kernels is exercised launcher by launcher; where the lattice accepted, the same call under set_force_generic(1) (one level per
launch, no lattice) agrees within the same tolerance.  Scaled inputs (Float32 2^+-40, Float64 2^+-400) run on the same shapes
with db4, its reversal and A(0.05, 0.05), compared relatively."""
import numpy as np
import pytest

import helpers
import qmf_family as QF
from helpers import TOL, relerr

pytestmark = pytest.mark.gpu

SCALED = ("db4", "rev_db4", "A(0.05,0.05)")
NOT_ORTHONORMAL = ("pert_1e-9",)


@pytest.fixture(scope="module")
def members(wx):
    """[(label, qmf, log2 of the input scale per dtype)]: the whole family at unit scale, then the scaled inputs"""
    fam = QF.family(wx)
    fam["db4"] = QF.table_qmf(wx, "db4")
    out = [(name, q, {8: 0, 4: 0}) for name, q in fam.items()]
    for name in SCALED:
        for sign in (1, -1):
            out.append(("%s*2^%s" % (name, "+" if sign > 0 else "-"), fam[name], {8: 400 * sign, 4: 40 * sign}))
    return out


def _input(rng, shape, dt, e):
    return np.asfortranarray(np.ldexp(rng.standard_normal(shape), e).astype(dt))


def _close(got, exp, dt, what):
    got = np.asarray(got)
    assert got.dtype == np.dtype(dt), what
    assert np.all(np.isfinite(got)), what + ("not finite",)
    e = relerr(got, exp)
    assert e <= TOL[np.dtype(dt)], what + (e,)


def _run(wx, members, dt, shape, lat, fwd, inv, ofwd, oinv):
    """fwd / inv: (x, wt) -> array by the library; ofwd / oinv: (x, qmf) -> array by the oracle.  lat = (L, elem_size) the case's
    launcher hands to the factorisation (the tree-driven Float32 kernels apply a wider range than (L, 4): accepted there means
    accepted by them)."""
    es = np.dtype(dt).itemsize
    verdicts = set()
    for i, (label, q, scale) in enumerate(members):
        wt = wx.OrthoFilter(q, label)
        x = _input(np.random.default_rng(1000 + i), shape, dt, scale[es])
        ok = wx.lattice_factor(q, lat[0], elem_size=lat[1]) is not None
        verdicts.add(ok)
        exp = ofwd(x, q)
        got = wx.to_numpy(fwd(x, wt))
        _close(got, exp, dt, (label, "forward", ok))
        back = None
        if inv is not None:
            c = np.asfortranarray(np.asarray(exp, dtype=dt))
            back = wx.to_numpy(inv(c, wt))
            # the inverse of the oracle's coefficients is x -- for an orthonormal filter; pert_1e-9 is not one, and there the
            # library must compute what the oracle's inverse computes with the same vector
            _close(back, oinv(c, q) if label in NOT_ORTHONORMAL else x, dt, (label, "inverse", ok))
        if ok:
            wx.set_force_generic(1)
            try:
                _close(wx.to_numpy(fwd(x, wt)), got, dt, (label, "forward against the general kernels"))
                if inv is not None:
                    _close(wx.to_numpy(inv(c, wt)), back, dt, (label, "inverse against the general kernels"))
            finally:
                wx.set_force_generic(0)
    assert verdicts == {True, False}, verdicts


# ---- 1-D full trees ---------------------------------------------------------------------------------------------------------------
# (n, L, B, L the factorisation sees): 64 / 256 interleaved, 1024, 4096 shallow (_lo), general, full depth (folded inverse from six
# rotations on), 8192 (first level in direct form), 16384 (top levels tiled, then the 4096-sample lattice)
F64_FULL = [(64, 6, 67, 6), (256, 8, 19, 8), (1024, 10, 5, 10), (4096, 3, 3, 3), (4096, 7, 3, 7), (4096, 12, 3, 12),
            (8192, 13, 3, 12), (16384, 14, 5, 12)]


@pytest.mark.parametrize("n,L,B,LW", F64_FULL)
def test_f64_full_trees(wx, oracle, members, n, L, B, LW):
    _run(wx, members, np.float64, (n, B), (LW, 8), lambda x, wt: wx.wptall(x, wt, L), lambda c, wt: wx.iwptall(c, wt, L),
         lambda x, q: oracle.wptall(x, q, L), lambda c, q: oracle.iwptall(c, q, L))


@pytest.mark.parametrize("n,B", [(256, 19), (1024, 5), (4096, 3)])
def test_f64_wpd(wx, oracle, members, n, B):
    L = wx.maxtransformlevels(n)
    _run(wx, members, np.float64, (n, B), (L, 8), lambda x, wt: wx.wpdall(x, wt, L), lambda t, wt: wx.iwpdall(t, wt, L),
         lambda x, q: oracle.wpdall(x, q, L), lambda t, q: oracle.iwpdall(t, q, L))


def _trees(wx, n):
    L = wx.maxtransformlevels(n)
    rng = np.random.default_rng(n)
    t = helpers.random_tree_1d(n, rng, 0.8)
    while not (t[:3].all() and t[3:7].any()):
        t = helpers.random_tree_1d(n, rng, 0.8)
    return [np.asarray(wx.maketree(n, L, "dwt"), dtype=bool), t]


@pytest.mark.parametrize("which", [0, 1], ids=["pyramid", "random"])
@pytest.mark.parametrize("n,B", [(256, 19), (4096, 3), (8192, 3)])
def test_f64_pyramid_and_random_tree(wx, oracle, members, n, B, which):
    tree = _trees(wx, n)[which]
    _run(wx, members, np.float64, (n, B), (min(wx.maxtransformlevels(n), 12), 8), lambda x, wt: wx.wptall(x, wt, tree),
         lambda c, wt: wx.iwptall(c, wt, tree), lambda x, q: oracle.wptall(x, q, tree), lambda c, q: oracle.iwptall(c, q, tree))


def _tree_matrix(wx, n, B):
    rng = np.random.default_rng(B)
    cols = _trees(wx, n) + [np.asarray(wx.maketree(n, wx.maxtransformlevels(n), "full"), dtype=bool)]
    while len(cols) < B:
        t = helpers.random_tree_1d(n, rng, (0.5, 0.7, 0.9)[len(cols) % 3])
        t[0] = True
        cols.append(t)
    return np.asfortranarray(np.stack(cols, axis=1))


@pytest.mark.parametrize("device", [False, True], ids=["host", "device"])
def test_f64_per_signal_trees(wx, oracle, members, device):
    n, B = 256, 19
    trees = _tree_matrix(wx, n, B)
    arg = wx.to_device(trees) if device else trees
    dev = wx.to_device if device else (lambda a: a)                   # device trees go with device data

    def per_signal(fn):
        return lambda a, q: np.stack([fn(a[:, i], q, trees[:, i]) for i in range(B)], axis=-1)
    _run(wx, members, np.float64, (n, B), (8, 8), lambda x, wt: wx.wptall(dev(x), wt, arg), lambda c, wt: wx.iwptall(dev(c), wt, arg),
         per_signal(oracle.wpt), per_signal(oracle.iwpt))


# ---- Float32 1-D: pairs of signals in Float32 arithmetic from 7 levels on, Float64 registers below and at 128 samples -------------
F32_FULL = [(256, 7, 35, 7, 4), (256, 8, 35, 8, 4), (1024, 7, 11, 7, 4), (1024, 10, 11, 10, 4), (4096, 7, 5, 7, 4), (4096, 12, 5, 12, 4),
            (4096, 6, 5, 6, 8), (128, 7, 67, 7, 8)]


@pytest.mark.parametrize("n,L,B,LW,es", F32_FULL)
def test_f32_full_trees(wx, oracle, members, n, L, B, LW, es):
    _run(wx, members, np.float32, (n, B), (LW, es), lambda x, wt: wx.wptall(x, wt, L), lambda c, wt: wx.iwptall(c, wt, L),
         lambda x, q: oracle.wptall(x, q, L), lambda c, q: oracle.iwptall(c, q, L))


def test_f32_random_tree(wx, oracle, members):
    """the tree-driven kernels normalise every level: the range of one level, the conditioning of all 8"""
    n, B = 256, 35
    tree = _trees(wx, n)[1]
    _run(wx, members, np.float32, (n, B), (8, 4), lambda x, wt: wx.wptall(x, wt, tree), lambda c, wt: wx.iwptall(c, wt, tree),
         lambda x, q: oracle.wptall(x, q, tree), lambda c, q: oracle.iwptall(c, q, tree))


# ---- 2-D ------------------------------------------------------------------------------------------------------------------------
def _o2(fn, *args):
    """the oracle image by image; Float32 images in Float64, as tests/test_gpu_lattice2d64.py holds them"""
    return lambda x, q: np.stack([fn(x[..., b].astype(np.float64), q, *args) for b in range(x.shape[-1])], axis=-1)


@pytest.mark.parametrize("dt", [np.float64, np.float32])
@pytest.mark.parametrize("L", [6, 3])
def test_64x64_full_quad_trees(wx, oracle, members, dt, L):
    _run(wx, members, dt, (64, 64, 5), (2 * L, np.dtype(dt).itemsize), lambda x, wt: wx.wptall(x, wt, L),
         lambda c, wt: wx.iwptall(c, wt, L), _o2(oracle.wpt, L), _o2(oracle.iwpt, L))


@pytest.mark.parametrize("dt", [np.float64, np.float32])
def test_64x64_quad_tree(wx, oracle, members, dt):
    tree = helpers.random_tree_2d(64, 64, np.random.default_rng(64), p=0.7)
    tree[:5] = True
    _run(wx, members, dt, (64, 64, 5), (6, 8) if dt == np.float64 else (12, 4), lambda x, wt: wx.wptall(x, wt, tree),
         lambda c, wt: wx.iwptall(c, wt, tree), _o2(oracle.wpt, tree), _o2(oracle.iwpt, tree))


@pytest.mark.parametrize("dt", [np.float64, np.float32])
def test_64x64_wpd(wx, oracle, members, dt):
    L = 6
    _run(wx, members, dt, (64, 64, 3), (2 * L, np.dtype(dt).itemsize), lambda x, wt: wx.wpdall(x, wt, L),
         lambda t, wt: wx.iwpdall(t, wt, L), _o2(oracle.wpd, L), _o2(oracle.iwpd, L))


def test_128x128_row_pass(wx, oracle, members):
    _run(wx, members, np.float64, (128, 128, 3), (3, 8), lambda x, wt: wx.wptall(x, wt, 3), lambda c, wt: wx.iwptall(c, wt, 3),
         _o2(oracle.wpt, 3), _o2(oracle.iwpt, 3))


def test_256x256_f32_full_depth(wx, oracle, members):
    _run(wx, members, np.float32, (256, 256, 3), (16, 4), lambda x, wt: wx.wptall(x, wt, 8), lambda c, wt: wx.iwptall(c, wt, 8),
         _o2(oracle.wpt, 8), _o2(oracle.iwpt, 8))


# ---- denoiseall in one pass -----------------------------------------------------------------------------------------------------
def test_denoiseall_one_pass(wx, oracle, members):
    """Float64, 256 samples: accepted filters give what the general kernels give (set_force_generic(1)) and what the oracle
    gives; declined ones must run at all, and give what the oracle gives"""
    n, B = 256, 53
    t = np.linspace(0, 1, n)
    base = 4 * np.sin(4 * np.pi * t) - np.sign(t - 0.3) - np.sign(0.72 - t)
    verdicts = set()
    for i, (label, q, scale) in enumerate(members):
        wt = wx.OrthoFilter(q, label)
        x = np.asfortranarray(np.ldexp(base[:, None] + 0.5 * np.random.default_rng(i).standard_normal((n, B)), scale[8]))
        ok = wx.lattice_factor(q, 8) is not None
        verdicts.add(ok)
        y = wx.to_numpy(wx.denoiseall(x, "sig", wt))
        assert y.shape == (n, B) and np.all(np.isfinite(y)), label
        exp = np.stack([oracle.denoise(x[:, b], "sig", q, th="hard", t=float(np.sqrt(2 * np.log(n)))) for b in range(B)], axis=-1)
        e = relerr(y, exp)
        assert e <= TOL[np.dtype(np.float64)], (label, ok, e)
        if ok:
            wx.set_force_generic(1)
            try:
                yg = wx.to_numpy(wx.denoiseall(x, "sig", wt))
            finally:
                wx.set_force_generic(0)
            e = relerr(y, yg)
            assert e <= TOL[np.dtype(np.float64)], (label, "against the general kernels", e)
    assert verdicts == {True, False}
