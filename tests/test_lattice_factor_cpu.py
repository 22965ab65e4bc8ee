"""CPU checks of the host factorisation every lattice launcher goes through (csrc/wx_lattice.hip: wx_lattice_factor and
wx_lattice_factor32, through the hook wx_debug_lattice_factor = wx.lattice_factor): the verdicts on the QMF family of
tests/qmf_family.py, the coefficients against tools/lattice_proto.py, and the Float32 window against a Float32 emulation of
the unnormalised lattice -- the recurrences the kernels run -- on unit-scale and on scaled inputs."""
import numpy as np
import pytest

import qmf_family as QF
from helpers import TOL

LD = np.longdouble
DEPTHS = (1, 3, 6, 7, 10, 12, 13)
F32_WINDOW_LOG2 = -50.0          # wx_lattice.hip, lat_window: Float32 arithmetic needs (LW + 1) log2 |g| >= -50
F32_COND = 1000.0                # ... and LT sum_j (1 + t_j^2) <= 1000


@pytest.fixture(scope="module")
def fam(wx):
    f = QF.family(wx)
    for n in QF.TABLE:
        f[n] = QF.table_qmf(wx, n)
    return f


def _proto(q):
    """(t, g, min |c|) of tools/lattice_proto.lattice_factor, or None where its own checks fail"""
    from tools.lattice_proto import lattice_factor
    if q.size // 2 > 10:
        return None
    try:
        with np.errstate(all="ignore"):
            t, g = lattice_factor(q)
    except AssertionError:
        return None
    if not np.all(np.isfinite(t)):
        return None
    return t, g, float(1 / np.sqrt(1 + np.abs(t).max() ** 2))


def test_the_family_is_orthonormal(fam):
    """sum q = sqrt(2), sum q^2 = 1 and the double-shift orthogonality, for every member built from angles and every reversal"""
    for name, q in fam.items():
        if name.startswith("pert") or name.startswith("pad"):
            continue
        assert abs(q.sum() - np.sqrt(2)) <= 4e-15, name
        for k in range(q.size // 2):
            d = float(np.dot(q[2 * k:], q[:q.size - 2 * k]))
            assert abs(d - (k == 0)) <= 4e-15, (name, k, d)


def test_named_cases_accept_and_decline(wx, fam):
    """Float64: every named case is accepted or declined as tests/qmf_family.py lists it; a member without a listed verdict
    follows the rule of the routine: every |c_j| >= 1e-3 and g^L inside 1e+-60"""
    seen = set()
    for name, q in fam.items():
        pr = _proto(q)
        for L in DEPTHS:
            got = wx.lattice_factor(q, L) is not None
            exp = QF.expected_f64(name, L)
            if exp is None:
                assert pr is not None, name
                exp = pr[2] >= 1e-3 and 1e-60 < abs(pr[1]) ** L < 1e60
            assert got == exp, (name, L, got, exp, pr and (pr[1], pr[2]))
            assert (wx.lattice_factor(q, L, inverse=True) is not None) == got, (name, L)
            seen.add(got)
    assert seen == {True, False}


def test_every_decline_branch_is_taken(wx, fam):
    """one member per reason, so that no branch of the routine goes untested: quarter turn, zero leading matrix, not
    paraunitary, gain outside the window, more rotations than the kernels have"""
    for name, L in (("A(0.0009,0.5)", 1), ("rev_db10", 1), ("pad_both", 1), ("pad_front", 1), ("pert_1e-9", 1),
                    ("A(0.004,0.004)", 13), ("rand22", 1), ("rand64", 1)):
        assert wx.lattice_factor(fam[name], L) is None, (name, L)
    for name, L in (("A(0.0011,0.5)", 12), ("rev_db9", 12), ("pert_1e-15", 12), ("A(0.004,0.004)", 12), ("rand20", 12)):
        assert wx.lattice_factor(fam[name], L) is not None, (name, L)
    # the thresholds themselves, from the angles: min |c| = sin(eps) = 1.1e-3 against 9e-4
    assert abs(np.cos(QF.angles_a(0.0011, 0.5)[0]) - 1.1e-3) < 1e-8 and abs(np.cos(QF.angles_a(0.0009, 0.5)[0]) - 9e-4) < 1e-8
    g = QF.gain(QF.angles_a(0.004, 0.004))
    assert abs(g) ** 12 > 1e-60 > abs(g) ** 13


def test_accepted_coefficients_agree_with_the_prototype(wx, fam):
    """p, kap, g0, g2 recomputed in long double from the prototype's tangents"""
    n = 0
    for name, q in fam.items():
        for L in (1, 7, 12):
            for inv in (False, True):
                lf = wx.lattice_factor(q, L, inverse=inv)
                if lf is None:
                    continue
                t, g, _ = _proto(q)
                t = t.astype(LD)
                sig, p, kap = LD(1), [], []
                for tj in t:
                    c2 = 1 / (1 + tj * tj)
                    p.append(tj / sig)
                    kap.append(sig * tj * c2)
                    sig = sig * c2
                gl = np.prod(1 / np.sqrt(1 + t * t))            # |g| from the tangents, the sign from the prototype
                gl = gl if g > 0 else -gl
                for got, exp in ((lf.p, np.array(p)), (lf.kap, np.array(kap)), (lf.g0, gl ** (-L if inv else L)),
                                 (lf.g2, gl ** (2 if inv else -2))):
                    err = np.abs(np.asarray(got, dtype=LD) - exp) / np.abs(exp)
                    assert np.all(err <= 1e-12), (name, L, inv, got, exp)
                n += 1
    assert n > 100


def _g(wx, q):
    lf = wx.lattice_factor(q, 1)
    return None if lf is None else lf.g0


def test_float32_window(wx, fam):
    """whenever the hook accepts for Float32 arithmetic, the Float64 window holds as well, g^(+-L) lies inside the window of
    csrc/wx_lattice.hip -- (L + 1) log2 |g| >= -50, hence 2^50.5 |g|^-L < 2^127 -- and the shears are well enough conditioned
    for it, L sum (1 + t_j^2) <= 1000; and it declines exactly the rest, each of the two rules alone deciding somewhere"""
    seen, by_rule = set(), set()
    for name, q in fam.items():
        g = _g(wx, q)
        for L in range(1, 25):
            a4 = wx.lattice_factor(q, L, elem_size=4) is not None
            a8 = wx.lattice_factor(q, L, elem_size=8) is not None
            if g is None:
                assert not a4 and not a8, (name, L)
                continue
            cond = float(np.sum(1 + _proto(q)[0].astype(LD) ** 2))
            in_range = (L + 1) * np.log2(abs(g)) >= F32_WINDOW_LOG2
            in_cond = L * cond <= F32_COND
            if abs(L * cond - F32_COND) < 1e-6 * F32_COND:
                continue                                                # on the threshold to rounding: either verdict
            assert a4 == (a8 and in_range and in_cond), (name, L, a4, a8, g, cond)
            if a4:
                assert 50.5 - L * np.log2(abs(g)) < 127 and abs(g) ** (L + 1) >= 2.0 ** -50
            seen.add((a4, a8))
            by_rule.add((in_range, in_cond))
    assert seen == {(True, True), (False, True), (False, False)}
    assert by_rule == {(True, True), (True, False), (False, True), (False, False)}


# ---- the lattice as the kernels run it: unnormalised shears, one gain per leaf at the end (forward) or at the start (inverse) ----
def _leaf_perm(n, L):
    from tools.lattice_proto import out_perm
    return out_perm(n, L)


def _leaf_gain(n, L, g0, g2):
    k = np.zeros(n, dtype=np.int64)
    p = np.arange(n)
    for b in range(L):
        k += (p >> b) & 1
    return np.float64(g0) * np.float64(g2) ** k                 # Float64 on the device as well (lat_gains), rounded to the type after


def _ftz(a):
    if a.dtype == np.float32:                                    # a flushed subnormal: the worst the device may do
        a[np.abs(a) < np.float32(2.0 ** -126)] = 0
    return a


def emu(x, lf, L, dtype, inverse):
    """full tree of depth L on x (n = len(x) a multiple of 2^L): u += p_j w, w -= kap_j u, advance (lattice_proto.level_fwd in
    the shear form of wx_lattice_dev.h), every operation rounded to dtype"""
    n = x.size
    p, kap = lf.p.astype(dtype), lf.kap.astype(dtype)
    J = p.size - 1
    perm = _leaf_perm(n, L)
    with np.errstate(all="ignore"):
        gain = _leaf_gain(n, L, lf.g0, lf.g2).astype(dtype)
        if not inverse:
            y = x.astype(dtype)
            for b in range(L):
                v = y.reshape(n >> (b + 1), 2, 1 << b)
                u, w = v[:, 0, :].copy(), v[:, 1, :].copy()
                for j in range(J + 1):
                    u = _ftz(u + _ftz(p[j] * w))
                    w = _ftz(w - _ftz(kap[j] * u))
                    if j < J:
                        w = np.roll(w, -1, axis=0)
                v[:, 0, :], v[:, 1, :] = u, np.roll(w, J, axis=0)
            out = np.empty_like(y)
            out[perm] = _ftz(y * gain)
            return out
        y = _ftz(x.astype(dtype)[perm] * gain)
        for b in range(L - 1, -1, -1):
            v = y.reshape(n >> (b + 1), 2, 1 << b)
            u, w = v[:, 0, :].copy(), np.roll(v[:, 1, :], -J, axis=0)
            for j in range(J, -1, -1):
                w = _ftz(w + _ftz(kap[j] * u))
                u = _ftz(u - _ftz(p[j] * w))
                if j > 0:
                    w = np.roll(w, 1, axis=0)
            v[:, 0, :], v[:, 1, :] = u, w
        return y


def reference(x, q, L, inverse):
    """the normalised lattice (rotations c [[1, t], [-t, 1]]) in long double from the prototype's tangents"""
    t, g, _ = _proto(q)
    t = t.astype(LD)
    c = 1 / np.sqrt(1 + t * t)
    sgn = LD(1 if g > 0 or L % 2 == 0 else -1)
    J = t.size - 1
    n = x.size
    perm = _leaf_perm(n, L)
    if not inverse:
        y = x.astype(LD)
        for b in range(L):
            v = y.reshape(n >> (b + 1), 2, 1 << b)
            u, w = v[:, 0, :].copy(), v[:, 1, :].copy()
            for j in range(J + 1):
                u, w = c[j] * (u + t[j] * w), c[j] * (w - t[j] * u)
                if j < J:
                    w = np.roll(w, -1, axis=0)
            v[:, 0, :], v[:, 1, :] = u, np.roll(w, J, axis=0)
        out = np.empty_like(y)
        out[perm] = y * sgn
        return out
    y = x.astype(LD)[perm] * sgn
    for b in range(L - 1, -1, -1):
        v = y.reshape(n >> (b + 1), 2, 1 << b)
        u, w = v[:, 0, :].copy(), np.roll(v[:, 1, :], -J, axis=0)
        for j in range(J, -1, -1):
            u, w = c[j] * (u - t[j] * w), c[j] * (w + t[j] * u)
            if j > 0:
                w = np.roll(w, 1, axis=0)
        v[:, 0, :], v[:, 1, :] = u, w
    return y


def _rel(a, b):
    b = np.asarray(b, dtype=LD)
    return float(np.abs(np.asarray(a, dtype=LD) - b).max() / np.abs(b).max())


def test_reference_lattice_is_the_oracle_transform(wx, oracle, fam):
    """the long-double lattice the emulation is held to computes what the oracle's direct form computes"""
    x = np.random.default_rng(5).standard_normal(256)
    for name in ("db4", "rev_db4", "coif2", "rev_db9", "A(0.02,0.02)", "rand18"):
        q = fam[name]
        ref = oracle.wpt(x, q, 6)
        assert _rel(reference(x, q, 6, False), ref) <= 1e-13, name
        assert _rel(reference(ref, q, 6, True), x) <= 1e-13, name


EMU_DEPTHS = (2, 4, 6, 7, 9, 10, 11, 12)
SCALES = (0, 40, -40)


def test_float32_emulation_on_every_accepted_filter(wx, fam):
    """Float32 arithmetic, every (filter, L) the Float32 window accepts, input of unit scale and scaled by 2^+-40: finite and
    within helpers.TOL of the long-double lattice, forward and inverse.  This is what the GPU parity test asks of the kernels,
    and it pins the window without a GPU: with the Float64 window (1e+-60) applied to Float32 arithmetic, A(0.02,0.02) at
    L = 12 (g^12 = 2.2e-42) returns NaN."""
    tol = TOL[np.dtype(np.float32)]
    rng = np.random.default_rng(11)
    ran = 0
    for name, q in fam.items():
        for L in EMU_DEPTHS:
            lf = wx.lattice_factor(q, L, elem_size=4)
            lfi = wx.lattice_factor(q, L, inverse=True, elem_size=4)
            assert (lf is None) == (lfi is None)
            if lf is None:
                continue
            x0 = rng.standard_normal(1 << L)
            for s in SCALES:
                x = np.ldexp(x0, s).astype(np.float32)
                ref = reference(x, q, L, False)
                got = emu(x, lf, L, np.float32, False)
                assert np.all(np.isfinite(got)), (name, L, s)
                e1 = _rel(got, ref)
                w = ref.astype(np.float32)
                back = emu(w, lfi, L, np.float32, True)
                assert np.all(np.isfinite(back)), (name, L, s)
                e2 = _rel(back, reference(w, q, L, True))
                assert e1 <= tol and e2 <= tol, (name, L, s, e1, e2)
            ran += 1
    assert ran >= 60


def test_float64_emulation_at_the_edges_of_its_window(wx, fam):
    """Float64 registers on the worst accepted members at L = 12, unit scale and 2^+-400: within helpers.TOL"""
    tol = TOL[np.dtype(np.float64)]
    x0 = np.random.default_rng(12).standard_normal(4096)
    for name in ("A(0.004,0.004)", "A(0.0011,0.5)", "rev_db9", "rev_coif6", "rev_db8", "rand20"):
        q = fam[name]
        lf, lfi = wx.lattice_factor(q, 12), wx.lattice_factor(q, 12, inverse=True)
        assert lf is not None and lfi is not None, name
        for s in (0, 400, -400):
            x = np.ldexp(x0, s)
            ref = reference(x, q, 12, False)
            got = emu(x, lf, 12, np.float64, False)
            back = emu(ref.astype(np.float64), lfi, 12, np.float64, True)
            assert np.all(np.isfinite(got)) and np.all(np.isfinite(back)), (name, s)
            e1, e2 = _rel(got, ref), _rel(back, x)
            assert e1 <= tol and e2 <= tol, (name, s, e1, e2)
