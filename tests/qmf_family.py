"""Orthonormal QMFs for the lattice tests, built from rotation angles, and the named cases around the thresholds of the host
factorisation (csrc/wx_lattice.hip: wx_lattice_factor).  Plain module: no fixtures, no GPU, no library.

    R(th) = [[cos th, sin th], [-sin th, cos th]],  P_0 = R(th_0),  P_j(w) = R(th_j) diag(1, w) P_{j-1}(w)
    q[2m], q[2m+1] = the w^m coefficients of P_J[0][0], P_J[0][1]

With sum th_j = pi/4 the filter has sum q = sqrt(2) and sum q^2 = 1, and the factorisation gives back t_j = tan th_j, so the
gain of one level is g = prod cos th_j.  Everything is computed in np.longdouble and rounded once."""
import numpy as np

LD = np.longdouble
PI = LD(np.pi) + LD(1.2246467991473532e-16)           # pi to the long double's precision (double-double split)

TABLE = ["haar", "db2", "db3", "db4", "db5", "db6", "db7", "db8", "db9", "db10", "coif2", "coif4", "coif6"]
RAND_F = [6, 10, 14, 18, 20, 22, 64]
LATTICE_MAX_F = 20                                     # 10 rotations: longer filters are beyond the lattice kernels


def qmf_from_angles(theta):
    th = np.asarray(theta, dtype=LD)
    J = th.size - 1
    P = np.zeros((J + 1, 2, 2), dtype=LD)

    def rot(a):
        return np.array([[np.cos(a), np.sin(a)], [-np.sin(a), np.cos(a)]], dtype=LD)

    P[0] = rot(th[0])
    for j in range(1, J + 1):
        S = np.zeros_like(P)
        S[:, 0, :] = P[:, 0, :]                        # diag(1, w): the second row moves up one power of w
        S[1:, 1, :] = P[:-1, 1, :]
        P = np.einsum("ij,mjk->mik", rot(th[j]), S)
    q = np.empty(2 * (J + 1), dtype=LD)
    q[0::2] = P[:, 0, 0]
    q[1::2] = P[:, 0, 1]
    return q.astype(np.float64)


def angles_a(e1, e2):
    """A(e1, e2): two rotations e1, e2 short of a quarter turn, 8 taps"""
    th = [PI / 2 - LD(e1), LD(0.3), -(PI / 2 - LD(e2))]
    th.append(PI / 4 - sum(th))
    return np.array(th, dtype=LD)


def angles_rand(F, seed=None):
    """F / 2 seeded angles in [-1.2, 1.2], the last one fixing the sum at pi / 4 (mod pi: R(th + pi) = -R(th), taken out so that
    the filter keeps sum q = sqrt(2))"""
    rng = np.random.default_rng(1000 + F if seed is None else seed)
    th = rng.uniform(-1.2, 1.2, F // 2).astype(LD)
    last = PI / 4 - th[:-1].sum()
    th[-1] = last - 2 * PI * np.round(last / (2 * PI))
    return th


def gain(theta):
    return float(np.prod(np.cos(np.asarray(theta, dtype=LD))))


def table_qmf(wx, name):
    return np.asarray(wx.wavelet(getattr(wx.WT, name)).qmf, dtype=np.float64)


def pert(q, delta, seed=7):
    r = np.random.default_rng(seed).standard_normal(q.size)
    return q + delta * r / np.linalg.norm(r)


A_CASES = [(0.05, 0.05), (0.02, 0.02), (0.004, 0.004), (0.0011, 0.5), (0.0009, 0.5)]


def family(wx):
    """name -> QMF (Float64) of every member"""
    fam = {}
    for n in TABLE:
        fam["rev_" + n] = table_qmf(wx, n)[::-1].copy()
    for e1, e2 in A_CASES:
        fam["A(%g,%g)" % (e1, e2)] = qmf_from_angles(angles_a(e1, e2))
    db2 = table_qmf(wx, "db2")
    fam["pad_both"] = np.concatenate([[0.0, 0.0], db2, [0.0, 0.0]])
    fam["pad_front"] = np.concatenate([[0.0, 0.0], db2])
    fam["pert_1e-15"] = pert(table_qmf(wx, "db4"), 1e-15)
    fam["pert_1e-9"] = pert(table_qmf(wx, "db4"), 1e-9)
    for F in RAND_F:
        fam["rand%d" % F] = qmf_from_angles(angles_rand(F))
    return fam


# The Float64 verdict of wx_lattice_factor at depth L for the named cases (None: not pinned by name -- the reversed table
# filters, whose verdict follows from their gain, are checked against it in tests/test_lattice_factor_cpu.py).
def expected_f64(name, L):
    if name in ("pad_both", "pad_front", "pert_1e-9", "A(0.0009,0.5)", "rand22", "rand64", "rev_db10"):
        return False                                   # zero leading matrix; not paraunitary; |c| < 1e-3; beyond 10 rotations
    if name == "A(0.004,0.004)":
        return L <= 12                                 # g^12 = 3.7e-59, g^13 = 4.6e-64: outside 1e+-60
    if name in ("A(0.05,0.05)", "A(0.02,0.02)", "A(0.0011,0.5)", "pert_1e-15", "rev_db4", "rev_db8", "rev_db9", "rev_coif6"):
        return True if L <= 12 else None
    if name.startswith("rand"):
        return True if L <= 12 else None
    return None
