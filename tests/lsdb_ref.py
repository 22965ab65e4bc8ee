"""numpy restatement of the reference's LSDB costs, the yardstick of tests/test_lsdb_cpu.py and tests/test_gpu_lsdb.py.

coefcost(x::Vector, DifferentialEntropyCost()) bestbasis/bestbasis_costs.jl:135-155 for every row of X seen as (nk, N),
vectorised over the rows; the node sums of tree_costs(X, LSDB(redundant)) bestbasis_tree.jl:104-147 for the four
geometries.  Two rules are restated from outside the reference tree (Julia Base's float range length and
AverageShiftedHistograms.jl's ash / pdf, neither of which is available here), in the same words as
csrc/wx_lsdb.hip: parity with them is unpinned.  The bin of an observation uses the division of the published rule,
floor((y - a) / step + 1.5), where oracle.ash_density multiplies by 1 / step: the two agree except for values within an
ulp of a bin edge.
"""
import math
from fractions import Fraction

import numpy as np

M = 50                                     # bestbasis_costs.jl:138 ("arbitrary large number M"; LDB uses 100)


def ash_params(N):
    """nbins, mbins and the largest grid length (nbins + 1) mbins of a row of N values (bestbasis_costs.jl:140-141)"""
    nbins = int(math.ceil((30 * N) ** (1 / 5)))
    mbins = -(-M // nbins)
    return nbins, mbins, (nbins + 1) * mbins


def range_length(start, step, stop):
    """length(start:step:stop) for Float64 by Base's fallback rule: lf = (stop - start) / step, len = round(lf) + 1
    (ties to even), minus one if start + (len - 1) step overshoots stop."""
    if step == 0:
        raise ValueError("range step cannot be zero")
    lf = (stop - start) / step
    if lf < 0:
        return 0
    if lf == 0:
        return 1
    n = int(round(lf)) + 1
    stopp = start + (n - 1) * step
    n -= int(start < stop < stopp) + int(start > stop > stopp)
    return n


def _rat(x):
    """Base.rat(x::Float64): continued-fraction approximation with |numerator|, |denominator| <= maxintfloat(Float32)"""
    y, a, b, c, d = x, 1, 0, 0, 1
    m = 16777216.0
    while abs(y) <= m:
        f = int(y)
        y -= f
        a, c = f * a + c, a
        b, d = f * b + d, b
        if max(abs(a), abs(b)) > m:
            return c, d
        if b != 0 and a / b == x:
            break
        if y == 0:
            break
        y = 1.0 / y
    return a, b


def rational_branch(start, step, stop):
    """True if Base's (:)(start, step, stop) for Float64 would take its rational branch instead of the fallback (its
    first conditions: exact small-rational forms of all three and a representable common denominator)."""
    sn, sd = _rat(step)
    if sd == 0 or sn / sd != step:
        return False
    an, ad = _rat(start)
    on, od = _rat(stop)
    if ad == 0 or od == 0 or an / ad != start or on / od != stop:
        return False
    den = ad * sd // math.gcd(ad, sd)
    return den != 0 and abs(start * den) <= 2.0 ** 53 and abs(step * den) <= 2.0 ** 53


class Degenerate(ValueError):
    """A row the reference throws for (max == min, N == 1, non-finite values): `rows` lists them."""

    def __init__(self, rows):
        super().__init__("degenerate rows %s" % list(rows[:8]))
        self.rows = rows


def _rn_sqrt(v):
    """the double nearest to sqrt(v) for an exact non-negative Fraction v"""
    if v == 0:
        return 0.0
    c = math.sqrt(float(v))
    while True:
        up, dn = math.nextafter(c, math.inf), math.nextafter(c, 0.0)
        mu, md = (Fraction(c) + Fraction(up)) / 2, (Fraction(c) + Fraction(dn)) / 2
        if mu * mu < v:
            c = up
        elif md * md > v:
            c = dn
        else:
            return c


def exact_std(x):
    """std(x) (corrected) of the exact values of a finite row, correctly rounded to Float64: the definition the library
    computes (double-double sums), within an ulp or two of Julia's two-pass std"""
    fr = [Fraction(v) for v in np.asarray(x, dtype=np.float64).tolist()]
    n = len(fr)
    S, Q = sum(fr), sum(f * f for f in fr)
    return _rn_sqrt((Q - S * S / n) / (n - 1))


def row_grid(X):
    """(a, delta, length, stop) per row of X (nk, N), the Float32 / Float64 rules of bestbasis_costs.jl:143-146"""
    X = np.asarray(X)
    N = X.shape[1]
    _, _, len0 = ash_params(N)
    x64 = X.astype(np.float64)
    fin = np.isfinite(x64).all(axis=1)
    sigma = np.array([exact_std(x64[r]) if fin[r] and N >= 2 else np.nan for r in range(X.shape[0])])
    if X.dtype == np.float32:
        mn, mx = X.min(axis=1), X.max(axis=1)
        sf = sigma.astype(np.float32)
        with np.errstate(invalid="ignore", over="ignore"):
            delta = (((mx - mn) + sf) / np.float32(len0 - 1)).astype(np.float64)
        s64 = sf.astype(np.float64)
        a, stop = mn.astype(np.float64) - 0.5 * s64, mx.astype(np.float64) + 0.5 * s64
    else:
        mn, mx = X.min(axis=1), X.max(axis=1)
        with np.errstate(invalid="ignore", over="ignore"):
            delta = (mx - mn + sigma) / float(len0 - 1)
        a, stop = mn - 0.5 * sigma, mx + 0.5 * sigma
    with np.errstate(invalid="ignore"):
        ok = np.isfinite(sigma) & fin & (mx > mn) & (delta > 0) & np.isfinite(delta) & (N >= 2)
    length = np.zeros(X.shape[0], dtype=np.int64)
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        lf = (stop - a) / delta
        ln = np.where(ok, np.rint(np.where(ok, lf, 0.0)), 0.0).astype(np.int64) + 1
        stopp = a + (ln - 1) * delta
    ln -= ((a < stop) & (stop < stopp)).astype(np.int64)
    length[ok] = ln[ok]
    return a, delta, length, stop, ok


def ash_density(x, a, delta, length, m):
    """density of ash(x, rng = a:delta:..., m = m, kernel = triangular) with `length` grid points (one row)"""
    ki = np.floor((np.asarray(x, dtype=np.float64) - a) / delta + 1.5).astype(np.int64)
    ki = ki[(ki >= 1) & (ki <= length)]
    counts = np.bincount(ki - 1, minlength=length).astype(np.float64)
    i = np.arange(length)
    dk = i[:, None] - i[None, :]
    W = np.where(np.abs(dk) < m, 1.0 - np.abs(dk / m), 0.0)
    dens = W @ counts
    return dens * (1.0 / (dens.sum() * delta))


def ash_pdf(dens, a, delta, x):
    """pdf(epdf, x) for an array x: searchsortedlast in rng[j] = a + (j - 1) delta, linear interpolation, 0 outside"""
    length = dens.size
    rng = a + np.arange(length) * delta
    x = np.asarray(x, dtype=np.float64)
    j = np.searchsorted(rng, x, side="right")
    inside = (j >= 1) & (j < length)
    jj = np.clip(j, 1, length - 1)
    r0, r1 = rng[jj - 1], rng[jj]
    w = dens[jj - 1] + (dens[jj] - dens[jj - 1]) * (x - r0) / (r1 - r0)
    return np.where(inside, w, 0.0)


def row_entropy(X, rows=None, check=True):
    """coefcost(X[e, :], DifferentialEntropyCost()) for the rows e of X (nk, N) (all, or the listed ones): Float64.
    Raises Degenerate for rows the reference throws for, unless check=False (those rows are then NaN)."""
    X = np.asarray(X)
    if rows is not None:
        X = X[np.asarray(rows)]
    N = X.shape[1]
    _, mbins, _ = ash_params(N)
    a, delta, length, _, ok = row_grid(X)
    if check and not ok.all():
        raise Degenerate(np.nonzero(~ok)[0])
    E = np.full(X.shape[0], np.nan)
    x64 = X.astype(np.float64)
    for r in np.nonzero(ok)[0]:
        dens = ash_density(x64[r], a[r], delta[r], int(length[r]), mbins)
        p = ash_pdf(dens, a[r], delta[r], x64[r])
        with np.errstate(divide="ignore"):
            E[r] = -(1.0 / N) * np.log(p).sum()
    return E


def node_costs(E, redundant=False):
    """tree_costs(X, LSDB(redundant)) from the row entropies E of the table: E (n, k) for 1-D, (n, m, k) for 2-D."""
    E = np.asarray(E, dtype=np.float64)
    if E.ndim == 2:
        n, k = E.shape
        if redundant:
            return np.array([E[:, i].sum() / (1 << ((i + 1).bit_length() - 1)) for i in range(k)])
        out = []
        for d in range(k):
            n0 = n >> d
            for j in range(1 << d):
                out.append(E[j * n0:(j + 1) * n0, d].sum())
        return np.array(out)
    from waveletsext_jl_amd.util import getcolrange, getdepth, getrowrange
    n, m, k = E.shape
    if redundant:
        return np.array([E[:, :, i].sum() / (1 << (2 * getdepth(i + 1, "quad"))) for i in range(k)])
    ncost = ((1 << (2 * k)) - 1) // 3
    out = []
    for i in range(1, ncost + 1):
        d = getdepth(i, "quad")
        rr, cc = getrowrange(n, i), getcolrange(m, i)
        out.append(E[rr[0] - 1:rr[-1], cc[0] - 1:cc[-1], d].sum())
    return np.array(out)


def tree_costs(X, redundant=False):
    """tree_costs(X, LSDB(redundant)) of a table X (n, k, N) or (n, m, k, N), Float64 costs"""
    X = np.asarray(X)
    sig = X.shape[:-1]
    E = row_entropy(X.reshape(-1, X.shape[-1], order="F"))
    return node_costs(E.reshape(sig, order="F"), redundant)
