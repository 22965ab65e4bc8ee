"""numpy restatement, in np.longdouble, of the three batch-sized reductions of Local Discriminant Basis (csrc/wx_ldb.hip), the
yardstick of tests/test_ldb_chunks_cpu.py and tests/test_gpu_ldb_chunks.py.

Straight from the definitions, over a table seen as (nk, N) with the first nroot rows of a signal being its root:
    energy map  Gamma[e, c] = sum_{i in c} X[e, i]^2 / sum_{i in c} ||root_i||^2       (ldb_energymap.jl:109-141)
    class mean  E[e, c]     = sum_{i in c} X[e, i] / n_c                                (ldb_measures.jl:441-479)
    class var   V[e, c]     = sum_{i in c} (X[e, i] - E[e, c])^2 / (n_c - 1), around the exact mean
A class is a list of signal indices (`members`), so that a test can drop a signal, count it twice or move it and see what the
comparison makes of that.  Non-finite values and empty or one-signal classes come out as numpy gives them (0 / 0 = NaN).

The rest is what the two test files share: the elementwise error measure, the bound it is held to, and the data of the cases.
"""
import collections

import numpy as np

LD = np.longdouble


def members(idx, nc):
    """the signals of every class in index order: nc index arrays (one stable sort: 100 classes of 4.2 M signals take 0.3 s)"""
    idx = np.asarray(idx)
    offs = np.cumsum(np.bincount(idx, minlength=nc))[:-1]
    return np.split(np.argsort(idx, kind="stable"), offs)


def _rows(X):
    X = np.asarray(X)
    return X.reshape((-1, X.shape[-1]), order="F")


def energy_map(Xw, mem, nroot):
    """(Gamma of shape Xw.shape[:-1] + (nc,), the nc sums of squared root norms), longdouble"""
    X2 = _rows(Xw)
    G = np.empty((X2.shape[0], len(mem)), dtype=LD)
    ns = np.empty(len(mem), dtype=LD)
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        for c, m in enumerate(mem):
            blk = X2[:, m].astype(LD)
            sq = blk * blk
            ns[c] = sq[:nroot].sum()
            G[:, c] = sq.sum(axis=1) / ns[c]
    return G.reshape(np.shape(Xw)[:-1] + (len(mem),), order="F"), ns


def class_mean(X, mem):
    """(class means, class means of |X|), both of shape X.shape[:-1] + (nc,), longdouble"""
    X2 = _rows(X)
    E = np.empty((X2.shape[0], len(mem)), dtype=LD)
    A = np.empty_like(E)
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        for c, m in enumerate(mem):
            blk = X2[:, m].astype(LD)
            E[:, c] = blk.sum(axis=1) / LD(len(m))
            A[:, c] = np.abs(blk).sum(axis=1) / LD(len(m))
    shp = np.shape(X)[:-1] + (len(mem),)
    return E.reshape(shp, order="F"), A.reshape(shp, order="F")


def class_var(X, mem):
    """class variances (n - 1 denominator, around the exact class mean), shape X.shape[:-1] + (nc,), longdouble"""
    X2 = _rows(X)
    V = np.empty((X2.shape[0], len(mem)), dtype=LD)
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        for c, m in enumerate(mem):
            blk = X2[:, m].astype(LD)
            d = blk - (blk.sum(axis=1) / LD(len(m)))[:, None]
            V[:, c] = (d * d).sum(axis=1) / LD(len(m) - 1)
    return V.reshape(np.shape(X)[:-1] + (len(mem),), order="F")


def fisher_power(E, V, counts):
    """discriminant_power(coefs, y, FishersClassSeparability()) from the class means and variances (ldb_measures.jl:472-477)"""
    p = np.asarray(counts, dtype=LD) / LD(np.sum(counts))
    Ea = E.mean(axis=-1, keepdims=True)
    return (((E - Ea * E) ** 2) * p).sum(axis=-1) / (V * p).sum(axis=-1)


def err(got, ref, scale=None):
    """the largest elementwise |got - ref| / scale (scale = |ref| unless given: a relative error per element, where
    helpers.relerr divides by the largest entry of the whole array and so cannot see the small deep columns).  Where ref is not
    finite, got must be the same NaN or the same infinity; where ref (or the scale) is zero, got must equal ref.  Anything else
    is an infinite error."""
    got, ref = np.asarray(got).astype(LD), np.asarray(ref, dtype=LD)
    assert got.shape == ref.shape, (got.shape, ref.shape)
    scale = np.abs(ref) if scale is None else np.asarray(scale, dtype=LD)
    fin = np.isfinite(ref)
    with np.errstate(invalid="ignore"):
        same = (np.isnan(got) & np.isnan(ref)) | (got == ref)
    if not same[~fin].all() or not np.isfinite(got[fin]).all():
        return np.inf
    live = fin & (scale > 0) & np.isfinite(scale)
    if not same[fin & ~live].all():
        return np.inf
    return float((np.abs(got[live] - ref[live]) / scale[live]).max()) if live.any() else 0.0


def bound(cnt_max, nchunks, dtype):
    """what err() may be for a class of at most cnt_max signals reduced in nchunks chunks in `dtype`: the kernel adds at most
    per = ceil(cnt_max / nchunks) terms one after the other, then the nchunks partials, and divides once; the squares, the
    rounding of the root norms and of the denominator are the + 8.  (per + nchunks + 8) eps, for sums of non-negative terms
    relative to the sum and for the means relative to the class mean of |X|."""
    per = -(-int(cnt_max) // int(nchunks))
    return (per + int(nchunks) + 8) * float(np.finfo(dtype).eps)


def decision_gaps(cost, power, n, nfeat):
    """how close fitdec! comes to another answer, on a 1-D fit's own numbers: (the smallest relative gap between a parent's cost and
    its children's best in the bottom-up `max` tree selection over all n - 1 nodes, the smallest relative gap between consecutive
    powers among the nfeat + 1 largest)"""
    c = np.array(cost, dtype=np.float64)
    gap_tree = np.inf
    for i in range(n - 1, 0, -1):
        pc, cc = c[i - 1], c[2 * i - 1] + c[2 * i]
        gap_tree = min(gap_tree, abs(cc - pc) / max(abs(cc), abs(pc)))
        c[i - 1] = max(pc, cc)
    top = np.sort(np.asarray(power, dtype=np.float64).ravel())[::-1][:nfeat + 1]
    gap_rank = float(((top[:-1] - top[1:]) / np.abs(top[:-1])).min())
    return float(gap_tree), gap_rank


# ---- the cases -------------------------------------------------------------------------------------------------------------
Case = collections.namedtuple("Case", "shape sizes nchunks seed")
# table shape (sz..., levels, signals), class sizes, chunks per class.  The sizes are the smallest that reach:
CASES = {
    # nk = 448 is no multiple of 256; chunks of 100, 100, 100, 97 = 4 * 24 + 1 signals (unrolled loop and tail) for the first class,
    # and for the class of 3 chunks of one signal and an empty fourth
    "A": Case((64, 7, 600), (397, 200, 3), 4, 7101),
    "B": Case((64, 7, 193), (65, 64, 64), 2, 7102),                 # one signal past the threshold, and ...
    "B1": Case((64, 7, 192), (64, 64, 64), 1, 7103),                # ... its single-chunk control
    "C": Case((2048, 2, 200), (129, 71), 2, 7104),                  # roots of 2048 samples: the 8-way unrolled loop of the root norm
    "D": Case((16, 16, 3, 300), (157, 143), 3, 7105),               # 2-D: the root (256 coefficients) is not a column of the table
}
E_SHAPE, E_NC, E_NCHUNKS, E_SEED = (2, 2, 4200000), 100, 655, 7106   # 657 chunks x 100 classes pass gridDim.y: 65535 / 100 = 655


def _in_order(y, nc):
    """swap signals so that the classes first appear in the order 0, 1, ...: unique(y) then lists them in this order"""
    pos = 0
    for c in range(nc):
        hit = np.flatnonzero(y[pos:] == c)
        if hit.size:
            j = pos + int(hit[0])
            y[pos], y[j] = y[j], y[pos]
            pos += 1
    return y


def labels(sizes, rng):
    """class index per signal for classes of the given sizes (int32), a random permutation, so that a chunk gathers signals from
    all over the table"""
    y = np.repeat(np.arange(len(sizes), dtype=np.int32), sizes)
    return _in_order(y[rng.permutation(y.size)], len(sizes))


def table(shape, y, rng, dtype):
    """X[e, i] = (1 + i % 7) exp(-6 e / nk) g[e, i] + y[i] / 2 with standard normal g, as a column-major table of `shape`: signals
    of seven sizes, energy that falls by e^6 from the first coefficient to the last, class means half a unit apart"""
    nk, N = int(np.prod(shape[:-1], dtype=np.int64)), int(shape[-1])
    X = rng.standard_normal((N, nk), dtype=np.float64 if np.dtype(dtype) == np.float64 else np.float32).T
    X = X * np.exp(-6.0 * np.arange(nk) / nk).astype(X.dtype)[:, None]
    X = X * (1 + np.arange(N) % 7).astype(X.dtype)[None, :] + (0.5 * np.asarray(y)).astype(X.dtype)[None, :]
    return np.asfortranarray(X.astype(dtype, copy=False)).reshape(shape, order="F")


def case_e(dtype):
    """(table, labels as an int32 array, nroot) of the case of E_SHAPE: 4 coefficients of 4.2 M signals in 100 classes drawn at random"""
    rng = np.random.default_rng(E_SEED)
    y = _in_order(rng.integers(0, E_NC, E_SHAPE[-1]).astype(np.int32), E_NC)
    return table(E_SHAPE, y, rng, dtype), y, E_SHAPE[0]


def case(name, dtype):
    """(table, labels, nroot) of a case of CASES"""
    c = CASES[name]
    rng = np.random.default_rng(c.seed)
    y = labels(c.sizes, rng)
    return table(c.shape, y, rng, dtype), y, int(np.prod(c.shape[:-2], dtype=np.int64))
