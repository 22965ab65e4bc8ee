"""GPU parity of the LDB class reductions (csrc/wx_ldb.hip: energy map, class means, class variances) where every class is
reduced in more than one chunk -- more than 64 signals in the average class, which no other test reaches -- against the
longdouble restatement of tests/ldb_ref.py.

Every case first asks wx_debug_ldb_chunks (the function the launch code calls) for the chunk count it was built for, then holds
Float64 and Float32 results to ldb_ref.bound: elementwise, (per + nchunks + 8) eps with per = ceil(largest class / nchunks),
relative to the value for the energy map and the variances (sums of non-negative terms) and to the class mean of |X| for the
means.  Derivation: k_ldb_class_partial adds at most per terms one after the other in T (per - 1 roundings of eps / 2 each, one
more per square), k_ldb_class_combine adds the nchunks partials and divides once; the root norms are accumulated in double and
rounded to T three times (sqrt, square, class sum).  The variance is taken around the kernel's own mean, as
discriminant_power does: its error shifts every deviation alike, which cancels to first order in the sum of squares.
tests/test_ldb_chunks_cpu.py shows that one signal lost, doubled or misplaced is hundreds of bounds away (Float32) or 10^11 (Float64).

The shapes are the smallest that reach each path; they are listed with their reasons in ldb_ref.CASES.  The means and the variances
are computed by calling wx_class_mean_* / wx_class_var_* the way discriminant_power(.., FishersClassSeparability()) does, so that
the two arrays are compared themselves and not only the power derived from them."""
import ctypes
import functools
import time

import numpy as np
import pytest

import ldb_ref
from helpers import TOL, relerr
from noisest_ref import same

pytestmark = pytest.mark.gpu

DTYPES = [np.float64, np.float32]
FIT_SEED = 7308        # case I: of the seeds 7301-7310 the one whose oracle fit is furthest from a tie (3e-3 costs, 5e-3 powers)


def _mean_var(X, idx, nc, var=True):
    """ldb.discriminant_power's two calls; X a host array or a device tensor of shape (..., signals)"""
    from waveletsext_jl_amd import _lib
    from waveletsext_jl_amd._arrays import Arg, to_numpy
    Xa = Arg(X)
    sz, N = Xa.shape[:-1], Xa.shape[-1]
    ne = int(np.prod(sz, dtype=np.int64))
    idx = np.ascontiguousarray(idx, dtype=np.int32)
    cp = ctypes.c_void_p(idx.ctypes.data)
    mean = Xa.new(tuple(sz) + (nc,))
    _lib.check(getattr(_lib.lib(), "wx_class_mean" + Xa.suffix)(Xa.ptr, ne, N, cp, nc, mean.ptr, Xa.stream()))
    if not var:
        return to_numpy(mean.arr), None
    v = Xa.new(tuple(sz) + (nc,))
    _lib.check(getattr(_lib.lib(), "wx_class_var" + Xa.suffix)(Xa.ptr, ne, N, cp, nc, mean.ptr, v.ptr, Xa.stream()))
    return to_numpy(mean.arr), to_numpy(v.arr)


def _first_seen_in_order(y):
    return (np.diff(np.unique(y, return_index=True)[1]) > 0).all()


@functools.lru_cache(maxsize=None)
def _case(name, dtype):
    """a case of ldb_ref.CASES with its reference (computed once; nobody writes to these arrays)"""
    c = ldb_ref.CASES[name]
    X, y, nroot = ldb_ref.case(name, dtype)
    mem = ldb_ref.members(y, len(c.sizes))
    assert tuple(len(m) for m in mem) == c.sizes and _first_seen_in_order(y)
    G, _ = ldb_ref.energy_map(X, mem, nroot)
    E, A = ldb_ref.class_mean(X, mem)
    for a in (X, y):
        a.setflags(write=False)
    return X, y, dict(G=G, E=E, A=A, V=ldb_ref.class_var(X, mem))


def _hold(tag, dtype, b, got, ref, scale=None):
    e = ldb_ref.err(got, ref, scale)
    print("%s %s: %.3f of the bound" % (tag, np.dtype(dtype).name, e / b))
    assert e <= b, (tag, e / b)


def _run(wx, X, y, nc):
    """the three arrays as the kernels give them, as numpy arrays"""
    G = wx.to_numpy(wx.energy_map(X, y))
    E, V = _mean_var(X, y, nc)
    return G, E, V


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("name", list(ldb_ref.CASES))
def test_chunked_reductions(wx, name, dtype):
    c = ldb_ref.CASES[name]
    nc = len(c.sizes)
    assert wx.ldb_chunks(int(np.prod(c.shape[:-1])), c.shape[-1], nc) == c.nchunks
    X, y, ref = _case(name, dtype)
    G, E, V = _run(wx, X, y, nc)
    assert G.dtype == E.dtype == V.dtype == np.dtype(dtype)
    b = ldb_ref.bound(max(c.sizes), c.nchunks, dtype)
    _hold(name + " energy", dtype, b, G, ref["G"])
    _hold(name + " mean", dtype, b, E, ref["E"], ref["A"])
    _hold(name + " var", dtype, b, V, ref["V"])


@pytest.mark.parametrize("dtype", DTYPES)
def test_device_resident_table_same_bits(wx, dtype):
    """case G: case A from a table that already lies on the device"""
    c = ldb_ref.CASES["A"]
    X, y, _ = _case("A", dtype)
    host = _run(wx, X, y, len(c.sizes))
    dev = _run(wx, wx.to_device(np.array(X, order="F")), y, len(c.sizes))      # (a copy: the shared table is read-only)
    for h, d in zip(host, dev):
        assert same(h, d)


@pytest.mark.parametrize("dtype", DTYPES)
def test_nan_and_inf_stay_in_their_entries(wx, dtype):
    """case H: case A with a NaN in one coefficient (not of the root) of one signal of the second class and a +Inf in one of the
    first class, each the last signal of a chunk: exactly those entries of the three arrays are not finite (the variance around an
    infinite mean is NaN), every other entry is within the bound"""
    c = ldb_ref.CASES["A"]
    nc, nroot = len(c.sizes), c.shape[0]
    X0, y, ref0 = _case("A", dtype)
    mem = ldb_ref.members(y, nc)
    e_nan, e_inf = (17, 3), (63, 6)                                  # (row, level): level 0 is the root
    i_inf = mem[0][2 * -(-c.sizes[0] // c.nchunks) - 1]              # the last signal of the first class's second chunk
    i_nan = mem[1][-(-c.sizes[1] // c.nchunks) - 1]                  # the last signal of the second class's first chunk
    X = np.array(X0, order="F")
    X[e_nan + (i_nan,)] = np.nan
    X[e_inf + (i_inf,)] = np.inf
    G, E, V = _run(wx, X, y, nc)
    for arr, at_inf in ((G, np.inf), (E, np.inf), (V, np.nan)):
        bad = ~np.isfinite(arr)
        assert bad.sum() == 2 and np.isnan(arr[e_nan + (1,)])
        assert np.isnan(arr[e_inf + (0,)]) if np.isnan(at_inf) else arr[e_inf + (0,)] == at_inf
    b = ldb_ref.bound(max(c.sizes), c.nchunks, dtype)
    Gr, _ = ldb_ref.energy_map(X, mem, nroot)
    Er, Ar = ldb_ref.class_mean(X, mem)
    Vr = ldb_ref.class_var(X, mem)
    for r, r0 in ((Gr, ref0["G"]), (Er, ref0["E"]), (Vr, ref0["V"])):   # the reference itself: two entries differ from case A's
        assert (~np.isfinite(r)).sum() == 2 and (np.isfinite(r) <= (r == r0)).all()
    _hold("H energy", dtype, b, G, Gr)
    _hold("H mean", dtype, b, E, Er, Ar)
    _hold("H var", dtype, b, V, Vr)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("per_class, nchunks, nchunks_whole", [(96, 1, 2), (97, 2, 3)])
def test_shards_with_an_absent_class(wx, dtype, per_class, nchunks, nchunks_whole):
    """case F: two shards of a batch, (s, s, 0) and (0, s, s) signals of the classes a, b, c.  A shard of 96 / 96 / 0 signals is
    still reduced in one chunk -- the average over the three classes it is told of, 64, decides -- so s = 97 is run as well, the
    smallest shard of this kind with two.  The absent class has a zero norm sum and an all-NaN map, the others are within the
    bound, and the maps and norm sums of the shards combine (test_gpu_ldb.py::test_energy_map_shards_combine) to the map of
    the whole batch within the shards' bound: map x norm sum is the chunked sum once more, and the total norm is a sum of two."""
    s, names = per_class, np.array(["a", "b", "c"])
    shape = (64, 7, 2 * s)
    assert wx.ldb_chunks(448, 2 * s, 3) == nchunks and wx.ldb_chunks(448, 4 * s, 3) == nchunks_whole
    rng = np.random.default_rng(7200 + s)
    y0, y1 = ldb_ref.labels((s, s, 0), rng), ldb_ref.labels((0, s, s), rng)
    X0, X1 = ldb_ref.table(shape, y0, rng, dtype), ldb_ref.table(shape, y1, rng, dtype)
    b = ldb_ref.bound(s, nchunks, dtype)
    parts = []
    for X, y, absent in ((X0, y0, 2), (X1, y1, 0)):
        G, n = wx.energy_map(X, list(names[y]), classes=list(names), return_norm_sum=True)
        assert n[absent] == 0 and np.isnan(G[..., absent]).all()
        Gr, nr = ldb_ref.energy_map(X, ldb_ref.members(y, 3), 64)
        assert np.isnan(Gr[..., absent]).all() and nr[absent] == 0
        _hold("F%d shard energy" % s, dtype, b, G, Gr)
        _hold("F%d shard norm sums" % s, dtype, b, n, nr)
        parts.append((np.nan_to_num(G).astype(ldb_ref.LD), n.astype(ldb_ref.LD)))
    (G0, n0), (G1, n1) = parts
    comb = (G0 * n0 + G1 * n1) / (n0 + n1)
    Xa, ya = np.asfortranarray(np.concatenate([X0, X1], axis=-1)), np.concatenate([y0, y1])
    Gr, _ = ldb_ref.energy_map(Xa, ldb_ref.members(ya, 3), 64)
    _hold("F%d combined shards" % s, dtype, b, comb, Gr)
    _hold("F%d whole batch" % s, dtype, ldb_ref.bound(2 * s, nchunks_whole, dtype), wx.energy_map(Xa, list(names[ya])), Gr)


@pytest.mark.parametrize("dtype", DTYPES)
def test_chunk_count_cut_to_the_grid_limit(wx, dtype):
    """case E: 4.2 M signals in 100 classes want 657 chunks a class, which is more workgroup rows than a grid has: 65535 / 100 = 655
    are launched.  Energy map and means.  The reference adds each class in longdouble (np.bincount only counts the signals: its
    weighted sums are accumulated in double, 42000 terms one after the other, which is coarser than the Float64 bound)."""
    nc = ldb_ref.E_NC
    assert wx.ldb_chunks(4, ldb_ref.E_SHAPE[-1], nc) == ldb_ref.E_NCHUNKS
    X, y, nroot = ldb_ref.case_e(dtype)
    assert isinstance(y, np.ndarray) and _first_seen_in_order(y)
    cnt = np.bincount(y, minlength=nc)
    mem = ldb_ref.members(y, nc)
    assert [len(m) for m in mem] == cnt.tolist() and cnt.min() > ldb_ref.E_NCHUNKS
    b = ldb_ref.bound(cnt.max(), ldb_ref.E_NCHUNKS, dtype)
    Gr, _ = ldb_ref.energy_map(X, mem, nroot)
    Er, Ar = ldb_ref.class_mean(X, mem)
    t0 = time.perf_counter()
    G = wx.energy_map(X, y)
    t1 = time.perf_counter()
    E, _ = _mean_var(X, y, nc, var=False)
    t2 = time.perf_counter()
    print("E %s: energy_map %.0f ms, wx_class_mean %.0f ms (host table, wall time)" % (np.dtype(dtype).name, 1e3 * (t1 - t0), 1e3 * (t2 - t1)))
    _hold("E energy", dtype, b, G, Gr)
    _hold("E mean", dtype, b, E, Er, Ar)


@pytest.mark.parametrize("dp", ["basis", "fisher"])
def test_fit_transform_with_two_chunks(wx, oracle, dp):
    """case I: fit_transform end to end on 3 x 70 signals of 64 samples, Float64, db2: the energy map (448 coefficients) and the class
    means / variances of Fisher's power (64) run in two chunks.  Tree and feature order must be the oracle's; the seed was chosen
    with the oracle alone so that no decision of the fit is closer than 1e-9 relative (asserted below on the oracle's own numbers),
    which a sum taken in another order cannot flip."""
    n, nfeat, sizes = 64, 10, (70, 70, 70)
    tol = TOL[np.dtype(np.float64)]
    assert wx.ldb_chunks(n * 7, sum(sizes), 3) == 2 and wx.ldb_chunks(n, sum(sizes), 3) == 2
    rng = np.random.default_rng(FIT_SEED)
    y = ldb_ref.labels(sizes, rng)
    X = ldb_ref.table((n, sum(sizes)), y, rng, np.float64)
    for dm, name, top_k in ((wx.AsymmetricRelativeEntropy(), "are", None), (wx.HellingerDistance(), "hellinger", 5)):
        f = wx.LocalDiscriminantBasis(wt=wx.wavelet(wx.WT.db2), dm=dm, top_k=top_k, n_features=nfeat,
                                      dp=wx.BasisDiscriminantMeasure() if dp == "basis" else wx.FishersClassSeparability())
        Xc = wx.fit_transform(f, X, y)
        Xw = oracle.wpdall(X, f.wt.qmf)
        exp = oracle.ldb_fitdec(Xw, y, dm=name, top_k=top_k, dp=dp)
        gap_tree, gap_rank = ldb_ref.decision_gaps(exp["cost"], exp["DP"], n, nfeat)
        print("I %s %s: closest cost decision %.2e, closest ranked powers %.2e" % (dp, name, gap_tree, gap_rank))
        assert gap_tree > 1e-9 and gap_rank > 1e-9
        assert relerr(f.cost, exp["cost"]) <= 50 * tol
        assert (f.tree == exp["tree"]).all()
        assert relerr(f.DP, exp["DP"]) <= 200 * tol
        assert (f.order[:nfeat] == exp["order"][:nfeat]).all()
        leaves = np.asfortranarray(np.stack([oracle.getbasiscoef(np.asfortranarray(Xw[:, :, i]), exp["tree"]) for i in range(X.shape[1])], axis=-1))
        assert relerr(Xc, leaves[exp["order"][:nfeat] - 1, :]) <= tol
