"""GPU parity of the shift-invariant packet transform (csrc/wx_siwt.hip, siwt.py) on the routes that the short,
single-signal cases of test_gpu_siwt.py never reach.  The oracle is oracle.siwpd / siwt_bestbasistree / isiwpd /
siwt_delete_node; table positions come from tests/siwt_trees.py (written from the header's layout), not from the
package.  Which test reaches what:

test_forward_long_routes
    (1024, 3, 2) db2, host arrays: k_siwt_fwd_level<FUSE=false> at j = 0 and <FUSE=true> at j = 1 with h2 = 256, four
        wavefronts per child through LDS, blockIdx.x > 0; jc = 1, so k_siwt_costs (cnt >= 256) runs for depths 0 and 1,
        several nodes and columns, output offset nodeoff[j] + (slot << j).
    (2048, 4, 4) db7: the any-length taps (FT = 0, 14 taps: the second block of eight partly filled), unfused j = 0, 1,
        fused j = 2 (h2 = 256) and j = 3 (h2 = 128, two wavefronts per child); jc = 2: k_siwt_costs over 7 columns,
        depth 2 = 4 columns x 4 nodes of 512.
    (768, 6, 3) db4: no fusing (not dyadic); k_siwt_costs with cnt = 768 and 384 (ragged strides of 256), then the
        lane-per-node branch.
    (1536, 9, 1) haar: the lane-per-node branch with 512 nodes per column, the second trip of node += 256.
    An all-zero signal in every batch: the nr == 0 route of the fused and the separate costs.
test_filter_lengths
    FT = 10, 12, 16, 18 and the any-length code with 14 taps of k_siwt_fwd_level and k_siwt_inv_level.
test_tree_selection_exact
    k_siwt_select_level and k_siwt_mark_level, every decision (ties included: haar, one- and two-sample nodes, the
        zero signal) against the oracle's selection run on the GPU's own costs, both element types.
test_inverse_along_trees / test_inverse_literal_flag
    k_siwt_build_map and k_siwt_inv_level on non-shifted, shifted, alternating, random and root-only trees, one per
        signal, with every node that is not a leaf set to NaN: which children are read, what is written;
        (2048, 4, 3) runs four workgroups per signal (blockIdx.x > 0); db10 is FT = 20.
test_batch_beyond_one_grid
    the gridDim.y chunks of api_siwpd / api_siwt_bestbasis / api_isiwpd: every b0 offset, batch = 65535 + 9.
test_null_costs
    wx_siwpd_* with costs == NULL (every level unfused, no norms) against the fused run.

Figures printed by test_forward_long_routes (Float32 costs against a Float64 recomputation from the oracle's own
Float32 node values) are there to be read with `pytest -s`; the asserted bounds are test_gpu_siwt.py's."""
import numpy as np
import pytest

import siwt_trees as st
from helpers import relerr

pytestmark = pytest.mark.gpu

DTYPES = [np.float64, np.float32]
TOLV = {np.float64: 0.0, np.float32: 1e-6}          # node values: Float64 bit-identical
TOLC = {np.float64: 1e-10, np.float32: 1e-4}        # node costs
TOLX = {np.float64: 1e-10, np.float32: 1e-5}        # reconstruction


def _wt(wx, name):
    return wx.wavelet(getattr(wx.WT, name))


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view({8: np.uint64, 4: np.uint32, 1: np.uint8}[a.dtype.itemsize])


def _signals(rng, n, B, dtype, zero=None, roll=None):
    X = rng.standard_normal((n, B))
    if zero is not None:
        X[:, zero] = 0.0
    if roll is not None:
        X[:, roll[0]] = np.roll(X[:, roll[1]], roll[2])
    return np.asfortranarray(X.astype(dtype))


def _node_rows(key, n, L, d):
    j, i, t = key
    np_ = n >> j
    return slice(i * np_, (i + 1) * np_), st.column_of(j, t, L, d)


def _cost64(v, nrm):
    """the node cost in Float64: -sum s log s, s = (v / nrm)^2"""
    s = (np.asarray(v, dtype=np.float64) / nrm) ** 2
    s = s[s > 0]
    return float(-(s * np.log(s)).sum())


def _check_forward(W, C, ref, b, n, L, d, dtype, tag):
    """every oracle node of signal b against the table W (n, NS, B) and the costs C (NN, B)"""
    assert set(ref.Nodes) == set(st.all_keys(L, d))
    worst_v = worst_c = gpu64 = ref64 = 0.0
    nrm = float(np.sqrt((ref.Nodes[(0, 0, 0)]["Value"].astype(np.float64) ** 2).sum()))
    for key, nd in ref.Nodes.items():
        rows, col = _node_rows(key, n, L, d)
        got = W[rows, col, b]
        if dtype == np.float64:
            assert np.array_equal(_bits(got), _bits(nd["Value"])), (tag, b, key)
        else:
            ev = float(np.abs(got.astype(np.float64) - nd["Value"]).max()) / max(1.0, float(np.abs(nd["Value"]).max()))
            worst_v = max(worst_v, ev)
            assert ev <= TOLV[dtype], (tag, b, key, ev)
        gc = float(C[st.node_index(*key, L, d), b])
        ec = abs(gc - nd["Cost"]) / max(1.0, abs(nd["Cost"]))
        worst_c = max(worst_c, ec)
        if dtype == np.float32 and nrm > 0:
            c64 = _cost64(nd["Value"], nrm)
            gpu64 = max(gpu64, abs(gc - c64) / max(1.0, abs(c64)))
            ref64 = max(ref64, abs(nd["Cost"] - c64) / max(1.0, abs(c64)))
    print("%s signal %d: worst value err %.3g, worst cost err %.3g (Float32 costs against Float64 recomputation: "
          "GPU %.3g, oracle %.3g)" % (tag, b, worst_v, worst_c, gpu64, ref64))
    assert worst_c <= TOLC[dtype], (tag, b, worst_c)


def _check_selection(C0, status, C1, ref, b, L, d, dtype, tag):
    """the oracle's selection on the GPU's costs C0[:, b] against status / C1 (costs after selection); returns the tree"""
    for key, nd in ref.Nodes.items():
        nd["Cost"] = float(C0[st.node_index(*key, L, d), b])
    import wx_oracle
    tree = wx_oracle.siwt_bestbasistree(ref)
    want = st.status_from_tree(tree, L, d)
    assert np.array_equal(status[:, b], want), (tag, b, np.flatnonzero(status[:, b] != want)[:8])
    for key, nd in ref.Nodes.items():
        assert dtype(C1[st.node_index(*key, L, d), b]) == dtype(nd["Cost"]), (tag, b, key)
    assert dtype(C1[0, b]) == dtype(ref.MinCost), (tag, b)
    return tree


FORWARD = [("db2", 1024, 3, 2, "host"), ("db7", 2048, 4, 4, "device"), ("db4", 768, 6, 3, "device"),
           ("haar", 1536, 9, 1, "device")]


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("wname,n,L,d,where", FORWARD)
def test_forward_long_routes(wx, oracle, wname, n, L, d, where, dtype):
    """Measured on an MI355X: Float32 node values equal the oracle's exactly at these lengths as well; the worst
    Float32 cost differs from the oracle's by 1.8e-6 (bound 1e-4), and against the Float64 recomputation from the
    oracle's Float32 values the GPU lies within 1.1e-7 and the oracle, which sums in Float32, within 1.8e-6."""
    wt = _wt(wx, wname)
    X = _signals(np.random.default_rng(n + L), n, 3, dtype, zero=1)
    batch = wx.siwpdall(X if where == "host" else wx.to_device(X), wt, L, d)
    assert isinstance(batch.Table, np.ndarray) == (where == "host")
    W, C = wx.to_numpy(batch.Table), wx.to_numpy(batch.Costs)
    assert W.shape == (n, st.ncols(L, d), 3) and C.shape == (st.nnodes(L, d), 3) and W.dtype == C.dtype == dtype
    for b in range(3):
        ref = oracle.siwpd(X[:, b], wt.qmf, L, d)
        assert batch[b].BestTree == ref.BestTree                       # the reference's push order
        _check_forward(W, C, ref, b, n, L, d, dtype, (wname, n, L, d))
    assert not W[:, :, 1].any() and not C[:, 1].any()                  # the zero signal: values and costs all 0


def _forward_table(wx, X, wt, L, d):
    return wx.to_numpy(wx.siwpdall(wx.to_device(X), wt, L, d).Table)


def _run_isiwpd(wx, Wn, status, wt, L, d, literal):
    """wx_isiwpd_* through ctypes on device pointers: W (n, NS, B), status (NN, B) and xh (n, B) exactly as the header
    describes them; returns the table and xh after the call"""
    import torch
    n, _, B = Wn.shape
    Wd = wx.to_device(Wn)
    sd = torch.from_numpy(np.ascontiguousarray(status.T)).to(Wd.device)      # (B, NN) row-major = (NN, B) column-major
    xh = wx.jl_empty((n, B), Wd.dtype, Wd.device)
    q = np.ascontiguousarray(wt.qmf, dtype=np.float64)
    fn = getattr(wx._lib.lib(), "wx_isiwpd" + ("_f64" if Wn.dtype == np.float64 else "_f32"))
    rc = fn(Wd.data_ptr(), sd.data_ptr(), xh.data_ptr(), n, L, d, B, q.ctypes.data, int(q.size), literal,
            torch.cuda.current_stream(Wd.device).cuda_stream)
    assert rc == 0, wx._lib.lib().wx_last_error()
    torch.cuda.synchronize()
    return wx.to_numpy(Wd), wx.to_numpy(xh)


def _inverse_case(wx, oracle, wname, n, L, d, dtype, modes, rng, literal=0):
    """forward on the GPU, everything but the leaves of one tree per signal set to NaN, one wx_isiwpd_* call"""
    wt = _wt(wx, wname)
    B = len(modes)
    X = _signals(rng, n, B, dtype)
    Wf = _forward_table(wx, X, wt, L, d)
    NS, NN = st.ncols(L, d), st.nnodes(L, d)
    Wn = np.full((n, NS, B), np.nan, dtype=dtype, order="F")
    inner = np.zeros((n, NS, B), dtype=bool, order="F")
    status = np.zeros((NN, B), dtype=np.uint8, order="F")
    refs, trees = [], []
    for b, mode in enumerate(modes):
        full = oracle.siwpd(X[:, b], wt.qmf, L, d)
        keys = [(0, 0, 0)] if mode == "root" else st.random_tree(full, rng, mode)
        status[:, b] = st.status_from_tree(keys, L, d)
        for key in keys:
            rows, col = _node_rows(key, n, L, d)
            if status[st.node_index(*key, L, d), b] == 1:
                Wn[rows, col, b] = Wf[rows, col, b]
            else:
                inner[rows, col, b] = True
        refs.append(st.prune(full, keys)); trees.append(keys)
    assert np.isnan(Wn[:, 0, [b for b, m in enumerate(modes) if m != "root"]]).all()
    Wr, xr = _run_isiwpd(wx, Wn, status, wt, L, d, literal)
    assert Wr.shape == Wn.shape and xr.shape == (n, B) and Wr.dtype == xr.dtype == dtype
    tol = TOLX[dtype]
    assert np.isfinite(xr).all()
    for b, mode in enumerate(modes):
        tag = (wname, n, L, d, mode, b)
        scale = float(np.abs(X[:, b]).max())
        xo = oracle.isiwpd(refs[b], literal=bool(literal))
        assert relerr(xr[:, b], xo) <= tol, tag
        if not literal:
            assert relerr(xr[:, b], X[:, b]) <= tol, tag
            m = inner[:, :, b]                                         # internal nodes hold their forward values again
            assert float(np.abs(Wr[:, :, b][m].astype(np.float64) - Wf[:, :, b][m]).max(initial=0.0)) <= tol * scale, tag
        assert np.array_equal(xr[:, b], Wr[:, 0, b]), tag              # xh is the root column
    # no stray writes: leaves keep their values, NaNs stay NaN
    assert np.array_equal(_bits(Wr)[~inner], _bits(Wn)[~inner])
    assert np.isfinite(Wr[inner]).all()
    return trees


MODES5 = ("ns", "ss", "alt", "rand", "root")
INVERSE = [("haar", 64, 6, 6), ("db4", 48, 4, 2), ("db10", 256, 5, 3), ("db2", 2048, 4, 3)]


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("wname,n,L,d", INVERSE)
def test_inverse_along_trees(wx, oracle, wname, n, L, d, dtype):
    trees = _inverse_case(wx, oracle, wname, n, L, d, dtype, MODES5, np.random.default_rng(n * 3 + d))
    assert len({frozenset(t) for t in trees}) == len(MODES5)           # five different trees in one call


@pytest.mark.parametrize("dtype", DTYPES)
def test_inverse_literal_flag(wx, oracle, dtype):
    _inverse_case(wx, oracle, "db4", 48, 4, 2, dtype, MODES5, np.random.default_rng(5), literal=1)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("wname", ["db5", "db6", "db8", "db9", "db7"])
def test_filter_lengths(wx, oracle, wname, dtype):
    n, L, d = 64, 3, 2
    wt = _wt(wx, wname)
    assert len(wt.qmf) == {"db5": 10, "db6": 12, "db7": 14, "db8": 16, "db9": 18}[wname]
    X = _signals(np.random.default_rng(len(wt.qmf)), n, 2, dtype)
    batch = wx.siwpdall(wx.to_device(X), wt, L, d)
    W, C = wx.to_numpy(batch.Table), wx.to_numpy(batch.Costs)
    for b in range(2):
        _check_forward(W, C, oracle.siwpd(X[:, b], wt.qmf, L, d), b, n, L, d, dtype, (wname, n, L, d))
    _inverse_case(wx, oracle, wname, n, L, d, dtype, ("rand", "rand"), np.random.default_rng(len(wt.qmf) + 1))


SELECT = [("haar", 64, 6, 6), ("haar", 32, 5, 2), ("db2", 64, 6, 6), ("db4", 48, 4, 4), ("db4", 256, 5, 3)]


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("wname,n,L,d", SELECT)
def test_tree_selection_exact(wx, oracle, wname, n, L, d, dtype):
    """No tolerance anywhere: the oracle sums and compares in the signal's element type, so on the same costs every
    difference is a defect of k_siwt_select_level / k_siwt_mark_level."""
    wt = _wt(wx, wname)
    B, ZERO = 5, 2
    X = _signals(np.random.default_rng(n * 5 + d), n, B, dtype, zero=ZERO, roll=(4, 0, 3))
    batch = wx.siwpdall(wx.to_device(X), wt, L, d)
    C0 = wx.to_numpy(batch.Costs).copy()
    status = np.array(wx.bestbasistreeall_(batch))
    C1 = wx.to_numpy(batch.Costs)
    assert status.shape == C0.shape == C1.shape == (st.nnodes(L, d), B)
    assert float(batch.MinCost[ZERO]) == 0.0
    ties = 0
    for b in range(B):
        ref = oracle.siwpd(X[:, b], wt.qmf, L, d)
        full_ss = st.random_tree(ref, None, "ss") if b == ZERO else None
        for key in ref.Nodes if b != ZERO else ():                     # how many decisions the tie rule takes (the
            ns, ss = st._children(key)                                 # children's costs after their own selection)
            if ns[0] in ref.Nodes and ss[0] in ref.Nodes:
                cu = dtype(C1[st.node_index(*ns[0], L, d), b]) + dtype(C1[st.node_index(*ns[1], L, d), b])
                cs = dtype(C1[st.node_index(*ss[0], L, d), b]) + dtype(C1[st.node_index(*ss[1], L, d), b])
                ties += int(cu == cs)
        tree = _check_selection(C0, status, C1, ref, b, L, d, dtype, (wname, n, L, d))
        assert set(batch[b].BestTree) == set(tree), (wname, n, L, d, b)
        assert float(batch.MinCost[b]) == float(dtype(ref.MinCost))
        if b == ZERO:                                                  # all ties: shifted children wherever they exist
            assert set(tree) == set(full_ss)
            assert np.array_equal(status[:, b], st.status_from_tree(full_ss, L, d))
    print("%s: %d exact ties between the two child pairs in the %d nonzero signals" % ((wname, n, L, d), ties, B - 1))


@pytest.mark.parametrize("dtype", DTYPES)
def test_batch_beyond_one_grid(wx, oracle, dtype):
    """Columns repeat with period 7 and 65535 mod 7 = 1, so a chunk offset that is wrong by any number of signals that
    is not a multiple of 7 breaks the periodicity of the results; every signal has its own blockIdx.y, so equal
    signals give bit-equal results."""
    n, L, d, P = 8, 3, 2, 7
    B = 65535 + 9
    wt = _wt(wx, "haar")
    base = _signals(np.random.default_rng(11), n, P, dtype, zero=3)
    X = np.asfortranarray(base[:, np.arange(B) % P])
    batch = wx.siwpdall(wx.to_device(X), wt, L, d)
    W, C0 = wx.to_numpy(batch.Table).copy(), wx.to_numpy(batch.Costs).copy()
    status = np.array(wx.bestbasistreeall_(batch))
    C1 = wx.to_numpy(batch.Costs).copy()
    xr = wx.to_numpy(wx.isiwpdall(batch))
    assert W.shape == (n, st.ncols(L, d), B) and C0.shape == C1.shape == status.shape == (st.nnodes(L, d), B)
    for name, A in (("table", W), ("costs", C0), ("status", status), ("costs after selection", C1), ("output", xr)):
        A = _bits(A)
        assert np.array_equal(A[..., P:], A[..., :-P]), name
    for b in range(P):
        ref = oracle.siwpd(base[:, b], wt.qmf, L, d)
        _check_forward(W, C0, ref, b, n, L, d, dtype, ("haar", n, L, d))
        _check_selection(C0, status, C1, ref, b, L, d, dtype, ("haar", n, L, d))
    assert not W[:, :, 3].any() and not C0[:, 3].any()
    assert relerr(xr, X) <= TOLX[dtype]


@pytest.mark.parametrize("dtype", DTYPES)
def test_null_costs(wx, dtype):
    import torch
    n, L, d, B = 1024, 3, 2, 3
    wt = _wt(wx, "db2")
    Xd = wx.to_device(_signals(np.random.default_rng(2), n, B, dtype, zero=1))
    NS, NN = st.ncols(L, d), st.nnodes(L, d)
    W1, W2 = (wx.jl_empty((n, NS, B), Xd.dtype, Xd.device) for _ in range(2))
    W1.fill_(float("nan")); W2.fill_(float("nan"))
    costs = wx.jl_empty((NN, B), Xd.dtype, Xd.device)
    q = np.ascontiguousarray(wt.qmf, dtype=np.float64)
    fn = getattr(wx._lib.lib(), "wx_siwpd" + ("_f64" if dtype == np.float64 else "_f32"))
    stream = torch.cuda.current_stream(Xd.device).cuda_stream
    assert fn(Xd.data_ptr(), W1.data_ptr(), costs.data_ptr(), n, L, d, B, q.ctypes.data, int(q.size), stream) == 0
    assert fn(Xd.data_ptr(), W2.data_ptr(), None, n, L, d, B, q.ctypes.data, int(q.size), stream) == 0
    torch.cuda.synchronize()
    A1, A2 = wx.to_numpy(W1), wx.to_numpy(W2)
    assert np.isfinite(A1).all() and np.isfinite(wx.to_numpy(costs)).all()
    assert np.array_equal(_bits(A1), _bits(A2))
