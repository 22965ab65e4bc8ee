"""Per-signal tree matrices that stay in device memory (csrc/wx_trees_prep.hip): wptall / iwptall / iwpdall / getbasiscoefall with
`trees` a device tensor against the same call with the same trees as a host matrix (byte for byte) and against the oracle called
per signal (helpers.TOL); `wx.wpt_trees_route()` after every call, so that a silent trip through the host shows.

The prep kernel walks a column 64 nodes at a time, a wavefront per column up to 4095 nodes and a workgroup per column above; the
sizes: 8 (7 nodes: part of one word), 64 (63 nodes: one short of a wavefront), 128 (two steps), 1024 (sixteen steps, four per
iteration), 8192 Float64 / 16384 Float32 (the LDS limit; a workgroup per column).  Eleven signals: columns start at b * (n - 1),
every byte alignment."""
import ctypes

import numpy as np
import pytest

import helpers

pytestmark = pytest.mark.gpu

LDS, SINGLE, COPIED, GATHER, HOST = ("device prep + lds kernel", "device prep + single tree", "device trees copied to host",
                                     "device prep + gather", "host trees")


def _log2(n):
    return int(n).bit_length() - 1


def _deep(n, depth, right):
    """the chain root -> left (right) child -> ... decomposed `depth` times"""
    t = np.zeros(n - 1, dtype=bool)
    node = 1
    for _ in range(depth):
        t[node - 1] = True
        node = 2 * node + (1 if right else 0)
    return t


def _tree_mix(wx, n, rng, extra=0):
    """the batch of trees of tests/test_gpu_wpt_trees.py, asserted as there: [copy, full, :dwt, left-deep, right-deep, random p = 0.3, 0.7, 0.9, ...]"""
    L = _log2(n)
    cols = [np.zeros(n - 1, dtype=bool), wx.maketree(n, L, "full"), wx.maketree(n, L, "dwt"), _deep(n, L - 1, False), _deep(n, L, True)]
    seen = {c.tobytes() for c in cols}
    for i in range(3 + extra):
        p = (0.3, 0.7, 0.9)[i % 3]
        t = helpers.random_tree_1d(n, rng, p)
        while t.tobytes() in seen or not t[0]:                        # a new tree each time, never the bare root's copy
            t = helpers.random_tree_1d(n, rng, p)
        seen.add(t.tobytes())
        cols.append(t)
    trees = np.asfortranarray(np.stack(cols, axis=1))
    assert not trees[:, 0].any() and trees[:, 1].all()
    assert (trees[:, 2] == wx.maketree(n, L, "dwt")).all()
    left, right = trees[:, 3], trees[:, 4]
    assert left[[0, 1]].all() and not left[2] and right[[0, 2]].all() and not right[1]
    assert left.sum() == L - 1 and right.sum() == L
    assert len({trees[:, i].tobytes() for i in range(trees.shape[1])}) == trees.shape[1]
    assert all(wx.isvalidtree(np.zeros(n), trees[:, i]) for i in range(trees.shape[1]))
    return trees


def _per_signal(fn, a, qmf, trees):
    return np.stack([fn(a[..., i], qmf, trees[:, i]) for i in range(trees.shape[1])], axis=-1)


def _dev_trees(wx, trees, dtype=np.bool_):
    """a host tree matrix as a column-major device tensor of torch.bool / torch.uint8"""
    return wx.to_device(np.asfortranarray(trees.astype(dtype)))


def _same_bytes(wx, a, b):
    return wx.to_numpy(a).tobytes() == wx.to_numpy(b).tobytes()


def _four_calls(wx, xd, cd, td, wt, trees):
    """[(name, result)] of wptall(x), iwptall(c), iwpdall(table), getbasiscoefall(table) with `trees`, and the routes they took"""
    out, routes = [], []
    for name, fn in (("wptall", lambda: wx.wptall(xd, wt, trees)), ("iwptall", lambda: wx.iwptall(cd, wt, trees)),
                     ("iwpdall", lambda: wx.iwpdall(td, wt, trees)), ("getbasiscoefall", lambda: wx.getbasiscoefall(td, trees))):
        out.append((name, fn()))
        routes.append(wx.wpt_trees_route())
    return out, routes


def _check_all(wx, oracle, dtype, n, wname, trees, rng, want_route=LDS):
    import torch
    wt = wx.wavelet(wname)
    tol = helpers.TOL[np.dtype(dtype)]
    B = trees.shape[1]
    x = np.asfortranarray(rng.standard_normal((n, B)).astype(dtype))
    c = np.asfortranarray(rng.standard_normal((n, B)).astype(dtype))
    xd, cd = wx.to_device(x), wx.to_device(c)
    td = wx.wpdall(xd, wt)
    table = wx.to_numpy(td)
    dev, routes = _four_calls(wx, xd, cd, td, wt, _dev_trees(wx, trees))
    assert routes == [want_route] * 3 + [GATHER], routes
    host, hroutes = _four_calls(wx, xd, cd, td, wt, trees)
    assert hroutes == [HOST] * 4, hroutes
    ref = {"wptall": lambda: _per_signal(oracle.wpt, x, wt.qmf, trees), "iwptall": lambda: _per_signal(oracle.iwpt, c, wt.qmf, trees),
           "iwpdall": lambda: _per_signal(oracle.iwpd, table, wt.qmf, trees),
           "getbasiscoefall": lambda: np.stack([oracle.getbasiscoef(table[..., i], trees[:, i]) for i in range(B)], axis=-1)}
    for (name, d), (_, h) in zip(dev, host):
        assert isinstance(d, torch.Tensor) and d.is_cuda and tuple(d.shape) == (n, B), name
        e = helpers.relerr(wx.to_numpy(d), ref[name]())
        print(name, "against the oracle", e)
        assert e <= tol, name
        assert _same_bytes(wx, d, h), name + ": device trees and host trees differ"


def _limit(dtype):
    return 8192 if dtype == np.float64 else 16384


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("wname", ["haar", "db4", "db10"])
@pytest.mark.parametrize("n", [8, 64, 128, 1024, "limit"])
def test_device_trees_equal_host_trees_and_the_oracle(wx, oracle, n, wname, dtype):
    n = _limit(dtype) if n == "limit" else n
    rng = np.random.default_rng(77 * n + len(wname) + ord(wname[-1]))
    trees = _tree_mix(wx, n, rng, extra=3)
    assert trees.shape[1] == 11                                       # columns at every byte alignment (the stride n - 1 is odd)
    _check_all(wx, oracle, dtype, n, wname, trees, rng)


def test_workgroups_take_several_signals_in_turn(wx):
    """the construction of tests/test_gpu_wpt_trees.py: n = 64, a grid of 4096 workgroups of the LDS kernel, 3 * 4096 + 5 signals,
    every turn of a workgroup with another tree; the prep kernel's wavefronts stride over the columns as well (65536 / 4 per pass)"""
    n, grid = 64, 4096
    B = 3 * grid + 5
    rng = np.random.default_rng(64)
    wt = wx.wavelet(wx.WT.db4)
    pool = _tree_mix(wx, n, rng, extra=53)
    assert pool.shape[1] == 61
    b = np.arange(B)
    which = (b + b // grid) % 61
    assert (which[:-grid] != which[grid:]).all()
    trees = np.asfortranarray(pool[:, which])
    xd = wx.to_device(np.asfortranarray(rng.standard_normal((n, B))))
    td = wx.to_device(np.asfortranarray(rng.standard_normal((n, 7, B))))
    dev, routes = _four_calls(wx, xd, xd, td, wt, _dev_trees(wx, trees))
    assert routes == [LDS] * 3 + [GATHER]
    host, _ = _four_calls(wx, xd, xd, td, wt, trees)
    for (name, d), (_, h) in zip(dev, host):
        assert _same_bytes(wx, d, h), name


def test_more_columns_than_one_pass_of_the_prep_grid(wx):
    """n = 8: 65536 workgroups of four columns are one pass of the prep kernel's grid; 4 * 65536 + 7 columns need a second one"""
    n, B = 8, 4 * 65536 + 7
    rng = np.random.default_rng(8)
    wt = wx.wavelet(wx.WT.haar)
    pool = _tree_mix(wx, n, rng, extra=0)[:, :5]                       # n = 8 has few trees: the five fixed ones
    trees = np.asfortranarray(pool[:, (np.arange(B) * 3 + np.arange(B) // 65536) % 5])
    xd = wx.to_device(np.asfortranarray(rng.standard_normal((n, B))))
    d = wx.wptall(xd, wt, _dev_trees(wx, trees))
    assert wx.wpt_trees_route() == LDS
    assert _same_bytes(wx, d, wx.wptall(xd, wt, trees))


@pytest.mark.parametrize("n", [64, 8192])
def test_bytes_other_than_0_and_1(wx, n):
    """any non-zero byte means decomposed, as on the host"""
    rng = np.random.default_rng(2)
    wt = wx.wavelet(wx.WT.db4)
    trees = _tree_mix(wx, n, rng, extra=3)
    odd = np.where(trees, np.where(rng.random(trees.shape) < 0.5, 2, 255), 0).astype(np.uint8)
    assert set(np.unique(odd)) == {0, 2, 255}
    xd = wx.to_device(np.asfortranarray(rng.standard_normal((n, trees.shape[1]))))
    td = wx.wpdall(xd, wt)
    a, ra = _four_calls(wx, xd, xd, td, wt, _dev_trees(wx, odd, np.uint8))
    b, rb = _four_calls(wx, xd, xd, td, wt, _dev_trees(wx, trees, np.uint8))
    assert ra == rb == [LDS] * 3 + [GATHER]
    for (name, u), (_, v) in zip(a, b):
        assert _same_bytes(wx, u, v), name


def test_row_major_tensor(wx):
    import torch
    n = 128
    rng = np.random.default_rng(5)
    wt = wx.wavelet(wx.WT.db4)
    trees = _tree_mix(wx, n, rng, extra=3)
    rowmajor = torch.from_numpy(np.ascontiguousarray(trees)).to("cuda")      # (ntree, B), the last index fastest
    assert rowmajor.is_contiguous() and not wx._arrays.is_colmajor(rowmajor)
    xd = wx.to_device(np.asfortranarray(rng.standard_normal((n, trees.shape[1]))))
    td = wx.wpdall(xd, wt)
    a, ra = _four_calls(wx, xd, xd, td, wt, rowmajor)
    b, _ = _four_calls(wx, xd, xd, td, wt, trees)
    assert ra == [LDS] * 3 + [GATHER]
    for (name, u), (_, v) in zip(a, b):
        assert _same_bytes(wx, u, v), name


# ---- errors from the tree content ------------------------------------------------------------------------------------
def _valid9(wx, n, rng):
    return np.asfortranarray(_tree_mix(wx, n, rng, extra=1)[:, :9].copy())


def _orphan(trees, col, node):
    """node `node` (1-based) set under a cleared parent in column `col`"""
    t = trees.copy(order="F")
    t[:, col] = False
    t[0, col] = True                                                   # the root alone ...
    assert node >= 4 and not t[node // 2 - 1, col]
    t[node - 1, col] = True                                            # ... and a node whose parent is not decomposed
    return t


@pytest.mark.parametrize("col,node", [(4, 4), (4, 63), (8, 4), (8, 63)])
def test_invalid_trees_raise_assertion_errors(wx, col, node):
    """node 4 is the first that can lack its parent under a decomposed root (the defect at node 2 / 3 needs a cleared root: next test);
    node 63 = ntree is the last byte of the column, column 8 the last of the matrix"""
    n, B = 64, 9
    rng = np.random.default_rng(11)
    wt = wx.wavelet(wx.WT.db4)
    bad = _orphan(_valid9(wx, n, rng), col, node)
    xd = wx.to_device(np.asfortranarray(rng.standard_normal((n, B))))
    td = wx.wpdall(xd, wt)
    dt = _dev_trees(wx, bad)
    for call in (lambda: wx.wptall(xd, wt, dt), lambda: wx.iwptall(xd, wt, dt), lambda: wx.iwpdall(td, wt, dt),
                 lambda: wx.getbasiscoefall(td, dt)):
        with pytest.raises(AssertionError, match="isvalidtree"):
            call()
        assert wx.wpt_trees_route() == "none"


@pytest.mark.parametrize("col", [0, 8])
def test_child_at_node_2_under_a_cleared_root(wx, col):
    n, B = 64, 9
    rng = np.random.default_rng(12)
    wt = wx.wavelet(wx.WT.db4)
    bad = _valid9(wx, n, rng)
    bad[:, col] = False
    bad[1, col] = True                                                 # node 2 set, the root is not
    xd = wx.to_device(np.asfortranarray(rng.standard_normal((n, B))))
    td = wx.wpdall(xd, wt)
    dt = _dev_trees(wx, bad)
    for call in (lambda: wx.wptall(xd, wt, dt), lambda: wx.iwptall(xd, wt, dt), lambda: wx.iwpdall(td, wt, dt),
                 lambda: wx.getbasiscoefall(td, dt)):
        with pytest.raises(AssertionError, match="isvalidtree"):
            call()


def test_too_deep_trees_and_the_first_offending_column(wx):
    n, B, k = 64, 9, 4                                                 # a table of columns 0 .. 3: depth <= 3
    rng = np.random.default_rng(13)
    wt = wx.wavelet(wx.WT.db4)
    xd = wx.to_device(np.asfortranarray(rng.standard_normal((n, B))))
    td = wx.to_device(np.asfortranarray(rng.standard_normal((n, k, B))))
    ok = np.asfortranarray(np.stack([wx.maketree(n, 1 + i % 3, "full") for i in range(B)], axis=1))
    deep = ok.copy(order="F")
    deep[:, 2] = _deep(n, 4, True)                                     # depth 4 needs five columns
    for trees in (ok, deep):
        wx.wptall(xd, wt, _dev_trees(wx, trees))                       # no k here: fine either way
        assert wx.wpt_trees_route() == "device prep + lds kernel"
    wx.iwpdall(td, wt, _dev_trees(wx, ok))
    wx.getbasiscoefall(td, _dev_trees(wx, ok))
    for fn in (wx.iwpdall, wx.getbasiscoefall):
        args = (td, wt) if fn is wx.iwpdall else (td,)
        with pytest.raises(wx.ArgumentError, match="Not enough decomposition levels"):
            fn(*args, _dev_trees(wx, deep))
        both = _orphan(deep, 6, 4)                                     # too deep in column 2, invalid in column 6: the lower column decides
        with pytest.raises(wx.ArgumentError):
            fn(*args, _dev_trees(wx, both))
        swapped = both.copy(order="F")
        swapped[:, [2, 6]] = both[:, [6, 2]]
        with pytest.raises(AssertionError):
            fn(*args, _dev_trees(wx, swapped))
        for t in (deep, both, swapped):                                # the host route decides the same way
            with pytest.raises(wx.ArgumentError if t is not swapped else AssertionError):
                fn(*args, t)


@pytest.mark.parametrize("fam", ["wpt", "iwpt", "iwpd", "getbasiscoef"])
def test_rejected_trees_leave_the_output_untouched(wx, fam):
    """through the C ABI with a pre-filled device output: errors from the tree content come before any output element is written"""
    import torch
    n, B, k = 64, 9, 4
    rng = np.random.default_rng(14)
    lib = wx._lib.lib()
    q = np.ascontiguousarray(wx.wavelet(wx.WT.db4).qmf, dtype=np.float64)
    bad = _orphan(_valid9(wx, n, rng), 8, 63)
    if fam in ("iwpd", "getbasiscoef"):
        bad[:, 0] = _deep(n, 5, False)                                 # and a tree deeper than the table in front of it
    dt = _dev_trees(wx, bad, np.uint8)
    src = wx.to_device(np.asfortranarray(rng.standard_normal((n, k, B) if fam in ("iwpd", "getbasiscoef") else (n, B))))
    out = wx.jl_empty((n, B), torch.float64, "cuda")
    out.fill_(-7.25)
    P, L64, I = ctypes.c_void_p, ctypes.c_int64, ctypes.c_int
    st = P(torch.cuda.current_stream().cuda_stream)
    if fam == "getbasiscoef":
        rc = lib.wx_getbasiscoef1d_trees_f64(P(src.data_ptr()), P(out.data_ptr()), L64(n), I(k), P(dt.data_ptr()), L64(n - 1), L64(B), st)
    elif fam == "iwpd":
        rc = lib.wx_iwpd1d_trees_f64(P(src.data_ptr()), P(out.data_ptr()), L64(n), I(k), P(dt.data_ptr()), L64(n - 1), L64(B),
                                     P(q.ctypes.data), I(q.size), st)
    else:
        rc = getattr(lib, "wx_%s1d_trees_f64" % fam)(P(src.data_ptr()), P(out.data_ptr()), L64(n), P(dt.data_ptr()), L64(n - 1), L64(B),
                                                     P(q.ctypes.data), I(q.size), st)
    assert rc == (-2 if fam in ("iwpd", "getbasiscoef") else -1)
    assert lib.wx_wpt_trees_last_route() == 0
    torch.cuda.synchronize()
    assert bool((out == -7.25).all())


def test_python_refuses_mismatched_arguments(wx):
    import torch
    n, B = 64, 5
    wt = wx.wavelet(wx.WT.db4)
    dt = torch.zeros((n - 1, B), dtype=torch.bool, device="cuda")
    with pytest.raises(TypeError):
        wx.wptall(np.zeros((n, B)), wt, dt)                            # host data, device trees
    with pytest.raises(TypeError):
        wx.getbasiscoefall(np.zeros((n, 3, B)), dt)
    with pytest.raises(TypeError):
        wx.wptall(wx.to_device(np.zeros((n, B))), wt, dt.to(torch.float32))
    with pytest.raises(AssertionError):
        wx.wptall(wx.to_device(np.zeros((n, B + 1))), wt, dt)          # Utils.jl:210


# ---- the other routes -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_identical_columns_equal_the_single_tree_entry(wx, dtype):
    n, B = 256, 9
    rng = np.random.default_rng(9)
    wt = wx.wavelet(wx.WT.db4)
    tree = helpers.random_tree_1d(n, rng, 0.8)
    assert tree[0]
    dt = _dev_trees(wx, np.repeat(tree[:, None], B, axis=1))
    xd = wx.to_device(np.asfortranarray(rng.standard_normal((n, B)).astype(dtype)))
    td = wx.wpdall(xd, wt)
    for fn, a in ((wx.wptall, xd), (wx.iwptall, xd), (wx.iwpdall, td)):
        got = fn(a, wt, dt)
        assert wx.wpt_trees_route() == SINGLE
        assert _same_bytes(wx, got, fn(a, wt, tree)), fn.__name__


@pytest.mark.parametrize("n,dtype,wname", [(16384, np.float64, "db4"), (64, np.float32, "db11")])
def test_outside_the_window(wx, oracle, n, dtype, wname):
    """longer than the LDS holds, a filter of 22 taps: the matrix is copied to the host once and the host route runs"""
    rng = np.random.default_rng(n)
    L = _log2(n)
    trees = np.asfortranarray(np.stack([helpers.random_tree_1d(n, rng, 0.8) | wx.maketree(n, 2, "full"), _deep(n, L - 1, False),
                                        _deep(n, L, True)], axis=1))
    assert len({trees[:, i].tobytes() for i in range(3)}) == 3
    _check_all(wx, oracle, dtype, n, wname, trees, rng, want_route=COPIED)


# ---- 2-D gather -----------------------------------------------------------------------------------------------------
def _quad_trees(wx, m, rng):
    nt = wx.gettreelength(m, m)
    L = _log2(m)
    chain = np.zeros(nt, dtype=bool)
    node = 1
    for _ in range(L):                                                 # root -> its last child -> ... : the deepest nodes are the last bytes
        chain[node - 1] = True
        node = 4 * node + 1
    one = np.zeros(nt, dtype=bool)
    one[0] = True
    rnd = helpers.random_tree_2d(m, m, rng, 0.6)
    cols = [np.zeros(nt, dtype=bool), wx.maketree(m, m, L, "full"), rnd, chain, one]
    assert chain[nt - 1] and chain.sum() == L and rnd[0]
    return np.asfortranarray(np.stack(cols, axis=1)), L


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("m,k", [(16, 3), (16, 4), (64, 3), (64, 4)])
def test_gather_2d(wx, oracle, m, k, dtype):
    rng = np.random.default_rng(100 * m + k)
    trees, L = _quad_trees(wx, m, rng)
    B = trees.shape[1]
    depth = lambda t: 0 if not t.any() else max(oracle.getdepth(int(i) + 1, "quad") for i in np.flatnonzero(t)) + 1
    fits = np.array([depth(trees[:, i]) < k for i in range(B)])
    assert fits[[0, 4]].all() and not fits[[1, 3]].any()               # full and chain have depth L >= 4 > k - 1
    shallow = trees.copy(order="F")
    shallow[:, ~fits] = wx.maketree(m, m, k - 1, "full")[:, None]      # the deepest trees the table admits in their place
    Xd = wx.to_device(np.asfortranarray(rng.standard_normal((m, m, k, B)).astype(dtype)))
    got = wx.getbasiscoefall(Xd, _dev_trees(wx, shallow))
    assert wx.wpt_trees_route() == GATHER
    want = wx.getbasiscoefall(Xd, shallow)
    assert wx.wpt_trees_route() == HOST
    assert tuple(got.shape) == (m, m, B) and _same_bytes(wx, got, want)
    X = wx.to_numpy(Xd)
    exp = np.stack([oracle.getbasiscoef2d(X[..., i], shallow[:, i]) for i in range(B)], axis=-1)
    assert helpers.relerr(wx.to_numpy(got), exp) <= helpers.TOL[np.dtype(dtype)]
    with pytest.raises(wx.ArgumentError):                              # the full tree and the chain reach below the table
        wx.getbasiscoefall(Xd, _dev_trees(wx, trees))
    bad = shallow.copy(order="F")
    bad[:, 4] = False
    bad[trees.shape[0] - 1, 4] = True                                  # the last node of the last column, its parent cleared
    with pytest.raises(AssertionError):
        wx.getbasiscoefall(Xd, _dev_trees(wx, bad))
    bad2 = shallow.copy(order="F")
    bad2[:, 2] = False
    bad2[3, 2] = True                                                  # node 4, a child of the cleared root
    with pytest.raises(AssertionError):
        wx.getbasiscoefall(Xd, _dev_trees(wx, bad2))


# ---- the chain ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_best_basis_to_reconstruction_stays_on_the_device(wx, dtype):
    import torch
    n, B = 256, 33
    rng = np.random.default_rng(256)
    wt = wx.wavelet(wx.WT.db4)
    x = np.asfortranarray(np.cumsum(rng.standard_normal((n, B)), axis=0).astype(dtype))   # random walks: trees of many shapes
    xd = wx.to_device(x)
    table = wx.wpdall(xd, wt)
    t = wx.bestbasistreeall(table, wx.BB(), device=True)
    assert isinstance(t, torch.Tensor) and t.is_cuda and t.dtype == torch.bool and tuple(t.shape) == (n - 1, B)
    assert wx._arrays.is_colmajor(t)
    host = wx.bestbasistreeall(table, wx.BB())
    assert isinstance(host, np.ndarray) and (t.cpu().numpy() == host).all()
    assert len({host[:, i].tobytes() for i in range(B)}) > 1
    y = wx.wptall(xd, wt, t)
    assert wx.wpt_trees_route() == LDS
    assert _same_bytes(wx, y, wx.wptall(xd, wt, host))
    g = wx.getbasiscoefall(table, t)
    assert wx.wpt_trees_route() == GATHER
    assert helpers.relerr(wx.to_numpy(y), wx.to_numpy(g)) <= helpers.TOL[np.dtype(dtype)]
    back = wx.iwptall(y, wt, t)
    assert wx.wpt_trees_route() == LDS
    assert helpers.relerr(wx.to_numpy(back), x) <= helpers.TOL[np.dtype(dtype)]
    assert helpers.relerr(wx.to_numpy(wx.iwpdall(table, wt, t)), x) <= helpers.TOL[np.dtype(dtype)]
