"""Per-image quad-tree matrices that stay in device memory: wptall / iwptall / iwpdall of images with `trees` a device tensor against
the same call with the same trees as a host matrix (byte for byte) and against the oracle called per image (helpers.TOL);
`wx.wpt_trees_route()` after every call, so that a silent trip through the host shows.  The prep kernel's quad form walks a column
64 nodes at a time: 21 nodes (8 x 8, 8 x 32: part of one word), 85 (16 x 16: two steps), 1365 (64 x 64: 22 steps, 43 words)."""
import ctypes

import numpy as np
import pytest

import helpers

pytestmark = pytest.mark.gpu

LDS, SINGLE, COPIED, HOST = "device prep + lds kernel", "device prep + single tree", "device trees copied to host", "host trees"
TOP_RIGHT, BOTTOM_RIGHT = 1, 3                                       # child c of node i is 4 i - 2 + c


def _levels(m, n):
    return int(min(m, n)).bit_length() - 1


def _chain(nt, depth, child):
    t = np.zeros(nt, dtype=bool)
    node = 1
    for _ in range(depth):
        t[node - 1] = True
        node = 4 * node - 2 + child
    return t


def _tree_mix(wx, m, n, rng, extra=0):
    """the batch of trees of tests/test_gpu_wpt_trees2d.py: [copy, full, :dwt, top-right chain, bottom-right chain, random p = 0.3, 0.6, 0.9, ...]"""
    L = _levels(m, n)
    nt = wx.gettreelength(m, n)
    cols = [np.zeros(nt, dtype=bool), wx.maketree(m, n, L, "full"), wx.maketree(m, n, L, "dwt"), _chain(nt, L - 1, TOP_RIGHT),
            _chain(nt, L, BOTTOM_RIGHT)]
    seen = {c.tobytes() for c in cols}
    for i in range(3 + extra):
        p = (0.3, 0.6, 0.9)[i % 3]
        t = helpers.random_tree_2d(m, n, rng, p)
        while t.tobytes() in seen:
            t = helpers.random_tree_2d(m, n, rng, p)
        seen.add(t.tobytes())
        cols.append(t)
    trees = np.asfortranarray(np.stack(cols, axis=1))
    assert not trees[:, 0].any() and trees[:, 1].all() and trees[:, 2].sum() == L
    assert trees[:, 3].sum() == L - 1 and trees[:, 4].sum() == L and trees[nt - 1, 4]
    assert len({trees[:, i].tobytes() for i in range(trees.shape[1])}) == trees.shape[1]
    assert all(wx.isvalidtree(np.zeros((m, n)), trees[:, i]) for i in range(trees.shape[1]))
    return trees


def _per_image(fn, a, qmf, trees):
    return np.stack([fn(a[..., i], qmf, trees[:, i]) for i in range(trees.shape[1])], axis=-1)


def _dev_trees(wx, trees, dtype=np.bool_):
    return wx.to_device(np.asfortranarray(trees.astype(dtype)))


def _same_bytes(wx, a, b):
    return wx.to_numpy(a).tobytes() == wx.to_numpy(b).tobytes()


def _three_calls(wx, xd, cd, td, wt, trees):
    out, routes = [], []
    for name, fn in (("wptall", lambda: wx.wptall(xd, wt, trees)), ("iwptall", lambda: wx.iwptall(cd, wt, trees)),
                     ("iwpdall", lambda: wx.iwpdall(td, wt, trees))):
        out.append((name, fn()))
        routes.append(wx.wpt_trees_route())
    return out, routes


def _check_all(wx, oracle, dtype, m, n, wname, trees, rng, want_route=LDS):
    import torch
    wt = wx.wavelet(wname)
    tol = helpers.TOL[np.dtype(dtype)]
    B = trees.shape[1]
    x = np.asfortranarray(rng.standard_normal((m, n, B)).astype(dtype))
    c = np.asfortranarray(rng.standard_normal((m, n, B)).astype(dtype))
    xd, cd = wx.to_device(x), wx.to_device(c)
    td = wx.wpdall(xd, wt)
    table = wx.to_numpy(td)
    dev, routes = _three_calls(wx, xd, cd, td, wt, _dev_trees(wx, trees))
    assert routes == [want_route] * 3, routes
    host, hroutes = _three_calls(wx, xd, cd, td, wt, trees)
    assert hroutes == [HOST] * 3, hroutes
    ref = {"wptall": lambda: _per_image(oracle.wpt, x, wt.qmf, trees), "iwptall": lambda: _per_image(oracle.iwpt, c, wt.qmf, trees),
           "iwpdall": lambda: _per_image(oracle.iwpd, table, wt.qmf, trees)}
    for (name, d), (_, h) in zip(dev, host):
        assert isinstance(d, torch.Tensor) and d.is_cuda and tuple(d.shape) == (m, n, B), name
        e = helpers.relerr(wx.to_numpy(d), ref[name]())
        print(name, "against the oracle", e)
        assert e <= tol, name
        assert _same_bytes(wx, d, h), name + ": device trees and host trees differ"


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("wname", ["haar", "db4", "db10"])
@pytest.mark.parametrize("m,n", [(8, 8), (8, 32), (16, 16), (64, 64)])
def test_device_trees_equal_host_trees_and_the_oracle(wx, oracle, m, n, wname, dtype):
    rng = np.random.default_rng(77 * m + n + len(wname) + ord(wname[-1]))
    trees = _tree_mix(wx, m, n, rng, extra=3)
    assert trees.shape[1] == 11                                       # columns at every byte alignment (the tree lengths are odd)
    _check_all(wx, oracle, dtype, m, n, wname, trees, rng)


def test_bytes_other_than_0_and_1(wx):
    """any non-zero byte means decomposed, as on the host"""
    m = n = 16
    rng = np.random.default_rng(2)
    wt = wx.wavelet(wx.WT.db4)
    trees = _tree_mix(wx, m, n, rng, extra=3)
    odd = np.where(trees, np.where(rng.random(trees.shape) < 0.5, 2, 255), 0).astype(np.uint8)
    assert set(np.unique(odd)) == {0, 2, 255}
    xd = wx.to_device(np.asfortranarray(rng.standard_normal((m, n, trees.shape[1]))))
    td = wx.wpdall(xd, wt)
    a, ra = _three_calls(wx, xd, xd, td, wt, _dev_trees(wx, odd, np.uint8))
    b, rb = _three_calls(wx, xd, xd, td, wt, _dev_trees(wx, trees, np.uint8))
    assert ra == rb == [LDS] * 3
    for (name, u), (_, v) in zip(a, b):
        assert _same_bytes(wx, u, v), name


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("m", [16, 64])
def test_best_basis_to_reconstruction_stays_on_the_device(wx, m, dtype):
    """the direct output of bestbasistreeall(..., device=True) on a 2-D packet table feeds all three transforms.
    The reference normalises every block of a non-redundant 2-D table by its own norm (bestbasis_tree.jl:253), so a block costs
    nothing exactly when it holds at most one non-zero coefficient and any other image gets the full tree.  Haar images supported
    on one dyadic square of side 2^j put one coefficient into every block of depth j: trees that are full down to depth j."""
    import torch
    B = 13
    L = _levels(m, m)
    rng = np.random.default_rng(m)
    wt = wx.wavelet(wx.WT.haar)
    x = np.zeros((m, m, B), dtype=dtype, order="F")
    for b in range(B):
        s = 1 << (b % (L + 1))
        r0, c0 = (s * rng.integers(0, m // s, 2)).tolist()
        x[r0:r0 + s, c0:c0 + s, b] = rng.standard_normal((s, s))
    xd = wx.to_device(x)
    table = wx.wpdall(xd, wt)
    t = wx.bestbasistreeall(table, wx.BB(), device=True)
    nt = wx.gettreelength(m, m)
    assert isinstance(t, torch.Tensor) and t.is_cuda and tuple(t.shape) == (nt, B)
    host = wx.bestbasistreeall(table, wx.BB())
    assert isinstance(host, np.ndarray) and (t.cpu().numpy() == host).all()
    assert len({host[:, i].tobytes() for i in range(B)}) > 1
    tol = helpers.TOL[np.dtype(dtype)]
    y = wx.wptall(xd, wt, t)
    assert wx.wpt_trees_route() == LDS
    assert _same_bytes(wx, y, wx.wptall(xd, wt, host))
    assert wx.wpt_trees_route() == HOST
    assert helpers.relerr(wx.to_numpy(y), wx.to_numpy(wx.getbasiscoefall(table, t))) <= tol
    back = wx.iwptall(y, wt, t)
    assert wx.wpt_trees_route() == LDS
    assert _same_bytes(wx, back, wx.iwptall(y, wt, host))
    assert helpers.relerr(wx.to_numpy(back), x) <= tol
    rec = wx.iwpdall(table, wt, t)
    assert wx.wpt_trees_route() == LDS
    assert _same_bytes(wx, rec, wx.iwpdall(table, wt, host))
    assert helpers.relerr(wx.to_numpy(rec), x) <= tol


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_identical_columns_equal_the_single_tree_entry(wx, dtype):
    m = n = 64
    B = 9
    rng = np.random.default_rng(9)
    wt = wx.wavelet(wx.WT.db4)
    tree = helpers.random_tree_2d(m, n, rng, 0.7)
    assert tree[0] and not tree.all()
    dt = _dev_trees(wx, np.repeat(tree[:, None], B, axis=1))
    xd = wx.to_device(np.asfortranarray(rng.standard_normal((m, n, B)).astype(dtype)))
    td = wx.wpdall(xd, wt)
    for fn, a in ((wx.wptall, xd), (wx.iwptall, xd), (wx.iwpdall, td)):
        got = fn(a, wt, dt)
        assert wx.wpt_trees_route() == SINGLE
        assert _same_bytes(wx, got, fn(a, wt, tree)), fn.__name__


def test_outside_the_window(wx, oracle):
    """128 x 128 Float64 is more than the LDS holds: the matrix is copied to the host once and the host route runs"""
    m = n = 128
    rng = np.random.default_rng(128)
    nt = wx.gettreelength(m, n)
    L = _levels(m, n)
    trees = np.asfortranarray(np.stack([helpers.random_tree_2d(m, n, rng, 0.5), _chain(nt, L - 1, TOP_RIGHT), _chain(nt, L, BOTTOM_RIGHT)],
                                       axis=1))
    assert len({trees[:, i].tobytes() for i in range(3)}) == 3
    _check_all(wx, oracle, np.float64, m, n, "db4", trees, rng, want_route=COPIED)


# ---- errors from the tree content ------------------------------------------------------------------------------------
def _orphan(trees, col, node):
    """node `node` (1-based) set under a cleared parent in column `col`"""
    t = trees.copy(order="F")
    t[:, col] = False
    t[0, col] = True                                                   # the root alone ...
    assert node >= 6 and not t[(node + 2) // 4 - 1, col]
    t[node - 1, col] = True                                            # ... and a node whose parent is not decomposed
    return t


@pytest.mark.parametrize("col,node", [(4, 6), (8, 85)])
def test_invalid_and_too_deep_columns_raise_the_host_routes_errors(wx, col, node):
    """node 6 is the first that can lack its parent under a decomposed root; node 85 = ntree is the last byte of a column, column 8
    the last of the matrix"""
    m = n = 16
    B, k = 9, 3
    rng = np.random.default_rng(11)
    wt = wx.wavelet(wx.WT.db4)
    ok = np.asfortranarray(np.stack([wx.maketree(m, n, 1 + i % 2, "full") for i in range(B)], axis=1))   # depth <= 2 < k
    bad = _orphan(ok, col, node)
    deep = ok.copy(order="F")
    deep[:, 2] = wx.maketree(m, n, 3, "dwt")                           # depth 3 needs four slices
    xd = wx.to_device(np.asfortranarray(rng.standard_normal((m, n, B))))
    td = wx.to_device(np.asfortranarray(rng.standard_normal((m, n, k, B))))
    for call in (lambda t: wx.wptall(xd, wt, t), lambda t: wx.iwptall(xd, wt, t), lambda t: wx.iwpdall(td, wt, t)):
        for t in (_dev_trees(wx, bad), bad):
            with pytest.raises(AssertionError, match="isvalidtree"):
                call(t)
            assert wx.wpt_trees_route() == "none"
    wx.wptall(xd, wt, _dev_trees(wx, deep))                            # no k here: fine
    assert wx.wpt_trees_route() == LDS
    wx.iwpdall(td, wt, _dev_trees(wx, ok))
    assert wx.wpt_trees_route() == LDS
    both = deep.copy(order="F")
    both[:, col] = bad[:, col]                                         # too deep in column 2, invalid behind it: the lower column decides
    for t in (_dev_trees(wx, deep), deep, _dev_trees(wx, both), both):
        with pytest.raises(wx.ArgumentError, match="Not enough decomposition levels"):
            wx.iwpdall(td, wt, t)
        assert wx.wpt_trees_route() == "none"
    swapped = both.copy(order="F")
    swapped[:, [2, col]] = both[:, [col, 2]]
    for t in (_dev_trees(wx, swapped), swapped):
        with pytest.raises(AssertionError, match="isvalidtree"):
            wx.iwpdall(td, wt, t)


@pytest.mark.parametrize("fam", ["wpt", "iwpt", "iwpd"])
def test_rejected_trees_leave_the_output_untouched(wx, fam):
    """through the C ABI with a pre-filled device output: errors from the tree content come before any output element is written"""
    import torch
    m = n = 16
    B, k = 9, 3
    nt = wx.gettreelength(m, n)
    rng = np.random.default_rng(14)
    lib = wx._lib.lib()
    q = np.ascontiguousarray(wx.wavelet(wx.WT.db4).qmf, dtype=np.float64)
    ok = np.asfortranarray(np.stack([wx.maketree(m, n, 1 + i % 2, "full") for i in range(B)], axis=1))
    bad = _orphan(ok, 8, nt)
    if fam == "iwpd":
        bad[:, 0] = wx.maketree(m, n, 4, "dwt")                        # and a tree deeper than the table in front of it
    dt = _dev_trees(wx, bad, np.uint8)
    src = wx.to_device(np.asfortranarray(rng.standard_normal((m, n, k, B) if fam == "iwpd" else (m, n, B))))
    out = wx.jl_empty((m, n, B), torch.float64, "cuda")
    out.fill_(-7.25)
    P, L64, I = ctypes.c_void_p, ctypes.c_int64, ctypes.c_int
    st = P(torch.cuda.current_stream().cuda_stream)
    if fam == "iwpd":
        rc = lib.wx_iwpd2d_trees_f64(P(src.data_ptr()), P(out.data_ptr()), L64(m), L64(n), I(k), P(dt.data_ptr()), L64(nt), L64(B),
                                     P(q.ctypes.data), I(q.size), st)
    else:
        rc = getattr(lib, "wx_%s2d_trees_f64" % fam)(P(src.data_ptr()), P(out.data_ptr()), L64(m), L64(n), P(dt.data_ptr()), L64(nt), L64(B),
                                                     P(q.ctypes.data), I(q.size), st)
    assert rc == (-2 if fam == "iwpd" else -1)
    assert lib.wx_wpt_trees_last_route() == 0
    torch.cuda.synchronize()
    assert bool((out == -7.25).all())
