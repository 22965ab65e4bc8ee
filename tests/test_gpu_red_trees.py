"""iswpdall(xw, wt, M[, sm]) / iacwpdall(xw, M) with M an (n - 1, N) matrix -- one tree per signal, every signal rebuilt from its redundant
packet table along its own basis (csrc/wx_red_trees.hip) -- against the oracle called per signal with that signal's column, within
20 * helpers.TOL (the bound of tests/test_gpu_denoise.py for the redundant input types); host trees and device trees byte for byte;
repeated calls byte for byte; `wx.wpt_trees_route()` after every call.

The tables are the library's own swpdall / acwpdall of seeded normal signals, so every case is a round trip against x as well.  Eleven
trees of depth <= D per case (bare root, full to D, :dwt to D, left-deep D - 1, right-deep D, six random ones); the column stride n - 1
is odd, so the columns start at every byte alignment.  Shapes: n = 8, D = 3 (nodes shorter than the filters: the wrap); n = 64, D = 6 (one
wavefront per pass); n = 256, D = 8 (several wavefronts, a deep stack); n = 1024 with the deepest table the LDS window admits (D = 8 in
Float64, D = 10 in Float32); n = 1024, D = 10 in Float64, outside it."""
import ctypes

import numpy as np
import pytest

import helpers

pytestmark = pytest.mark.gpu

LDS, SINGLE, COPIED, HOST = "device prep + lds kernel", "device prep + single tree", "device trees copied to host", "host trees"


def _deep(n, depth, right):
    """the chain root -> left (right) child -> ... decomposed `depth` times"""
    t = np.zeros(n - 1, dtype=bool)
    node = 1
    for _ in range(depth):
        t[node - 1] = True
        node = 2 * node + (1 if right else 0)
    return t


def _clip(t, D):
    """no node of depth >= D decomposed: a tree of depth <= D"""
    t = t.copy()
    t[(1 << D) - 1:] = False
    return t


def _trees11(wx, n, D, rng, extra=6):
    """[bare root, full to D, :dwt to D, left-deep D - 1, right-deep D, random p = 0.3, 0.7, 0.9, 0.3, 0.7, 0.9 (, ...)], all different"""
    cols = [np.zeros(n - 1, dtype=bool), wx.maketree(n, D, "full"), wx.maketree(n, D, "dwt"), _deep(n, D - 1, False), _deep(n, D, True)]
    seen = {c.tobytes() for c in cols}
    count = 1                                                          # trees of depth <= d: t(0) = 1, t(d) = 1 + t(d - 1)^2
    for _ in range(D):
        count = 1 + count * count
    assert 3 <= D <= int(n).bit_length() - 1 and count >= 5 + extra or extra == 0, "not that many trees of this depth"
    for i in range(extra):
        p = (0.3, 0.7, 0.9)[i % 3]
        t = _clip(helpers.random_tree_1d(n, rng, p), D)
        while t.tobytes() in seen or not t[0]:
            t = _clip(helpers.random_tree_1d(n, rng, p), D)
        seen.add(t.tobytes())
        cols.append(t)
    trees = np.asfortranarray(np.stack(cols, axis=1))
    assert len({trees[:, i].tobytes() for i in range(trees.shape[1])}) == trees.shape[1]
    assert all(wx.isvalidtree(np.zeros(n), trees[:, i]) for i in range(trees.shape[1]))
    assert not trees[(1 << D) - 1:].any() and trees[(1 << D) - 2, 1] and trees[(1 << D) - 2, 4]   # depth <= D, reached by two of them
    return trees


def _dev(wx, trees, dtype=np.bool_):
    return wx.to_device(np.asfortranarray(trees.astype(dtype)))


def _bytes(wx, a):
    return wx.to_numpy(a).tobytes()


def _window_depth(n, dtype):
    """the deepest table whose 2 D n values, 512 bytes of filter and tree bits fit 136 KiB"""
    D = int(n).bit_length() - 1
    while 512 + 2 * D * n * np.dtype(dtype).itemsize + 4 * max(1, n // 32) > 136 * 1024:
        D -= 1
    return D


def _sms(D):
    """no shift, the smallest, the largest the table admits, and one between (several bits set from D = 3 on: 4, 39, 159, 639)"""
    sms = [0, 1, (1 << D) - 1, max(2, ((1 << D) - 1) * 5 // 8)]
    assert D >= 2 and len(set(sms)) == 4 and 1 < sms[3] < sms[2]
    return sms


def _check(wx, oracle, n, D, wname, dtype, inside=True, cols=None):
    """every mode of one shape: average, four shifts, and the autocorrelation transform in Float64"""
    import torch
    rng = np.random.default_rng(1000 * n + 10 * D + len(wname))
    wt = wx.wavelet(wname)
    tol = 20 * helpers.TOL[np.dtype(dtype)]
    trees = _trees11(wx, n, D, rng)
    if cols is not None:
        trees = np.asfortranarray(trees[:, cols])
    B = trees.shape[1]
    x = np.asfortranarray(rng.standard_normal((n, B)).astype(dtype))
    xd = wx.to_device(x)
    sms = _sms(D)
    modes = [("swpd", sm) for sm in [None] + sms] + ([("acwpd", None)] if dtype == np.float64 else [])
    tables = {"swpd": wx.swpdall(xd, wt, D)}
    if dtype == np.float64:
        tables["acwpd"] = wx.acwpdall(xd, wt, D)
    host_tables = {k: wx.to_numpy(v) for k, v in tables.items()}
    assert tuple(tables["swpd"].shape) == (n, (1 << (D + 1)) - 1, B)
    dtb, dtu = _dev(wx, trees), _dev(wx, trees, np.uint8)
    want_dev = LDS if inside else COPIED
    for kind, sm in modes:
        td, th = tables[kind], host_tables[kind]
        if kind == "swpd":
            call = lambda t, tr: wx.iswpdall(t, wt, tr) if sm is None else wx.iswpdall(t, wt, tr, sm)
            ref = np.stack([oracle.iswpd(th[:, :, i], wt.qmf, trees[:, i], sm) for i in range(B)], axis=-1)
        else:
            call = lambda t, tr: wx.iacwpdall(t, tr)
            ref = np.stack([oracle.iacwpd(th[:, :, i], trees[:, i]) for i in range(B)], axis=-1)
        got = {}
        got["host data, host trees"] = call(th, trees)
        assert wx.wpt_trees_route() == HOST
        got["device data, host trees"] = call(td, trees)
        assert wx.wpt_trees_route() == HOST
        got["device data, bool device trees"] = call(td, dtb)
        assert wx.wpt_trees_route() == want_dev, wx.wpt_trees_route()
        got["device data, uint8 device trees"] = call(td, dtu)
        assert wx.wpt_trees_route() == want_dev
        got["again"] = call(td, dtb)
        assert wx.wpt_trees_route() == want_dev
        assert isinstance(got["host data, host trees"], np.ndarray) and isinstance(got["again"], torch.Tensor) and got["again"].is_cuda
        first = wx.to_numpy(got["host data, host trees"])
        assert first.shape == (n, B) and first.dtype == np.dtype(dtype)
        for i in range(B):
            e = helpers.relerr(first[:, i], ref[:, i])
            assert e <= tol, (kind, sm, i, e)
        e = helpers.relerr(first, x)
        print(kind, sm, "round trip", e, "oracle", helpers.relerr(first, ref))
        assert e <= tol, (kind, sm, "round trip", e)
        for name, g in got.items():
            assert _bytes(wx, g) == first.tobytes(), (kind, sm, name)


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("wname", ["haar", "db4", "db8"])
@pytest.mark.parametrize("n,D", [(8, 3), (64, 6), (256, 8), (1024, "window")])
def test_parity_with_the_oracle_per_signal(wx, oracle, n, D, wname, dtype):
    if D == "window":
        D = _window_depth(n, dtype)
        assert D == (8 if dtype == np.float64 else 10)
    _check(wx, oracle, n, D, wname, dtype)


def test_shallow_table_of_a_long_signal(wx, oracle):
    """the table's depth, not the signal's, sizes the LDS slots and bounds the shift"""
    _check(wx, oracle, 512, 3, "db4", np.float64)


def test_just_outside_the_window(wx, oracle):
    """n = 1024 with a table of depth 10 needs 160 KiB in Float64: the single-tree entry once per signal, a device matrix coming to the
    host first"""
    assert _window_depth(1024, np.float64) < 10
    _check(wx, oracle, 1024, 10, "db4", np.float64, inside=False, cols=[4, 7, 9])   # right-deep to 10 and two random trees


def test_workgroups_take_several_signals_in_turn(wx, oracle):
    """n = 64 with a table of depth 2: a grid of 4096 workgroups, 3 * 4096 + 5 signals, every turn of a workgroup with another tree"""
    n, D, grid = 64, 2, 4096
    B = 3 * grid + 5
    rng = np.random.default_rng(64)
    wt = wx.wavelet(wx.WT.db4)
    pool = _trees11(wx, n, D, rng, extra=0)
    b = np.arange(B)
    which = (b + b // grid) % 5
    assert (which[:-grid] != which[grid:]).all()
    trees = np.asfortranarray(pool[:, which])
    x = np.asfortranarray(rng.standard_normal((n, B)))
    xd = wx.to_device(x)
    dt = _dev(wx, trees)
    sample = np.r_[0:8, grid - 3:grid + 3, 2 * grid - 3:2 * grid + 3, B - 8:B]
    for kind in ("swpd", "acwpd"):
        td = wx.swpdall(xd, wt, D) if kind == "swpd" else wx.acwpdall(xd, wt, D)
        th = wx.to_numpy(td)[:, :, sample]
        for sm in ((None, 3) if kind == "swpd" else (None,)):
            if kind == "swpd":
                call = lambda tr: wx.iswpdall(td, wt, tr) if sm is None else wx.iswpdall(td, wt, tr, sm)
                ref = np.stack([oracle.iswpd(th[:, :, j], wt.qmf, trees[:, i], sm) for j, i in enumerate(sample)], axis=-1)
            else:
                call = lambda tr: wx.iacwpdall(td, wt, tr)
                ref = np.stack([oracle.iacwpd(th[:, :, j], trees[:, i]) for j, i in enumerate(sample)], axis=-1)
            got = call(dt)
            assert wx.wpt_trees_route() == LDS
            g = wx.to_numpy(got)
            assert helpers.relerr(g[:, sample], ref) <= 20 * helpers.TOL[np.dtype(np.float64)]
            assert helpers.relerr(g, x) <= 20 * helpers.TOL[np.dtype(np.float64)]
            assert _bytes(wx, call(trees)) == g.tobytes()
            assert wx.wpt_trees_route() == HOST


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_identical_columns_equal_the_single_tree_entry(wx, dtype):
    n, D, B = 256, 5, 9
    rng = np.random.default_rng(9)
    wt = wx.wavelet(wx.WT.db4)
    tree = _clip(helpers.random_tree_1d(n, rng, 0.8), D)
    assert tree[0]
    M = np.repeat(tree[:, None], B, axis=1)
    xd = wx.to_device(np.asfortranarray(rng.standard_normal((n, B)).astype(dtype)))
    td = wx.swpdall(xd, wt, D)
    for sm in (None, 5):
        got = wx.iswpdall(td, wt, _dev(wx, M), sm)
        assert wx.wpt_trees_route() == SINGLE
        assert _bytes(wx, got) == _bytes(wx, wx.iswpdall(td, wt, tree, sm))
        assert _bytes(wx, got) == _bytes(wx, wx.iswpdall(td, wt, M, sm))
        assert wx.wpt_trees_route() == HOST
    if dtype == np.float64:
        ta = wx.acwpdall(xd, wt, D)
        got = wx.iacwpdall(ta, _dev(wx, M))
        assert wx.wpt_trees_route() == SINGLE
        assert _bytes(wx, got) == _bytes(wx, wx.iacwpdall(ta, tree))


def test_single_signal_forms_take_a_one_column_matrix(wx, oracle):
    n, D = 64, 4
    rng = np.random.default_rng(3)
    wt = wx.wavelet(wx.WT.db4)
    tree = _clip(helpers.random_tree_1d(n, rng, 0.8), D)
    assert tree[0]
    x = rng.standard_normal(n)
    xw, xa = wx.swpd(x, wt, D), wx.acwpd(x, wt, D)
    tol = 20 * helpers.TOL[np.dtype(np.float64)]
    for sm in (None, 6):
        got = wx.iswpd(xw, wt, tree[:, None], sm)
        assert got.shape == (n,) and helpers.relerr(got, oracle.iswpd(xw, wt.qmf, tree, sm)) <= tol
        d = wx.iswpd(wx.to_device(xw), wt, _dev(wx, tree[:, None]), sm)
        assert tuple(d.shape) == (n,) and _bytes(wx, d) == got.tobytes()
    got = wx.iacwpd(xa, tree[:, None])
    assert got.shape == (n,) and helpers.relerr(got, oracle.iacwpd(xa, tree)) <= tol
    assert _bytes(wx, wx.iacwpd(wx.to_device(xa), wt, _dev(wx, tree[:, None], np.uint8))) == got.tobytes()


# ---- errors from the tree content, on the device route --------------------------------------------------------------
def _orphan(trees, col):
    """node 4 set under a cleared node 2 in column `col`"""
    t = trees.copy(order="F")
    t[:, col] = False
    t[[0, 3], col] = True
    return t


@pytest.mark.parametrize("fam", ["iswpd", "iswpd_f32", "iacwpd"])
def test_the_lowest_offending_column_decides_and_nothing_is_written(wx, fam):
    """through the C ABI with a pre-filled device output: an invalid column 5 and a too-deep column 2 give WX_EBOUNDS, swapped they
    give WX_EASSERT, and x stays at its sentinel either way"""
    import torch
    n, D, B = 64, 3, 9
    rng = np.random.default_rng(14)
    lib = wx._lib.lib()
    q = np.ascontiguousarray(wx.wavelet(wx.WT.db4).qmf, dtype=np.float64)
    ok = _trees11(wx, n, D, rng, extra=4)
    assert ok.shape[1] == B
    both = _orphan(ok, 5)
    both[:, 2] = _deep(n, D + 1, True)                                 # depth 4 under a table of depth 3
    swapped = both.copy(order="F")
    swapped[:, [2, 5]] = both[:, [5, 2]]
    tdt = torch.float32 if fam.endswith("f32") else torch.float64
    src = wx.to_device(np.asfortranarray(rng.standard_normal((n, 15, B)).astype(np.float32 if fam.endswith("f32") else np.float64)))
    P, L64, I = ctypes.c_void_p, ctypes.c_int64, ctypes.c_int
    st = P(torch.cuda.current_stream().cuda_stream)
    for trees, code in ((both, -3), (swapped, -1)):
        dt = _dev(wx, trees, np.uint8)
        out = wx.jl_empty((n, B), tdt, "cuda")
        out.fill_(-7.25)
        if fam == "iacwpd":
            rc = lib.wx_iacwpd1d_trees_f64(P(src.data_ptr()), P(out.data_ptr()), L64(n), L64(15), P(dt.data_ptr()), L64(n - 1), L64(B), st)
        else:
            fn = lib.wx_iswpd1d_trees_f32 if fam.endswith("f32") else lib.wx_iswpd1d_trees_f64
            rc = fn(P(src.data_ptr()), P(out.data_ptr()), L64(n), L64(15), P(dt.data_ptr()), L64(n - 1), L64(-1), L64(B),
                    P(q.ctypes.data), I(q.size), st)
        assert rc == code
        assert lib.wx_wpt_trees_last_route() == 0
        torch.cuda.synchronize()
        assert bool((out == -7.25).all())
    # the Python side raises what the single-tree forms raise, on either route
    wt = wx.wavelet(wx.WT.db4)
    if fam == "iswpd":
        for t in (both, _dev(wx, both)):
            with pytest.raises(IndexError, match="below the last column"):
                wx.iswpdall(src, wt, t)
            assert wx.wpt_trees_route() == "none"
        for t in (swapped, _dev(wx, swapped)):
            with pytest.raises(AssertionError, match="isvalidtree"):
                wx.iswpdall(src, wt, t, 1)
        with pytest.raises(AssertionError, match="main2depthshift"):
            wx.iswpdall(src, wt, _dev(wx, ok), 8)                      # sm < 2^3


# ---- the chain ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_redundant_best_basis_to_reconstruction_stays_on_the_device(wx, dtype):
    import torch
    n, D, B = 256, 6, 33
    rng = np.random.default_rng(256)
    wt = wx.wavelet(wx.WT.db4)
    tol = 20 * helpers.TOL[np.dtype(dtype)]
    x = np.asfortranarray(np.cumsum(rng.standard_normal((n, B)), axis=0).astype(dtype))   # random walks: trees of many shapes
    xd = wx.to_device(x)
    xw = wx.swpdall(xd, wt, D)
    M = wx.bestbasistreeall(xw, wx.BB(redundant=True), device=True)
    assert isinstance(M, torch.Tensor) and M.is_cuda and M.dtype == torch.bool and tuple(M.shape) == (n - 1, B)
    host = M.cpu().numpy()
    assert len({host[:, i].tobytes() for i in range(B)}) > 1
    back = wx.iswpdall(xw, wt, M)
    assert wx.wpt_trees_route() == LDS
    assert helpers.relerr(wx.to_numpy(back), x) <= tol
    assert _bytes(wx, back) == _bytes(wx, wx.iswpdall(xw, wt, host))
    assert helpers.relerr(wx.to_numpy(wx.iswpdall(xw, wt, M, 37)), x) <= tol
    if dtype == np.float64:
        xa = wx.acwpdall(xd, wt, D)
        Ma = wx.bestbasistreeall(xa, wx.BB(redundant=True), device=True)
        hosta = Ma.cpu().numpy()
        assert len({hosta[:, i].tobytes() for i in range(B)}) > 1
        back = wx.iacwpdall(xa, Ma)
        assert wx.wpt_trees_route() == LDS
        assert helpers.relerr(wx.to_numpy(back), x) <= tol
        assert _bytes(wx, back) == _bytes(wx, wx.iacwpdall(xa, wt, hosta))
