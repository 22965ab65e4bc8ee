"""wptall / iwptall / iwpdall of images with one quad tree per image (csrc/wx_wpt_trees2d.hip): what can be checked without a device
-- the six entry points exist at every layer, and every argument error is reported with its code before a device is needed."""
import ctypes
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OK, EASSERT, EARG = 0, -1, -2
i64, ci, vp = ctypes.c_int64, ctypes.c_int, ctypes.c_void_p
SYMS = [f + s for f in ("wx_wpt2d_trees", "wx_iwpt2d_trees", "wx_iwpd2d_trees") for s in ("_f64", "_f32")]
FAMS = ("wpt", "iwpt", "iwpd")


def test_symbols_exported_and_declared(wx):
    lib = ctypes.CDLL(wx.LIB_PATH)
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "waveletsext_hip.h")).read(), flags=re.S)
    jl = open(os.path.join(ROOT, "waveletsext.jl_amd", "julia", "libwx.jl")).read()
    for s in SYMS:
        assert hasattr(lib, s), s
        assert re.search(r"\bint %s\s*\(" % s, hdr), s
        assert "ccall((:%s, LIB)" % s in jl, s
        assert getattr(wx._lib.lib(), s).argtypes is not None, s       # the ctypes table has its prototype


class _Abi:
    """the three families at the C level, called the way the header declares them"""

    def __init__(self, wx, dtype, m, n, batch, k=3):
        self.lib = ctypes.CDLL(wx.LIB_PATH)
        self.suf = "_f64" if dtype == np.float64 else "_f32"
        q = np.ascontiguousarray(wx.wavelet(wx.WT.db4).qmf, dtype=np.float64)
        self.q, self.F = q, q.size
        self.k = k
        cnt = max(1, m * n * max(batch, 1))
        self.x = np.zeros(cnt, dtype=dtype)
        self.xw = np.zeros(cnt * k, dtype=dtype)
        self.y = np.ones(cnt, dtype=dtype)

    def call(self, fam, m, n, trees, ntree, batch, src=None, dst=None):
        fn = getattr(self.lib, "wx_%s2d_trees%s" % (fam, self.suf))
        fn.restype = ci
        src = (self.xw if fam == "iwpd" else self.x) if src is None else src
        dst = self.y if dst is None else dst
        tp = vp(trees.ctypes.data) if trees is not None else vp(0)
        args = [vp(src.ctypes.data), vp(dst.ctypes.data), i64(m), i64(n)]
        if fam == "iwpd":
            args.append(ci(self.k))
        args += [tp, i64(ntree), i64(batch), vp(self.q.ctypes.data), ci(self.F), vp(0)]
        return fn(*args)


def _tree(nt, *nodes):
    t = np.zeros(nt, dtype=np.uint8)
    t[[i - 1 for i in nodes]] = 1
    return t


def _cols(*trees):
    return np.asfortranarray(np.stack(trees, axis=1))


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("fam", FAMS)
def test_argument_errors_have_their_codes(wx, fam, dtype):
    m, n, B, nt = 8, 32, 3, 21                                         # gettreelength(8, 32) = 21: the shorter side decides
    assert wx.gettreelength(m, n) == nt
    a = _Abi(wx, dtype, m, n, B)
    good = _cols(_tree(nt, 1, 2), _tree(nt, 1, 5, 21), _tree(nt))
    # bad dimensions
    assert a.call(fam, 0, n, good, nt, B) == EARG
    assert a.call(fam, m, n, good, nt, -1) == EARG
    # ntree != gettreelength(m, n)
    assert a.call(fam, m, n, good, 85, B) == EASSERT
    assert a.call(fam, m, n, good, 20, B) == EASSERT
    # an invalid tree in the second of three columns: node 6 set under the cleared node 2
    bad = _cols(_tree(nt, 1, 2), _tree(nt, 1, 3, 6), _tree(nt))
    assert a.call(fam, m, n, bad, nt, B) == EASSERT
    # a tree deeper than both sides divide by: 8 x 12 has 21 nodes, but 12 = 4 * 3 takes two levels only
    assert wx.gettreelength(8, 12) == nt
    assert a.call(fam, 8, 12, _cols(_tree(nt, 1, 2), _tree(nt, 1, 5, 21), _tree(nt)), nt, B) == EASSERT
    # NULL trees
    assert a.call(fam, m, n, None, nt, B) == EARG
    # equal in / out pointers
    buf = a.xw if fam == "iwpd" else a.x
    assert a.call(fam, m, n, good, nt, B, src=buf, dst=buf) == EARG
    # nothing was written by any of them
    assert (a.y == 1).all()


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_iwpd_tree_deeper_than_the_table(wx, dtype):
    m, n, B, nt = 8, 8, 3, 21
    a = _Abi(wx, dtype, m, n, B, k=3)                                  # slices 0 .. 2: trees of depth <= 2
    deep = _cols(_tree(nt, 1, 2), _tree(nt, 1, 5, 21), _tree(nt))      # the second tree has depth 3
    assert a.call("iwpd", m, n, deep, nt, B) == EARG
    assert (a.y == 1).all()


def test_sides_rule_in_column_order(wx):
    """a tree deeper than both sides divide by is WX_EASSERT with the message of the sides, and the lowest offending column decides
    between it and a tree that is too deep for the table.  Only a side that is not dyadic admits such a tree: 8 x 12 has 21 nodes,
    12 = 4 * 3 takes two levels; on 8 x 32 the deepest tree of 21 nodes has depth 3 = min(log2 8, log2 32) and is no offender."""
    lib = ctypes.CDLL(wx.LIB_PATH)
    lib.wx_last_error.restype = ctypes.c_char_p
    nt, B = 21, 5
    a = _Abi(wx, np.float32, 8, 32, B, k=2)                            # buffers for either image
    three, two, flat = _tree(nt, 1, 5, 21), _tree(nt, 1, 2), _tree(nt)   # depth 3: deeper than 12 divides; depth 2: too deep for k = 2
    assert a.call("iwpd", 8, 12, _cols(flat, two, flat, three, flat), nt, B) == EARG          # behind a too deep one
    assert b"Not enough decomposition levels" in lib.wx_last_error()
    assert a.call("iwpd", 8, 12, _cols(flat, three, flat, two, flat), nt, B) == EASSERT       # and before it
    assert b"both sides must be divisible" in lib.wx_last_error()
    assert a.call("iwpd", 8, 12, _cols(flat, three, flat, flat, flat), nt, B) == EASSERT      # a column that is both: the sides first
    assert b"both sides must be divisible" in lib.wx_last_error()
    assert a.call("wpt", 8, 12, _cols(flat, two, flat, three, flat), nt, B) == EASSERT        # no k
    assert b"both sides must be divisible" in lib.wx_last_error()
    assert a.call("iwpd", 8, 32, _cols(flat, flat, flat, three, flat), nt, B) == EARG         # within the sides, below the table
    assert b"Not enough decomposition levels" in lib.wx_last_error()
    assert (a.y == 1).all()
    # the gather has no such rule, its sides need not be dyadic: the same tree is too deep for a table of 3 slices, nothing else
    fn = lib.wx_getbasiscoef2d_trees_f32
    fn.restype = ci
    xw, t = np.zeros(96 * 3 * B, dtype=np.float32), _cols(flat, three, flat, two, flat)
    assert fn(vp(xw.ctypes.data), vp(a.y.ctypes.data), i64(8), i64(12), ci(3), vp(t.ctypes.data), i64(nt), i64(B), vp(0)) == EARG
    assert b"Not enough decomposition levels" in lib.wx_last_error()
    assert (a.y == 1).all()


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("fam", FAMS)
def test_empty_batch_is_ok(wx, fam, dtype):
    a = _Abi(wx, dtype, 8, 8, 0)
    assert a.call(fam, 8, 8, None, 21, 0) == OK
    assert a.call(fam, 8, 8, np.zeros((21, 0), dtype=np.uint8), 21, 0) == OK


def test_python_number_of_nodes(wx):
    """ntree != gettreelength(m, n) gives AssertionError"""
    wt = wx.wavelet(wx.WT.db4)
    m, n, B = 8, 8, 3
    for rows in (20, 22, 85):
        trees = np.zeros((rows, B), dtype=bool)
        with pytest.raises(AssertionError, match="gettreelength"):
            wx.wptall(np.zeros((m, n, B)), wt, trees)
        with pytest.raises(AssertionError, match="gettreelength"):
            wx.iwptall(np.zeros((m, n, B)), wt, trees)
        with pytest.raises(AssertionError, match="gettreelength"):
            wx.iwpdall(np.zeros((m, n, 3, B)), wt, trees)
    with pytest.raises(AssertionError):                                # Utils.jl:210: one column per image
        wx.wptall(np.zeros((m, n, B)), wt, np.zeros((21, B + 1), dtype=bool))


def test_python_child_under_an_unset_parent(wx):
    """the lowest offending column decides: column 1 is no valid tree, column 2 would be too deep for the table"""
    wt = wx.wavelet(wx.WT.db4)
    m, n, nt = 8, 8, 21
    trees = _cols(_tree(nt, 1, 2), _tree(nt, 1, 3, 6), _tree(nt, 1, 5, 21)).astype(bool)
    with pytest.raises(AssertionError, match="isvalidtree"):
        wx.wptall(np.zeros((m, n, 3)), wt, trees)
    with pytest.raises(AssertionError, match="isvalidtree"):
        wx.iwptall(np.zeros((m, n, 3)), wt, trees)
    with pytest.raises(AssertionError, match="isvalidtree"):
        wx.iwpdall(np.zeros((m, n, 3, 3)), wt, trees)
    swapped = np.asfortranarray(trees[:, [0, 2, 1]])
    with pytest.raises(wx.ArgumentError, match="Not enough decomposition levels"):
        wx.iwpdall(np.zeros((m, n, 3, 3)), wt, swapped)


def test_python_empty_batch(wx):
    wt = wx.wavelet(wx.WT.db4)
    y = wx.wptall(np.zeros((8, 8, 0), order="F"), wt, np.zeros((21, 0), dtype=bool))
    assert y.shape == (8, 8, 0)
    assert wx.wpt_trees_route() == "host trees"
    xh = wx.iwpdall(np.zeros((8, 8, 3, 0), order="F"), wt, np.zeros((21, 0), dtype=bool))
    assert xh.shape == (8, 8, 0)
    assert wx.wpt_trees_route() == "host trees"


def test_python_host_data_with_device_trees(wx):
    import torch
    wt = wx.wavelet(wx.WT.db4)
    dt = torch.zeros((21, 3), dtype=torch.bool, device="meta")          # a tensor that is not in host memory; its bytes are never read
    with pytest.raises(TypeError, match="same device"):
        wx.wptall(np.zeros((8, 8, 3)), wt, dt)
    with pytest.raises(TypeError, match="same device"):
        wx.iwptall(np.zeros((8, 8, 3)), wt, dt)
    with pytest.raises(TypeError, match="same device"):
        wx.iwpdall(np.zeros((8, 8, 3, 3)), wt, dt)
