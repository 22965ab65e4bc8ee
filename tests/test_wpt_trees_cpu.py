"""wptall / iwptall / iwpdall with one tree per signal (csrc/wx_wpt_trees.hip): what can be checked without a device -- the six
entry points exist at every layer, and every argument error is reported with its code before a device is needed."""
import ctypes
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OK, EASSERT, EARG = 0, -1, -2
i64, ci, vp = ctypes.c_int64, ctypes.c_int, ctypes.c_void_p
SYMS = [f + s for f in ("wx_wpt1d_trees", "wx_iwpt1d_trees", "wx_iwpd1d_trees") for s in ("_f64", "_f32")]


def test_symbols_exported_and_declared(wx):
    lib = ctypes.CDLL(wx.LIB_PATH)
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "waveletsext_hip.h")).read(), flags=re.S)
    jl = open(os.path.join(ROOT, "waveletsext.jl_amd", "julia", "libwx.jl")).read()
    for s in SYMS:
        assert hasattr(lib, s), s
        assert re.search(r"\bint %s\s*\(" % s, hdr), s
        assert "ccall((:%s, LIB)" % s in jl, s


class _Abi:
    """the three families at the C level, called the way the header declares them"""

    def __init__(self, wx, dtype, n, batch, k=4):
        self.lib = ctypes.CDLL(wx.LIB_PATH)
        self.suf = "_f64" if dtype == np.float64 else "_f32"
        q = np.ascontiguousarray(wx.wavelet(wx.WT.db4).qmf, dtype=np.float64)
        self.q, self.F = q, q.size
        self.k = k
        cnt = max(1, abs(n) * max(batch, 1))
        self.x = np.zeros(cnt, dtype=dtype)
        self.xw = np.zeros(cnt * k, dtype=dtype)
        self.y = np.ones(cnt, dtype=dtype)

    def call(self, fam, n, trees, ntree, batch, src=None, dst=None):
        fn = getattr(self.lib, "wx_%s1d_trees%s" % (fam, self.suf))
        fn.restype = ci
        src = (self.xw if fam == "iwpd" else self.x) if src is None else src
        dst = self.y if dst is None else dst
        tp = vp(trees.ctypes.data) if trees is not None else vp(0)
        args = [vp(src.ctypes.data), vp(dst.ctypes.data), i64(n)]
        if fam == "iwpd":
            args.append(ci(self.k))
        args += [tp, i64(ntree), i64(batch), vp(self.q.ctypes.data), ci(self.F), vp(0)]
        return fn(*args)


FAMS = ("wpt", "iwpt", "iwpd")


def _cols(*trees):
    return np.asfortranarray(np.stack([np.asarray(t, dtype=np.uint8) for t in trees], axis=1))


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("fam", FAMS)
def test_argument_errors_have_their_codes(wx, fam, dtype):
    n, B = 8, 3
    a = _Abi(wx, dtype, n, B)
    good = _cols([1, 1, 0, 0, 0, 0, 0], [1, 0, 1, 0, 0, 0, 0], [0] * 7)
    # ntree != n - 1
    assert a.call(fam, n, good, 6, B) == EASSERT
    # n not dyadic
    assert a.call(fam, 12, _cols([0] * 11, [0] * 11, [0] * 11), 11, B) == EASSERT
    # an invalid tree in the second of three columns: node 4 set under the cleared node 2
    bad = _cols([1, 1, 0, 0, 0, 0, 0], [1, 0, 1, 1, 0, 0, 0], [0] * 7)
    assert a.call(fam, n, bad, 7, B) == EASSERT
    # NULL trees
    assert a.call(fam, n, None, 7, B) == EARG
    # equal in / out pointers
    buf = a.xw if fam == "iwpd" else a.x
    assert a.call(fam, n, good, 7, B, src=buf, dst=buf) == EARG
    # nothing was written by any of them
    assert (a.y == 1).all()


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_iwpd_tree_deeper_than_the_table(wx, dtype):
    n, B = 8, 3
    a = _Abi(wx, dtype, n, B, k=3)                      # columns 0 .. 2: trees of depth <= 2
    deep = _cols([1, 1, 0, 0, 0, 0, 0], [1, 1, 1, 0, 1, 0, 0], [0] * 7)      # the second tree has depth 3
    assert a.call("iwpd", n, deep, 7, B) == EARG
    assert (a.y == 1).all()


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("fam", FAMS)
def test_empty_batch_is_ok(wx, fam, dtype):
    a = _Abi(wx, dtype, 8, 0)
    assert a.call(fam, 8, None, 7, 0) == OK
    assert a.call(fam, 8, np.zeros((7, 0), dtype=np.uint8), 7, 0) == OK


def test_python_checks_the_number_of_trees(wx):
    wt = wx.wavelet(wx.WT.db4)
    n, B = 16, 3
    trees = np.zeros((n - 1, B + 1), dtype=bool)
    with pytest.raises(AssertionError):
        wx.wptall(np.zeros((n, B)), wt, trees)
    with pytest.raises(AssertionError):
        wx.iwptall(np.zeros((n, B)), wt, trees)
    with pytest.raises(AssertionError):
        wx.iwpdall(np.zeros((n, 5, B)), wt, trees)
