"""iswpdall / iacwpdall with one tree per signal (csrc/wx_red_trees.hip): what can be checked without a device -- the three entry
points exist at every layer, and every argument error is reported with the code of the single-tree entries before a device is needed,
with the output untouched and the route reset."""
import ctypes
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OK, EASSERT, EARG, EBOUNDS, EUNSUPPORTED = 0, -1, -2, -3, -11
i64, ci, vp = ctypes.c_int64, ctypes.c_int, ctypes.c_void_p
SYMS = ["wx_iswpd1d_trees_f64", "wx_iswpd1d_trees_f32", "wx_iacwpd1d_trees_f64"]
FAMS = [("iswpd", np.float64), ("iswpd", np.float32), ("iacwpd", np.float64)]


def test_symbols_exported_declared_bound_and_typed(wx):
    lib = ctypes.CDLL(wx.LIB_PATH)
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "waveletsext_hip.h")).read(), flags=re.S)
    jl = open(os.path.join(ROOT, "waveletsext.jl_amd", "julia", "libwx.jl")).read()
    shim = open(os.path.join(ROOT, "waveletsext.jl_amd", "julia", "WaveletsExtHIP.jl")).read()
    for s in SYMS:
        assert hasattr(lib, s), s
        assert re.search(r"\bint %s\s*\(" % s, hdr), s
        assert "ccall((:%s, LIB)" % s in jl, s
        assert re.search(r"\b%s\(" % s[:-4], shim), s
        fn = getattr(wx._lib.lib(), s)
        assert fn.argtypes is not None and len(fn.argtypes) == (8 if "iacwpd" in s else 11), s
    assert not hasattr(lib, "wx_iacwpd1d_trees_f32")                  # the autocorrelation family is Float64 only


class _Abi:
    """the two families at the C level, called the way the header declares them; x starts at the sentinel 1"""

    def __init__(self, wx, fam, dtype, n, ncols, batch):
        self.lib = ctypes.CDLL(wx.LIB_PATH)
        self.fam = fam
        self.fn = getattr(self.lib, "wx_%s1d_trees%s" % (fam, "_f64" if dtype == np.float64 else "_f32"))
        self.fn.restype = ci
        self.route = self.lib.wx_wpt_trees_last_route
        self.route.restype = ci
        q = np.ascontiguousarray(wx.wavelet(wx.WT.db4).qmf, dtype=np.float64)
        self.q, self.F = q, q.size
        self.ncols = ncols
        self.xw = np.zeros(max(1, abs(n) * abs(ncols) * max(batch, 1)), dtype=dtype)
        self.x = np.ones(max(1, abs(n) * max(batch, 1)), dtype=dtype)

    def call(self, n, trees, ntree, batch, sm=-1, src=None, dst=None, ncols=None):
        src = self.xw if src is None else src
        dst = self.x if dst is None else dst
        tp = vp(trees.ctypes.data) if trees is not None else vp(0)
        args = [vp(src.ctypes.data), vp(dst.ctypes.data), i64(n), i64(self.ncols if ncols is None else ncols), tp, i64(ntree)]
        if self.fam == "iswpd":
            args += [i64(sm), i64(batch), vp(self.q.ctypes.data), ci(self.F), vp(0)]
        else:
            args += [i64(batch), vp(0)]
        return self.fn(*args)

    def rejected(self, code, *args, **kw):
        """the code, the output at its sentinel, the route reset"""
        rc = self.call(*args, **kw)
        return rc == code and bool((self.x == 1).all()) and self.route() == 0


def _cols(*trees):
    return np.asfortranarray(np.stack([np.asarray(t, dtype=np.uint8) for t in trees], axis=1))


GOOD = ([1, 1, 0, 0, 0, 0, 0], [1, 0, 1, 0, 0, 0, 0], [0] * 7)        # depths 2, 2, 0
BAD = [1, 0, 1, 1, 0, 0, 0]                                           # node 4 set under the cleared node 2
DEEP = [1, 1, 1, 0, 1, 0, 0]                                          # depth 3


@pytest.mark.parametrize("fam,dtype", FAMS)
def test_argument_errors_have_their_codes(wx, fam, dtype):
    n, B, m = 8, 3, 7                                                 # a table of depth 2: columns 1 .. 7
    a = _Abi(wx, fam, dtype, n, m, B)
    good = _cols(*GOOD)
    # bad dimensions
    assert a.rejected(EARG, 0, good, 7, B)
    assert a.rejected(EARG, n, good, 7, -1)
    assert a.rejected(EARG, n, good, 7, B, ncols=0)
    # equal in / out pointers, NULL trees
    assert a.rejected(EARG, n, good, 7, B, src=a.x, dst=a.x)
    assert a.rejected(EARG, n, None, 7, B)
    # n not dyadic, ntree != n - 1
    assert a.rejected(EASSERT, 12, _cols([0] * 11, [0] * 11, [0] * 11), 11, B)
    assert a.rejected(EASSERT, n, good, 6, B)
    # an invalid tree in the second of three columns
    assert a.rejected(EASSERT, n, _cols(GOOD[0], BAD, GOOD[2]), 7, B)
    # a tree deeper than the table, in the last column
    assert a.rejected(EBOUNDS, n, _cols(GOOD[0], GOOD[1], DEEP), 7, B)
    # the lowest offending column decides
    assert a.rejected(EBOUNDS, n, _cols(GOOD[0], DEEP, BAD), 7, B)
    assert a.rejected(EASSERT, n, _cols(GOOD[0], BAD, DEEP), 7, B)
    # depth 2 needs seven columns: six hold depth 1 only
    assert a.rejected(EBOUNDS, n, good, 7, B, ncols=6)


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_shift_beyond_the_table_depth(wx, dtype):
    n, B, m = 8, 3, 7
    a = _Abi(wx, "iswpd", dtype, n, m, B)
    good = _cols(*GOOD)
    assert a.rejected(EASSERT, n, good, 7, B, sm=4)                   # main2depthshift: sm < 2^getdepth(7) = 4
    assert a.rejected(EASSERT, n, good, 7, B, sm=1 << 40)
    # the content-free check comes before the columns are read
    assert a.rejected(EASSERT, n, _cols(GOOD[0], DEEP, GOOD[2]), 7, B, sm=4)


@pytest.mark.parametrize("fam,dtype", FAMS)
def test_empty_batch_is_ok(wx, fam, dtype):
    a = _Abi(wx, fam, dtype, 8, 7, 0)
    assert a.call(8, None, 7, 0) == OK
    assert a.call(8, np.zeros((7, 0), dtype=np.uint8), 7, 0) == OK
    assert (a.x == 1).all()


def test_python_rejects_images_with_a_matrix(wx):
    wt = wx.wavelet(wx.WT.db4)
    B = 3
    quad = np.zeros((5, B), dtype=bool)                               # gettreelength(8, 8) = 5
    for call in (lambda: wx.iswpdall(np.zeros((8, 8, 5, B)), wt, quad),
                 lambda: wx.iswpdall(np.zeros((8, 8, 5, B)), wt, quad, 1),
                 lambda: wx.iacwpdall(np.zeros((8, 8, 5, B)), quad),
                 lambda: wx.iacwpdall(np.zeros((8, 8, 5, B)), wt, quad),
                 lambda: wx.iswpd(np.zeros((8, 8, 5)), wt, quad[:, :1]),
                 lambda: wx.iacwpd(np.zeros((8, 8, 5)), quad[:, :1])):
        with pytest.raises(wx.WxError) as e:
            call()
        assert e.value.code == EUNSUPPORTED


def test_python_checks_the_number_of_trees(wx):
    wt = wx.wavelet(wx.WT.db4)
    n, B = 16, 3
    trees = np.zeros((n - 1, B + 1), dtype=bool)
    with pytest.raises(AssertionError):
        wx.iswpdall(np.zeros((n, 7, B)), wt, trees)
    with pytest.raises(AssertionError):
        wx.iswpdall(np.zeros((n, 7, B)), wt, trees.astype(np.uint8), 2)
    with pytest.raises(AssertionError):
        wx.iacwpdall(np.zeros((n, 7, B)), trees)
    with pytest.raises(AssertionError):
        wx.iacwpdall(np.zeros((n, 7, B)), wt, trees)
    with pytest.raises(AssertionError):                               # a single signal takes one column
        wx.iswpd(np.zeros((n, 7)), wt, trees[:, :2])
    with pytest.raises(AssertionError):
        wx.iacwpd(np.zeros((n, 7)), trees[:, :2])
