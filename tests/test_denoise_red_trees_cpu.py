"""denoiseall(xw, "swpd" | "acwpd", wt, tree=M) with one tree per signal (csrc/wx_denoise_red_trees.hip): what can be checked without a
device -- the entries are exported and declared at every layer, every argument error comes back with its code before a device is needed
(nothing written, the route record reset), the lowest offending column of a host matrix decides, and the Python side refuses the
estimators that have no per-signal leaf masks and, as before, a packet table in host memory."""
import ctypes
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OK, EASSERT, EARG, EBOUNDS, EUNSUPPORTED = 0, -1, -2, -3, -11
P, L64, I, D = ctypes.c_void_p, ctypes.c_int64, ctypes.c_int, ctypes.c_double
ENTRIES = ("wx_denoise_swpd1d_trees_f64", "wx_denoise_swpd1d_trees_f32", "wx_denoise_acwpd1d_trees_f64")


def test_header_lib_and_julia_agree_on_the_entries(wx):
    lib = ctypes.CDLL(wx.LIB_PATH)
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "waveletsext_hip.h")).read(), flags=re.S)
    jl = open(os.path.join(ROOT, "waveletsext.jl_amd", "julia", "libwx.jl")).read()
    shim = open(os.path.join(ROOT, "waveletsext.jl_amd", "julia", "WaveletsExtHIP.jl")).read()
    for name in ENTRIES:
        assert hasattr(lib, name), name
        m = re.search(r"\bint %s\s*\(([^;]*)\)\s*;" % name, hdr)
        assert m, name
        nargs = len(m.group(1).split(","))
        assert nargs == (14 if "acwpd" in name else 16)
        assert len(getattr(wx._lib.lib(), name).argtypes) == nargs, name
        c = re.search(r"ccall\(\(:%s, LIB\), Cint, \(([^)]*)\)" % name, jl)
        assert c and len(c.group(1).split(",")) == nargs, name
    assert not hasattr(lib, "wx_denoise_acwpd1d_trees_f32")           # the autocorrelation family is Float64 only
    assert "wx_denoise_swpd1d_trees(T, " in shim and "wx_denoise_acwpd1d_trees(Float64, " in shim


def _call(wx, name="wx_denoise_swpd1d_trees_f64", n=8, ncols=15, B=2, ntree=None, th_kind=0, nthr=0, thr=False, alias=False, trees=True, out=True,
          sigma=True, bits=None):
    dt = np.float32 if name.endswith("f32") else np.float64
    q = np.ascontiguousarray(wx.wavelet(wx.WT.haar).qmf, dtype=np.float64)
    ntree = n - 1 if ntree is None else ntree
    x = np.zeros((max(n, 1), max(ncols, 1), max(B, 1)), dtype=dt, order="F")
    y = np.full((max(n, 1), max(B, 1)), -7.25, dtype=dt, order="F")
    s = np.full(max(B, 1), -7.25, dtype=dt)
    t = np.zeros((max(ntree, 1), max(B, 1)), dtype=np.uint8, order="F") if bits is None else np.asfortranarray(bits.astype(np.uint8))
    tv = np.ones(max(B, 1), dtype=dt)
    fn = getattr(wx._lib.lib(), name)
    head = (P(x.ctypes.data), P(x.ctypes.data if alias else (y.ctypes.data if out else 0)), L64(n), L64(ncols), P(t.ctypes.data if trees else 0),
            L64(ntree), L64(B))
    tail = (I(th_kind), D(1.0), P(tv.ctypes.data if thr else 0), L64(nthr), I(0), P(s.ctypes.data if sigma else 0), P(0))
    rc = fn(*head, *tail) if "acwpd" in name else fn(*head, P(q.ctypes.data), I(q.size), *tail)
    assert (y == -7.25).all() and (s == -7.25).all()                  # nothing is written by a call that does not reach a device
    return rc


def _route(wx):
    return wx._lib.lib().wx_wpt_trees_last_route()


@pytest.mark.parametrize("name", ENTRIES)
def test_earg_before_a_device_is_needed(wx, name):
    for kw in ({"n": 0, "ntree": 0}, {"ncols": 0}, {"B": -1},          # bad dimensions
               {"trees": False}, {"alias": True},
               {"th_kind": 4}, {"th_kind": -1},
               {"nthr": 3, "thr": True, "B": 5},                       # neither 0, 1 nor the batch
               {"nthr": 1, "thr": False}, {"nthr": 0, "thr": True},
               {"out": False, "sigma": False}):
        assert _call(wx, name, **kw) == EARG, kw
        assert _route(wx) == 0, kw


@pytest.mark.parametrize("name", ENTRIES)
def test_eassert_before_a_device_is_needed(wx, name):
    n = 16
    bad = np.zeros((n - 1, 3), dtype=bool)
    bad[0, :] = True
    bad[3, 1] = True                                                   # node 4 under a cleared node 2
    for kw in ({"n": 12, "ntree": 11},                                 # not dyadic
               {"ntree": 6}, {"ntree": 8},
               {"n": n, "ncols": 31, "B": 3, "bits": bad}):
        assert _call(wx, name, **kw) == EASSERT, kw
        assert _route(wx) == 0, kw
    assert "isvalidtree" in wx._lib.lib().wx_last_error().decode()
    # the order of the driver: the dimensions and the aliasing come before the entry's own arguments, those before the tree's length
    assert _call(wx, name, th_kind=9, alias=True) == EARG and _call(wx, name, th_kind=9, ntree=3) == EARG
    assert _call(wx, name, n=12, ntree=3) == EASSERT


@pytest.mark.parametrize("name", ENTRIES)
def test_ebounds_for_a_column_deeper_than_the_table(wx, name):
    n = 16
    deep = np.zeros((n - 1, 3), dtype=bool)
    deep[0, :] = True
    deep[1, 2] = True                                                  # depth 2: leaves in columns 3 .. 6
    assert _call(wx, name, n=n, ncols=3, B=3, bits=deep) == EBOUNDS   # a table of depth 1
    assert _route(wx) == 0
    assert "below the last column" in wx._lib.lib().wx_last_error().decode()
    assert _call(wx, name, n=n, ncols=6, B=3, bits=deep) == EBOUNDS   # 2^(2 + 1) - 1 = 7 columns are needed
    assert _route(wx) == 0


@pytest.mark.parametrize("name", ENTRIES)
def test_the_lowest_offending_column_decides(wx, name):
    n, B = 16, 6
    base = np.zeros((n - 1, B), dtype=bool)
    base[0, :] = True
    invalid = np.zeros(n - 1, dtype=bool)
    invalid[0] = invalid[3] = True                                     # node 4 under a cleared node 2
    deep = np.zeros(n - 1, dtype=bool)
    deep[0] = deep[1] = True                                           # depth 2 in a table of depth 1
    a = base.copy()
    a[:, 2], a[:, 4] = deep, invalid
    assert _call(wx, name, n=n, ncols=3, B=B, bits=a) == EBOUNDS
    assert _route(wx) == 0
    b = base.copy()
    b[:, 2], b[:, 4] = invalid, deep
    assert _call(wx, name, n=n, ncols=3, B=B, bits=b) == EASSERT
    assert _route(wx) == 0


@pytest.mark.parametrize("name", ENTRIES)
def test_an_empty_batch_is_ok(wx, name):
    assert _call(wx, name, B=0) == OK
    assert _route(wx) == 1
    assert _call(wx, name, B=0, out=False, sigma=False) == OK         # nothing is asked of an empty batch


def test_python_refuses_the_selections_without_leaf_masks(wx):
    wt = wx.wavelet(wx.WT.db4)
    n, B = 16, 3
    M = np.zeros((n - 1, B), dtype=bool)
    for it in ("swpd", "acwpd"):
        for est in (wx.relerrorthreshold, wx.surethreshold):
            with pytest.raises(wx.WxError) as e:
                wx.denoiseall(np.zeros((n, 7, B)), it, wt, tree=M, estnoise=est)
            assert e.value.code == EUNSUPPORTED and "leaf masks" in str(e.value), (it, est)
        with pytest.raises(wx.WxError) as e:                           # an estimator the device path does not have
            wx.denoiseall(np.zeros((n, 7, B)), it, wt, tree=M, estnoise=lambda x, r, t: 1.0)
        assert e.value.code == EUNSUPPORTED
        with pytest.raises(wx.WxError) as e:                           # tables of images
            wx.denoiseall(np.zeros((n, n, 5, B)), it, wt, tree=M)
        assert e.value.code == EUNSUPPORTED and "1-D" in str(e.value)


def test_python_keeps_refusing_a_packet_table_in_host_memory(wx):
    """the Python layer takes a tree matrix with a redundant table only where the table is a device tensor; a numpy table is refused as it
    always was (tests/test_denoise_trees_cpu.py), now with a message that names the way out.  The C entries take either."""
    wt = wx.wavelet(wx.WT.db4)
    n, B = 16, 3
    M = np.zeros((n - 1, B), dtype=bool)
    calls = [lambda: wx.denoiseall(np.zeros((n, 7, B)), "swpd", wt, tree=M), lambda: wx.denoiseall(np.zeros((n, 7, B)), "swpd", None, tree=M),
             lambda: wx.denoiseall(np.zeros((n, 7, B)), "acwpd", wt, tree=M), lambda: wx.denoiseall(np.zeros((n, 7, B)), "swpd", wt, tree=M, estnoise=1.0),
             lambda: wx.denoise(np.zeros((n, 7)), "swpd", wt, tree=M[:, :1]), lambda: wx.noisestall(np.zeros((n, 7, B)), True, M),
             lambda: wx.denoiseall(np.zeros((n, 7, 0)), "swpd", wt, tree=M[:, :0])]
    for i, call in enumerate(calls):
        with pytest.raises(wx.WxError) as e:
            call()
        assert e.value.code == EUNSUPPORTED and "on the device" in str(e.value), i
