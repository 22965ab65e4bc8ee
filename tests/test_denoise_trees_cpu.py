"""denoiseall with one tree per signal (csrc/wx_denoise_trees.hip): what can be checked without a device -- the entry is exported and
declared at every layer, every argument error comes back with its code before a device is needed (and resets the route record), and
the Python side refuses what the entry does not cover (images, redundant input types)."""
import ctypes
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OK, EASSERT, EARG, EUNSUPPORTED = 0, -1, -2, -11
P, L64, I, D = ctypes.c_void_p, ctypes.c_int64, ctypes.c_int, ctypes.c_double


def test_entries_are_exported_and_declared(wx):
    lib = ctypes.CDLL(wx.LIB_PATH)
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "waveletsext_hip.h")).read(), flags=re.S)
    jl = open(os.path.join(ROOT, "waveletsext.jl_amd", "julia", "libwx.jl")).read()
    shim = open(os.path.join(ROOT, "waveletsext.jl_amd", "julia", "WaveletsExtHIP.jl")).read()
    for suf in ("_f64", "_f32"):
        name = "wx_denoise_wpt1d_trees" + suf
        assert hasattr(lib, name)
        assert re.search(r"\bint %s\s*\(" % name, hdr)
        assert "ccall((:%s, LIB)" % name in jl
        assert getattr(wx._lib.lib(), name).argtypes is not None
    assert "wx_denoise_wpt1d_trees(T, " in shim and "tree::Union{BitVector,BitMatrix}" in shim
    assert callable(wx.noisestall)


def _call(wx, n=8, B=2, ntree=None, th_kind=0, nthr=0, thr=False, alias=False, trees=True, out=True, sigma=True, bits=None, suffix="_f64"):
    dt = np.float64 if suffix == "_f64" else np.float32
    q = np.ascontiguousarray(wx.wavelet(wx.WT.haar).qmf, dtype=np.float64)
    ntree = n - 1 if ntree is None else ntree
    x = np.zeros((max(n, 1), max(B, 1)), dtype=dt, order="F")
    y = np.full(x.shape, -7.25, dtype=dt, order="F")
    s = np.full(max(B, 1), -7.25, dtype=dt)
    t = np.zeros((max(ntree, 1), max(B, 1)), dtype=np.uint8, order="F") if bits is None else np.asfortranarray(bits.astype(np.uint8))
    tv = np.ones(max(B, 1), dtype=dt)
    fn = getattr(wx._lib.lib(), "wx_denoise_wpt1d_trees" + suffix)
    rc = fn(P(x.ctypes.data), P(x.ctypes.data if alias else (y.ctypes.data if out else 0)), L64(n), P(t.ctypes.data if trees else 0), L64(ntree),
            L64(B), P(q.ctypes.data), I(q.size), I(th_kind), D(1.0), P(tv.ctypes.data if thr else 0), L64(nthr), I(0),
            P(s.ctypes.data if sigma else 0), P(0))
    assert (y == -7.25).all() and (s == -7.25).all()                  # nothing is written by a call that does not reach a device
    return rc


@pytest.mark.parametrize("suffix", ["_f64", "_f32"])
def test_argument_errors_need_no_device(wx, suffix):
    lib = wx._lib.lib()
    c = lambda **kw: _call(wx, suffix=suffix, **kw)
    for kw, code in (({"th_kind": 4}, EARG), ({"th_kind": -1}, EARG),
                     ({"nthr": 3, "thr": True, "B": 5}, EARG),         # neither 0, 1 nor the batch
                     ({"nthr": 1, "thr": False}, EARG), ({"nthr": 0, "thr": True}, EARG),
                     ({"ntree": 6}, EASSERT), ({"ntree": 8}, EASSERT),
                     ({"n": 12, "ntree": 11}, EASSERT),                # not dyadic
                     ({"alias": True}, EARG), ({"trees": False}, EARG), ({"n": 0, "ntree": 0}, EARG), ({"B": -1}, EARG),
                     ({"out": False, "sigma": False}, EARG)):
        assert c(**kw) == code, kw
        assert lib.wx_wpt_trees_last_route() == 0, kw
    assert c(B=0) == OK                                                # an empty batch is WX_OK before a device is needed
    assert lib.wx_wpt_trees_last_route() == 1
    # the order of the driver: the dimensions and the aliasing come before the entry's own arguments, those before the tree's length
    assert c(th_kind=9, alias=True) == EARG and c(th_kind=9, ntree=3) == EARG and c(n=12, ntree=3) == EASSERT


def test_invalid_tree_is_reported_before_a_device_is_needed(wx):
    """a host matrix is checked on the host (wx_trees_check_host): the first offending column decides, nothing is written"""
    n, B = 16, 5
    bits = np.zeros((n - 1, B), dtype=bool)
    bits[0, :] = True
    bits[3, 3] = True                                                  # node 4 under a cleared node 2
    assert _call(wx, n=n, B=B, bits=bits) == EASSERT
    assert "isvalidtree" in wx._lib.lib().wx_last_error().decode()
    assert wx._lib.lib().wx_wpt_trees_last_route() == 0


def test_python_refuses_what_the_entry_does_not_cover(wx):
    wt = wx.wavelet(wx.WT.db4)
    n, B = 16, 3
    M = np.zeros((n - 1, B), dtype=bool)
    for it, shape in (("dwt", (n, B)), ("sig", (n, B)), ("sdwt", (n, 3, B)), ("swpd", (n, 7, B)), ("acdwt", (n, 3, B)), ("acwpd", (n, 7, B))):
        with pytest.raises(wx.WxError) as e:
            wx.denoiseall(np.zeros(shape), it, wt, tree=M)
        assert e.value.code == EUNSUPPORTED, it
    with pytest.raises(wx.WxError) as e:                               # images: the quad trees of wptall have no denoising entry
        wx.denoiseall(np.zeros((n, n, B)), "wpt", wt, tree=np.zeros((wx.gettreelength(n, n), B), dtype=bool))
    assert e.value.code == EUNSUPPORTED
    with pytest.raises(wx.WxError) as e:
        wx.noisestall(np.zeros((n, 3, B)), True, M)
    assert e.value.code == EUNSUPPORTED
    with pytest.raises(wx.WxError) as e:                               # an estimator the device path does not have
        wx.denoiseall(np.zeros((n, B)), "wpt", wt, tree=M, estnoise=lambda x, r, t: 1.0)
    assert e.value.code == EUNSUPPORTED
    with pytest.raises(AssertionError):                                # Utils.jl:210: one column per signal
        wx.denoiseall(np.zeros((n, B)), "wpt", wt, tree=np.zeros((n - 1, B + 1), dtype=bool))
    assert wx.denoiseall(np.zeros((n, 0)), "wpt", wt, tree=np.zeros((n - 1, 0), dtype=bool)).shape == (n, 0)
    assert wx.noisestall(np.zeros((n, 0)), False, np.zeros((n - 1, 0), dtype=bool)).shape == (0,)
