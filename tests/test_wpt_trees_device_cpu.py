"""Per-signal tree matrices in device memory (csrc/wx_trees_prep.hip): what can be checked without a device -- the route query
exists at every layer, bestbasistreeall(..., device=True) refuses host arrays before it needs a device, and the bit layout that the
host pass and the prep kernel share (csrc/wx_tree_bits.h) is numpy's little-endian packing."""
import ctypes
import os
import re

import numpy as np
import pytest

import helpers

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_route_query_is_exported_and_declared(wx):
    lib = ctypes.CDLL(wx.LIB_PATH)
    assert hasattr(lib, "wx_wpt_trees_last_route")
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "waveletsext_hip.h")).read(), flags=re.S)
    assert re.search(r"\bint wx_wpt_trees_last_route\s*\(void\)", hdr)
    jl = open(os.path.join(ROOT, "waveletsext.jl_amd", "julia", "libwx.jl")).read()
    assert "ccall((:wx_wpt_trees_last_route, LIB)" in jl
    assert wx.wpt_trees_route() in wx.WPT_TREES_ROUTES.values()
    assert sorted(wx.WPT_TREES_ROUTES) == list(range(6)) and len(set(wx.WPT_TREES_ROUTES.values())) == 6


def test_route_is_none_after_a_refused_call_and_host_after_an_empty_one(wx):
    wt = wx.wavelet(wx.WT.db4)
    wx.wptall(np.zeros((8, 0)), wt, np.zeros((7, 0), dtype=bool))     # an empty batch is WX_OK before a device is needed
    assert wx.wpt_trees_route() == "host trees"
    with pytest.raises(AssertionError):
        wx.wptall(np.zeros((8, 2)), wt, np.ones((6, 2), dtype=bool))  # ntree != n - 1
    assert wx.wpt_trees_route() == "none"


def test_device_trees_of_a_host_array_is_a_type_error(wx):
    with pytest.raises(TypeError):
        wx.bestbasistreeall(np.zeros((8, 4, 3)), wx.BB(), device=True)
    import torch
    with pytest.raises(TypeError):
        wx.bestbasistreeall(torch.zeros((8, 4, 3), dtype=torch.float64), wx.BB(), device=True)   # a CPU tensor is no device tensor


def _mix(wx, n, rng):
    L = int(n).bit_length() - 1
    chain = np.zeros(n - 1, dtype=bool)
    node = 1
    for _ in range(L):
        chain[node - 1] = True
        node = 2 * node + 1                                            # right-deep: ends at node n - 1, the last byte
    cols = [np.zeros(n - 1, dtype=bool), wx.maketree(n, L, "full"), wx.maketree(n, L, "dwt"), chain]
    cols += [helpers.random_tree_1d(n, rng, p) for p in (0.3, 0.7, 0.9)]
    return cols


@pytest.mark.parametrize("n", [8, 64, 128])
def test_shared_bit_layout_is_little_endian_packbits(wx, n):
    """csrc/wx_debug.h: wx_debug_pack_tree1d runs wt_pack_host of csrc/wx_tree_bits.h, the routine of the host route"""
    lib = ctypes.CDLL(wx.LIB_PATH)
    lib.wx_debug_pack_tree1d.argtypes = [ctypes.c_void_p, ctypes.c_int64, ctypes.c_void_p]
    lib.wx_debug_pack_tree1d.restype = ctypes.c_int
    rng = np.random.default_rng(n)
    nw = max(n // 32, 1)
    for t in _mix(wx, n, rng):
        for val in (1, 2, 255):                                        # any non-zero byte is a decomposed node
            tb = np.ascontiguousarray(t.astype(np.uint8) * val)
            words = np.full(nw + 1, 0xDEADBEEF, dtype=np.uint32)
            assert lib.wx_debug_pack_tree1d(tb.ctypes.data, n, words.ctypes.data) == nw
            want = np.zeros(nw * 4, dtype=np.uint8)
            packed = np.packbits(t, bitorder="little")
            want[:packed.size] = packed
            assert (words[:nw].view(np.uint8) == want).all()
            assert words[nw] == 0xDEADBEEF                             # nothing past the column's words
            for i in range(1, n):                                      # node i is bit (i - 1) & 31 of word (i - 1) >> 5
                assert bool((int(words[(i - 1) >> 5]) >> ((i - 1) & 31)) & 1) == bool(t[i - 1])
    assert lib.wx_debug_pack_tree1d(None, n, None) == -2
