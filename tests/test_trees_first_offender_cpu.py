"""The column check of a HOST tree matrix (wx_trees_check_host, csrc/wx_trees_prep.hip), as every per-signal-tree entry reports it:
the lowest offending column decides the code -- no valid tree WX_EASSERT, too deep for the table WX_EARG -- whether one thread
checks the matrix or, from 2^22 matrix bytes on, up to eight do, a range of columns each.  Argument errors return before a device is
needed, so this runs anywhere; a call that passes the checks ends at WX_EHIP where no device is visible and at WX_OK where one is."""
import ctypes
import functools

import numpy as np
import pytest

OK, EASSERT, EARG, EHIP = 0, -1, -2, -10
i64, ci, vp = ctypes.c_int64, ctypes.c_int, ctypes.c_void_p
K = 3
# (sides, nodes per tree, columns of a matrix of >= 2^22 bytes, columns of a small one)
SHAPES = {"1d": ((1024,), 1023, 4104, 9), "2d": ((16, 16), 85, 49352, 9)}
# nodes of a tree of depth 3 (too deep for k = 3) and of one with a node under an unset parent, in either heap
DEEP = {"1d": (1, 2, 4), "2d": (1, 2, 6)}
ORPHAN = {"1d": (1, 3, 4), "2d": (1, 3, 6)}
FAMS = ("wpt", "iwpt", "iwpd", "getbasiscoef")


@functools.lru_cache(maxsize=None)
def _buffers(dim, batch):
    """input (zeros, never touched before a call passes its checks), output (ones)"""
    sides = SHAPES[dim][0]
    cnt = int(np.prod(sides)) * batch
    return np.zeros(cnt * K, dtype=np.float32), np.ones(cnt, dtype=np.float32)


def _call(wx, fam, dim, sides, trees, batch, k=K):
    lib = ctypes.CDLL(wx.LIB_PATH)
    fn = getattr(lib, "wx_%s%s_trees_f32" % (fam, dim))
    fn.restype = ci
    src, dst = _buffers(dim, batch)
    args = [vp(src.ctypes.data), vp(dst.ctypes.data)] + [i64(s) for s in sides]
    if fam in ("iwpd", "getbasiscoef"):
        args.append(ci(k))
    args += [vp(trees.ctypes.data), i64(trees.shape[0]), i64(batch)]
    if fam != "getbasiscoef":
        q = np.ascontiguousarray(wx.wavelet(wx.WT.db4).qmf, dtype=np.float64)
        args += [vp(q.ctypes.data), ci(q.size)]
    rc = fn(*args, vp(0))
    lib.wx_last_error.restype = ctypes.c_char_p
    return rc, (lib.wx_last_error() or b"").decode()


def _matrix(ntree, batch, special):
    """valid trees of depth <= 1 that are not all equal, and `special`: column -> nodes"""
    t = np.zeros((ntree, batch), dtype=np.uint8, order="F")
    t[0, 1::2] = 1
    for col, nodes in special.items():
        t[:, col] = 0
        t[[i - 1 for i in nodes], col] = 1
    return t


def _passed(wx):
    return OK if ctypes.CDLL(wx.LIB_PATH).wx_device_count() >= 1 else EHIP


@pytest.mark.parametrize("large", [True, False], ids=["threads", "one_thread"])
@pytest.mark.parametrize("dim", ["1d", "2d"])
def test_first_offending_column_decides(wx, dim, large):
    sides, ntree, big, small = SHAPES[dim]
    batch = big if large else small
    assert (batch * ntree >= 2 ** 22) == large
    last = batch - 1 - (batch // 16 if large else 0)                   # a column of the last eighth
    assert last >= batch * 7 // 8 + 1
    out = _buffers(dim, batch)[1]
    deep_first = _matrix(ntree, batch, {1: DEEP[dim], last: ORPHAN[dim]})
    orphan_first = _matrix(ntree, batch, {1: ORPHAN[dim], last: DEEP[dim]})
    for fam in ("iwpd", "getbasiscoef"):
        rc, msg = _call(wx, fam, dim, sides, deep_first, batch)
        assert rc == EARG and "Not enough decomposition levels" in msg, (fam, rc, msg)
        rc, msg = _call(wx, fam, dim, sides, orphan_first, batch)
        assert rc == EASSERT and "isvalidtree" in msg, (fam, rc, msg)
    # no k: an orphan in the last eighth alone, and behind a deep tree, which is a tree like any other here
    for fam in ("wpt", "iwpt"):
        for trees in (_matrix(ntree, batch, {last: ORPHAN[dim]}), deep_first):
            rc, msg = _call(wx, fam, dim, sides, trees, batch)
            assert rc == EASSERT and "isvalidtree" in msg, (fam, rc, msg)
    assert (out == 1).all()                                           # nothing was written by any of them
    valid = _matrix(ntree, batch, {})
    for fam in FAMS:
        assert _call(wx, fam, dim, sides, valid, batch)[0] == _passed(wx), fam
