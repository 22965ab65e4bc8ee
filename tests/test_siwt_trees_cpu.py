"""CPU checks of tests/siwt_trees.py, the index and tree helpers that tests/test_gpu_siwt_routes.py relies on: the
helper's (depth, index, shift) -> table position map against the node set the oracle's recursion creates and
against the library's own wx_siwt_ncols / wx_siwt_nnodes, and its trees against the oracle's validity check and
inverse."""
import copy

import numpy as np
import pytest

import siwt_trees as st

LD = [(L, d) for L in range(1, 9) for d in range(1, L + 1)]


@pytest.mark.parametrize("L,d", LD)
def test_index_map_is_the_oracles_node_set(wx, oracle, L, d):
    x = np.random.default_rng(L * 9 + d).standard_normal(1 << L)
    ref = oracle.siwpd(x, wx.wavelet(wx.WT.haar).qmf, L, d)
    keys = [(j, i, t) for j in range(L + 1) for i in range(1 << j) for t in range(1 << j)
            if st.node_index(j, i, t, L, d) is not None]
    assert set(keys) == set(ref.Nodes)
    idx = sorted(st.node_index(*k, L, d) for k in keys)
    assert idx == list(range(st.nnodes(L, d)))                       # a bijection onto range(NN)
    assert st.all_keys(L, d) == sorted(keys, key=lambda k: st.node_index(*k, L, d))
    # the columns: one per (depth, shift), in depth order, and a node's shift exists exactly when its column does
    cols = sorted({st.column_of(j, t, L, d) for (j, _, t) in keys})
    assert cols == list(range(st.ncols(L, d)))
    for j in range(L + 1):
        for t in range(1 << j):
            assert (st.column_of(j, t, L, d) is None) == (st.node_index(j, 0, t, L, d) is None)
    assert st.node_index(L + 1, 0, 0, L, d) is None and st.node_index(1, 2, 0, L, d) is None
    assert st.node_index(1, 0, 2, L, d) is None and st.column_of(L + 1, 0, L, d) is None


def test_sizes_agree_with_the_library(wx):
    lib = wx._lib.lib()
    for L in range(13):
        for d in range(L + 1):
            assert st.ncols(L, d) == sum(1 << min(j, d) for j in range(L + 1)) == lib.wx_siwt_ncols(L, d)
            assert st.nnodes(L, d) == sum((1 << j) << min(j, d) for j in range(L + 1)) == lib.wx_siwt_nnodes(L, d)
            for j in range(L + 2):
                assert st.coloff(j, d) == sum(1 << min(i, d) for i in range(j))
                assert st.nodeoff(j, d) == sum((1 << i) << min(i, d) for i in range(j))
    for L, d in ((3, 4), (0, 1), (-1, 0), (-1, -1), (31, 2), (31, 31), (30, 31), (4, -1)):
        assert lib.wx_siwt_ncols(L, d) == -1 and lib.wx_siwt_nnodes(L, d) == -1, (L, d)
    assert lib.wx_siwt_ncols(30, 30) == (1 << 31) - 1 and lib.wx_siwt_nnodes(30, 0) == (1 << 31) - 1


@pytest.mark.parametrize("wname", ["haar", "db2"])
@pytest.mark.parametrize("n,L,d", [(64, 6, 6), (48, 4, 2), (256, 5, 3), (1024, 4, 3)])
def test_trees_are_valid_and_invert(wx, oracle, wname, n, L, d):
    rng = np.random.default_rng(n + 7 * L + d)
    x = rng.standard_normal(n)
    full = oracle.siwpd(x, wx.wavelet(getattr(wx.WT, wname)).qmf, L, d)
    seen = set()
    for mode in st.MODES:
        keys = st.random_tree(full, rng, mode)
        assert len(keys) == len(set(keys)) and keys[0] == (0, 0, 0)
        seen.add(frozenset(keys))
        ref = st.prune(copy.deepcopy(full), keys)
        assert oracle.siwt_isvalidtree(ref)
        status = st.status_from_tree(keys, L, d)
        assert int((status != 0).sum()) == len(keys)
        if mode == "ns":
            assert all(t == 0 for (_, _, t) in keys) and len(keys) == (2 << L) - 1
            assert set(status[status != 0]) == {1, 2}
        if mode == "ss":                                             # a shifted node is decomposed d - depth times more
            assert len(keys) == (2 << d) - 1 and set(status[status != 0]) == {1, 3}
        if mode == "alt":
            assert set(status[status != 0]) == {1, 2, 3}
        assert float(np.abs(oracle.isiwpd(ref) - x).max()) <= 1e-12
        assert list(ref.Nodes) == [(0, 0, 0)]
    assert len(seen) == len(st.MODES)                                # four different trees
    assert set(full.Nodes) == set(st.all_keys(L, d))                 # random_tree / prune left the full object alone
