"""Test helpers for the shift-invariant packet table, written from the layout in include/waveletsext_hip.h
("Shift-invariant wavelet packet decomposition") and not from the package's own index functions: depth j owns the
2^min(j,d) columns that start at sum_{i<j} 2^min(i,d); column `slot` of depth j is TransformShift slot << max(0, j-d);
the cost / status entry of node (j, i, t) is sum_{i'<j} 2^i' 2^min(i',d) + (slot << j) + i.  Trees are lists of
(Depth, IndexAtDepth, TransformShift) keys of an oracle object (oracle.siwpd)."""
import numpy as np

MODES = ("ns", "ss", "alt", "rand")


def ncols(L, d):
    """number of table columns, closed form of sum_{j<=L} 2^min(j,d)"""
    return (1 << (d + 1)) - 1 + (L - d) * (1 << d)


def coloff(j, d):
    """first column of depth j"""
    return (1 << j) - 1 if j <= d else (1 << d) - 1 + (j - d) * (1 << d)


def nodeoff(j, d):
    """first cost / status entry of depth j: sum_{i<j} 2^i 2^min(i,d)"""
    if j <= d:
        return ((1 << (2 * j)) - 1) // 3
    return ((1 << (2 * d)) - 1) // 3 + (1 << d) * ((1 << j) - (1 << d))


def nnodes(L, d):
    return nodeoff(L + 1, d)


def _slot(j, t, d):
    m = max(0, j - d)
    if not 0 <= t < (1 << j) or t & ((1 << m) - 1):
        return None
    return t >> m


def node_index(j, i, t, L, d):
    """index of node (j, i, t) in the costs / status arrays; None if that shift does not exist at that depth"""
    if not (0 <= j <= L and 0 <= i < (1 << j)):
        return None
    s = _slot(j, t, d)
    return None if s is None else nodeoff(j, d) + (s << j) + i


def column_of(j, t, L, d):
    """table column of depth j, shift t"""
    s = _slot(j, t, d) if 0 <= j <= L else None
    return None if s is None else coloff(j, d) + s


def all_keys(L, d):
    """every (j, i, t) that has an index, in index order"""
    out = []
    for j in range(L + 1):
        m = max(0, j - d)
        for s in range(1 << min(j, d)):
            out.extend((j, i, s << m) for i in range(1 << j))
    return out


def _children(key):
    j, i, t = key
    ns = ((j + 1, 2 * i, t), (j + 1, 2 * i + 1, t))
    ss = ((j + 1, 2 * i, t + (1 << j)), (j + 1, 2 * i + 1, t + (1 << j)))
    return ns, ss


def status_from_tree(keys, L, d):
    """(NN,) uint8: 0 absent, 1 leaf, 2 kept with its non-shifted children, 3 kept with its shifted children"""
    keys = set(keys)
    st = np.zeros(nnodes(L, d), dtype=np.uint8)
    for key in keys:
        ns, ss = _children(key)
        has_ns, has_ss = ns[0] in keys and ns[1] in keys, ss[0] in keys and ss[1] in keys
        assert not (has_ns and has_ss), key
        st[node_index(*key, L, d)] = 3 if has_ss else 2 if has_ns else 1
    return st


def random_tree(ref, rng, mode):
    """keys of a valid tree inside the oracle object `ref` (all of whose nodes must still be there).
    "ns": non-shifted children everywhere, to full depth; "ss": shifted children wherever the shifted pair exists;
    "alt": non-shifted at even depths, shifted at odd ones; "rand": a leaf with probability 0.2 (never the root),
    otherwise either pair with equal probability."""
    assert mode in MODES
    nodes = ref.Nodes
    out = []

    def walk(key):
        out.append(key)
        ns, ss = _children(key)
        has_ns, has_ss = ns[0] in nodes, ss[0] in nodes
        if not has_ns and not has_ss:
            return
        if mode == "rand":
            if key[0] > 0 and rng.random() < 0.2:
                return
            shifted = bool(rng.integers(2))
        else:
            shifted = mode == "ss" or (mode == "alt" and key[0] % 2 == 1)
        pair = ss if (shifted and has_ss) or not has_ns else ns
        walk(pair[0]); walk(pair[1])

    walk((0, 0, 0))
    return out


def prune(ref, keys):
    """delete every node of `ref` that is not in `keys` (oracle.siwt_delete_node); returns ref"""
    import wx_oracle                                              # tests/conftest.py puts oracle/ on the path
    keys = set(keys)
    # siwt_delete_node filters the whole BestTree list once per deleted node: set the list aside, filter it once
    order, ref.BestTree = ref.BestTree, []
    for key in sorted(ref.Nodes):                                 # parents first: one call removes a whole subtree
        if key not in keys and key in ref.Nodes:
            wx_oracle.siwt_delete_node(ref, key)
    ref.BestTree = [k for k in order if k in ref.Nodes]
    assert set(ref.Nodes) == keys == set(ref.BestTree)
    return ref
