"""Without a device: the chunk count of the LDB class reductions (csrc/wx_ldb.hip, through wx_debug_ldb_chunks, which runs the
function the launch code calls), and the yardstick of tests/test_gpu_ldb_chunks.py -- that tests/ldb_ref.py agrees with the oracle's
restatement of the reference, and that the comparison the GPU test makes would notice one signal lost, doubled or misplaced at a
chunk seam."""
import ctypes

import numpy as np
import pytest

import ldb_ref


def test_chunk_count_table(wx):
    for name, c in ldb_ref.CASES.items():
        nk = int(np.prod(c.shape[:-1]))
        assert wx.ldb_chunks(nk, c.shape[-1], len(c.sizes)) == c.nchunks, name
        assert sum(c.sizes) == c.shape[-1], name
    assert wx.ldb_chunks(4, ldb_ref.E_SHAPE[-1], ldb_ref.E_NC) == ldb_ref.E_NCHUNKS == 65535 // 100
    # a shard of 96 / 96 / 0 signals is reduced in one chunk (the average class, ceil(192 / 3) = 64, decides); 97 / 97 / 0 in two
    assert wx.ldb_chunks(448, 192, 3) == 1 and wx.ldb_chunks(448, 194, 3) == 2
    assert wx.ldb_chunks(448, 210, 3) == 2 and wx.ldb_chunks(64, 210, 3) == 2       # the end-to-end fit: energy map, Fisher's power
    assert wx.ldb_chunks(448, 27, 3) == 1                                       # tests/test_gpu_ldb.py
    assert wx.ldb_chunks(192, 600, 100) == 1                                    # test_gpu_limits.py::test_more_than_64_classes
    assert wx.ldb_chunks(53248, 4096, 4) == 10                                  # limited by the workgroups wanted, not by the class
    assert wx.ldb_chunks(4, 4194304, 64) == 1023                                # 1024 chunks, then 65535 / 64
    assert wx.ldb_chunks(4, 4161000, 1000) == 65                                # 66 chunks, then 65535 / 1000
    assert wx.ldb_chunks(1, 1, 2) == 1 and wx.ldb_chunks(1, (1 << 31) - 1, 65535) == 1


def test_chunk_count_refuses_bad_arguments(wx):
    lib = ctypes.CDLL(wx.LIB_PATH)
    i64, ci = ctypes.c_int64, ctypes.c_int
    EARG = -2
    q = lambda nk, N, nc: lib.wx_debug_ldb_chunks(i64(nk), i64(N), ci(nc))
    assert q(0, 600, 3) == EARG and q(-1, 600, 3) == EARG
    assert q(448, 0, 3) == EARG and q(448, 1 << 31, 3) == EARG
    assert q(448, 600, 1) == EARG and q(448, 600, 0) == EARG and q(448, 600, 65536) == EARG
    assert q(448, 600, 3) == 4
    with pytest.raises(wx.ArgumentError):
        wx.ldb_chunks(448, 600, 1)


def _three(X, mem, nroot):
    G, _ = ldb_ref.energy_map(X, mem, nroot)
    E, A = ldb_ref.class_mean(X, mem)
    return G, E, ldb_ref.class_var(X, mem), A


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("name", ["A", "B", "C", "D"])
def test_comparison_sees_one_signal_at_a_seam(name, dtype):
    """the last signal of the first chunk of the largest class (where one signal weighs least) dropped from the reference, counted
    twice, or moved to the next class: each moves every one of the three arrays by more than 100 bounds"""
    c = ldb_ref.CASES[name]
    X, y, nroot = ldb_ref.case(name, dtype)
    mem = ldb_ref.members(y, len(c.sizes))
    assert tuple(len(m) for m in mem) == c.sizes
    big = int(np.argmax(c.sizes))
    other = (big + 1) % len(c.sizes)
    per = -(-c.sizes[big] // c.nchunks)
    j = mem[big][per - 1]
    b = ldb_ref.bound(max(c.sizes), c.nchunks, dtype)
    G, E, V, A = _three(X, mem, nroot)
    swaps = {"dropped": {big: np.delete(mem[big], per - 1)},
             "twice": {big: np.insert(mem[big], per, j)},
             "moved": {big: np.delete(mem[big], per - 1), other: np.sort(np.append(mem[other], j))}}
    for what, change in swaps.items():
        mut = [change.get(k, m) for k, m in enumerate(mem)]
        G1, E1, V1, _ = _three(X, mut, nroot)
        for arr, got, ref, scale in (("energy", G1, G, None), ("mean", E1, E, A), ("var", V1, V, None)):
            e = ldb_ref.err(got, ref, scale)
            print("%s %s %s %s: %.3g bounds" % (name, np.dtype(dtype).name, what, arr, e / b))
            assert e >= 100 * b, (what, arr, e / b)


def test_reference_agrees_with_oracle(oracle):
    """tests/ldb_ref.py against the oracle's loop restatement of energy_map and of Fisher's class separability, case A in Float64;
    the oracle adds a class's 397 signals one after the other in Float64, the chunked kernel at most 100, so the same bound holds
    for it only because rounding errors do not all point the same way (measured: 0.09 of the bound for the map; 0.40 for the
    power, a quotient of sums over the classes of the rounded means and variances)"""
    c = ldb_ref.CASES["A"]
    X, y, nroot = ldb_ref.case("A", np.float64)
    mem = ldb_ref.members(y, len(c.sizes))
    b = ldb_ref.bound(max(c.sizes), c.nchunks, np.float64)
    G, _ = ldb_ref.energy_map(X, mem, nroot)
    e = ldb_ref.err(oracle.ldb_energy_map(X, y), G)
    print("energy map: %.3g bounds" % (e / b))
    assert e <= b
    E, _ = ldb_ref.class_mean(X, mem)
    P = ldb_ref.fisher_power(E, ldb_ref.class_var(X, mem), c.sizes)
    e = ldb_ref.err(oracle.ldb_fisher_power(X, y), P)
    print("Fisher's power: %.3g bounds" % (e / b))
    assert e <= b


def test_error_measure():
    ref = np.array([1.0, 1e-8, 0.0, np.nan, np.inf])
    assert ldb_ref.err(ref.copy(), ref) == 0.0
    assert ldb_ref.err(np.array([1.0, 1.01e-8, 0.0, np.nan, np.inf]), ref) == pytest.approx(0.01)     # helpers.relerr: 1e-10
    assert ldb_ref.err(np.array([1.0, 1e-8, 1e-300, np.nan, np.inf]), ref) == np.inf
    assert ldb_ref.err(np.array([1.0, 1e-8, 0.0, 1.0, np.inf]), ref) == np.inf
    assert ldb_ref.err(np.array([1.0, 1e-8, 0.0, np.nan, -np.inf]), ref) == np.inf
    assert ldb_ref.err(np.array([1.0, np.nan, 0.0, np.nan, np.inf]), ref) == np.inf
    assert ldb_ref.err(np.array([1.5, 1e-8]), np.array([1.0, 1e-8]), scale=np.array([2.0, 1.0])) == 0.25
