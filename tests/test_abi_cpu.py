"""CPU-side checks of the boundary: the C-ABI library loads, exports every symbol that
include/waveletsext_hip.h declares, rejects bad arguments with the reference's error classes
before touching a device, and fails loudly (no CPU fallback) when no HIP device exists."""
import ctypes
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _declared_symbols():
    txt = open(os.path.join(ROOT, "include", "waveletsext_hip.h")).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    return sorted(set(re.findall(r"\b(wx_[a-z0-9_]+)\s*\(", txt)))


def test_library_exports_every_declared_symbol(wx):
    lib = ctypes.CDLL(wx.LIB_PATH)
    syms = _declared_symbols()
    assert len(syms) >= 10
    for s in syms:
        assert hasattr(lib, s), "declared in include/waveletsext_hip.h but not exported: " + s
    assert lib.wx_version() >= 100


def test_argument_errors_mirror_the_reference(wx):
    wt = wx.wavelet(wx.WT.db4)
    x = np.zeros((8, 3))
    with pytest.raises(AssertionError):
        wx.wpdall(x, wt, 4)                                   # dwt_all.jl:266
    with pytest.raises(AssertionError):
        wx.wpdall(np.zeros(8), wt)                            # dwt_all.jl:265 ndims > 1
    with pytest.raises(AssertionError):
        wx.wpd(np.zeros(12), wt)                              # DWT.jl:64
    with pytest.raises(AssertionError):
        wx.wptall(x, wt, np.array([0, 1, 0, 0, 0, 0, 0], dtype=bool))   # invalid tree
    with pytest.raises(AssertionError):
        wx.wptall(x, wt, np.ones(4, dtype=bool))              # wrong tree length
    with pytest.raises(AssertionError):
        wx.iwpdall(np.zeros((8, 5, 2)), wt)                   # k-1 <= maxtransformlevels (Utils.jl:110)
    with pytest.raises(wx.ArgumentError):
        wx.iwpdall(np.zeros((8, 2, 2)), wt, 3)                # not enough levels (Utils.jl:120)
    with pytest.raises(AssertionError):
        wx.iwpd_(np.zeros(4), np.zeros((8, 4)), wt)           # DWT.jl:344 size mismatch
    with pytest.raises(wx.ArgumentError):
        wx.OrthoFilter([1.0, 2.0, 3.0])                       # odd-length filter


def test_no_cpu_fallback_without_gpu(wx):
    if wx.device_count() > 0:
        pytest.skip("a HIP device is present")
    with pytest.raises(wx.WxError) as ei:
        wx.wpdall(np.zeros((8, 2)), wx.wavelet(wx.WT.haar))
    assert ei.value.code == -10
    # every family fails the same way: there is no host implementation behind the API
    wt = wx.wavelet(wx.WT.haar)
    X3 = np.zeros((8, 4, 2))
    calls = [
        lambda: wx.wptall(np.zeros((8, 2)), wt), lambda: wx.iwptall(np.zeros((8, 2)), wt),
        lambda: wx.swptall(np.zeros((8, 2)), wt, 2), lambda: wx.iswptall(np.zeros((8, 4, 2)), wt),
        lambda: wx.acwpdall(np.zeros((8, 2)), wt, 2), lambda: wx.wptall(np.zeros((8, 8, 2)), wt, 1),
        lambda: wx.bestbasistree(X3, wx.JBB()), lambda: wx.bestbasistreeall(X3, wx.BB()),
        lambda: wx.denoiseall(np.zeros((8, 2)), "sig", wt), lambda: wx.noisest(np.zeros(8), False),
        lambda: wx.energy_map(X3, [0, 1]), lambda: wx.acwpd_jbb_moments(np.zeros((8, 2)), wt),
        lambda: wx.siwpd(np.ones(8), wt), lambda: wx.siwpdall(np.ones((8, 2)), wt, 2, 1),
        lambda: wx.ShiftInvariantWaveletTransformObject(np.ones(8), wt),
    ]
    for c in calls:
        with pytest.raises(wx.WxError) as ei:
            c()
        assert ei.value.code == -10


def test_treeselect_host_routine_matches_oracle(wx, oracle):
    """wx_treeselect_* is pure host code (BestBasis.jl:59-83): bit-exact vs the oracle on CPU."""
    rng = np.random.default_rng(4)
    for n in (4, 16, 64):
        for k in ((2 * n - 1), n - 1, 3):
            for kind in ("min", "max"):
                costs = rng.standard_normal(k) ** 2
                assert (wx.bestbasis_treeselection(costs, n, kind) == oracle.bestbasis_treeselection(costs, n, kind)).all()
        ties = np.ones(2 * n - 1)
        ties[1:] = 0.5                      # children sum == parent at the root: strict < keeps the parent
        assert not wx.bestbasis_treeselection(ties, n)[0]
    with pytest.raises(wx.ArgumentError):
        wx.bestbasis_treeselection(rng.standard_normal(15), 8, "fail")          # test/bestbasis.jl:43
    with pytest.raises(AssertionError):
        wx.bestbasis_treeselection(rng.standard_normal(7), 3)                   # test/bestbasis.jl:44
    for k in (5, 6, 2):                                                         # not 2^(L+1)-1: the children of depth
        with pytest.raises(IndexError):                                         # L-1 would be read past the vector
            wx.bestbasis_treeselection(rng.standard_normal(k), 16)
    with pytest.raises(IndexError):
        wx.bestbasis_treeselection(rng.standard_normal(7), 4, 4)                # quad tree: 5 costs of depth 1 needed


def test_treeselect_gap_host_routine(wx, oracle):
    """wx_treeselect_gap_*: the same tree as wx_treeselect_* / the oracle, and the margin of the closest decision TAKEN
    (nodes pruned with an ancestor's subtree before their turn do not count), against a restatement of BestBasis.jl:59-83."""
    rng = np.random.default_rng(44)
    for n in (4, 16, 64, 256):
        for kind in ("min", "max"):
            for dt in (np.float64, np.float32):
                costs = (rng.standard_normal(2 * n - 1) ** 2).astype(dt)
                tree, gap = wx.bestbasis_treeselection(costs, n, kind, return_gap=True)
                assert (tree == oracle.bestbasis_treeselection(costs, n, kind)).all()
                c = costs.astype(dt).copy()
                alive = np.zeros(n - 1, dtype=bool)
                alive[:n - 1] = True
                ref = np.inf
                for i in range(n - 1, 0, -1):
                    if not alive[i - 1]:
                        continue
                    pc, cc = c[i - 1], dt(c[2 * i - 1] + c[2 * i])
                    ref = min(ref, abs(float(cc) - float(pc)) / abs(float(pc)))
                    if (cc < pc) if kind == "min" else (cc > pc):
                        c[i - 1] = cc
                    else:
                        stack = [i]
                        while stack:
                            j = stack.pop()
                            if j <= n - 1 and alive[j - 1]:
                                alive[j - 1] = False
                                stack += [2 * j, 2 * j + 1]
                assert (alive == tree).all()
                assert gap == pytest.approx(ref, rel=1e-12)
    ties = np.ones(7)
    ties[1:] = 0.5
    assert wx.bestbasis_treeselection(ties, 4, return_gap=True)[1] == 0.0       # an exact tie is margin 0
    assert wx.bestbasis_treeselection(np.ones(1), 4, return_gap=True)[1] == np.inf   # L = 0: no decision


def test_acwpd_jbb_moments_is_float64_only(wx):
    """ACWT is Float64-only like the reference (acwt_one_level.jl:101-106): Float32 data must be refused, never
    reinterpreted (there is no wx_acwpd_jbb_moments_f32)"""
    wt = wx.wavelet(wx.WT.db4)
    with pytest.raises(wx.WxError) as ei:
        wx.acwpd_jbb_moments(np.zeros((16, 4), dtype=np.float32), wt, 2)
    assert ei.value.code == -11
    with pytest.raises(TypeError):
        wx.acwpd_jbb_moments(np.zeros((16, 4)), wt, 2, accumulate_into=(np.zeros((16, 7), dtype=np.float32),
                                                                         np.zeros((16, 7), dtype=np.float32)))


def test_redundant_argument_errors(wx):
    wt = wx.wavelet(wx.WT.db4)
    with pytest.raises(wx.ArgumentError):
        wx.swpt(np.zeros(8), wt, 4)                                             # SWT.jl:64
    with pytest.raises(wx.ArgumentError):
        wx.acwpd(np.zeros(8), wt, 0)                                            # L >= 1
    with pytest.raises(wx.ArgumentError):
        wx.iswpt(np.zeros((8, 3)), wt)                                          # columns not dyadic
    with pytest.raises(AssertionError):
        wx.iswpd(np.zeros((8, 15)), wt, np.array([0, 1, 0, 0, 0, 0, 0], dtype=bool))
    p, q = wx.make_acreverseqmfpair(wx.wavelet(wx.WT.haar))
    np.testing.assert_allclose(p, [0.35355339, 0.70710678, 0.35355339], atol=1e-8)
    np.testing.assert_allclose(q, [-0.35355339, 0.70710678, -0.35355339], atol=1e-8)


def test_redundant2d_argument_errors(wx):
    """the 2-D redundant entry points refuse bad arguments with the reference's error classes before any device is
    touched (so this runs without one): through the Python layer, and at the C ABI itself"""
    import ctypes
    wt = wx.wavelet(wx.WT.db4)
    img = np.zeros((8, 16))
    for fwd in (wx.sdwt, wx.swpt, wx.swpd, wx.acdwt, wx.acwpt, wx.acwpd):
        with pytest.raises(wx.ArgumentError):
            fwd(img, wt, 0)                                                     # L >= 1
        with pytest.raises(wx.ArgumentError):
            fwd(img, wt, 4)                                                     # SWT.jl:137-139, ACWT.jl:135-137: 8 rows
    L = 2
    for sm in (0, 1 << L):
        with pytest.raises(AssertionError):
            wx.isdwt(np.zeros((8, 16, 3 * L + 1)), wt, sm)                      # SWT.jl:293, Utils.jl:298
    with pytest.raises(AssertionError):
        wx.iswpt(np.zeros((8, 16, 16)), wt, 1 << L)                             # main2depthshift: sm < 1 << L
    with pytest.raises(AssertionError):
        wx.iswpt(np.zeros((8, 16, 256)), wt)                                    # SWT.jl:656: 4 levels of 8 rows
    for inv in (wx.iswpt, wx.iacwpt):
        with pytest.raises(wx.ArgumentError):
            inv(np.zeros((8, 16, 8)), wt)                                       # SWT.jl:653, ACWT.jl:617: not a power of 4
    bad = np.zeros(21, dtype=bool)
    bad[1] = True                                                               # a child without its parent
    for inv in (wx.iswpd, wx.iacwpd):
        with pytest.raises(AssertionError):
            inv(np.zeros((8, 16, 21)), wt, bad)                                 # SWT.jl:1101, ACWT.jl:973
        with pytest.raises(AssertionError):
            inv(np.zeros((8, 16, 21)), wt, np.ones(5, dtype=bool))              # wrong tree length
        with pytest.raises(IndexError):
            inv(np.zeros((8, 16, 5)), wt, wx.maketree(8, 16, 2, "full"))        # the tree reaches below the last slice
    with pytest.raises(AssertionError):
        wx.iswpd(np.zeros((8, 16, 21)), wt, None, 4)                            # sm < 1 << (depth of the table)
    # the C ABI makes the same checks itself (status codes of include/waveletsext_hip.h), whatever the binding does
    lib = ctypes.CDLL(wx.LIB_PATH)
    q = np.ascontiguousarray(wt.qmf, dtype=np.float64)
    qp, F = q.ctypes.data_as(ctypes.c_void_p), ctypes.c_int(q.size)
    buf = np.zeros(8 * 16 * 21)
    p = buf.ctypes.data_as(ctypes.c_void_p)
    i64, ci = ctypes.c_int64, ctypes.c_int
    EASSERT, EARG, EBOUNDS = -1, -2, -3
    for name in ("wx_sdwt2d_f64", "wx_swpt2d_f64", "wx_swpd2d_f64", "wx_acdwt2d_f64", "wx_acwpt2d_f64", "wx_acwpd2d_f64"):
        assert getattr(lib, name)(p, p, i64(8), i64(16), ci(0), i64(1), qp, F, None) == EARG, name
        assert getattr(lib, name)(p, p, i64(8), i64(16), ci(4), i64(1), qp, F, None) == EARG, name
    for sm in (0, 4):
        assert lib.wx_isdwt2d_f64(p, p, i64(8), i64(16), ci(2), i64(sm), i64(1), qp, F, None) == EASSERT
    assert lib.wx_iswpt2d_f64(p, p, i64(8), i64(16), ci(2), i64(4), i64(1), qp, F, None) == EASSERT
    assert lib.wx_iswpt2d_f64(p, p, i64(8), i64(16), ci(4), i64(-1), i64(1), qp, F, None) == EASSERT
    t8 = np.ascontiguousarray(bad, dtype=np.uint8)
    tp = t8.ctypes.data_as(ctypes.c_void_p)
    assert lib.wx_iswpd2d_f64(p, p, i64(8), i64(16), i64(21), ci(0), tp, i64(21), i64(-1), i64(1), qp, F, None) == EASSERT
    assert lib.wx_iacwpd2d_f64(p, p, i64(8), i64(16), i64(21), ci(0), tp, i64(21), i64(1), None) == EASSERT
    full2 = np.zeros(21, dtype=np.uint8)
    full2[:5] = 1
    fp = full2.ctypes.data_as(ctypes.c_void_p)
    assert lib.wx_iswpd2d_f64(p, p, i64(8), i64(16), i64(5), ci(0), fp, i64(21), i64(-1), i64(1), qp, F, None) == EBOUNDS
    assert lib.wx_iacwpd2d_f64(p, p, i64(8), i64(16), i64(5), ci(0), fp, i64(21), i64(1), None) == EBOUNDS


def test_swt1d_debug_entry_points_refuse_bad_arguments(wx):
    """csrc/wx_debug.h: the launch record and the schedule query of the 1-D redundant transforms, at the C level (no device)"""
    lib = ctypes.CDLL(wx.LIB_PATH)
    EARG = -2
    i64, ci = ctypes.c_int64, ctypes.c_int
    lib.wx_debug_swt1d_trace_dropped.restype = i64
    row = (ctypes.c_int32 * 11)()
    assert lib.wx_debug_swt1d_trace_end(row, ci(1)) == EARG                     # end without begin
    lib.wx_debug_swt1d_trace_begin()
    assert lib.wx_debug_swt1d_trace_end(row, ci(0)) == EARG                     # cap = 0: refused, the record stays armed
    assert lib.wx_debug_swt1d_trace_end(None, ci(4)) == EARG
    assert lib.wx_debug_swt1d_trace_end(row, ci(1)) == 0                        # nothing was launched
    assert lib.wx_debug_swt1d_trace_dropped() == 0
    assert lib.wx_debug_swt1d_trace_end(row, ci(1)) == EARG                     # that end disarmed it
    with wx.swt1d_trace() as tr:
        pass
    assert list(tr) == [] and tr.dropped == 0
    assert set(wx.SWT1D_ROUTES) == set(range(1, 20)) and len(set(wx.SWT1D_ROUTES.values())) == 19
    out = (ctypes.c_int32 * (4 * 24))()
    plan = lambda layout, L, F, sm, n, es: lib.wx_debug_swt_inv_plan(ci(layout), ci(L), ci(F), i64(sm), i64(n), ci(es), ci(0), ci(0), out)
    assert plan(1, 3, 8, -1, 0, 8) == EARG                                      # n = 0
    assert plan(1, 7, 8, -1, 64, 8) == EARG                                     # wpt: more levels than the length admits
    assert plan(1, 3, 8, -1, 64, 2) == EARG                                     # no such element type
    assert plan(3, 3, 8, -1, 64, 8) == EARG and plan(1, -1, 8, -1, 64, 8) == EARG and plan(1, 25, 8, -1, 1 << 26, 8) == EARG
    assert lib.wx_debug_swt_inv_plan(ci(1), ci(3), ci(8), i64(-1), i64(64), ci(8), ci(0), ci(0), None) == EARG
    assert plan(0, 3, 8, -1, 64, 8) == 3 and list(out[:12]) == [3, 2, 0, 1, 2, 1, 0, 1, 1, 0, 0, 1]
    assert plan(1, 0, 8, -1, 64, 8) == 0
    with pytest.raises(wx.ArgumentError):
        wx.swt_inv_plan("wpt", 3, 8, 0, 8)


def test_dwt2d_debug_entry_points_refuse_bad_arguments(wx):
    """csrc/wx_debug.h: the launch record of the 2-D decimated transforms, at the C level (no device): the protocol of the 1-D record"""
    lib = ctypes.CDLL(wx.LIB_PATH)
    EARG = -2
    i64, ci = ctypes.c_int64, ctypes.c_int
    lib.wx_debug_dwt2d_trace_dropped.restype = i64
    row = (ctypes.c_int32 * 16)()
    assert lib.wx_debug_dwt2d_trace_end(row, ci(1)) == EARG                     # end without begin
    lib.wx_debug_dwt2d_trace_begin()
    assert lib.wx_debug_dwt2d_trace_end(row, ci(0)) == EARG                     # cap = 0: refused, the record stays armed
    assert lib.wx_debug_dwt2d_trace_end(row, ci(-1)) == EARG
    assert lib.wx_debug_dwt2d_trace_end(None, ci(4)) == EARG                    # NULL output pointer: refused, still armed
    assert lib.wx_debug_dwt2d_trace_end(row, ci(1)) == 0                        # an empty record: nothing was launched
    assert lib.wx_debug_dwt2d_trace_dropped() == 0
    assert lib.wx_debug_dwt2d_trace_end(row, ci(1)) == EARG                     # that end disarmed it
    with wx.dwt2d_trace() as tr:
        pass
    assert list(tr) == [] and tr.dropped == 0
    with wx.dwt2d_trace() as tr, wx.swt1d_trace() as tr1:                       # the two records are independent
        pass
    assert list(tr) == [] and list(tr1) == []
    assert set(wx.DWT2D_ROUTES) == set(range(1, 19)) and len(set(wx.DWT2D_ROUTES.values())) == 18
    assert len(wx.Dwt2dLaunch._fields) == 16                                    # WX_DWT2D_TRACE_FIELDS


def test_dwt1d_debug_entry_points_refuse_bad_arguments(wx):
    """csrc/wx_debug.h: the launch record of the 1-D decimated transforms, at the C level (no device): the protocol of the other records"""
    lib = ctypes.CDLL(wx.LIB_PATH)
    EARG = -2
    i64, ci = ctypes.c_int64, ctypes.c_int
    lib.wx_debug_dwt1d_trace_dropped.restype = i64
    row = (ctypes.c_int32 * 16)()
    assert lib.wx_debug_dwt1d_trace_end(row, ci(1)) == EARG                     # end without begin
    lib.wx_debug_dwt1d_trace_begin()
    assert lib.wx_debug_dwt1d_trace_end(row, ci(0)) == EARG                     # cap = 0: refused, the record stays armed
    assert lib.wx_debug_dwt1d_trace_end(row, ci(-1)) == EARG
    assert lib.wx_debug_dwt1d_trace_end(None, ci(4)) == EARG                    # NULL output pointer: refused, still armed
    assert lib.wx_debug_dwt1d_trace_end(row, ci(1)) == 0                        # an empty record: nothing was launched
    assert lib.wx_debug_dwt1d_trace_dropped() == 0
    assert lib.wx_debug_dwt1d_trace_end(row, ci(1)) == EARG                     # that end disarmed it
    with wx.dwt1d_trace() as tr:
        pass
    assert list(tr) == [] and tr.dropped == 0
    with wx.dwt1d_trace() as tr, wx.dwt2d_trace() as tr2, wx.swt1d_trace() as tr1:   # the three records are independent
        pass
    assert list(tr) == [] and list(tr2) == [] and list(tr1) == []
    assert set(wx.DWT1D_ROUTES) == set(range(1, 19)) and len(set(wx.DWT1D_ROUTES.values())) == 18
    assert len(wx.Dwt1dLaunch._fields) == 16                                    # WX_DWT1D_TRACE_FIELDS


def test_header_compiles_as_c_and_example_links(tmp_path, wx):
    """include/waveletsext_hip.h is a C header: examples/roundtrip.c builds with gcc -std=c99 against the .so
    (and, without a GPU, fails loudly with the library's status instead of computing on the CPU)"""
    import os
    import subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    lib = os.path.join(root, "waveletsext.jl_amd", "csrc")
    exe = str(tmp_path / "roundtrip")
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-I" + os.path.join(root, "include"),
                    os.path.join(root, "examples", "roundtrip.c"), "-o", exe, "-L" + lib, "-lwaveletsext_hip", "-lm",
                    "-Wl,-rpath," + lib], check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    import waveletsext_jl_amd as wx
    if wx.device_count() == 0:
        assert r.returncode == 1 and "no HIP device" in r.stderr
    else:
        assert r.returncode == 0, r.stderr
