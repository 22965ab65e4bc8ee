"""surethresholdall / relerrorthresholdall(xw, True, M) with M an (n - 1, N) matrix -- one tree per signal, every threshold selected over the
leaf columns of its own tree in its redundant packet table (csrc/wx_shrink_trees.hip) -- and what rests on them: denoiseall(xw, "swpd" |
"acwpd", wt, tree=M, estnoise=relerrorthreshold | surethreshold) on a device table, and swpd_denoiseall / acwpd_denoiseall /
bestbasis_denoiseall with the same estimators straight from device signals.

The cases are those of tests/shrink_trees_cases.py, whose fixture guard (tests/test_shrink_trees_cpu.py) shows that no criterion has a
runner-up within 1e-8 of its pick: the Float64 thresholds are the oracle's picks to rel = 1e-13 (the bound of tests/test_gpu_shrink.py above
the LDS window) with no tie clause.  Both element types are bit for bit what the single-tree entry returns for that signal alone -- the
Float32 criterion, since a Float32 pick may differ from the Float64 oracle's (tests/test_gpu_shrink.py::test_threshold_selection_float32).
The tables are the library's own swpdall / acwpdall copied to the host, so the library and the oracle see the same bits; every reference is
computed once per (case, transform) and shared."""
import ctypes
import functools

import numpy as np
import pytest

import helpers
import shrink_trees_cases as cases
from test_gpu_red_trees import _bytes, _dev

pytestmark = pytest.mark.gpu

LDS, SINGLE, HOST = "device prep + lds kernel", "device prep + single tree", "host trees"
P, L64, I = ctypes.c_void_p, ctypes.c_int64, ctypes.c_int
NS = [n for n, _, _ in cases.CASES]
KINDS = ("swpd", "acwpd")
ELBOWS = (1, 2, 3)


@functools.lru_cache(maxsize=None)
def _table(n, kind, dtname):
    """(device table (n, ncols, N), its bits on the host) of a case; neither is ever modified"""
    import waveletsext_jl_amd as wx
    x, trees, D = cases.case(n)
    wt = wx.wavelet(cases.WAVELET)
    xd = wx.to_device(np.asfortranarray(x.astype(dtname)))
    td = wx.swpdall(xd, wt, D) if kind == "swpd" else wx.acwpdall(xd, wt, D)
    th = wx.to_numpy(td)
    assert th.shape == (n, (2 << D) - 1, trees.shape[1]) and th.dtype == np.dtype(dtname)
    th.setflags(write=False)
    return td, th


@functools.lru_cache(maxsize=None)
def _oracle(n, kind):
    """the oracle's thresholds on the Float64 table, signal by signal: {"sure": (N,), 1: (N,), 2: (N,), 3: (N,)}"""
    import wx_oracle
    wx_oracle.build()
    _, trees, _ = cases.case(n)
    _, th = _table(n, kind, "float64")
    N = trees.shape[1]
    want = {"sure": np.array([wx_oracle.surethreshold(th[:, :, i], True, trees[:, i]) for i in range(N)])}
    for e in ELBOWS:
        want[e] = np.array([wx_oracle.relerrorthreshold(th[:, :, i], True, trees[:, i], e) for i in range(N)])
    for v in want.values():
        v.setflags(write=False)
    return want


def _abi(wx, rule, td, trees, elbows=2, host_table=None):
    """the C entry: table and thresholds on the device (or, host_table, both in host memory), `trees` a device tensor or a numpy matrix"""
    import torch
    from waveletsext_jl_amd._arrays import Arg, trees_arg
    xa = Arg(td if host_table is None else host_table)
    n, ncols, N = xa.shape
    tb, tp, nt = trees_arg(trees, N, Arg(td))
    if host_table is None:
        out = torch.full((N,), -7.25, dtype=td.dtype, device=td.device)
        op = P(out.data_ptr())
    else:
        out = np.full(N, -7.25, dtype=xa.dtype)
        op = P(out.ctypes.data)
    fn = getattr(wx._lib.lib(), ("wx_surethreshold_trees" if rule == "sure" else "wx_relerrorthreshold_trees") + xa.suffix)
    head = (xa.ptr, L64(n), L64(ncols), tp, L64(nt), L64(N))
    tail = (op, P(torch.cuda.current_stream().cuda_stream))
    rc = fn(*head, *tail) if rule == "sure" else fn(*head, I(elbows), *tail)
    assert rc == 0, wx._lib.lib().wx_last_error()
    torch.cuda.synchronize()
    return out.cpu().numpy() if host_table is None else out


def _close(got, want, what):
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape and got.dtype == np.float64
    err = np.abs(got - want) / np.abs(want)
    print(what, "largest relative difference", err.max())
    assert (err <= 1e-13).all(), (what, np.flatnonzero(err > 1e-13), got[err > 1e-13], want[err > 1e-13])


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("n", NS)
def test_float64_thresholds_are_the_oracles_picks(wx, oracle, n, kind):
    import torch
    _, trees, _ = cases.case(n)
    td, th = _table(n, kind, "float64")
    want = _oracle(n, kind)
    dtb = _dev(wx, trees)
    _close(_abi(wx, "sure", td, dtb), want["sure"], "C surethreshold")
    assert wx.wpt_trees_route() == LDS
    s = wx.surethresholdall(td, True, dtb)
    assert isinstance(s, torch.Tensor) and s.is_cuda and tuple(s.shape) == (trees.shape[1],)
    _close(wx.to_numpy(s), want["sure"], "surethresholdall")
    for e in ELBOWS:
        _close(_abi(wx, "relerror", td, dtb, e), want[e], "C relerrorthreshold, %d elbows" % e)
        r = wx.relerrorthresholdall(td, True, dtb, e)
        assert isinstance(r, torch.Tensor) and r.is_cuda
        _close(wx.to_numpy(r), want[e], "relerrorthresholdall, %d elbows" % e)
    assert wx.relerrorthresholdall(td, True, dtb).cpu().numpy().tobytes() == wx.relerrorthresholdall(td, True, dtb, 2).cpu().numpy().tobytes()
    # a numpy table gives numpy thresholds
    r = wx.relerrorthresholdall(th, True, np.asarray(trees))
    assert isinstance(r, np.ndarray) and r.dtype == np.float64
    _close(r, want[2], "relerrorthresholdall, numpy table")
    # redundant = False: all coefficients, whatever the tree -- the call of before
    assert wx.surethresholdall(th, False, np.asarray(trees)).tobytes() == wx.surethresholdall(th, False).tobytes()


@pytest.mark.parametrize("dtname,kind", [("float64", "swpd"), ("float64", "acwpd"), ("float32", "swpd")])
@pytest.mark.parametrize("n", NS)
def test_bit_for_bit_the_single_tree_entry_signal_by_signal(wx, n, dtname, kind):
    """the same sorted magnitudes and the same scan: the same bits.  Every result is one of that signal's leaf magnitudes (up to the two
    roundings of the arithmetic that returns it)."""
    _, trees, _ = cases.case(n)
    td, th = _table(n, kind, dtname)
    N = trees.shape[1]
    dtb = _dev(wx, trees)
    s = wx.to_numpy(wx.surethresholdall(td, True, dtb))
    r = wx.to_numpy(wx.relerrorthresholdall(td, True, dtb))
    r3 = wx.to_numpy(wx.relerrorthresholdall(td, True, dtb, 3))
    assert s.dtype == r.dtype == np.dtype(dtname)
    for i in range(N):
        one = td[:, :, i:i + 1]
        assert wx.surethresholdall(one, True, trees[:, i]).tobytes() == s[i:i + 1].tobytes(), ("sure", i)
        assert wx.relerrorthresholdall(one, True, trees[:, i]).tobytes() == r[i:i + 1].tobytes(), ("relerror", i)
        assert wx.relerrorthresholdall(one, True, trees[:, i], 3).tobytes() == r3[i:i + 1].tobytes(), ("relerror 3", i)
        # a pick from the signal's own leaf magnitudes: sqrt(v v) and (v / xmax) xmax round twice, so within two spacings of one of them
        # (or 0, the first point of the curve)
        mags = np.append(np.abs(th[:, cases.leaves_of(trees[:, i]), i]).ravel(), 0).astype(np.float64)
        for t in (s[i], r[i], r3[i]):
            assert np.abs(mags - float(t)).min() <= 2 * np.finfo(dtname).eps * float(t), (i, t)


@pytest.mark.parametrize("dtname", ["float64", "float32"])
def test_the_same_bytes_whatever_the_callers_form(wx, dtname):
    n = 256
    _, trees, _ = cases.case(n)
    td, th = _table(n, "swpd", dtname)
    dtb, dtu = _dev(wx, trees), _dev(wx, trees, np.uint8)
    for rule in ("sure", "relerror"):
        f = (lambda t, m: wx.surethresholdall(t, True, m)) if rule == "sure" else (lambda t, m: wx.relerrorthresholdall(t, True, m))
        g = _bytes(wx, f(td, dtb))
        assert wx.wpt_trees_route() == LDS
        assert _bytes(wx, f(td, dtu)) == g and wx.wpt_trees_route() == LDS
        assert _bytes(wx, f(td, dtb)) == g                             # a repeated call
        assert _bytes(wx, f(td, np.asarray(trees))) == g and wx.wpt_trees_route() == HOST
        assert _abi(wx, rule, td, dtb).tobytes() == g and wx.wpt_trees_route() == LDS
        assert _abi(wx, rule, td, np.asarray(trees), host_table=th).tobytes() == g and wx.wpt_trees_route() == HOST
        assert f(th, np.asarray(trees)).tobytes() == g
    assert _bytes(wx, td) == th.tobytes(), "the input table was modified"


@pytest.mark.parametrize("kind", KINDS)
def test_identical_columns_take_the_single_tree_entry(wx, oracle, kind):
    n = 256
    _, trees, _ = cases.case(n)
    td, th = _table(n, kind, "float64")
    N = trees.shape[1]
    for col in (1, 4):                                                 # 33 leaves: outside the LDS window; the bare root
        M = np.asfortranarray(np.repeat(np.asarray(trees[:, col])[:, None], N, axis=1))
        want_s = np.array([oracle.surethreshold(th[:, :, i], True, M[:, i]) for i in range(N)])
        want_r = np.array([oracle.relerrorthreshold(th[:, :, i], True, M[:, i]) for i in range(N)])
        _close(wx.to_numpy(wx.surethresholdall(td, True, _dev(wx, M))), want_s, "identical columns, sure")
        assert wx.wpt_trees_route() == SINGLE
        r = wx.relerrorthresholdall(td, True, _dev(wx, M))
        assert wx.wpt_trees_route() == SINGLE
        _close(wx.to_numpy(r), want_r, "identical columns, relerror")
        assert _bytes(wx, wx.relerrorthresholdall(td, True, M)) == _bytes(wx, r) and wx.wpt_trees_route() == HOST
        assert wx.relerrorthresholdall(td, True, M[:, 0]).tobytes() == _bytes(wx, r)   # the single-tree call itself


def _estimators(wx):
    return (("relerror", wx.RelErrorShrink(wx.HardTH(), 0.3), wx.relerrorthreshold, 2),
            ("sure", wx.SureShrink(wx.HardTH(), 0.3), wx.surethreshold, "sure"))


def _oracle_denoise(oracle, th, kind, qmf, trees, est, smooth):
    return np.stack([oracle.denoise(th[:, :, i], kind, qmf, tree=trees[:, i], th="hard", t=0.3, smooth=smooth, estnoise=float(est[i]))
                     for i in range(trees.shape[1])], axis=-1)


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("n", NS)
def test_denoiseall_on_a_table(wx, oracle, n, kind):
    import torch
    _, trees, _ = cases.case(n)
    trees = np.asarray(trees)
    td, th = _table(n, kind, "float64")
    N = trees.shape[1]
    want_t = _oracle(n, kind)
    wt = wx.wavelet(cases.WAVELET)
    dtb = _dev(wx, trees)
    tol = 20 * helpers.TOL[np.dtype(np.float64)]
    for name, dnt, est, key in _estimators(wx):
        if n >= 64:                                                    # on the oracle alone: every signal has zeroed and kept leaf coefficients
            o = _oracle_denoise(oracle, th, "swpd", None, trees, want_t[key], "regular")
            for i in range(N):
                leaves = cases.leaves_of(trees[:, i])
                assert (o[:, leaves, i] == 0).any() and (o[:, leaves, i] != 0).any(), (name, i)
        for smooth in ("regular", "undersmooth"):
            d = wx.denoiseall(td, kind, wt, tree=dtb, dnt=dnt, estnoise=est, smooth=smooth)
            assert wx.wpt_trees_route() == LDS
            assert isinstance(d, torch.Tensor) and d.is_cuda and tuple(d.shape) == (n, N)
            g = wx.to_numpy(d)
            want = _oracle_denoise(oracle, th, kind, wt.qmf, trees, want_t[key], smooth)
            errs = [helpers.relerr(g[:, i], want[:, i]) for i in range(N)]
            print(name, smooth, "against the oracle", max(errs))
            assert max(errs) <= tol, (name, smooth, int(np.argmax(errs)), max(errs))
            assert _bytes(wx, wx.denoiseall(td, kind, wt, tree=trees, dnt=dnt, estnoise=est, smooth=smooth)) == g.tobytes()   # host trees
            want_u = want                                              # after the loop: the oracle's undersmoothed signals
        # one summary threshold for the batch
        d = wx.denoiseall(td, kind, wt, tree=dtb, dnt=dnt, estnoise=est, bestTH=np.mean)
        want = _oracle_denoise(oracle, th, kind, wt.qmf, trees, np.full(N, np.mean(want_t[key])), "regular")
        e = helpers.relerr(wx.to_numpy(d), want)
        print(name, "bestTH = mean", e)
        assert e <= tol, (name, "bestTH", e)
        # the single-signal form with a one-column matrix (one column is a uniform batch: the single-tree pipeline)
        d1 = wx.denoise(td[:, :, 1], kind, wt, tree=dtb[:, 1:2], dnt=dnt, estnoise=est, smooth="undersmooth")
        assert tuple(d1.shape) == (n,) and helpers.relerr(wx.to_numpy(d1), want_u[:, 1]) <= tol, name
        if kind == "swpd":
            # wt = None: the thresholded table byte for byte, given the same threshold
            used = wx.to_numpy(wx.relerrorthresholdall(td, True, dtb) if name == "relerror" else wx.surethresholdall(td, True, dtb))
            for smooth in ("regular", "undersmooth"):
                tb = wx.denoiseall(td, "swpd", None, tree=dtb, dnt=dnt, estnoise=est, smooth=smooth)
                assert tuple(tb.shape) == tuple(td.shape)
                want = _oracle_denoise(oracle, th, "swpd", None, trees, used, smooth)
                got = wx.to_numpy(tb)
                assert got.dtype == want.dtype and got.tobytes() == want.tobytes(), (name, smooth)
    assert _bytes(wx, td) == th.tobytes(), "the input table was modified"


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("n", NS)
def test_from_the_signals_equals_the_table_way(wx, n, kind):
    from waveletsext_jl_amd import denoising
    x, trees, D = cases.case(n)
    trees = np.asarray(trees)
    td, _ = _table(n, kind, "float64")
    N = trees.shape[1]
    wt = wx.wavelet(cases.WAVELET)
    xd, dtb = wx.to_device(np.array(x)), _dev(wx, trees)
    f = wx.swpd_denoiseall if kind == "swpd" else wx.acwpd_denoiseall
    for name, dnt, est, _ in _estimators(wx):
        for smooth in ("regular", "undersmooth"):
            want = _bytes(wx, wx.denoiseall(td, kind, wt, tree=dtb, dnt=dnt, estnoise=est, smooth=smooth))
            assert _bytes(wx, f(xd, wt, dtb, D, dnt=dnt, estnoise=est, smooth=smooth)) == want, (name, smooth)
        assert _bytes(wx, f(xd, wt, trees, D, dnt=dnt, estnoise=est, smooth=smooth)) == want, (name, "host trees")
        want = _bytes(wx, wx.denoiseall(td, kind, wt, tree=dtb, dnt=dnt, estnoise=est, bestTH=np.mean))
        assert _bytes(wx, f(xd, wt, dtb, D, dnt=dnt, estnoise=est, bestTH=np.mean)) == want, (name, "bestTH")
    # the chunk budget forced small: tables of 10 signals, so the batch takes chunks of 10, 10 and a ragged rest
    budget = 10 * n * ((2 << D) - 1) * 8
    assert N > 20 and N % 10 != 0
    dnt, est = wx.RelErrorShrink(wx.HardTH(), 0.3), wx.relerrorthreshold
    want = _bytes(wx, wx.denoiseall(td, kind, wt, tree=dtb, dnt=dnt, estnoise=est))
    got = denoising._red_denoiseall(xd, wt, dtb, D, dnt, est, None, "regular", kind, select_budget=budget)
    assert _bytes(wx, got) == want
    thr = denoising._red_select(denoising.Arg(xd), wt, dtb, D, kind, 1, budget=budget)
    assert _bytes(wx, thr.arr) == _bytes(wx, wx.relerrorthresholdall(td, True, dtb))


@pytest.mark.parametrize("kind", KINDS)
def test_bestbasis_denoiseall_with_the_selections(wx, kind):
    """every signal in its own translation-invariant best basis, the trees never leaving the device: the table way with the same trees"""
    n = 64
    x, _, D = cases.case(n)
    wt = wx.wavelet(cases.WAVELET)
    xd = wx.to_device(np.array(x))
    trees = (wx.swpd_bestbasistreeall if kind == "swpd" else wx.acwpd_bestbasistreeall)(xd, wt, D, None, device=True)
    td, _ = _table(n, kind, "float64")
    for name, dnt, est, _ in _estimators(wx):
        want = _bytes(wx, wx.denoiseall(td, kind, wt, tree=trees, dnt=dnt, estnoise=est))
        assert _bytes(wx, wx.bestbasis_denoiseall(xd, wt, D, kind, dnt=dnt, estnoise=est)) == want, name
