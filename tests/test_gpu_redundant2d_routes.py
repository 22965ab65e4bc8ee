"""GPU parity of the 2-D redundant transforms (csrc/wx_swt2d.hip) on every launch route, beyond one workgroup.

The host picks among seven kernels (routes F1 F2 F3 forward, I1 I2 I3 I4 inverse: csrc/wx_debug.h).  Every case here
first asks `wx.red2d_route` -- computed by the function the launch code itself calls -- and fails if the case no
longer takes the route it was written for, then compares with the CPU oracle (oracle.red2d_fwd / red2d_inv, a
restatement of SWT.jl / ACWT.jl and swt_one_level.jl:334-469) at helpers.TOL, per slice: each slice of a coefficient
table against that slice's own maximum.  The autocorrelation inverses and `swpt == swpd[..., -4^L:]` are exact.

The oracle always works in Float64 here, for a Float32 case on the same Float32 values (_ofwd, _oinv).  Run in Float32
it rounds after every tap, as the reference does, and that error is the larger one where a slice is small.  At depth 3
of an 8 x 8 image (part c) a slice holds a few Fourier components only (slice 0 is 8 times the image's mean in every
element), so some are 0.007 to 0.03 at most where their table reaches 2 to 3, and there the Float32 oracle is itself
1.8e-05 to 6.8e-05 of the slice's maximum away from its Float64 run (images 679, 1746, 3298, 4095 of
test_blockidx_y_wraps_two_pass_kernels_float32: slices 20, 0, 48, 0).  The kernels sum in Float64 and round once per
pass; against the Float32 oracle image 679 came out 2.14e-05 away on an MI355X, against the Float64 oracle it is
4.4e-06 away.

  a. several workgroups and several strips per image, all three containers, fused against forced two-pass
  b. the shift-based inverse for every shift
  c. every grid wrap-around loop goes round once (blockIdx.y 65535 jobs, blockIdx.x 2048 workgroups of 256 elements,
     the fused kernels' loop over 2048 workgroups)
The route table itself (test_route_table_*) needs no device and is not marked gpu."""
import numpy as np
import pytest

from helpers import TOL, random_tree_2d

gpu = pytest.mark.gpu
FLEN = {"haar": 2, "db4": 8, "db8": 16}
F64, F32 = np.float64, np.float32

# (m, n, dtype, wavelet, L, forward route, R of the deepest level, average-inverse route, R)
CASES_A = [
    (64, 128, F64, "db4", 3, "F1", 16, "I1", 16),     # 4 strips; n * 8 == 1024: on the boundary of I1
    (64, 128, F64, "haar", 3, "F1", 16, "I1", 16),
    (64, 256, F64, "db4", 3, "F1", 8, "I2", 0),       # just past the boundary
    (8, 128, F64, "db4", 3, "F1", 8, "I1", 8),        # 1 strip of 8 rows
    (4, 256, F64, "db4", 2, "F3", 0, "I2", 0),        # m % 8 != 0: two passes, 4 workgroups
    (4, 256, F64, "haar", 2, "F3", 0, "I2", 0),
    (96, 40, F64, "db4", 3, "F1", 16, "I2", 0),       # not dyadic, 6 strips
    (40, 96, F64, "db4", 3, "F1", 8, "I2", 0),
    (96, 40, F32, "db4", 3, "F1", 32, "I2", 0),
    (40, 96, F32, "db4", 3, "F3", 0, "I2", 0),
    (128, 128, F32, "db4", 3, "F1", 32, "I1", 32),
    (64, 256, F32, "db4", 3, "F1", 16, "I1", 16),     # n * 4 == 1024
    (64, 512, F32, "db4", 2, "F3", 0, "I2", 0),
    (32, 512, F64, "db4", 4, "F2", 8, "I2", 0),       # strips of 16 rows for s <= 4, of 8 rows for s = 8; last tile partial
    (32, 512, F64, "haar", 4, "F2", 16, "I2", 0),
    (32, 512, F64, "db8", 3, "F2", 8, "I2", 0),
    (32, 512, F64, "db8", 4, "F3", 0, "I2", 0),       # no geometry at s = 8: two passes for the whole call
]
# autocorrelation family, Float64: (m, n, wavelet, L, forward route, R)
CASES_AC = [
    (96, 40, "db4", 3, "F1", 16),
    (96, 40, "haar", 3, "F1", 16),
    (64, 128, "db4", 3, "F1", 16),
    (32, 512, "db4", 3, "F2", 16),                    # halo 2(F-1)s = 56 columns at s = 4 still fits tiles of 16 rows
]


def _id_a(c):
    return "%dx%d-%s-%s-L%d-%s-%s" % (c[0], c[1], np.dtype(c[2]).name, c[3], c[4], c[5], c[7])


def _wt(wx, name):
    return wx.wavelet(getattr(wx.WT, name))


def _img(rng, shape, dtype):
    return np.asfortranarray(rng.standard_normal(shape).astype(dtype))


def _fwd_route(wx, m, n, L, dtype, wname, ac=False):
    return wx.red2d_route(False, m, n, L, np.dtype(dtype).itemsize, FLEN[wname], ac=ac)


def _inv_routes(wx, m, n, L, dtype, wname, ac=False, shift=False):
    """the route of every level d = 0..L-1 of an inverse call"""
    return {wx.red2d_route(True, m, n, l, np.dtype(dtype).itemsize, FLEN[wname], ac=ac, shift=shift) for l in range(1, L + 1)}


def _need_fwd(wx, want, m, n, L, dtype, wname, ac=False):
    got = _fwd_route(wx, m, n, L, dtype, wname, ac)
    assert got == want, "forward %dx%d %s %s L=%d ac=%s takes route %s (R=%d), the case was written for %s (R=%d)" % (
        m, n, np.dtype(dtype).name, wname, L, ac, got[0], got[1], want[0], want[1])


def _need_inv(wx, want, m, n, L, dtype, wname, ac=False, shift=False):
    got = _inv_routes(wx, m, n, L, dtype, wname, ac, shift)
    assert got == {want}, "inverse %dx%d %s %s L=%d ac=%s shift=%s takes routes %s, the case was written for %s" % (
        m, n, np.dtype(dtype).name, wname, L, ac, shift, sorted(got), want)


def _close(got, exp, tol, what):
    """every slice (along dim 3) within tol of its own largest magnitude"""
    got = np.asarray(got, dtype=np.float64)
    exp = np.asarray(exp, dtype=np.float64)
    assert got.shape == exp.shape, (what, got.shape, exp.shape)
    if exp.ndim == 2:
        got, exp = got[..., None], exp[..., None]
    err = np.abs(got - exp).max(axis=(0, 1))
    den = np.abs(exp).max(axis=(0, 1))
    rel = err / np.where(den > 0, den, 1.0)
    k = int(np.argmax(rel))
    assert np.isfinite(got).all() and rel[k] <= tol, "%s: slice %d: error %.3g of the slice's maximum (tolerance %.3g)" % (
        what, k, rel[k], tol)


def _ofwd(oracle, kind, x, qmf, L):
    """the oracle's forward transform in Float64 of x's values"""
    return oracle.red2d_fwd(kind, np.asfortranarray(x, dtype=np.float64), qmf, L)


def _oinv(oracle, kind, xw, qmf, arg=None, sm=None):
    """the oracle's inverse in Float64 of xw's values"""
    return oracle.red2d_inv(kind, np.asfortranarray(xw, dtype=np.float64), qmf, arg, sm)


def _clip_tree(tree, L):
    """no node at depth L or below (the table has L levels)"""
    tree = tree.copy()
    tree[(4 ** L - 1) // 3:] = False
    return tree


def _default_or(wx, m, n, L):
    """iswpd(xw, wt) reconstructs from depth maxtransformlevels(min(m, n)): None only for a table of that depth"""
    return None if L == wx.maxtransformlevels(min(m, n)) else L


def _trees(wx, m, n, L, rng):
    """iswpd's second argument: the table's depth (left to the default where that is the depth of the table), a level
    below it, the pyramid, two random trees (nodes skipped and nodes kept)"""
    res = [_default_or(wx, m, n, L), max(L - 1, 1), _clip_tree(wx.maketree(m, n, L, "dwt"), L)]
    nfull = (4 ** L - 1) // 3
    for p in (0.6, 0.9):
        t = _clip_tree(random_tree_2d(m, n, rng, p), L)
        while not (t[1:5].any() and not t[:nfull].all()):                        # some nodes kept, some skipped
            t = _clip_tree(random_tree_2d(m, n, rng, p), L)
        res.append(t)
    return res


class _forced:
    """wx.set_force_generic(1) for a block: the two-pass kernels instead of the one-pass levels"""

    def __init__(self, wx):
        self.wx = wx

    def __enter__(self):
        self.wx.set_force_generic(1)

    def __exit__(self, *exc):
        self.wx.set_force_generic(0)


# ---- the route table: needs no device ---------------------------------------------------------------------------------
def test_route_table_normal_dispatch(wx):
    for (m, n, dtype, wname, L, fr, fR, ir, iR) in CASES_A:
        _need_fwd(wx, (fr, fR), m, n, L, dtype, wname)
        _need_inv(wx, (ir, iR), m, n, L, dtype, wname)
        _need_inv(wx, ("I3", 0), m, n, L, dtype, wname, shift=True)
    seen = set()
    for (m, n, wname, L, fr, fR) in CASES_AC:
        _need_fwd(wx, (fr, fR), m, n, L, F64, wname, ac=True)
        _need_inv(wx, ("I4", 0), m, n, L, F64, wname, ac=True)
        seen.add(fr)
    assert seen >= {"F1", "F2"}
    assert {c[5] for c in CASES_A} == {"F1", "F2", "F3"} and {c[7] for c in CASES_A} == {"I1", "I2"}
    # the strip height of F2 changes between the levels of one call (32 x 512 Float64 db4)
    assert [_fwd_route(wx, 32, 512, L, F64, "db4") for L in (1, 2, 3, 4)] == [("F2", 16)] * 3 + [("F2", 8)]
    with pytest.raises(ValueError):
        wx.red2d_route(False, 8, 8, 1, 2, 8)


def test_route_table_forced_two_pass(wx):
    with _forced(wx):
        for (m, n, dtype, wname, L, fr, fR, ir, iR) in CASES_A:
            _need_fwd(wx, ("F3", 0), m, n, L, dtype, wname)
            _need_inv(wx, ("I2", 0), m, n, L, dtype, wname)
            _need_inv(wx, ("I3", 0), m, n, L, dtype, wname, shift=True)
        for (m, n, wname, L, fr, fR) in CASES_AC:
            _need_fwd(wx, ("F3", 0), m, n, L, F64, wname, ac=True)
            _need_inv(wx, ("I4", 0), m, n, L, F64, wname, ac=True)
    _need_fwd(wx, ("F1", 16), 64, 128, 3, F64, "db4")               # and back


# ---- a. several workgroups and several strips per image ----------------------------------------------------------------
@gpu
@pytest.mark.parametrize("case", CASES_A, ids=_id_a)
def test_all_containers_forward_and_average_inverse(wx, oracle, case):
    m, n, dtype, wname, L, fr, fR, ir, iR = case
    _need_fwd(wx, (fr, fR), m, n, L, dtype, wname)
    _need_inv(wx, (ir, iR), m, n, L, dtype, wname)
    rng = np.random.default_rng(5100 + m + n)
    wt = _wt(wx, wname)
    tol = TOL[np.dtype(dtype)]
    x = _img(rng, (m, n), dtype)
    exp = {kind: _ofwd(oracle, kind, x, wt.qmf, L) for kind in ("dwt", "wpt", "wpd")}
    got = {"dwt": wx.sdwt(x, wt, L), "wpt": wx.swpt(x, wt, L), "wpd": wx.swpd(x, wt, L)}
    for kind in exp:
        assert got[kind].dtype == dtype
        _close(got[kind], exp[kind], tol, "forward " + kind)
    assert (got["wpt"] == got["wpd"][:, :, -4 ** L:]).all()                     # test/transforms.jl:111-112
    if fr != "F3":
        # the one-pass level computes each sum in the order of the two passes: the same bits
        with _forced(wx):
            _need_fwd(wx, ("F3", 0), m, n, L, dtype, wname)
            two = {"dwt": wx.sdwt(x, wt, L), "wpt": wx.swpt(x, wt, L), "wpd": wx.swpd(x, wt, L)}
        for kind in exp:
            assert (got[kind] == two[kind]).all(), "one-pass and two-pass forward differ: " + kind
    # inverses of the oracle's coefficients, in the case's type
    coef = {kind: np.asfortranarray(exp[kind], dtype=dtype) for kind in exp}
    calls = [("dwt", None, lambda: wx.isdwt(coef["dwt"], wt)), ("wpt", None, lambda: wx.iswpt(coef["wpt"], wt))]
    for arg in _trees(wx, m, n, L, rng):
        calls.append(("wpd", arg, lambda arg=arg: wx.iswpd(coef["wpd"], wt, arg)))
    for kind, arg, fn in calls:
        what = "inverse %s %s" % (kind, "" if arg is None else ("L=%d" % arg if isinstance(arg, int) else "tree"))
        back = fn()
        assert back.dtype == dtype
        ref = _oinv(oracle, kind, coef[kind], wt.qmf, arg)
        _close(back, ref, tol, what + " against the oracle")
        _close(back, x, 20 * tol, what + " against the image")
        if ir == "I1":
            # the one-pass level merges dim 1 first, the two passes dim 2 first: equal to rounding
            with _forced(wx):
                _need_inv(wx, ("I2", 0), m, n, L, dtype, wname)
                _close(fn(), back, tol, what + ": two-pass against one-pass")


@gpu
@pytest.mark.parametrize("case", CASES_AC, ids=lambda c: "%dx%d-%s-%s" % (c[0], c[1], c[2], c[4]))
def test_autocorrelation_family(wx, oracle, case):
    m, n, wname, L, fr, fR = case
    _need_fwd(wx, (fr, fR), m, n, L, F64, wname, ac=True)
    _need_inv(wx, ("I4", 0), m, n, L, F64, wname, ac=True)
    rng = np.random.default_rng(5200 + m + n)
    wt = _wt(wx, wname)
    tol = TOL[np.dtype(F64)]
    x = _img(rng, (m, n), F64)
    exp = {kind: oracle.red2d_fwd(kind, x, wt.qmf, L, ac=True) for kind in ("dwt", "wpt", "wpd")}
    got = {"dwt": wx.acdwt(x, wt, L), "wpt": wx.acwpt(x, wt, L), "wpd": wx.acwpd(x, wt, L)}
    for kind in exp:
        _close(got[kind], exp[kind], tol, "ac forward " + kind)
    assert (got["wpt"] == got["wpd"][:, :, -4 ** L:]).all()                     # test/transforms.jl:169-170
    with _forced(wx):
        _need_fwd(wx, ("F3", 0), m, n, L, F64, wname, ac=True)
        two = {"dwt": wx.acdwt(x, wt, L), "wpt": wx.acwpt(x, wt, L), "wpd": wx.acwpd(x, wt, L)}
    for kind in exp:
        assert (got[kind] == two[kind]).all(), "one-pass and two-pass ac forward differ: " + kind
    # the ac inverse is a pairwise sum in the reference's order: exact
    calls = [("dwt", None, lambda: wx.iacdwt(exp["dwt"])), ("wpt", None, lambda: wx.iacwpt(exp["wpt"]))]
    for arg in _trees(wx, m, n, L, rng)[1:]:
        calls.append(("wpd", arg, lambda arg=arg: wx.iacwpd(exp["wpd"], wt, arg)))
    for kind, arg, fn in calls:
        back = fn()
        assert (back == oracle.red2d_inv(kind, exp[kind], None, arg, ac=True)).all(), ("ac inverse", kind, arg)
        _close(back, x, tol, "ac inverse %s against the image" % kind)


# ---- b. the shift-based inverse for every shift -------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("wname", ["db4", "haar"])
@pytest.mark.parametrize("shape", [(96, 40, F64), (40, 96, F32), (32, 64, F64)], ids=lambda s: "%dx%d-%s" % (s[0], s[1], np.dtype(s[2]).name))
def test_shift_based_inverse_every_shift(wx, oracle, shape, wname):
    m, n, dtype = shape
    L = 3
    _need_inv(wx, ("I3", 0), m, n, L, dtype, wname, shift=True)
    rng = np.random.default_rng(5300 + m)
    wt = _wt(wx, wname)
    tol = TOL[np.dtype(dtype)]
    x = _img(rng, (m, n), dtype)
    exp = {kind: np.asfortranarray(_ofwd(oracle, kind, x, wt.qmf, L), dtype=dtype) for kind in ("dwt", "wpt", "wpd")}
    tree = _clip_tree(random_tree_2d(m, n, rng, 0.7), L)
    calls = [("dwt", None, sm) for sm in range(1, 1 << L)]
    calls += [("wpt", None, sm) for sm in range(1 << L)]
    calls += [("wpd", arg, sm) for arg in (_default_or(wx, m, n, L), tree) for sm in range(1 << L)]
    for kind, arg, sm in calls:
        if kind == "dwt":
            back = wx.isdwt(exp[kind], wt, sm)
        elif kind == "wpt":
            back = wx.iswpt(exp[kind], wt, sm)
        else:
            back = wx.iswpd(exp[kind], wt, arg, sm)
        what = "shift inverse %s sm=%d%s" % (kind, sm, " tree" if isinstance(arg, np.ndarray) else "")
        assert back.dtype == dtype
        _close(back, _oinv(oracle, kind, exp[kind], wt.qmf, arg, sm), tol, what + " against the oracle")
        _close(back, x, 20 * tol, what + " against the image")


@gpu
def test_iswpd_table_deeper_than_the_tree(wx, oracle):
    m, n, L = 96, 40, 3
    rng = np.random.default_rng(5400)
    wt = _wt(wx, "db4")
    tol = TOL[np.dtype(F64)]
    x = _img(rng, (m, n), F64)
    xw = oracle.red2d_fwd("wpd", x, wt.qmf, L)
    full2 = wx.maketree(m, n, 2, "full")
    assert full2[:5].all() and not full2[5:].any()
    for arg in (2, full2):
        for sm in (None, 0, 1, 2, 3, 5, 7):
            back = wx.iswpd(xw, wt, arg, sm)
            _close(back, oracle.red2d_inv("wpd", xw, wt.qmf, arg, sm), tol, "depth-2 tree, sm=%s" % sm)
            _close(back, x, 20 * tol, "depth-2 tree, sm=%s against the image" % sm)


# ---- c. every wrap-around loop wraps once -------------------------------------------------------------------------------
def _sample(last, special):
    return sorted(set(special) | set(range(0, last + 1, 97)) | {0, last})


@gpu
def test_blockidx_y_wraps_two_pass_kernels_float32(wx, oracle):
    """8 x 8 images, L = 3, wpt container, 4097 images: 65552 jobs at depth 2 (k_red2d_fwd_dim1, k_red2d_inv_dim1) and
    131104 half-jobs (k_red2d_fwd_dim2, k_red2d_inv_dim2) on a grid.y of 65535; Float32 has no strip of 8 rows, so the
    routes are F3, I2 and (with a shift) I3.  Job 65535 belongs to image 4095, half-job 65535 to image 2047.

    The smallest slice among the sampled images is slice 0 of image 1746 (0.0072 at most, 2.3 for its table): storing
    the two passes of three levels in Float32 alone puts it 9.9e-06 of that maximum from the Float64 oracle (the
    module's docstring has the Float32 oracle's own figures)."""
    m = n = 8
    L, B = 3, 4097
    assert B * 16 > 65535 and B * 4 <= 65535
    _need_fwd(wx, ("F3", 0), m, n, L, F32, "db4")
    _need_inv(wx, ("I2", 0), m, n, L, F32, "db4")
    _need_inv(wx, ("I3", 0), m, n, L, F32, "db4", shift=True)
    rng = np.random.default_rng(5500)
    wt = _wt(wx, "db4")
    tol = TOL[np.dtype(F32)]
    X = _img(rng, (m, n, B), F32)
    xw = wx.swptall(X, wt, L)
    back = wx.iswptall(xw, wt)
    back5 = wx.iswptall(xw, wt, 5)
    assert xw.dtype == back.dtype == back5.dtype == F32
    for i in _sample(B - 1, (2047, 2048, 4094, 4095)):
        xi, wi = np.asfortranarray(X[..., i]), np.asfortranarray(xw[..., i])
        _close(wi, _ofwd(oracle, "wpt", xi, wt.qmf, L), tol, "image %d forward" % i)
        _close(back[..., i], _oinv(oracle, "wpt", wi, wt.qmf), tol, "image %d average inverse" % i)
        _close(back5[..., i], _oinv(oracle, "wpt", wi, wt.qmf, sm=5), tol, "image %d shift inverse" % i)
    _close(back, X, 20 * tol, "average inverse, every image")                 # (slices here are the images)
    _close(back5, X, 20 * tol, "shift inverse, every image")


@gpu
def test_blockidx_y_wraps_autocorrelation_inverse(wx, oracle):
    """the same batch through acwpt / iacwpt in Float64: k_red2d_iac has 65552 jobs at depth 2"""
    m = n = 8
    L, B = 3, 4097
    _need_inv(wx, ("I4", 0), m, n, L, F64, "db4", ac=True)
    fr = _fwd_route(wx, m, n, L, F64, "db4", ac=True)
    assert fr == ("F1", 8), fr
    rng = np.random.default_rng(5501)
    wt = _wt(wx, "db4")
    X = _img(rng, (m, n, B), F64)
    xw = wx.acwptall(X, wt, L)
    back = wx.iacwptall(xw)
    for i in _sample(B - 1, (4094, 4095)):
        xi, wi = np.asfortranarray(X[..., i]), np.asfortranarray(xw[..., i])
        _close(wi, oracle.red2d_fwd("wpt", xi, wt.qmf, L, ac=True), 1e-10, "image %d ac forward" % i)
        assert (back[..., i] == oracle.red2d_inv("wpt", wi, ac=True)).all(), i
    _close(back, X, 1e-10, "ac inverse, every image")


@gpu
def test_blockidx_x_wraps_two_pass_kernels(wx, oracle):
    """1024 x 1024 Float32, L = 1: 4096 workgroups of elements on a grid.x of 2048 (k_red2d_fwd_dim1 / _dim2,
    k_red2d_inv_dim2 / _dim1, average based)"""
    m = n = 1024
    assert m * n > 2048 * 256
    _need_fwd(wx, ("F3", 0), m, n, 1, F32, "db4")
    _need_inv(wx, ("I2", 0), m, n, 1, F32, "db4")
    rng = np.random.default_rng(5600)
    wt = _wt(wx, "db4")
    tol = TOL[np.dtype(F32)]
    x = _img(rng, (m, n), F32)
    exp = _ofwd(oracle, "dwt", x, wt.qmf, 1)
    got = wx.sdwt(x, wt, 1)
    _close(got, exp, tol, "forward")
    coef = np.asfortranarray(exp, dtype=F32)
    back = wx.isdwt(coef, wt)
    assert got.dtype == back.dtype == F32
    _close(back, _oinv(oracle, "dwt", coef, wt.qmf), tol, "average inverse against the oracle")
    _close(back, x, 20 * tol, "average inverse against the image")


@gpu
def test_blockidx_x_wraps_shift_based_inverse(wx, oracle):
    """2048 x 1024 Float32, L = 1, sm = 1: the rows pass of the shift-based inverse handles (m / 2) * n = 1 Mi
    elements per half-job, the columns pass m * n = 2 Mi, on a grid.x of 2048 workgroups"""
    m, n = 2048, 1024
    assert (m >> 1) * n > 2048 * 256
    _need_inv(wx, ("I3", 0), m, n, 1, F32, "db4", shift=True)
    rng = np.random.default_rng(5601)
    wt = _wt(wx, "db4")
    tol = TOL[np.dtype(F32)]
    x = _img(rng, (m, n), F32)
    xw = wx.sdwt(x, wt, 1)
    back = wx.isdwt(xw, wt, 1)
    assert xw.dtype == back.dtype == F32
    _close(back, _oinv(oracle, "dwt", xw, wt.qmf, sm=1), tol, "shift inverse against the oracle")
    _close(back, x, 20 * tol, "shift inverse against the image")


@gpu
def test_blockidx_x_wraps_autocorrelation_inverse(wx, oracle):
    """1024 x 1024 Float64, L = 1: k_red2d_iac over 4096 workgroups of elements on a grid.x of 2048"""
    m = n = 1024
    _need_inv(wx, ("I4", 0), m, n, 1, F64, "db4", ac=True)
    rng = np.random.default_rng(5602)
    wt = _wt(wx, "db4")
    x = _img(rng, (m, n), F64)
    exp = oracle.red2d_fwd("dwt", x, wt.qmf, 1, ac=True)
    _close(wx.acdwt(x, wt, 1), exp, 1e-10, "ac forward")
    back = wx.iacdwt(exp)
    assert (back == oracle.red2d_inv("dwt", exp, ac=True)).all()
    _close(back, x, 1e-10, "ac inverse against the image")


@gpu
def test_fused_block_loop_wraps_whole_rows(wx, oracle):
    """33 images 16 x 16 Float64, L = 4, wpt container: at depth 3 the one-pass kernels have 33 * 64 = 2112 strips for
    2048 workgroups (k_red2d_fwd_fused with whole rows, k_red2d_inv_fused); the strips past the cap are image 32"""
    m = n = 16
    L, B = 4, 33
    assert B * 64 > 2048 and (B - 1) * 64 <= 2048
    _need_fwd(wx, ("F1", 16), m, n, L, F64, "db4")
    _need_inv(wx, ("I1", 16), m, n, L, F64, "db4")
    rng = np.random.default_rng(5700)
    wt = _wt(wx, "db4")
    tol = TOL[np.dtype(F64)]
    X = _img(rng, (m, n, B), F64)
    xw = wx.swptall(X, wt, L)
    back = wx.iswptall(xw, wt)
    for i in range(B):
        xi, wi = np.asfortranarray(X[..., i]), np.asfortranarray(xw[..., i])
        _close(wi, oracle.red2d_fwd("wpt", xi, wt.qmf, L), tol, "image %d forward" % i)
        _close(back[..., i], oracle.red2d_inv("wpt", wi, wt.qmf), tol, "image %d inverse" % i)
    _close(back, X, 20 * tol, "inverse, every image")


@gpu
def test_fused_block_loop_wraps_column_tiles(wx, oracle):
    """16 x 288 Float64, sdwt with db4, L = 1: one strip of 16 rows and 3 column tiles (115 + 115 + 58 columns) per
    image, so 683 images are 2049 workgroups' worth for a grid of 2048: the tile past the cap is the partial one of
    the last image"""
    m, n, B = 16, 288, 683
    _need_fwd(wx, ("F2", 16), m, n, 1, F64, "db4")
    tiles = -(-n // (128 - 7 - 6))
    assert tiles == 3 and B * tiles > 2048 and (B - 1) * tiles <= 2048
    rng = np.random.default_rng(5701)
    wt = _wt(wx, "db4")
    tol = TOL[np.dtype(F64)]
    X = _img(rng, (m, n, B), F64)
    xw = wx.sdwtall(X, wt, 1)
    for i in (0, 1, 341, 681, 682):
        _close(xw[..., i], oracle.red2d_fwd("dwt", np.asfortranarray(X[..., i]), wt.qmf, 1), tol, "image %d forward" % i)
    _close(wx.isdwtall(xw, wt), X, 20 * tol, "round trip, every image")
