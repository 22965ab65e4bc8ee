"""numpy restatement of the noise estimate and the threshold rules, the yardstick of tests/test_noisest_ref_cpu.py and
tests/test_gpu_noisest_nonfinite.py.

noisest = Wavelets.Threshold.mad!(finest details) / 0.6745 (Denoising.jl:214-232) in the element type T, with
Statistics.median!: NaN as soon as any value is NaN, else the middle of the sorted values, or middle(a, b) = a/2 + b/2
rounded in T; the deviations |y - m| are rounded in T, so Inf - Inf makes NaN ones and a finite difference that
overflows T makes +Inf.  The four threshold loops (HardTH, SoftTH, SemiSoftTH with the upper knee at 2t, SteinTH) are
restated as oracle/wx_oracle_impl.h writes them.  Wavelets.jl is not vendored: what the rules do with a NaN or
infinite t (and with 2|x| or 2t overflowing) follows that restatement, and parity with the package is unpinned.

cases() builds the non-finite and overflow detail vectors the tests feed to every noise-estimate kernel.
"""
import numpy as np

TH_KINDS = {"hard": 0, "soft": 1, "semisoft": 2, "stein": 3}


def median(y):
    """Statistics.median! of a 1-D array, in its dtype"""
    T = y.dtype.type
    if np.isnan(y).any():
        return T(np.nan)
    s = np.sort(y)
    n = s.size
    if n & 1:
        return s[n // 2]
    with np.errstate(invalid="ignore", over="ignore"):
        return T(T(s[n // 2 - 1] / T(2)) + T(s[n // 2] / T(2)))


def mad(y):
    """Wavelets.Threshold.mad!: median of |y - median(y)|, every step rounded in the dtype of y"""
    m = median(y)
    with np.errstate(invalid="ignore", over="ignore"):
        d = np.abs(y - m)
    return median(d)


def noisest_range(v):
    """mad!(v) / 0.6745 of a 1-D array of Float32 or Float64 values"""
    v = np.ascontiguousarray(v).ravel()
    T = v.dtype.type
    with np.errstate(over="ignore"):
        return T(mad(v) / T(0.6745))


def threshold(x, th, t):
    """threshold!(x, TH, t) of an array of Float32 or Float64 values (a copy), t rounded to the same type"""
    x = np.asarray(x)
    T = x.dtype.type
    t = T(t)
    two, one, zero = T(2), T(1), T(0)
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        av = np.abs(x)
        sg = np.where(x > 0, one, np.where(x < 0, -one, x)).astype(x.dtype)
        if th == "hard":
            out = np.where(av <= t, zero, x)
        elif th == "soft":
            sh = (av - t).astype(x.dtype)
            out = np.where(sh < 0, zero, sg * sh)
        elif th == "semisoft":
            tmp = ((two * av).astype(x.dtype) - T(two * t)).astype(x.dtype)
            out = np.where(av > T(two * t), x, np.where(tmp < 0, zero, sg * tmp))
        elif th == "stein":
            sh = (one - (T(t * t) / (x * x).astype(x.dtype)).astype(x.dtype)).astype(x.dtype)
            out = np.where(sh < 0, zero, x * sh)
        else:
            raise ValueError(th)
    return out.astype(x.dtype)


def same(a, b):
    """bit-equal arrays, any NaN matching any NaN (signed zeros must agree)"""
    a, b = np.asarray(a), np.asarray(b)
    if a.shape != b.shape or a.dtype != b.dtype:
        return False
    na, nb = np.isnan(a), np.isnan(b)
    if not (na == nb).all():
        return False
    it = np.int64 if a.dtype == np.float64 else np.int32
    return bool((a[~na].view(it) == b[~nb].view(it)).all())


def big(dtype):
    """a finite magnitude whose differences overflow the type: Float32 3e38, Float64 1.7e308"""
    return np.dtype(dtype).type(3e38 if np.dtype(dtype) == np.float32 else 1.7e308)


CASES = ("pinf", "ninf", "both", "inf_half_m1", "inf_half", "inf_half_p1", "half_ninf_half_pinf", "nan_inf",
         "mad_inf", "overflow", "wide", "subnormal", "signed_zero", "sigma_overflow")


def cases(cnt, dtype, rng):
    """{name: detail vector of cnt values} for every case of CASES: one +Inf; one -Inf; both; +Inf in cnt/2 - 1, cnt/2,
    cnt/2 + 1 slots (the median turns +Inf and NaN deviations follow); half -Inf, half +Inf (median NaN); NaN with Inf;
    40 % -Inf and 40 % +Inf around finite values (finite median, MAD +Inf); finite values whose deviations overflow the
    type; a Float64 range wider than DBL_MAX (+-1.5e308 among ordinary values); subnormals only; signed zeros with a
    few small values; a finite sigma with sigma * sqrt(2 log n) above the largest finite value"""
    T = np.dtype(dtype).type
    inf = T(np.inf)

    def base():
        return rng.standard_normal(cnt).astype(dtype)

    def put(v, m, val):
        m = max(0, min(cnt, m))
        v[rng.permutation(cnt)[:m]] = val
        return v

    out = {}
    out["pinf"] = put(base(), 1, inf)
    out["ninf"] = put(base(), 1, -inf)
    v = base()
    p = rng.permutation(cnt)
    v[p[0]] = inf
    if cnt > 1:
        v[p[1]] = -inf
    out["both"] = v
    out["inf_half_m1"] = put(base(), cnt // 2 - 1, inf)
    out["inf_half"] = put(base(), cnt // 2, inf)
    out["inf_half_p1"] = put(base(), cnt // 2 + 1, inf)
    v = np.full(cnt, inf, dtype=dtype)
    v[rng.permutation(cnt)[:cnt // 2]] = -inf
    out["half_ninf_half_pinf"] = v
    v = put(base(), 1, inf)
    v[rng.integers(cnt)] = np.nan
    out["nan_inf"] = v
    v = base()
    p = rng.permutation(cnt)
    v[p[:(2 * cnt) // 5]] = -inf
    v[p[(2 * cnt) // 5:(4 * cnt) // 5]] = inf
    out["mad_inf"] = v
    b = big(dtype)
    s = np.where(rng.random(cnt) < 0.6, 1.0, -1.0)
    out["overflow"] = (s * rng.uniform(0.5, 1.0, cnt) * float(b)).astype(dtype)
    v = base()
    w = T(1.5e308) if T is np.float64 else b
    m = max(1, cnt // 20)
    p = rng.permutation(cnt)
    v[p[:m]] = w
    v[p[m:2 * m]] = -w
    out["wide"] = v
    tiny = np.finfo(dtype).smallest_subnormal
    out["subnormal"] = (rng.integers(-1000, 1000, cnt) * float(tiny)).astype(dtype)
    v = np.where(rng.random(cnt) < 0.5, T(-0.0), T(0.0)).astype(dtype)
    v = put(v, cnt // 8, T(0.25))
    out["signed_zero"] = v
    out["sigma_overflow"] = (rng.uniform(-1.0, 1.0, cnt) * float(b)).astype(dtype)
    assert tuple(out) == CASES
    return out
