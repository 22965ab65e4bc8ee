"""The noise-estimate and threshold yardstick (tests/noisest_ref.py) against the CPU oracle, without a GPU: every non-finite
and overflow case of noisest_ref.cases() at the detail counts the GPU kernels are chosen by, in both types, and the four
threshold rules on +-0, subnormals, +-t, +-2t, huge values, +-Inf and NaN with t = 0, finite, +Inf and NaN.  NaN cases
compare with the oracle too: its median is NaN as soon as a value is NaN, like Statistics.median!."""
import numpy as np
import pytest

import noisest_ref as R

COUNTS = (1, 2, 3, 5, 16, 32, 33, 100, 128, 256, 300, 512, 1024, 3000, 8192)


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_noisest_ref_matches_the_oracle(oracle, dtype):
    rng = np.random.default_rng(6745)
    for cnt in COUNTS:
        for name, v in R.cases(cnt, dtype, rng).items():
            got = R.noisest_range(v)
            exp = oracle.noisest_range(v)
            assert got.dtype == np.dtype(dtype)
            assert R.same(np.array([got]), np.array([exp], dtype=dtype)), (cnt, name, got, exp)


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_cases_reach_the_semantics_they_name(dtype):
    """the cases make what they are meant to: NaN where the median is not finite, +Inf MAD, overflowing deviations"""
    rng = np.random.default_rng(31)
    T = np.dtype(dtype).type
    for cnt in (256, 1024):
        c = R.cases(cnt, dtype, rng)
        for name in ("inf_half_p1", "half_ninf_half_pinf", "nan_inf"):
            assert np.isnan(R.noisest_range(c[name])), name
        for name in ("pinf", "ninf", "both", "inf_half_m1", "overflow", "wide", "subnormal", "signed_zero", "sigma_overflow"):
            assert np.isfinite(R.noisest_range(c[name])), name
        assert np.isnan(R.noisest_range(c["inf_half"]))              # cnt/2 copies: middle(x, Inf) = Inf
        assert R.noisest_range(c["mad_inf"]) == np.inf
        with np.errstate(over="ignore"):
            assert np.isinf(np.abs(c["overflow"] - R.median(c["overflow"]))).any()
            assert not np.isfinite(T(R.noisest_range(c["sigma_overflow"]) * T(np.sqrt(2 * np.log(2 * cnt)))))
        assert R.noisest_range(c["subnormal"]) > 0 and np.abs(c["subnormal"]).max() < np.finfo(dtype).tiny
        assert R.noisest_range(c["signed_zero"]) == 0
        if dtype == np.float64:
            with np.errstate(over="ignore"):
                assert np.ptp(c["wide"]) == np.inf                      # hi - lo overflows
    assert np.isnan(R.median(np.array([1.0, np.nan, 2.0])))
    assert np.isnan(R.median(np.array([-np.inf, np.inf])))


def threshold_values(dtype, t):
    T = np.dtype(dtype).type
    tiny = np.finfo(dtype).smallest_subnormal
    huge = R.big(dtype)
    base = [0.0, -0.0, tiny, -tiny, 1.0, -1.0, huge, -huge, np.inf, -np.inf, np.nan, 0.35, -2.5]
    if np.isfinite(t):
        base += [t, -t, 2 * t, -2 * t, np.nextafter(t, np.inf), np.nextafter(2 * t, 0.0)]
    with np.errstate(over="ignore"):
        return np.array(base, dtype=T)


THRESHOLDS = (0.0, 0.7, np.inf, np.nan)


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("th", ["hard", "soft", "semisoft", "stein"])
def test_threshold_ref_matches_the_oracle(oracle, dtype, th):
    for t in THRESHOLDS + (float(R.big(dtype)),):
        x = threshold_values(dtype, t)
        got = R.threshold(x, th, t)
        exp = oracle.threshold(x, th, t)
        assert R.same(got, exp), (th, t, x, got, exp)
    # the Hard rule on the infinite threshold: abs(x) <= Inf drops +-Inf too, NaN stays
    y = R.threshold(np.array([np.inf, -np.inf, np.nan, 1.0], dtype=dtype), "hard", np.inf)
    assert y[0] == 0 and y[1] == 0 and np.isnan(y[2]) and y[3] == 0
