// wx_acfilt.h -- the autocorrelation-shell half filter of a QMF, packed on the host for the kernels of the autocorrelation family
// (wx_swt1d.hip, wx_swt2d.hip through wx_api_swt.hip; wx_red_bb.hip).
#pragma once
#include "wx_common.h"
#include <math.h>
#include <string.h>

// acwt_utils.jl:7-48: a_k = 2 sum_i q[i] q[i+k]; b = c2 * a with c1 = 1/sqrt(2), c2 = c1/2
static inline void wx_pack_acfilter(const WxFilt &f, WxAcFilt *ac)
{
    memset(ac, 0, sizeof *ac);
    ac->F = f.F;
    ac->c1 = 1.0 / sqrt(2.0);
    const double c2 = ac->c1 / 2;
    for (int k = 1; k <= f.F - 1; ++k) {
        double r = 0.0;
        for (int i = 1; i <= f.F - k; ++i) r += f.q[i - 1] * f.q[i + k - 1];
        r *= 2;
        ac->b[k - 1] = c2 * r;
    }
}
