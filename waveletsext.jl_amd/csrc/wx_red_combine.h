// wx_red_combine.h -- the synthesis step of the depth-first walks over a redundant packet tree: two child columns of n values in LDS are
// combined into their parent's column, one lane per parent position.  Shared by k_red_trees (wx_red_trees.hip), k_denoise_red_trees
// (wx_denoise_red_trees.hip) and k_denoise_red_sig (wx_denoise_red_sig.hip).
// d = the parent's depth, s = 2^d, u = p >> d, np = n >> d:
//   RT_AVG    isdwt_step!(v, w1, w2, d, h, g), swt/swt_one_level.jl:257-277: the reconstruction from the children's class p mod s
//             (t0 = u + 1 mod np) plus the one from the class shifted by s (t0 = u), halved; either sum runs over the taps in the
//             reference's order (:305-316, with `m-1<<d` read as m - (1 << d)), in Float64 with fma, the child indices wrapped by true
//             modulo, so nodes shorter than the filter need no periodised taps -- the arithmetic of k_swt_inv_level (wx_swt1d.hip);
//   RT_SHIFT  isdwt_step!(v, w1, w2, d, sv, sw, h, g), :279-318, sv = sm mod 2^d and sw = sm mod 2^(d + 1).  Only the positions
//             p = sv (mod s) are produced, every other position of the parent is ZERO;
//   RT_AC     v = (w1 + w2) / sqrt(2) per node, acwt/acwt_one_level.jl:217-224, rounded node by node like the reference.
// qs: the QMF's taps (LDS or any memory every lane reads alike; not read by RT_AC).  The caller's barriers order the call against the
// writers of w1, w2 and the readers of out.
#pragma once
#include "wx_common.h"

namespace {

enum { RT_AVG = 0, RT_SHIFT = 1, RT_AC = 2 };

template <typename T, int KIND>
__device__ __forceinline__ void rt_combine(const T *w1, const T *w2, T *out, int n, int d, int sm, int F, const double *qs, int tid, int NT)
{
    if (KIND == RT_AC) {
        const double sqrt2 = 1.4142135623730951;
        for (int p = tid; p < n; p += NT) out[p] = (T)(((double)w1[p] + (double)w2[p]) / sqrt2);
    } else {
        const int s = 1 << d, np = n >> d, nc = np >> 1;
        const int sv = sm & (s - 1);                       // main2depthshift: sd[d]; sd[d + 1] = sv or sv + s
        const int shifted = (sm >> d) & 1;
        for (int p = tid; p < n; p += NT) {
            const int cls = p & (s - 1), u = p >> d;
            if (KIND == RT_SHIFT && cls != sv) { out[p] = (T)0; continue; }   // never the root: s = 1 there
            double acc = 0.0;
            for (int var = (KIND == RT_SHIFT ? shifted : 0); var <= (KIND == RT_SHIFT ? shifted : 1); ++var) {
                // var 0: sw == sv, parent sample t0 sits at class position t0 - 1; var 1: sw == sv + s
                const int swc = cls + var * s;
                const int t0 = var ? u : (u + 1 == np ? 0 : u + 1);
                const bool odd = t0 & 1;
                int k1 = t0 >> 1, k2 = k1;
                double v = 0.0;
                for (int m = 0; m < F / 2; ++m) {
                    const double a = (double)w1[swc + k1 * 2 * s], c = (double)w2[swc + k2 * 2 * s];
                    const double q0 = qs[2 * m], q1 = qs[2 * m + 1];
                    v = fma(odd ? q1 : q0, a, v);
                    v = fma(odd ? q0 : -q1, c, v);
                    k1 = k1 == 0 ? nc - 1 : k1 - 1;
                    k2 = k2 + 1 == nc ? 0 : k2 + 1;
                }
                acc += v;
            }
            out[p] = (T)(KIND == RT_AVG ? acc * 0.5 : acc);
        }
    }
}

}  // namespace
