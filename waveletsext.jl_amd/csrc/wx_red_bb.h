// wx_red_bb.h -- what the two kernels that start from the SIGNALS of a redundant packet decomposition share: k_red_bb (wx_red_bb.hip: costs
// and best-basis trees) and k_denoise_red_sig (wx_denoise_red_sig.hip: denoising along given trees).  The analysis step, the launch
// geometry (also asked by wx_debug_red_bb_grid, so that the tests see the functions the launches call) and the route record.
#pragma once
#include "wx_common.h"
#include "wx_host.h"
#include "wx_tree_bits.h"
#include "wx_trees_geom.h"                     // wx_trees_threads, wx_trees_grid: the launch geometry of the per-signal-tree kernels

// wx_red_bb_last_route (include/waveletsext_hip.h), per thread; defined in wx_red_bb.hip
enum { RB_ROUTE_NONE = 0, RB_ROUTE_FUSED = 1, RB_ROUTE_CHUNKED = 2, RB_ROUTE_TRIVIAL = 3 };
void wx_red_bb_route_set(int route);

namespace {

constexpr size_t RB_LDS_MAX = 160 * 1024;
constexpr size_t RB_CHUNK_TABLE_BYTES = (size_t)256 << 20;       // route 2: packet table of one chunk of signals
constexpr int RB_RED = 16;                                       // wavefronts of a workgroup, at most
enum { RB_TREES = 0, RB_DENOISE = 1 };                           // `which` of wx_debug_red_bb_grid

// Both children of position i of a column v of n = msk + 1 values (LDS or global) at dilation s = 2^depth, Float64 accumulators with fma:
//   stationary       sdwt_step!, swt/swt_one_level.jl:99-127: a = sum_j q[j] v[i + (j - 1) s], dd = sum_j (-1)^j q[j] v[i - j s] in the
//                    reference's tap order, the positions wrapped by true modulo -- the arithmetic of k_swt_fwd_level (wx_swt1d.hip);
//   autocorrelation  acdwt_step!, acwt/acwt_one_level.jl:101-128: a = c1 v[i] + S, dd = c1 v[i] - S, S = sum over the odd lags l of
//                    b_l (v[i - l s] + v[i + l s]), qs[l - 1] = b_l (acwt_utils.jl:7-72; the even lags are exactly zero and skipped).
template <typename T, bool AC>
__device__ __forceinline__ void rb_step(const T *v, int i, int s, int msk, int F, const double *qs, double c1, double &a, double &dd)
{
    if (!AC) {
        a = 0.0; dd = 0.0;
        int k1 = (i - s) & msk, k2 = i;
        for (int j = 0; j < F; ++j) {
            const double q = qs[j];
            a = fma(q, (double)v[k1], a);
            dd = fma((j & 1) ? -q : q, (double)v[k2], dd);
            k1 = (k1 + s) & msk;
            k2 = (k2 - s) & msk;
        }
    } else {
        double S = 0.0;
        int km = (i - s) & msk, kp = (i + s) & msk;
        for (int l = 1; l < F; l += 2) {                               // odd lags only
            S = fma(qs[l - 1], (double)v[km] + (double)v[kp], S);
            km = (km - 2 * s) & msk;
            kp = (kp + 2 * s) & msk;
        }
        const double cv = c1 * (double)v[i];
        a = cv + S;
        dd = cv - S;
    }
}

// k_red_bb:           64 doubles of taps | RB_RED + 4 RB_RED doubles of partial sums | 2 L + 1 columns | 2^(L+1) - 1 costs | as many flag bytes
// k_denoise_red_sig:  64 doubles of taps | 2 L columns | the tree's words | 16 bytes of static LDS (the estimate)
inline size_t rb_lds(int64_t n, int L, size_t esz, int which)
{
    size_t b;
    if (which == RB_TREES) {
        const size_t ncost = ((size_t)2 << L) - 1;
        b = sizeof(double) * (WX_MAXF + 5 * RB_RED) + (size_t)(2 * L + 1) * (size_t)n * esz + ncost * (esz + 1);
    } else {
        b = sizeof(double) * WX_MAXF + (size_t)(2 * L) * (size_t)n * esz + sizeof(uint32_t) * wt_words(n) + 16;
    }
    return (b + 15) & ~(size_t)15;
}

// dyadic 8 <= n, even filters of 2 .. 20 taps, 1 <= L <= log2 n, 160 KiB; the denoise kernel holds the estimate's column in 16 registers
// per lane: n <= 1024
inline bool rb_window(int64_t n, int L, int F, size_t esz, int which)
{
    if (!wx_isdyadic(n) || n < 8 || n > ((int64_t)1 << 20) || F < 2 || F > 20 || (F & 1)) return false;
    if (L < 1 || L > wx_maxtransformlevels(n)) return false;
    if (which == RB_DENOISE && n > 1024) return false;
    return rb_lds(n, L, esz, which) <= RB_LDS_MAX;
}

inline int rb_threads(int64_t n) { return wx_trees_threads(2 * n); }   // one lane per position of a column

// workgroups of a launch: as many as stay resident, never more than signals
inline int rb_grid(int64_t n, int L, size_t esz, int which, int64_t batch)
{ return wx_trees_grid(rb_lds(n, L, esz, which), rb_threads(n), batch); }

}  // namespace
