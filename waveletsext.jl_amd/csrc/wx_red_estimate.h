// wx_red_estimate.h -- the noise estimate of the per-signal-tree denoising kernels on redundant packet trees, by one wavefront, and the two
// nodes of a tree it and the undersmoothing rule need.  Shared by k_denoise_red_trees (wx_denoise_red_trees.hip: the column comes from the
// table) and k_denoise_red_sig (wx_denoise_red_sig.hip: the column has been computed into LDS).
//   sigma = mad(column of the finest detail node) / 0.6745 (noisest, Denoising.jl:228-231): the n values go straight into n / 64 registers
//   per lane and the two medians are found by counting against pivots with ballots (dn_noisest, wx_select_count.h: exact order statistics,
//   middle(a, b) = a/2 + b/2, the deviations rounded in T, NaN for a NaN among the details or a non-finite median -- the arithmetic of
//   k_mad_count, so the result is wx_noisest_*'s bit for bit).  n < 64: the lanes beyond n hold +Inf, which the counting never ranks.
#pragma once
#include "wx_common.h"
#include "wx_select_count.h"
#include "wx_tree_bits.h"

namespace {

constexpr int DRT_MAXLOG2N = 10;                                       // 16 registers per lane (32 spill in the Float32 kernel)

// sigma of the n = 2^log2n values of `col`, by one whole wavefront (every lane calls): NR = max(1, n / 64) registers per lane
template <typename T, int NR> __device__ __forceinline__ T drt_mad(const T *__restrict__ col, int n, int lane)
{
    double e[NR];
#pragma unroll
    for (int u = 0; u < NR; ++u) {
        const int i = lane + 64 * u;
        e[u] = i < n ? (double)col[i] : __builtin_inf();
    }
    double sg[1];
    dn_noisest<-1, 64, 1, NR, T>(e, sg, true, n);
    return (T)sg[0];
}
template <typename T> __device__ __forceinline__ T drt_estimate(const T *__restrict__ col, int log2n, int lane)
{
    const int n = 1 << log2n;
    switch (log2n) {                                                   // uniform
    case 10: return drt_mad<T, 16>(col, n, lane);
    case 9: return drt_mad<T, 8>(col, n, lane);
    case 8: return drt_mad<T, 4>(col, n, lane);
    case 7: return drt_mad<T, 2>(col, n, lane);
    default: return drt_mad<T, 1>(col, n, lane);
    }
}

// the finest detail node of the tree whose words are tg (global or LDS): right children from the root; depth < dmax holds for every tree
// that passed the check, and keeps the node's column inside the table whatever the words hold
__device__ __forceinline__ int drt_finest(const uint32_t *tg, int ntree, int dmax)
{
    int node = 1;
    for (int d = 0; node <= ntree && d < dmax && wt_set(tg, node); ++d) node = 2 * node + 1;
    return node;
}
// the coarsest scaling node: left children from the root, the strict `<` of Utils.jl:363-367
__device__ __forceinline__ int drt_coarsest(const uint32_t *tg, int ntree, int dmax)
{
    int node = 1;
    for (int d = 0; node < ntree && d < dmax && wt_set(tg, node); ++d) node = 2 * node;
    return node;
}

}  // namespace
