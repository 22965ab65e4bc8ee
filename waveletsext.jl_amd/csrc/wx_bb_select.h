// wx_bb_select.h -- the two sweeps of the bottom-up best-basis selection over one signal's cost vector, shared by the selection kernels
// of wx_bb.hip (costs staged from a cost matrix) and the fused kernel of wx_wpd_bb.hip (costs computed where they lie).
//   bestbasis_treeselection        BestBasis.jl:59-110, delete_subtree! :128-140
// The sequential reference (i = ntree..1: keep the children's sum when it beats the parent, else delete_subtree!(i)) is
// level-synchronous: a node's decision needs only its children's final costs, and deleting a subtree clears exactly the nodes that
// have a pruned ancestor-or-self, so   tree[i] = full[i] && !pruned[i] && tree[parent(i)].
#pragma once
#include "wx_common.h"

namespace {

// c: the costs of the full tree of depth L in heap order (T, mutated like the reference); flag: one byte per node, 1 = pruned after the
// first sweep, the tree bit after the second.  `tid` of `nt` lanes share the vectors; sync() orders one level after the other for
// them (a workgroup barrier, or a wavefront fence where one wavefront owns the vectors) and is called by all of them, 2 L times.
template <typename T, int ARITY, typename I, typename Sync>
__device__ __forceinline__ void bb_select_sweeps(T *c, uint8_t *flag, int L, int type_max, I tid, I nt, Sync sync)
{
    // first 1-based index of depth d: binary 2^d, quad (4^d - 1)/3 + 1
    auto first = [](int d) -> int64_t { return ARITY == 2 ? ((int64_t)1 << d) : ((((int64_t)1 << (2 * d)) - 1) / 3 + 1); };
    for (int d = L - 1; d >= 0; --d) {
        const int64_t lo = first(d), hi = first(d + 1);
        for (int64_t i = lo + tid; i < hi; i += nt) {
            const T pc = c[i - 1];
            T cc;
            if (ARITY == 2) cc = (T)(c[2 * i - 1] + c[2 * i]);
            else cc = (T)((T)((T)(c[4 * i - 3] + c[4 * i - 2]) + c[4 * i - 1]) + c[4 * i]);
            const bool better = type_max ? (cc > pc) : (cc < pc);
            if (better) c[i - 1] = cc;
            flag[i - 1] = better ? 0 : 1;
        }
        sync();
    }
    // top down, in place: flag[] of shallower depths already holds the tree bit
    for (int d = 0; d < L; ++d) {
        const int64_t lo = first(d), hi = first(d + 1);
        for (int64_t i = lo + tid; i < hi; i += nt) {
            bool keep = !flag[i - 1];
            if (i > 1) {
                const int64_t par = ARITY == 2 ? (i >> 1) : ((i + 2) >> 2);
                keep = keep && flag[par - 1];
            }
            flag[i - 1] = keep ? 1 : 0;
        }
        sync();
    }
}

}  // namespace
