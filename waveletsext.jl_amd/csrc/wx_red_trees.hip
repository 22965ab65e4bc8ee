// wx_red_trees.hip -- iswpdall / iacwpdall with ONE tree per signal: back from a redundant packet table (swpdall, acwpdall) along the
// basis bestbasistreeall(X, BB(redundant = true)) (BestBasis.jl:253-262) chose for each signal.  The reference takes one BitVector for
// the whole batch (swt/swt_all.jl:343-392, acwt/acwt_all.jl:300-333); the (ntree, batch) convention is that of its getbasiscoefall
// (Utils.jl:199-225), as in wx_wpt_trees.hip.
//
// Kernel: a workgroup takes a signal and strides over the batch; the signal's tree bits sit in LDS (the layout of wx_tree_bits.h, reloaded
// for every signal behind a barrier).  A node of a redundant table is a column of n values, so a level of the tree does not fit in LDS, and
// the reference's reverse-heap order (SWT.jl:1079-1093, 1150-1162; ACWT.jl:953-966) needs a copy of the table.  Here the tree is walked
// depth first, post-order: LDS holds two columns per depth 1 .. D -- the finished left child and the right child under construction --
// where D bounds every tree the table admits (2^(D + 1) - 1 <= ncols, D <= log2 n), so the size is known before the trees are read.
//   leaf       loaded once from its column of the table (consecutive lanes, consecutive elements) into the slot of its depth and side;
//              a left leaf whose sibling is a leaf as well brings that neighbouring column along, so that both loads are in flight;
//   node       its two child slots are combined into its own slot;
//   root       its combine writes x; a root that is a leaf copies column 1.
// The walk's state is the heap index of the current node and its depth: the bits of the index ARE the stack (at most log2 n entries), and
// they come from tree words every lane reads alike, passed through readfirstlane, so the state is scalar and every barrier sits in uniform
// control flow.  A barrier stands before every combine (its children are complete, and the slot it writes has been read) and before a
// leaf load that follows a combine.  No scratch memory, no atomics: every leaf element is read from HBM once, every element of x is written
// once, by one lane.
// Combines (rt_combine, wx_red_combine.h), one lane per parent position p, d = the parent's depth, s = 2^d, u = p >> d, np = n >> d:
//   SWT average (sm < 0)   isdwt_step!(v, w1, w2, d, h, g), swt/swt_one_level.jl:257-277: the reconstruction from the children's class
//                          p mod s (t0 = u + 1 mod np) plus the one from the class shifted by s (t0 = u), halved; either sum runs over the
//                          taps in the reference's order (:305-316, with `m-1<<d` read as m - (1 << d)), in Float64 with fma, the child
//                          indices wrapped by true modulo, so nodes shorter than the filter need no periodised taps -- the arithmetic
//                          of k_swt_inv_level (wx_swt1d.hip);
//   SWT shift (sm >= 0)    isdwt_step!(v, w1, w2, d, sv, sw, h, g), :279-318, sv = sm mod 2^d and sw = sm mod 2^(d + 1): main2depthshift
//                          (Utils.jl:297-305) on the TABLE's depth getdepth(ncols, :binary), as SWT.jl:1075-1076 -- which only enters
//                          through the assertion sm < 2^depth.  Only the positions p = sv (mod s) are produced, and only those are read
//                          further up.  A slot written by a combine holds ZERO at every other position (a leaf's slot holds the whole
//                          column); at the root s = 1 and every position is produced, so nothing but results reaches x;
//   ACWT                   v = (w1 + w2) / sqrt(2) per node, acwt/acwt_one_level.jl:217-224, rounded node by node like the reference.
// Window: n dyadic and >= 8, SWT with even filters of 2 .. 20 taps, and  WX_MAXF doubles + 2 D n sizeof(T) + the tree's words <= 136 KiB
// (of 160): Float64 takes every depth up to n = 512 and depth 8 at n = 1024 (depth 9 needs 144 KiB).  Outside it the driver runs the
// single-tree entry once per signal; byte-identical columns go to the single-tree entry whole (wx_trees_host.h).
#include "wx_kernels.h"
#include "wx_red_combine.h"                     // RT_AVG, RT_SHIFT, RT_AC, rt_combine
#include "wx_trees_host.h"

namespace {

// xw: (n, ncols, batch); x: (n, batch); trees: wt_words(n) words of tree bits per signal.  dmax: the deepest tree the table admits (the
// slots of LDS).  LDS: WX_MAXF doubles | 2 dmax columns of n elements | the tree's words.
template <typename T, int KIND>
__global__ __launch_bounds__(1024) void k_red_trees(const T *__restrict__ xw, T *__restrict__ x, int log2n, int64_t ncols, int dmax, int sm,
                                                    int64_t batch, const uint32_t *__restrict__ trees, WxFilt filt)
{
    extern __shared__ __attribute__((aligned(16))) char rt_smem[];
    const int n = 1 << log2n, ntree = n - 1;
    double *qs = reinterpret_cast<double *>(rt_smem);
    T *slots = reinterpret_cast<T *>(qs + WX_MAXF);                    // child c of a node of depth d - 1: slots + (2 (d - 1) + c) n
    uint32_t *tree = reinterpret_cast<uint32_t *>(slots + (size_t)2 * dmax * n);
    const int nw = wt_words(n);
    const int tid = threadIdx.x, NT = blockDim.x, F = filt.F;
    if (KIND != RT_AC && tid == 0)
        for (int i = 0; i < F; ++i) qs[i] = filt.q[i];                 // read below as LDS broadcasts

    for (int64_t b = blockIdx.x; b < batch; b += gridDim.x) {
        const uint32_t *tg = trees + b * (int64_t)nw;
        __syncthreads();                                               // the previous signal's walk is done with the tree
        for (int i = tid; i < nw; i += NT) tree[i] = tg[i];
        __syncthreads();
        const T *cols = xw + b * ncols * n;
        T *xs = x + b * (int64_t)n;
        int node = 1, depth = 0;                                       // scalar: the same for every lane
        bool read = false;                                             // a combine has read its slots since the last barrier
        while (true) {
            // depth < dmax holds for every tree that passed the check; it keeps the slots inside LDS whatever the words hold
            const bool kids = node <= ntree && depth < dmax &&
                              ((__builtin_amdgcn_readfirstlane(tree[(node - 1) >> 5]) >> ((node - 1) & 31)) & 1u);
            if (kids) { node = 2 * node; ++depth; continue; }
            const T *src = cols + (int64_t)(node - 1) * n;             // a leaf: heap index node, column node - 1
            if (node == 1) {                                           // the root is a leaf
                for (int i = tid; i < n; i += NT) xs[i] = src[i];
                break;
            }
            if (read) { __syncthreads(); read = false; }
            T *slot = slots + (size_t)(2 * (depth - 1) + (node & 1)) * n;
            // a left leaf whose sibling is a leaf too (every deepest node has such a pair): the next column with it, both loads in flight
            const bool pair = !(node & 1) && !(node + 1 <= ntree && depth < dmax &&
                                                ((__builtin_amdgcn_readfirstlane(tree[node >> 5]) >> (node & 31)) & 1u));
            if (pair) {
                for (int i = tid; i < n; i += NT) {
                    const T a = src[i], c = src[i + n];
                    slot[i] = a;
                    slot[i + n] = c;
                }
                ++node;
            } else {
                for (int i = tid; i < n; i += NT) slot[i] = src[i];
            }
            while (node > 1 && (node & 1)) {                           // a right child is complete: its parent's combine
                __syncthreads();
                node >>= 1;
                --depth;
                const int d = depth;
                const T *w1 = slots + (size_t)(2 * d) * n, *w2 = w1 + n;
                T *out = node == 1 ? xs : slots + (size_t)(2 * (d - 1) + (node & 1)) * n;
                rt_combine<T, KIND>(w1, w2, out, n, d, sm, F, qs, tid, NT);
                read = true;
            }
            if (node == 1) break;
            ++node;                                                    // a left child is complete: on to its sibling
        }
    }
}

// what the driver (wx_trees_host.h) needs to know of a redundant packet table of ncols columns of n samples
struct RtShape {
    int64_t n, ncols, sm;                                              // sm < 0: average based
    bool ac, has_filter;                                               // the ACWT entry has no filter
    static constexpr bool quad = false;
    static constexpr bool extras = true;                               // sm and ncols travel with the shape; the ACWT has no filter
    static constexpr bool table = true;                                // the input item is the table; its depth bounds the trees
    bool dims_ok() const { return n >= 1 && ncols >= 1; }
    int64_t count() const { return n; }
    int64_t in_count() const { return n * ncols; }
    // the deepest tree the table holds: 2^(D + 1) - 1 <= ncols (api_swt_inv, api_iac: wx_api_swt.hip), never deeper than a valid tree
    int dmax() const
    {
        int D = 0;
        while (D < 30 && ((int64_t)1 << (D + 2)) - 1 <= ncols && ((int64_t)2 << D) <= n) ++D;
        return D;
    }
    int tree_k() const { return dmax() + 1; }                          // a column of depth >= this reaches below the table
    int too_deep() const { return wx_set_error(WX_EBOUNDS, "tree reaches below the last column of xw"); }
    int check(bool, int, int64_t ntree) const
    {
        WX_REQUIRE(ac || has_filter, WX_EARG, "iswpdall(trees): NULL filter");
        WX_REQUIRE(wx_isdyadic(n), WX_EASSERT, "maketree/isvalidtree: signal length must be dyadic (Wavelets.jl)");
        WX_REQUIRE(ntree == n - 1, WX_EASSERT, "@assert n_t == gettreelength(sz...) (Utils.jl:211)");
        // SWT.jl:1074-1075: L = getdepth(m, :binary), main2depthshift(sm, L)
        if (!ac && sm >= 0) WX_REQUIRE(sm < ((int64_t)1 << wx_getdepth_binary(ncols)), WX_EASSERT, "main2depthshift: @assert sm < 1<<L (Utils.jl:298)");
        WX_REQUIRE(n < ((int64_t)1 << 30) && ncols < ((int64_t)1 << 31), WX_EUNSUPPORTED, "iswpdall(trees): table too large");
        return WX_OK;
    }
    int check_host(const uint8_t *trees, int64_t ntree, int64_t batch, int k, uint32_t *bits, int nw, uint8_t *depths, bool *same) const
    { return wx_trees_check_host(false, n, 1, trees, ntree, batch, k, -1, bits, nw, depths, same); }
    // WX_MAXF doubles | two columns per depth | the tree's words
    template <typename T> size_t lds() const { return sizeof(double) * WX_MAXF + (size_t)2 * dmax() * n * sizeof(T) + sizeof(uint32_t) * wt_words(n); }
    template <typename T> bool window(int64_t, int F) const
    { return wx_isdyadic(n) && n >= 8 && (ac || (F >= 2 && F <= 20 && F % 2 == 0)) && n <= ((int64_t)1 << 20) && lds<T>() <= 136 * 1024; }
    RtShape at(int64_t) const { return *this; }
    bool stage(WxIO &, int64_t) const { return true; }
    int single(int, const double *xw, double *x, int, const uint8_t *t, int64_t nt, int64_t batch, const double *qmf, int F, void *st) const
    {
        if (ac) return wx_iacwpd1d_f64(xw, x, n, ncols, 0, t, nt, batch, st);
        return wx_iswpd1d_f64(xw, x, n, ncols, 0, t, nt, sm, batch, qmf, F, st);
    }
    int single(int, const float *xw, float *x, int, const uint8_t *t, int64_t nt, int64_t batch, const double *qmf, int F, void *st) const
    {
        if (ac) return wx_set_error(WX_EUNSUPPORTED, "the autocorrelation transforms are Float64 only");
        return wx_iswpd1d_f32(xw, x, n, ncols, 0, t, nt, sm, batch, qmf, F, st);
    }
    template <typename T, int KIND>
    hipError_t launch_kind(const T *dx, T *dy, int64_t batch, const uint32_t *dt, const WxFilt &filt, hipStream_t st) const
    {
        const size_t bytes = lds<T>();
        const int nt = wx_trees_threads(2 * n);                        // one lane per parent position, not per pair
        auto kern = k_red_trees<T, KIND>;
        hipError_t e = hipSuccess;
        if (bytes > 48 * 1024) e = hipFuncSetAttribute(reinterpret_cast<const void *>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes);
        if (e != hipSuccess) return e;
        int log2n = 0;
        while (((int64_t)1 << log2n) < n) ++log2n;
        hipLaunchKernelGGL(kern, dim3(wx_trees_grid(bytes, nt, batch)), dim3(nt), bytes, st, dx, dy, log2n, ncols, dmax(), (int)(sm < 0 ? 0 : sm),
                           batch, dt, filt);
        return hipGetLastError();
    }
    template <typename T, int MODE>
    hipError_t launch(const T *dx, T *dy, int64_t, int, int64_t batch, const uint32_t *dt, const uint8_t *, const WxFilt &filt, hipStream_t st) const
    {
        if constexpr (sizeof(T) == 8)
            if (ac) return launch_kind<T, RT_AC>(dx, dy, batch, dt, filt, st);
        if (sm >= 0) return launch_kind<T, RT_SHIFT>(dx, dy, batch, dt, filt, st);
        return launch_kind<T, RT_AVG>(dx, dy, batch, dt, filt, st);
    }
};

}  // namespace

extern "C" {

int wx_iswpd1d_trees_f64(const double *xw, double *x, int64_t n, int64_t ncols, const uint8_t *trees, int64_t ntree, int64_t sm, int64_t batch,
                         const double *qmf, int F, void *stream)
{ return wx_trees_api<double, WX_TREES_INV>(RtShape{n, ncols, sm, false, qmf != nullptr}, xw, x, 1, trees, ntree, batch, qmf, F, stream); }
int wx_iswpd1d_trees_f32(const float *xw, float *x, int64_t n, int64_t ncols, const uint8_t *trees, int64_t ntree, int64_t sm, int64_t batch,
                         const double *qmf, int F, void *stream)
{ return wx_trees_api<float, WX_TREES_INV>(RtShape{n, ncols, sm, false, qmf != nullptr}, xw, x, 1, trees, ntree, batch, qmf, F, stream); }
int wx_iacwpd1d_trees_f64(const double *xw, double *x, int64_t n, int64_t ncols, const uint8_t *trees, int64_t ntree, int64_t batch, void *stream)
{ return wx_trees_api<double, WX_TREES_INV>(RtShape{n, ncols, -1, true, false}, xw, x, 1, trees, ntree, batch, nullptr, 0, stream); }

}  // extern "C"
