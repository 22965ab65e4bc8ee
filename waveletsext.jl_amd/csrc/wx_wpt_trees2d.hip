// wx_wpt_trees2d.hip -- wptall / iwptall / iwpdall of IMAGES with ONE quad tree per image: the 2-D sibling of wx_wpt_trees.hip and the
// consumer of what bestbasistreeall(X, BB()) returns for an (m, n, k, N) packet table.  The reference loops wpt! / iwpt! / iwpd!
// (DWT.jl:500-548, 662-710, 340-401) over the batch with one tree (dwt/dwt_all.jl:152-166, 210-225, 324-342); its getbasiscoefall
// already accepts a BitMatrix of quad trees (Utils.jl:199-225), and the same (ntree, batch) convention is taken here.
//
// Kernel: a workgroup takes an image and strides over the batch.  The image lives in LDS in two buffers, column-major like the
// caller's; the image's own tree sits next to it as bits and is reloaded for every image behind a barrier.  A level of a decomposed
// node is dwt_step! (dwt/dwt_one_level.jl:319-354): all columns `cur -> nxt`, then all rows `nxt -> cur`, the intermediate rounded to
// T as the reference's `temp` is.  An item is one output pair of a pass, and neighbouring lanes run along dimension 1 in both passes:
//   column pass  the taps 2 t + u of neighbouring lanes would be two elements apart, so `cur` keeps the ROWS of every node even rows
//                first (row s of a node of mm rows at s / 2 + (s & 1) mm / 2, the layout of k_wpt_trees along dimension 1): the
//                taps of neighbouring lanes are neighbours in LDS.  `nxt` is in natural order.
//   row pass     the taps are whole columns apart (stride m) and neighbouring lanes neighbouring rows: conflict-free as it is.  It
//                writes the four children into `cur`, each with its own rows even first.
//   forward      a leaf -- a node that is not decomposed under a decomposed parent -- leaves `cur` for HBM the moment it appears, at
//                its own rectangle (where wpt! puts it and where the packet table has it); nothing below it is touched again.  The
//                levels run to the tree's own depth.
//   inverse      the mirror, bottom-up (idwt_step!, dwt_one_level.jl:401-436: rows `cur -> nxt`, columns `nxt -> cur`), everything
//                in natural order (the taps t - j, t + j of neighbouring lanes are neighbours); a level ends in `cur`, where its
//                siblings' leaves were staged, and the root's column pass writes HBM.
//   iwpd         the inverse kernel whose loads take every position from the slice of its leaf's depth (getbasiscoef, Utils.jl:101-134).
// True modulo wrap (the sides are powers of two), so nodes shorter than the filter need no periodised taps.  The filter length is a
// loop bound, two taps per turn, the taps scalar loads from the kernel arguments (no LDS traffic for them): six kernels in all
// (3 directions x 2 types); the arithmetic is Float64 for either type.  No atomics; every output
// element is written by exactly one lane.
// The kernel gets the trees as bits (wx_tree_bits.h: node i is bit i - 1, heap order) and one depth byte per image.
// Window: both sides dyadic and >= 8, m n <= 8192 (Float64) / 16384 (Float32) -- two buffers and the tree's bits are at
// most 129 of the 160 KiB --, even filters of 2 .. 20 taps.
// This file holds the kernel and WqShape, what the host driver needs to know of an image; the driver itself is wx_trees_host.h,
// shared with wx_wpt_trees.hip.
#include "wx_trees_host.h"

namespace {

enum { WQ_FWD = WX_TREES_FWD, WQ_INV = WX_TREES_INV, WQ_IWPD = WX_TREES_IWPD };

// the bits of v (< 256) at the even positions
__device__ __forceinline__ int wq_spread(int v)
{
    v = (v | (v << 4)) & 0x0f0f;
    v = (v | (v << 2)) & 0x3333;
    return (v | (v << 1)) & 0x5555;
}
// the node of depth d that holds block (jr, jc) of the 2^d x 2^d blocks: the first node of a depth is (4^d - 1) / 3 + 1, and the
// children 4 i - 2 .. 4 i + 1 of i are (top, left), (top, right), (bottom, left), (bottom, right)
__device__ __forceinline__ int wq_node(int d, int jr, int jc) { return (((1 << (2 * d)) - 1) / 3) + 1 + ((wq_spread(jr) << 1) | wq_spread(jc)); }
__device__ __forceinline__ bool wq_split(const uint32_t *tree, int ntree, int node) { return node <= ntree && wt_set(tree, node); }

// depth of the leaf that owns (r, c) (gt_depth2d of wx_gathertrees.hip on the bits; d < min(lm, ln) inside the loop)
__device__ __forceinline__ int wq_leaf_depth(const uint32_t *tree, int ntree, int r, int c, int lm, int ln)
{
    int node = 1, d = 0;
    while (wq_split(tree, ntree, node)) {
        node = 4 * node - 2 + 2 * ((r >> (lm - 1 - d)) & 1) + ((c >> (ln - 1 - d)) & 1);
        ++d;
    }
    return d;
}

// x: (m, n, batch) for wpt / iwpt, (m, n, k, batch) for iwpd; y: (m, n, batch); m = 2^lm, n = 2^ln; trees: nw words of tree bits per
// image; depths: batch bytes, the depth of each tree (0 = the root is a leaf; at most min(lm, ln)).
// LDS: two buffers of m n elements | the tree's words.
template <typename T, int MODE>
__global__ __launch_bounds__(1024) void k_wpt_trees2d(const T *__restrict__ x, T *__restrict__ y, int lm, int ln, int ntree, int nw, int k,
                                                      int64_t batch, const uint32_t *__restrict__ trees, const uint8_t *__restrict__ depths,
                                                      WxFilt filt)
{
    extern __shared__ __attribute__((aligned(16))) char wq_smem[];
    typedef typename WxVec2<T>::type V2;
    const int m = 1 << lm, mn = 1 << (lm + ln), half = mn >> 1;
    T *buf0 = reinterpret_cast<T *>(wq_smem);
    T *buf1 = buf0 + mn;
    uint32_t *tree = reinterpret_cast<uint32_t *>(buf1 + mn);
    const int tid = threadIdx.x, NT = blockDim.x, F = filt.F;             // the taps are read from the kernel arguments: scalar loads
    const int64_t in_stride = MODE == WQ_IWPD ? (int64_t)k * mn : (int64_t)mn;

    for (int64_t b = blockIdx.x; b < batch; b += gridDim.x) {
        const uint32_t *tg = trees + b * (int64_t)nw;
        __syncthreads();                                               // the previous image's last pass is done with tree and buffers
        for (int i = tid; i < nw; i += NT) tree[i] = tg[i];
        const int depth = depths[b];
        const T *xs = x + b * in_stride;
        T *ys = y + b * (int64_t)mn;
        if (MODE == WQ_IWPD) __syncthreads();                          // the loads walk the tree
        T *cur = buf0, *nxt = buf1;
        for (int e = tid; e < mn; e += NT) {
            const int r = e & (m - 1), c = e >> lm;
            const T *src = xs + e;
            if (MODE == WQ_IWPD) src += (int64_t)wq_leaf_depth(tree, ntree, r, c, lm, ln) * mn;
            const T v = *src;
            if (depth == 0) ys[e] = v;                                 // the root is a leaf: copy
            else if (MODE == WQ_FWD) cur[(c << lm) + (r & 1) * (m >> 1) + (r >> 1)] = v;   // the root's rows, even rows first
            else cur[e] = v;
        }
        __syncthreads();
        if (depth == 0) continue;
        if (MODE == WQ_FWD) {
            // Level `depth` decomposes nothing: it only sends off the leaves of the deepest level.
            for (int d = 0; d <= depth; ++d) {
                const int lmd = lm - d, lnd = ln - d;                  // log2 of a node's sides
                if (d < depth) {                                       // all columns of the decomposed nodes: cur -> nxt
                    const int hm = (1 << lmd) >> 1, msk = hm - 1;
                    for (int i = tid; i < half; i += NT) {
                        const int ri = i & ((m >> 1) - 1), c = i >> (lm - 1), jr = (2 * ri) >> lmd;
                        if (!wq_split(tree, ntree, wq_node(d, jr, c >> lnd))) continue;
                        const int rbase = jr << lmd, t = ri - (rbase >> 1);
                        const T *v = cur + (c << lm) + rbase;
                        double a = 0.0, dd = 0.0;
                        for (int j = 0; j < F / 2; ++j) {              // a: v[(2t + u) mod mm], d: v[(2t + 1 - u) mod mm], u = 2j, 2j + 1
                            const double q0 = filt.q[2 * j], q1 = filt.q[2 * j + 1];
                            const int up = (t + j) & msk, dn = (t - j) & msk;
                            const double e0 = (double)v[up], o0 = (double)v[hm + up], e1 = (double)v[dn], o1 = (double)v[hm + dn];
                            a = fma(q0, e0, a);
                            dd = fma(q0, o1, dd);
                            a = fma(q1, o0, a);
                            dd = fma(-q1, e1, dd);
                        }
                        T *o = nxt + (c << lm) + rbase + t;
                        o[0] = (T)a;
                        o[hm] = (T)dd;
                    }
                }
                if (d > 0) {                                           // the leaves of this level: cur -> HBM
                    const int mm = 1 << lmd;
                    for (int e = tid; e < mn; e += NT) {
                        const int r = e & (m - 1), c = e >> lm, jr = r >> lmd;
                        const int node = wq_node(d, jr, c >> lnd);
                        if (wq_split(tree, ntree, node) || !wt_set(tree, (node + 2) >> 2)) continue;   // the parent is a node of the tree
                        const int s = r - (jr << lmd);
                        ys[e] = cur[(c << lm) + (jr << lmd) + (s & 1) * (mm >> 1) + (s >> 1)];
                    }
                }
                if (d == depth) break;                                 // (the next image starts behind a barrier)
                __syncthreads();
                {                                                      // all rows of the decomposed nodes: nxt -> cur
                    const int hn = (1 << lnd) >> 1, mskn = (1 << lnd) - 1, hm = (1 << lmd) >> 1;
                    for (int i = tid; i < half; i += NT) {
                        const int r = i & (m - 1), ci = i >> lm, jr = r >> lmd, jc = (2 * ci) >> lnd;
                        if (!wq_split(tree, ntree, wq_node(d, jr, jc))) continue;
                        const int cbase = jc << lnd, t = ci - (cbase >> 1);
                        const T *v = nxt + r + (cbase << lm);
                        double a = 0.0, dd = 0.0;
                        for (int j = 0; j < F / 2; ++j) {
                            const double q0 = filt.q[2 * j], q1 = filt.q[2 * j + 1];
                            const int up = 2 * (t + j), dn = 2 * (t - j);
                            const double e0 = (double)v[(up & mskn) << lm], o0 = (double)v[((up + 1) & mskn) << lm];
                            const double e1 = (double)v[(dn & mskn) << lm], o1 = (double)v[((dn + 1) & mskn) << lm];
                            a = fma(q0, e0, a);
                            dd = fma(q0, o1, dd);
                            a = fma(q1, o0, a);
                            dd = fma(-q1, e1, dd);
                        }
                        // row r of the node is row s2 of its upper or lower children, whose rows are kept even rows first
                        const int s = r - (jr << lmd), hi = s >= hm ? hm : 0, s2 = s - hi;
                        T *o = cur + (jr << lmd) + hi + (s2 & 1) * (hm >> 1) + (s2 >> 1) + ((cbase + t) << lm);
                        o[0] = (T)a;
                        o[hn << lm] = (T)dd;
                    }
                }
                __syncthreads();
            }
        } else {
            for (int d = depth - 1; d >= 0; --d) {
                const int lmd = lm - d, lnd = ln - d;
                {                                                      // all rows of the decomposed nodes: cur -> nxt
                    const int hn = (1 << lnd) >> 1, mskn = hn - 1;
                    for (int i = tid; i < half; i += NT) {
                        const int r = i & (m - 1), ci = i >> lm, jr = r >> lmd, jc = (2 * ci) >> lnd;
                        if (!wq_split(tree, ntree, wq_node(d, jr, jc))) continue;
                        const int cbase = jc << lnd, t = ci - (cbase >> 1);
                        const T *a = cur + r + (cbase << lm), *dv = a + (hn << lm);
                        double v0 = 0.0, v1 = 0.0;
                        for (int j = 0; j < F / 2; ++j) {
                            const double q0 = filt.q[2 * j], q1 = filt.q[2 * j + 1];
                            const double av = (double)a[((t - j) & mskn) << lm], dw = (double)dv[((t + j) & mskn) << lm];
                            v0 = fma(q0, av, v0);
                            v0 = fma(-q1, dw, v0);
                            v1 = fma(q1, av, v1);
                            v1 = fma(q0, dw, v1);
                        }
                        T *o = nxt + r + ((cbase + 2 * t) << lm);
                        o[0] = (T)v0;
                        o[m] = (T)v1;
                    }
                }
                __syncthreads();
                {                                                      // all columns: nxt -> cur, the root's into HBM
                    const int hm = (1 << lmd) >> 1, msk = hm - 1;
                    T *out = d == 0 ? ys : cur;
                    for (int i = tid; i < half; i += NT) {
                        const int ri = i & ((m >> 1) - 1), c = i >> (lm - 1), jr = (2 * ri) >> lmd;
                        if (!wq_split(tree, ntree, wq_node(d, jr, c >> lnd))) continue;
                        const int rbase = jr << lmd, t = ri - (rbase >> 1);
                        const T *a = nxt + (c << lm) + rbase, *dv = a + hm;
                        double v0 = 0.0, v1 = 0.0;
                        for (int j = 0; j < F / 2; ++j) {
                            const double q0 = filt.q[2 * j], q1 = filt.q[2 * j + 1];
                            const double av = (double)a[(t - j) & msk], dw = (double)dv[(t + j) & msk];
                            v0 = fma(q0, av, v0);
                            v0 = fma(-q1, dw, v0);
                            v1 = fma(q1, av, v1);
                            v1 = fma(q0, dw, v1);
                        }
                        V2 o; o.x = (T)v0; o.y = (T)v1;
                        *reinterpret_cast<V2 *>(out + (c << lm) + rbase + 2 * t) = o;
                    }
                }
                __syncthreads();
            }
        }
    }
}

// what the driver (wx_trees_host.h) needs to know of an image of m x n samples
struct WqShape {
    int64_t m, n;
    static constexpr bool quad = true;
    bool dims_ok() const { return m >= 1 && n >= 1; }
    int64_t count() const { return m * n; }
    // with the codes of the 1-D entries, of the single-tree 2-D entries (wx_check_tree2d, wx_api_2d.hip) and of getbasiscoefall
    int check(bool iwpd, int k, int64_t ntree) const
    {
        if (iwpd)
            WX_REQUIRE(k - 1 <= wx_maxtransformlevels(m < n ? m : n), WX_EASSERT, "getbasiscoef: @assert k-1 <= maxtransformlevels(x) (Utils.jl:110)");
        WX_REQUIRE(ntree == wx_gettreelength2d(m, n), WX_EASSERT, "@assert n_t == gettreelength(sz...) (Utils.jl:211)");
        WX_REQUIRE(m < ((int64_t)1 << 20) && n < ((int64_t)1 << 20) && ntree < ((int64_t)1 << 31), WX_EUNSUPPORTED, "wptall(trees): image side >= 2^20");
        return WX_OK;
    }
    // no tree may be deeper than both sides divide by
    int check_host(const uint8_t *trees, int64_t ntree, int64_t batch, int k, uint32_t *bits, int nw, uint8_t *depths, bool *same) const
    {
        const int Lm = wx_maxtransformlevels(m), Ln = wx_maxtransformlevels(n);
        return wx_trees_check_host(true, m, n, trees, ntree, batch, k, Lm < Ln ? Lm : Ln, bits, nw, depths, same);
    }
    // two buffers of m n elements | the tree's words
    template <typename T> size_t lds(int64_t ntree) const { return (size_t)2 * m * n * sizeof(T) + sizeof(uint32_t) * wq_words(ntree); }
    // the window of one launch
    template <typename T> bool window(int64_t ntree, int F) const
    {
        if (!wx_isdyadic(m) || !wx_isdyadic(n) || m < 8 || n < 8) return false;
        if (m * n > (sizeof(T) == 8 ? 8192 : 16384)) return false;
        if (F < 2 || F > 20 || (F & 1)) return false;
        return lds<T>(ntree) <= 160 * 1024;
    }
    int single(int mode, const double *x, double *y, int k, const uint8_t *t, int64_t nt, int64_t batch, const double *qmf, int F, void *st) const
    {
        if (mode == WQ_FWD) return wx_wpt2d_f64(x, y, m, n, 0, t, nt, batch, qmf, F, st);
        if (mode == WQ_INV) return wx_iwpt2d_f64(x, y, m, n, 0, t, nt, batch, qmf, F, st);
        return wx_iwpd2d_f64(x, y, m, n, k, 0, t, nt, batch, qmf, F, st);
    }
    int single(int mode, const float *x, float *y, int k, const uint8_t *t, int64_t nt, int64_t batch, const double *qmf, int F, void *st) const
    {
        if (mode == WQ_FWD) return wx_wpt2d_f32(x, y, m, n, 0, t, nt, batch, qmf, F, st);
        if (mode == WQ_INV) return wx_iwpt2d_f32(x, y, m, n, 0, t, nt, batch, qmf, F, st);
        return wx_iwpd2d_f32(x, y, m, n, k, 0, t, nt, batch, qmf, F, st);
    }
    template <typename T, int MODE>
    hipError_t launch(const T *dx, T *dy, int64_t ntree, int k, int64_t batch, const uint32_t *dt, const uint8_t *dd, const WxFilt &filt,
                      hipStream_t st) const
    {
        const size_t bytes = lds<T>(ntree);
        const int nt = wx_trees_threads(m * n);
        auto kern = k_wpt_trees2d<T, MODE>;
        hipError_t e = hipSuccess;
        if (bytes > 64 * 1024) e = hipFuncSetAttribute(reinterpret_cast<const void *>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes);
        if (e != hipSuccess) return e;
        hipLaunchKernelGGL(kern, dim3(wx_trees_grid(bytes, nt, batch)), dim3(nt), bytes, st, dx, dy, wx_maxtransformlevels(m),
                           wx_maxtransformlevels(n), (int)ntree, wq_words(ntree), k, batch, dt, dd, filt);
        return hipGetLastError();
    }
};

}  // namespace

extern "C" {

int wx_wpt2d_trees_f64(const double *x, double *y, int64_t m, int64_t n, const uint8_t *trees, int64_t ntree, int64_t batch, const double *qmf,
                       int F, void *stream)
{ return wx_trees_api<double, WQ_FWD>(WqShape{m, n}, x, y, 1, trees, ntree, batch, qmf, F, stream); }
int wx_wpt2d_trees_f32(const float *x, float *y, int64_t m, int64_t n, const uint8_t *trees, int64_t ntree, int64_t batch, const double *qmf,
                       int F, void *stream)
{ return wx_trees_api<float, WQ_FWD>(WqShape{m, n}, x, y, 1, trees, ntree, batch, qmf, F, stream); }
int wx_iwpt2d_trees_f64(const double *xw, double *xhat, int64_t m, int64_t n, const uint8_t *trees, int64_t ntree, int64_t batch,
                        const double *qmf, int F, void *stream)
{ return wx_trees_api<double, WQ_INV>(WqShape{m, n}, xw, xhat, 1, trees, ntree, batch, qmf, F, stream); }
int wx_iwpt2d_trees_f32(const float *xw, float *xhat, int64_t m, int64_t n, const uint8_t *trees, int64_t ntree, int64_t batch,
                        const double *qmf, int F, void *stream)
{ return wx_trees_api<float, WQ_INV>(WqShape{m, n}, xw, xhat, 1, trees, ntree, batch, qmf, F, stream); }
int wx_iwpd2d_trees_f64(const double *xw, double *xhat, int64_t m, int64_t n, int k, const uint8_t *trees, int64_t ntree, int64_t batch,
                        const double *qmf, int F, void *stream)
{ return wx_trees_api<double, WQ_IWPD>(WqShape{m, n}, xw, xhat, k, trees, ntree, batch, qmf, F, stream); }
int wx_iwpd2d_trees_f32(const float *xw, float *xhat, int64_t m, int64_t n, int k, const uint8_t *trees, int64_t ntree, int64_t batch,
                        const double *qmf, int F, void *stream)
{ return wx_trees_api<float, WQ_IWPD>(WqShape{m, n}, xw, xhat, k, trees, ntree, batch, qmf, F, stream); }

}  // extern "C"
