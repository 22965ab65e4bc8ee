// wx_wpt_trees.hip -- wptall / iwptall / iwpdall with ONE tree per signal: the transforms that consume what bestbasistreeall(X, BB())
// (BestBasis.jl:253-262) returns.  The reference takes one tree for the whole batch (dwt/dwt_all.jl:152-166, 210-225, 324-342); its
// getbasiscoefall already accepts a BitMatrix of trees (Utils.jl:199-225), and the same (ntree, batch) convention is taken here.
//
// Kernel: a workgroup takes a signal and strides over the batch.  The signal lives in LDS (two buffers, a level reads one and writes
// the other; the forward kernel keeps every node's even samples before its odd ones, the inverse keeps natural order: either way
// the taps of neighbouring lanes are neighbours in LDS).  The signal's own tree sits next to it and is reloaded for every signal --
// behind a barrier, so that the previous signal's last level has finished reading it (k_gather_trees1d, wx_gathertrees.hip).  An
// item is one output pair of a level:
//   forward   a decomposed node is transformed into the other buffer (dwt_step!, dwt/dwt_one_level.jl:79-107, true modulo wrap, so
//             nodes shorter than the filter need no periodised taps); a leaf -- a node that is not decomposed under a decomposed
//             parent -- leaves for HBM at once, at its own range, which is where Wavelets.jl's wpt puts it and where the packet table
//             has it; the regions below a leaf are not touched again.  The levels run to the tree's own depth.
//   inverse   the mirror, bottom-up from the tree's own depth (idwt_step!, dwt/dwt_one_level.jl:192-223); the coefficients are staged
//             into both buffers, so a leaf is found in whichever buffer its sibling was rebuilt into; the root's pass writes HBM.
//   iwpd      the inverse kernel whose loads take every position from the column of its leaf's depth in the packet table
//             (getbasiscoef, Utils.jl:101-134).
// The kernel gets the trees as bits, n / 8 bytes per signal instead of n - 1, and one depth byte per signal.
// The filter length is a loop bound: six kernels in all (3 directions x 2 types), the arithmetic is Float64 for either type like the
// one-level kernels of wx_dwt1d.hip.  No atomics; every output element is written by exactly one lane.
// Window: what wx_fused1d_ok admits (dyadic 8 <= n <= 8192 Float64 / 16384 Float32, even filters of 2 .. 20 taps).
// This file holds the kernel and WtShape, what the host driver needs to know of a signal; the driver itself -- argument checks, the
// check and packing of the trees on the host or the device, the routes around the window, staging and waits -- is wx_trees_host.h.
#include "wx_kernels.h"
#include "wx_trees_host.h"

namespace {

enum { WT_FWD = WX_TREES_FWD, WT_INV = WX_TREES_INV, WT_IWPD = WX_TREES_IWPD };

// the tree of a signal as bits: wt_words, wt_set (wx_tree_bits.h)

// depth of the leaf that owns position p (binary heap: children 2i, 2i + 1; utils_tree.jl:57-75)
__device__ __forceinline__ int wt_leaf_depth(const uint32_t *tree, int ntree, int p, int log2n)
{
    int node = 1, d = 0;
    while (node <= ntree && wt_set(tree, node)) {
        node = 2 * node + ((p >> (log2n - 1 - d)) & 1);
        ++d;
    }
    return d;
}

// x: (n, batch) for wpt / iwpt, (n, k, batch) for iwpd; y: (n, batch); trees: wt_words(n) words of tree bits per signal; depths: batch
// bytes, the depth of each tree (0 = the root is a leaf).  LDS: WX_MAXF doubles | two buffers of n elements | the tree's words.
template <typename T, int MODE>
__global__ __launch_bounds__(1024) void k_wpt_trees(const T *__restrict__ x, T *__restrict__ y, int log2n, int k, int64_t batch,
                                                    const uint32_t *__restrict__ trees, const uint8_t *__restrict__ depths, WxFilt filt)
{
    extern __shared__ __attribute__((aligned(16))) char wt_smem[];
    typedef typename WxVec2<T>::type V2;
    const int n = 1 << log2n, ntree = n - 1, half = n >> 1;
    double *qs = reinterpret_cast<double *>(wt_smem);
    T *buf0 = reinterpret_cast<T *>(qs + WX_MAXF);
    T *buf1 = buf0 + n;
    uint32_t *tree = reinterpret_cast<uint32_t *>(buf1 + n);
    const int nw = wt_words(n);
    const int tid = threadIdx.x, NT = blockDim.x, F = filt.F;
    if (tid == 0)
        for (int i = 0; i < F; ++i) qs[i] = filt.q[i];                 // read below as LDS broadcasts
    const int64_t in_stride = MODE == WT_IWPD ? (int64_t)k * n : (int64_t)n;

    for (int64_t b = blockIdx.x; b < batch; b += gridDim.x) {
        const uint32_t *tg = trees + b * (int64_t)nw;
        __syncthreads();                                               // the previous signal's last level is done with tree and buffers
        for (int i = tid; i < nw; i += NT) tree[i] = tg[i];
        const int depth = depths[b];
        const T *xs = x + b * in_stride;
        T *ys = y + b * (int64_t)n;
        if (MODE == WT_IWPD) __syncthreads();                          // the loads walk the tree
        for (int i = tid; i < half; i += NT) {
            const int p = 2 * i;
            const T *src = xs + p;
            if (MODE == WT_IWPD) src += (int64_t)wt_leaf_depth(tree, ntree, p, log2n) * n;   // both samples of a pair share their leaf's depth
            const V2 v = *reinterpret_cast<const V2 *>(src);
            if (depth == 0) *reinterpret_cast<V2 *>(ys + p) = v;       // the root is a leaf: copy
            else if (MODE == WT_FWD) { buf0[i] = v.x; buf0[half + i] = v.y; }   // even samples first, see below
            else {
                *reinterpret_cast<V2 *>(buf0 + p) = v;
                *reinterpret_cast<V2 *>(buf1 + p) = v;
            }
        }
        __syncthreads();
        if (depth == 0) continue;
        T *cur = buf0, *nxt = buf1;
        if (MODE == WT_FWD) {
            // A node of the forward buffers is stored even samples first: sample s of a node of `len` samples at base sits at
            // base + (s & 1) * len / 2 + s / 2, so the taps of neighbouring lanes (2 t + u) are neighbours in LDS.
            // Level `depth` decomposes nothing: it only sends off the leaves of the deepest level.
            for (int d = 0; d <= depth; ++d) {
                const int lsh = log2n - d;                             // log2 of the node length
                for (int i = tid; i < half; i += NT) {
                    const int p = 2 * i, j = p >> lsh, node = (1 << d) + j;
                    const int h = (1 << lsh) >> 1, base = j << lsh, t = i - (base >> 1), msk = h - 1;
                    if (node <= ntree && wt_set(tree, node)) {
                        const T *v = cur + base;
                        double a = 0.0, dd = 0.0;
                        for (int u = 0; u < F; ++u) {                  // a: v[(2t + u) mod np], d: v[(2t + 1 - u) mod np]
                            const double q = qs[u];
                            const int par = (u & 1) * h;
                            a = fma(q, (double)v[par + ((t + (u >> 1)) & msk)], a);
                            dd = fma((u & 1) ? -q : q, (double)v[(h - par) + ((t - (u >> 1)) & msk)], dd);
                        }
                        T *o = nxt + base + (t & 1) * (h >> 1) + (t >> 1);
                        o[0] = (T)a;
                        o[h] = (T)dd;
                    } else if (d > 0 && wt_set(tree, node >> 1)) {       // the parent (node >> 1 <= ntree) was decomposed: a leaf
                        V2 o;                                          // samples p, p + 1; nodes of one sample (lsh == 0) lie side by side
                        o.x = cur[base + t];
                        o.y = cur[base + t + (lsh ? h : 1)];
                        *reinterpret_cast<V2 *>(ys + p) = o;
                    }
                }
                __syncthreads();
                T *tmp = cur; cur = nxt; nxt = tmp;
            }
        } else {
            for (int d = depth - 1; d >= 0; --d) {
                const int lsh = log2n - d;
                T *out = d == 0 ? ys : nxt;
                for (int i = tid; i < half; i += NT) {
                    const int p = 2 * i, j = p >> lsh, node = (1 << d) + j;   // node < 2^depth <= n, i.e. node <= ntree
                    if (wt_set(tree, node)) {
                        const int np = 1 << lsh, h = np >> 1, base = j << lsh, t = i - (base >> 1), msk = h - 1;
                        const T *a = cur + base, *dv = a + h;
                        double v0 = 0.0, v1 = 0.0;
                        for (int m = 0; m < F / 2; ++m) {
                            const double q0 = qs[2 * m], q1 = qs[2 * m + 1];
                            const double av = (double)a[(t - m) & msk], dw = (double)dv[(t + m) & msk];
                            v0 = fma(q0, av, v0);
                            v0 = fma(-q1, dw, v0);
                            v1 = fma(q1, av, v1);
                            v1 = fma(q0, dw, v1);
                        }
                        V2 o; o.x = (T)v0; o.y = (T)v1;
                        *reinterpret_cast<V2 *>(out + base + 2 * t) = o;
                    }
                }
                __syncthreads();
                T *tmp = cur; cur = nxt; nxt = tmp;
            }
        }
    }
}

// what the driver (wx_trees_host.h) needs to know of a signal of n samples
struct WtShape {
    int64_t n;
    static constexpr bool quad = false;
    bool dims_ok() const { return n >= 1; }
    int64_t count() const { return n; }
    int check(bool iwpd, int k, int64_t ntree) const
    {
        WX_REQUIRE(wx_isdyadic(n), WX_EASSERT, "maketree/isvalidtree: signal length must be dyadic (Wavelets.jl)");
        if (iwpd) WX_REQUIRE(k - 1 <= wx_maxtransformlevels(n), WX_EASSERT, "getbasiscoef: @assert k-1 <= L (Utils.jl:110)");
        WX_REQUIRE(ntree == n - 1, WX_EASSERT, "@assert n_t == gettreelength(sz...) (Utils.jl:211)");
        WX_REQUIRE(n < ((int64_t)1 << 30), WX_EUNSUPPORTED, "wptall(trees): signal length >= 2^30 not supported");
        return WX_OK;
    }
    int check_host(const uint8_t *trees, int64_t ntree, int64_t batch, int k, uint32_t *bits, int nw, uint8_t *depths, bool *same) const
    { return wx_trees_check_host(false, n, 1, trees, ntree, batch, k, -1, bits, nw, depths, same); }
    // WX_MAXF doubles | two buffers of n elements | the tree's words: wt_words(n), which is wq_words(n - 1) for every dyadic n
    template <typename T> size_t lds() const { return sizeof(double) * WX_MAXF + (size_t)2 * n * sizeof(T) + sizeof(uint32_t) * wt_words(n); }
    template <typename T> bool window(int64_t, int F) const { return wx_fused1d_ok<T>(n, F) && lds<T>() <= 160 * 1024; }
    int single(int mode, const double *x, double *y, int k, const uint8_t *t, int64_t nt, int64_t batch, const double *qmf, int F, void *st) const
    {
        if (mode == WT_FWD) return wx_wpt1d_f64(x, y, n, 0, t, nt, batch, qmf, F, st);
        if (mode == WT_INV) return wx_iwpt1d_f64(x, y, n, 0, t, nt, batch, qmf, F, st);
        return wx_iwpd1d_f64(x, y, n, k, 0, t, nt, batch, qmf, F, st);
    }
    int single(int mode, const float *x, float *y, int k, const uint8_t *t, int64_t nt, int64_t batch, const double *qmf, int F, void *st) const
    {
        if (mode == WT_FWD) return wx_wpt1d_f32(x, y, n, 0, t, nt, batch, qmf, F, st);
        if (mode == WT_INV) return wx_iwpt1d_f32(x, y, n, 0, t, nt, batch, qmf, F, st);
        return wx_iwpd1d_f32(x, y, n, k, 0, t, nt, batch, qmf, F, st);
    }
    template <typename T, int MODE>
    hipError_t launch(const T *dx, T *dy, int64_t, int k, int64_t batch, const uint32_t *dt, const uint8_t *dd, const WxFilt &filt,
                      hipStream_t st) const
    {
        const size_t bytes = lds<T>();
        const int nt = wx_trees_threads(n);
        auto kern = k_wpt_trees<T, MODE>;
        hipError_t e = hipSuccess;
        if (bytes > 64 * 1024) e = hipFuncSetAttribute(reinterpret_cast<const void *>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes);
        if (e != hipSuccess) return e;
        int log2n = 0;
        while (((int64_t)1 << log2n) < n) ++log2n;
        hipLaunchKernelGGL(kern, dim3(wx_trees_grid(bytes, nt, batch)), dim3(nt), bytes, st, dx, dy, log2n, k, batch, dt, dd, filt);
        return hipGetLastError();
    }
};

}  // namespace

extern "C" {

int wx_wpt1d_trees_f64(const double *x, double *y, int64_t n, const uint8_t *trees, int64_t ntree, int64_t batch, const double *qmf, int F,
                       void *stream)
{ return wx_trees_api<double, WT_FWD>(WtShape{n}, x, y, 1, trees, ntree, batch, qmf, F, stream); }
int wx_wpt1d_trees_f32(const float *x, float *y, int64_t n, const uint8_t *trees, int64_t ntree, int64_t batch, const double *qmf, int F,
                       void *stream)
{ return wx_trees_api<float, WT_FWD>(WtShape{n}, x, y, 1, trees, ntree, batch, qmf, F, stream); }
int wx_iwpt1d_trees_f64(const double *xw, double *xhat, int64_t n, const uint8_t *trees, int64_t ntree, int64_t batch, const double *qmf,
                        int F, void *stream)
{ return wx_trees_api<double, WT_INV>(WtShape{n}, xw, xhat, 1, trees, ntree, batch, qmf, F, stream); }
int wx_iwpt1d_trees_f32(const float *xw, float *xhat, int64_t n, const uint8_t *trees, int64_t ntree, int64_t batch, const double *qmf,
                        int F, void *stream)
{ return wx_trees_api<float, WT_INV>(WtShape{n}, xw, xhat, 1, trees, ntree, batch, qmf, F, stream); }
int wx_iwpd1d_trees_f64(const double *xw, double *xhat, int64_t n, int k, const uint8_t *trees, int64_t ntree, int64_t batch,
                        const double *qmf, int F, void *stream)
{ return wx_trees_api<double, WT_IWPD>(WtShape{n}, xw, xhat, k, trees, ntree, batch, qmf, F, stream); }
int wx_iwpd1d_trees_f32(const float *xw, float *xhat, int64_t n, int k, const uint8_t *trees, int64_t ntree, int64_t batch,
                        const double *qmf, int F, void *stream)
{ return wx_trees_api<float, WT_IWPD>(WtShape{n}, xw, xhat, k, trees, ntree, batch, qmf, F, stream); }

}  // extern "C"
