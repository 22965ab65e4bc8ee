// wx_denoise_red_trees.hip -- denoise / denoiseall(xw, :swpd | :acwpd, wt; tree, dnt, estnoise, smooth) with ONE tree per signal: every signal
// is denoised from its redundant packet table (swpdall, acwpdall: heap ordered, node i in column i - 1) in the basis
// bestbasistreeall(X, BB(redundant = true)) (BestBasis.jl:253-262) chose for it.  The reference takes a single BitVector here
// (Denoising.jl:544-594, 651-712); the extension follows the (ntree, batch) convention of its getbasiscoefall (Utils.jl:199-225), like
// wx_denoise_trees.hip does for :wpt and wx_red_trees.hip for iswpdall / iacwpdall.
//
// Kernel (k_denoise_red_trees): the depth-first walk of k_red_trees (wx_red_trees.hip) -- a workgroup takes a signal and strides over the
// batch, the signal's tree bits sit in LDS, two columns of LDS per depth, the walk's state is scalar -- with two steps in front of it:
//   nodes      the finest detail node, reached from the root by right children while i <= ntree && T[i] (finestdetailrange, Utils.jl:428-433),
//              and the coarsest scaling node, reached by left children while i < ntree && T[i] (Utils.jl:363-367, with its strict `<`);
//   estimate   sigma = mad(column of the finest detail node) / 0.6745 (noisest, Denoising.jl:228-231) by ONE wavefront of the workgroup: the n
//              values go from HBM straight into n / 64 registers per lane and the two medians are found by counting against pivots with
//              ballots (dn_noisest, wx_select_count.h: exact order statistics, middle(a, b) = a/2 + b/2, the deviations rounded in T, NaN
//              for a NaN among the details or a non-finite median -- the arithmetic of k_mad_count, so the result is wx_noisest_*'s bit for
//              bit).  No barrier inside the selection and no LDS beyond one word for the result: the other wavefronts load the tree and
//              wait at the barrier that publishes it.  n < 64: the lanes beyond n hold +Inf, which the counting never ranks.
// and one change inside it:
//   threshold  every leaf load passes wx_thresh(v, (T)(sigma scale), kind), the rounding of wx_threshold_*, except the coarsest scaling node
//              when undersmoothing.  The detail column is a leaf as well and is read a second time here (the walk goes left child first,
//              and the threshold needs the estimate).
// The combines are those of k_red_trees, kinds RT_AVG (iswpd(x, wt, T), no shift: Denoising.jl:561) and RT_AC (iacwpd(x, T)).  No scratch
// memory, no atomics: every leaf element is read from HBM once for the walk, every element of x is written once, by one lane.
// Window: n dyadic, 8 <= n <= 1024 (16 registers per lane hold the detail column; k_red_trees has no such bound), SWT with even filters
// of 2 .. 20 taps, and  WX_MAXF doubles + 2 D n sizeof(T) + the tree's words + 16 bytes <= 136 KiB (of 160), D the deepest tree the table
// admits: Float64 every depth up to n = 512 and depth 8 at n = 1024.  Outside it the driver (wx_trees_host.h) runs the single-tree pipeline
// -- wx_noisest_*, wx_threshold_* with the leaf mask, wx_iswpd1d_* / wx_iacwpd1d_f64 -- once per signal; byte-identical columns go to it
// whole.
// Without an output only sigma is wanted, and without a filter (:swpd, wt = nothing) the output is the thresholded copy of the table: then
// there is nothing to walk.  k_drt_sigma estimates with one wavefront per signal, four signals per workgroup, no LDS; k_drt_table is the
// elementwise pass with the per-signal leaf masks, a workgroup per column.
#include "wx_kernels.h"
#include "wx_red_combine.h"                     // rt_combine
#include "wx_red_estimate.h"                    // drt_estimate, drt_finest, drt_coarsest, DRT_MAXLOG2N
#include "wx_trees_host.h"

namespace {

enum { DRT_AVG = RT_AVG, DRT_AC = RT_AC };                             // the kinds of k_red_trees this kernel has (wx_red_combine.h)

// xw: (n, ncols, batch); x: (n, batch); trees: wt_words(n) words of tree bits per signal.  dmax: the deepest tree the table admits (the
// slots of LDS).  thr != nullptr: the thresholds before scaling (per_thr: one per signal), no estimate.  sigma (optional): batch values.
// LDS: WX_MAXF doubles | 2 dmax columns of n elements | the tree's words (dynamic), the estimate (static).
template <typename T, int KIND>
__global__ __launch_bounds__(1024) void k_denoise_red_trees(const T *__restrict__ xw, T *__restrict__ x, int log2n, int64_t ncols, int dmax,
                                                            int64_t batch, const uint32_t *__restrict__ trees, WxFilt filt, int th_kind,
                                                            double scale, const T *__restrict__ thr, int per_thr, int undersmooth,
                                                            T *__restrict__ sigma)
{
    extern __shared__ __attribute__((aligned(16))) char drt_smem[];
    __shared__ T sg_sh;
    const int n = 1 << log2n, ntree = n - 1;
    double *qs = reinterpret_cast<double *>(drt_smem);
    T *slots = reinterpret_cast<T *>(qs + WX_MAXF);                    // child c of a node of depth d - 1: slots + (2 (d - 1) + c) n
    uint32_t *tree = reinterpret_cast<uint32_t *>(slots + (size_t)2 * dmax * n);
    const int nw = wt_words(n);
    const int tid = threadIdx.x, NT = blockDim.x, F = filt.F;
    if (KIND != DRT_AC && tid == 0)
        for (int i = 0; i < F; ++i) qs[i] = filt.q[i];                 // read below as LDS broadcasts

    for (int64_t b = blockIdx.x; b < batch; b += gridDim.x) {
        const uint32_t *tg = trees + b * (int64_t)nw;
        const T *cols = xw + b * ncols * n;
        __syncthreads();                                               // the previous signal's walk is done with the tree and the estimate
        for (int i = tid; i < nw; i += NT) tree[i] = tg[i];
        if (!thr && tid < 64) {                                        // the first wavefront: the estimate, from the words in global memory
            const int fin = __builtin_amdgcn_readfirstlane(drt_finest(tg, ntree, dmax));
            const T s = drt_estimate<T>(cols + (int64_t)(fin - 1) * n, log2n, tid);
            if (tid == 0) {
                sg_sh = s;
                if (sigma) sigma[b] = s;
            }
        }
        __syncthreads();
        T sg;
        if (thr) {
            sg = thr[per_thr ? b : 0];
            if (tid == 0 && sigma) sigma[b] = sg;
        } else sg = sg_sh;
        const T tt = (T)((double)sg * scale);
        const int keep = undersmooth ? __builtin_amdgcn_readfirstlane(drt_coarsest(tree, ntree, dmax)) : 0;   // no node has index 0
        T *xs = x + b * (int64_t)n;
        int node = 1, depth = 0;                                       // scalar: the same for every lane
        bool read = false;                                             // a combine has read its slots since the last barrier
        while (true) {
            // depth < dmax holds for every tree that passed the check; it keeps the slots inside LDS whatever the words hold
            const bool kids = node <= ntree && depth < dmax &&
                              ((__builtin_amdgcn_readfirstlane(tree[(node - 1) >> 5]) >> ((node - 1) & 31)) & 1u);
            if (kids) { node = 2 * node; ++depth; continue; }
            const T *src = cols + (int64_t)(node - 1) * n;             // a leaf: heap index node, column node - 1
            const bool th0 = node != keep;
            if (node == 1) {                                           // the root is a leaf
                for (int i = tid; i < n; i += NT) { const T a = src[i]; xs[i] = th0 ? wx_thresh<T>(a, tt, th_kind) : a; }
                break;
            }
            if (read) { __syncthreads(); read = false; }
            T *slot = slots + (size_t)(2 * (depth - 1) + (node & 1)) * n;
            // a left leaf whose sibling is a leaf too (every deepest node has such a pair): the next column with it, both loads in flight
            const bool pair = !(node & 1) && !(node + 1 <= ntree && depth < dmax &&
                                                ((__builtin_amdgcn_readfirstlane(tree[node >> 5]) >> (node & 31)) & 1u));
            if (pair) {
                const bool th1 = node + 1 != keep;
                for (int i = tid; i < n; i += NT) {
                    const T a = src[i], c = src[i + n];
                    slot[i] = th0 ? wx_thresh<T>(a, tt, th_kind) : a;
                    slot[i + n] = th1 ? wx_thresh<T>(c, tt, th_kind) : c;
                }
                ++node;
            } else {
                for (int i = tid; i < n; i += NT) { const T a = src[i]; slot[i] = th0 ? wx_thresh<T>(a, tt, th_kind) : a; }
            }
            while (node > 1 && (node & 1)) {                           // a right child is complete: its parent's combine
                __syncthreads();
                node >>= 1;
                --depth;
                const int d = depth;
                const T *w1 = slots + (size_t)(2 * d) * n, *w2 = w1 + n;
                T *out = node == 1 ? xs : slots + (size_t)(2 * (d - 1) + (node & 1)) * n;
                rt_combine<T, KIND>(w1, w2, out, n, d, 0, F, qs, tid, NT);
                read = true;
            }
            if (node == 1) break;
            ++node;                                                    // a left child is complete: on to its sibling
        }
    }
}

// sigma only: one wavefront per signal, four per workgroup; thr != nullptr: sigma[b] = the threshold given for signal b
template <typename T>
__global__ __launch_bounds__(256) void k_drt_sigma(const T *__restrict__ xw, int log2n, int64_t ncols, int dmax, int64_t batch,
                                                   const uint32_t *__restrict__ trees, const T *__restrict__ thr, int per_thr,
                                                   T *__restrict__ sigma)
{
    const int n = 1 << log2n, nw = wt_words(n);
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    for (int64_t b = (int64_t)blockIdx.x * 4 + wave; b < batch; b += (int64_t)gridDim.x * 4) {
        T s;
        if (thr) s = thr[per_thr ? b : 0];
        else {
            const int fin = __builtin_amdgcn_readfirstlane(drt_finest(trees + b * (int64_t)nw, n - 1, dmax));
            s = drt_estimate<T>(xw + (b * ncols + (fin - 1)) * n, log2n, lane);
        }
        if (lane == 0) sigma[b] = s;
    }
}

// wt = nothing: y = the table with the leaf columns of every signal's own tree thresholded (Denoising.jl:549-558), a workgroup per column
template <typename T>
__global__ __launch_bounds__(256) void k_drt_table(const T *__restrict__ xw, T *__restrict__ y, int n, int64_t ncols, int dmax, int64_t batch,
                                                   const uint32_t *__restrict__ trees, int th_kind, double scale, const T *__restrict__ sg,
                                                   int per_sg, int undersmooth)
{
    const int ntree = n - 1, nw = wt_words(n);
    const int64_t total = ncols * batch;
    for (int64_t g = blockIdx.x; g < total; g += gridDim.x) {
        const int64_t b = g / ncols, node = g - b * ncols + 1;
        const uint32_t *tg = trees + b * (int64_t)nw;
        // a valid tree: a node is decomposed only under decomposed ancestors, so a leaf is a bare node that is the root or has a decomposed parent
        bool leaf = !(node <= ntree && wt_set(tg, (int)node)) && (node == 1 || ((node >> 1) <= ntree && wt_set(tg, (int)(node >> 1))));
        if (leaf && undersmooth) leaf = node != drt_coarsest(tg, ntree, dmax);
        const T tt = (T)((double)sg[per_sg ? b : 0] * scale);
        const T *src = xw + g * n;
        T *dst = y + g * n;
        for (int i = threadIdx.x; i < n; i += blockDim.x) { const T a = src[i]; dst[i] = leaf ? wx_thresh<T>(a, tt, th_kind) : a; }
    }
}

// tv[i] = (T)(src[i] scale) (per: else src[0]), the rounding of the kernels above, and sigma[i] = src[i] where it is wanted
template <typename T>
__global__ __launch_bounds__(256) void k_drt_scale(const T *__restrict__ src, int per, double scale, T *__restrict__ tv, T *__restrict__ sigma,
                                                   int64_t batch)
{
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < batch; i += (int64_t)gridDim.x * blockDim.x) {
        const T s = src[per ? i : 0];
        tv[i] = (T)((double)s * scale);
        if (sigma) sigma[i] = s;
    }
}

inline int drt_noisest(const double *X, int64_t n, int64_t k, int64_t nb, int64_t col, double *s, void *st) { return wx_noisest_f64(X, n, k, nb, 0, col, s, st); }
inline int drt_noisest(const float *X, int64_t n, int64_t k, int64_t nb, int64_t col, float *s, void *st) { return wx_noisest_f32(X, n, k, nb, 0, col, s, st); }
inline int drt_threshold(const double *X, double *Y, int64_t n, int64_t k, int64_t nb, int kind, const double *t, const uint8_t *mask, void *st)
{ return wx_threshold_f64(X, Y, n, k, nb, kind, t, nb, 0, mask, st); }
inline int drt_threshold(const float *X, float *Y, int64_t n, int64_t k, int64_t nb, int kind, const float *t, const uint8_t *mask, void *st)
{ return wx_threshold_f32(X, Y, n, k, nb, kind, t, nb, 0, mask, st); }
inline int drt_inverse(bool ac, const double *xw, double *x, int64_t n, int64_t k, const uint8_t *t, int64_t nt, int64_t nb, const double *qmf, int F, void *st)
{ return ac ? wx_iacwpd1d_f64(xw, x, n, k, 0, t, nt, nb, st) : wx_iswpd1d_f64(xw, x, n, k, 0, t, nt, -1, nb, qmf, F, st); }
inline int drt_inverse(bool ac, const float *xw, float *x, int64_t n, int64_t k, const uint8_t *t, int64_t nt, int64_t nb, const double *qmf, int F, void *st)
{
    if (ac) return wx_set_error(WX_EUNSUPPORTED, "the autocorrelation transforms are Float64 only");
    return wx_iswpd1d_f32(xw, x, n, k, 0, t, nt, -1, nb, qmf, F, st);
}

// what the driver (wx_trees_host.h) needs to know of a redundant packet table and of the denoising arguments that travel with it
template <typename T> struct DrtShape {
    int64_t n, ncols, batch;
    bool ac, has_filter, has_out;                                      // the ACWT entry has no filter; xhat is there
    int th_kind;
    double scale;
    const T *thr;
    int64_t nthr;
    int undersmooth;
    T *sigma;
    mutable const T *dthr = nullptr;                                  // stage(): thr and sigma as device pointers
    mutable T *dsigma = nullptr;
    static constexpr bool quad = false;
    static constexpr bool extras = true;
    static constexpr bool table = true;                                // the input item is the table; its depth bounds the trees
    bool walks() const { return ac || has_filter; }                    // else the output is the thresholded table
    bool dims_ok() const { return n >= 1 && ncols >= 1; }
    int64_t count() const { return walks() ? n : n * ncols; }
    int64_t in_count() const { return n * ncols; }
    // the deepest tree the table holds: 2^(D + 1) - 1 <= ncols, never deeper than a valid tree (RtShape, wx_red_trees.hip)
    int dmax() const
    {
        int D = 0;
        while (D < 30 && ((int64_t)1 << (D + 2)) - 1 <= ncols && ((int64_t)2 << D) <= n) ++D;
        return D;
    }
    int tree_k() const { return dmax() + 1; }
    int too_deep() const { return wx_set_error(WX_EBOUNDS, "tree reaches below the last column of xw"); }
    int check(bool, int, int64_t ntree) const
    {
        WX_REQUIRE(th_kind >= 0 && th_kind <= 3, WX_EARG, "th_kind: 0 HardTH, 1 SoftTH, 2 SemiSoftTH, 3 SteinTH");
        WX_REQUIRE(nthr == 0 || nthr == 1 || nthr == batch, WX_EARG, "no threshold (the noise is estimated), one, or one per signal");
        WX_REQUIRE((thr != nullptr) == (nthr != 0) || batch == 0, WX_EARG, "thr and nthr disagree");
        WX_REQUIRE(has_out || sigma != nullptr || batch == 0, WX_EARG, "denoiseall(trees): neither xhat nor sigma");
        WX_REQUIRE(wx_isdyadic(n), WX_EASSERT, "maketree/isvalidtree: signal length must be dyadic (Wavelets.jl)");
        WX_REQUIRE(ntree == n - 1, WX_EASSERT, "@assert n_t == gettreelength(sz...) (Utils.jl:211)");
        WX_REQUIRE(n < ((int64_t)1 << 30) && ncols < ((int64_t)1 << 31), WX_EUNSUPPORTED, "denoiseall(trees): table too large");
        return WX_OK;
    }
    int check_host(const uint8_t *trees, int64_t ntree, int64_t nb, int k, uint32_t *bits, int nw, uint8_t *depths, bool *same) const
    { return wx_trees_check_host(false, n, 1, trees, ntree, nb, k, -1, bits, nw, depths, same); }
    // WX_MAXF doubles | two columns per depth | the tree's words | the estimate
    size_t lds() const { return sizeof(double) * WX_MAXF + (size_t)2 * dmax() * n * sizeof(T) + sizeof(uint32_t) * wt_words(n) + 16; }
    template <typename U> bool window(int64_t, int F) const
    {
        return wx_isdyadic(n) && n >= 8 && n <= ((int64_t)1 << DRT_MAXLOG2N) && (!has_filter || (F >= 2 && F <= 20 && F % 2 == 0)) &&
               lds() <= 136 * 1024;
    }
    // item b alone: its threshold and its estimate
    DrtShape at(int64_t b) const
    {
        DrtShape s = *this;
        s.batch = 1;
        if (thr) { s.thr = nthr == batch ? thr + b : thr; s.nthr = 1; }
        if (sigma) s.sigma = sigma + b;
        return s;
    }
    bool stage(WxIO &io, int64_t nb) const
    {
        dthr = thr ? (const T *)io.in(thr, sizeof(T) * nthr) : nullptr;
        dsigma = sigma ? (T *)io.out(sigma, sizeof(T) * nb) : nullptr;
        return (dthr || !thr) && (dsigma || !sigma);
    }
    // one tree for `nb` signals: wx_noisest_* on the column of its finest detail node, wx_threshold_* with its leaf mask, then the inverse
    int single(int, const T *x, T *y, int, const uint8_t *t, int64_t nt, int64_t nb, const double *qmf, int F, void *stream) const
    {
        int64_t fin = 1, coarse = 1;
        while (fin <= nt && t[fin - 1]) fin = 2 * fin + 1;             // Utils.jl:428-433
        while (coarse < nt && t[coarse - 1]) coarse = 2 * coarse;      // Utils.jl:363-367: n = 2 with a decomposed root stays at the root
        std::vector<uint8_t> mask((size_t)ncols);
        for (int64_t i = 1; i <= ncols; ++i)
            mask[(size_t)(i - 1)] = !(i <= nt && t[i - 1]) && (i == 1 || ((i >> 1) <= nt && t[(i >> 1) - 1]));
        if (undersmooth && coarse <= ncols) mask[(size_t)(coarse - 1)] = 0;
        hipStream_t st = wx_stream(stream);
        WxScratch scr(st);
        T *est = nullptr;
        int rc;
        if (!thr) {
            if (!(est = (T *)scr.alloc(sizeof(T) * nb))) return WX_EHIP;
            if ((rc = drt_noisest(x, n, ncols, nb, fin - 1, est, stream))) return rc;
        }
        T *tv = (T *)scr.alloc(sizeof(T) * nb);                         // the thresholds after scaling
        if (!tv) return WX_EHIP;
        {
            WxIO io(st);
            const T *src = thr ? (const T *)io.in(thr, sizeof(T) * nthr) : est;
            T *ds = sigma ? (T *)io.out(sigma, sizeof(T) * nb) : nullptr;
            if (!src || (sigma && !ds)) return io.finish(WX_EHIP);
            const int64_t g = (nb + 255) / 256;
            hipLaunchKernelGGL(k_drt_scale<T>, dim3((unsigned)(g < 4096 ? g : 4096)), dim3(256), 0, st, src, !thr || (nthr == nb && nb > 1) ? 1 : 0,
                               scale, tv, ds, nb);
            if (hipGetLastError() != hipSuccess) return io.finish(wx_set_error(WX_EHIP, "denoiseall(trees): kernel failed to launch"));
            if ((rc = io.finish(WX_OK))) return rc;
        }
        if (!y) return WX_OK;
        if (!walks()) return drt_threshold(x, y, n, ncols, nb, th_kind, tv, mask.data(), stream);
        T *xt = (T *)scr.alloc(sizeof(T) * (size_t)(n * ncols) * (size_t)nb);   // the thresholded copy (the reference leaves x alone)
        if (!xt) return WX_EHIP;
        if ((rc = drt_threshold(x, xt, n, ncols, nb, th_kind, tv, mask.data(), stream))) return rc;
        return drt_inverse(ac, xt, y, n, ncols, t, nt, nb, qmf, F, stream);
    }
    template <typename U, int KIND>
    hipError_t launch_kind(const T *dx, T *dy, int log2n, int64_t nb, const uint32_t *dt, const WxFilt &filt, int per, hipStream_t st) const
    {
        const size_t bytes = lds() - 16;                               // the estimate's word is static
        const int nt = wx_trees_threads(2 * n);                        // one lane per parent position, not per pair
        auto kern = k_denoise_red_trees<T, KIND>;
        hipError_t e = hipSuccess;
        if (bytes > 48 * 1024) e = hipFuncSetAttribute(reinterpret_cast<const void *>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes);
        if (e != hipSuccess) return e;
        hipLaunchKernelGGL(kern, dim3(wx_trees_grid(lds(), nt, nb)), dim3(nt), bytes, st, dx, dy, log2n, ncols, dmax(), nb, dt, filt, th_kind, scale,
                           dthr, per, undersmooth, dsigma);
        return hipGetLastError();
    }
    template <typename U, int MODE>
    hipError_t launch(const T *dx, T *dy, int64_t, int, int64_t nb, const uint32_t *dt, const uint8_t *, const WxFilt &filt, hipStream_t st) const
    {
        int log2n = 0;
        while (((int64_t)1 << log2n) < n) ++log2n;
        int per = nthr == nb && nb > 1 ? 1 : 0;
        if (dy && walks()) {
            if constexpr (sizeof(T) == 8)
                if (ac) return launch_kind<T, DRT_AC>(dx, dy, log2n, nb, dt, filt, per, st);
            return launch_kind<T, DRT_AVG>(dx, dy, log2n, nb, dt, filt, per, st);
        }
        // nothing to walk: the estimates (or the thresholds given, where sigma wants them), then the table
        WxScratch scr(st);
        const T *sg = dthr;
        if (!dthr || dsigma) {
            T *s = dsigma;
            if (!s && !(s = (T *)scr.alloc(sizeof(T) * nb))) return hipErrorOutOfMemory;
            const int64_t g = (nb + 3) / 4;
            hipLaunchKernelGGL(k_drt_sigma<T>, dim3((unsigned)(g < 8192 ? g : 8192)), dim3(256), 0, st, dx, log2n, ncols, dmax(), nb, dt, dthr, per, s);
            if (!dthr) { sg = s; per = 1; }
        }
        if (dy) {
            const int64_t g = ncols * nb;
            hipLaunchKernelGGL(k_drt_table<T>, dim3((unsigned)(g < 8192 ? g : 8192)), dim3(256), 0, st, dx, dy, (int)n, ncols, dmax(), nb, dt, th_kind,
                               scale, sg, per, undersmooth);
        }
        return hipGetLastError();
    }
};

template <typename T>
int api_denoise_red_trees(bool ac, const T *xw, T *out, int64_t n, int64_t ncols, const uint8_t *trees, int64_t ntree, int64_t batch,
                          const double *qmf, int F, int th_kind, double scale, const T *thr, int64_t nthr, int undersmooth, T *sigma, void *stream)
{
    const DrtShape<T> s{n, ncols, batch, ac, qmf != nullptr, out != nullptr, th_kind, scale, thr, nthr, undersmooth, sigma};
    return wx_trees_api<T, WX_TREES_INV>(s, xw, out, 1, trees, ntree, batch, qmf, F, stream);
}

}  // namespace

extern "C" {

int wx_denoise_swpd1d_trees_f64(const double *xw, double *out, int64_t n, int64_t ncols, const uint8_t *trees, int64_t ntree, int64_t batch,
                                const double *qmf, int F, int th_kind, double scale, const double *thr, int64_t nthr, int undersmooth,
                                double *sigma, void *stream)
{ return api_denoise_red_trees<double>(false, xw, out, n, ncols, trees, ntree, batch, qmf, F, th_kind, scale, thr, nthr, undersmooth, sigma, stream); }
int wx_denoise_swpd1d_trees_f32(const float *xw, float *out, int64_t n, int64_t ncols, const uint8_t *trees, int64_t ntree, int64_t batch,
                                const double *qmf, int F, int th_kind, double scale, const float *thr, int64_t nthr, int undersmooth,
                                float *sigma, void *stream)
{ return api_denoise_red_trees<float>(false, xw, out, n, ncols, trees, ntree, batch, qmf, F, th_kind, scale, thr, nthr, undersmooth, sigma, stream); }
int wx_denoise_acwpd1d_trees_f64(const double *xw, double *out, int64_t n, int64_t ncols, const uint8_t *trees, int64_t ntree, int64_t batch,
                                 int th_kind, double scale, const double *thr, int64_t nthr, int undersmooth, double *sigma, void *stream)
{ return api_denoise_red_trees<double>(true, xw, out, n, ncols, trees, ntree, batch, nullptr, 0, th_kind, scale, thr, nthr, undersmooth, sigma, stream); }

}  // extern "C"
