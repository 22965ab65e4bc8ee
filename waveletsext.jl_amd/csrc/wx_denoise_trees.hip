// wx_denoise_trees.hip -- denoise / denoiseall(xw, :wpt, wt; tree, dnt, estnoise, smooth) with ONE tree per signal: every signal is denoised in
// its own basis, the one bestbasistreeall(X, BB()) (BestBasis.jl:253-262) chose for it.  The reference takes a single BitVector here
// (Denoising.jl:483-599, 651-712); the extension follows the (ntree, batch) convention of its getbasiscoefall (Utils.jl:199-225), like
// wx_wpt_trees.hip does for the transforms.
//
// Kernel: the inverse branch of k_wpt_trees (wx_wpt_trees.hip) -- a workgroup takes a signal and strides over the batch, the coefficients are
// staged into both LDS buffers, the signal's tree bits sit next to them -- with three steps between the staging and the inverse levels, all
// of them from the signal's own tree:
//   ranges     the finest detail range [n - (n >> j_r), n), j_r = the length of the chain of decomposed right children from the root
//              (finestdetailrange, Utils.jl:416-436), and the end n >> j_l of the coarsest scaling range, j_l = the left chain
//              (coarsestscalingrange, Utils.jl:351-370, with its strict `<`); a root that is a leaf has j_r = j_l = 0: the details are the
//              whole signal, and :undersmooth thresholds nothing;
//   estimate   sigma = mad(details) / 0.6745 (noisest, Denoising.jl:214-232) with the arithmetic and the non-finite rules of k_mad
//              (wx_denoise.hip): exact order statistics by the workgroup's LDS selection (wx_select_lds.h), middle(a, b) = a/2 + b/2, the
//              deviations rounded in T.  They live in the second buffer's copy of the details, which the next step writes again: no LDS
//              beyond the buffers, the tree and the selection's scratch;
//   threshold  rows [lo, n) with wx_thresh(v, (T)(sigma scale), kind), the rounding of k_threshold_copy / wx_iwpt1d_thresh_*; lo = the
//              coarsest scaling end when undersmoothing, else 0.
// Without a filter the thresholded coefficients are the output; without an output only sigma is written; with thresholds given the
// estimate is skipped.  No atomics on global memory; every output element is written by exactly one lane.
// The host side is the driver of wx_trees_host.h with DnShape: the same checks, packing, routes and waits as wx_iwpt1d_trees_*.
#include "wx_kernels.h"
#include "wx_select_lds.h"
#include "wx_trees_host.h"

namespace {

// x, y: (n, batch); trees: wt_words(n) words of tree bits per signal; depths: batch bytes.  filt.F == 0: no inverse.  y == nullptr: sigma only.
// thr != nullptr: the thresholds before scaling (per_thr: one per signal), no estimate.  sigma (optional): batch values.
// LDS: WX_MAXF doubles | two buffers of n elements | the tree's words (dynamic), the selection's scratch (static).
template <typename T>
__global__ __launch_bounds__(1024) void k_denoise_trees(const T *__restrict__ x, T *__restrict__ y, int log2n, int64_t batch,
                                                        const uint32_t *__restrict__ trees, const uint8_t *__restrict__ depths, WxFilt filt,
                                                        int th_kind, double scale, const T *__restrict__ thr, int per_thr, int undersmooth,
                                                        T *__restrict__ sigma)
{
    extern __shared__ __attribute__((aligned(16))) char dt_smem[];
    __shared__ WxSelScratch S;
    typedef typename WxVec2<T>::type V2;
    const int n = 1 << log2n, ntree = n - 1, half = n >> 1;
    double *qs = reinterpret_cast<double *>(dt_smem);
    T *buf0 = reinterpret_cast<T *>(qs + WX_MAXF);
    T *buf1 = buf0 + n;
    uint32_t *tree = reinterpret_cast<uint32_t *>(buf1 + n);
    const int nw = wt_words(n);
    const int tid = threadIdx.x, NT = blockDim.x, F = filt.F;
    if (tid == 0)
        for (int i = 0; i < F; ++i) qs[i] = filt.q[i];                 // read below as LDS broadcasts

    for (int64_t b = blockIdx.x; b < batch; b += gridDim.x) {
        const uint32_t *tg = trees + b * (int64_t)nw;
        __syncthreads();                                               // the previous signal's last level is done with tree and buffers
        for (int i = tid; i < nw; i += NT) tree[i] = tg[i];
        const int depth = depths[b];
        const T *xs = x + b * (int64_t)n;
        for (int i = tid; i < half; i += NT) {
            const int p = 2 * i;
            const V2 v = *reinterpret_cast<const V2 *>(xs + p);
            *reinterpret_cast<V2 *>(buf0 + p) = v;
            *reinterpret_cast<V2 *>(buf1 + p) = v;
        }
        __syncthreads();
        // the chains from the root: right children 1, 3, 7, ... (the last one, node n - 1 = ntree, has two samples), left children 1, 2, 4, ...
        int jr = 0, jl = 0;
        for (int node = 1; node <= ntree && wt_set(tree, node); node = 2 * node + 1) ++jr;
        for (int node = 1; node < ntree && wt_set(tree, node); node = 2 * node) ++jl;
        T sg;
        if (thr) sg = thr[per_thr ? b : 0];
        else {
            const int cnt = n >> jr;                                   // 1 ... n details, the tail of the signal
            T *dv = buf1 + (n - cnt);
            int nan = 0;
            for (int i = tid; i < cnt; i += NT) nan |= dv[i] != dv[i];
            nan = __syncthreads_or(nan);
            const T m = wx_median_lds<T>(dv, cnt, &S);
            // a NaN among the details, or a median of +-Inf or NaN (the deviations then hold Inf - Inf): NaN, as k_mad (uniform over the workgroup)
            if (nan || !(fabs((double)m) < (double)INFINITY)) sg = (T)__builtin_nan("");
            else {
                for (int i = tid; i < cnt; i += NT) dv[i] = (T)fabs((double)(T)(dv[i] - m));
                __syncthreads();
                const T r = wx_median_lds<T>(dv, cnt, &S);
                sg = (T)(r / (T)0.6745);
            }
        }
        if (tid == 0 && sigma) sigma[b] = sg;
        if (!y) continue;
        // threshold from the first buffer, which still holds the coefficients; the second one gets its details back with it
        const T tt = (T)((double)sg * scale);
        const int lo = undersmooth ? n >> jl : 0;
        const bool direct = depth == 0 || F == 0;                      // the root is a leaf, or no transform: the thresholded coefficients leave
        T *ys = y + b * (int64_t)n;
        for (int i = tid; i < half; i += NT) {
            const int p = 2 * i;
            V2 v = *reinterpret_cast<const V2 *>(buf0 + p);
            if (p >= lo) v.x = wx_thresh<T>(v.x, tt, th_kind);
            if (p + 1 >= lo) v.y = wx_thresh<T>(v.y, tt, th_kind);
            if (direct) *reinterpret_cast<V2 *>(ys + p) = v;
            else {
                *reinterpret_cast<V2 *>(buf0 + p) = v;
                *reinterpret_cast<V2 *>(buf1 + p) = v;
            }
        }
        __syncthreads();
        if (direct) continue;
        // the inverse levels of k_wpt_trees, bottom-up from the tree's own depth (idwt_step!, dwt/dwt_one_level.jl:192-223)
        T *cur = buf0, *nxt = buf1;
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

// sigma[i] = thr[i] (per) or thr[0]: the thresholds used, where they were given and the single-tree entries ran
template <typename T>
__global__ __launch_bounds__(256) void k_denoise_trees_given(const T *__restrict__ thr, int per, T *__restrict__ sigma, int64_t batch)
{
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < batch; i += (int64_t)gridDim.x * blockDim.x) sigma[i] = thr[per ? i : 0];
}

inline int dt_noisest(const double *X, int64_t n, int64_t batch, int64_t lo, double *s, void *st) { return wx_noisest_f64(X, n, 1, batch, lo, 0, s, st); }
inline int dt_noisest(const float *X, int64_t n, int64_t batch, int64_t lo, float *s, void *st) { return wx_noisest_f32(X, n, 1, batch, lo, 0, s, st); }
inline int dt_iwpt_thresh(const double *x, double *y, int64_t n, const uint8_t *t, int64_t nt, int64_t batch, const double *qmf, int F, int kind,
                          const double *tv, int64_t ntv, int64_t lo, double scale, void *st)
{ return wx_iwpt1d_thresh_f64(x, y, n, 0, t, nt, batch, qmf, F, kind, tv, ntv, lo, scale, st); }
inline int dt_iwpt_thresh(const float *x, float *y, int64_t n, const uint8_t *t, int64_t nt, int64_t batch, const double *qmf, int F, int kind,
                          const float *tv, int64_t ntv, int64_t lo, double scale, void *st)
{ return wx_iwpt1d_thresh_f32(x, y, n, 0, t, nt, batch, qmf, F, kind, tv, ntv, lo, scale, st); }

// what the driver (wx_trees_host.h) needs to know of a signal of n samples and of the denoising arguments that travel with it
template <typename T> struct DnShape {
    int64_t n, batch;
    int th_kind;
    double scale;
    const T *thr;
    int64_t nthr;
    int undersmooth;
    T *sigma;
    bool has_out, has_filter;                                          // xhat and qmf are there
    mutable const T *dthr = nullptr;                                  // stage(): thr and sigma as device pointers
    mutable T *dsigma = nullptr;
    static constexpr bool quad = false;
    static constexpr bool extras = true;
    bool dims_ok() const { return n >= 1; }
    int64_t count() const { return n; }
    int check(bool, int, int64_t ntree) const
    {
        WX_REQUIRE(th_kind >= 0 && th_kind <= 3, WX_EARG, "th_kind: 0 HardTH, 1 SoftTH, 2 SemiSoftTH, 3 SteinTH");
        WX_REQUIRE(nthr == 0 || nthr == 1 || nthr == batch, WX_EARG, "no threshold (the noise is estimated), one, or one per signal");
        WX_REQUIRE((thr != nullptr) == (nthr != 0) || batch == 0, WX_EARG, "thr and nthr disagree");
        WX_REQUIRE(has_out || sigma != nullptr || batch == 0, WX_EARG, "denoiseall(trees): neither xhat nor sigma");
        WX_REQUIRE(wx_isdyadic(n), WX_EASSERT, "maketree/isvalidtree: signal length must be dyadic (Wavelets.jl)");
        WX_REQUIRE(ntree == n - 1, WX_EASSERT, "@assert n_t == gettreelength(sz...) (Utils.jl:211)");
        WX_REQUIRE(n < ((int64_t)1 << 30), WX_EUNSUPPORTED, "denoiseall(trees): signal length >= 2^30 not supported");
        return WX_OK;
    }
    int check_host(const uint8_t *trees, int64_t ntree, int64_t nb, int k, uint32_t *bits, int nw, uint8_t *depths, bool *same) const
    { return wx_trees_check_host(false, n, 1, trees, ntree, nb, k, -1, bits, nw, depths, same); }
    size_t lds() const { return sizeof(double) * WX_MAXF + (size_t)2 * n * sizeof(T) + sizeof(uint32_t) * wt_words(n); }
    // the window of k_wpt_trees; without a filter the kernel has no taps to loop over, and any length of filter would do
    template <typename U> bool window(int64_t, int F) const
    { return wx_fused1d_ok<T>(n, has_filter ? F : 2) && lds() + sizeof(WxSelScratch) <= 160 * 1024; }
    // item b alone: its threshold and its estimate
    DnShape at(int64_t b) const
    {
        DnShape s = *this;
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
    // one tree for `nb` signals: wx_noisest_* on its finest detail range, then the threshold on the loads of wx_iwpt1d_thresh_*
    int single(int, const T *x, T *y, int, const uint8_t *t, int64_t nt, int64_t nb, const double *qmf, int F, void *stream) const
    {
        int jr = 0, jl = 0;
        for (int64_t node = 1; node <= nt && t[node - 1]; node = 2 * node + 1) ++jr;     // Utils.jl:416-436
        for (int64_t node = 1; node < nt && t[node - 1]; node = 2 * node) ++jl;          // Utils.jl:351-370
        const int64_t lo = undersmooth ? n >> jl : 0;
        hipStream_t st = wx_stream(stream);
        WxScratch scr(st);
        const T *tv = thr;
        int64_t ntv = nthr;
        int rc;
        if (thr) {
            if (sigma) {
                WxIO io(st);
                const T *dt = (const T *)io.in(thr, sizeof(T) * nthr);
                T *ds = (T *)io.out(sigma, sizeof(T) * nb);
                if (!dt || !ds) return io.finish(WX_EHIP);
                const int64_t g = (nb + 255) / 256;
                hipLaunchKernelGGL(k_denoise_trees_given<T>, dim3((unsigned)(g < 4096 ? g : 4096)), dim3(256), 0, st, dt, nthr == nb && nb > 1 ? 1 : 0, ds, nb);
                if (hipGetLastError() != hipSuccess) return io.finish(wx_set_error(WX_EHIP, "denoiseall(trees): kernel failed to launch"));
                if ((rc = io.finish(WX_OK))) return rc;
            }
        } else {
            T *sg = sigma;
            if (!sg && !(sg = (T *)scr.alloc(sizeof(T) * nb))) return WX_EHIP;
            if ((rc = dt_noisest(x, n, nb, n - (n >> jr), sg, stream))) return rc;
            tv = sg;
            ntv = nb;
        }
        if (!y) return WX_OK;
        if (qmf) return dt_iwpt_thresh(x, y, n, t, nt, nb, qmf, F, th_kind, tv, ntv, lo, scale, stream);
        // wt = nothing: the thresholded coefficients
        WxIO io(st);
        const T *dx = (const T *)io.in(x, sizeof(T) * n * nb);
        T *dy = (T *)io.out(y, sizeof(T) * n * nb);
        const T *dt = (const T *)io.in(tv, sizeof(T) * ntv);
        if (!dx || !dy || !dt) return io.finish(WX_EHIP);
        return io.finish(wx_dev_threshold_copy<T>(dx, dy, n, nb, th_kind, dt, ntv == nb && nb > 1 ? 1 : 0, lo, scale, st));
    }
    template <typename U, int MODE>
    hipError_t launch(const T *dx, T *dy, int64_t, int, int64_t nb, const uint32_t *dt, const uint8_t *dd, const WxFilt &filt, hipStream_t st) const
    {
        const size_t bytes = lds();
        int nt = wx_trees_threads(n);
        if (nt < 256) nt = 256;                                        // the selection's scratch is sized for 4 ... 16 wavefronts' worth of candidates
        auto kern = k_denoise_trees<T>;
        hipError_t e = hipSuccess;
        if (bytes > 48 * 1024) e = hipFuncSetAttribute(reinterpret_cast<const void *>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes);
        if (e != hipSuccess) return e;
        int log2n = 0;
        while (((int64_t)1 << log2n) < n) ++log2n;
        hipLaunchKernelGGL(kern, dim3(wx_trees_grid(bytes + sizeof(WxSelScratch), nt, nb)), dim3(nt), bytes, st, dx, dy, log2n, nb, dt, dd, filt,
                           th_kind, scale, dthr, nthr == nb && nb > 1 ? 1 : 0, undersmooth, dsigma);
        return hipGetLastError();
    }
};

template <typename T>
int api_denoise_trees(const T *xw, T *xhat, int64_t n, const uint8_t *trees, int64_t ntree, int64_t batch, const double *qmf, int F, int th_kind,
                      double scale, const T *thr, int64_t nthr, int undersmooth, T *sigma, void *stream)
{
    const DnShape<T> s{n, batch, th_kind, scale, thr, nthr, undersmooth, sigma, xhat != nullptr, qmf != nullptr};
    return wx_trees_api<T, WX_TREES_INV>(s, xw, xhat, 1, trees, ntree, batch, qmf, F, stream);
}

}  // namespace

extern "C" {

int wx_denoise_wpt1d_trees_f64(const double *xw, double *xhat, int64_t n, const uint8_t *trees, int64_t ntree, int64_t batch, const double *qmf,
                               int F, int th_kind, double scale, const double *thr, int64_t nthr, int undersmooth, double *sigma, void *stream)
{ return api_denoise_trees<double>(xw, xhat, n, trees, ntree, batch, qmf, F, th_kind, scale, thr, nthr, undersmooth, sigma, stream); }
int wx_denoise_wpt1d_trees_f32(const float *xw, float *xhat, int64_t n, const uint8_t *trees, int64_t ntree, int64_t batch, const double *qmf,
                               int F, int th_kind, double scale, const float *thr, int64_t nthr, int undersmooth, float *sigma, void *stream)
{ return api_denoise_trees<float>(xw, xhat, n, trees, ntree, batch, qmf, F, th_kind, scale, thr, nthr, undersmooth, sigma, stream); }

}  // extern "C"
