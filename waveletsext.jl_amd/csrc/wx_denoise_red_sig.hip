// wx_denoise_red_sig.hip -- denoiseall(swpdall(x, wt, L), :swpd, wt; tree = M, ...) and the same on acwpdall with ONE tree per signal, straight
// from the SIGNALS: every signal is analysed along its own tree only, thresholded at that tree's leaves and synthesised again, and the
// (n, 2^(L+1) - 1, batch) packet table that wx_denoise_swpd1d_trees_* / wx_denoise_acwpd1d_trees_f64 (wx_denoise_red_trees.hip) start
// from is never written.
//   sdwt_step! / acdwt_step!       swt/swt_one_level.jl:99-127, acwt/acwt_one_level.jl:101-128 (rb_step, wx_red_bb.h)
//   noisest(x, true, tree)         Denoising.jl:228-231 on finestdetailrange, Utils.jl:428-433 (wx_red_estimate.h)
//   denoise(x, :swpd | :acwpd)     Denoising.jl:544-594: the leaves of getleaf(tree) thresholded, coarsestscalingrange (Utils.jl:363-367)
//                                  left alone when undersmoothing, then iswpd without a shift (:561) or iacwpd (:594)
//   isdwt_step! / iacdwt_step!     swt/swt_one_level.jl:257-277, acwt/acwt_one_level.jl:217-224 (rt_combine, wx_red_combine.h)
//
// Kernel (k_denoise_red_sig<T, AC>): a workgroup takes a signal and strides over the batch; the signal's tree bits sit in LDS, and two
// columns per depth 1 .. L: 2 L n sizeof(T) bytes, the window of k_red_trees with the table's depth replaced by the argument L -- so the
// size is known before any tree is read.
//   estimate   the finest detail node is reached from the root by right children while decomposed: a chain of at most L steps from the
//              signal, each into the right-child slot of its depth, a barrier between them.  Then ONE wavefront runs dn_noisest on
//              the last column (the signal itself in global memory for a bare root), exactly as k_denoise_red_trees does on a column of
//              the table.  Skipped when the thresholds are given.
//   walk       pre-order down, post-order up; the state is the heap index and the depth, read from tree words every lane reads alike
//              through readfirstlane: scalar, so every barrier sits in uniform control flow.
//              down   a decomposed node writes both children into the slots of the next depth (the root is read from x in global
//                     memory, every other parent from its slot).  A child that is a leaf passes wx_thresh(v, (T)((double)sigma * scale),
//                     kind) on the way, after the rounding to T the table would have given it -- except the coarsest scaling node
//                     when undersmoothing;
//              up     when a right child is complete, its parent's combine (rt_combine: RT_AVG or RT_AC) writes the parent's slot,
//                     which nothing reads any more; the root's combine writes out.
//              A barrier stands before every expansion and every combine.  A bare root is thresholded from x to out.
//   out == NULL  the estimate only (noisestall, bestTH).
// No scratch memory, no atomics; every element of x is read from global memory by the root's expansion (and the estimate's first step),
// every element of out is written once, by one lane.
// Window: dyadic 8 <= n <= 1024 (16 registers per lane hold the estimate's column), even filters of 2 .. 20 taps, 1 <= L, and
//   64 doubles of taps + 2 L n sizeof(T) + the tree's words + 16 bytes <= 160 KiB:
// Float64 every depth up to n = 512 and depth 9 at n = 1024; Float32 every depth.  Outside it (route 2) the checked batch goes through the
// table entries in chunks of signals: wx_swpd1d_* / wx_acwpd1d_f64 into scratch of at most 256 MiB (one signal's table if that alone is
// larger), then wx_denoise_swpd1d_trees_* / wx_denoise_acwpd1d_trees_f64 on the chunk.  L = 0 (route 3) admits bare roots only: the
// signal is its own one-column table.
#include "wx_kernels.h"
#include "wx_acfilt.h"
#include "wx_red_bb.h"
#include "wx_red_combine.h"
#include "wx_red_estimate.h"
#include "wx_trees_host.h"

namespace {

// x: (n, batch); out: (n, batch) or nullptr; trees: wt_words(n) words of tree bits per signal, no tree deeper than L.
// filt: the QMF, and for AC in `acf` b_l at q[l - 1].  thr != nullptr: the thresholds before scaling (per_thr: one per signal), no
// estimate.  sigma (optional): batch values.  LDS: WX_MAXF doubles | 2 L columns of n elements | the tree's words (dynamic), the estimate (static).
template <typename T, bool AC>
__global__ __launch_bounds__(1024) void k_denoise_red_sig(const T *__restrict__ x, T *__restrict__ out, int log2n, int L, int64_t batch,
                                                          const uint32_t *__restrict__ trees, WxFilt filt, double c1, int th_kind, double scale,
                                                          const T *__restrict__ thr, int per_thr, int undersmooth, T *__restrict__ sigma)
{
    extern __shared__ __attribute__((aligned(16))) char drs_smem[];
    __shared__ T sg_sh;
    const int n = 1 << log2n, msk = n - 1, ntree = n - 1;
    double *qs = reinterpret_cast<double *>(drs_smem);
    T *slots = reinterpret_cast<T *>(qs + WX_MAXF);                    // child c of a node of depth d - 1: slots + (2 (d - 1) + c) n
    uint32_t *tree = reinterpret_cast<uint32_t *>(slots + (size_t)2 * L * n);
    const int nw = wt_words(n);
    const int tid = threadIdx.x, NT = blockDim.x, F = filt.F;
    if (tid == 0)
        for (int i = 0; i < F; ++i) qs[i] = filt.q[i];                 // read below as LDS broadcasts (AC: b_l of the odd lags l < F)
    constexpr int KIND = AC ? RT_AC : RT_AVG;

    for (int64_t b = blockIdx.x; b < batch; b += gridDim.x) {
        const uint32_t *tg = trees + b * (int64_t)nw;
        const T *xs = x + b * (int64_t)n;
        __syncthreads();                                               // the previous signal's walk is done with the tree, the slots and the estimate
        for (int i = tid; i < nw; i += NT) tree[i] = tg[i];
        __syncthreads();
        T sg;
        if (thr) {
            sg = thr[per_thr ? b : 0];
            if (tid == 0 && sigma) sigma[b] = sg;
        } else {
            // depth < L holds for every tree that passed the check; it keeps the slots inside LDS whatever the words hold
            const int fin = __builtin_amdgcn_readfirstlane(drt_finest(tree, ntree, L));
            const T *col = xs;                                         // the chain of high-pass steps root -> fin: 3, 7, 15, ...
            int d = 0;
            for (int node = 1; node != fin; node = 2 * node + 1, ++d) {
                T *hi = slots + (size_t)(2 * d + 1) * n;
                for (int i = tid; i < n; i += NT) {
                    double a, dd;
                    rb_step<T, AC>(col, i, 1 << d, msk, F, qs, c1, a, dd);
                    hi[i] = (T)dd;
                }
                __syncthreads();                                       // uniform: fin is scalar
                col = hi;
            }
            if (tid < 64) {                                            // the first wavefront: the estimate
                const T s = drt_estimate<T>(col, log2n, tid);
                if (tid == 0) {
                    sg_sh = s;
                    if (sigma) sigma[b] = s;
                }
            }
            __syncthreads();
            sg = sg_sh;
        }
        if (!out) continue;                                            // uniform: a kernel argument
        const T tt = (T)((double)sg * scale);
        const int keep = undersmooth ? __builtin_amdgcn_readfirstlane(drt_coarsest(tree, ntree, L)) : 0;   // no node has index 0
        T *xo = out + b * (int64_t)n;
        auto kids = [&](int node, int depth) -> bool {
            return node <= ntree && depth < L && ((__builtin_amdgcn_readfirstlane(tree[(node - 1) >> 5]) >> ((node - 1) & 31)) & 1u);
        };
        if (!kids(1, 0)) {                                             // the root is a leaf
            const bool th0 = keep != 1;
            for (int i = tid; i < n; i += NT) { const T a = xs[i]; xo[i] = th0 ? wx_thresh<T>(a, tt, th_kind) : a; }
            continue;
        }
        int node = 1, depth = 0;                                       // scalar: the same for every lane
        while (true) {
            if (kids(node, depth)) {
                // down: both children into the slots of depth + 1, thresholded where they are leaves
                const T *v = node == 1 ? xs : slots + (size_t)(2 * (depth - 1) + (node & 1)) * n;
                T *lo = slots + (size_t)(2 * depth) * n, *hi = lo + n;
                const bool thl = !kids(2 * node, depth + 1) && 2 * node != keep;
                const bool thh = !kids(2 * node + 1, depth + 1) && 2 * node + 1 != keep;
                __syncthreads();                                       // v is complete, and the slots of depth + 1 have been read
                for (int i = tid; i < n; i += NT) {
                    double a, dd;
                    rb_step<T, AC>(v, i, 1 << depth, msk, F, qs, c1, a, dd);
                    const T ta = (T)a, td = (T)dd;
                    lo[i] = thl ? wx_thresh<T>(ta, tt, th_kind) : ta;
                    hi[i] = thh ? wx_thresh<T>(td, tt, th_kind) : td;
                }
                node = 2 * node;
                ++depth;
                continue;
            }
            while (node > 1 && (node & 1)) {                           // a right child is complete: its parent's combine
                __syncthreads();
                node >>= 1;
                --depth;
                const T *w1 = slots + (size_t)(2 * depth) * n, *w2 = w1 + n;
                T *o = node == 1 ? xo : slots + (size_t)(2 * (depth - 1) + (node & 1)) * n;
                rt_combine<T, KIND>(w1, w2, o, n, depth, 0, F, qs, tid, NT);
            }
            if (node == 1) break;
            ++node;                                                    // a left child is complete: on to its sibling
        }
    }
}

inline int drs_table(bool ac, const double *x, double *y, int64_t n, int L, int64_t b, const double *q, int F, void *s)
{ return ac ? wx_acwpd1d_f64(x, y, n, L, b, q, F, s) : wx_swpd1d_f64(x, y, n, L, b, q, F, s); }
inline int drs_table(bool ac, const float *x, float *y, int64_t n, int L, int64_t b, const double *q, int F, void *s)
{ return ac ? wx_set_error(WX_EUNSUPPORTED, "the autocorrelation transforms are Float64 only") : wx_swpd1d_f32(x, y, n, L, b, q, F, s); }
inline int drs_denoise(bool ac, const double *xw, double *out, int64_t n, int64_t ncols, const uint8_t *t, int64_t nt, int64_t nb, const double *q, int F,
                       int kind, double scale, const double *thr, int64_t nthr, int us, double *sigma, void *s)
{
    if (ac) return wx_denoise_acwpd1d_trees_f64(xw, out, n, ncols, t, nt, nb, kind, scale, thr, nthr, us, sigma, s);
    return wx_denoise_swpd1d_trees_f64(xw, out, n, ncols, t, nt, nb, q, F, kind, scale, thr, nthr, us, sigma, s);
}
inline int drs_denoise(bool ac, const float *xw, float *out, int64_t n, int64_t ncols, const uint8_t *t, int64_t nt, int64_t nb, const double *q, int F,
                       int kind, double scale, const float *thr, int64_t nthr, int us, float *sigma, void *s)
{
    if (ac) return wx_set_error(WX_EUNSUPPORTED, "the autocorrelation transforms are Float64 only");
    return wx_denoise_swpd1d_trees_f32(xw, out, n, ncols, t, nt, nb, q, F, kind, scale, thr, nthr, us, sigma, s);
}

// what the driver (wx_trees_host.h) needs to know of the signals and of the denoising arguments that travel with them
template <typename T> struct DrsShape {
    int64_t n, L, batch;
    bool ac, has_filter, has_out;
    int th_kind;
    double scale;
    const T *thr;
    int64_t nthr;
    int undersmooth;
    T *sigma;
    mutable const T *dthr = nullptr;                                  // stage(): thr and sigma as device pointers
    mutable T *dsigma = nullptr;
    mutable int route = RB_ROUTE_NONE;                                // the way the call went
    static constexpr bool quad = false;
    static constexpr bool extras = true;
    static constexpr bool table = true;                                // the depth L bounds the trees, whatever the mode
    static constexpr bool by_chunks = true;                            // no single-tree entry takes signals: chunks through the table entries
    bool dims_ok() const { return n >= 1; }
    int64_t count() const { return n; }
    int64_t in_count() const { return n; }
    int tree_k() const { return (int)L + 1; }                          // a column of depth >= this decomposes a node of depth >= L
    int too_deep() const { return wx_set_error(WX_EBOUNDS, "tree decomposes a node of depth >= L"); }
    int check(bool, int, int64_t ntree) const
    {
        WX_REQUIRE(has_filter, WX_EARG, "denoiseall(signals, trees): NULL filter");
        WX_REQUIRE(th_kind >= 0 && th_kind <= 3, WX_EARG, "th_kind: 0 HardTH, 1 SoftTH, 2 SemiSoftTH, 3 SteinTH");
        WX_REQUIRE(nthr == 0 || nthr == 1 || nthr == batch, WX_EARG, "no threshold (the noise is estimated), one, or one per signal");
        WX_REQUIRE((thr != nullptr) == (nthr != 0) || batch == 0, WX_EARG, "thr and nthr disagree");
        WX_REQUIRE(has_out || sigma != nullptr || batch == 0, WX_EARG, "denoiseall(signals, trees): neither xhat nor sigma");
        WX_REQUIRE(wx_isdyadic(n), WX_EASSERT, "maketree/isvalidtree: signal length must be dyadic (Wavelets.jl)");
        WX_REQUIRE(L >= 0 && L <= wx_maxtransformlevels(n), WX_EASSERT, "swpd / acwpd: @assert 0 <= L <= maxtransformlevels(x)");
        WX_REQUIRE(ntree == n - 1, WX_EASSERT, "@assert n_t == gettreelength(sz...) (Utils.jl:211)");
        WX_REQUIRE(n < ((int64_t)1 << 30), WX_EUNSUPPORTED, "denoiseall(signals, trees): signal length >= 2^30 not supported");
        return WX_OK;
    }
    int check_host(const uint8_t *trees, int64_t ntree, int64_t nb, int k, uint32_t *bits, int nw, uint8_t *depths, bool *same) const
    { return wx_trees_check_host(false, n, 1, trees, ntree, nb, k, -1, bits, nw, depths, same); }
    template <typename U> bool window(int64_t, int F) const { return rb_window(n, (int)L, F, sizeof(T), RB_DENOISE); }
    bool stage(WxIO &io, int64_t nb) const
    {
        dthr = thr ? (const T *)io.in(thr, sizeof(T) * nthr) : nullptr;
        dsigma = sigma ? (T *)io.out(sigma, sizeof(T) * nb) : nullptr;
        return (dthr || !thr) && (dsigma || !sigma);
    }
    template <typename U, int MODE>
    hipError_t launch(const T *dx, T *dy, int64_t, int, int64_t nb, const uint32_t *dt, const uint8_t *, const WxFilt &filt, hipStream_t st) const
    {
        const size_t all = rb_lds(n, (int)L, sizeof(T), RB_DENOISE), bytes = all - 16;   // the estimate's word is static
        const int nt = rb_threads(n);
        int log2n = 0;
        while (((int64_t)1 << log2n) < n) ++log2n;
        const int per = nthr == nb && nb > 1 ? 1 : 0;
        WxFilt kf = filt;
        double c1 = 0.0;
        if (ac) {
            WxAcFilt acf;
            wx_pack_acfilter(filt, &acf);
            for (int i = 0; i < WX_MAXF; ++i) kf.q[i] = acf.b[i];
            c1 = acf.c1;
        }
        auto go = [&](auto kern) -> hipError_t {
            hipError_t e = hipSuccess;
            if (bytes > 48 * 1024) e = hipFuncSetAttribute(reinterpret_cast<const void *>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes);
            if (e != hipSuccess) return e;
            hipLaunchKernelGGL(kern, dim3(rb_grid(n, (int)L, sizeof(T), RB_DENOISE, nb)), dim3(nt), bytes, st, dx, dy, log2n, (int)L, nb, dt, kf, c1,
                               th_kind, scale, dthr, per, undersmooth, dsigma);
            return hipGetLastError();
        };
        route = RB_ROUTE_FUSED;
        if constexpr (sizeof(T) == 8)
            if (ac) return go(k_denoise_red_sig<T, true>);
        return go(k_denoise_red_sig<T, false>);
    }
    // outside the window: the checked batch (trees in host memory) in chunks of signals through the table entries
    int chunked(const T *x, T *y, const uint8_t *trees, int64_t ntree, int64_t nb, const double *qmf, int F, void *stream) const
    {
        auto part = [&](const T *tab, int64_t ncols, int64_t b0, int64_t cnt) {
            return drs_denoise(ac, tab, y ? y + b0 * n : y, n, ncols, trees + b0 * ntree, ntree, cnt, qmf, F, th_kind, scale,
                               thr ? (nthr == nb && nb > 1 ? thr + b0 : thr) : thr, thr ? (nthr == nb && nb > 1 ? cnt : 1) : 0, undersmooth,
                               sigma ? sigma + b0 : sigma, stream);
        };
        if (L == 0) {                                                  // bare roots only: the signal is its own one-column table
            route = RB_ROUTE_TRIVIAL;
            return part(x, 1, 0, nb);
        }
        route = RB_ROUTE_CHUNKED;
        const int64_t ncols = ((int64_t)2 << L) - 1;
        const size_t sig_table = sizeof(T) * (size_t)n * (size_t)ncols;
        int64_t per = (int64_t)(RB_CHUNK_TABLE_BYTES / sig_table);
        if (per < 1) per = 1;
        if (per > nb) per = nb;
        WxScratch scr(wx_stream(stream));
        T *tab = (T *)scr.alloc(sig_table * (size_t)per);
        if (!tab) return WX_EHIP;
        for (int64_t b0 = 0; b0 < nb; b0 += per) {
            const int64_t cnt = nb - b0 < per ? nb - b0 : per;
            int rc = drs_table(ac, x + b0 * n, tab, n, (int)L, cnt, qmf, F, stream);
            if (rc == WX_OK) rc = part(tab, ncols, b0, cnt);
            if (rc) return rc;
        }
        return WX_OK;
    }
};

template <typename T>
int api_denoise_red_sig(bool ac, const T *x, T *out, int64_t n, int64_t L, const uint8_t *trees, int64_t ntree, int64_t batch, const double *qmf,
                        int F, int th_kind, double scale, const T *thr, int64_t nthr, int undersmooth, T *sigma, void *stream)
{
    wx_red_bb_route_set(RB_ROUTE_NONE);
    WX_REQUIRE(batch <= 0 || x != nullptr, WX_EARG, "denoiseall(signals, trees): NULL signals");
    const DrsShape<T> s{n, L, batch, ac, qmf != nullptr, out != nullptr, th_kind, scale, thr, nthr, undersmooth, sigma};
    const int rc = wx_trees_api<T, WX_TREES_INV>(s, x, out, 1, trees, ntree, batch, qmf, F, stream);
    if (rc == WX_OK) wx_red_bb_route_set(batch == 0 ? RB_ROUTE_TRIVIAL : s.route);
    return rc;
}

}  // namespace

extern "C" {

int wx_denoise_swpd1d_sig_trees_f64(const double *x, double *out, int64_t n, int64_t L, const uint8_t *trees, int64_t ntree, int64_t batch,
                                    const double *qmf, int F, int th_kind, double scale, const double *thr, int64_t nthr, int undersmooth,
                                    double *sigma, void *stream)
{ return api_denoise_red_sig<double>(false, x, out, n, L, trees, ntree, batch, qmf, F, th_kind, scale, thr, nthr, undersmooth, sigma, stream); }
int wx_denoise_swpd1d_sig_trees_f32(const float *x, float *out, int64_t n, int64_t L, const uint8_t *trees, int64_t ntree, int64_t batch,
                                    const double *qmf, int F, int th_kind, double scale, const float *thr, int64_t nthr, int undersmooth,
                                    float *sigma, void *stream)
{ return api_denoise_red_sig<float>(false, x, out, n, L, trees, ntree, batch, qmf, F, th_kind, scale, thr, nthr, undersmooth, sigma, stream); }
int wx_denoise_acwpd1d_sig_trees_f64(const double *x, double *out, int64_t n, int64_t L, const uint8_t *trees, int64_t ntree, int64_t batch,
                                     const double *qmf, int F, int th_kind, double scale, const double *thr, int64_t nthr, int undersmooth,
                                     double *sigma, void *stream)
{ return api_denoise_red_sig<double>(true, x, out, n, L, trees, ntree, batch, qmf, F, th_kind, scale, thr, nthr, undersmooth, sigma, stream); }

}  // extern "C"
