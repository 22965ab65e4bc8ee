// wx_red_bb.hip -- per-signal best bases of the REDUNDANT packet decompositions straight from the signals: swpd / acwpd, entropy costs
// and tree selection in one kernel.
//   sdwt_step!                     swt/swt_one_level.jl:99-127   (one stationary analysis step of a node at depth d, dilation 2^d)
//   acdwt_step!                    acwt/acwt_one_level.jl:101-128 (the autocorrelation step; filters of acwt_utils.jl:7-72)
//   swpd / acwpd                   SWT.jl:840-868, ACWT.jl:733-759 (the heap-ordered (n, 2^(L+1)-1) table these steps fill)
//   tree_costs(X, BB(redundant))   bestbasis/bestbasis_tree.jl:210-233 (:215-220 the redundant branch: a node's cost / 2^depth)
//   coefcost(x, ::BBCost, nrm)     bestbasis/bestbasis_costs.jl:104-124 (wx_bbcost.h)
//   bestbasis_treeselection        BestBasis.jl:59-83 (wx_bb_select.h)
//   bestbasistreeall(X, ::BB)      BestBasis.jl:253-262  (the batch loop: one tree per signal)
// bestbasistreeall(swpdall(x, wt, L), BB(redundant = true)) reads a table of 2^(L+1) - 1 columns of n values per signal and keeps n - 1
// bytes of it.  Here the table is never written: a workgroup takes a signal and strides over the batch; the n - 1 tree bytes (and, on
// request, the 2^(L+1) - 1 costs) are all that leaves for HBM.
//
// Kernel (k_red_bb<T, AC>), per signal:
//   load      x[:, b] into column 0 of LDS, sum x^2 in Float64 (fma) on the way; nrm = (T)sqrt(sum) like k_wpd_bb.
//             nrm == 0: every cost is 0 and the tree all false (bestbasis_costs.jl:119), the signal is done.
//   walk      the full tree of depth L, depth first.  A node is a whole column of n values, so a level does not fit in LDS; a
//             root-to-node path does.  LDS holds the root and TWO columns per depth 1 .. L: expanding a node writes both children
//             in ONE barrier interval, one lane per position, and the lane sums the cost terms of the two values it has just rounded to
//             T from its registers.  The right child waits in its slot while the left subtree is walked (deeper slots only).  The
//             walk's state is the heap index and the depth, functions of kernel arguments alone: every barrier sits in uniform
//             control flow.
//   costs     lane partials in a fixed order, a butterfly over the wavefront, one Float64 partial per wavefront in LDS; behind the
//             interval's barrier lanes 0 and 1 add the wavefronts' partials in order and store (T)((T)tot / (T)2^depth) at heap
//             position i - 1: the arithmetic of k_bb_costs1d's redundant branch (wx_bb.hip).  The partials alternate between two
//             lists, so the next interval never overwrites what lanes 0 and 1 still read.
//   select    the two sweeps of wx_bb_select.h on the LDS costs, after the unmutated costs have left for HBM if the caller wants them.
// Steps, s = 2^d, positions wrapped by true modulo (a mask: n is dyadic), so columns shorter than the filter need nothing special:
//   stationary       a[i] = sum_j q[j] v[i + (j - 1) s],  d[i] = sum_j (-1)^j q[j] v[i - j s], the reference's tap order, Float64
//                    accumulators with fma -- the arithmetic of k_swt_fwd_level (wx_swt1d.hip);
//   autocorrelation  w1 = v / sqrt2 + S, w2 = v / sqrt2 - S, S = sum over the odd lags l of b_l (v[i - l s] + v[i + l s]): the 2F - 1
//                    taps of make_acreverseqmfpair with the even lags, which are exactly zero, skipped (k_swt_fwd_level).  Float64 only.
// No atomics, one writer per output byte, every sum in a fixed order: repeated calls give the same bits.
//
// Window of the kernel: dyadic 8 <= n, even filters of 2 .. 20 taps, and RB_LDS_MAX = 160 KiB (one workgroup per CU at the top) for
//   64 doubles of taps | 16 + 64 doubles of partial sums | 2 L + 1 columns | 2^(L+1) - 1 costs | as many flag bytes
// Float64 takes every depth up to n = 512 and depth 8 at n = 1024 (141.6 KiB); Float32 depth 10 at n = 1024 (95 KiB).
// Outside the window (route 2) the host loops over chunks of signals: wx_swpd1d_* / wx_acwpd1d_f64 into scratch, wx_bb_costs_*
// (redundant), wx_treeselect_batch_*, the chunk sized so that its table stays under RB_CHUNK_TABLE_BYTES (one signal's table if that alone
// is larger).  The whole table is never allocated.
#include "../../include/waveletsext_hip.h"     // the definitions below must match the public prototypes
#include "wx_common.h"
#include "wx_host.h"
#include "wx_acfilt.h"
#include "wx_bbcost.h"
#include "wx_bb_select.h"
#include "wx_debug.h"
#include "wx_red_bb.h"                          // rb_step, rb_lds / rb_window / rb_grid, the route record

#define WX_REQUIRE(cond, code, msg) \
    do { if (!(cond)) return wx_set_error(code, msg); } while (0)

static thread_local int g_wx_red_bb_route = RB_ROUTE_NONE;
void wx_red_bb_route_set(int route) { g_wx_red_bb_route = route; }

namespace {

__device__ __forceinline__ double rb_wave_sum(double v)
{
    for (int w = 32; w > 0; w >>= 1) v += __shfl_xor(v, w, 64);
    return v;
}

// x: (n, batch); trees: (n - 1, batch) bytes; costs: nullptr or (2^(L+1) - 1, batch).  1 <= L <= log2n, n >= 8.
// filt: the QMF (stationary), or b_l at q[l - 1] with F the length of the generating QMF (autocorrelation, c1 = 1 / sqrt2).
template <typename T, bool AC>
__global__ __launch_bounds__(1024) void k_red_bb(const T *__restrict__ x, int log2n, int L, int64_t batch, int cost_kind,
                                                 uint8_t *__restrict__ trees, T *__restrict__ costs, WxFilt filt, double c1)
{
    extern __shared__ __attribute__((aligned(16))) char rb_smem[];
    const int n = 1 << log2n, msk = n - 1, ntree = n - 1;
    const int ncost = (2 << L) - 1;
    double *qs = reinterpret_cast<double *>(rb_smem);
    double *red = qs + WX_MAXF;                                        // RB_RED wavefront sums of x^2
    double *part = red + RB_RED;                                       // [list 0 / 1][left / right child][wavefront]
    T *cols = reinterpret_cast<T *>(part + 4 * RB_RED);                // the root, then child c of a node of depth d - 1 at 1 + 2 (d - 1) + c
    T *c = cols + (size_t)(2 * L + 1) * n;
    uint8_t *flag = reinterpret_cast<uint8_t *>(c + ncost);
    const int tid = threadIdx.x, NT = blockDim.x, F = filt.F;
    const int lane = tid & 63, wave = tid >> 6, nwave = NT >> 6;
    if (tid == 0)
        for (int i = 0; i < (AC ? F - 1 : F); ++i) qs[i] = filt.q[i];  // read below as LDS broadcasts

    for (int64_t b = blockIdx.x; b < batch; b += gridDim.x) {
        const T *xs = x + b * (int64_t)n;
        uint8_t *tout = trees + b * (int64_t)ntree;
        T *cout = costs ? costs + b * (int64_t)ncost : nullptr;
        __syncthreads();                                               // the previous signal's selection is done with costs, flags and sums
        double a2 = 0.0;
        for (int i = tid; i < n; i += NT) {
            const T v = xs[i];
            cols[i] = v;
            const double dv = (double)v;
            a2 = fma(dv, dv, a2);
        }
        a2 = rb_wave_sum(a2);
        if (lane == 0) red[wave] = a2;
        __syncthreads();
        double tot = 0.0;
        for (int w = 0; w < nwave; ++w) tot += red[w];                 // the same order in every lane
        const T nr = (T)sqrt(tot);
        if (nr == (T)0) {                                              // uniform: every lane has read the same sums
            for (int i = tid; i < ntree; i += NT) tout[i] = 0;
            if (cout)
                for (int i = tid; i < ncost; i += NT) cout[i] = (T)0;
            continue;
        }
        const WxNorm<T> nrw(nr);
        // the root's cost: list 0
        {
            double t = 0.0;
            for (int i = tid; i < n; i += NT) t += bb_term<T>(cols[i], nrw, cost_kind);
            t = rb_wave_sum(t);
            if (lane == 0) part[wave] = t;
            __syncthreads();
            if (tid == 0) {
                double s = 0.0;
                for (int w = 0; w < nwave; ++w) s += part[w];
                c[0] = (T)((T)s / (T)1);
            }
        }
        int node = 1, depth = 0, list = 1;                             // scalar: kernel arguments decide the whole walk
        while (true) {
            if (depth < L) {
                // expand: both children of `node` into the slots of depth + 1, their cost terms on the way
                const T *v = node == 1 ? cols : cols + (size_t)(1 + 2 * (depth - 1) + (node & 1)) * n;
                T *lo = cols + (size_t)(1 + 2 * depth) * n, *hi = lo + n;
                const int s = 1 << depth;
                double tl = 0.0, th = 0.0;
                for (int i = tid; i < n; i += NT) {
                    double a, dd;
                    rb_step<T, AC>(v, i, s, msk, F, qs, c1, a, dd);
                    const T ta = (T)a, td = (T)dd;
                    lo[i] = ta;
                    hi[i] = td;
                    tl += bb_term<T>(ta, nrw, cost_kind);
                    th += bb_term<T>(td, nrw, cost_kind);
                }
                tl = rb_wave_sum(tl);
                th = rb_wave_sum(th);
                if (lane == 0) {
                    part[(2 * list + 0) * RB_RED + wave] = tl;
                    part[(2 * list + 1) * RB_RED + wave] = th;
                }
                __syncthreads();                                       // uniform: node, depth and L are scalar
                if (tid < 2) {                                         // heap indices 2 node and 2 node + 1, depth + 1
                    const double *p = part + (2 * list + tid) * RB_RED;
                    double sum = 0.0;
                    for (int w = 0; w < nwave; ++w) sum += p[w];
                    c[2 * node - 1 + tid] = (T)((T)sum / (T)(2 << depth));
                }
                list ^= 1;
                node = 2 * node;
                ++depth;
                continue;
            }
            while (node > 1 && (node & 1)) { node >>= 1; --depth; }    // a right child is done: so is its parent
            if (node == 1) break;
            ++node;                                                    // a left child is done: its sibling waits in its slot
        }
        __syncthreads();                                               // the last costs are in place
        if (cout) {                                                    // before the selection folds children into parents
            for (int i = tid; i < ncost; i += NT) cout[i] = c[i];
            __syncthreads();                                           // uniform (a kernel argument): no lane folds a cost another still copies
        }
        bb_select_sweeps<T, 2>(c, flag, L, 0, tid, NT, [] { __syncthreads(); });
        const int nfull = (1 << L) - 1;
        for (int i = tid; i < ntree; i += NT) tout[i] = i < nfull ? flag[i] : 0;
    }
}

int need_device()
{
    if (wx_device_count() < 1) return wx_set_error(WX_EHIP, "no HIP device visible: the MI355X kernels cannot run");
    return WX_OK;
}

inline int redwpd(bool ac, const double *x, double *y, int64_t n, int L, int64_t b, const double *q, int F, void *s)
{ return ac ? wx_acwpd1d_f64(x, y, n, L, b, q, F, s) : wx_swpd1d_f64(x, y, n, L, b, q, F, s); }
inline int redwpd(bool ac, const float *x, float *y, int64_t n, int L, int64_t b, const double *q, int F, void *s)
{ return ac ? wx_set_error(WX_EUNSUPPORTED, "the autocorrelation transforms are Float64 only") : wx_swpd1d_f32(x, y, n, L, b, q, F, s); }
inline int bbcosts(const double *X, double *c, int64_t n, int64_t k, int64_t b, int kind, void *s) { return wx_bb_costs_f64(X, c, n, k, b, 1, kind, s); }
inline int bbcosts(const float *X, float *c, int64_t n, int64_t k, int64_t b, int kind, void *s) { return wx_bb_costs_f32(X, c, n, k, b, 1, kind, s); }
inline int treesel(double *c, int64_t nc, int64_t n, int64_t b, uint8_t *t, void *s) { return wx_treeselect_batch_f64(c, nc, n, 0, 0, b, t, s); }
inline int treesel(float *c, int64_t nc, int64_t n, int64_t b, uint8_t *t, void *s) { return wx_treeselect_batch_f32(c, nc, n, 0, 0, b, t, s); }

template <typename T, bool AC>
int api_red_bbtrees(const T *x, int64_t n, int64_t L, int64_t batch, const double *qmf, int F, int cost_kind, uint8_t *trees, T *costs,
                    void *stream)
{
    g_wx_red_bb_route = RB_ROUTE_NONE;
    // argument errors are reported before any device is needed
    WxFilt filt;
    int rc = wx_pack_filter(qmf, F, &filt);
    if (rc) return rc;
    WX_REQUIRE(n >= 1 && batch >= 0, WX_EARG, "red_bbtrees: bad dimensions");
    WX_REQUIRE(cost_kind == 0 || cost_kind == 1, WX_EARG, "cost_kind must be 0 (ShannonEntropyCost) or 1 (LogEnergyEntropyCost)");
    WX_REQUIRE(batch == 0 || (x && trees), WX_EARG, "NULL argument");
    WX_REQUIRE(wx_isdyadic(n), WX_EASSERT, "maketree(n, L, :full): signal length must be dyadic (Wavelets.jl)");
    WX_REQUIRE(L >= 0 && L <= wx_maxtransformlevels(n), WX_EASSERT, "swpd / acwpd: @assert 0 <= L <= maxtransformlevels(x)");
    WX_REQUIRE(n < ((int64_t)1 << 30) && L <= 29, WX_EUNSUPPORTED, "red_bbtrees: signal length >= 2^30 not supported");
    if (batch == 0) { g_wx_red_bb_route = RB_ROUTE_TRIVIAL; return WX_OK; }
    if ((rc = need_device())) return rc;
    const int64_t ntree = n - 1, ncost = ((int64_t)2 << L) - 1;
    hipStream_t st = wx_stream(stream);
    WxIO io(st);
    const T *dx = (const T *)io.in(x, sizeof(T) * (size_t)n * batch);
    uint8_t *dt = ntree ? (uint8_t *)io.out(trees, (size_t)ntree * batch) : trees;
    T *dc = costs ? (T *)io.out(costs, sizeof(T) * (size_t)ncost * batch) : nullptr;
    if (!dx || (ntree && !dt) || (costs && !dc)) return io.finish(WX_EHIP);
    if (L == 0) {
        // the root alone: no node is decomposed; its cost is that of a one-column table
        if (ntree) {
            const hipError_t e = hipMemsetAsync(dt, 0, (size_t)ntree * batch, st);
            if (e != hipSuccess) return io.finish(wx_set_hip_error(e, "red_bbtrees: clearing the trees", __FILE__, __LINE__));
        }
        if (dc && (rc = bbcosts(dx, dc, n, 1, batch, cost_kind, stream))) return io.finish(rc);
        rc = io.finish(WX_OK);
        if (rc == WX_OK) g_wx_red_bb_route = RB_ROUTE_TRIVIAL;
        return rc;
    }
    if (rb_window(n, (int)L, F, sizeof(T), RB_TREES)) {
        const size_t bytes = rb_lds(n, (int)L, sizeof(T), RB_TREES);
        const int nt = rb_threads(n);
        auto kern = k_red_bb<T, AC>;
        if (bytes > 48 * 1024) {
            const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void *>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes);
            if (e != hipSuccess) return io.finish(wx_set_hip_error(e, "red_bbtrees: hipFuncSetAttribute(LDS)", __FILE__, __LINE__));
        }
        WxFilt kf = filt;
        double c1 = 0.0;
        if (AC) {
            WxAcFilt acf;
            wx_pack_acfilter(filt, &acf);
            for (int i = 0; i < WX_MAXF; ++i) kf.q[i] = acf.b[i];
            c1 = acf.c1;
        }
        int log2n = 0;
        while (((int64_t)1 << log2n) < n) ++log2n;
        hipLaunchKernelGGL(kern, dim3(rb_grid(n, (int)L, sizeof(T), RB_TREES, batch)), dim3(nt), bytes, st, dx, log2n, (int)L, batch, cost_kind,
                           dt, dc, kf, c1);
        const hipError_t e = hipGetLastError();
        if (e != hipSuccess) return io.finish(wx_set_hip_error(e, "red_bbtrees launch", __FILE__, __LINE__));
        rc = io.finish(WX_OK);
        if (rc == WX_OK) g_wx_red_bb_route = RB_ROUTE_FUSED;
        return rc;
    }
    // outside the window: chunks of signals through the table kernels, the table of one chunk at most RB_CHUNK_TABLE_BYTES
    const size_t sig_table = sizeof(T) * (size_t)n * (size_t)ncost;
    int64_t per = (int64_t)(RB_CHUNK_TABLE_BYTES / sig_table);
    if (per < 1) per = 1;
    if (per > batch) per = batch;
    WxScratch scr(st);
    T *tab = (T *)scr.alloc(sig_table * (size_t)per);
    T *cs = (T *)scr.alloc(sizeof(T) * (size_t)ncost * per);          // the selection mutates its costs: never the caller's
    if (!tab || !cs) return io.finish(WX_EHIP);
    for (int64_t b0 = 0; b0 < batch; b0 += per) {
        const int64_t nb = batch - b0 < per ? batch - b0 : per;
        if ((rc = redwpd(AC, dx + b0 * n, tab, n, (int)L, nb, qmf, F, stream))) return io.finish(rc);
        if ((rc = bbcosts(tab, cs, n, ncost, nb, cost_kind, stream))) return io.finish(rc);
        if (dc) {
            const hipError_t e = hipMemcpyAsync(dc + b0 * ncost, cs, sizeof(T) * (size_t)ncost * nb, hipMemcpyDeviceToDevice, st);
            if (e != hipSuccess) return io.finish(wx_set_hip_error(e, "red_bbtrees: costs of a chunk", __FILE__, __LINE__));
        }
        if ((rc = treesel(cs, ncost, n, nb, dt + b0 * ntree, stream))) return io.finish(rc);
    }
    rc = io.finish(WX_OK);
    if (rc == WX_OK) g_wx_red_bb_route = RB_ROUTE_CHUNKED;
    return rc;
}

}  // namespace

extern "C" {
int wx_swpd_bbtrees_f64(const double *x, int64_t n, int64_t L, int64_t batch, const double *qmf, int F, int cost_kind, uint8_t *trees,
                        double *costs, void *stream)
{ return api_red_bbtrees<double, false>(x, n, L, batch, qmf, F, cost_kind, trees, costs, stream); }
int wx_swpd_bbtrees_f32(const float *x, int64_t n, int64_t L, int64_t batch, const double *qmf, int F, int cost_kind, uint8_t *trees,
                        float *costs, void *stream)
{ return api_red_bbtrees<float, false>(x, n, L, batch, qmf, F, cost_kind, trees, costs, stream); }
int wx_acwpd_bbtrees_f64(const double *x, int64_t n, int64_t L, int64_t batch, const double *qmf, int F, int cost_kind, uint8_t *trees,
                         double *costs, void *stream)
{ return api_red_bbtrees<double, true>(x, n, L, batch, qmf, F, cost_kind, trees, costs, stream); }
int wx_red_bb_last_route(void) { return g_wx_red_bb_route; }
int wx_debug_red_bb_grid(int64_t n, int L, int F, int elem_size, int ac, int which, int64_t batch)
{
    if (L < 1 || batch < 1 || n < 1 || L > wx_maxtransformlevels(n) || (elem_size != 8 && elem_size != 4) || (ac && elem_size != 8)) return 0;
    if (which != RB_TREES && which != RB_DENOISE) return 0;
    return rb_window(n, L, F, (size_t)elem_size, which) ? rb_grid(n, L, (size_t)elem_size, which, batch) : 0;
}
}
