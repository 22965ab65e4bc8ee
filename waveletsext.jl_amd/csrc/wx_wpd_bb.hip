// wx_wpd_bb.hip -- per-signal best bases straight from the signals: wpd, entropy costs and tree selection in one kernel.
//   wpd levels                     dwt/dwt_one_level.jl:79-107 (dwt_step!, one periodic decimated analysis step per node)
//   tree_costs(X, ::BB)            bestbasis/bestbasis_tree.jl:210-233
//   coefcost(x, ::BBCost, nrm)     bestbasis/bestbasis_costs.jl:104-124 (wx_bbcost.h)
//   bestbasis_treeselection        BestBasis.jl:59-83 (wx_bb_select.h)
//   bestbasistreeall(X, ::BB)      BestBasis.jl:253-262  (the batch loop: one tree per signal)
// bestbasistreeall(wpdall(x, wt, L), BB()) reads the (n, L+1, N) packet table once and keeps n - 1 bytes per signal.  Here the table is
// never written: a workgroup takes a signal and strides over the batch, every level of the signal lives in LDS only as long as its
// costs and the next level are being computed from it, and the n - 1 tree bytes (and, on request, the 2^(L+1) - 1 costs) are all that
// leaves for HBM.
//
// Kernel (k_wpd_bb), per signal:
//   load      x[:, b] with 16-byte loads into buffer 0, sum x^2 in Float64 (fma) on the way; nrm = (T)sqrt(sum) like k_bb_costs1d_wave.
//             nrm == 0: every cost is 0 and the tree all false (bestbasis_costs.jl:119), the signal is done.
//   level d   ONE barrier interval holds the cost terms of level d (bb_term of every coefficient, Float64 partials) and the analysis step
//             d -> d + 1 into the other buffer: both only read level d.  A node of the buffers is stored even samples first like
//             k_wpt_trees' (wx_wpt_trees.hip): the taps of neighbouring lanes are neighbours in LDS, the wrap is a true modulo (a mask:
//             nodes are dyadic), so nodes shorter than the filter, down to one sample, need nothing special.  The permutation stays inside a
//             node, which is all a node's cost sees.
//   sums      nodes of < 64 coefficients: butterfly over the node's lanes, its first lane stores the cost.  Longer nodes: every
//             wavefront leaves the sum of its 64 coefficients in LDS, and in the NEXT interval (the list alternates between two
//             halves) one lane per 64-chunk folds the chunks of a node with a second butterfly.  Every sum has a fixed order: repeated
//             calls give the same bits.
//   select    the two sweeps of wx_bb_select.h on the LDS costs, after the unmutated costs have left for HBM if the caller wants them.
// No atomics, one writer per output byte, barriers in uniform control flow only (every loop bound and every branch around a barrier
// depends on kernel arguments and on the norm, which all lanes read from the same LDS word).  Arithmetic of the analysis step: Float64
// accumulators for either element type, like the one-level kernels of wx_dwt1d.hip and k_wpt_trees.
//
// Window of the kernel: dyadic 8 <= n, even filters of 2 .. 20 taps, and WPB_LDS_MAX = 160 KiB (one workgroup per CU) for
//   64 doubles of taps | 2 x max(n/64, 1) + 16 doubles of partial sums | two level buffers | 2^(L+1) - 1 costs | as many flag bytes
// Float64 n = 4096, L = 12: 137.6 KiB; n = 8192 fits at partial depth only (L <= 10); Float32 reaches n = 8192 at full depth.
// Outside the window (route 2) the host loops over chunks of signals: wx_wpd1d_* into scratch, wx_bb_costs_*, wx_treeselect_batch_*,
// the chunk sized so that its table stays under WPB_CHUNK_TABLE_BYTES (one signal's table if that alone is larger).
#include "../../include/waveletsext_hip.h"     // the definitions below must match the public prototypes
#include "wx_common.h"
#include "wx_host.h"
#include "wx_bbcost.h"
#include "wx_bb_select.h"
#include "wx_debug.h"
#include "wx_trees_host.h"                     // wx_trees_threads, wx_trees_grid: the launch geometry of the per-signal-tree kernels

#undef WX_REQUIRE
#define WX_REQUIRE(cond, code, msg) \
    do { if (!(cond)) return wx_set_error(code, msg); } while (0)

namespace {

constexpr size_t WPB_LDS_MAX = 160 * 1024;
constexpr size_t WPB_CHUNK_TABLE_BYTES = (size_t)256 << 20;      // route 2: packet table of one chunk of signals
constexpr int WPB_RED = 16;                                      // wavefronts of a workgroup, at most

enum { WPB_ROUTE_NONE = 0, WPB_ROUTE_FUSED = 1, WPB_ROUTE_CHUNKED = 2, WPB_ROUTE_TRIVIAL = 3 };
thread_local int g_wpb_route = WPB_ROUTE_NONE;

template <typename T> struct WpbVec;
template <> struct WpbVec<double> { typedef double2 type; static constexpr int W = 2; };
template <> struct WpbVec<float> { typedef float4 type; static constexpr int W = 4; };

__device__ __forceinline__ double wpb_wave_sum(double v, int width)
{
    for (int w = width >> 1; w > 0; w >>= 1) v += __shfl_xor(v, w, 64);
    return v;
}

// x: (n, batch); trees: (n - 1, batch) bytes; costs: nullptr or (2^(L+1) - 1, batch).  1 <= L <= log2n, n >= 8.
template <typename T>
__global__ __launch_bounds__(1024) void k_wpd_bb(const T *__restrict__ x, int log2n, int L, int64_t batch, int cost_kind,
                                                 uint8_t *__restrict__ trees, T *__restrict__ costs, WxFilt filt)
{
    extern __shared__ __attribute__((aligned(16))) char wpb_smem[];
    typedef typename WpbVec<T>::type VW;
    constexpr int W = WpbVec<T>::W;
    const int n = 1 << log2n, half = n >> 1, ntree = n - 1;
    const int ncost = (2 << L) - 1;
    const int nch = n >= 64 ? n >> 6 : 1;                              // 64-coefficient chunks of a level
    double *qs = reinterpret_cast<double *>(wpb_smem);
    double *red = qs + WX_MAXF;                                        // WPB_RED wavefront sums of x^2
    double *wpart = red + WPB_RED;                                     // two lists of nch chunk sums
    T *buf0 = reinterpret_cast<T *>(wpart + 2 * nch);
    T *buf1 = buf0 + n;
    T *c = buf1 + n;
    uint8_t *flag = reinterpret_cast<uint8_t *>(c + ncost);
    const int tid = threadIdx.x, NT = blockDim.x, F = filt.F;
    const int lane = tid & 63, wave = tid >> 6, nwave = NT >> 6;
    if (tid == 0)
        for (int i = 0; i < F; ++i) qs[i] = filt.q[i];                 // read below as LDS broadcasts

    for (int64_t b = blockIdx.x; b < batch; b += gridDim.x) {
        const T *xs = x + b * (int64_t)n;
        uint8_t *tout = trees + b * (int64_t)ntree;
        T *cout = costs ? costs + b * (int64_t)ncost : nullptr;
        __syncthreads();                                               // the previous signal's selection is done with costs, flags and sums
        double a2 = 0.0;
        for (int i = tid; i < n / W; i += NT) {
            const VW v = *reinterpret_cast<const VW *>(xs + W * i);
            const T *ve = reinterpret_cast<const T *>(&v);
#pragma unroll
            for (int e = 0; e < W; ++e) {                              // sample s of the root at (s & 1) * n / 2 + s / 2: even samples first
                const int s = W * i + e;
                buf0[(s & 1) * half + (s >> 1)] = ve[e];
                const double dv = (double)ve[e];
                a2 = fma(dv, dv, a2);
            }
        }
        a2 = wpb_wave_sum(a2, 64);
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
        T *cur = buf0, *nxt = buf1;
        for (int d = 0; d <= L; ++d) {
            const int lsh = log2n - d;                                 // log2 of the node length
            const int cnt = 1 << lsh;
            // chunk sums of level d - 1, left by the previous interval: one lane per chunk, `per` chunks to a node
            if (d > 0 && lsh + 1 >= 6) {
                const int per = (cnt << 1) >> 6;
                const double *wp = wpart + ((d - 1) & 1) * nch;
                T *o = c + ((1 << (d - 1)) - 1);
                for (int c0 = wave * 64; c0 < nch; c0 += NT) {         // whole wavefronts: every lane of one joins the butterfly
                    const int ch = c0 + lane;
                    double w = ch < nch ? wp[ch] : 0.0;
                    if (per <= 64) {
                        w = wpb_wave_sum(w, per);
                        if (ch < nch && (ch & (per - 1)) == 0) o[ch / per] = (T)w;
                    } else if (ch < nch && (ch & (per - 1)) == 0) {    // n > 4096 at the top levels: a few lanes add their node's chunks
                        double t = 0.0;
                        for (int q = 0; q < per; ++q) t += wp[ch + q];
                        o[ch / per] = (T)t;
                    }
                }
            }
            // cost terms of level d
            {
                double *wp = wpart + (d & 1) * nch;
                T *o = c + ((1 << d) - 1);
                for (int p0 = 0; p0 < n; p0 += NT) {
                    const int p = p0 + tid;
                    double v = p < n ? bb_term<T>(cur[p], nrw, cost_kind) : 0.0;
                    if (cnt >= 64) {
                        v = wpb_wave_sum(v, 64);
                        if (lane == 0) wp[p >> 6] = v;
                    } else {
                        v = wpb_wave_sum(v, cnt);
                        if (p < n && (lane & (cnt - 1)) == 0) o[p >> lsh] = (T)v;
                    }
                }
            }
            // analysis step d -> d + 1 (k_wpt_trees, every node decomposed): item i is output pair t of node j
            if (d < L) {
                const int h = cnt >> 1, msk = h - 1;
                for (int i = tid; i < half; i += NT) {
                    const int p = 2 * i, j = p >> lsh, base = j << lsh, t = i - (base >> 1);
                    const T *v = cur + base;
                    double a = 0.0, dd = 0.0;
                    for (int u = 0; u < F; ++u) {                      // a: v[(2t + u) mod np], d: v[(2t + 1 - u) mod np]
                        const double q = qs[u];
                        const int par = (u & 1) * h;
                        a = fma(q, (double)v[par + ((t + (u >> 1)) & msk)], a);
                        dd = fma((u & 1) ? -q : q, (double)v[(h - par) + ((t - (u >> 1)) & msk)], dd);
                    }
                    T *o = nxt + base + (t & 1) * (h >> 1) + (t >> 1);
                    o[0] = (T)a;
                    o[h] = (T)dd;
                }
            }
            __syncthreads();
            T *tmp = cur; cur = nxt; nxt = tmp;
        }
        // chunk sums of level L
        if (log2n - L >= 6) {
            const int per = (n >> L) >> 6;
            const double *wp = wpart + (L & 1) * nch;
            T *o = c + ((1 << L) - 1);
            for (int c0 = wave * 64; c0 < nch; c0 += NT) {
                const int ch = c0 + lane;
                double w = ch < nch ? wp[ch] : 0.0;
                if (per <= 64) {
                    w = wpb_wave_sum(w, per);
                    if (ch < nch && (ch & (per - 1)) == 0) o[ch / per] = (T)w;
                } else if (ch < nch && (ch & (per - 1)) == 0) {
                    double t = 0.0;
                    for (int q = 0; q < per; ++q) t += wp[ch + q];
                    o[ch / per] = (T)t;
                }
            }
            __syncthreads();                                           // uniform: kernel arguments only
        }
        if (cout) {                                                    // before the selection folds children into parents
            for (int i = tid; i < ncost; i += NT) cout[i] = c[i];
            __syncthreads();                                           // uniform (a kernel argument): no lane folds a cost another still copies
        }
        bb_select_sweeps<T, 2>(c, flag, L, 0, tid, NT, [] { __syncthreads(); });
        const int nfull = (1 << L) - 1;
        for (int i = tid; i < ntree; i += NT) tout[i] = i < nfull ? flag[i] : 0;
    }
}

template <typename T> size_t wpb_lds(int64_t n, int L)
{
    const size_t ncost = ((size_t)2 << L) - 1;
    const size_t nch = n >= 64 ? (size_t)(n >> 6) : 1;
    const size_t b = sizeof(double) * (WX_MAXF + WPB_RED + 2 * nch) + 2 * (size_t)n * sizeof(T) + ncost * (sizeof(T) + 1);
    return (b + 15) & ~(size_t)15;
}

template <typename T> bool wpb_window(int64_t n, int L, int F)
{
    if (!wx_isdyadic(n) || n < 8 || n > ((int64_t)1 << 20) || F < 2 || F > 20 || (F & 1)) return false;
    return wpb_lds<T>(n, L) <= WPB_LDS_MAX;
}

// workgroups of a launch: as many as stay resident, never more than signals
template <typename T> int wpb_grid(int64_t n, int L, int64_t batch) { return wx_trees_grid(wpb_lds<T>(n, L), wx_trees_threads(n), batch); }

int need_device()
{
    if (wx_device_count() < 1) return wx_set_error(WX_EHIP, "no HIP device visible: the MI355X kernels cannot run");
    return WX_OK;
}

inline int wpd1d(const double *x, double *y, int64_t n, int L, int64_t b, const double *q, int F, void *s) { return wx_wpd1d_f64(x, y, n, L, b, q, F, s); }
inline int wpd1d(const float *x, float *y, int64_t n, int L, int64_t b, const double *q, int F, void *s) { return wx_wpd1d_f32(x, y, n, L, b, q, F, s); }
inline int bbcosts(const double *X, double *c, int64_t n, int64_t k, int64_t b, int kind, void *s) { return wx_bb_costs_f64(X, c, n, k, b, 0, kind, s); }
inline int bbcosts(const float *X, float *c, int64_t n, int64_t k, int64_t b, int kind, void *s) { return wx_bb_costs_f32(X, c, n, k, b, 0, kind, s); }
inline int treesel(double *c, int64_t nc, int64_t n, int64_t b, uint8_t *t, void *s) { return wx_treeselect_batch_f64(c, nc, n, 0, 0, b, t, s); }
inline int treesel(float *c, int64_t nc, int64_t n, int64_t b, uint8_t *t, void *s) { return wx_treeselect_batch_f32(c, nc, n, 0, 0, b, t, s); }

template <typename T>
int api_wpd_bbtrees(const T *x, int64_t n, int64_t L, int64_t batch, const double *qmf, int F, int cost_kind, uint8_t *trees, T *costs,
                    void *stream)
{
    g_wpb_route = WPB_ROUTE_NONE;
    // argument errors are reported before any device is needed
    WxFilt filt;
    int rc = wx_pack_filter(qmf, F, &filt);
    if (rc) return rc;
    WX_REQUIRE(n >= 1 && batch >= 0, WX_EARG, "wpd_bbtrees: bad dimensions");
    WX_REQUIRE(cost_kind == 0 || cost_kind == 1, WX_EARG, "cost_kind must be 0 (ShannonEntropyCost) or 1 (LogEnergyEntropyCost)");
    WX_REQUIRE(batch == 0 || (x && trees), WX_EARG, "NULL argument");
    WX_REQUIRE(wx_isdyadic(n), WX_EASSERT, "maketree(n, L, :full): signal length must be dyadic (Wavelets.jl)");
    WX_REQUIRE(L >= 0 && L <= wx_maxtransformlevels(n), WX_EASSERT, "wpd: @assert 0 <= L <= maxtransformlevels(x)");
    WX_REQUIRE(n < ((int64_t)1 << 30) && L <= 29, WX_EUNSUPPORTED, "wpd_bbtrees: signal length >= 2^30 not supported");
    if (batch == 0) { g_wpb_route = WPB_ROUTE_TRIVIAL; return WX_OK; }
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
            if (e != hipSuccess) return io.finish(wx_set_hip_error(e, "wpd_bbtrees: clearing the trees", __FILE__, __LINE__));
        }
        if (dc && (rc = bbcosts(dx, dc, n, 1, batch, cost_kind, stream))) return io.finish(rc);
        rc = io.finish(WX_OK);
        if (rc == WX_OK) g_wpb_route = WPB_ROUTE_TRIVIAL;
        return rc;
    }
    if (wpb_window<T>(n, (int)L, F)) {
        const size_t bytes = wpb_lds<T>(n, (int)L);
        const int nt = wx_trees_threads(n);
        auto kern = k_wpd_bb<T>;
        if (bytes > 64 * 1024) {
            const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void *>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes);
            if (e != hipSuccess) return io.finish(wx_set_hip_error(e, "wpd_bbtrees: hipFuncSetAttribute(LDS)", __FILE__, __LINE__));
        }
        int log2n = 0;
        while (((int64_t)1 << log2n) < n) ++log2n;
        hipLaunchKernelGGL(kern, dim3(wpb_grid<T>(n, (int)L, batch)), dim3(nt), bytes, st, dx, log2n, (int)L, batch, cost_kind, dt, dc, filt);
        const hipError_t e = hipGetLastError();
        if (e != hipSuccess) return io.finish(wx_set_hip_error(e, "wpd_bbtrees launch", __FILE__, __LINE__));
        rc = io.finish(WX_OK);
        if (rc == WX_OK) g_wpb_route = WPB_ROUTE_FUSED;
        return rc;
    }
    // outside the window: chunks of signals through the table kernels, the table of one chunk at most WPB_CHUNK_TABLE_BYTES
    const size_t sig_table = sizeof(T) * (size_t)n * (size_t)(L + 1);
    int64_t per = (int64_t)(WPB_CHUNK_TABLE_BYTES / sig_table);
    if (per < 1) per = 1;
    if (per > batch) per = batch;
    WxScratch scr(st);
    T *tab = (T *)scr.alloc(sig_table * (size_t)per);
    T *cs = (T *)scr.alloc(sizeof(T) * (size_t)ncost * per);          // the selection mutates its costs: never the caller's
    if (!tab || !cs) return io.finish(WX_EHIP);
    for (int64_t b0 = 0; b0 < batch; b0 += per) {
        const int64_t nb = batch - b0 < per ? batch - b0 : per;
        if ((rc = wpd1d(dx + b0 * n, tab, n, (int)L, nb, qmf, F, stream))) return io.finish(rc);
        if ((rc = bbcosts(tab, cs, n, L + 1, nb, cost_kind, stream))) return io.finish(rc);
        if (dc) {
            const hipError_t e = hipMemcpyAsync(dc + b0 * ncost, cs, sizeof(T) * (size_t)ncost * nb, hipMemcpyDeviceToDevice, st);
            if (e != hipSuccess) return io.finish(wx_set_hip_error(e, "wpd_bbtrees: costs of a chunk", __FILE__, __LINE__));
        }
        if ((rc = treesel(cs, ncost, n, nb, dt + b0 * ntree, stream))) return io.finish(rc);
    }
    rc = io.finish(WX_OK);
    if (rc == WX_OK) g_wpb_route = WPB_ROUTE_CHUNKED;
    return rc;
}

}  // namespace

extern "C" {
int wx_wpd_bbtrees_f64(const double *x, int64_t n, int64_t L, int64_t batch, const double *qmf, int F, int cost_kind, uint8_t *trees,
                       double *costs, void *stream)
{ return api_wpd_bbtrees<double>(x, n, L, batch, qmf, F, cost_kind, trees, costs, stream); }
int wx_wpd_bbtrees_f32(const float *x, int64_t n, int64_t L, int64_t batch, const double *qmf, int F, int cost_kind, uint8_t *trees,
                       float *costs, void *stream)
{ return api_wpd_bbtrees<float>(x, n, L, batch, qmf, F, cost_kind, trees, costs, stream); }
int wx_wpd_bb_last_route(void) { return g_wpb_route; }
int wx_debug_wpd_bb_grid(int64_t n, int L, int F, int elem_size, int64_t batch)
{
    if (L < 1 || batch < 1 || n < 1 || L > wx_maxtransformlevels(n)) return 0;
    if (elem_size == 8) return wpb_window<double>(n, L, F) ? wpb_grid<double>(n, L, batch) : 0;
    return elem_size == 4 && wpb_window<float>(n, L, F) ? wpb_grid<float>(n, L, batch) : 0;
}
}
