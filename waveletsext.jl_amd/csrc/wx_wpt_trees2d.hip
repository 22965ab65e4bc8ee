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
// The host checks every tree, notes its depth and packs it into bits in the same pass (wx_tree_bits.h: node i is bit i - 1, heap
// order); a tree matrix in DEVICE memory gets the same pass as one launch (wx_trees_prep.hip, quad form).
// Window: both sides dyadic and >= 8, m n <= 8192 (Float64) / 16384 (Float32) -- two buffers and the tree's bits are at
// most 129 of the 160 KiB --, even filters of 2 .. 20 taps.  Outside it the entry calls the single-tree entry once per image (slow,
// correct).  Byte-identical columns go to the single-tree entry whole.
#include "../../include/waveletsext_hip.h"
#include "wx_common.h"
#include "wx_host.h"
#include "wx_tree_bits.h"
#include "wx_trees_prep.h"
#include <cstring>
#include <thread>
#include <vector>

#define WX_REQUIRE(cond, code, msg) \
    do { if (!(cond)) return wx_set_error(code, msg); } while (0)

extern "C" int wx_device_count(void);

namespace {

enum { WQ_FWD = 0, WQ_INV = 1, WQ_IWPD = 2 };

// words of tree bits per image (at least one)
__host__ __device__ __forceinline__ int wq_words(int64_t ntree) { return ntree > 32 ? (int)((ntree + 31) >> 5) : 1; }

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

template <typename T> size_t wq_lds_bytes(int64_t mn, int64_t ntree) { return (size_t)2 * mn * sizeof(T) + sizeof(uint32_t) * wq_words(ntree); }

// the window of one launch
template <typename T> bool wq_lds_path(int64_t m, int64_t n, int64_t ntree, int F)
{
    if (!wx_isdyadic(m) || !wx_isdyadic(n) || m < 8 || n < 8) return false;
    if (m * n > (sizeof(T) == 8 ? 8192 : 16384)) return false;
    if (F < 2 || F > 20 || (F & 1)) return false;
    return wq_lds_bytes<T>(m * n, ntree) <= 160 * 1024;
}

// one lane per output pair of a pass, at most 1024
int wq_threads(int64_t mn)
{
    int nt = 64;
    while (nt < 1024 && nt < mn / 2) nt <<= 1;
    return nt;
}

// workgroups resident on the 256 CUs (160 KiB of LDS and 2048 lanes each, at most 16 workgroups), never more than images
int wq_grid(size_t lds, int nt, int64_t batch)
{
    int per_cu = (int)((160 * 1024) / lds);
    if (per_cu > 2048 / nt) per_cu = 2048 / nt;
    if (per_cu > 16) per_cu = 16;
    if (per_cu < 1) per_cu = 1;
    const int64_t g = (int64_t)256 * per_cu;
    return (int)(g < batch ? g : batch);
}

int wq_single(const double *x, double *y, int64_t m, int64_t n, int k, const uint8_t *t, int64_t nt, int64_t batch, const double *qmf, int F,
              void *st, int mode)
{
    if (mode == WQ_FWD) return wx_wpt2d_f64(x, y, m, n, 0, t, nt, batch, qmf, F, st);
    if (mode == WQ_INV) return wx_iwpt2d_f64(x, y, m, n, 0, t, nt, batch, qmf, F, st);
    return wx_iwpd2d_f64(x, y, m, n, k, 0, t, nt, batch, qmf, F, st);
}
int wq_single(const float *x, float *y, int64_t m, int64_t n, int k, const uint8_t *t, int64_t nt, int64_t batch, const double *qmf, int F,
              void *st, int mode)
{
    if (mode == WQ_FWD) return wx_wpt2d_f32(x, y, m, n, 0, t, nt, batch, qmf, F, st);
    if (mode == WQ_INV) return wx_iwpt2d_f32(x, y, m, n, 0, t, nt, batch, qmf, F, st);
    return wx_iwpd2d_f32(x, y, m, n, k, 0, t, nt, batch, qmf, F, st);
}

int wq_log2(int64_t v) { int l = 0; while (v > 1) { v >>= 1; ++l; } return l; }

// the launch of k_wpt_trees2d: dt = the trees' bits, dd = one depth byte per image, both in device memory
template <typename T, int MODE>
hipError_t wq_launch(const T *dx, T *dy, int64_t m, int64_t n, int64_t ntree, int k, int64_t batch, const uint32_t *dt, const uint8_t *dd,
                     const WxFilt &filt, hipStream_t st)
{
    const size_t lds = wq_lds_bytes<T>(m * n, ntree);
    const int nt = wq_threads(m * n);
    auto kern = k_wpt_trees2d<T, MODE>;
    hipError_t e = hipSuccess;
    if (lds > 64 * 1024) e = hipFuncSetAttribute(reinterpret_cast<const void *>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(kern, dim3(wq_grid(lds, nt, batch)), dim3(nt), lds, st, dx, dy, wq_log2(m), wq_log2(n), (int)ntree, wq_words(ntree), k,
                       batch, dt, dd, filt);
    return hipGetLastError();
}

template <typename T, int MODE>
int wq_host_trees(const T *x, T *y, int64_t m, int64_t n, int k, const uint8_t *trees, int64_t ntree, int64_t batch, const double *qmf, int F,
                  void *stream, const WxFilt &filt);

// trees in device memory (batch > 0, the argument checks that need no tree content are done): see include/waveletsext_hip.h
template <typename T, int MODE>
int wq_device_trees(const T *x, T *y, int64_t m, int64_t n, int k, const uint8_t *trees, int64_t ntree, int64_t batch, const double *qmf, int F,
                    void *stream, const WxFilt &filt)
{
    WX_REQUIRE(!wx_on_other_device(trees), WX_EARG, "tree matrix lives on another device than the current one");
    hipStream_t st = wx_stream(stream);
    if (!wq_lds_path<T>(m, n, ntree, F)) {
        // outside the LDS kernel's window: the matrix comes to the host once and the host path runs (correct and slow)
        std::vector<uint8_t> ht((size_t)(ntree > 0 ? ntree * batch : 1));
        if (ntree > 0) {
            hipError_t e = hipMemcpyAsync(ht.data(), trees, (size_t)ntree * batch, hipMemcpyDeviceToHost, st);
            if (e == hipSuccess) e = hipStreamSynchronize(st);
            if (e != hipSuccess) {
                (void)hipStreamSynchronize(st);
                return wx_set_hip_error(e, "wptall(trees): tree matrix to the host", __FILE__, __LINE__);
            }
        }
        const int rc = wq_host_trees<T, MODE>(x, y, m, n, k, ht.data(), ntree, batch, qmf, F, stream, filt);
        if (rc == WX_OK) wx_trees_route_set(WX_TREES_ROUTE_DEV_COPIED);
        return rc;
    }
    // inside the window both sides are dyadic: no valid tree is deeper than either side divides by
    const int nw = wq_words(ntree);
    const int64_t mn = m * n;
    WxScratch scr(st);
    const size_t tbytes = sizeof(uint32_t) * nw * (size_t)batch;
    uint8_t *dt = (uint8_t *)scr.alloc(tbytes + (size_t)batch);         // the trees' bits, then one depth byte per image
    if (!dt) return WX_EHIP;
    uint8_t *dd = dt + tbytes;
    std::vector<uint8_t> col0((size_t)ntree);
    bool same = true;
    int rc = wx_trees_prep(true, trees, ntree, batch, MODE == WQ_IWPD ? k : 0, (uint32_t *)dt, nw, dd, col0.data(), &same, st);
    if (rc) return rc;                                                 // nothing has been written to y
    if (same) {                                                        // one tree after all: as the host path does, with the same result
        rc = wq_single(x, y, m, n, k, col0.data(), ntree, batch, qmf, F, stream, MODE);
        if (rc == WX_OK) wx_trees_route_set(WX_TREES_ROUTE_DEV_SINGLE);
        return rc;
    }
    WxIO io(st);
    const T *dx = (const T *)io.in(x, sizeof(T) * mn * (MODE == WQ_IWPD ? k : 1) * batch);
    T *dy = (T *)io.out(y, sizeof(T) * mn * batch);
    if (!dx || !dy) return io.finish(WX_EHIP);
    const hipError_t e = wq_launch<T, MODE>(dx, dy, m, n, ntree, k, batch, (const uint32_t *)dt, dd, filt, st);
    if (e != hipSuccess) {
        (void)hipStreamSynchronize(st);
        return io.finish(wx_set_hip_error(e, "wptall(trees) launch", __FILE__, __LINE__));
    }
    rc = io.finish(WX_OK);                                             // device arrays: nothing waits, the scratch is freed in stream order
    if (rc == WX_OK) wx_trees_route_set(WX_TREES_ROUTE_DEV_LDS);
    return rc;
}

template <typename T, int MODE>
int api_wpt_trees2d(const T *x, T *y, int64_t m, int64_t n, int k, const uint8_t *trees, int64_t ntree, int64_t batch, const double *qmf, int F,
                    void *stream)
{
    wx_trees_route_set(WX_TREES_ROUTE_NONE);
    WxFilt filt;
    int rc = wx_pack_filter(qmf, F, &filt);
    if (rc) return rc;
    // argument errors are reported before any device is needed, with the codes of the 1-D entries, of the single-tree 2-D entries
    // (wx_check_tree2d, wx_api_2d.hip) and of getbasiscoefall
    WX_REQUIRE(m >= 1 && n >= 1 && batch >= 0 && k >= 1, WX_EARG, "wptall(trees): bad dimensions");
    WX_REQUIRE(batch == 0 || trees != nullptr, WX_EARG, "NULL tree matrix");
    WX_REQUIRE(batch == 0 || (const void *)x != (const void *)y, WX_EARG, "wptall(trees): input and output must not be the same array");
    if (MODE == WQ_IWPD)
        WX_REQUIRE(k - 1 <= wx_maxtransformlevels(m < n ? m : n), WX_EASSERT, "getbasiscoef: @assert k-1 <= maxtransformlevels(x) (Utils.jl:110)");
    WX_REQUIRE(ntree == wx_gettreelength2d(m, n), WX_EASSERT, "@assert n_t == gettreelength(sz...) (Utils.jl:211)");
    WX_REQUIRE(m < ((int64_t)1 << 20) && n < ((int64_t)1 << 20) && ntree < ((int64_t)1 << 31), WX_EUNSUPPORTED, "wptall(trees): image side >= 2^20");
    if (batch > 0 && wx_is_device_ptr(trees)) return wq_device_trees<T, MODE>(x, y, m, n, k, trees, ntree, batch, qmf, F, stream, filt);
    rc = wq_host_trees<T, MODE>(x, y, m, n, k, trees, ntree, batch, qmf, F, stream, filt);
    if (rc == WX_OK) wx_trees_route_set(WX_TREES_ROUTE_HOST);
    return rc;
}

// trees in host memory
template <typename T, int MODE>
int wq_host_trees(const T *x, T *y, int64_t m, int64_t n, int k, const uint8_t *trees, int64_t ntree, int64_t batch, const double *qmf, int F,
                  void *stream, const WxFilt &filt)
{
    int rc;
    // every tree is checked like the reference does (Utils.jl:209), must not be deeper than both sides divide by (the size asserts of
    // the 2-D dwt_step!, wx_check_tree2d) and for iwpd must not reach below the table (Utils.jl:120); the first offending column
    // decides the error.  A large matrix is checked by a few host threads, a range of columns each.
    // The LDS kernel takes the trees as bits (an eighth of the bytes to upload), packed by the same pass.
    const bool lds_path = wq_lds_path<T>(m, n, ntree, F);
    const int nw = wq_words(ntree);
    const int64_t mn = m * n;
    const int Lm = wx_maxtransformlevels(m), Ln = wx_maxtransformlevels(n), Lside = Lm < Ln ? Lm : Ln;
    std::vector<uint8_t> depths((size_t)(batch > 0 ? batch : 1));
    std::vector<uint32_t> bits(lds_path ? (size_t)nw * batch : 0);
    enum { BAD_TREE = 1, BAD_SIDES = 2, BAD_K = 3 };
    struct Part { int code = 0; bool same = true; };                   // of a range of columns: its first error, all equal to column 0
    auto check = [&](int64_t b0, int64_t b1, Part *out) {
        for (int64_t b = b0; b < b1; ++b) {
            const uint8_t *t = trees + b * ntree;
            int code = 0;
            if (!wx_isvalidtree2d(m, n, t, ntree)) code = BAD_TREE;
            else {
                const int depth = wx_tree_depth2d(t, ntree);
                depths[(size_t)b] = (uint8_t)depth;
                if (depth > Lside) code = BAD_SIDES;
                else if (MODE == WQ_IWPD && depth >= k) code = BAD_K;
            }
            if (code) { out->code = code; return; }
            if (out->same && ntree > 0) out->same = memcmp(trees, t, (size_t)ntree) == 0;
            if (lds_path) wt_pack_host(t, ntree, bits.data() + (size_t)b * nw);    // zero-initialised
        }
    };
    unsigned nth = 1;
    if (batch * ntree >= ((int64_t)1 << 22)) {
        nth = std::thread::hardware_concurrency();
        nth = nth < 1 ? 1 : (nth > 8 ? 8 : nth);
    }
    std::vector<Part> parts(nth);
    if (nth == 1) check(0, batch, &parts[0]);
    else {
        std::vector<std::thread> pool;
        for (unsigned i = 0; i < nth; ++i) pool.emplace_back(check, batch * i / nth, batch * (i + 1) / nth, &parts[i]);
        for (auto &th : pool) th.join();
    }
    bool same = true;
    for (const Part &pt : parts) {                                      // in column order
        if (pt.code == BAD_TREE) return wx_set_error(WX_EASSERT, "@assert all(mapslices(isvalidtree, tree)) (Utils.jl:209)");
        if (pt.code == BAD_SIDES) return wx_set_error(WX_EASSERT, "both sides must be divisible by 2^depth(tree) (dwt_step! size asserts)");
        if (pt.code) return wx_set_error(WX_EARG, "getbasiscoef: Not enough decomposition levels in Xw (Utils.jl:120)");
        same = same && pt.same;
    }
    if (batch == 0) return WX_OK;
    if (wx_device_count() < 1) return wx_set_error(WX_EHIP, "no HIP device visible: the MI355X kernels cannot run");
    // one tree after all: the single-tree entry has the register kernels of 64 x 64 images
    if (same) return wq_single(x, y, m, n, k, trees, ntree, batch, qmf, F, stream, MODE);
    // outside the LDS kernel's window: the single-tree path once per image.  Slow (a tree upload and a launch sequence per image).
    if (!lds_path) {
        const int64_t xs = MODE == WQ_IWPD ? mn * (int64_t)k : mn;
        for (int64_t b = 0; b < batch; ++b)
            if ((rc = wq_single(x + b * xs, y + b * mn, m, n, k, trees + b * ntree, ntree, 1, qmf, F, stream, MODE))) return rc;
        return WX_OK;
    }
    hipStream_t st = wx_stream(stream);
    WxScratch scr(st);
    const size_t tbytes = sizeof(uint32_t) * nw * (size_t)batch;
    uint8_t *dt = (uint8_t *)scr.alloc(tbytes + (size_t)batch);         // the trees' bits, then one depth byte per image
    if (!dt) return WX_EHIP;
    uint8_t *dd = dt + tbytes;
    WxIO io(st);
    const T *dx = (const T *)io.in(x, sizeof(T) * mn * (MODE == WQ_IWPD ? k : 1) * batch);
    T *dy = (T *)io.out(y, sizeof(T) * mn * batch);
    if (!dx || !dy) return io.finish(WX_EHIP);
    // the packed trees go over from pageable memory of this call: every return behind these copies waits for the stream first.  (The
    // caller's matrix is not read past this point: it may be released on return, as with wx_getbasiscoef2d_trees_*.)
    hipError_t e = hipMemcpyAsync(dt, bits.data(), tbytes, hipMemcpyHostToDevice, st);
    if (e == hipSuccess) e = hipMemcpyAsync(dd, depths.data(), (size_t)batch, hipMemcpyHostToDevice, st);
    if (e != hipSuccess) {
        (void)hipStreamSynchronize(st);
        return io.finish(wx_set_hip_error(e, "wptall(trees): tree upload", __FILE__, __LINE__));
    }
    e = wq_launch<T, MODE>(dx, dy, m, n, ntree, k, batch, (const uint32_t *)dt, dd, filt, st);
    if (e == hipSuccess) e = hipStreamSynchronize(st);                 // `bits` and `depths` are released on return
    if (e != hipSuccess) {
        (void)hipStreamSynchronize(st);
        return io.finish(wx_set_hip_error(e, "wptall(trees) launch", __FILE__, __LINE__));
    }
    return io.finish(WX_OK);
}

}  // namespace

extern "C" {

int wx_wpt2d_trees_f64(const double *x, double *y, int64_t m, int64_t n, const uint8_t *trees, int64_t ntree, int64_t batch, const double *qmf,
                       int F, void *stream)
{ return api_wpt_trees2d<double, WQ_FWD>(x, y, m, n, 1, trees, ntree, batch, qmf, F, stream); }
int wx_wpt2d_trees_f32(const float *x, float *y, int64_t m, int64_t n, const uint8_t *trees, int64_t ntree, int64_t batch, const double *qmf,
                       int F, void *stream)
{ return api_wpt_trees2d<float, WQ_FWD>(x, y, m, n, 1, trees, ntree, batch, qmf, F, stream); }
int wx_iwpt2d_trees_f64(const double *xw, double *xhat, int64_t m, int64_t n, const uint8_t *trees, int64_t ntree, int64_t batch,
                        const double *qmf, int F, void *stream)
{ return api_wpt_trees2d<double, WQ_INV>(xw, xhat, m, n, 1, trees, ntree, batch, qmf, F, stream); }
int wx_iwpt2d_trees_f32(const float *xw, float *xhat, int64_t m, int64_t n, const uint8_t *trees, int64_t ntree, int64_t batch,
                        const double *qmf, int F, void *stream)
{ return api_wpt_trees2d<float, WQ_INV>(xw, xhat, m, n, 1, trees, ntree, batch, qmf, F, stream); }
int wx_iwpd2d_trees_f64(const double *xw, double *xhat, int64_t m, int64_t n, int k, const uint8_t *trees, int64_t ntree, int64_t batch,
                        const double *qmf, int F, void *stream)
{ return api_wpt_trees2d<double, WQ_IWPD>(xw, xhat, m, n, k, trees, ntree, batch, qmf, F, stream); }
int wx_iwpd2d_trees_f32(const float *xw, float *xhat, int64_t m, int64_t n, int k, const uint8_t *trees, int64_t ntree, int64_t batch,
                        const double *qmf, int F, void *stream)
{ return api_wpt_trees2d<float, WQ_IWPD>(xw, xhat, m, n, k, trees, ntree, batch, qmf, F, stream); }

}  // extern "C"
