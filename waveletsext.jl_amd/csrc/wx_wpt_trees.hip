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
// The host checks every tree (a few threads for a large matrix), notes its depth and packs it into bits in the same pass: the kernel
// gets n / 8 bytes of tree per signal instead of n - 1.  A tree matrix in DEVICE memory (bestbasistreeall's own output) gets the
// same pass as one launch (wx_trees_prep.hip) and never visits the host inside the window.
// The filter length is a loop bound: six kernels in all (3 directions x 2 types), the arithmetic is Float64 for either type like the
// one-level kernels of wx_dwt1d.hip.  No atomics; every output element is written by exactly one lane.
// Window: what wx_fused1d_ok admits (dyadic 8 <= n <= 8192 Float64 / 16384 Float32, even filters of 2 .. 20 taps).  Outside it the
// entry calls the single-tree entry once per signal (slow, correct).  Byte-identical columns go to the single-tree entry whole.
#include "../../include/waveletsext_hip.h"
#include "wx_common.h"
#include "wx_host.h"
#include "wx_kernels.h"
#include "wx_tree_bits.h"
#include "wx_trees_prep.h"
#include <cstring>
#include <thread>
#include <vector>

#define WX_REQUIRE(cond, code, msg) \
    do { if (!(cond)) return wx_set_error(code, msg); } while (0)

extern "C" int wx_device_count(void);

namespace {

enum { WT_FWD = 0, WT_INV = 1, WT_IWPD = 2 };

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

template <typename T> size_t wt_lds_bytes(int64_t n) { return sizeof(double) * WX_MAXF + (size_t)2 * n * sizeof(T) + sizeof(uint32_t) * wt_words(n); }

// one lane per output pair of a level, at most 1024
int wt_threads(int64_t n)
{
    int nt = 64;
    while (nt < 1024 && nt < n / 2) nt <<= 1;
    return nt;
}

// workgroups resident on the 256 CUs (160 KiB of LDS and 2048 lanes each, at most 16 workgroups), never more than signals
int wt_grid(size_t lds, int nt, int64_t batch)
{
    int per_cu = (int)((160 * 1024) / lds);
    if (per_cu > 2048 / nt) per_cu = 2048 / nt;
    if (per_cu > 16) per_cu = 16;
    if (per_cu < 1) per_cu = 1;
    const int64_t g = (int64_t)256 * per_cu;
    return (int)(g < batch ? g : batch);
}

int wt_single(const double *x, double *y, int64_t n, int k, const uint8_t *t, int64_t nt, int64_t batch, const double *qmf, int F, void *st, int mode)
{
    if (mode == WT_FWD) return wx_wpt1d_f64(x, y, n, 0, t, nt, batch, qmf, F, st);
    if (mode == WT_INV) return wx_iwpt1d_f64(x, y, n, 0, t, nt, batch, qmf, F, st);
    return wx_iwpd1d_f64(x, y, n, k, 0, t, nt, batch, qmf, F, st);
}
int wt_single(const float *x, float *y, int64_t n, int k, const uint8_t *t, int64_t nt, int64_t batch, const double *qmf, int F, void *st, int mode)
{
    if (mode == WT_FWD) return wx_wpt1d_f32(x, y, n, 0, t, nt, batch, qmf, F, st);
    if (mode == WT_INV) return wx_iwpt1d_f32(x, y, n, 0, t, nt, batch, qmf, F, st);
    return wx_iwpd1d_f32(x, y, n, k, 0, t, nt, batch, qmf, F, st);
}

template <typename T> bool wt_lds_path(int64_t n, int F) { return wx_fused1d_ok<T>(n, F) && wt_lds_bytes<T>(n) <= 160 * 1024; }

// the launch of k_wpt_trees: dt = the trees' bits, dd = one depth byte per signal, both in device memory
template <typename T, int MODE>
hipError_t wt_launch(const T *dx, T *dy, int64_t n, int k, int64_t batch, const uint32_t *dt, const uint8_t *dd, const WxFilt &filt,
                     hipStream_t st)
{
    const size_t lds = wt_lds_bytes<T>(n);
    const int nt = wt_threads(n);
    auto kern = k_wpt_trees<T, MODE>;
    hipError_t e = hipSuccess;
    if (lds > 64 * 1024) e = hipFuncSetAttribute(reinterpret_cast<const void *>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    if (e != hipSuccess) return e;
    int log2n = 0;
    while (((int64_t)1 << log2n) < n) ++log2n;
    hipLaunchKernelGGL(kern, dim3(wt_grid(lds, nt, batch)), dim3(nt), lds, st, dx, dy, log2n, k, batch, dt, dd, filt);
    return hipGetLastError();
}

template <typename T, int MODE>
int wt_host_trees(const T *x, T *y, int64_t n, int k, const uint8_t *trees, int64_t ntree, int64_t batch, const double *qmf, int F,
                  void *stream, const WxFilt &filt);

// trees in device memory (batch > 0, the argument checks that need no tree content are done): see include/waveletsext_hip.h
template <typename T, int MODE>
int wt_device_trees(const T *x, T *y, int64_t n, int k, const uint8_t *trees, int64_t ntree, int64_t batch, const double *qmf, int F,
                    void *stream, const WxFilt &filt)
{
    WX_REQUIRE(!wx_on_other_device(trees), WX_EARG, "tree matrix lives on another device than the current one");
    hipStream_t st = wx_stream(stream);
    if (!wt_lds_path<T>(n, F)) {
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
        const int rc = wt_host_trees<T, MODE>(x, y, n, k, ht.data(), ntree, batch, qmf, F, stream, filt);
        if (rc == WX_OK) wx_trees_route_set(WX_TREES_ROUTE_DEV_COPIED);
        return rc;
    }
    const int nw = wt_words(n);
    WxScratch scr(st);
    const size_t tbytes = sizeof(uint32_t) * nw * (size_t)batch;
    uint8_t *dt = (uint8_t *)scr.alloc(tbytes + (size_t)batch);         // the trees' bits, then one depth byte per signal
    if (!dt) return WX_EHIP;
    uint8_t *dd = dt + tbytes;
    std::vector<uint8_t> col0((size_t)ntree);
    bool same = true;
    int rc = wx_trees_prep(false, trees, ntree, batch, MODE == WT_IWPD ? k : 0, (uint32_t *)dt, nw, dd, col0.data(), &same, st);
    if (rc) return rc;                                                 // nothing has been written to y
    if (same) {                                                        // one tree after all: as the host path does, with the same result
        rc = wt_single(x, y, n, k, col0.data(), ntree, batch, qmf, F, stream, MODE);
        if (rc == WX_OK) wx_trees_route_set(WX_TREES_ROUTE_DEV_SINGLE);
        return rc;
    }
    WxIO io(st);
    const T *dx = (const T *)io.in(x, sizeof(T) * n * (MODE == WT_IWPD ? k : 1) * batch);
    T *dy = (T *)io.out(y, sizeof(T) * n * batch);
    if (!dx || !dy) return io.finish(WX_EHIP);
    const hipError_t e = wt_launch<T, MODE>(dx, dy, n, k, batch, (const uint32_t *)dt, dd, filt, st);
    if (e != hipSuccess) {
        (void)hipStreamSynchronize(st);
        return io.finish(wx_set_hip_error(e, "wptall(trees) launch", __FILE__, __LINE__));
    }
    rc = io.finish(WX_OK);                                             // device arrays: nothing waits, the scratch is freed in stream order
    if (rc == WX_OK) wx_trees_route_set(WX_TREES_ROUTE_DEV_LDS);
    return rc;
}

template <typename T, int MODE>
int api_wpt_trees(const T *x, T *y, int64_t n, int k, const uint8_t *trees, int64_t ntree, int64_t batch, const double *qmf, int F,
                  void *stream)
{
    wx_trees_route_set(WX_TREES_ROUTE_NONE);
    WxFilt filt;
    int rc = wx_pack_filter(qmf, F, &filt);
    if (rc) return rc;
    // argument errors are reported before any device is needed, with the codes of the single-tree entries and of getbasiscoefall
    WX_REQUIRE(n >= 1 && batch >= 0 && k >= 1, WX_EARG, "wptall(trees): bad dimensions");
    WX_REQUIRE(batch == 0 || trees != nullptr, WX_EARG, "NULL tree matrix");
    WX_REQUIRE(batch == 0 || (const void *)x != (const void *)y, WX_EARG, "wptall(trees): input and output must not be the same array");
    WX_REQUIRE(wx_isdyadic(n), WX_EASSERT, "maketree/isvalidtree: signal length must be dyadic (Wavelets.jl)");
    if (MODE == WT_IWPD) WX_REQUIRE(k - 1 <= wx_maxtransformlevels(n), WX_EASSERT, "getbasiscoef: @assert k-1 <= L (Utils.jl:110)");
    WX_REQUIRE(ntree == n - 1, WX_EASSERT, "@assert n_t == gettreelength(sz...) (Utils.jl:211)");
    WX_REQUIRE(n < ((int64_t)1 << 30), WX_EUNSUPPORTED, "wptall(trees): signal length >= 2^30 not supported");
    if (batch > 0 && wx_is_device_ptr(trees)) return wt_device_trees<T, MODE>(x, y, n, k, trees, ntree, batch, qmf, F, stream, filt);
    rc = wt_host_trees<T, MODE>(x, y, n, k, trees, ntree, batch, qmf, F, stream, filt);
    if (rc == WX_OK) wx_trees_route_set(WX_TREES_ROUTE_HOST);
    return rc;
}

// trees in host memory
template <typename T, int MODE>
int wt_host_trees(const T *x, T *y, int64_t n, int k, const uint8_t *trees, int64_t ntree, int64_t batch, const double *qmf, int F,
                  void *stream, const WxFilt &filt)
{
    int rc;
    // every tree is checked like the reference does (Utils.jl:209), and for iwpd must not reach below the table (Utils.jl:120); the
    // first offending column decides the error.  A large matrix is checked by a few host threads, a range of columns each.
    // The LDS kernel takes the trees as bits (an eighth of the bytes to upload), packed by the same pass.
    const bool lds_path = wt_lds_path<T>(n, F);
    const int nw = wt_words(n);
    std::vector<uint8_t> depths((size_t)(batch > 0 ? batch : 1));
    std::vector<uint32_t> bits(lds_path ? (size_t)nw * batch : 0);
    struct Part { int code = WX_OK; bool same = true; };               // of a range of columns: its first error, all equal to column 0
    auto check = [&](int64_t b0, int64_t b1, Part *out) {
        for (int64_t b = b0; b < b1; ++b) {
            const uint8_t *t = trees + b * ntree;
            int code = WX_OK;
            if (!wx_isvalidtree1d(n, t, ntree)) code = WX_EASSERT;
            else {
                const int depth = wx_tree_depth1d(t, ntree);
                depths[(size_t)b] = (uint8_t)depth;
                if (MODE == WT_IWPD && depth >= k) code = WX_EARG;
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
        if (pt.code == WX_EASSERT) return wx_set_error(WX_EASSERT, "@assert all(mapslices(isvalidtree, tree)) (Utils.jl:209)");
        if (pt.code) return wx_set_error(WX_EARG, "getbasiscoef: Not enough decomposition levels in Xw (Utils.jl:120)");
        same = same && pt.same;
    }
    if (batch == 0) return WX_OK;
    if (wx_device_count() < 1) return wx_set_error(WX_EHIP, "no HIP device visible: the MI355X kernels cannot run");
    // one tree after all: the single-tree entry has the lattice kernels
    if (same) return wt_single(x, y, n, k, trees, ntree, batch, qmf, F, stream, MODE);
    // outside the LDS kernel's window: the single-tree path once per signal.  Slow (a tree upload and a launch sequence per signal).
    if (!lds_path) {
        const int64_t xs = MODE == WT_IWPD ? n * (int64_t)k : n;
        for (int64_t b = 0; b < batch; ++b)
            if ((rc = wt_single(x + b * xs, y + b * n, n, k, trees + b * ntree, ntree, 1, qmf, F, stream, MODE))) return rc;
        return WX_OK;
    }
    hipStream_t st = wx_stream(stream);
    WxScratch scr(st);
    const size_t tbytes = sizeof(uint32_t) * nw * (size_t)batch;
    uint8_t *dt = (uint8_t *)scr.alloc(tbytes + (size_t)batch);         // the trees' bits, then one depth byte per signal
    if (!dt) return WX_EHIP;
    uint8_t *dd = dt + tbytes;
    WxIO io(st);
    const T *dx = (const T *)io.in(x, sizeof(T) * n * (MODE == WT_IWPD ? k : 1) * batch);
    T *dy = (T *)io.out(y, sizeof(T) * n * batch);
    if (!dx || !dy) return io.finish(WX_EHIP);
    // the packed trees go over from pageable memory of this call: every return behind these copies waits for the stream first.  (The
    // caller's matrix is not read past this point: it may be released on return, as with wx_getbasiscoef1d_trees_*.)
    hipError_t e = hipMemcpyAsync(dt, bits.data(), tbytes, hipMemcpyHostToDevice, st);
    if (e == hipSuccess) e = hipMemcpyAsync(dd, depths.data(), (size_t)batch, hipMemcpyHostToDevice, st);
    if (e != hipSuccess) {
        (void)hipStreamSynchronize(st);
        return io.finish(wx_set_hip_error(e, "wptall(trees): tree upload", __FILE__, __LINE__));
    }
    e = wt_launch<T, MODE>(dx, dy, n, k, batch, (const uint32_t *)dt, dd, filt, st);
    if (e == hipSuccess) e = hipStreamSynchronize(st);                 // `bits` and `depths` are released on return
    if (e != hipSuccess) {
        (void)hipStreamSynchronize(st);
        return io.finish(wx_set_hip_error(e, "wptall(trees) launch", __FILE__, __LINE__));
    }
    return io.finish(WX_OK);
}

}  // namespace

extern "C" {

int wx_wpt1d_trees_f64(const double *x, double *y, int64_t n, const uint8_t *trees, int64_t ntree, int64_t batch, const double *qmf, int F,
                       void *stream)
{ return api_wpt_trees<double, WT_FWD>(x, y, n, 1, trees, ntree, batch, qmf, F, stream); }
int wx_wpt1d_trees_f32(const float *x, float *y, int64_t n, const uint8_t *trees, int64_t ntree, int64_t batch, const double *qmf, int F,
                       void *stream)
{ return api_wpt_trees<float, WT_FWD>(x, y, n, 1, trees, ntree, batch, qmf, F, stream); }
int wx_iwpt1d_trees_f64(const double *xw, double *xhat, int64_t n, const uint8_t *trees, int64_t ntree, int64_t batch, const double *qmf,
                        int F, void *stream)
{ return api_wpt_trees<double, WT_INV>(xw, xhat, n, 1, trees, ntree, batch, qmf, F, stream); }
int wx_iwpt1d_trees_f32(const float *xw, float *xhat, int64_t n, const uint8_t *trees, int64_t ntree, int64_t batch, const double *qmf,
                        int F, void *stream)
{ return api_wpt_trees<float, WT_INV>(xw, xhat, n, 1, trees, ntree, batch, qmf, F, stream); }
int wx_iwpd1d_trees_f64(const double *xw, double *xhat, int64_t n, int k, const uint8_t *trees, int64_t ntree, int64_t batch,
                        const double *qmf, int F, void *stream)
{ return api_wpt_trees<double, WT_IWPD>(xw, xhat, n, k, trees, ntree, batch, qmf, F, stream); }
int wx_iwpd1d_trees_f32(const float *xw, float *xhat, int64_t n, int k, const uint8_t *trees, int64_t ntree, int64_t batch,
                        const double *qmf, int F, void *stream)
{ return api_wpt_trees<float, WT_IWPD>(xw, xhat, n, k, trees, ntree, batch, qmf, F, stream); }

}  // extern "C"
