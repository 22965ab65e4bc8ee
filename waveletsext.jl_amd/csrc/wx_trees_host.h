// wx_trees_host.h -- the host side of wptall / iwptall / iwpdall with ONE tree per signal (wx_wpt_trees.hip) or one quad tree per image
// (wx_wpt_trees2d.hip): everything around the kernel, once.  A file defines its kernel and, next to it, a small shape struct S with
// what differs between signals and images:
//   static constexpr bool quad         the heap of its trees (wx_trees_prep.h)
//   bool dims_ok()                     the sides are positive
//   int64_t count()                    elements of one item
//   int check(iwpd, k, ntree)          the argument checks of the shape, in its order, with its messages; the expected ntree is one
//   int check_host(trees, ...)         wx_trees_check_host with the shape's heap, sides and maximum depth
//   bool window<T>(ntree, F)           whether the LDS kernel takes the shape
//   int single(mode, x, y, k, ...)     the single-tree entry of the mode, for double and for float
//   hipError_t launch<T, MODE>(...)    the launch of the kernel: dt = the trees' bits (wq_words(ntree) words each, wx_tree_bits.h),
//                                      dd = one depth byte per item, both in device memory
// Routes (wx_trees_prep.h): a matrix in host memory is checked and packed by wx_trees_check_host, one in device memory by
// wx_trees_prep.  Byte-identical columns go to the single-tree entry whole; outside the window the single-tree entry runs once per
// item (slow, correct), a device matrix coming to the host first.  The host route returns after the stream has finished, because
// it uploads from memory of the call; the device route with device data waits for nothing but the prep record.
// A shape with `static constexpr bool extras = true` carries more arguments than these (wx_denoise_trees.hip: thresholds, estimates); then
//   S at(b)                            the shape of item b alone, for the single-tree entry once per item
//   bool stage(io, batch)              its own arrays as device pointers for launch(), through the call's WxIO
// and y and qmf may be NULL where the shape's check() admits it.
// A shape with `static constexpr bool table = true` reads each item from a table of its own (wx_red_trees.hip: the redundant packet tables) and has
//   int64_t in_count()                 elements of one input item
//   int tree_k()                       no tree may be as deep as this: the `k` of the trees' check, whatever the mode
//   int too_deep()                     the error of a tree that is, with the code and message of the shape's single-tree entry
// A shape with `static constexpr bool by_chunks = true` has no single-tree entry to fall back on (wx_denoise_red_sig.hip: the items are signals,
// the table entries want tables): inside the window the kernel runs whether the columns are equal or not, and outside it
//   int chunked(x, y, trees, ...)      runs the whole checked batch, the tree matrix in host memory, by a loop of its own
// replaces single() once per item.
#pragma once
#include "../../include/waveletsext_hip.h"
#include "wx_common.h"
#include "wx_host.h"
#include "wx_tree_bits.h"
#include "wx_trees_geom.h"                      // wx_trees_threads, wx_trees_grid
#include "wx_trees_prep.h"
#include <type_traits>
#include <vector>

#define WX_REQUIRE(cond, code, msg) \
    do { if (!(cond)) return wx_set_error(code, msg); } while (0)

extern "C" int wx_device_count(void);

enum { WX_TREES_FWD = 0, WX_TREES_INV = 1, WX_TREES_IWPD = 2 };

template <typename S, typename = void> struct WxTreesExtras { static constexpr bool value = false; };
template <typename S> struct WxTreesExtras<S, std::void_t<decltype(S::extras)>> { static constexpr bool value = S::extras; };
template <typename S, typename = void> struct WxTreesTable { static constexpr bool value = false; };
template <typename S> struct WxTreesTable<S, std::void_t<decltype(S::table)>> { static constexpr bool value = S::table; };
template <typename S, typename = void> struct WxTreesChunked { static constexpr bool value = false; };
template <typename S> struct WxTreesChunked<S, std::void_t<decltype(S::by_chunks)>> { static constexpr bool value = S::by_chunks; };

// elements of one input item, and the depth no tree may reach (0: any)
template <int MODE, typename S> inline int64_t wx_trees_in_count(const S &s, int k)
{
    if constexpr (WxTreesTable<S>::value) return s.in_count();
    else return MODE == WX_TREES_IWPD ? s.count() * k : s.count();
}
template <int MODE, typename S> inline int wx_trees_k(const S &s, int k)
{
    if constexpr (WxTreesTable<S>::value) return s.tree_k();
    else return MODE == WX_TREES_IWPD ? k : 0;
}

// trees in host memory
template <typename T, int MODE, typename S>
int wx_trees_from_host(const S &s, const T *x, T *y, int k, const uint8_t *trees, int64_t ntree, int64_t batch, const double *qmf, int F,
                       void *stream, const WxFilt &filt)
{
    // every tree is checked like the reference does (Utils.jl:209), an image's must not be deeper than both sides divide by (the size
    // asserts of the 2-D dwt_step!, wx_check_tree2d) and for iwpd it must not reach below the table (Utils.jl:120); the first
    // offending column decides the error.  The LDS kernel takes the trees as bits (an eighth of the bytes to upload), packed by the
    // same pass.
    const bool lds_path = s.template window<T>(ntree, F);
    const int nw = wq_words(ntree);
    const int64_t cnt = s.count(), xs = wx_trees_in_count<MODE>(s, k);
    std::vector<uint8_t> depths((size_t)(batch > 0 ? batch : 1));
    std::vector<uint32_t> bits(lds_path ? (size_t)nw * batch : 0);     // zero-initialised
    bool same = true;
    int rc = s.check_host(trees, ntree, batch, wx_trees_k<MODE>(s, k), lds_path ? bits.data() : nullptr, nw, depths.data(), &same);
    if constexpr (WxTreesTable<S>::value)
        if (rc == WX_EARG) return s.too_deep();
    if (rc == WX_EARG) return wx_set_error(WX_EARG, "getbasiscoef: Not enough decomposition levels in Xw (Utils.jl:120)");
    if (rc) return rc;
    if (batch == 0) return WX_OK;
    if (wx_device_count() < 1) return wx_set_error(WX_EHIP, "no HIP device visible: the MI355X kernels cannot run");
    if constexpr (WxTreesChunked<S>::value) {
        if (!lds_path) return s.chunked(x, y, trees, ntree, batch, qmf, F, stream);
    } else {
        // one tree after all: the single-tree entry has the lattice kernels and the register kernels of 64 x 64 images
        if (same) return s.single(MODE, x, y, k, trees, ntree, batch, qmf, F, stream);
        // outside the LDS kernel's window: the single-tree path once per item.  Slow (a tree upload and a launch sequence per item).
        if (!lds_path) {
            for (int64_t b = 0; b < batch; ++b) {
                if constexpr (WxTreesExtras<S>::value)
                    rc = s.at(b).single(MODE, x + b * xs, y ? y + b * cnt : y, k, trees + b * ntree, ntree, 1, qmf, F, stream);
                else rc = s.single(MODE, x + b * xs, y + b * cnt, k, trees + b * ntree, ntree, 1, qmf, F, stream);
                if (rc) return rc;
            }
            return WX_OK;
        }
    }
    hipStream_t st = wx_stream(stream);
    WxScratch scr(st);
    const size_t tbytes = sizeof(uint32_t) * nw * (size_t)batch;
    uint8_t *dt = (uint8_t *)scr.alloc(tbytes + (size_t)batch);         // the trees' bits, then one depth byte per item
    if (!dt) return WX_EHIP;
    uint8_t *dd = dt + tbytes;
    WxIO io(st);
    const T *dx = (const T *)io.in(x, sizeof(T) * xs * batch);
    T *dy = WxTreesExtras<S>::value && !y ? nullptr : (T *)io.out(y, sizeof(T) * cnt * batch);
    if (!dx || (!dy && (y || !WxTreesExtras<S>::value))) return io.finish(WX_EHIP);
    if constexpr (WxTreesExtras<S>::value)
        if (!s.stage(io, batch)) return io.finish(WX_EHIP);
    // the packed trees go over from pageable memory of this call: every return behind these copies waits for the stream first.  (The
    // caller's matrix is not read past this point: it may be released on return, as with wx_getbasiscoef*_trees_*.)
    hipError_t e = hipMemcpyAsync(dt, bits.data(), tbytes, hipMemcpyHostToDevice, st);
    if (e == hipSuccess) e = hipMemcpyAsync(dd, depths.data(), (size_t)batch, hipMemcpyHostToDevice, st);
    if (e != hipSuccess) {
        (void)hipStreamSynchronize(st);
        return io.finish(wx_set_hip_error(e, "wptall(trees): tree upload", __FILE__, __LINE__));
    }
    e = s.template launch<T, MODE>(dx, dy, ntree, k, batch, (const uint32_t *)dt, dd, filt, st);
    if (e == hipSuccess) e = hipStreamSynchronize(st);                 // `bits` and `depths` are released on return
    if (e != hipSuccess) {
        (void)hipStreamSynchronize(st);
        return io.finish(wx_set_hip_error(e, "wptall(trees) launch", __FILE__, __LINE__));
    }
    return io.finish(WX_OK);
}

// trees in device memory (batch > 0, the argument checks that need no tree content are done): see include/waveletsext_hip.h
template <typename T, int MODE, typename S>
int wx_trees_from_device(const S &s, const T *x, T *y, int k, const uint8_t *trees, int64_t ntree, int64_t batch, const double *qmf, int F,
                         void *stream, const WxFilt &filt)
{
    WX_REQUIRE(!wx_on_other_device(trees), WX_EARG, "tree matrix lives on another device than the current one");
    hipStream_t st = wx_stream(stream);
    if (!s.template window<T>(ntree, F)) {
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
        const int rc = wx_trees_from_host<T, MODE>(s, x, y, k, ht.data(), ntree, batch, qmf, F, stream, filt);
        if (rc == WX_OK) wx_trees_route_set(WX_TREES_ROUTE_DEV_COPIED);
        return rc;
    }
    // inside the window every side is dyadic: no valid tree is deeper than a side divides by
    const int nw = wq_words(ntree);
    const int64_t cnt = s.count();
    WxScratch scr(st);
    const size_t tbytes = sizeof(uint32_t) * nw * (size_t)batch;
    uint8_t *dt = (uint8_t *)scr.alloc(tbytes + (size_t)batch);         // the trees' bits, then one depth byte per item
    if (!dt) return WX_EHIP;
    uint8_t *dd = dt + tbytes;
    std::vector<uint8_t> col0((size_t)ntree);
    bool same = true;
    int rc = wx_trees_prep(S::quad, trees, ntree, batch, wx_trees_k<MODE>(s, k), (uint32_t *)dt, nw, dd, col0.data(), &same, st);
    if constexpr (WxTreesTable<S>::value)
        if (rc == WX_EARG) return s.too_deep();
    if (rc) return rc;                                                 // nothing has been written to y
    if constexpr (!WxTreesChunked<S>::value) {
        if (same) {                                                    // one tree after all: as the host path does, with the same result
            rc = s.single(MODE, x, y, k, col0.data(), ntree, batch, qmf, F, stream);
            if (rc == WX_OK) wx_trees_route_set(WX_TREES_ROUTE_DEV_SINGLE);
            return rc;
        }
    }
    WxIO io(st);
    const T *dx = (const T *)io.in(x, sizeof(T) * wx_trees_in_count<MODE>(s, k) * batch);
    T *dy = WxTreesExtras<S>::value && !y ? nullptr : (T *)io.out(y, sizeof(T) * cnt * batch);
    if (!dx || (!dy && (y || !WxTreesExtras<S>::value))) return io.finish(WX_EHIP);
    if constexpr (WxTreesExtras<S>::value)
        if (!s.stage(io, batch)) return io.finish(WX_EHIP);
    const hipError_t e = s.template launch<T, MODE>(dx, dy, ntree, k, batch, (const uint32_t *)dt, dd, filt, st);
    if (e != hipSuccess) {
        (void)hipStreamSynchronize(st);
        return io.finish(wx_set_hip_error(e, "wptall(trees) launch", __FILE__, __LINE__));
    }
    rc = io.finish(WX_OK);                                             // device arrays: nothing waits, the scratch is freed in stream order
    if (rc == WX_OK) wx_trees_route_set(WX_TREES_ROUTE_DEV_LDS);
    return rc;
}

template <typename T, int MODE, typename S>
int wx_trees_api(const S &s, const T *x, T *y, int k, const uint8_t *trees, int64_t ntree, int64_t batch, const double *qmf, int F, void *stream)
{
    wx_trees_route_set(WX_TREES_ROUTE_NONE);
    WxFilt filt;
    int rc = WX_OK;
    if (WxTreesExtras<S>::value && !qmf) filt.F = 0;                   // no transform (the shape's check() decides whether that is allowed)
    else rc = wx_pack_filter(qmf, F, &filt);
    if (rc) return rc;
    // argument errors are reported before any device is needed, with the codes of the single-tree entries and of getbasiscoefall
    WX_REQUIRE(s.dims_ok() && batch >= 0 && k >= 1, WX_EARG, "wptall(trees): bad dimensions");
    WX_REQUIRE(batch == 0 || trees != nullptr, WX_EARG, "NULL tree matrix");
    WX_REQUIRE(batch == 0 || (const void *)x != (const void *)y, WX_EARG, "wptall(trees): input and output must not be the same array");
    if ((rc = s.check(MODE == WX_TREES_IWPD, k, ntree))) return rc;
    if (batch > 0 && wx_is_device_ptr(trees)) return wx_trees_from_device<T, MODE>(s, x, y, k, trees, ntree, batch, qmf, F, stream, filt);
    rc = wx_trees_from_host<T, MODE>(s, x, y, k, trees, ntree, batch, qmf, F, stream, filt);
    if (rc == WX_OK) wx_trees_route_set(WX_TREES_ROUTE_HOST);
    return rc;
}
