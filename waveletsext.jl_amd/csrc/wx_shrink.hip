// wx_shrink.hip -- threshold selection of the reference's SureShrink and RelErrorShrink on the device, one workgroup per
// signal (the part round 1 left out).
//
// Reference (paths relative to /root/reference/src/mod):
//   surethreshold(coef, redundant, tree)              Denoising.jl:146-166
//       a = sort(abs.(y)).^2; b = cumsum(a); risk_i = (n - 2 i + b_i + (n - i) a_i) / n; t = sqrt(a[argmin(risk)])
//   relerrorthreshold(coef, redundant, tree, elbows)  Denoising.jl:285-327
//       x = sort(abs.(c), rev = true); r = orth2relerror(c) (Denoising.jl:344-349: sqrt(|sum - cumsum|) / sqrt(sum) of the
//       squares sorted downwards); the curve (x reversed / xmax, r reversed / ymax) with the point (0, r_n) in front and
//       r_1 repeated at the end; `elbows` nested applications of findelbow (Denoising.jl:367-381: the point farthest
//       from the chord between the first and the last point of the current prefix); t = x[elbow] * xmax
// Both are what `denoiseall(...; estnoise = relerrorthreshold)` evaluates for every signal (test/denoising.jl:59-83), so
// they are batched here exactly like the MAD noise estimate of wx_denoise.hip: the selected coefficients of one signal are
// sorted by a bitonic network in LDS (up to 8192 Float64 / 16384 Float32 coefficients; above that in a global scratch window that stays in L2;
// above the LDS window with launches over the whole chip),
// the cumulative sums are a workgroup scan, and argmin / argmax keep the first index on ties like Julia's findmin /
// findmax.  The results are picks from the sorted magnitudes, so they equal the reference's unless two candidates tie to
// within the rounding of the sums (the reference adds sequentially / pairwise, the scan adds by chunks).
#include "../../include/waveletsext_hip.h"     // the definitions below must match the public prototypes
#include "wx_common.h"
#include "wx_kernels.h"
#include "wx_host.h"
#include "wx_shrink_dev.h"
#include <vector>

#define WX_REQUIRE(cond, code, msg) \
    do { if (!(cond)) return wx_set_error(code, msg); } while (0)

extern "C" int wx_device_count(void);

namespace {

// the staging, the sorts, the scan, the argmin / argmax and the two selections themselves: wx_shrink_dev.h (shared with wx_shrink_trees.hip)

// ---- SureShrink: t = sqrt(a[argmin risk]) ---------------------------------------------------------------
template <typename T, bool SORTED = false>
__global__ __launch_bounds__(SH_NT) void k_surethreshold(const T *__restrict__ X, int64_t sig_stride, int n, const int *__restrict__ cols,
                                                         int ncols, int cnt, int npad, T *gscratch, T *__restrict__ tout)
{
    __shared__ ShShared<T> S;
    T *v = sh_window<T>(gscratch, npad);
    if (!SORTED) {
        sh_stage<T>(v, X + (int64_t)blockIdx.x * sig_stride, n, cols, ncols, cnt, npad);
        sh_bitonic<T>(v, npad);
    }
    const T t = sh_sure_pick<T>(v, cnt, npad, S);
    if (threadIdx.x == 0) tout[blockIdx.x] = t;
}

// ---- RelErrorShrink ---------------------------------------------------------------------------------------
template <typename T, bool SORTED = false>
__global__ __launch_bounds__(SH_NT) void k_relerrorthreshold(const T *__restrict__ X, int64_t sig_stride, int n,
                                                             const int *__restrict__ cols, int ncols, int cnt, int npad, int elbows,
                                                             T *gscratch, T *__restrict__ tout)
{
    __shared__ ShShared<T> S;
    T *v = sh_window<T>(gscratch, npad);
    if (!SORTED) {
        sh_stage<T>(v, X + (int64_t)blockIdx.x * sig_stride, n, cols, ncols, cnt, npad);
        sh_bitonic<T>(v, npad);
    }
    const T t = sh_relerror_pick<T>(v, cnt, npad, elbows, S);
    if (threadIdx.x == 0) tout[blockIdx.x] = t;
}

int need_device()
{
    if (wx_device_count() < 1) return wx_set_error(WX_EHIP, "no HIP device visible: the MI355X kernels cannot run");
    return WX_OK;
}

// kind 0: surethreshold, 1: relerrorthreshold
template <typename T>
int api_shrink(int kind, const T *X, int64_t n, int64_t k, int64_t batch, const uint8_t *colmask, int elbows, T *t, void *stream)
{
    WX_REQUIRE(n >= 1 && k >= 1 && batch >= 0, WX_EARG, "bad dimensions");
    WX_REQUIRE(kind == 0 || elbows >= 1, WX_EASSERT, "@assert elbows >= 1 (Denoising.jl:291)");
    std::vector<int> cols;
    if (colmask) for (int64_t c = 0; c < k; ++c) if (colmask[c]) cols.push_back((int)c);
    const int64_t ncols = colmask ? (int64_t)cols.size() : k;
    const int64_t cnt = n * ncols;
    WX_REQUIRE(cnt >= 1, WX_EARG, "no coefficient selected");
    // one workgroup sorts one signal's selection in LDS (up to 8192 Float64 values) or in a global scratch window (WX_SHRINK_WG_MAX, a knob: nothing by default);
    // larger selections -- redundant tables with many leaf columns -- sort with launches over the whole chip (round 4: until then
    // 2^20 coefficients per signal were the limit, and the window path above 2^16 took seconds per signal)
    WX_REQUIRE(cnt <= ((int64_t)1 << 27), WX_EUNSUPPORTED, "threshold selection over more than 2^27 coefficients per signal");
    int rc;
    if ((rc = need_device())) return rc;
    if (batch == 0) return WX_OK;
    int64_t npad = 2;
    while (npad < cnt) npad <<= 1;
    hipStream_t st = wx_stream(stream);
    WxScratch scr(st);
    WxIO io(st);
    const T *dX = (const T *)io.in(X, sizeof(T) * n * k * batch);
    T *dt = (T *)io.out(t, sizeof(T) * batch);
    if (!dX || !dt) return io.finish(WX_EHIP);
    const int *dcols = nullptr;
    if (colmask) {
        dcols = (const int *)scr.upload(cols.data(), cols.size() * sizeof(int));
        if (!dcols) return io.finish(WX_EHIP);
    }
    const size_t win = (size_t)(2 * npad + 8) * sizeof(T);              // sorted magnitudes + the curve (cnt + 1 points)
    const bool in_lds = win <= 144 * 1024;
    if (in_lds && win > 48 * 1024) {
        const void *f = kind == 0 ? reinterpret_cast<const void *>(k_surethreshold<T>) : reinterpret_cast<const void *>(k_relerrorthreshold<T>);
        if (hipFuncSetAttribute(f, hipFuncAttributeMaxDynamicSharedMemorySize, (int)win) != hipSuccess)
            return io.finish(wx_set_error(WX_EHIP, "hipFuncSetAttribute(LDS)"));
    }
    // signals per launch when the windows live in global memory: at most 1 GiB of scratch
    int64_t per = batch;
    T *gs = nullptr;
    if (!in_lds) {
        per = ((int64_t)1 << 30) / (int64_t)win;
        if (per < 1) per = 1;
        if (per > batch) per = batch;
        gs = (T *)scr.alloc(win * per);
        if (!gs) return io.finish(WX_EHIP);
    }
    static const int64_t wg_max = wx_getenv("WX_SHRINK_WG_MAX") ? atoll(wx_getenv("WX_SHRINK_WG_MAX")) : ((int64_t)1 << 13);     // (2^16 values, 4 signals: 7.7 ms in the window, under 3 ms with launches)
    const bool chip_sort = !in_lds && npad > wg_max && npad >= 2 * SH_CH;
    for (int64_t b0 = 0; b0 < batch; b0 += per) {
        const int64_t nb = batch - b0 < per ? batch - b0 : per;
        if (chip_sort) {
            const unsigned gx = (unsigned)((npad / 2 + SH_NT - 1) / SH_NT < 65535 ? (npad / 2 + SH_NT - 1) / SH_NT : 65535);
            for (int64_t s0 = 0; s0 < nb; s0 += 65535) {                  // gridDim.y limit
                const unsigned ns = (unsigned)(nb - s0 < 65535 ? nb - s0 : 65535);
                T *g0 = gs + s0 * (2 * npad + 8);
                hipLaunchKernelGGL(k_sh_stage_g<T>, dim3(gx, ns), dim3(SH_NT), 0, st, dX + (b0 + s0) * n * k, n * k, (int)n, dcols, (int)cnt,
                                   (int)npad, g0);
                sh_chip_sort<T>(g0, npad, ns, st);
            }
            if (kind == 0)
                hipLaunchKernelGGL((k_surethreshold<T, true>), dim3((unsigned)nb), dim3(SH_NT), 0, st, dX + b0 * n * k, n * k, (int)n,
                                   dcols, (int)ncols, (int)cnt, (int)npad, gs, dt + b0);
            else
                hipLaunchKernelGGL((k_relerrorthreshold<T, true>), dim3((unsigned)nb), dim3(SH_NT), 0, st, dX + b0 * n * k, n * k, (int)n,
                                   dcols, (int)ncols, (int)cnt, (int)npad, elbows, gs, dt + b0);
            if (hipGetLastError() != hipSuccess) return io.finish(wx_set_error(WX_EHIP, "threshold selection kernel failed to launch"));
            continue;
        }
        if (kind == 0)
            hipLaunchKernelGGL(k_surethreshold<T>, dim3((unsigned)nb), dim3(SH_NT), in_lds ? win : 0, st, dX + b0 * n * k, n * k, (int)n,
                               dcols, (int)ncols, (int)cnt, (int)npad, gs, dt + b0);
        else
            hipLaunchKernelGGL(k_relerrorthreshold<T>, dim3((unsigned)nb), dim3(SH_NT), in_lds ? win : 0, st, dX + b0 * n * k, n * k, (int)n,
                               dcols, (int)ncols, (int)cnt, (int)npad, elbows, gs, dt + b0);
        if (hipGetLastError() != hipSuccess) return io.finish(wx_set_error(WX_EHIP, "threshold selection kernel failed to launch"));
    }
    return io.finish(WX_OK);
}

}  // namespace

extern "C" {
int wx_surethreshold_f64(const double *X, int64_t n, int64_t k, int64_t batch, const uint8_t *colmask, double *t, void *stream)
{ return api_shrink<double>(0, X, n, k, batch, colmask, 1, t, stream); }
int wx_surethreshold_f32(const float *X, int64_t n, int64_t k, int64_t batch, const uint8_t *colmask, float *t, void *stream)
{ return api_shrink<float>(0, X, n, k, batch, colmask, 1, t, stream); }
int wx_relerrorthreshold_f64(const double *X, int64_t n, int64_t k, int64_t batch, const uint8_t *colmask, int elbows, double *t,
                             void *stream)
{ return api_shrink<double>(1, X, n, k, batch, colmask, elbows, t, stream); }
int wx_relerrorthreshold_f32(const float *X, int64_t n, int64_t k, int64_t batch, const uint8_t *colmask, int elbows, float *t,
                             void *stream)
{ return api_shrink<float>(1, X, n, k, batch, colmask, elbows, t, stream); }
}
