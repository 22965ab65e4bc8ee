// wx_shrink_dev.h -- the device side of the threshold selections of SureShrink and RelErrorShrink (Denoising.jl:146-166, 285-381), shared
// by wx_shrink.hip (one column list and one count for the whole batch) and wx_shrink_trees.hip (the leaf columns and the count of every
// signal's own tree): staging, the bitonic sorts in LDS and over the whole chip, the workgroup scan, the first-index argmin / argmax, and
// the two selections on a sorted window.  A selection reads nothing but the signal's sorted magnitudes v[0, cnt) and cnt, so two kernels
// that hand it the same magnitudes return the same bits.  Its translation units are built with -ffp-contract=on (csrc/Makefile): the
// products and sums below round where the statements say.
#pragma once
#include "wx_common.h"

namespace {

constexpr int SH_NT = 256;

template <typename T> __device__ __forceinline__ T sh_inf();
template <> __device__ __forceinline__ double sh_inf<double>() { return __longlong_as_double(0x7ff0000000000000LL); }
template <> __device__ __forceinline__ float sh_inf<float>() { return __int_as_float(0x7f800000); }

// |X[row, cols[c], signal]| of the selected columns into v[0, cnt), +Inf padding up to npad
template <typename T>
__device__ void sh_stage(T *v, const T *x, int n, const int *cols, int ncols, int cnt, int npad)
{
    for (int e = threadIdx.x; e < npad; e += SH_NT) {
        T val = sh_inf<T>();
        if (e < cnt) {
            const int c = e / n, row = e - c * n;
            val = (T)fabs((double)x[(int64_t)(cols ? cols[c] : c) * n + row]);
        }
        v[e] = val;
    }
    __syncthreads();
}

template <typename T> __device__ void sh_bitonic(T *v, int npad)       // ascending
{
    for (int k = 2; k <= npad; k <<= 1)
        for (int j = k >> 1; j > 0; j >>= 1) {
            for (int i = threadIdx.x; i < (npad >> 1); i += SH_NT) {
                const int lo = ((i & ~(j - 1)) << 1) | (i & (j - 1)), hi = lo | j;
                const bool up = (lo & k) == 0;
                const T a = v[lo], b = v[hi];
                if ((a > b) == up) { v[lo] = b; v[hi] = a; }
            }
            __syncthreads();
        }
}

// w[pos(e)] = f(inclusive running sum of g(e)), e = 0 .. cnt-1: every thread owns a contiguous chunk, the chunk sums are
// scanned through LDS; returns the total to every thread
template <typename T, typename G, typename W>
__device__ T sh_scan(int cnt, T *part, G g, W put)
{
    const int C = (cnt + SH_NT - 1) / SH_NT, e0 = threadIdx.x * C, e1 = min(cnt, e0 + C);
    T s = 0;
    for (int e = e0; e < e1; ++e) s += g(e);
    part[threadIdx.x] = s;
    __syncthreads();
    if (threadIdx.x == 0) {
        T run = 0;
        for (int t = 0; t < SH_NT; ++t) { const T p = part[t]; part[t] = run; run += p; }
        part[SH_NT] = run;
    }
    __syncthreads();
    T run = part[threadIdx.x];
    for (int e = e0; e < e1; ++e) { run += g(e); put(e, run); }
    const T total = part[SH_NT];
    __syncthreads();
    return total;
}

// first index of the extreme value of f(j), j = 0 .. m-1 (MAXIMUM: largest, else smallest), as findmax / argmin
template <typename T, bool MAXIMUM, typename F>
__device__ int sh_argext(int m, T *rv, int *ri, F f)
{
    T best = 0;
    int bi = -1;
    for (int j = threadIdx.x; j < m; j += SH_NT) {
        const T val = f(j);
        if (bi < 0 || (MAXIMUM ? val > best : val < best)) { best = val; bi = j; }
    }
    rv[threadIdx.x] = best; ri[threadIdx.x] = bi;
    __syncthreads();
    for (int s = SH_NT >> 1; s > 0; s >>= 1) {
        if (threadIdx.x < s) {
            const int oi = ri[threadIdx.x + s];
            const T ov = rv[threadIdx.x + s];
            const int mi = ri[threadIdx.x];
            const T mv = rv[threadIdx.x];
            if (oi >= 0 && (mi < 0 || (MAXIMUM ? ov > mv : ov < mv) || (ov == mv && oi < mi))) { rv[threadIdx.x] = ov; ri[threadIdx.x] = oi; }
        }
        __syncthreads();
    }
    const int res = ri[0];
    __syncthreads();
    return res;
}

template <typename T> struct ShShared { T part[SH_NT + 1]; T rv[SH_NT]; int ri[SH_NT]; };

template <typename T>
__device__ __forceinline__ T *sh_window(T *gscratch, int npad)
{
    extern __shared__ __attribute__((aligned(16))) char sh_smem[];
    return gscratch ? gscratch + (int64_t)blockIdx.x * (2 * (int64_t)npad + 8) : reinterpret_cast<T *>(sh_smem);
}

// ---- large selections: the sort as launches over the whole chip ------------------------------------------------------------
// Above SH_WG_MAX values one workgroup per signal would spend log2(npad)^2 / 2 barrier-bound passes over a window in global memory
// (minutes per signal at 2^24).  Instead: stage, then a bitonic network whose passes are launches over (pairs, signals) -- strides
// of at least SH_CH in global memory (k_sh_bitonic_g), all smaller strides of a merge step inside a chunk of SH_CH values in LDS
// (k_sh_bitonic_lds): 44 launches for 2^20 values, 90 for 2^24.  The selection kernels below then run on the sorted window (SORTED).
constexpr int SH_CH = 4096;
template <typename T>
__global__ __launch_bounds__(SH_NT) void k_sh_stage_g(const T *__restrict__ X, int64_t sig_stride, int n, const int *__restrict__ cols, int cnt,
                                                      int npad, T *__restrict__ gs)
{
    const T *x = X + (int64_t)blockIdx.y * sig_stride;
    T *v = gs + (int64_t)blockIdx.y * (2 * (int64_t)npad + 8);
    for (int64_t e = (int64_t)blockIdx.x * SH_NT + threadIdx.x; e < npad; e += (int64_t)gridDim.x * SH_NT) {
        T val = sh_inf<T>();
        if (e < cnt) {
            const int c = (int)(e / n), row = (int)(e - (int64_t)c * n);
            val = (T)fabs((double)x[(int64_t)(cols ? cols[c] : c) * n + row]);
        }
        v[e] = val;
    }
}
// one compare-exchange pass of stride j >= SH_CH of the merge step k
template <typename T>
__global__ __launch_bounds__(SH_NT) void k_sh_bitonic_g(T *__restrict__ gs, int npad, int k, int j)
{
    T *v = gs + (int64_t)blockIdx.y * (2 * (int64_t)npad + 8);
    for (int64_t i = (int64_t)blockIdx.x * SH_NT + threadIdx.x; i < (npad >> 1); i += (int64_t)gridDim.x * SH_NT) {
        const int64_t lo = ((i & ~(int64_t)(j - 1)) << 1) | (i & (j - 1)), hi = lo | j;
        const bool up = (lo & k) == 0;
        const T a = v[lo], b = v[hi];
        if ((a > b) == up) { v[lo] = b; v[hi] = a; }
    }
}
// chunk of SH_CH values in LDS: every merge step up to SH_CH (FIRST), or the strides below SH_CH of the merge step k
template <typename T, bool FIRST>
__global__ __launch_bounds__(SH_NT) void k_sh_bitonic_lds(T *__restrict__ gs, int npad, int k)
{
    __shared__ T w[SH_CH];
    T *v = gs + (int64_t)blockIdx.y * (2 * (int64_t)npad + 8) + (int64_t)blockIdx.x * SH_CH;
    const int64_t g0 = (int64_t)blockIdx.x * SH_CH;                        // global index of w[0]: the direction of a pair depends on it
    for (int e = threadIdx.x; e < SH_CH; e += SH_NT) w[e] = v[e];
    __syncthreads();
    for (int kk = FIRST ? 2 : k; kk <= (FIRST ? SH_CH : k); kk <<= 1)
        for (int j = (FIRST ? kk : SH_CH) >> 1; j > 0; j >>= 1) {
            for (int i = threadIdx.x; i < (SH_CH >> 1); i += SH_NT) {
                const int lo = ((i & ~(j - 1)) << 1) | (i & (j - 1)), hi = lo | j;
                const bool up = ((g0 + lo) & kk) == 0;
                const T a = w[lo], b = w[hi];
                if ((a > b) == up) { w[lo] = b; w[hi] = a; }
            }
            __syncthreads();
        }
    for (int e = threadIdx.x; e < SH_CH; e += SH_NT) v[e] = w[e];
}
// the launches of that network over `ns` windows of 2 npad + 8 values at gs (npad >= 2 SH_CH, ns <= 65535: gridDim.y), after the staging
template <typename T>
inline void sh_chip_sort(T *gs, int64_t npad, unsigned ns, hipStream_t st)
{
    const unsigned gx = (unsigned)((npad / 2 + SH_NT - 1) / SH_NT < 65535 ? (npad / 2 + SH_NT - 1) / SH_NT : 65535);
    hipLaunchKernelGGL((k_sh_bitonic_lds<T, true>), dim3((unsigned)(npad / SH_CH), ns), dim3(SH_NT), 0, st, gs, (int)npad, 0);
    for (int64_t kk = 2 * SH_CH; kk <= npad; kk <<= 1) {
        for (int64_t j = kk >> 1; j >= SH_CH; j >>= 1)
            hipLaunchKernelGGL(k_sh_bitonic_g<T>, dim3(gx, ns), dim3(SH_NT), 0, st, gs, (int)npad, (int)kk, (int)j);
        hipLaunchKernelGGL((k_sh_bitonic_lds<T, false>), dim3((unsigned)(npad / SH_CH), ns), dim3(SH_NT), 0, st, gs, (int)npad, (int)kk);
    }
}

// ---- the selections on the sorted window v[0, cnt) (ascending), v + npad the npad + 8 values of working space behind it ------------
// SureShrink: t = sqrt(a[argmin risk]); the value to every thread
template <typename T>
__device__ T sh_sure_pick(T *v, int cnt, int npad, ShShared<T> &S)
{
    T *b = v + npad;
    sh_scan<T>(cnt, S.part, [&](int e) { const T a = v[e] * v[e]; return a; }, [&](int e, T run) { b[e] = run; });
    const int im = sh_argext<T, false>(cnt, S.rv, S.ri, [&](int i) {
        const T a = v[i] * v[i];
        const T ca = (T)(cnt - 1 - i) * a;                               // c .* a, rounded on its own
        const T s = b[i] + ca;
        return (T)((T)(cnt - 2 * (i + 1)) + s) / (T)cnt;
    });
    const T a = v[im] * v[im];
    return (T)sqrt((double)a);
}

// RelErrorShrink; the value to every thread
template <typename T>
__device__ T sh_relerror_pick(T *v, int cnt, int npad, int elbows, ShShared<T> &S)
{
    T *w = v + npad;                                                      // cnt + 1 <= npad + 8 entries
    // orth2relerror: squares sorted downwards, sum, |sum - cumsum|^0.5 / sum^0.5; r_k lands at curve position cnt - k
    auto sq_desc = [&](int e) { const T a = v[cnt - 1 - e] * v[cnt - 1 - e]; return a; };
    const T total = sh_scan<T>(cnt, S.part, sq_desc, [&](int e, T run) { w[cnt - 1 - e] = run; });
    const T rt = (T)sqrt((double)total);
    for (int j = threadIdx.x; j < cnt; j += SH_NT) w[j] = (T)sqrt(fabs((double)(T)(total - w[j]))) / rt;
    __syncthreads();
    if (threadIdx.x == 0) w[cnt] = w[cnt - 1];                            // pushfirst!(r, r[1])
    __syncthreads();
    const int m = cnt + 1;
    const int iy = sh_argext<T, true>(m, S.rv, S.ri, [&](int j) { return w[j]; });
    const T ymax = w[iy], xmax = v[cnt - 1];
    __syncthreads();
    for (int j = threadIdx.x; j < m; j += SH_NT) w[j] = w[j] / ymax;
    __syncthreads();
    auto xs = [&](int j) { return j == 0 ? (T)0 / xmax : v[j - 1] / xmax; };
    int last = m - 1;
    for (int e = 0; e < elbows; ++e) {
        const T x1 = xs(0), y1 = w[0];
        T vx = xs(last) - x1, vy = w[last] - y1;
        const T nv = (T)sqrt((double)(T)(vx * vx + vy * vy));
        vx = vx / nv; vy = vy / nv;
        last = sh_argext<T, true>(last + 1, S.rv, S.ri, [&](int j) {
            const T dx = xs(j) - x1, dy = w[j] - y1;
            const T dx2 = dx * dx, dy2 = dy * dy;
            const T H = (T)sqrt((double)(T)(dx2 + dy2));
            const T A = dx * vx + dy * vy;
            const T H2 = H * H, A2 = A * A;
            return (T)sqrt(fabs((double)(T)(H2 - A2)));
        });
    }
    return xs(last) * xmax;
}

}  // namespace
