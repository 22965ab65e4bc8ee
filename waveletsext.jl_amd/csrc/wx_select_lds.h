// wx_select_lds.h -- exact order statistics of values in LDS (or in global memory) by a whole workgroup: the selection behind
// k_mad / k_mad_g (wx_denoise.hip) and behind the per-signal noise estimate of k_denoise_trees (wx_denoise_trees.hip).
// Value bucketing instead of a sort: with the exact min / max of the candidates, bucket(x) = floor((x - lo) * scale)
// is monotone, so the k-th smallest lies in the bucket where the running count crosses k.  One histogram pass
// (1024 buckets: coefficients spread over them, so the LDS atomics do not pile up on one word) leaves a handful
// of candidates, which are ranked directly.  Degenerate data (everything in one bucket) narrows [lo, hi] to that
// bucket's own min / max and repeats; equal candidates end the search.  No arithmetic on the result: exact.  Infinite bounds are split off
// before the bucketing, and the offsets are scaled so that lo and hi always land in different buckets: every input ends (wx_select_kth).
// Workgroups of 1 ... WX_SELW wavefronts (64 ... 1024 lanes); every lane of the workgroup calls, with the same arguments.
#pragma once
#include "wx_common.h"
#include "wx_select_count.h"

namespace {

constexpr int WX_NB = 1024;       // buckets
constexpr int WX_LST = 256;       // candidates ranked directly
constexpr int WX_SELW = 16;       // wavefronts of the widest workgroup: one slot each in the block reductions

template <typename T> __device__ __forceinline__ T wx_wave_min(T v)
{
    for (int o = 32; o > 0; o >>= 1) { const T u = __shfl_xor(v, o, 64); v = u < v ? u : v; }
    return v;
}
template <typename T> __device__ __forceinline__ T wx_wave_max(T v)
{
    for (int o = 32; o > 0; o >>= 1) { const T u = __shfl_xor(v, o, 64); v = u > v ? u : v; }
    return v;
}
struct WxSelScratch {
    unsigned int hist[WX_NB];
    double lst[WX_LST];
    double red[2 * WX_SELW + 1];  // minima | maxima of the wavefronts | the selected candidate
    int ired[4 + WX_SELW];        // bucket, count before it, count in it, list length | counts of the wavefronts
};

// block-wide min and max of f(i) over i in [0, cnt) restricted by pred; every thread gets the result
template <typename T, typename P>
__device__ void wx_block_minmax(const T *v, int cnt, P pred, WxSelScratch *S, T &mn, T &mx)
{
    T a = (T)INFINITY, b = (T)-INFINITY;
    for (int i = threadIdx.x; i < cnt; i += blockDim.x) { const T x = v[i]; if (pred(x)) { a = x < a ? x : a; b = x > b ? x : b; } }
    a = wx_wave_min(a); b = wx_wave_max(b);
    const int w = threadIdx.x >> 6;
    __syncthreads();
    if ((threadIdx.x & 63) == 0) { S->red[w] = (double)a; S->red[WX_SELW + w] = (double)b; }
    __syncthreads();
    double m0 = S->red[0], m1 = S->red[WX_SELW];
    for (int j = 1; j < (int)(blockDim.x >> 6); ++j) { m0 = S->red[j] < m0 ? S->red[j] : m0; m1 = S->red[WX_SELW + j] > m1 ? S->red[WX_SELW + j] : m1; }
    mn = (T)m0; mx = (T)m1;
}

// block-wide #{i in [0, cnt): pred(v[i])}; every thread gets the result
template <typename T, typename P>
__device__ __forceinline__ int wx_block_count(const T *v, int cnt, P pred, WxSelScratch *S)
{
    int c = 0;
    for (int i = threadIdx.x; i < cnt; i += blockDim.x) c += pred(v[i]) ? 1 : 0;
    for (int o = 32; o > 0; o >>= 1) c += __shfl_xor(c, o, 64);
    const int w = threadIdx.x >> 6;
    __syncthreads();
    if ((threadIdx.x & 63) == 0) S->ired[4 + w] = c;
    __syncthreads();
    int s = 0;
    for (int j = 0; j < (int)(blockDim.x >> 6); ++j) s += S->ired[4 + j];
    __syncthreads();
    return s;
}

// k-th smallest (0-based) of v[0..cnt); all threads return the same value.  Every pass ends the search or removes at least one distinct value
// from the candidates [lo, hi]: an infinite end is split off by counting its copies (they hold rank kk, or they leave), and the bucketing then
// works on finite lo < hi, puts lo in bucket 0 and hi in bucket WX_NB - 1, so the bucket it narrows to misses lo or hi.
template <typename T>
__device__ T wx_select_kth(const T *v, int cnt, int k, WxSelScratch *S)
{
    const T inf = (T)INFINITY;
    T lo, hi;
    wx_block_minmax(v, cnt, [](T) { return true; }, S, lo, hi);
    int kk = k;                                       // rank among the candidates lo <= x <= hi
    for (;;) {
        if (!(lo < hi)) return lo;                    // all candidates equal (or NaN-degenerate)
        if (lo == -inf) {
            // rare: the copies of -Inf hold ranks 0 ... c - 1; else the search goes on above them
            const int c = wx_block_count(v, cnt, [](T x) { return x == -(T)INFINITY; }, S);
            if (kk < c) return lo;
            kk -= c;
            const T chi = hi;
            T nlo, nhi;
            wx_block_minmax(v, cnt, [chi](T x) { return x > -(T)INFINITY && x <= chi; }, S, nlo, nhi);
            lo = nlo;
            continue;
        }
        if (hi == inf) {
            // rare: the c finite candidates rank below the copies of +Inf
            const T clo = lo;
            if (kk >= wx_block_count(v, cnt, [clo](T x) { return x >= clo && x < (T)INFINITY; }, S)) return hi;
            T nlo, nhi;
            wx_block_minmax(v, cnt, [clo](T x) { return x >= clo && x < (T)INFINITY; }, S, nlo, nhi);
            hi = nhi;
            continue;
        }
        // finite lo < hi.  The offsets are taken on the values times sh: 1, or 1/2 where hi - lo overflows, or 2^900 where WX_NB / (hi - lo)
        // would (then every candidate is below 2^-947 in magnitude and the scaling is exact).  The scale is finite, x -> (x sh - lo sh) scale
        // rounds monotonically, lo maps to 0 and hi to WX_NB up to rounding: buckets 0 and WX_NB - 1.  (sh = 1 is the plain x - lo.)
        const double dr = (double)hi - (double)lo;
        const double sh = !(dr <= 1.7976931348623157e308) ? 0.5 : (dr < 0x1p-1000 ? 0x1p900 : 1.0);
        const double losh = (double)lo * sh;
        const double scale = (double)WX_NB / ((double)hi * sh - losh);
        auto bucket = [&](T x) { int b = (int)(((double)x * sh - losh) * scale); return b < WX_NB ? b : WX_NB - 1; };
        for (int i = threadIdx.x; i < WX_NB; i += blockDim.x) S->hist[i] = 0;
        __syncthreads();
        for (int i = threadIdx.x; i < cnt; i += blockDim.x) {
            const T x = v[i];
            if (x >= lo && x <= hi) atomicAdd(&S->hist[bucket(x)], 1u);
        }
        __syncthreads();
        if (threadIdx.x == 0) S->ired[2] = -1;
        __syncthreads();
        if (threadIdx.x < 64) {
            // lane l owns buckets 16l .. 16l+15: wave-wide scan of the lane sums, then the crossing bucket
            unsigned sum = 0;
            for (int j = 0; j < WX_NB / 64; ++j) sum += S->hist[(WX_NB / 64) * threadIdx.x + j];
            unsigned incl = sum;
            for (int o = 1; o < 64; o <<= 1) { const unsigned up = __shfl_up(incl, o, 64); if ((int)threadIdx.x >= o) incl += up; }
            const unsigned excl = incl - sum;
            if ((unsigned)kk >= excl && (unsigned)kk < incl) {
                unsigned c = excl;
                int b = (WX_NB / 64) * threadIdx.x;
                const int bend = b + WX_NB / 64 - 1;
                while (b < bend && (unsigned)kk >= c + S->hist[b]) { c += S->hist[b]; ++b; }
                S->ired[0] = b; S->ired[1] = (int)c; S->ired[2] = (int)S->hist[b];
            }
        }
        __syncthreads();
        const int bsel = S->ired[0], before = S->ired[1], cb = S->ired[2];
        if (cb < 0) return (T)NAN;                     // rank beyond the comparable elements (NaNs in the data)
        if (cb <= WX_LST) {
            // gather the bucket's candidates and rank them (ties by slot): the (kk - before)-th is the answer
            if (threadIdx.x == 0) S->ired[3] = 0;
            __syncthreads();
            for (int i = threadIdx.x; i < cnt; i += blockDim.x) {
                const T x = v[i];
                if (x >= lo && x <= hi && bucket(x) == bsel) S->lst[atomicAdd(&S->ired[3], 1)] = (double)x;
            }
            __syncthreads();
            const int want = kk - before;
            for (int s = threadIdx.x; s < cb; s += blockDim.x) {       // (one round for workgroups of WX_LST lanes and more)
                const double x = S->lst[s];
                int rank = 0;
                for (int j = 0; j < cb; ++j) { const double y = S->lst[j]; rank += (y < x) || (y == x && j < s); }
                if (rank == want) S->red[2 * WX_SELW] = x;
            }
            __syncthreads();
            const T r = (T)S->red[2 * WX_SELW];
            __syncthreads();
            return r;
        }
        // too many candidates in one bucket: narrow to that bucket's own range and repeat
        T nlo, nhi;
        const T clo = lo, chi = hi;
        wx_block_minmax(v, cnt, [&](T x) { return x >= clo && x <= chi && bucket(x) == bsel; }, S, nlo, nhi);
        lo = nlo; hi = nhi; kk -= before;
    }
}

// median as Statistics.median!: middle element, or middle(a, b) = a/2 + b/2 of the two middle ones
template <typename T> __device__ T wx_median_lds(const T *v, int cnt, WxSelScratch *S)
{
    const T a = wx_select_kth<T>(v, cnt, (cnt - 1) / 2, S);
    if (cnt & 1) return a;
    // the next order statistic: a again if at least (cnt/2 + 1) elements are <= a, else the smallest element > a
    int le = 0;
    T nx = (T)INFINITY;
    for (int i = threadIdx.x; i < cnt; i += blockDim.x) { const T x = v[i]; le += x <= a; if (x > a && x < nx) nx = x; }
    nx = wx_wave_min(nx);
    for (int o = 32; o > 0; o >>= 1) le += __shfl_xor(le, o, 64);
    const int w = threadIdx.x >> 6;
    __syncthreads();
    if ((threadIdx.x & 63) == 0) { S->red[w] = (double)nx; S->ired[4 + w] = le; }
    __syncthreads();
    double m = S->red[0];
    int tot = S->ired[4];
    for (int j = 1; j < (int)(blockDim.x >> 6); ++j) { m = S->red[j] < m ? S->red[j] : m; tot += S->ired[4 + j]; }
    __syncthreads();
    const T b = tot >= cnt / 2 + 1 ? a : (T)m;
    return dn_middle<T>(a, b);
}

}  // namespace
