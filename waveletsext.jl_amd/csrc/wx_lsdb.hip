// wx_lsdb.hip -- least statistically dependent basis (LSDB): differential-entropy costs of a packet table for gfx950.
//
// Reference (paths relative to /root/reference/src/mod):
//   tree_costs(X::Array{T,3}, ::LSDB)  bestbasis/bestbasis_tree.jl:104-126 (1-D), tree_costs(X::Array{T,4}, ::LSDB) :128-147 (2-D)
//       node cost = coefcost(the node's block of X, DifferentialEntropyCost()); redundant: coefcost(X[.., i, :]) / 2^d (4^d)
//   coefcost(x::AbstractArray, ::DifferentialEntropyCost)  bestbasis/bestbasis_costs.jl:157-164: the sum, in Float64, of the
//       per-row cost of every coefficient position of the block (a row = that position's N values, one per signal)
//   coefcost(x::Vector, ::DifferentialEntropyCost)  :135-155, N = length(x):
//       nbins = ceil((30N)^(1/5)), mbins = ceil(50 / nbins); sigma = std(x) (corrected);
//       delta = (max - min + sigma) / ((nbins + 1) mbins - 1); rng = (min - 0.5 sigma):delta:(max + 0.5 sigma);
//       epdf = ash(x, rng = rng, m = mbins, kernel = triangular); cost = -(1/N) sum_k log(pdf(epdf, x[k]))
// Two rules come from outside the reference tree (neither Julia Base nor AverageShiftedHistograms.jl is in it) and are
// restated here; parity with them is unpinned, like the other ASH paths (wx_ldbstat.hip):
//   * the length of the float range start:step:stop (Base's fallback for IEEE floats): lf = (stop - start) / step,
//     len = round(lf) + 1 (ties to even), minus one if start + (len - 1) step > stop.  Base takes a rational branch instead
//     when start, step and stop all have exact small-rational forms, which the data of a real table do not have; the
//     length is (nbins + 1) mbins or one less, and it changes the density's normalisation, so it is part of parity.
//   * ash / pdf: bin of an observation ki = floor((y - first(rng)) / step + 1.5) (1-based, counted if 1 <= ki <= len);
//     density[i] = sum over the bins k with |i - k| < m of counts[k] (1 - |i - k| / m), scaled by 1 / (sum(density) step);
//     pdf(x) interpolates the density linearly between the two points of rng around x (searchsortedlast), 0 outside;
//     rng[j] = first + (j - 1) step.
// Float32 input: min, max, sigma and delta are Float32 as in the reference; sigma is computed in Float64 and rounded to
// Float32 (within about an ulp of Julia's Float32 std).  sigma is the correctly rounded standard deviation of the row's exact
// values; Julia's std (pairwise sums, two passes) is within an ulp or two of it, which is the unpinned part of the grid length.  The range ends are Float64 (0.5 is a Float64 literal), the density,
// the log-likelihood and the cost are Float64.  The reference throws for a row with max == min ("range step cannot be zero"),
// N == 1 and non-finite values; such a row sets the status word (the lowest offending row) and the call returns WX_EARG.
//
// X is seen as (nk, N) column-major.  Every kernel gives a lane one row (coefficient position) and a workgroup 64
// consecutive rows, so each load of a signal's values is one contiguous 512-byte (256-byte) run; the signal axis is split
// into chunks across workgroups when the row tiles alone cannot fill the GPU.  Three streamed passes over X:
//   1. k_lsdb_stats: per (chunk, row) min, max and the double-double sums of x and x^2 -> k_lsdb_grid: chunks merged in
//      order, sigma (correctly rounded), delta, range start and length;
//   2. k_lsdb_count: integer bin counts of the chunk in LDS ([bin][lane]: a lane's column is its own, no atomics), written
//      per chunk -> k_lsdb_sumcounts: chunks summed (integers: exact) -> k_lsdb_density: the triangular smoothing and the
//      normalisation;
//   3. k_lsdb_logsum: the row's density in LDS ([bin][lane], Float64: conflict free), sum of log pdf(x) per chunk
//      -> k_lsdb_finish: chunks summed in order.
// The table is streamed three times rather than staged in LDS once: a row of a table worth the GPU has thousands of values
// (the second and third reads of a small table come from the caches).  Every combine runs in a fixed order and there are no
// floating-point atomics, so the costs are the same to the bit from run to run.  The node sums (k_lsdb_nodes1d / 2d) are
// workgroup reductions in a fixed order over the node geometry of wx_nodegeom.h, shared with JBB.
#include "../../include/waveletsext_hip.h"     // the definitions below must match the public prototypes
#include "wx_common.h"
#include "wx_host.h"
#include "wx_nodegeom.h"
#include <cmath>
#include <string>

#define WX_REQUIRE(cond, code, msg) \
    do { if (!(cond)) return wx_set_error(code, msg); } while (0)

extern "C" int wx_device_count(void);

namespace {

constexpr int LD_NT = 64;          // one wave per workgroup, lane = row
constexpr int LD_U = 8;            // values per lane in flight
constexpr int LD_WAVES = 2048;     // waves the streamed passes aim for (8 per CU) before the signal axis is split further
constexpr int LD_MINCHUNK = 256;   // no chunk shorter than this many signals

struct LdStat { double sh, sl, qh, ql, mn, mx; };  // per (chunk, row): sum and sum of squares as double-doubles, extrema
struct LdGrid { double a, delta; int len, pad; };   // per row; len = 0 marks a degenerate row

// Double-double arithmetic (error-free transformations; this file is compiled without contraction, fma() is explicit).  The
// sums of x and x^2 carry about 106 bits, so sigma below is the correctly rounded standard deviation of the row's exact values
// (up to ties at the 1e-30 level) whatever the order of the sums: the chunking of the signal axis does not move it by an ulp.
// That matters: the grid length, (stop - start) / step = (nbins + 1) mbins - 1 up to a few ulps, is decided by those ulps.
struct Dd { double h, l; };
__device__ __forceinline__ Dd dd_fast(double a, double b) { const double s = a + b; return Dd{s, b - (s - a)}; }
__device__ __forceinline__ Dd dd_two_sum(double a, double b)
{
    const double s = a + b, bb = s - a;
    return Dd{s, (a - (s - bb)) + (b - bb)};
}
__device__ __forceinline__ Dd dd_add(Dd a, Dd b)
{
    const Dd s = dd_two_sum(a.h, b.h);
    return dd_fast(s.h, s.l + (a.l + b.l));
}
__device__ __forceinline__ Dd dd_neg(Dd a) { return Dd{-a.h, -a.l}; }
__device__ __forceinline__ Dd dd_sq(double v) { const double p = v * v; return Dd{p, fma(v, v, -p)}; }
__device__ __forceinline__ Dd dd_mul(Dd a, Dd b)
{
    const double p = a.h * b.h;
    return dd_fast(p, fma(a.h, b.h, -p) + (a.h * b.l + a.l * b.h));
}
__device__ __forceinline__ Dd dd_div(Dd a, double d)
{
    const double q1 = a.h / d, p = q1 * d;
    const Dd r = dd_add(a, Dd{-p, -fma(q1, d, -p)});
    return dd_fast(q1, r.h / d);
}

template <typename T>
__global__ __launch_bounds__(LD_NT) void k_lsdb_stats(const T *__restrict__ X, int64_t nk, int64_t N, int64_t chunk,
                                                      LdStat *__restrict__ part)
{
    const int64_t e = (int64_t)blockIdx.x * LD_NT + threadIdx.x;
    if (e >= nk) return;
    const int64_t c = blockIdx.y, b0 = c * chunk, b1 = b0 + chunk < N ? b0 + chunk : N;
    const T *p = X + e;
    Dd S{0, 0}, Q{0, 0};
    T mn = p[b0 * nk], mx = mn;
    int64_t b = b0;
    for (; b + LD_U <= b1; b += LD_U) {
        T v[LD_U];
#pragma unroll
        for (int u = 0; u < LD_U; ++u) v[u] = p[(b + u) * nk];
#pragma unroll
        for (int u = 0; u < LD_U; ++u) {
            const double x = (double)v[u];
            S = dd_add(S, Dd{x, 0.0});
            Q = dd_add(Q, dd_sq(x));
            mn = v[u] < mn ? v[u] : mn;
            mx = v[u] > mx ? v[u] : mx;
        }
    }
    for (; b < b1; ++b) {
        const T v = p[b * nk];
        S = dd_add(S, Dd{(double)v, 0.0});
        Q = dd_add(Q, dd_sq((double)v));
        mn = v < mn ? v : mn;
        mx = v > mx ? v : mx;
    }
    // a NaN is skipped by the comparisons above but poisons the sums, which flags the row
    part[c * nk + e] = LdStat{S.h, S.l, Q.h, Q.l, (double)mn, (double)mx};
}

// the range of one row from the merged statistics, Float32 / Float64 rules of the reference
template <typename T> __device__ void ld_range(double sigma, double mn, double mx, int len0, double &a, double &stop, double &delta);
template <> __device__ void ld_range<double>(double sigma, double mn, double mx, int len0, double &a, double &stop, double &delta)
{
    delta = (mx - mn + sigma) / (double)(len0 - 1);
    a = mn - 0.5 * sigma;
    stop = mx + 0.5 * sigma;
}
template <> __device__ void ld_range<float>(double sigma, double mn, double mx, int len0, double &a, double &stop, double &delta)
{
    const float sf = (float)sigma, mnf = (float)mn, mxf = (float)mx;
    const float w = mxf - mnf;
    const float df = (w + sf) / (float)(len0 - 1);
    delta = (double)df;
    a = (double)mnf - 0.5 * (double)sf;
    stop = (double)mxf + 0.5 * (double)sf;
}

template <typename T>
__global__ __launch_bounds__(256) void k_lsdb_grid(const LdStat *__restrict__ part, int64_t nk, int64_t N, int64_t chunk,
                                                   int nchunks, int len0, LdGrid *__restrict__ grid,
                                                   unsigned long long *__restrict__ status)
{
    const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= nk) return;
    Dd S{0, 0}, Q{0, 0};
    double mn = 0, mx = 0;
#pragma unroll 8
    for (int c = 0; c < nchunks; ++c) {
        const LdStat s = part[(int64_t)c * nk + e];
        if (c == 0) { mn = s.mn; mx = s.mx; }
        else { mn = s.mn < mn ? s.mn : mn; mx = s.mx > mx ? s.mx : mx; }
        S = dd_add(S, Dd{s.sh, s.sl});
        Q = dd_add(Q, Dd{s.qh, s.ql});
    }
    // var = (sum x^2 - (sum x)^2 / N) / (N - 1) in double-double; sigma = its square root rounded once (one Newton step on the
    // double root)
    const Dd V = dd_div(dd_add(Q, dd_neg(dd_div(dd_mul(S, S), (double)N))), (double)(N - 1));
    double sigma = V.h;                                        // 0 stays 0, NaN stays NaN
    if (V.h > 0.0) {
        const double s0 = sqrt(V.h);
        const Dd r = dd_add(V, dd_neg(dd_sq(s0)));
        sigma = s0 + (r.h + r.l) / (2.0 * s0);
    }
    double a, stop, delta;
    ld_range<T>(sigma, mn, mx, len0, a, stop, delta);
    bool ok = N >= 2 && mx > mn && isfinite(S.h) && isfinite(Q.h) && sigma >= 0.0 && isfinite(sigma) && isfinite(mn) &&
              isfinite(mx) && delta > 0.0 && isfinite(delta);
    int len = 0;
    if (ok) {
        // Base's fallback length of start:step:stop
        const double lf = (stop - a) / delta;
        int64_t l = (int64_t)rint(lf) + 1;
        const double stopp = a + (double)(l - 1) * delta;
        if (a < stop && stop < stopp) --l;
        ok = l >= 2 && l <= len0;
        len = ok ? (int)l : 0;
    }
    if (!ok) atomicMin(status, (unsigned long long)e);
    grid[e] = LdGrid{a, delta, len, 0};
}

template <typename T>
__global__ __launch_bounds__(LD_NT) void k_lsdb_count(const T *__restrict__ X, int64_t nk, int64_t N, int64_t chunk,
                                                      const LdGrid *__restrict__ grid, int len0, int *__restrict__ cpart)
{
    extern __shared__ __attribute__((aligned(16))) char ld_smem[];
    int *cnt = reinterpret_cast<int *>(ld_smem);            // [len0][64]
    const int lane = threadIdx.x;
    const int64_t e = (int64_t)blockIdx.x * LD_NT + lane;
    const int64_t c = blockIdx.y, b0 = c * chunk, b1 = b0 + chunk < N ? b0 + chunk : N;
    for (int i = 0; i < len0; ++i) cnt[i * LD_NT + lane] = 0;
    if (e >= nk) return;                                     // lanes own their columns: no barrier needed
    const LdGrid g = grid[e];
    if (g.len > 0) {
        const T *p = X + e;
        const double hi = (double)g.len;
        int64_t b = b0;
        for (; b + LD_U <= b1; b += LD_U) {
            T v[LD_U];
#pragma unroll
            for (int u = 0; u < LD_U; ++u) v[u] = p[(b + u) * nk];
#pragma unroll
            for (int u = 0; u < LD_U; ++u) {
                const double ki = floor(((double)v[u] - g.a) / g.delta + 1.5);
                if (ki >= 1.0 && ki <= hi) ++cnt[((int)ki - 1) * LD_NT + lane];
            }
        }
        for (; b < b1; ++b) {
            const double ki = floor(((double)p[b * nk] - g.a) / g.delta + 1.5);
            if (ki >= 1.0 && ki <= hi) ++cnt[((int)ki - 1) * LD_NT + lane];
        }
    }
    for (int i = 0; i < len0; ++i) cpart[(c * len0 + i) * nk + e] = cnt[i * LD_NT + lane];
}

// counts of all chunks (integers: the order does not matter) -> tot[bin * nk + e].  Workgroup: one bin of 64 rows x 16 waves,
// wave w adds chunks w, w + 16, ...
constexpr int LD_DW = 16;
__global__ __launch_bounds__(LD_NT * LD_DW) void k_lsdb_sumcounts(const int *__restrict__ cpart, int64_t nk, int nchunks, int len0,
                                                                  int *__restrict__ tot)
{
    __shared__ int red[LD_DW][LD_NT];
    const int lane = threadIdx.x & (LD_NT - 1), w = threadIdx.x / LD_NT, i = blockIdx.y;
    const int64_t e = (int64_t)blockIdx.x * LD_NT + lane;
    int s = 0;
    if (e < nk) {
#pragma unroll 4
        for (int c = w; c < nchunks; c += LD_DW) s += cpart[((int64_t)c * len0 + i) * nk + e];
    }
    red[w][lane] = s;
    __syncthreads();
    if (w != 0 || e >= nk) return;
    for (int v = 1; v < LD_DW; ++v) s += red[v][lane];
    tot[(int64_t)i * nk + e] = s;
}

// total counts -> normalised density dens[bin * nk + e] (the row's counts in LDS, [bin][lane])
__global__ __launch_bounds__(LD_NT) void k_lsdb_density(const int *__restrict__ tot, int64_t nk, int mbins,
                                                        const LdGrid *__restrict__ grid, double *__restrict__ dens)
{
    extern __shared__ __attribute__((aligned(16))) char ld_smem[];
    int *cnt = reinterpret_cast<int *>(ld_smem);            // [len][64]
    const int lane = threadIdx.x;
    const int64_t e = (int64_t)blockIdx.x * LD_NT + lane;
    if (e >= nk) return;                                     // lanes own their columns: no barrier needed
    const LdGrid g = grid[e];
    const int len = g.len;
    for (int i = 0; i < len; ++i) cnt[i * LD_NT + lane] = tot[(int64_t)i * nk + e];
    double sum = 0;
    for (int i = 0; i < len; ++i) {
        double d = 0;
        const int k0 = i - mbins + 1 > 0 ? i - mbins + 1 : 0, k1 = i + mbins - 1 < len - 1 ? i + mbins - 1 : len - 1;
        for (int k = k0; k <= k1; ++k) {
            const int ck = cnt[k * LD_NT + lane];
            if (ck) d += ck * (1.0 - fabs((double)(i - k) / mbins));
        }
        dens[(int64_t)i * nk + e] = d;
        sum += d;
    }
    const double scale = 1.0 / (sum * g.delta);
    for (int i = 0; i < len; ++i) dens[(int64_t)i * nk + e] *= scale;
}

template <typename T>
__global__ __launch_bounds__(LD_NT) void k_lsdb_logsum(const T *__restrict__ X, int64_t nk, int64_t N, int64_t chunk,
                                                       const LdGrid *__restrict__ grid, const double *__restrict__ dens, int len0,
                                                       double *__restrict__ lpart)
{
    extern __shared__ __attribute__((aligned(16))) char ld_smem[];
    double *dl = reinterpret_cast<double *>(ld_smem);       // [len0][64]
    const int lane = threadIdx.x;
    const int64_t e = (int64_t)blockIdx.x * LD_NT + lane;
    if (e >= nk) return;                                     // lanes own their columns: no barrier needed
    const int64_t c = blockIdx.y, b0 = c * chunk, b1 = b0 + chunk < N ? b0 + chunk : N;
    const LdGrid g = grid[e];
    double s = 0;
    if (g.len > 0) {
        for (int i = 0; i < g.len; ++i) dl[i * LD_NT + lane] = dens[(int64_t)i * nk + e];
        const double a = g.a, delta = g.delta, dinv = 1.0 / delta;
        const int len = g.len;
        // pdf(epdf, x): j = searchsortedlast(rng, x) by a guess and exact corrections, then linear interpolation
        auto lpdf = [&](double x) {
            double t = floor((x - a) * dinv) + 1.0;
            t = t < 0.0 ? 0.0 : (t > (double)len ? (double)len : t);
            int j = (int)t;
            while (j >= 1 && a + (double)(j - 1) * delta > x) --j;
            while (j < len && a + (double)j * delta <= x) ++j;
            double w = 0.0;
            if (j >= 1 && j < len) {
                const double r0 = a + (double)(j - 1) * delta, r1 = a + (double)j * delta;
                const double d0 = dl[(j - 1) * LD_NT + lane], d1 = dl[j * LD_NT + lane];
                w = d0 + (d1 - d0) * (x - r0) / (r1 - r0);
            }
            return log(w);
        };
        const T *p = X + e;
        int64_t b = b0;
        for (; b + LD_U <= b1; b += LD_U) {
            T v[LD_U];
#pragma unroll
            for (int u = 0; u < LD_U; ++u) v[u] = p[(b + u) * nk];
#pragma unroll
            for (int u = 0; u < LD_U; ++u) s += lpdf((double)v[u]);
        }
        for (; b < b1; ++b) s += lpdf((double)p[b * nk]);
    }
    lpart[c * nk + e] = s;
}

__global__ __launch_bounds__(256) void k_lsdb_finish(const double *__restrict__ lpart, int64_t nk, int64_t N, int nchunks,
                                                     const LdGrid *__restrict__ grid, double *__restrict__ E)
{
    const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= nk) return;
    double s = 0;
#pragma unroll 8
    for (int c = 0; c < nchunks; ++c) s += lpart[(int64_t)c * nk + e];
    E[e] = grid[e].len > 0 ? -(1.0 / (double)N) * s : __longlong_as_double(0x7ff8000000000000LL);
}

__device__ double ld_block_sum(double v, double *red)
{
    red[threadIdx.x] = v;
    __syncthreads();
    for (int w = 128; w > 0; w >>= 1) {
        if ((int)threadIdx.x < w) red[threadIdx.x] += red[threadIdx.x + w];
        __syncthreads();
    }
    return red[0];
}

// one workgroup per cost entry: the Float64 sum of the node's row entropies, / 2^d when redundant, stored as T
template <typename T>
__global__ __launch_bounds__(256) void k_lsdb_nodes1d(const double *__restrict__ E, int n, int redundant, T *__restrict__ costs)
{
    __shared__ double red[256];
    const WxNode1d g = wx_node1d((int)blockIdx.x, n, redundant);
    double acc = 0;
    for (int i = threadIdx.x; i < g.len; i += 256) acc += E[(int64_t)g.col * n + g.off + i];
    const double s = ld_block_sum(acc, red);
    if (threadIdx.x == 0) costs[blockIdx.x] = (T)(redundant ? s / (double)((int64_t)1 << g.depth) : s);
}

template <typename T>
__global__ __launch_bounds__(256) void k_lsdb_nodes2d(const double *__restrict__ E, int m, int n, int redundant, T *__restrict__ costs)
{
    __shared__ double red[256];
    const WxNode2d g = wx_node2d((int64_t)blockIdx.x, m, n, redundant);
    double acc = 0;
    const int cnt = g.nr * g.ncl;
    for (int i = threadIdx.x; i < cnt; i += 256) {
        const int r = g.r0 + i % g.nr, c = g.c0 + i / g.nr;
        acc += E[g.slice * (int64_t)m * n + (int64_t)c * m + r];
    }
    const double s = ld_block_sum(acc, red);
    if (threadIdx.x == 0) costs[blockIdx.x] = (T)(redundant ? s / (double)((int64_t)1 << (2 * g.depth)) : s);
}

int need_device()
{
    if (wx_device_count() < 1) return wx_set_error(WX_EHIP, "no HIP device visible: the MI355X kernels cannot run");
    return WX_OK;
}

// nbins, mbins and the largest grid length (nbins + 1) mbins of a row of N values (bestbasis_costs.jl:138-141)
void ld_params(int64_t N, int *mbins, int *len0)
{
    const int nbins = (int)std::ceil(std::pow((double)(30 * N), 1.0 / 5.0));
    *mbins = (50 + nbins - 1) / nbins;
    *len0 = (nbins + 1) * *mbins;
}

// per-row entropies E[nk] (device) of X (device, (nk, N)); *bad = lowest degenerate row or -1.  Synchronises the stream.
template <typename T>
int ld_entropy(const T *dX, int64_t nk, int64_t N, double *dE, hipStream_t st, WxScratch &scr, int64_t *bad)
{
    int mbins, len0;
    ld_params(N, &mbins, &len0);
    const int64_t tiles = (nk + LD_NT - 1) / LD_NT;
    int64_t nchunks = (LD_WAVES + tiles - 1) / tiles;
    const int64_t maxch = (N + LD_MINCHUNK - 1) / LD_MINCHUNK;
    if (nchunks > maxch) nchunks = maxch;
    if (nchunks > 65535) nchunks = 65535;
    if (nchunks < 1) nchunks = 1;
    int64_t chunk = (N + nchunks - 1) / nchunks;
    nchunks = (N + chunk - 1) / chunk;                       // no empty chunk
    WX_REQUIRE(tiles <= 0x7fffffff, WX_EUNSUPPORTED, "LSDB: too many coefficients per signal");
    LdStat *part = (LdStat *)scr.alloc(sizeof(LdStat) * nchunks * nk);
    LdGrid *grid = (LdGrid *)scr.alloc(sizeof(LdGrid) * nk);
    int *cpart = (int *)scr.alloc(sizeof(int) * nchunks * len0 * nk);
    int *tot = (int *)scr.alloc(sizeof(int) * len0 * nk);
    double *dens = (double *)scr.alloc(sizeof(double) * len0 * nk);
    double *lpart = (double *)scr.alloc(sizeof(double) * nchunks * nk);
    unsigned long long *status = (unsigned long long *)scr.alloc(sizeof(unsigned long long));
    if (!part || !grid || !cpart || !tot || !dens || !lpart || !status) return WX_EHIP;
    WX_HIP_CHECK(hipMemsetAsync(status, 0xff, sizeof(unsigned long long), st));
    const dim3 g2((unsigned)tiles, (unsigned)nchunks), g1((unsigned)((nk + 255) / 256));
    const size_t lds_cnt = sizeof(int) * len0 * LD_NT, lds_dens = sizeof(double) * len0 * LD_NT;
    WX_REQUIRE(lds_dens <= 160 * 1024, WX_EUNSUPPORTED, "LSDB: too many histogram bins for the LDS");
    if (lds_dens > 64 * 1024)
        WX_HIP_CHECK(hipFuncSetAttribute(reinterpret_cast<const void *>(k_lsdb_logsum<T>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_dens));
    if (lds_cnt > 64 * 1024) {
        WX_HIP_CHECK(hipFuncSetAttribute(reinterpret_cast<const void *>(k_lsdb_count<T>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_cnt));
        WX_HIP_CHECK(hipFuncSetAttribute(reinterpret_cast<const void *>(k_lsdb_density), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_cnt));
    }
    hipLaunchKernelGGL(k_lsdb_stats<T>, g2, dim3(LD_NT), 0, st, dX, nk, N, chunk, part);
    hipLaunchKernelGGL(k_lsdb_grid<T>, g1, dim3(256), 0, st, part, nk, N, chunk, (int)nchunks, len0, grid, status);
    hipLaunchKernelGGL(k_lsdb_count<T>, g2, dim3(LD_NT), lds_cnt, st, dX, nk, N, chunk, grid, len0, cpart);
    hipLaunchKernelGGL(k_lsdb_sumcounts, dim3((unsigned)tiles, (unsigned)len0), dim3(LD_NT * LD_DW), 0, st, cpart, nk, (int)nchunks, len0, tot);
    hipLaunchKernelGGL(k_lsdb_density, dim3((unsigned)tiles), dim3(LD_NT), lds_cnt, st, tot, nk, mbins, grid, dens);
    hipLaunchKernelGGL(k_lsdb_logsum<T>, g2, dim3(LD_NT), lds_dens, st, dX, nk, N, chunk, grid, dens, len0, lpart);
    hipLaunchKernelGGL(k_lsdb_finish, g1, dim3(256), 0, st, lpart, nk, N, (int)nchunks, grid, dE);
    WX_HIP_CHECK(hipGetLastError());
    unsigned long long h = 0;
    WX_HIP_CHECK(hipMemcpyAsync(&h, status, sizeof(h), hipMemcpyDeviceToHost, st));
    WX_HIP_CHECK(hipStreamSynchronize(st));
    *bad = h == ~0ULL ? -1 : (int64_t)h;
    return WX_OK;
}

std::string ld_reason(int64_t N)
{
    return N < 2 ? "one signal: std of a single value is NaN (the reference throws)"
                 : "range step cannot be zero (a constant or non-finite coefficient row)";
}

template <typename T>
int api_entropy(const T *X, int64_t nk, int64_t N, double *E, void *stream)
{
    WX_REQUIRE(nk >= 1 && N >= 1, WX_EARG, "bad dimensions");
    int rc;
    if ((rc = need_device())) return rc;
    hipStream_t st = wx_stream(stream);
    WxScratch scr(st);
    WxIO io(st);
    const T *dX = (const T *)io.in(X, sizeof(T) * nk * N);
    double *dE = (double *)io.out(E, sizeof(double) * nk);
    if (!dX || !dE) return io.finish(WX_EHIP);
    int64_t bad = -1;
    if ((rc = ld_entropy<T>(dX, nk, N, dE, st, scr, &bad))) return io.finish(rc);
    if (bad >= 0) {
        static thread_local std::string msg;
        msg = "LSDB DifferentialEntropyCost: " + ld_reason(N) + " at coefficient row " + std::to_string(bad);
        return io.finish(wx_set_error(WX_EARG, msg.c_str()));
    }
    return io.finish(WX_OK);
}

// 1-D (n, k, N) when m == 0, else 2-D (m rows, n cols, k, N)
template <typename T>
int api_costs(const T *X, int64_t m, int64_t n, int64_t k, int64_t N, int redundant, T *costs, void *stream)
{
    const bool two = m > 0;
    WX_REQUIRE(n >= 1 && k >= 1 && N >= 1, WX_EARG, "bad dimensions");
    if (!redundant) {
        if (two) WX_REQUIRE(k - 1 <= wx_maxtransformlevels(m < n ? m : n) && k <= 14, WX_EASSERT, "more packet levels than the image admits");
        else WX_REQUIRE(k - 1 <= wx_maxtransformlevels(n) && k <= 30, WX_EASSERT, "more packet levels than the signal admits");
    }
    WX_REQUIRE(n < ((int64_t)1 << 31) && m < ((int64_t)1 << 31) && k <= 0x7fffffff, WX_EUNSUPPORTED, "LSDB: table too large");
    int rc;
    if ((rc = need_device())) return rc;
    const int64_t rows = two ? m : n, nk = rows * (two ? n : 1) * k;
    const int64_t ncost = redundant ? k : two ? ((((int64_t)1 << (2 * k)) - 1) / 3) : (((int64_t)1 << k) - 1);
    WX_REQUIRE(ncost <= 0x7fffffff, WX_EUNSUPPORTED, "LSDB: too many tree nodes");
    hipStream_t st = wx_stream(stream);
    WxScratch scr(st);
    WxIO io(st);
    const T *dX = (const T *)io.in(X, sizeof(T) * nk * N);
    T *dc = (T *)io.out(costs, sizeof(T) * ncost);
    double *dE = (double *)scr.alloc(sizeof(double) * nk);
    if (!dX || !dc || !dE) return io.finish(WX_EHIP);
    int64_t bad = -1;
    if ((rc = ld_entropy<T>(dX, nk, N, dE, st, scr, &bad))) return io.finish(rc);
    if (bad >= 0) {
        // name the coefficient and the first node (heap order) whose block holds it
        const int64_t per = two ? m * n : n, col = bad / per, pos = bad % per;
        std::string where;
        if (two) {
            const int64_t r = pos % m, c = pos / m;
            where = "coefficient (" + std::to_string(r + 1) + ", " + std::to_string(c + 1) + ") of slice " + std::to_string(col + 1);
            if (!redundant) {
                const int64_t nr = m >> col, nc = n >> col, jr = r / nr, jc = c / nc;
                int64_t start = 1, mort = 0;
                for (int64_t t = 0; t < col; ++t) start = 4 * start - 2;
                for (int64_t t = 0; t < col; ++t) mort |= (((jr >> t) & 1) << (2 * t + 1)) | (((jc >> t) & 1) << (2 * t));
                where += ", node " + std::to_string(start + mort);
            } else where += ", node " + std::to_string(col + 1);
        } else {
            where = "coefficient " + std::to_string(pos + 1) + " of column " + std::to_string(col + 1);
            if (!redundant) where += ", node " + std::to_string(((int64_t)1 << col) + pos / (n >> col));
            else where += ", node " + std::to_string(col + 1);
        }
        static thread_local std::string msg;
        msg = "LSDB DifferentialEntropyCost: " + ld_reason(N) + " at " + where;
        return io.finish(wx_set_error(WX_EARG, msg.c_str()));
    }
    if (two) hipLaunchKernelGGL(k_lsdb_nodes2d<T>, dim3((unsigned)ncost), dim3(256), 0, st, dE, (int)m, (int)n, redundant, dc);
    else hipLaunchKernelGGL(k_lsdb_nodes1d<T>, dim3((unsigned)ncost), dim3(256), 0, st, dE, (int)n, redundant, dc);
    if (hipGetLastError() != hipSuccess) return io.finish(wx_set_error(WX_EHIP, "LSDB node-cost kernel failed to launch"));
    return io.finish(WX_OK);
}

}  // namespace

extern "C" {
int wx_lsdb_entropy_f64(const double *X, int64_t nk, int64_t N, double *E, void *stream)
{ return api_entropy<double>(X, nk, N, E, stream); }
int wx_lsdb_entropy_f32(const float *X, int64_t nk, int64_t N, double *E, void *stream)
{ return api_entropy<float>(X, nk, N, E, stream); }
int wx_lsdb_costs_f64(const double *X, int64_t n, int64_t k, int64_t N, int redundant, double *costs, void *stream)
{ return api_costs<double>(X, 0, n, k, N, redundant, costs, stream); }
int wx_lsdb_costs_f32(const float *X, int64_t n, int64_t k, int64_t N, int redundant, float *costs, void *stream)
{ return api_costs<float>(X, 0, n, k, N, redundant, costs, stream); }
int wx_lsdb_costs2d_f64(const double *X, int64_t m, int64_t n, int64_t k, int64_t N, int redundant, double *costs, void *stream)
{ return api_costs<double>(X, m, n, k, N, redundant, costs, stream); }
int wx_lsdb_costs2d_f32(const float *X, int64_t m, int64_t n, int64_t k, int64_t N, int redundant, float *costs, void *stream)
{ return api_costs<float>(X, m, n, k, N, redundant, costs, stream); }
}
