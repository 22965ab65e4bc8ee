// wx_wavemult.hip -- WaveMult: the Beylkin-Coifman-Rokhlin standard and non-standard forms of an operator and their products with
// a BATCH of vectors (src/mod/wavemult/{utils,transforms,mat2sparse,wavemult}.jl).
//
//   ns_dwt / ns_idwt      transforms.jl:52-70, 124-142   x (n, B) <-> nxw (2n, B); level l keeps s_l AND d_l (ndyad, utils.jl:146-155)
//   sft / isft            transforms.jl:171-228          L pyramid levels on every column, then on every row
//   sparse forms          mat2sparse.jl:38-55, 89-100    keep |Mw| > eps * max column norm; stretchmatrix (utils.jl:98-114) in closed form
//   the product           wavemult.jl:67-76, 143-152     y = idwt(SM * dwt(x)),  y = ns_idwt(NM * ns_dwt(x))
//
// One analysis / synthesis step is dwt_step! / idwt_step! (dwt/dwt_one_level.jl:79-107, 192-223) with (g, h) written out in the qmf q:
//   s[t] = sum_k q[k] v[2t + k],  d[t] = sum_k (-1)^k q[k] v[2t + 1 - k],
//   v[2t] = sum_m (q[2m] s[t - m] - q[2m+1] d[t + m]),  v[2t+1] = sum_m (q[2m+1] s[t - m] + q[2m] d[t + m])    (indices mod the node),
// in the reference's order of operations: Float64 products, one term added at a time, the running value rounded to the element type
// after every addition, no fused multiply-add (the Makefile builds this unit with -ffp-contract=off; the product below asks for its
// fma by name).  ns_dwt / ns_idwt therefore reproduce the reference's 16-digit doctest.  Nodes are dyadic, so the periodic wrap is
// a mask; a filter longer than the node wraps more than once and the mask covers that too.  Kernels are instantiated on the element
// type only, the filter length is a loop bound.
//
// The product Y (N, B) = A X (N, B) is row-oriented: the plan cuts the rows of A into pieces of at most `cap` entries ("virtual
// rows": a row far longer than the mean would otherwise stall its slice), groups 64 virtual rows into a slice padded to its longest
// member and stores a slice column-major, so a wavefront reads values and column indices coalesced.  A workgroup takes one slice and
// 32 signals (4 wavefronts x 8 accumulators): the slice's entries are read once per tile of signals, not once per signal.  Every
// element of Y is summed by ONE lane in ascending column order; the pieces of a cut row go to a side buffer and are added in
// ascending order by one thread.  No floating-point atomics anywhere: two runs give the same bits.  The plan is built on the host by
// a counting sort over the columns in order (deterministic, O(nnz), once per operator).
#include "../../include/waveletsext_hip.h"     // the definitions below must match the public prototypes
#include "wx_common.h"
#include "wx_host.h"
#include <algorithm>
#include <new>

#define WX_REQUIRE(cond, code, msg) \
    do { if (!(cond)) return wx_set_error(code, msg); } while (0)

extern "C" int wx_device_count(void);

namespace {

constexpr int NS_LDS_MAX = 4096;     // longest signal the one-workgroup ns_dwt / ns_idwt kernels keep in LDS (1.5 n elements, 48 KiB of Float64)
constexpr int SPMM_TS = 8;           // signals per wavefront of the product (accumulators per lane)
constexpr int SPMM_TILE = 4 * SPMM_TS;

// ------------------------------------------------------------------------------------------------------------------------------
// one-level steps on a node of `mask + 1` samples (analysis) / from two halves of `mask + 1` samples (synthesis)
// ------------------------------------------------------------------------------------------------------------------------------
template <typename T>
static __device__ __forceinline__ void ana_pair(const T *v, int mask, int t, const WxFilt &f, T &s, T &d)
{
    s = (T)(f.q[0] * (double)v[(2 * t) & mask]);
    d = (T)(f.q[0] * (double)v[(2 * t + 1) & mask]);
    for (int k = 1; k < f.F; ++k) {
        s = (T)((double)s + f.q[k] * (double)v[(2 * t + k) & mask]);
        d = (T)((double)d + ((k & 1) ? -f.q[k] : f.q[k]) * (double)v[(2 * t + 1 - k) & mask]);
    }
}

template <typename T>
static __device__ __forceinline__ void syn_pair(const T *s, const T *d, int mask, int t, const WxFilt &f, T &v0, T &v1)
{
    {
        const double sv = (double)s[t], dv = (double)d[t];
        v0 = (T)(f.q[0] * sv + -f.q[1] * dv);
        v1 = (T)(f.q[1] * sv + f.q[0] * dv);
    }
    for (int m = 1; m < f.F / 2; ++m) {
        const double sv = (double)s[(t - m) & mask], dv = (double)d[(t + m) & mask];
        v0 = (T)((double)v0 + (f.q[2 * m] * sv + -f.q[2 * m + 1] * dv));
        v1 = (T)((double)v1 + (f.q[2 * m + 1] * sv + f.q[2 * m] * dv));
    }
}

// ------------------------------------------------------------------------------------------------------------------------------
// ns_dwt / ns_idwt, signals that fit LDS: 256 / tps signals per workgroup, tps threads each (tps = min(n / 2, 256), a power of two).
// nxw of one signal, 0-based, h = n >> l: s_l at [2h, 3h), d_l at [3h, 4h); [0, n >> L) = s_L, [n >> L, 2 (n >> L)) stays 0.
// ------------------------------------------------------------------------------------------------------------------------------
template <typename T>
__global__ __launch_bounds__(256) void k_ns_dwt_lds(const T *__restrict__ x, T *__restrict__ nxw, int n, int L, int64_t batch, int tps,
                                                    WxFilt filt)
{
    extern __shared__ __align__(16) unsigned char wx_wm_smem[];
    const int spb = 256 / tps, sl = threadIdx.x / tps, tl = threadIdx.x % tps;
    const int64_t sig = (int64_t)blockIdx.x * spb + sl;
    const bool live = sig < batch;
    T *cur = reinterpret_cast<T *>(wx_wm_smem) + (size_t)sl * (n + n / 2);
    T *nxt = cur + n;
    const T *xi = x + (live ? sig : 0) * n;
    T *o = nxw + (live ? sig : 0) * 2 * n;
    if (live)
        for (int i = tl; i < n; i += tps) cur[i] = xi[i];
    __syncthreads();
    int nl = n;
    for (int l = 1; l <= L; ++l) {
        const int h = nl >> 1;
        if (live)
            for (int t = tl; t < h; t += tps) {
                T s, d;
                ana_pair(cur, nl - 1, t, filt, s, d);
                nxt[t] = s;
                o[2 * h + t] = s;
                o[3 * h + t] = d;
            }
        __syncthreads();
        T *sw = cur; cur = nxt; nxt = sw;
        nl = h;
    }
    if (live)
        for (int t = tl; t < nl; t += tps) {
            o[t] = cur[t];
            o[nl + t] = (T)0;
        }
}

template <typename T>
__global__ __launch_bounds__(256) void k_ns_idwt_lds(const T *__restrict__ nxw, T *__restrict__ x, int n, int L, int64_t batch, int tps,
                                                     WxFilt filt)
{
    extern __shared__ __align__(16) unsigned char wx_wm_smem[];
    const int spb = 256 / tps, sl = threadIdx.x / tps, tl = threadIdx.x % tps;
    const int64_t sig = (int64_t)blockIdx.x * spb + sl;
    const bool live = sig < batch;
    T *X = reinterpret_cast<T *>(wx_wm_smem) + (size_t)sl * (n + n / 2);
    T *W = X + n;
    const T *in = nxw + (live ? sig : 0) * 2 * n;
    if (live)
        for (int t = tl; t < (n >> L); t += tps) X[t] = in[t];
    __syncthreads();
    for (int l = L; l >= 1; --l) {
        const int h = n >> l;
        if (live)
            for (int t = tl; t < h; t += tps) W[t] = (T)(in[2 * h + t] + X[t]);        // transforms.jl:136
        __syncthreads();
        if (live)
            for (int t = tl; t < h; t += tps) {
                T v0, v1;
                syn_pair(W, in + 3 * h, h - 1, t, filt, v0, v1);
                X[2 * t] = v0;
                X[2 * t + 1] = v1;
            }
        __syncthreads();
    }
    if (live)
        for (int i = tl; i < n; i += tps) x[sig * n + i] = X[i];
}

// ------------------------------------------------------------------------------------------------------------------------------
// longer signals: one launch per level over (pair, signal).  The forward level reads s_{l-1} from the region the previous level
// wrote (or x) and writes a disjoint one; the inverse level forms w1 in scratch first because it overwrites the x it reads.
// ------------------------------------------------------------------------------------------------------------------------------
template <typename T>
__global__ __launch_bounds__(256) void k_ns_dwt_level(const T *__restrict__ src, int64_t sstride, T *__restrict__ nxw, int64_t n, int nl,
                                                      int64_t batch, WxFilt filt)
{
    const int h = nl >> 1;
    const int64_t total = (int64_t)h * batch;
    for (int64_t g = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; g < total; g += (int64_t)gridDim.x * blockDim.x) {
        const int64_t b = g / h;
        const int t = (int)(g - b * h);
        T s, d;
        ana_pair(src + b * sstride, nl - 1, t, filt, s, d);
        T *o = nxw + b * 2 * n;
        o[2 * h + t] = s;
        o[3 * h + t] = d;
    }
}

template <typename T>
__global__ __launch_bounds__(256) void k_ns_head(T *__restrict__ nxw, int64_t n, int m, int64_t batch)
{
    const int64_t total = (int64_t)m * batch;
    for (int64_t g = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; g < total; g += (int64_t)gridDim.x * blockDim.x) {
        const int64_t b = g / m;
        const int t = (int)(g - b * m);
        T *o = nxw + b * 2 * n;
        o[t] = o[2 * m + t];
        o[m + t] = (T)0;
    }
}

template <typename T>
__global__ __launch_bounds__(256) void k_ns_w1(const T *__restrict__ nxw, const T *__restrict__ xs, int64_t xstride, T *__restrict__ w1,
                                               int64_t n, int h, int64_t batch)
{
    const int64_t total = (int64_t)h * batch;
    for (int64_t g = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; g < total; g += (int64_t)gridDim.x * blockDim.x) {
        const int64_t b = g / h;
        const int t = (int)(g - b * h);
        w1[g] = (T)(nxw[b * 2 * n + 2 * h + t] + xs[b * xstride + t]);
    }
}

template <typename T>
__global__ __launch_bounds__(256) void k_ns_idwt_level(const T *__restrict__ w1, const T *__restrict__ nxw, T *__restrict__ x, int64_t n,
                                                       int h, int64_t batch, WxFilt filt)
{
    const int64_t total = (int64_t)h * batch;
    for (int64_t g = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; g < total; g += (int64_t)gridDim.x * blockDim.x) {
        const int64_t b = g / h;
        const int t = (int)(g - b * h);
        T v0, v1;
        syn_pair(w1 + b * h, nxw + b * 2 * n + 3 * h, h - 1, t, filt, v0, v1);
        x[b * n + 2 * t] = v0;
        x[b * n + 2 * t + 1] = v1;
    }
}

unsigned grid_for(int64_t total)
{
    int64_t g = (total + 255) / 256;
    if (g > 256 * 64) g = 256 * 64;
    if (g < 1) g = 1;
    return (unsigned)g;
}

int ns_tps(int64_t n) { return (int)std::min<int64_t>(256, std::max<int64_t>(1, n / 2)); }

// device pointers in, device pointers out; everything on st
template <typename T>
int ns_dwt_dev(const T *dx, T *dnxw, int64_t n, int L, int64_t batch, const WxFilt &filt, hipStream_t st)
{
    if (n <= NS_LDS_MAX) {
        const int tps = ns_tps(n), spb = 256 / tps;
        const size_t lds = sizeof(T) * (size_t)spb * (n + n / 2);
        hipLaunchKernelGGL(k_ns_dwt_lds<T>, dim3((unsigned)((batch + spb - 1) / spb)), dim3(256), lds, st, dx, dnxw, (int)n, L, batch, tps,
                           filt);
    } else {
        for (int l = 1; l <= L; ++l) {
            const int nl = (int)(n >> (l - 1));
            const T *src = l == 1 ? dx : dnxw + 2 * nl;               // s_{l-1} sits at [2 nl, 3 nl)
            hipLaunchKernelGGL(k_ns_dwt_level<T>, dim3(grid_for((int64_t)(nl / 2) * batch)), dim3(256), 0, st, src,
                               l == 1 ? n : 2 * n, dnxw, n, nl, batch, filt);
        }
        const int m = (int)(n >> L);
        hipLaunchKernelGGL(k_ns_head<T>, dim3(grid_for((int64_t)m * batch)), dim3(256), 0, st, dnxw, n, m, batch);
    }
    WX_HIP_CHECK(hipGetLastError());
    return WX_OK;
}

template <typename T>
int ns_idwt_dev(const T *dnxw, T *dx, int64_t n, int L, int64_t batch, const WxFilt &filt, hipStream_t st, WxScratch &scr)
{
    if (n <= NS_LDS_MAX) {
        const int tps = ns_tps(n), spb = 256 / tps;
        const size_t lds = sizeof(T) * (size_t)spb * (n + n / 2);
        hipLaunchKernelGGL(k_ns_idwt_lds<T>, dim3((unsigned)((batch + spb - 1) / spb)), dim3(256), lds, st, dnxw, dx, (int)n, L, batch, tps,
                           filt);
    } else {
        T *w1 = (T *)scr.alloc(sizeof(T) * (size_t)(n / 2) * batch);
        if (!w1) return WX_EHIP;
        for (int l = L; l >= 1; --l) {
            const int h = (int)(n >> l);
            const unsigned g = grid_for((int64_t)h * batch);
            hipLaunchKernelGGL(k_ns_w1<T>, dim3(g), dim3(256), 0, st, dnxw, l == L ? dnxw : (const T *)dx, l == L ? 2 * n : n, w1, n, h, batch);
            hipLaunchKernelGGL(k_ns_idwt_level<T>, dim3(g), dim3(256), 0, st, (const T *)w1, dnxw, dx, n, h, batch, filt);
        }
    }
    WX_HIP_CHECK(hipGetLastError());
    return WX_OK;
}

// ns_dwt / ns_idwt assert 1 <= L <= Lmax and ispow2(n) (transforms.jl:57-58, 129-130)
int ns_check(int64_t n, int L, int64_t batch)
{
    WX_REQUIRE(n >= 1 && batch >= 0, WX_EARG, "ns_dwt: bad dimensions");
    WX_REQUIRE(wx_isdyadic(n), WX_EASSERT, "ns_dwt: the signal length must be a power of two (transforms.jl:58)");
    WX_REQUIRE(1 <= L && L <= wx_maxtransformlevels(n), WX_EASSERT, "ns_dwt: 1 <= L <= maxtransformlevels(x) (transforms.jl:57)");
    WX_REQUIRE(n <= ((int64_t)1 << 28), WX_EUNSUPPORTED, "ns_dwt: signals longer than 2^28 samples");
    return WX_OK;
}

template <typename T>
int api_ns(const T *in, T *out, int64_t n, int L, int64_t batch, const double *qmf, int F, bool inverse, void *stream)
{
    WxFilt filt;
    int rc = wx_pack_filter(qmf, F, &filt);
    if (rc) return rc;
    if ((rc = ns_check(n, L, batch))) return rc;
    if (wx_device_count() < 1) return wx_set_error(WX_EHIP, "no HIP device visible: the MI355X kernels cannot run");
    if (batch == 0) return WX_OK;
    hipStream_t st = wx_stream(stream);
    WxScratch scr(st);
    WxIO io(st);
    const T *din = (const T *)io.in(in, sizeof(T) * (size_t)(inverse ? 2 * n : n) * batch);
    T *dout = (T *)io.out(out, sizeof(T) * (size_t)(inverse ? n : 2 * n) * batch);
    if (!din || !dout) return io.finish(io.err ? io.err : WX_EHIP);
    rc = inverse ? ns_idwt_dev<T>(din, dout, n, L, batch, filt, st, scr) : ns_dwt_dev<T>(din, dout, n, L, batch, filt, st);
    return io.finish(rc);
}

// ------------------------------------------------------------------------------------------------------------------------------
// sft / isft: pyramid over the columns, transpose, pyramid over the rows, transpose back (the inverse: rows first)
// ------------------------------------------------------------------------------------------------------------------------------
template <typename T>
__global__ __launch_bounds__(256) void k_transpose(const T *__restrict__ in, T *__restrict__ out, int64_t r, int64_t c)
{
    __shared__ T tile[32][33];
    const int64_t i0 = (int64_t)blockIdx.x * 32, j0 = (int64_t)blockIdx.y * 32;
    const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
    for (int jj = ty; jj < 32; jj += 8)
        if (i0 + tx < r && j0 + jj < c) tile[jj][tx] = in[(i0 + tx) + (j0 + jj) * r];
    __syncthreads();
    for (int ii = ty; ii < 32; ii += 8)
        if (j0 + tx < c && i0 + ii < r) out[(j0 + tx) + (i0 + ii) * c] = tile[tx][ii];
}

inline int pyr(const double *a, double *b, int64_t n, const uint8_t *tree, int64_t nt, int64_t batch, const double *qmf, int F, bool inv,
               void *s)
{ return inv ? wx_iwpt1d_f64(a, b, n, 0, tree, nt, batch, qmf, F, s) : wx_wpt1d_f64(a, b, n, 0, tree, nt, batch, qmf, F, s); }
inline int pyr(const float *a, float *b, int64_t n, const uint8_t *tree, int64_t nt, int64_t batch, const double *qmf, int F, bool inv,
               void *s)
{ return inv ? wx_iwpt1d_f32(a, b, n, 0, tree, nt, batch, qmf, F, s) : wx_wpt1d_f32(a, b, n, 0, tree, nt, batch, qmf, F, s); }

// L levels of dwt / idwt on `batch` device signals of length n: the packet transform along the :dwt tree (nodes 1, 2, 4, ... split)
template <typename T>
int pyramid_dev(const T *a, T *b, int64_t n, int L, int64_t batch, const double *qmf, int F, bool inv, void *stream)
{
    std::vector<uint8_t> tree((size_t)std::max<int64_t>(n - 1, 0), 0);
    for (int i = 0; i < L; ++i) tree[((size_t)1 << i) - 1] = 1;
    return pyr(a, b, n, L > 0 ? tree.data() : nullptr, L > 0 ? (int64_t)tree.size() : 0, batch, qmf, F, inv, stream);
}

template <typename T>
void transpose_dev(const T *in, T *out, int64_t r, int64_t c, hipStream_t st)
{
    hipLaunchKernelGGL(k_transpose<T>, dim3((unsigned)((r + 31) / 32), (unsigned)((c + 31) / 32)), dim3(256), 0, st, in, out, r, c);
}

template <typename T>
int api_sft(const T *M, T *Mw, int64_t n, int64_t m, int L, int inverse, const double *qmf, int F, void *stream)
{
    WxFilt filt;
    int rc = wx_pack_filter(qmf, F, &filt);
    if (rc) return rc;
    WX_REQUIRE(n >= 1 && m >= 1, WX_EARG, "sft: bad dimensions");
    WX_REQUIRE(1 <= L && L <= wx_maxtransformlevels(std::min(n, m)), WX_EASSERT, "sft: 1 <= L <= maxtransformlevels(M) (transforms.jl:174, 217)");
    WX_REQUIRE(wx_isdyadic(n) && wx_isdyadic(m), WX_EUNSUPPORTED, "sft: both sides must be powers of two");
    WX_REQUIRE(n < ((int64_t)1 << 21) && m < ((int64_t)1 << 21), WX_EUNSUPPORTED, "sft: a side of 2^21 or more");
    if (wx_device_count() < 1) return wx_set_error(WX_EHIP, "no HIP device visible: the MI355X kernels cannot run");
    hipStream_t st = wx_stream(stream);
    WxScratch scr(st);
    WxIO io(st);
    const size_t bytes = sizeof(T) * (size_t)n * m;
    const T *din = (const T *)io.in(M, bytes);
    T *dout = (T *)io.out(Mw, bytes);
    T *t1 = (T *)scr.alloc(bytes), *t2 = (T *)scr.alloc(bytes);
    if (!din || !dout || !t1 || !t2) return io.finish(io.err ? io.err : WX_EHIP);
    if (!inverse) {
        if ((rc = pyramid_dev<T>(din, t1, n, L, m, qmf, F, false, stream))) return io.finish(rc);      // columns
        transpose_dev<T>(t1, t2, n, m, st);
        if ((rc = pyramid_dev<T>(t2, t1, m, L, n, qmf, F, false, stream))) return io.finish(rc);       // rows
        transpose_dev<T>(t1, dout, m, n, st);
    } else {
        transpose_dev<T>(din, t1, n, m, st);
        if ((rc = pyramid_dev<T>(t1, t2, m, L, n, qmf, F, true, stream))) return io.finish(rc);        // rows
        transpose_dev<T>(t2, t1, m, n, st);
        if ((rc = pyramid_dev<T>(t1, dout, n, L, m, qmf, F, true, stream))) return io.finish(rc);      // columns
    }
    WX_HIP_CHECK(hipGetLastError());
    return io.finish(WX_OK);
}

// ------------------------------------------------------------------------------------------------------------------------------
// sparse forms.  Output column c (0-based) of the stretched matrix in closed form, K = Lmax - L, p = 2^K:
//   c < p: source column c, rows [0, p), no shift;  p <= c < 2p: empty;
//   2^(k+1) <= c < 2^(k+2), k = K .. Lmax-1: source column j = c - 2^(k+1), rows [0, 2^(k+1)) if j >= 2^k else [2^k, 2^(k+1)),
//   every row index moved by 2^(k+1).  Rows stay ascending inside a column, so the result is CSC without a sort.
// ------------------------------------------------------------------------------------------------------------------------------
struct ColMap { int64_t j; int r0, r1; int64_t shift; };

static __device__ __forceinline__ ColMap nz_colmap(int64_t c, int n, int Lns, int Lmax)
{
    ColMap cm;
    if (Lns == 0) { cm.j = c; cm.r0 = 0; cm.r1 = n; cm.shift = 0; return cm; }
    const int64_t p = (int64_t)1 << (Lmax - Lns);
    if (c < p) { cm.j = c; cm.r0 = 0; cm.r1 = (int)p; cm.shift = 0; return cm; }
    if (c < 2 * p) { cm.j = 0; cm.r0 = 0; cm.r1 = 0; cm.shift = 0; return cm; }
    const int k = 62 - __clzll((long long)c);                  // floor(log2 c) - 1
    const int64_t hk = (int64_t)1 << k;
    cm.j = c - 2 * hk;
    cm.r0 = cm.j >= hk ? 0 : (int)hk;
    cm.r1 = (int)(2 * hk);
    cm.shift = 2 * hk;
    return cm;
}

// norm of every column (Float64 partial sums combined in a fixed order), rounded to T like norm(::Vector{T})
template <typename T>
__global__ __launch_bounds__(256) void k_colnorm(const T *__restrict__ Mw, int64_t n, double *__restrict__ nrm)
{
    __shared__ double red[256];
    red[threadIdx.x] = wx_sumsq_strided(Mw + (int64_t)blockIdx.x * n, n);
    __syncthreads();
    for (int s = 128; s > 0; s >>= 1) {
        if ((int)threadIdx.x < s) red[threadIdx.x] += red[threadIdx.x + s];
        __syncthreads();
    }
    if (threadIdx.x == 0) nrm[blockIdx.x] = (double)(T)sqrt(red[0]);
}

// thr = T(eps) * max_j norm_j in the arithmetic of T (mat2sparse.jl:46-47, 96-97)
template <typename T>
__global__ __launch_bounds__(256) void k_threshold(const double *__restrict__ nrm, int64_t n, double eps, T *__restrict__ thr)
{
    __shared__ double red[256];
    double m = 0.0;
    for (int64_t i = threadIdx.x; i < n; i += 256) m = fmax(m, nrm[i]);
    red[threadIdx.x] = m;
    __syncthreads();
    for (int s = 128; s > 0; s >>= 1) {
        if ((int)threadIdx.x < s) red[threadIdx.x] = fmax(red[threadIdx.x], red[threadIdx.x + s]);
        __syncthreads();
    }
    if (threadIdx.x == 0) thr[0] = (T)((T)eps * (T)red[0]);
}

template <typename T> static __device__ __forceinline__ bool nz_keep(T v, T thr)
{
    const T a = v < (T)0 ? -v : v;
    return a > thr && v != (T)0;
}

// one wavefront per output column
template <typename T>
__global__ __launch_bounds__(256) void k_nz_count(const T *__restrict__ Mw, int n, int Lns, int Lmax, int64_t N, const T *__restrict__ thrp,
                                                  int64_t *__restrict__ cnt)
{
    const int64_t c = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    if (c >= N) return;
    const ColMap cm = nz_colmap(c, n, Lns, Lmax);
    const T thr = thrp[0];
    const T *col = Mw + cm.j * n;
    int k = 0;
    for (int r = cm.r0 + lane; r < cm.r1; r += 64) k += nz_keep(col[r], thr) ? 1 : 0;
    for (int off = 32; off > 0; off >>= 1) k += __shfl_down(k, off, 64);
    if (lane == 0) cnt[c] = k;
}

// colptr[i] = 1 + sum_{c < i} cnt[c], i = 0 .. N (one workgroup; each thread owns a contiguous run)
__global__ __launch_bounds__(1024) void k_scan_colptr(const int64_t *__restrict__ cnt, int64_t N, int64_t *__restrict__ colptr)
{
    __shared__ int64_t part[1024];
    const int64_t chunk = (N + 1023) / 1024;
    const int64_t lo0 = (int64_t)threadIdx.x * chunk, lo = lo0 < N ? lo0 : N, hi = lo + chunk < N ? lo + chunk : N;
    int64_t s = 0;
    for (int64_t i = lo; i < hi; ++i) s += cnt[i];
    part[threadIdx.x] = s;
    __syncthreads();
    if (threadIdx.x == 0) {
        int64_t acc = 1;
        for (int i = 0; i < 1024; ++i) { const int64_t v = part[i]; part[i] = acc; acc += v; }
        colptr[N] = acc;
    }
    __syncthreads();
    int64_t acc = part[threadIdx.x];
    for (int64_t i = lo; i < hi; ++i) { colptr[i] = acc; acc += cnt[i]; }
}

// one wavefront per output column: ballot + prefix count give every kept row its place, ascending
template <typename T>
__global__ __launch_bounds__(256) void k_nz_fill(const T *__restrict__ Mw, int n, int Lns, int Lmax, int64_t N, T thr,
                                                 const int64_t *__restrict__ colptr, int64_t nnz, int64_t *__restrict__ rowval, T *__restrict__ nzval)
{
    const int64_t c = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    if (c >= N) return;
    const ColMap cm = nz_colmap(c, n, Lns, Lmax);
    const T *col = Mw + cm.j * n;
    int64_t base = colptr[c] - 1;
    const int64_t end = colptr[c + 1] - 1 < nnz ? colptr[c + 1] - 1 : nnz;
    for (int r0 = cm.r0; r0 < cm.r1; r0 += 64) {
        const int r = r0 + lane;
        const T v = r < cm.r1 ? col[r] : (T)0;
        const bool keep = r < cm.r1 && nz_keep(v, thr);
        const unsigned long long mask = __ballot(keep);
        const int64_t pos = base + __popcll(mask & ((1ull << lane) - 1ull));
        if (keep && pos >= 0 && pos < end) {              // a colptr that does not belong to (Mw, thr) cannot write outside rowval / nzval
            rowval[pos] = (int64_t)r + cm.shift + 1;
            nzval[pos] = v;
        }
        base += __popcll(mask);
    }
}

int sparse_check(int64_t n, int Lns)
{
    WX_REQUIRE(n >= 1 && n <= ((int64_t)1 << 20), WX_EARG, "sparse form: bad matrix size");
    WX_REQUIRE(Lns >= 0, WX_EASSERT, "stretchmatrix: 1 <= L <= maxtransformlevels(n) (utils.jl:101)");
    if (Lns > 0) WX_REQUIRE(wx_isdyadic(n) && Lns <= wx_maxtransformlevels(n), WX_EASSERT, "stretchmatrix: 1 <= L <= maxtransformlevels(n) (utils.jl:101)");
    if (wx_device_count() < 1) return wx_set_error(WX_EHIP, "no HIP device visible: the MI355X kernels cannot run");
    return WX_OK;
}

template <typename T>
int api_sparse_count(const T *Mw, int64_t n, int Lns, double eps, int64_t *colptr, T *thr_out, void *stream)
{
    int rc = sparse_check(n, Lns);
    if (rc) return rc;
    const int64_t N = Lns ? 2 * n : n;
    hipStream_t st = wx_stream(stream);
    WxScratch scr(st);
    WxIO io(st);
    const T *dM = (const T *)io.in(Mw, sizeof(T) * (size_t)n * n);
    int64_t *dcp = (int64_t *)io.out(colptr, sizeof(int64_t) * (size_t)(N + 1));
    T *dthr = (T *)io.out(thr_out, sizeof(T));
    double *nrm = (double *)scr.alloc(sizeof(double) * (size_t)n);
    int64_t *cnt = (int64_t *)scr.alloc(sizeof(int64_t) * (size_t)N);
    if (!dM || !dcp || !dthr || !nrm || !cnt) return io.finish(io.err ? io.err : WX_EHIP);
    hipLaunchKernelGGL(k_colnorm<T>, dim3((unsigned)n), dim3(256), 0, st, dM, n, nrm);
    hipLaunchKernelGGL(k_threshold<T>, dim3(1), dim3(256), 0, st, (const double *)nrm, n, eps, dthr);
    hipLaunchKernelGGL(k_nz_count<T>, dim3((unsigned)((N + 3) / 4)), dim3(256), 0, st, dM, (int)n, Lns, wx_maxtransformlevels(n), N,
                       (const T *)dthr, cnt);
    hipLaunchKernelGGL(k_scan_colptr, dim3(1), dim3(1024), 0, st, (const int64_t *)cnt, N, dcp);
    WX_HIP_CHECK(hipGetLastError());
    return io.finish(WX_OK);
}

template <typename T>
int api_sparse_fill(const T *Mw, int64_t n, int Lns, double thr, const int64_t *colptr, int64_t *rowval, T *nzval, void *stream)
{
    int rc = sparse_check(n, Lns);
    if (rc) return rc;
    const int64_t N = Lns ? 2 * n : n;
    hipStream_t st = wx_stream(stream);
    WxIO io(st);
    // the number of entries is colptr[N] - 1: read it where colptr lives
    int64_t last = 0;
    WX_REQUIRE(colptr != nullptr, WX_EARG, "sparse form: colptr is NULL");
    if (wx_is_device_ptr(colptr)) {
        WX_HIP_CHECK(hipMemcpyAsync(&last, colptr + N, sizeof last, hipMemcpyDeviceToHost, st));
        WX_HIP_CHECK(hipStreamSynchronize(st));
    } else last = colptr[N];
    const int64_t nnz = last - 1;
    WX_REQUIRE(nnz >= 0 && nnz <= n * n, WX_EARG, "sparse form: colptr does not end in 1 + the number of entries");
    const T *dM = (const T *)io.in(Mw, sizeof(T) * (size_t)n * n);
    const int64_t *dcp = (const int64_t *)io.in(colptr, sizeof(int64_t) * (size_t)(N + 1));
    int64_t *drv = (int64_t *)io.out(rowval, sizeof(int64_t) * (size_t)nnz);
    T *dnz = (T *)io.out(nzval, sizeof(T) * (size_t)nnz);
    if (!dM || !dcp || (nnz && (!drv || !dnz))) return io.finish(io.err ? io.err : WX_EHIP);
    if (nnz)
        hipLaunchKernelGGL(k_nz_fill<T>, dim3((unsigned)((N + 3) / 4)), dim3(256), 0, st, dM, (int)n, Lns, wx_maxtransformlevels(n), N, (T)thr,
                           dcp, nnz, drv, dnz);
    WX_HIP_CHECK(hipGetLastError());
    return io.finish(WX_OK);
}

// ------------------------------------------------------------------------------------------------------------------------------
// the product
// ------------------------------------------------------------------------------------------------------------------------------
constexpr uint32_t PLAN_MAGIC = 0x57584d50u;          // "WXMP"

struct Plan {
    uint32_t magic;
    int elem;                                          // sizeof(T)
    int dev;
    int64_t N, nnz, nv, nslices, nsplit, npart, padded, cap, layout_bytes;
    int64_t *slice_ptr;                                // nslices + 1: first entry of every slice
    int32_t *vlen;                                     // nv: entries of every virtual row
    int64_t *vdst;                                     // nv: row of Y, or -(index into the side buffer) - 1 for a piece of a cut row
    void *vals;                                        // padded entries, column-major inside a slice
    int32_t *cols;
    int64_t *split_row, *split_first;                  // nsplit: row of Y, first piece in the side buffer
    int32_t *split_nseg;
};

template <typename T>
__global__ __launch_bounds__(256) void k_spmm(const int64_t *__restrict__ slice_ptr, const int32_t *__restrict__ vlen,
                                              const int64_t *__restrict__ vdst, const T *__restrict__ vals, const int32_t *__restrict__ cols,
                                              const T *__restrict__ X, T *__restrict__ Y, T *__restrict__ P, int64_t N, int64_t npart, int64_t B,
                                              int64_t nv, int64_t nslices)
{
    const int64_t slice = blockIdx.x % nslices, tile = blockIdx.x / nslices;
    const int lane = threadIdx.x & 63;
    const int64_t s0 = (tile * 4 + (threadIdx.x >> 6)) * SPMM_TS;
    if (s0 >= B) return;
    const int ns = B - s0 < SPMM_TS ? (int)(B - s0) : SPMM_TS;
    const int64_t v = slice * 64 + lane;
    const int len = v < nv ? vlen[v] : 0;
    const int64_t base = slice_ptr[slice];
    const int width = (int)((slice_ptr[slice + 1] - base) >> 6);
    const T *xs = X + s0 * N;
    T acc[SPMM_TS];
#pragma unroll
    for (int u = 0; u < SPMM_TS; ++u) acc[u] = (T)0;
    if (ns == SPMM_TS) {
        for (int k = 0; k < width; ++k) {
            if (k < len) {
                const T a = vals[base + (int64_t)k * 64 + lane];
                const T *xp = xs + cols[base + (int64_t)k * 64 + lane];
#pragma unroll
                for (int u = 0; u < SPMM_TS; ++u) acc[u] = fma(a, xp[u * N], acc[u]);
            }
        }
    } else {
        for (int k = 0; k < width; ++k) {
            if (k < len) {
                const T a = vals[base + (int64_t)k * 64 + lane];
                const T *xp = xs + cols[base + (int64_t)k * 64 + lane];
#pragma unroll
                for (int u = 0; u < SPMM_TS; ++u)
                    if (u < ns) acc[u] = fma(a, xp[u * N], acc[u]);
            }
        }
    }
    if (v >= nv) return;
    const int64_t dst = vdst[v];
    T *o = dst >= 0 ? Y + dst + s0 * N : P + (-dst - 1) + s0 * npart;
    const int64_t os = dst >= 0 ? N : npart;
#pragma unroll
    for (int u = 0; u < SPMM_TS; ++u)
        if (u < ns) o[u * os] = acc[u];
}

// rows that were cut: their pieces added in ascending order by one thread
template <typename T>
__global__ __launch_bounds__(256) void k_spmm_combine(const int64_t *__restrict__ split_row, const int64_t *__restrict__ split_first,
                                                      const int32_t *__restrict__ split_nseg, const T *__restrict__ P, T *__restrict__ Y,
                                                      int64_t N, int64_t npart, int64_t nsplit, int64_t B)
{
    const int64_t total = nsplit * B;
    for (int64_t g = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; g < total; g += (int64_t)gridDim.x * blockDim.x) {
        const int64_t s = g / nsplit, i = g - s * nsplit;
        const T *p = P + split_first[i] + s * npart;
        T acc = p[0];
        for (int q = 1; q < split_nseg[i]; ++q) acc += p[q];
        Y[split_row[i] + s * N] = acc;
    }
}

template <typename T>
int spmm_dev(const Plan *pl, const T *X, T *Y, int64_t B, hipStream_t st, WxScratch &scr)
{
    const int64_t tiles = (B + SPMM_TILE - 1) / SPMM_TILE;
    WX_REQUIRE(tiles * pl->nslices < ((int64_t)1 << 31), WX_EUNSUPPORTED, "wavemult: more than 2^31 (slice, tile) workgroups");
    T *P = nullptr;
    if (pl->nsplit) {
        P = (T *)scr.alloc(sizeof(T) * (size_t)pl->npart * B);
        if (!P) return WX_EHIP;
    }
    hipLaunchKernelGGL(k_spmm<T>, dim3((unsigned)(tiles * pl->nslices)), dim3(256), 0, st, (const int64_t *)pl->slice_ptr,
                       (const int32_t *)pl->vlen, (const int64_t *)pl->vdst, (const T *)pl->vals, (const int32_t *)pl->cols, X, Y, P, pl->N,
                       pl->npart, B, pl->nv, pl->nslices);
    if (pl->nsplit)
        hipLaunchKernelGGL(k_spmm_combine<T>, dim3(grid_for(pl->nsplit * B)), dim3(256), 0, st, (const int64_t *)pl->split_row,
                           (const int64_t *)pl->split_first, (const int32_t *)pl->split_nseg, (const T *)P, Y, pl->N, pl->npart, pl->nsplit, B);
    WX_HIP_CHECK(hipGetLastError());
    return WX_OK;
}

void plan_free(Plan *pl)
{
    void *ptrs[] = {pl->slice_ptr, pl->vlen, pl->vdst, pl->vals, pl->cols, pl->split_row, pl->split_first, pl->split_nseg};
    for (void *p : ptrs)
        if (p && hipFree(p) != hipSuccess) (void)hipGetLastError();
    pl->magic = 0;
    delete pl;
}

template <typename U>
int plan_upload(U **dst, const std::vector<U> &src, hipStream_t st)
{
    *dst = nullptr;
    WX_HIP_CHECK(hipMalloc((void **)dst, std::max<size_t>(16, sizeof(U) * src.size())));
    if (!src.empty()) WX_HIP_CHECK(hipMemcpyAsync(*dst, src.data(), sizeof(U) * src.size(), hipMemcpyHostToDevice, st));
    return WX_OK;
}

template <typename U>
int fetch_host(std::vector<U> &dst, const U *src, size_t count, hipStream_t st)
{
    dst.resize(count);
    if (!count) return WX_OK;
    WX_REQUIRE(src != nullptr, WX_EARG, "wavemult plan: NULL array");
    if (wx_is_device_ptr(src)) {
        WX_HIP_CHECK(hipMemcpyAsync(dst.data(), src, sizeof(U) * count, hipMemcpyDeviceToHost, st));
        WX_HIP_CHECK(hipStreamSynchronize(st));
    } else std::copy(src, src + count, dst.begin());
    return WX_OK;
}

template <typename T>
int api_plan_create(const int64_t *colptr, const int64_t *rowval, const T *nzval, int64_t N, void **plan, void *stream)
{
    WX_REQUIRE(plan != nullptr, WX_EARG, "wavemult plan: plan is NULL");
    *plan = nullptr;
    WX_REQUIRE(N >= 1 && N < ((int64_t)1 << 31), WX_EARG, "wavemult plan: bad matrix size");
    if (wx_device_count() < 1) return wx_set_error(WX_EHIP, "no HIP device visible: the MI355X kernels cannot run");
    hipStream_t st = wx_stream(stream);
    std::vector<int64_t> cp, rv;
    std::vector<T> nz;
    int rc = fetch_host(cp, colptr, (size_t)N + 1, st);
    if (rc) return rc;
    WX_REQUIRE(cp[0] == 1, WX_EARG, "wavemult plan: colptr must start at 1 (SparseMatrixCSC)");
    for (int64_t j = 0; j < N; ++j) WX_REQUIRE(cp[j + 1] >= cp[j], WX_EARG, "wavemult plan: colptr must not decrease");
    const int64_t nnz = cp[N] - 1;
    if ((rc = fetch_host(rv, rowval, (size_t)nnz, st)) || (rc = fetch_host(nz, nzval, (size_t)nnz, st))) return rc;
    // rows: counts, then a counting sort that walks the columns in order -> every row's entries in ascending column order
    std::vector<int64_t> rowptr((size_t)N + 1, 0);
    for (int64_t e = 0; e < nnz; ++e) {
        WX_REQUIRE(rv[e] >= 1 && rv[e] <= N, WX_EARG, "wavemult plan: row index outside 1 .. N");
        ++rowptr[rv[e]];
    }
    for (int64_t r = 0; r < N; ++r) rowptr[r + 1] += rowptr[r];
    std::vector<int64_t> fillp(rowptr.begin(), rowptr.end() - 1);
    std::vector<int32_t> ccol((size_t)nnz);
    std::vector<T> cval((size_t)nnz);
    for (int64_t j = 0; j < N; ++j)
        for (int64_t e = cp[j] - 1; e < cp[j + 1] - 1; ++e) {
            const int64_t p = fillp[rv[e] - 1]++;
            ccol[p] = (int32_t)j;
            cval[p] = nz[e];
        }
    // virtual rows of at most cap entries
    const int64_t cap = std::max<int64_t>(64, 4 * ((nnz + N - 1) / N));
    std::vector<int32_t> vlen, split_nseg;
    std::vector<int64_t> vdst, vsrc, split_row, split_first;
    int64_t npart = 0;
    for (int64_t r = 0; r < N; ++r) {
        const int64_t cnt = rowptr[r + 1] - rowptr[r];
        const int64_t nseg = std::max<int64_t>(1, (cnt + cap - 1) / cap);
        if (nseg > 1) { split_row.push_back(r); split_first.push_back(npart); split_nseg.push_back((int32_t)nseg); }
        for (int64_t g = 0; g < nseg; ++g) {
            vlen.push_back((int32_t)std::min<int64_t>(cap, cnt - g * cap));
            vsrc.push_back(rowptr[r] + g * cap);
            vdst.push_back(nseg > 1 ? -(npart++) - 1 : r);
        }
    }
    const int64_t nv = (int64_t)vlen.size(), nslices = (nv + 63) / 64;
    std::vector<int64_t> slice_ptr((size_t)nslices + 1, 0);
    for (int64_t s = 0; s < nslices; ++s) {
        int32_t w = 0;
        for (int64_t v = s * 64; v < std::min(nv, s * 64 + 64); ++v) w = std::max(w, vlen[v]);
        slice_ptr[s + 1] = slice_ptr[s] + (int64_t)w * 64;
    }
    const int64_t padded = slice_ptr[nslices];
    std::vector<T> vals((size_t)padded, (T)0);
    std::vector<int32_t> cols((size_t)padded, 0);
    for (int64_t v = 0; v < nv; ++v)
        for (int32_t k = 0; k < vlen[v]; ++k) {
            const int64_t p = slice_ptr[v >> 6] + (int64_t)k * 64 + (v & 63);
            vals[p] = cval[vsrc[v] + k];
            cols[p] = ccol[vsrc[v] + k];
        }
    Plan *pl = new (std::nothrow) Plan();
    WX_REQUIRE(pl != nullptr, WX_EHIP, "wavemult plan: out of host memory");
    pl->magic = PLAN_MAGIC; pl->elem = (int)sizeof(T);
    pl->N = N; pl->nnz = nnz; pl->nv = nv; pl->nslices = nslices; pl->nsplit = (int64_t)split_row.size(); pl->npart = npart;
    pl->padded = padded; pl->cap = cap;
    pl->layout_bytes = padded * (int64_t)(sizeof(T) + sizeof(int32_t)) + nv * 12 + (nslices + 1) * 8;
    (void)hipGetDevice(&pl->dev);
    T *dvals = nullptr;
    if ((rc = plan_upload(&pl->slice_ptr, slice_ptr, st)) || (rc = plan_upload(&pl->vlen, vlen, st)) || (rc = plan_upload(&pl->vdst, vdst, st)) ||
        (rc = plan_upload(&dvals, vals, st)) || (rc = plan_upload(&pl->cols, cols, st)) || (rc = plan_upload(&pl->split_row, split_row, st)) ||
        (rc = plan_upload(&pl->split_first, split_first, st)) || (rc = plan_upload(&pl->split_nseg, split_nseg, st))) {
        pl->vals = dvals;
        plan_free(pl);
        return rc;
    }
    pl->vals = dvals;
    const hipError_t e = hipStreamSynchronize(st);      // the host vectors above go away with this frame
    if (e != hipSuccess) { plan_free(pl); return wx_set_hip_error(e, "hipStreamSynchronize(plan)", __FILE__, __LINE__); }
    *plan = pl;
    return WX_OK;
}

template <typename T>
int api_apply(const void *plan, int nonstd, const T *x, T *y, int64_t n, int L, int64_t batch, const double *qmf, int F, void *stream)
{
    const Plan *pl = (const Plan *)plan;
    WX_REQUIRE(pl != nullptr && pl->magic == PLAN_MAGIC, WX_EARG, "wavemult: not a plan");
    WX_REQUIRE(pl->elem == (int)sizeof(T), WX_EARG, "wavemult: the plan was made for the other element type");
    WxFilt filt;
    int rc = wx_pack_filter(qmf, F, &filt);
    if (rc) return rc;
    WX_REQUIRE(n >= 1 && batch >= 0, WX_EARG, "wavemult: bad dimensions");
    WX_REQUIRE(wx_isdyadic(n), WX_EASSERT, "wavemult: the signal length must be a power of two");
    // ns_dwt asserts 1 <= L (transforms.jl:57); dwt of the standard form takes L = 0 as well
    WX_REQUIRE((nonstd ? 1 : 0) <= L && L <= wx_maxtransformlevels(n), WX_EASSERT, "wavemult: L outside the levels of x");
    WX_REQUIRE(pl->N == (nonstd ? 2 * n : n), WX_EASSERT, "wavemult: the sparse matrix must be n x n (standard) or 2n x 2n (non-standard)");
    WX_REQUIRE(n <= ((int64_t)1 << 28), WX_EUNSUPPORTED, "wavemult: signals longer than 2^28 samples");
    if (wx_device_count() < 1) return wx_set_error(WX_EHIP, "no HIP device visible: the MI355X kernels cannot run");
    if (batch == 0) return WX_OK;
    hipStream_t st = wx_stream(stream);
    WxScratch scr(st);
    WxIO io(st);
    const T *dx = (const T *)io.in(x, sizeof(T) * (size_t)n * batch);
    T *dy = (T *)io.out(y, sizeof(T) * (size_t)n * batch);
    const size_t wb = sizeof(T) * (size_t)pl->N * batch;
    T *xw = (T *)scr.alloc(wb), *yw = (T *)scr.alloc(wb);
    if (!dx || !dy || !xw || !yw) return io.finish(io.err ? io.err : WX_EHIP);
    if (nonstd) {
        if ((rc = ns_dwt_dev<T>(dx, xw, n, L, batch, filt, st))) return io.finish(rc);
        if ((rc = spmm_dev<T>(pl, xw, yw, batch, st, scr))) return io.finish(rc);
        rc = ns_idwt_dev<T>(yw, dy, n, L, batch, filt, st, scr);
    } else {
        if ((rc = pyramid_dev<T>(dx, xw, n, L, batch, qmf, F, false, stream))) return io.finish(rc);
        if ((rc = spmm_dev<T>(pl, xw, yw, batch, st, scr))) return io.finish(rc);
        rc = pyramid_dev<T>(yw, dy, n, L, batch, qmf, F, true, stream);
    }
    return io.finish(rc);
}

// Y (N, batch) = A X (N, batch): the product alone
template <typename T>
int api_product(const void *plan, const T *X, T *Y, int64_t batch, void *stream)
{
    const Plan *pl = (const Plan *)plan;
    WX_REQUIRE(pl != nullptr && pl->magic == PLAN_MAGIC, WX_EARG, "wavemult: not a plan");
    WX_REQUIRE(pl->elem == (int)sizeof(T), WX_EARG, "wavemult: the plan was made for the other element type");
    WX_REQUIRE(batch >= 0, WX_EARG, "wavemult: bad dimensions");
    if (wx_device_count() < 1) return wx_set_error(WX_EHIP, "no HIP device visible: the MI355X kernels cannot run");
    if (batch == 0) return WX_OK;
    hipStream_t st = wx_stream(stream);
    WxScratch scr(st);
    WxIO io(st);
    const T *dX = (const T *)io.in(X, sizeof(T) * (size_t)pl->N * batch);
    T *dY = (T *)io.out(Y, sizeof(T) * (size_t)pl->N * batch);
    if (!dX || !dY) return io.finish(io.err ? io.err : WX_EHIP);
    WX_REQUIRE(dX != dY, WX_EARG, "wavemult: the product cannot run in place");
    return io.finish(spmm_dev<T>(pl, dX, dY, batch, st, scr));
}

}  // namespace

extern "C" {
int wx_ns_dwt1d_f64(const double *x, double *nxw, int64_t n, int L, int64_t batch, const double *qmf, int F, void *stream)
{ return api_ns<double>(x, nxw, n, L, batch, qmf, F, false, stream); }
int wx_ns_dwt1d_f32(const float *x, float *nxw, int64_t n, int L, int64_t batch, const double *qmf, int F, void *stream)
{ return api_ns<float>(x, nxw, n, L, batch, qmf, F, false, stream); }
int wx_ns_idwt1d_f64(const double *nxw, double *x, int64_t n, int L, int64_t batch, const double *qmf, int F, void *stream)
{ return api_ns<double>(nxw, x, n, L, batch, qmf, F, true, stream); }
int wx_ns_idwt1d_f32(const float *nxw, float *x, int64_t n, int L, int64_t batch, const double *qmf, int F, void *stream)
{ return api_ns<float>(nxw, x, n, L, batch, qmf, F, true, stream); }

int wx_sft_f64(const double *M, double *Mw, int64_t n, int64_t m, int L, int inverse, const double *qmf, int F, void *stream)
{ return api_sft<double>(M, Mw, n, m, L, inverse, qmf, F, stream); }
int wx_sft_f32(const float *M, float *Mw, int64_t n, int64_t m, int L, int inverse, const double *qmf, int F, void *stream)
{ return api_sft<float>(M, Mw, n, m, L, inverse, qmf, F, stream); }

int wx_sparseform_count_f64(const double *Mw, int64_t n, int L_nonstd, double eps, int64_t *colptr, double *thr_out, void *stream)
{ return api_sparse_count<double>(Mw, n, L_nonstd, eps, colptr, thr_out, stream); }
int wx_sparseform_count_f32(const float *Mw, int64_t n, int L_nonstd, double eps, int64_t *colptr, float *thr_out, void *stream)
{ return api_sparse_count<float>(Mw, n, L_nonstd, eps, colptr, thr_out, stream); }
int wx_sparseform_fill_f64(const double *Mw, int64_t n, int L_nonstd, double thr, const int64_t *colptr, int64_t *rowval, double *nzval,
                           void *stream)
{ return api_sparse_fill<double>(Mw, n, L_nonstd, thr, colptr, rowval, nzval, stream); }
int wx_sparseform_fill_f32(const float *Mw, int64_t n, int L_nonstd, double thr, const int64_t *colptr, int64_t *rowval, float *nzval,
                           void *stream)
{ return api_sparse_fill<float>(Mw, n, L_nonstd, thr, colptr, rowval, nzval, stream); }

int wx_wavemult_plan_create_f64(const int64_t *colptr, const int64_t *rowval, const double *nzval, int64_t N, void **plan, void *stream)
{ return api_plan_create<double>(colptr, rowval, nzval, N, plan, stream); }
int wx_wavemult_plan_create_f32(const int64_t *colptr, const int64_t *rowval, const float *nzval, int64_t N, void **plan, void *stream)
{ return api_plan_create<float>(colptr, rowval, nzval, N, plan, stream); }
int wx_wavemult_apply_f64(const void *plan, int nonstd, const double *x, double *y, int64_t n, int L, int64_t batch, const double *qmf,
                          int F, void *stream)
{ return api_apply<double>(plan, nonstd, x, y, n, L, batch, qmf, F, stream); }
int wx_wavemult_apply_f32(const void *plan, int nonstd, const float *x, float *y, int64_t n, int L, int64_t batch, const double *qmf,
                          int F, void *stream)
{ return api_apply<float>(plan, nonstd, x, y, n, L, batch, qmf, F, stream); }

int wx_wavemult_product_f64(const void *plan, const double *X, double *Y, int64_t batch, void *stream)
{ return api_product<double>(plan, X, Y, batch, stream); }
int wx_wavemult_product_f32(const void *plan, const float *X, float *Y, int64_t batch, void *stream)
{ return api_product<float>(plan, X, Y, batch, stream); }

int wx_wavemult_plan_info(const void *plan, int64_t *info)
{
    const Plan *pl = (const Plan *)plan;
    WX_REQUIRE(pl != nullptr && pl->magic == PLAN_MAGIC && info != nullptr, WX_EARG, "wavemult: not a plan");
    const int64_t v[8] = {pl->N, pl->nnz, pl->padded, pl->nslices, pl->nsplit, pl->cap, pl->layout_bytes, SPMM_TILE};
    std::copy(v, v + 8, info);
    return WX_OK;
}

int wx_wavemult_plan_destroy(void *plan)
{
    if (!plan) return WX_OK;
    Plan *pl = (Plan *)plan;
    WX_REQUIRE(pl->magic == PLAN_MAGIC, WX_EARG, "wavemult: not a plan");
    // a product that still reads the plan may be in flight on some stream: wait for the device before the memory goes away
    if (hipDeviceSynchronize() != hipSuccess) (void)hipGetLastError();
    plan_free(pl);
    return WX_OK;
}
}
