// wx_shrink_trees.hip -- surethreshold / relerrorthreshold(xw, true, tree[, elbows]) with ONE tree per signal: the threshold of signal b is
// selected over the leaf columns of ITS tree in its redundant packet table (swpdall, acwpdall: heap ordered, node i in column i - 1), what
// the reference does for a single BitVector with coef[:, getleaf(tree)] (Denoising.jl:150-157, 293-300).  The (ntree, batch) convention is
// that of getbasiscoefall (Utils.jl:199-225), as in wx_denoise_red_trees.hip, whose thresholds these are when estnoise is one of the two
// selections (test/denoising.jl:59-83).
//
// The signals differ in the columns they read and in how many coefficients they rank, cnt_b = n leaves_b; the arithmetic of the selection
// is that of wx_shrink.hip (wx_shrink_dev.h), which depends on the sorted magnitudes and on cnt_b alone.  So every signal is sorted in a
// window padded to ITS OWN npad_b = the power of two >= max(cnt_b, 2), and the result is bit for bit what wx_surethreshold_* /
// wx_relerrorthreshold_* return for that signal alone with the column mask of its tree.  Launches, from the packed bits of the driver
// (wx_trees_host.h):
//   k_sht_leaves    a wavefront per signal: its leaf columns in ascending order (a leaf is a bare node that is the root or has a decomposed
//                   parent, as in k_drt_table) and cnt_b.  Only nodes of the levels the table holds are looked at, and at most 2^dmax of
//                   them are kept: no later kernel reads a column >= ncols or more than n 2^dmax values, whatever the words hold.
//   k_sht_classes   one workgroup: the signals grouped by log2 npad_b (1 .. 27) into one index list, class after class, and the 32 class
//                   sizes -- the only thing that comes back to the host (128 bytes, one wait).  No atomics: every thread owns a
//                   contiguous range of signals, counts it, and the counts are scanned.
//   per class       window = (2 npad + 8) sizeof(T) bytes: the sorted magnitudes, then the curve / the running sums.
//     <= 144 KiB    (npad <= 8192 Float64, 16384 Float32) one launch of k_sht_select, a workgroup per signal of the class, window in LDS
//                   of the class's own size: stage from the signal's leaf columns, sh_bitonic, the selection.
//     larger        windows in global scratch, `per` signals of the class at a time: k_sht_stage_g, the chip-wide bitonic launches of
//                   wx_shrink.hip over (pairs, signals of the chunk), then k_sht_select<SORTED>.  `per` keeps a chunk's windows within
//                   SHT_CHUNK bytes (half the 256 MiB Infinity Cache: a chunk is read and written by every one of the 16 .. 90 passes, and
//                   the caller's table, read once, should not have to evict it), one window where a window is larger, never more than
//                   the 1 GiB of wx_shrink.hip unless one window is.
// At most 27 classes exist and at most 14 of them are outside LDS (2^14 .. 2^27 Float64), so the number of launches does not depend on
// the batch.  Byte-identical columns go to wx_surethreshold_* / wx_relerrorthreshold_* with the leaf mask of that tree (the driver's
// single()).  Nothing is estimated on the host and the tree matrix never travels to it.
#include "wx_shrink_dev.h"
#include "wx_trees_host.h"

namespace {

constexpr int SHT_CLASSES = 32;                                        // class c: npad = 1 << c, c = 1 .. 27
constexpr int64_t SHT_MAX = (int64_t)1 << 27;                          // coefficients per signal, the limit of wx_shrink.hip
constexpr size_t SHT_LDS = 144 * 1024;                                 // the largest window in LDS, as wx_shrink.hip
constexpr size_t SHT_CHUNK = (size_t)128 << 20;                        // the windows of one chunk of the scratch tier

// leaf[b maxleaves + j] = the column of the j-th leaf of tree b, cnt[b] = n * its leaves.  nodes: the nodes of the levels the table holds.
__global__ __launch_bounds__(256) void k_sht_leaves(const uint32_t *__restrict__ trees, int nw, int ntree, int nodes, int n, int maxleaves,
                                                    int64_t batch, int *__restrict__ cnt, int *__restrict__ leaf)
{
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    for (int64_t b = (int64_t)blockIdx.x * 4 + wave; b < batch; b += (int64_t)gridDim.x * 4) {
        const uint32_t *tg = trees + b * (int64_t)nw;
        int *lf = leaf + b * (int64_t)maxleaves;
        int found = 0;
        for (int base = 1; base <= nodes; base += 64) {
            const int node = base + lane;                              // nodes < 2^30: no overflow
            // a valid tree: a node is decomposed only under decomposed ancestors, so a leaf is a bare node that is the root or has a decomposed parent
            const bool is = node <= nodes && !(node <= ntree && wt_set(tg, node)) &&
                            (node == 1 || ((node >> 1) <= ntree && wt_set(tg, node >> 1)));
            const unsigned long long m = __ballot(is);
            const int pos = found + __popcll(m & (((unsigned long long)1 << lane) - 1));
            if (is && pos < maxleaves) lf[pos] = node - 1;
            found += __popcll(m);
        }
        if (lane == 0) cnt[b] = n * min(found, maxleaves);
    }
}

__device__ __forceinline__ int sht_class(int cnt)                       // log2 of the power of two >= max(cnt, 2); 0: nothing selected
{
    if (cnt < 1) return 0;
    int c = 1;
    while (((int64_t)1 << c) < cnt) ++c;
    return c;
}

// list: the signals of class 1, then of class 2, ... in ascending order within a class; hist[c] = the size of class c (hist[0]: signals
// without a leaf, which no checked tree has; they are in no list)
__global__ __launch_bounds__(256) void k_sht_classes(const int *__restrict__ cnt, int batch, int *__restrict__ hist, int *__restrict__ list)
{
    __shared__ int part[SHT_CLASSES][256];
    __shared__ int off[SHT_CLASSES];
    const int t = threadIdx.x;
    const int C = (batch + 255) / 256, b0 = min(batch, t * C), b1 = min(batch, b0 + C);
    for (int c = 0; c < SHT_CLASSES; ++c) part[c][t] = 0;
    for (int b = b0; b < b1; ++b) ++part[sht_class(cnt[b])][t];
    __syncthreads();
    if (t < SHT_CLASSES) {                                             // class t: the exclusive scan over the threads' counts
        int run = 0;
        for (int i = 0; i < 256; ++i) { const int p = part[t][i]; part[t][i] = run; run += p; }
        off[t] = run;
        hist[t] = run;
    }
    __syncthreads();
    if (t == 0) {
        int run = 0;
        for (int c = 1; c < SHT_CLASSES; ++c) { const int p = off[c]; off[c] = run; run += p; }
    }
    __syncthreads();
    for (int b = b0; b < b1; ++b) {
        const int c = sht_class(cnt[b]);
        if (c > 0) list[off[c] + part[c][t]++] = b;
    }
}

// |xw[row, leaf column, signal]| of the signals list[blockIdx.y] into their windows of the chunk, +Inf up to npad
template <typename T>
__global__ __launch_bounds__(SH_NT) void k_sht_stage_g(const T *__restrict__ X, int64_t sig_stride, int n, const int *__restrict__ list,
                                                       const int *__restrict__ cnts, const int *__restrict__ leaf, int maxleaves, int npad,
                                                       T *__restrict__ gs)
{
    const int sig = list[blockIdx.y];
    const int cnt = min(cnts[sig], npad);
    const T *x = X + (int64_t)sig * sig_stride;
    const int *cols = leaf + (int64_t)sig * maxleaves;
    T *v = gs + (int64_t)blockIdx.y * (2 * (int64_t)npad + 8);
    for (int64_t e = (int64_t)blockIdx.x * SH_NT + threadIdx.x; e < npad; e += (int64_t)gridDim.x * SH_NT) {
        T val = sh_inf<T>();
        if (e < cnt) {
            const int c = (int)(e / n), row = (int)(e - (int64_t)c * n);
            val = (T)fabs((double)x[(int64_t)cols[c] * n + row]);
        }
        v[e] = val;
    }
}

// the selection of signal list[blockIdx.x] (KIND 0: SureShrink, 1: RelErrorShrink) in its window: LDS of (2 npad + 8) values, staged and
// sorted here, or (SORTED) window blockIdx.x of the chunk in global scratch, sorted by the launches before
template <typename T, int KIND, bool SORTED>
__global__ __launch_bounds__(SH_NT) void k_sht_select(const T *__restrict__ X, int64_t sig_stride, int n, const int *__restrict__ list,
                                                      const int *__restrict__ cnts, const int *__restrict__ leaf, int maxleaves, int npad,
                                                      int elbows, T *gscratch, T *__restrict__ tout)
{
    __shared__ ShShared<T> S;
    const int sig = list[blockIdx.x];
    const int cnt = min(cnts[sig], npad);                              // the class says cnt <= npad; the window holds no more
    T *v = sh_window<T>(gscratch, npad);
    if (!SORTED) {
        sh_stage<T>(v, X + (int64_t)sig * sig_stride, n, leaf + (int64_t)sig * maxleaves, maxleaves, cnt, npad);
        sh_bitonic<T>(v, npad);
    }
    const T t = KIND == 0 ? sh_sure_pick<T>(v, cnt, npad, S) : sh_relerror_pick<T>(v, cnt, npad, elbows, S);
    if (threadIdx.x == 0) tout[sig] = t;
}

inline int sht_single(int kind, const double *X, int64_t n, int64_t k, int64_t nb, const uint8_t *mask, int elbows, double *t, void *st)
{ return kind == 0 ? wx_surethreshold_f64(X, n, k, nb, mask, t, st) : wx_relerrorthreshold_f64(X, n, k, nb, mask, elbows, t, st); }
inline int sht_single(int kind, const float *X, int64_t n, int64_t k, int64_t nb, const uint8_t *mask, int elbows, float *t, void *st)
{ return kind == 0 ? wx_surethreshold_f32(X, n, k, nb, mask, t, st) : wx_relerrorthreshold_f32(X, n, k, nb, mask, elbows, t, st); }

// what the driver (wx_trees_host.h) needs to know of a redundant packet table and of the selection: one output value per item
template <typename T> struct ShtShape {
    int64_t n, ncols, batch;
    int kind, elbows;                                                  // kind 0: surethreshold, 1: relerrorthreshold
    bool has_out;
    static constexpr bool quad = false;
    static constexpr bool extras = true;
    static constexpr bool table = true;                                // the input item is the table; its depth bounds the trees
    bool dims_ok() const { return n >= 1 && ncols >= 1; }
    int64_t count() const { return 1; }
    int64_t in_count() const { return n * ncols; }
    // the deepest tree the table holds: 2^(D + 1) - 1 <= ncols, never deeper than a valid tree (DrtShape, wx_denoise_red_trees.hip)
    int dmax() const
    {
        int D = 0;
        while (D < 30 && ((int64_t)1 << (D + 2)) - 1 <= ncols && ((int64_t)2 << D) <= n) ++D;
        return D;
    }
    int tree_k() const { return dmax() + 1; }
    int too_deep() const { return wx_set_error(WX_EBOUNDS, "tree reaches below the last column of xw"); }
    int check(bool, int, int64_t ntree) const
    {
        WX_REQUIRE(has_out || batch == 0, WX_EARG, "NULL t");
        WX_REQUIRE(kind == 0 || elbows >= 1, WX_EASSERT, "@assert elbows >= 1 (Denoising.jl:291)");
        WX_REQUIRE(wx_isdyadic(n), WX_EASSERT, "maketree/isvalidtree: signal length must be dyadic (Wavelets.jl)");
        WX_REQUIRE(ntree == n - 1, WX_EASSERT, "@assert n_t == gettreelength(sz...) (Utils.jl:211)");
        WX_REQUIRE(n < ((int64_t)1 << 30) && ncols < ((int64_t)1 << 31) && batch < ((int64_t)1 << 31), WX_EUNSUPPORTED,
                   "threshold selection (trees): table too large");
        // the deepest tree the table admits has 2^dmax leaves
        WX_REQUIRE(n <= (SHT_MAX >> dmax()), WX_EUNSUPPORTED, "threshold selection over more than 2^27 coefficients per signal");
        return WX_OK;
    }
    int check_host(const uint8_t *trees, int64_t ntree, int64_t nb, int k, uint32_t *bits, int nw, uint8_t *depths, bool *same) const
    { return wx_trees_check_host(false, n, 1, trees, ntree, nb, k, -1, bits, nw, depths, same); }
    template <typename U> bool window(int64_t, int) const { return true; }   // both tiers are launch()'s
    ShtShape at(int64_t) const
    {
        ShtShape s = *this;
        s.batch = 1;
        return s;
    }
    bool stage(WxIO &, int64_t) const { return true; }
    // one tree for `nb` signals: the single-tree entry with the leaf mask of that tree
    int single(int, const T *x, T *y, int, const uint8_t *t, int64_t nt, int64_t nb, const double *, int, void *stream) const
    {
        std::vector<uint8_t> mask((size_t)ncols);
        for (int64_t i = 1; i <= ncols; ++i)
            mask[(size_t)(i - 1)] = !(i <= nt && t[i - 1]) && (i == 1 || ((i >> 1) <= nt && t[(i >> 1) - 1]));
        return sht_single(kind, x, n, ncols, nb, mask.data(), elbows, y, stream);
    }
    template <int KIND, bool SORTED>
    void select(unsigned grid, size_t lds, hipStream_t st, const T *dx, const int *list, const int *cnt, const int *leaf, int maxleaves,
                int npad, T *gs, T *dy) const
    {
        hipLaunchKernelGGL((k_sht_select<T, KIND, SORTED>), dim3(grid), dim3(SH_NT), lds, st, dx, n * ncols, (int)n, list, cnt, leaf, maxleaves,
                           npad, elbows, gs, dy);
    }
    template <typename U, int MODE>
    hipError_t launch(const T *dx, T *dy, int64_t ntree, int, int64_t nb, const uint32_t *dt, const uint8_t *, const WxFilt &, hipStream_t st) const
    {
        const int D = dmax(), maxleaves = 1 << D;
        const int nodes = (int)((((int64_t)2 << D) - 1 < ncols) ? ((int64_t)2 << D) - 1 : ncols);
        WxScratch scr(st);
        int *cnt = (int *)scr.alloc(sizeof(int) * ((size_t)2 * nb + SHT_CLASSES));
        int *leaf = (int *)scr.alloc(sizeof(int) * (size_t)maxleaves * (size_t)nb);
        if (!cnt || !leaf) return hipErrorOutOfMemory;
        int *list = cnt + nb, *hist = list + nb;
        const int64_t g = (nb + 3) / 4;
        hipLaunchKernelGGL(k_sht_leaves, dim3((unsigned)(g < 8192 ? g : 8192)), dim3(256), 0, st, dt, wq_words(ntree), (int)ntree, nodes, (int)n,
                           maxleaves, nb, cnt, leaf);
        hipLaunchKernelGGL(k_sht_classes, dim3(1), dim3(256), 0, st, cnt, (int)nb, hist, list);
        hipError_t e = hipGetLastError();
        int h[SHT_CLASSES];
        if (e == hipSuccess) e = hipMemcpyAsync(h, hist, sizeof(h), hipMemcpyDeviceToHost, st);
        if (e == hipSuccess) e = hipStreamSynchronize(st);             // the one record that comes back: how many signals each class has
        if (e != hipSuccess) return e;
        // signals of class c per chunk of the scratch tier (0: the class is empty or sorts in LDS), and one scratch for the largest chunk
        auto chunk = [&](int c) -> int64_t {
            const size_t win = (size_t)(((int64_t)2 << c) + 8) * sizeof(T);
            if (h[c] == 0 || win <= SHT_LDS) return 0;
            int64_t per = (int64_t)(SHT_CHUNK / win);
            if (per < 1) per = 1;
            if (per > h[c]) per = h[c];
            return per < 65535 ? per : 65535;                          // gridDim.y
        };
        size_t need = 0;
        for (int c = 1; c < SHT_CLASSES; ++c) {
            const size_t b = (size_t)chunk(c) * (size_t)(((int64_t)2 << c) + 8) * sizeof(T);
            if (b > need) need = b;
        }
        T *gs = need ? (T *)scr.alloc(need) : nullptr;
        if (need && !gs) return hipErrorOutOfMemory;
        int64_t first = 0;                                             // of the class in `list`
        for (int c = 1; c < SHT_CLASSES; first += h[c], ++c) {
            if (h[c] == 0) continue;
            const int64_t npad = (int64_t)1 << c;
            const size_t win = (size_t)(2 * npad + 8) * sizeof(T);      // sorted magnitudes + the curve (cnt + 1 points)
            const int *cl = list + first;
            if (win <= SHT_LDS) {
                if (win > 48 * 1024) {
                    const void *f = kind == 0 ? reinterpret_cast<const void *>(k_sht_select<T, 0, false>)
                                              : reinterpret_cast<const void *>(k_sht_select<T, 1, false>);
                    if ((e = hipFuncSetAttribute(f, hipFuncAttributeMaxDynamicSharedMemorySize, (int)win)) != hipSuccess) return e;
                }
                if (kind == 0) select<0, false>((unsigned)h[c], win, st, dx, cl, cnt, leaf, maxleaves, (int)npad, nullptr, dy);
                else select<1, false>((unsigned)h[c], win, st, dx, cl, cnt, leaf, maxleaves, (int)npad, nullptr, dy);
                continue;
            }
            // windows in global scratch (npad >= 2 SH_CH here), `per` signals of the class at a time
            const int64_t per = chunk(c);
            const unsigned gx = (unsigned)((npad + SH_NT - 1) / SH_NT < 65535 ? (npad + SH_NT - 1) / SH_NT : 65535);
            for (int64_t s0 = 0; s0 < h[c]; s0 += per) {
                const unsigned ns = (unsigned)(h[c] - s0 < per ? h[c] - s0 : per);
                hipLaunchKernelGGL(k_sht_stage_g<T>, dim3(gx, ns), dim3(SH_NT), 0, st, dx, n * ncols, (int)n, cl + s0, cnt, leaf, maxleaves, (int)npad,
                                   gs);
                sh_chip_sort<T>(gs, npad, ns, st);
                if (kind == 0) select<0, true>(ns, 0, st, dx, cl + s0, cnt, leaf, maxleaves, (int)npad, gs, dy);
                else select<1, true>(ns, 0, st, dx, cl + s0, cnt, leaf, maxleaves, (int)npad, gs, dy);
            }
        }
        return hipGetLastError();
    }
};

template <typename T>
int api_shrink_trees(int kind, const T *xw, int64_t n, int64_t ncols, const uint8_t *trees, int64_t ntree, int64_t batch, int elbows, T *t,
                     void *stream)
{
    const ShtShape<T> s{n, ncols, batch, kind, elbows, t != nullptr};
    return wx_trees_api<T, WX_TREES_INV>(s, xw, t, 1, trees, ntree, batch, nullptr, 0, stream);
}

}  // namespace

extern "C" {

int wx_surethreshold_trees_f64(const double *xw, int64_t n, int64_t ncols, const uint8_t *trees, int64_t ntree, int64_t batch, double *t,
                               void *stream)
{ return api_shrink_trees<double>(0, xw, n, ncols, trees, ntree, batch, 1, t, stream); }
int wx_surethreshold_trees_f32(const float *xw, int64_t n, int64_t ncols, const uint8_t *trees, int64_t ntree, int64_t batch, float *t,
                               void *stream)
{ return api_shrink_trees<float>(0, xw, n, ncols, trees, ntree, batch, 1, t, stream); }
int wx_relerrorthreshold_trees_f64(const double *xw, int64_t n, int64_t ncols, const uint8_t *trees, int64_t ntree, int64_t batch, int elbows,
                                   double *t, void *stream)
{ return api_shrink_trees<double>(1, xw, n, ncols, trees, ntree, batch, elbows, t, stream); }
int wx_relerrorthreshold_trees_f32(const float *xw, int64_t n, int64_t ncols, const uint8_t *trees, int64_t ntree, int64_t batch, int elbows,
                                   float *t, void *stream)
{ return api_shrink_trees<float>(1, xw, n, ncols, trees, ntree, batch, elbows, t, stream); }

}  // extern "C"
