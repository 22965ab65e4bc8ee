// wx_trees_prep.hip -- the check of a matrix of per-signal trees, for every consumer: wptall / iwptall / iwpdall with one tree per
// signal or image (wx_trees_host.h) and getbasiscoefall (wx_gathertrees.hip).  One pass checks every column (wx_isvalidtree*,
// wx_tree_depth*), compares it with column 0 and packs it into bits: wx_trees_check_host for a matrix in host memory, and
// k_trees_prep, the same pass as one launch, for one that stays on the device -- bestbasistreeall(X, BB()) selects every signal's
// tree on the GPU (wx_treeselect_batch_*, an (ntree, batch) byte matrix) --, from which only a record of three words comes back.
//
// A wavefront walks a column 64 nodes at a time: lane l of step s holds node 64 s + l + 1, and the ballot of "decomposed" IS
// words 2 s and 2 s + 1 of the column's bit layout (wx_tree_bits.h).  The parent of a node (c >> 1, quad trees (c + 2) >> 2) lies
// in an earlier part of the same column: its byte is read again (the column has just come through the cache) instead of kept.
// Up to 4095 nodes a wavefront takes a column on its own (four columns per workgroup, no barrier); longer columns are shared by
// the sixteen wavefronts of a workgroup, which combine their flags and highest nodes through LDS.
// Columns start at b * ntree, an odd stride: every load is a byte load, and every index is clamped to the column, so nothing is
// read past the matrix.  Every output element has one writer; the record takes atomicMin.
#include "../../include/waveletsext_hip.h"
#include "wx_common.h"
#include "wx_debug.h"
#include "wx_host.h"
#include "wx_tree_bits.h"
#include "wx_trees_prep.h"
#include <thread>
#include <vector>

namespace {

// rec[0]: lowest invalid column; rec[1]: lowest column of depth >= k; rec[2]: 0 once a column differs from column 0.  All ones on entry.
enum { REC_INVALID = 0, REC_DEEP = 1, REC_SAME = 2, REC_WORDS = 3 };

template <bool QUAD, bool TEAM>
__global__ __launch_bounds__(TEAM ? 1024 : 256) void k_trees_prep(const uint8_t *__restrict__ trees, int ntree, int64_t batch, int k,
                                                                  uint32_t *__restrict__ bits, int nw, uint8_t *__restrict__ depths,
                                                                  int want_same, unsigned long long *__restrict__ rec)
{
    __shared__ int s_top[16], s_flags[16];
    const int lane = threadIdx.x & (WX_WAVE - 1), wave = threadIdx.x / WX_WAVE, nwave = blockDim.x / WX_WAVE;
    const int64_t per_block = TEAM ? 1 : nwave;                       // columns a workgroup has in hand
    const int sub = TEAM ? wave : 0, nsub = TEAM ? nwave : 1;          // this wavefront's share of the column's steps
    const int nstep = (ntree + WX_WAVE - 1) / WX_WAVE;
    for (int64_t b = (int64_t)blockIdx.x * per_block + (TEAM ? 0 : wave); b < batch; b += (int64_t)gridDim.x * per_block) {
        const uint8_t *tg = trees + b * (int64_t)ntree;
        bool bad = false, diff = false;
        int top = 0;                                                   // the highest decomposed node seen (1-based), wave-uniform
        for (int s0 = sub; s0 < nstep; s0 += 4 * nsub) {               // four steps' loads in flight, then their ballots
            uint8_t v[4], pv[4], v0[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const int i = (s0 + u * nsub) * WX_WAVE + lane;
                const int ii = i < ntree ? i : ntree - 1;              // loads stay inside the column whatever the lane and the step
                const int c = ii + 1, par = QUAD ? (c + 2) >> 2 : c >> 1;   // par == 0: the root
                v[u] = tg[ii];
                pv[u] = tg[par > 0 ? par - 1 : 0];
                v0[u] = want_same ? trees[ii] : v[u];
            }
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const int s = s0 + u * nsub;
                if (s >= nstep) break;                                 // wave-uniform
                const int i = s * WX_WAVE + lane;
                const bool set = i < ntree && v[u] != 0;
                bad |= set && i > 0 && pv[u] == 0;
                diff |= v[u] != v0[u];
                const unsigned long long m = __ballot(set);
                if (bits && lane < 2 && 2 * s + lane < nw) bits[b * (int64_t)nw + 2 * s + lane] = (uint32_t)(m >> (32 * lane));
                if (m) top = s * WX_WAVE + 64 - __clzll((long long)m);
            }
        }
        int flags = (__ballot(bad) != 0 ? 1 : 0) | (__ballot(diff) != 0 ? 2 : 0);
        if (TEAM) {
            __syncthreads();                                           // the previous column has been read out of s_top / s_flags
            if (lane == 0) { s_top[wave] = top; s_flags[wave] = flags; }
            __syncthreads();
            for (int w = 0; w < nwave; ++w) { top = max(top, s_top[w]); flags |= s_flags[w]; }
        }
        if (lane == 0 && sub == 0) {
            // depth of the deepest decomposed node + 1: wx_getdepth_binary / wx_getdepth_quad of `top`
            const int depth = top == 0 ? 0 : (QUAD ? ((63 - __clzll(3LL * top - 2)) >> 1) + 1 : 32 - __clz(top));
            if (depths) depths[b] = (uint8_t)depth;
            if (flags & 1) atomicMin(rec + REC_INVALID, (unsigned long long)b);
            else if (k > 0 && depth >= k) atomicMin(rec + REC_DEEP, (unsigned long long)b);
            if (flags & 2) atomicMin(rec + REC_SAME, 0ULL);
        }
    }
}

thread_local int g_trees_route = WX_TREES_ROUTE_NONE;

}  // namespace

void wx_trees_route_set(int route) { g_trees_route = route; }

int wx_trees_prep(bool quad, const uint8_t *trees, int64_t ntree, int64_t batch, int k, uint32_t *bits, int nw, uint8_t *depths,
                  uint8_t *col0, bool *same, hipStream_t st)
{
    if (same) *same = true;
    if (ntree <= 0 || batch <= 0) return WX_OK;
    if (ntree >= ((int64_t)1 << 31)) return wx_set_error(WX_EUNSUPPORTED, "tree matrix: 2^31 nodes and more per tree not supported");
    WxScratch scr(st);
    unsigned long long *rec = (unsigned long long *)scr.alloc(sizeof(unsigned long long) * REC_WORDS);
    if (!rec) return WX_EHIP;
    hipError_t e = hipMemsetAsync(rec, 0xff, sizeof(unsigned long long) * REC_WORDS, st);
    if (e != hipSuccess) return wx_set_hip_error(e, "tree matrix: status record", __FILE__, __LINE__);
    const bool team = ntree > 4095;
    const int64_t per_block = team ? 1 : 4;
    const int64_t want = (batch + per_block - 1) / per_block;
    const dim3 grid((unsigned)(want < 65536 ? want : 65536)), block(team ? 1024 : 256);
    const int want_same = same ? 1 : 0;
    if (quad) {
        if (team) hipLaunchKernelGGL((k_trees_prep<true, true>), grid, block, 0, st, trees, (int)ntree, batch, k, bits, nw, depths, want_same, rec);
        else hipLaunchKernelGGL((k_trees_prep<true, false>), grid, block, 0, st, trees, (int)ntree, batch, k, bits, nw, depths, want_same, rec);
    } else {
        if (team) hipLaunchKernelGGL((k_trees_prep<false, true>), grid, block, 0, st, trees, (int)ntree, batch, k, bits, nw, depths, want_same, rec);
        else hipLaunchKernelGGL((k_trees_prep<false, false>), grid, block, 0, st, trees, (int)ntree, batch, k, bits, nw, depths, want_same, rec);
    }
    e = hipGetLastError();
    unsigned long long host[REC_WORDS] = {0, 0, 0};
    if (e == hipSuccess) e = hipMemcpyAsync(host, rec, sizeof host, hipMemcpyDeviceToHost, st);
    if (e == hipSuccess && same && col0) e = hipMemcpyAsync(col0, trees, (size_t)ntree, hipMemcpyDeviceToHost, st);
    if (e == hipSuccess) e = hipStreamSynchronize(st);                 // the one wait: the record decides what is launched next
    if (e != hipSuccess) {
        (void)hipStreamSynchronize(st);
        return wx_set_hip_error(e, "tree matrix: check on the device", __FILE__, __LINE__);
    }
    // a column is counted once, as invalid or as too deep: the lower index is the first offending column
    if (host[REC_INVALID] < host[REC_DEEP]) return wx_set_error(WX_EASSERT, "@assert all(mapslices(isvalidtree, tree)) (Utils.jl:209)");
    if (host[REC_DEEP] != ~0ULL) return wx_set_error(WX_EARG, "Not enough decomposition levels in Xw (Utils.jl:120)");
    if (same) *same = host[REC_SAME] != 0;
    return WX_OK;
}

int wx_trees_check_host(bool quad, int64_t m, int64_t n, const uint8_t *trees, int64_t ntree, int64_t batch, int k, int max_depth,
                        uint32_t *bits, int nw, uint8_t *depths, bool *same)
{
    enum { BAD_TREE = 1, BAD_SIDES = 2, BAD_K = 3 };
    struct Part { int code = 0; bool same = true; };                   // of a range of columns: its first error, all equal to column 0
    auto check = [&](int64_t b0, int64_t b1, Part *out) {
        for (int64_t b = b0; b < b1; ++b) {
            const uint8_t *t = trees + b * ntree;
            int code = 0;
            if (!(quad ? wx_isvalidtree2d(m, n, t, ntree) : wx_isvalidtree1d(m, t, ntree))) code = BAD_TREE;
            else {
                const int depth = quad ? wx_tree_depth2d(t, ntree) : wx_tree_depth1d(t, ntree);
                if (depths) depths[b] = (uint8_t)depth;
                if (max_depth >= 0 && depth > max_depth) code = BAD_SIDES;
                else if (k > 0 && depth >= k) code = BAD_K;
            }
            if (code) { out->code = code; return; }
            if (same && out->same && ntree > 0) out->same = memcmp(trees, t, (size_t)ntree) == 0;
            if (bits) wt_pack_host(t, ntree, bits + (size_t)b * nw);
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
    bool all_same = true;
    for (const Part &pt : parts) {                                      // in column order
        if (pt.code == BAD_TREE) return wx_set_error(WX_EASSERT, "@assert all(mapslices(isvalidtree, tree)) (Utils.jl:209)");
        if (pt.code == BAD_SIDES) return wx_set_error(WX_EASSERT, "both sides must be divisible by 2^depth(tree) (dwt_step! size asserts)");
        if (pt.code) return wx_set_error(WX_EARG, "Not enough decomposition levels in Xw (Utils.jl:120)");
        all_same = all_same && pt.same;
    }
    if (same) *same = all_same;
    return WX_OK;
}

extern "C" int wx_wpt_trees_last_route(void) { return g_trees_route; }

// wx_debug.h: the host form of the bit layout, for the suite to compare with its own packing
extern "C" int wx_debug_pack_tree1d(const uint8_t *tree, int64_t n, uint32_t *words)
{
    if (!tree || !words || n < 2) return WX_EARG;
    const int nw = wt_words(n);
    memset(words, 0, sizeof(uint32_t) * (size_t)nw);
    wt_pack_host(tree, n - 1, words);
    return nw;
}
