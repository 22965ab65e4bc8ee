// wx_nodegeom.h -- which coefficients of a packet table one entry of a best-basis cost vector covers (heap order), shared by
// the JBB and LSDB node-cost kernels.
//   1-D, bestbasis/bestbasis_tree.jl:104-126, 150-180: entry idx (0-based) of a (n, k) table is node (depth d, node j) with
//       idx + 1 = 2^d + j, i.e. rows [j n/2^d, (j+1) n/2^d) of column d; redundant: all n rows of column idx, weight 1/2^d.
//   2-D, :128-147, 182-207: quad-tree heap index idx + 1 of an (m rows, n cols, k) table; the node's (rows, cols) block of slice
//       d (Utils.jl:465-542 geometry through the morton code of the heap index); redundant: all of slice idx, weight 1/4^d.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

struct WxNode1d { int col, off, len, depth; };

static __device__ __forceinline__ WxNode1d wx_node1d(int idx, int n, int redundant)
{
    WxNode1d g;
    g.depth = 0;
    for (int t = idx + 1; t > 1; t >>= 1) ++g.depth;             // heap order == (lvl, node) order
    if (redundant) { g.col = idx; g.off = 0; g.len = n; }
    else {
        const int node = idx + 1 - (1 << g.depth);
        g.col = g.depth; g.len = n >> g.depth; g.off = node * g.len;
    }
    return g;
}

struct WxNode2d { int64_t slice; int r0, c0, nr, ncl, depth; };

static __device__ __forceinline__ WxNode2d wx_node2d(int64_t idx, int m, int n, int redundant)
{
    WxNode2d g;
    g.depth = 0;
    { int64_t t = 3 * (idx + 1) - 2; while (t >= 4) { t >>= 2; ++g.depth; } }
    int64_t start = 1;
    for (int t = 0; t < g.depth; ++t) start = 4 * start - 2;
    const int64_t mort = idx + 1 - start;
    int jr = 0, jc = 0;
    for (int t = 0; t < g.depth; ++t) { jr |= (int)((mort >> (2 * t + 1)) & 1) << t; jc |= (int)((mort >> (2 * t)) & 1) << t; }
    if (redundant) { g.slice = idx; g.r0 = 0; g.c0 = 0; g.nr = m; g.ncl = n; }
    else { g.slice = g.depth; g.nr = m >> g.depth; g.ncl = n >> g.depth; g.r0 = jr * g.nr; g.c0 = jc * g.ncl; }
    return g;
}
