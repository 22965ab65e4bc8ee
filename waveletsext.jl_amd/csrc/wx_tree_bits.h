// wx_tree_bits.h -- the bit layout of a tree as k_wpt_trees (wx_wpt_trees.hip, binary heap) and k_wpt_trees2d (wx_wpt_trees2d.hip,
// quad heap) read it, shared by the host pass that packs a host tree matrix and by the kernel that packs a device one (both in
// wx_trees_prep.hip): node i (1-based, heap order of either heap) is bit (i - 1) & 31 of word (i - 1) >> 5; ceil(ntree / 32) words
// per tree (at least one), the bits past node ntree are zero.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string.h>

// words of tree bits per tree, from the signal length n (k_wpt_trees) and from the number of nodes: wt_words(n) == wq_words(n - 1)
// for every dyadic n, the only lengths with trees
__host__ __device__ __forceinline__ int wt_words(int64_t n) { return n >= 32 ? (int)(n >> 5) : 1; }
__host__ __device__ __forceinline__ int wq_words(int64_t ntree) { return ntree > 32 ? (int)((ntree + 31) >> 5) : 1; }
__host__ __device__ __forceinline__ bool wt_set(const uint32_t *tree, int node) { return (tree[(node - 1) >> 5] >> ((node - 1) & 31)) & 1u; }

// one column of a host tree matrix (ntree bytes, any non-zero byte = decomposed) into its words; `words` is zero on entry (little-endian
// host).  Eight nodes at a time: 0x80 where a byte is non-zero, then the eight flags gathered into one byte by a multiplication.
static inline void wt_pack_host(const uint8_t *t, int64_t ntree, uint32_t *words)
{
    uint8_t *w = reinterpret_cast<uint8_t *>(words);
    int64_t i = 0;
    for (; i + 8 <= ntree; i += 8) {
        uint64_t v;
        memcpy(&v, t + i, 8);
        v = ((((v & 0x7f7f7f7f7f7f7f7fULL) + 0x7f7f7f7f7f7f7f7fULL) | v) & 0x8080808080808080ULL) >> 7;
        w[i >> 3] = (uint8_t)((v * 0x0102040810204080ULL) >> 56);
    }
    for (; i < ntree; ++i) w[i >> 3] |= (uint8_t)((t[i] != 0) << (i & 7));
}
