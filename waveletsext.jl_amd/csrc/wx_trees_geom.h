// wx_trees_geom.h -- the launch geometry of the kernels in which a workgroup takes one item (a signal, an image) and strides over the
// batch: the per-signal-tree kernels behind wx_trees_host.h, and the kernels that start from the signals (wx_wpd_bb.hip, wx_red_bb.h).
#pragma once
#include <stddef.h>
#include <stdint.h>

// one lane per output pair of a level or pass, at most 1024
inline int wx_trees_threads(int64_t count)
{
    int nt = 64;
    while (nt < 1024 && nt < count / 2) nt <<= 1;
    return nt;
}

// workgroups resident on the 256 CUs (160 KiB of LDS and 2048 lanes each, at most 16 workgroups), never more than items
inline int wx_trees_grid(size_t lds, int nt, int64_t batch)
{
    int per_cu = (int)((160 * 1024) / lds);
    if (per_cu > 2048 / nt) per_cu = 2048 / nt;
    if (per_cu > 16) per_cu = 16;
    if (per_cu < 1) per_cu = 1;
    const int64_t g = (int64_t)256 * per_cu;
    return (int)(g < batch ? g : batch);
}
