// wx_dwt2d_trace.h -- the launch record of the 2-D decimated transforms (wx_debug.h: wx_debug_dwt2d_trace_begin / _end).  Test
// infrastructure: the launchers append what they launch, nothing in the product path reads the record.  Disarmed (always, outside
// a test's trace block) a hook is one relaxed load of the flag.
#pragma once
#include <atomic>
#include <stddef.h>
#include <hip/hip_runtime.h>

// route ids of wx_debug.h
enum {
    WX_R2_Q64W = 1, WX_R2_Q64TPREP, WX_R2_Q64T, WX_R2_Q64, WX_R2_PYR, WX_R2_TAIL, WX_R2_L2DF, WX_R2_L2DC, WX_R2_COL1D, WX_R2_LROWS,
    WX_R2_ROWS, WX_R2_TILE, WX_R2_TILEP, WX_R2_ITILE, WX_R2_ITILEP, WX_R2_TWO, WX_R2_COPYB, WX_R2_GATHER
};

extern std::atomic<int> wx_dwt2d_trace_armed;                                   // wx_dwt2d.hip
void wx_dwt2d_trace_add(int route, int inverse, int depth, int K, size_t esz, dim3 grid, dim3 block, size_t lds, int e0 = 0, int e1 = 0,
                        int e2 = 0, int e3 = 0, int e4 = 0, int e5 = 0);

#define WX_DWT2D_TRACE(...) \
    do { if (wx_dwt2d_trace_armed.load(std::memory_order_relaxed)) wx_dwt2d_trace_add(__VA_ARGS__); } while (0)
