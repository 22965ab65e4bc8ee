// wx_swt1d_trace.h -- the launch record of the 1-D redundant transforms (wx_debug.h: wx_debug_swt1d_trace_begin / _end).  Test
// infrastructure: the launchers append what they launch, nothing in the product path reads the record.  Disarmed (always, outside
// a test's trace block) a hook is one relaxed load of the flag.
#pragma once
#include <atomic>
#include <stddef.h>
#include <hip/hip_runtime.h>

// route ids of wx_debug.h
enum {
    WX_RT_FG = 1, WX_RT_FSD, WX_RT_FSDIP, WX_RT_FTWO, WX_RT_FLVL, WX_RT_FM, WX_RT_FMRC, WX_RT_FHAAR6, WX_RT_FDEEP,
    WX_RT_ISD, WX_RT_ISDIP, WX_RT_IM, WX_RT_IHAAR6, WX_RT_IDEEP, WX_RT_ITILE, WX_RT_ILVL, WX_RT_IACDWT, WX_RT_IACWPT, WX_RT_IACWPD
};

extern std::atomic<int> wx_swt1d_trace_armed;                                   // wx_swt1d.hip
void wx_swt1d_trace_add(int route, int depth, int K, int R, int OPT, size_t esz, dim3 grid, dim3 block, size_t lds);

#define WX_SWT1D_TRACE(...) \
    do { if (wx_swt1d_trace_armed.load(std::memory_order_relaxed)) wx_swt1d_trace_add(__VA_ARGS__); } while (0)
