// wx_dwt1d_trace.h -- the launch record of the 1-D decimated transforms (wx_debug.h: wx_debug_dwt1d_trace_begin / _end): wpd, wpt,
// iwpt, iwpd, dwt / idwt of signals and the thresholded inverse behind denoise.  Test infrastructure: the dispatch code (wx_api.hip,
// wx_dwt1d.hip) appends what it launches, nothing in the product path reads the record.  Disarmed (always, outside a test's trace
// block) a hook is one relaxed load of the flag.  The one-pass kernels of denoiseall (wx_lattice_denoise*_f64, wx_lattice_dn.h) are
// NOT recorded: test_gpu_denoise_onepass.py covers them, and a call they take leaves an empty record.
#pragma once
#include <atomic>
#include <stddef.h>
#include <stdint.h>

// route ids of wx_debug.h
enum {
    WX_R1_LATF64 = 1, WX_R1_LATWPD, WX_R1_LATF32, WX_R1_LATTREE, WX_R1_LAT8KT, WX_R1_LANETREE, WX_R1_SMALLTREE, WX_R1_HAAR, WX_R1_TOP,
    WX_R1_TOPWPD, WX_R1_FUSED, WX_R1_L1TILE, WX_R1_LEVEL, WX_R1_GATHER, WX_R1_TAIL, WX_R1_ITAIL, WX_R1_THRFUSED, WX_R1_THRCOPY
};

extern std::atomic<int> wx_dwt1d_trace_armed;                                   // wx_dwt1d.hip
// signals is clamped to int32; block, grid and lds are those of the kernels wx_dwt1d.hip launches itself, 0 for the other launchers
void wx_dwt1d_trace_add(int route, int inverse, size_t esz, int64_t n, int depth, int K, int64_t signals, int F, int e0 = 0, int e1 = 0,
                        int e2 = 0, int e3 = 0, int e4 = 0, unsigned block = 0, unsigned grid = 0, size_t lds = 0);
// What a launcher cannot see, or its caller cannot: the caller of a launcher of wx_dwt1d.hip that records its own row (FUSED, L1TILE)
// leaves the depth its pass starts from; wx_lattice_launch (wx_lattice.hip) leaves whether it took the folded full-depth inverse, which
// its arguments do not tell from the general kernel.  Thread-local; the next row of this thread that wants the value takes and clears it.
// Every entry of the dispatch (wx_dev_wpd1d, _wpt1d, _iwpt1d, _dwt_long, ...) clears the depth, and wx_lattice_wpt_f64 / _iwpt_f64 clear
// `folded`, so a note that nobody took (a launcher that returned an error before its hook, a caller outside this record) never reaches a later row.
void wx_dwt1d_trace_set_depth(int depth);
void wx_dwt1d_trace_set_folded(int folded);
int wx_dwt1d_trace_take_depth();
int wx_dwt1d_trace_take_folded();

#define WX_DWT1D_TRACE(...) \
    do { if (wx_dwt1d_trace_armed.load(std::memory_order_relaxed)) wx_dwt1d_trace_add(__VA_ARGS__); } while (0)
#define WX_DWT1D_TRACE_DEPTH(d) \
    do { if (wx_dwt1d_trace_armed.load(std::memory_order_relaxed)) wx_dwt1d_trace_set_depth(d); } while (0)
#define WX_DWT1D_TRACE_FOLDED(f) \
    do { if (wx_dwt1d_trace_armed.load(std::memory_order_relaxed)) wx_dwt1d_trace_set_folded(f); } while (0)
