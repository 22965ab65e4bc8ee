// wx_debug.h -- NOT part of the C ABI (include/waveletsext_hip.h): dispatch override used by the parity suite to run the same
// inputs through more than one kernel family.  Process-global; nothing in the product path calls it.
#pragma once
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif
/* 0 = normal dispatch; 1 = one level per launch instead of the fused kernels; 2 = keep the fused LDS kernels but skip the
 * register-resident ones (Haar Walsh-Hadamard, lattice); 3 = normal dispatch, but the full-depth lattice inverse without the fold
 * of its deepest levels (wx_lattice_fold.h): the general kernel, as for every other depth */
void wx_debug_set_dispatch(int mode);

/* The node matrix (row-major, NF x NF, NF = 2, 4 or 8) that folds the deepest log2(NF) levels of a full-depth lattice transform for
 * the QMF q of length F, as the launchers build it (wx_lattice_fold_matrix).  Returns NF, or 0 when this filter does not fold. */
int wx_debug_lattice_fold(const double *q, int F, int NF, int inverse, double *m);

/* The lattice factorisation of the QMF q of length F as the launchers run it for a transform of L levels (wx_lattice_factor for
 * elem_size 8: kernels with Float64 registers; wx_lattice_factor32 with LW = L for elem_size 4: kernels that compute in Float32 and
 * normalise once -- the tree-driven Float32 kernels normalise every level and apply the window of L = 1).  p and kap receive 10
 * values (zero past F / 2), g0 = g^(+-L), g2 = g^(-+2).  Returns 1 = accepted, 0 = declined (the direct-form kernels run) or
 * arguments outside 2 <= F <= 64, L >= 1.  Needs no device. */
int wx_debug_lattice_factor(const double *q, int F, int L, int inverse, int elem_size, double *p, double *kap, double *g0, double *g2);

/* Which kernels the 2-D redundant transforms (wx_swt2d.hip) launch under the current dispatch mode; computed by the very
 * function the launch code calls.  elem_size 8 / 4 = Float64 / Float32, F = filter length, ac = autocorrelation family,
 * shift = shift-based inverse (sm given).  Returns route + 256 * R, or -1 for arguments outside the transforms' domain:
 *   forward (inverse = 0), one route for the whole call of L levels:
 *     1  F1  k_red2d_fwd_fused, strips of R rows over whole rows        2  F2  k_red2d_fwd_fused, column tiles with halo
 *     3  F3  k_red2d_fwd_dim1 + k_red2d_fwd_dim2
 *   inverse (inverse = 1), the route of the level of depth L - 1 (ask every L' in 1..L for a whole call):
 *     4  I1  k_red2d_inv_fused, strips of R rows                        5  I2  k_red2d_inv_dim2 + _dim1, average based
 *     6  I3  k_red2d_inv_dim2 + _dim1, shift based                      7  I4  k_red2d_iac
 * R is the strip height of the deepest level (depth L - 1) for F1, F2 and I1, and 0 for the other routes.  Mode 1 of
 * wx_debug_set_dispatch turns F1 / F2 into F3 and I1 into I2. */
int wx_debug_red2d_route(int inverse, int64_t m, int64_t n, int L, int elem_size, int F, int ac, int shift);

/* Launch record of the 1-D redundant transforms (wx_swt1d.hip, wx_haarswt.hip, wx_swtdeep*.hip): between _begin and _end every
 * kernel launch of wx_dev_swt_fwd, wx_dev_swt_inv, wx_dev_iacdwt / _iacwpt / _iacwpd and of the Haar and lane-local register
 * passes appends one row, written next to the launch from the variables the launch uses.  The record is process-global and
 * mutex-protected; disarmed, a launch site pays one load of a flag.  The fused acwpd + moments path (wx_dev_acwpd_top_moments,
 * wx_acsubtree.hip) is not recorded.  A row is WX_SWT1D_TRACE_FIELDS int32:
 *     route, depth, K, R, OPT, elem_size, blockDim.x, gridDim.x, gridDim.y, gridDim.z, dynamic LDS bytes
 * depth = the depth the pass starts from (forward: the parents' depth; inverse: the children's depth), K = levels in the pass.
 * R and OPT are the residue classes per workgroup and the rows per thread of FMRC and IM; the other routes keep their own
 * extras there (0 where none is named):
 *   forward                                                             R                              OPT
 *     1  FG      k_swt_fwd_level_g, one level from global memory                                       1 = autocorrelation
 *     2  FSD     k_sdwt_fused, all K = L levels                         compile-time taps, 0 = runtime  1 = autocorrelation
 *     3  FSDIP   k_sdwt_fused_ip, all K = L levels in place             compile-time taps, 0 = runtime  1 = autocorrelation
 *     4  FTWO    k_swpd_fwd_two, K = 2                                                                  1 = autocorrelation
 *     5  FLVL    k_swt_fwd_level, K = 1                                                                 1 = autocorrelation
 *     6  FM      k_swt_fwd_multi, whole columns, K = 2 or 3
 *     7  FMRC    k_swt_fwd_multi_rc, K = 2 or 3                         classes per workgroup           rows per thread
 *     8  FHAAR6  k_haar_swpt6_fwd, K = 6
 *     9  FDEEP   lane-local pass, K = LP                                1 = heap table (swpd / acwpd)   1 = autocorrelation
 *   inverse
 *    10  ISD     k_isdwt_avg_fused, all K = L levels                    compile-time taps, 0 = runtime  1 = pipelined
 *    11  ISDIP   k_isdwt_avg_fused_ip, all K = L levels in place
 *    12  IM      k_swt_inv_multi, K = 2 or 3                            classes per workgroup           rows per thread
 *    13  IHAAR6  k_haar_iswpt, K = wx_haar_iswpt_levels()
 *    14  IDEEP   lane-local pass, K = LP
 *    15  ITILE   k_swt_inv_level_tile, K = 1                            HF = taps / 2
 *    16  ILVL    k_swt_inv_level, K = 1                                                                 1 = shift based
 *    17  IACDWT  18  IACWPT  19  IACWPD   k_iacdwt / k_iacwpt / k_iacwpd, all K = L levels
 * _end disarms, copies the first min(cap, recorded) rows to out and returns the number recorded, which is at most
 * WX_SWT1D_TRACE_MAX: launches past that are counted by _dropped (until the next _begin) and not recorded.  _end returns
 * WX_EARG (-2) without _begin before it, or (leaving the record armed) for out == NULL or cap <= 0. */
#define WX_SWT1D_TRACE_FIELDS 11
#define WX_SWT1D_TRACE_MAX (1 << 18)
void wx_debug_swt1d_trace_begin(void);
int wx_debug_swt1d_trace_end(int32_t *out, int cap);
int64_t wx_debug_swt1d_trace_dropped(void);

/* Launch record of the 2-D decimated transforms (wpd, wpt, iwpt, iwpd and dwt / idwt of images: wx_api_2d.hip, wx_dwt2d.hip,
 * wx_lattice_2d64*.h / .hip, wx_lattice_rows.h, wx_lattice2d.h, wx_pyr2d.hip, wx_dwttail.hip): between _begin and _end every
 * kernel launch of that path appends one row, written next to the launch from the variables the launch uses.  Same protocol
 * as the 1-D record above: process-global, mutex-protected, one relaxed load of a flag per launch site when disarmed.  The
 * device-to-device copies (hipMemcpy2DAsync: slice 0 of wpd, depth-0 trees, the inverse without a node list) are not kernels
 * and are not recorded.  A row is WX_DWT2D_TRACE_FIELDS int32:
 *     route, inverse, depth, K, elem_size, blockDim.x, gridDim.x, gridDim.y, gridDim.z, dynamic LDS bytes, e0, e1, e2, e3, e4, e5
 * depth = the depth the pass starts from (forward: the parents' depth; inverse: the children's depth), K = levels in the pass.
 * NS = lattice stages of the kernel's template instance (wx_lat_stages(F)).  Extras e0 .. (0 where none is named):
 *     1  Q64W      k_lat2d64_wpd<NS>: wpd of 64 x 64 images, one wavefront each      NS
 *     2  Q64TPREP  k_lat2d64t_prep: the quad tree's masks and addresses for Q64T
 *     3  Q64T      k_lat2d64t_f64<NS>: 64 x 64 images along a quad tree              NS
 *     4  Q64       k_lat2d64_f64<NS>: 64 x 64 images, full tree                      NS
 *     5  PYR       k_pyr2d_small<T, FT>: whole pyramid of an image in LDS            FT (compile-time taps, 0 = runtime), log2 m, log2 n
 *     6  TAIL      k_dwt2d_tail<T, F>: the K levels from the 8 x 8 approximation on   F, m   (depth is not known there: 0)
 *     7  L2DF      k_lat2d_fused_f32<NS, inverse, HB, E>: both passes, one piece     NS, HB, E, units of the piece
 *                  (a batch of more than 65534 units is as many consecutive L2DF rows as it has pieces)
 *     8  L2DC      k_lat2d_colT_f32<NS, .., HB = 1>: one transposing pass, forward   NS, HB, pass (1 / 2)
 *     9  COL1D     the column pass of the fast path: ONE row from the 2-D caller for the call of the 1-D dispatch
 *                  (wx_dev_wpt1d / wx_dev_iwpt1d; its kernels appear in the 1-D record below when that one is armed, not
 *                  here); block, grid and LDS are 0                                  m, n
 *    10  LROWS     k_lat_rows_g_f64<NS, 2, SH>: row pass on the lattice kernels      NS, SH, wavefronts per workgroup
 *    11  ROWS      k_rows_fused<T, F, INVERSE, V, KI, REGL>: row pass in LDS strips  F, V, KI, REGL, strip height R, pitch S
 *    12  TILE      k_dwt2d_level_tile<T, F>, K = 1 (one row per launch of <= 65535 images)     F, by_node, tree status given, tiles
 *    13  TILEP     k_dwt2d_level_tile_p<T, F>, persistent, K = 1                     F, by_node, tree status given, tiles
 *    14  ITILE     k_idwt2d_level_tile<T, F>, K = 1 (one row per launch)             F, by_node, tree status given, tiles
 *    15  ITILEP    k_idwt2d_level_tile_p<T, F>, persistent, K = 1                    F, by_node, tree status given, tiles
 *    16  TWO       k_dwt2d_dim1 + k_dwt2d_dim2 (inverse: _dim2 + _dim1), K = 1: ONE row for the pair, which shares a grid
 *                                                                                    node list given, copy_inactive, tree status given, nodes
 *    17  COPYB     k_copy_blocks2d, K = 0, depth = first depth below the tile levels nodes
 *    18  GATHER    k_gather_leaves2d, K = 0, always recorded with inverse = 1: iwpd along a partial tree, and getbasiscoef of an
 *                  image table (wx_api_swt2d.hip), which shares the launcher     blocks per side, slices k
 * _end, _dropped and the WX_EARG cases are those of wx_debug_swt1d_trace_end / _dropped. */
#define WX_DWT2D_TRACE_FIELDS 16
#define WX_DWT2D_TRACE_MAX (1 << 16)
void wx_debug_dwt2d_trace_begin(void);
int wx_debug_dwt2d_trace_end(int32_t *out, int cap);
int64_t wx_debug_dwt2d_trace_dropped(void);

/* Launch record of the 1-D decimated transforms (wpd, wpt, iwpt, iwpd, dwt / idwt of signals, the thresholded inverse behind
 * denoise: wx_api.hip, wx_dwt1d.hip and the launchers they call): between _begin and _end every kernel launch of that dispatch
 * appends one row.  A hook sits in the caller, next to the call, and is written from the variables the call uses: a launcher that
 * answers 0 = declined / 1 = launched is recorded when it answers 1, one that always launches just before the call.  The kernels
 * wx_dwt1d.hip launches itself (FUSED, L1TILE, LEVEL, GATHER) record in their launchers, with block, grid and dynamic LDS; those are 0
 * for the other routes.  Same protocol as the records above: process-global, mutex-protected, one relaxed load of a flag per site when
 * disarmed.  Device-to-device copies (hipMemcpy*Async: L = 0, slice 0 of wpd, the densifying copies of iwpd, leaves of long trees)
 * are not kernels and are not recorded; the one-pass kernels of denoiseall (wx_lattice_denoise*_f64) are not recorded either.  The
 * column pass of the 2-D fast path (COL1D above) and the per-signal-tree entries call the same dispatch and show up here.
 * A row is WX_DWT1D_TRACE_FIELDS int32:
 *     route, inverse, elem_size, n, depth, K, signals, F, e0, e1, e2, e3, e4, blockDim.x, gridDim.x, dynamic LDS bytes
 * n and signals are what the launcher was given (the node length and batch << d0 for sub-signal launches; signals clamped to
 * 2^31 - 1), depth = the depth the pass starts from (forward: the parents' depth; inverse: the deepest children's depth), K = levels
 * in the pass, F = filter length.  Extras e0 .. e4 (0 where none is named):
 *     1  LATF64     wx_lattice_wpt_f64 / _iwpt_f64 (n, L fix the kernel: _g 64 .. 512, _sh 1024 / 2048, _lo 4096 at L <= 5, the general
 *                   kernel 4096 at L 6 .. 12, 8k)                                    stages wx_lat_stages(F), folded, in_stride != n
 *     2  LATWPD     wx_lattice_wpd_f64 / wx_lattice_wpd_g_f32                        stages
 *     3  LATF32     wx_lattice_f32                                                   stages, 0, in_stride != n
 *     4  LATTREE    wx_lattice_tree_f64 / _f32 (wx_lattice_tree_T)                   tree of ones for a full tree, col_stride != 0,
 *                                                                                    threshold or head on the loads, out_stride != n, in_stride != n
 *     5  LAT8KT     wx_lattice_tree8k_fwd_f64 / _inv_f64                             depth of the subtree of node (1, 0), of node (1, 1)
 *     6  LANETREE   wx_lane_tree_f64 / _f32                                          full tree (all-ones mask)
 *     7  SMALLTREE  wx_dev_small_tree                                                tree status given
 *     8  HAAR       wx_haar_wpt_f64 / wx_haar_iwpt_f64
 *     9  TOP        wx_dev_top_levels                                                NL, split mask, deep given, input stride != n, deep mask
 *    10  TOPWPD     wx_dev_top_levels_wpd
 *    11  FUSED      k_fwd1d_fused / k_fwd1d_inplace / k_inv1d_fused                  wpd layout, in-place kernel, tree status given,
 *                                                                                    input 0 dense / 1 strided / 2 colmap, sub-signal (WxSub)
 *    12  L1TILE     k_level1_tile, K = 1                                             nodes per signal, src_stride != node length, dst_stride != node length,
 *                                                                                    0, 0 (unused; the pinned rows keep their layout)
 *    13  LEVEL      k_fwd1d_level / k_inv1d_level, K = 1                             tree status given, packet-table stride
 *    14  GATHER     k_gather_leaves1d, K = 0, always recorded with inverse = 1: iwpd along a tree under mode 1 and getbasiscoef, F = 0
 *                                                                                    slices k, positions per block
 *    15  TAIL       wx_dwt_tail, the lane-local deepest levels of a pyramid          tail levels, threshold in thr
 *    16  ITAIL      wx_idwt_tail                                                     tail levels, threshold in thr
 *    17  THRFUSED   wx_dev_iwpt1d_thresh: ONE row for the call, followed by the LATTREE or FUSED row of the kernel that took it
 *                                                                                    th_kind, one threshold per signal, head given, row_lo > 0
 *    18  THRCOPY    wx_dev_threshold_copy, K = 0                                     th_kind, one threshold per signal, 0, row_lo > 0
 * _end, _dropped and the WX_EARG cases are those of wx_debug_swt1d_trace_end / _dropped. */
#define WX_DWT1D_TRACE_FIELDS 16
#define WX_DWT1D_TRACE_MAX (1 << 16)
void wx_debug_dwt1d_trace_begin(void);
int wx_debug_dwt1d_trace_end(int32_t *out, int cap);
int64_t wx_debug_dwt1d_trace_dropped(void);

/* The schedule of the 1-D redundant inverse (wx_swt_inv_plan, the function wx_swt1d's caller runs) under the current dispatch mode;
 * needs no device.  layout 0 / 1 / 2 = dwt / wpt / wpd container, sm < 0 = average based, haar6 = the caller's wx_haar_swpt6_ok.
 * out receives from, to, R, OPT of every pass (4 * L values at most; OPT = 0 marks the Haar register pass, -1 the lane-local one);
 * returns the number of passes, or WX_EARG (-2) for n < 1, L outside 0..24 (wpt: 2^L > n), F < 2, another layout or element size. */
int wx_debug_swt_inv_plan(int layout, int L, int F, int64_t sm, int64_t n, int elem_size, int has_tree, int haar6, int32_t *out);

/* The bit layout the per-signal-tree kernel reads (csrc/wx_tree_bits.h), by the host routine that packs host tree matrices: tree =
 * n - 1 bytes (any non-zero byte = decomposed), words receives max(n / 32, 1) words with the bits past node n - 1 zero.  Needs no
 * device.  Returns the number of words, or WX_EARG (-2) for a NULL pointer or n < 2. */
int wx_debug_pack_tree1d(const uint8_t *tree, int64_t n, uint32_t *words);

/* The number of chunks every class's signals are split into by the LDB class reductions (wx_ldb.hip: wx_energy_map_*, wx_class_mean_*,
 * wx_class_var_*) over nk coefficients of N signals in nc classes, by the very function the launch code calls: one workgroup row per
 * class and chunk, chunks of at least 64 signals of the average class, classes x chunks <= 65535.  Needs no device.  Returns
 * WX_EARG (-2) for arguments those entry points refuse: nk < 1, N outside 1 .. 2^31 - 1, nc outside 2 .. 65535. */
int wx_debug_ldb_chunks(int64_t nk, int64_t N, int nc);

/* The workgroups wx_wpd_bbtrees_* launches its fused kernel with (wx_wpd_bb.hip) for `batch` signals of n samples at depth L under a
 * filter of F taps, elem_size 8 / 4 = Float64 / Float32, by the very functions the launch calls; 0 when the shape is outside the
 * kernel's window (the chunked route) or L < 1.  Needs no device. */
int wx_debug_wpd_bb_grid(int64_t n, int L, int F, int elem_size, int64_t batch);

/* The workgroups of the kernels that start from the signals of a redundant decomposition (wx_red_bb.hip), for `batch` signals of n
 * samples at depth L under a filter of F taps, elem_size 8 / 4 = Float64 / Float32, ac != 0 = the autocorrelation family (Float64 only),
 * by the very functions the launch calls; 0 when the shape is outside the kernel's window (the chunked route) or L < 1.  which: 0 = the
 * trees (wx_swpd_bbtrees_*, wx_acwpd_bbtrees_f64), 1 = the denoising (wx_denoise_swpd1d_sig_trees_*, wx_denoise_acwpd1d_sig_trees_f64,
 * wx_denoise_red_sig.hip); any other value answers 0.  Needs no device. */
int wx_debug_red_bb_grid(int64_t n, int L, int F, int elem_size, int ac, int which, int64_t batch);
#ifdef __cplusplus
}
#endif
