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
#ifdef __cplusplus
}
#endif
