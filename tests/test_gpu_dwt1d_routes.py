"""GPU parity of the 1-D decimated transforms (wpd, wpt, iwpt, iwpd, dwt / idwt of signals and the thresholded inverse behind
denoise: csrc/wx_api.hip, wx_dwt1d.hip and the launchers they call) on their launch routes.

One public call ends in one of about twenty kernel families, chosen by length, type, filter length, depth, tree shape, `x is y`,
packet-table stride and batch thresholds.  Every case here runs the public entry point on device tensors inside `wx.dwt1d_trace()`
-- the record the dispatch code writes next to each launch (csrc/wx_debug.h) -- and carries two expectations: `expect`, the route
names written by hand from the conditions in the code, and PINS[case], the full rows (route, depth, K, n, signals, extras; grids,
blocks and LDS bytes are recorded but not pinned; tools/dwt1d_pins.py regenerates them on an MI355X).  The output is compared with
the Float64 CPU oracle on the case's own values at helpers.TOL (1e-10 / 1e-5), every signal against its own largest magnitude; the
inverse is fed the oracle's coefficients and compared with the oracle's inverse and (10 x TOL) with the signal.  Inputs are white
noise with a seed per case.  Batches are the smallest the route's threshold admits plus a remainder (67 signals of 64 samples for
`batch >= 4096 / n`, 3 signals for the long ones); one case sits exactly at that threshold and one just under it.

  a. test_route_and_parity: the cases of CASES_A.  `forced` cases repeat the call under wx.set_force_generic(1), which must record
     LEVEL, GATHER and THRCOPY only and agree to 1e-13 (Float64) / TOL (Float32); `modes` cases repeat it under modes 2 (no
     register kernels) and 3 (no fold).
  b. test_grid_loops_go_round: the launchers of this path that cap their grid, with more work items than workgroups (asserted from
     the recorded grid): signals b >= 251 are copies of signal b mod 251, every output signal must be bit-identical to that of its
     original, and the first 251 are compared with the oracle.
  c. test_pins_cover_what_is_reachable: the (route, type, direction, deciding extras) keys pinned in a and b == REACHABLE, which
     is written out by hand below and never taken from a record.

Routes (csrc/wx_debug.h) and the cases that pin them:
  LATF64     Float64 full trees: _g at 64 / 512 (latg-*), _sh at 1024 / 2048 (lat-1024, lat-2048), _lo at 4096 L <= 5 (lat-4096-L3),
             the general kernel (lat-4096-L8, -L8-F12; mode 2 turns it into FUSED), the folded full-depth inverse (lat-4096-L12-F12: folded
             1, 0 under mode 3), 8192 (lat-8192-L8); on the 4096-sample nodes of long signals (lf-f64-16384-L9, lf-f64-131072-L11);
             with the stride of a packet table (wpd-f64-64, -1024, -4096: iwpd of a full tree reads slice L)
  LATWPD     wpd-f64-64, -1024, -4096, wpd-f32-128
  LATF32     f32full-128-L1 (from api_wpt1d), lf-f32-16384-L9 (4096-sample nodes), wpd-f32-128 (strided inverse)
  LATTREE    short masked kernels, every stage count: lts-f64-64-F2 .. F16, lts-f64-128 .. 512, lts-f32-*; pyramids without a tail
             cut: spyr-* (spyr-f64-512-B8 / -B7: exactly at and just under `batch >= 4096 / n`); Float32 full trees as a tree of ones: f32full-256, f32full-128-L3, iwpd of wpd-f32-256-B33; full trees above 8 taps:
             full-*-64-F12; 1024 samples and the thresholded loads: pyr-*-1024, thr-*; long pyramids with out_stride != n:
             lp-*-16384-full; the 4096-sample subtrees of long trees: lt-f64-32768-deep, lt-f64-32768-rand (depth 15: four
             subtrees of 12 levels); iwpd along a tree: wpdt-f64-64
  LAT8KT     lt-f64-8192, lt-f64-8192-rand (a random tree of depth 13)
  LANETREE   lane-f64, lane-f32; under the batch threshold (lts-f64-64-B63); 18 taps (lts-f64-64-F18); Float32 full tree where
             wx_lattice_f32 declines (f32full-128-F20)
  SMALLTREE  small-f64
  HAAR       haar-f64-1024-L2 (the lattice declines `L + SH < 6`)
  TOP        one pass: lf-*-L3, lp-f64-8192-L3, lp-f32-8192-L3; two passes: lp-f64-65536-L6, lf-f64-262144-L6, lf-f64-131072-L11; with `deep`:
             lp-*-16384-full, lt-f64-32768-*; strided input: wpd-f64-16384 (iwpd in one tiled pass)
  TOPWPD     wpd-f64-16384, wpd-f64-16384-L9
  FUSED      plain, in-place kernel or not, with a status, wpd layout, sub-signals (WxSub), colmap, strided: lts-f64-512-B7,
             f32full-256-B15, ip-*, wpd-f32-256-*, wpd-f64-16384*, wpdt-f64-64-B5, lf-f64-8192-L3 (inverse), lf-f64-262144-L6; a filter the lattice declines on long
             signals: lp-f64-16384-declined (the finisher of the long pyramid, status and stride), lf-f64-16384-declined
  L1TILE     ip-f64-16384-L3, ip-f64-32768-L3 (`x is y` keeps a long full tree from the tiled passes)
  LEVEL      non-dyadic and tiny signals (wpd-f64-24, wpd-f64-4, lvl-f32-4), `x is y` on a long tree (ip-f64-16384-tree, ip-f64-16384-L1), every
             forced repeat
  GATHER     wpdt-f64-64 under force, gbc-f64-64 (getbasiscoefall: exact)
  TAIL / ITAIL   pyr-*-1024, lp-*-16384-full, ip-f64-512-dwt; with a threshold: thr-f64-1024-tail
  THRFUSED   pyr-*-1024 inverse (head, no threshold), thr-*-1024-tree, thr-f64-1024-hard, thr-f64-1024-tail, thr-f64-128-pyr
  THRCOPY    thr-f64-64-short (then LATTREE), thr-f64-1024-full (then LATF64), thr-f64-16384-pyr (then the long pyramid)

Not reachable from the 1-D entry points (the condition is quoted from the code).  Four branches that stood in this list or beside it
have since been deleted, with their proofs in profiles/dwt1d_routes.md, "Removed as unreachable": the second long-signal block of
wx_dev_wpt1d / wx_dev_iwpt1d, the L1TILE branch of wx_dev_dwt_long / wx_dev_idwt_long, the split form of k_level1_tile that only
that branch used, and the per-level fallback of wx_dev_wpt_long_tree.  What is left:
  * the `d0 > 0` blocks of wx_dev_wpt1d / wx_dev_iwpt1d out of place: they need `!wx_fused1d_ok<T>(n, filt.F)` with a filter of
    at most 20 taps, i.e. n > 8192 (Float32 16384), where the first long-signal block applies.  In place (`x is y`) they are
    reached: ip-f64-16384-L3.
  * the Float32 full-as-tree branch of wx_dev_wpt1d (`batch >= 2 * 4096 / n`) from wptall: api_wpt1d's full_long takes the same
    shapes from `batch >= 4096 / n` on; the branch serves the column pass of the 2-D transforms.  Its inverse twin is reached by
    iwpd (wpd-f32-256-B33).
  * `Ld - tail >= 2` false in api_wpt1d: tail > 0 wants n >= 128 and Ld - tail = log2(n) - 6, so only n = 128, which small_pyr takes
    first; through api_iwpt1d_thresh it is reached (thr-f64-128-pyr).  `wx_fused1d_ok || (allow_long && wx_dwt_long_ok)` false
    wants a length beyond 2^24.
  * wpd with `x is y`: the shapes (n, B) and (n, L + 1, B) differ.
Reachable and not pinned here: nothing that REACHABLE names (test c).  Of the larger shapes only batches beyond 2^31 - 1 signals
(the launchers' `batch > 0x7fffffff` declines) are left out, for their size.
Grid loops: LEVEL and GATHER (wx_grid_for: 4096 workgroups), FUSED (wx_fused_grid: at most 4096) and TOP (wx_top_grid: at most
8 persistent workgroups per CU) are wrapped in part b; the lane
tree, the small tree (`dim3((unsigned)wgs)`), TAIL / ITAIL (`dim3((unsigned)((batch + 63) / 64))`), L1TILE and the lattice kernels
launch one workgroup per item or group of items (no cap)."""
import numpy as np
import pytest

from helpers import TOL

gpu = pytest.mark.gpu
F64, F32 = np.float64, np.float32
WF = {2: "haar", 4: "db2", 6: "db3", 8: "db4", 10: "db5", 12: "db6", 14: "db7", 16: "db8", 18: "db9", 20: "db10"}
P = 251                                                   # part b: signals b >= P are copies of signal b mod P
T3 = ("nodes", [1, 2, 5])                                 # depth 3, neither full nor a pyramid: the root, its left child, that one's right child
GENERIC = {"LEVEL", "GATHER", "THRCOPY"}


class Case:
    """op: "wpt" (arg = depth of a full tree, or a tree spec ("dwt", L) / ("nodes", [heap indices of the decomposed nodes])),
    "dwt" (arg = depth of the pyramid, through dwtall / idwtall), "wpd" (arg = depth; the inverse is iwpdall along `iarg`, default
    the full tree of that depth), "gbc" (getbasiscoefall along the tree `arg` of the oracle's table of depth 3), "thr"
    (denoising._iwpt_thresh along the tree `arg`; th, per, row_lo).  expect = (forward route names, inverse route names), None
    where the direction does not exist.  inplace: one signal through wpt_ / iwpt_ with y is x.  tol: where an existing test holds
    a tighter figure than helpers.TOL for the same kernel (the constants below name the test).  qmf: a member of tests/qmf_family.py
    instead of the table wavelet of F taps.  A tree spec may also be ("rand", p, seed): helpers.random_tree_1d."""

    def __init__(self, cid, op, dtype, n, arg, F, B, expect, forced=False, inplace=False, modes=None, iarg=None, th="hard", per=False,
                 row_lo=0, tol=None, qmf=None):
        self.id, self.op, self.dtype, self.n, self.arg, self.F, self.B, self.expect = cid, op, dtype, n, arg, F, B, expect
        self.forced, self.inplace, self.modes, self.iarg, self.th, self.per, self.row_lo = forced, inplace, modes, iarg, th, per, row_lo
        self.tol, self.qmf = tol, qmf


def _t(dtype):
    return "f64" if dtype == F64 else "f32"


LT = ("LATTREE",)
# Tighter figures that existing tests hold for the same kernels (all of them on the largest magnitude of the whole batch; here
# every signal is held to the figure against its own):
T_LAT = 1e-12     # test_gpu_lattice.py: test_lattice_matches_oracle_every_depth (4096 samples), the short-lattice tests (64 .. 2048:
#                   wptall / iwptall / wpdall / iwpdall of full trees)
T_8K = 1e-12      # test_gpu_lattice_8k.py: full trees, trees and pyramids of 8192 samples
T_HAAR = 1e-13    # test_gpu_dwt1d.py: test_haar_walsh_hadamard_path
T_PYR = 1e-12     # test_gpu_dwt1d.py: test_pyramid_deep_levels_in_the_registers_of_a_lane (dwtall of 128 / 1024 / 4096 samples)


def _rand_tree(n, p, seed):
    from helpers import random_tree_1d
    return np.asarray(random_tree_1d(n, np.random.default_rng(seed), p), dtype=bool)


def _tree_depth(t):
    return int(np.floor(np.log2(np.nonzero(t)[0].max() + 1))) + 1


def _split_at(t, d):
    """decomposed nodes of depth d (a random tree's node is decomposed only under a decomposed parent)"""
    return int(t[(1 << d) - 1:(1 << (d + 1)) - 1].sum())


# random trees of the long-tree path, deep enough for 12-level subtrees under the 4096-sample nodes
RT8K, RT32K = ("rand", 0.85, 2), ("rand", 0.8, 3)
assert _tree_depth(_rand_tree(8192, *RT8K[1:])) == 13 and _split_at(_rand_tree(8192, *RT8K[1:]), 1) == 2
assert _tree_depth(_rand_tree(32768, *RT32K[1:])) == 15 and _split_at(_rand_tree(32768, *RT32K[1:]), 3) == 4
CASES_A = [
    # ---- short signals, api_wpt1d ------------------------------------------------------------------------------------------------
    # one lane per signal: `small` and the masked lattice declines `batch < per`
    Case("lane-f64", "wpt", F64, 64, T3, 8, 5, (("LANETREE",), ("LANETREE",)), forced=True),
    Case("lane-f32", "wpt", F32, 128, T3, 8, 5, (("LANETREE",), ("LANETREE",))),
    Case("small-f64", "wpt", F64, 256, T3, 8, 5, (("SMALLTREE",), ("SMALLTREE",)), forced=True),
    # lat_short: `batch >= 4096 / n`, a tree that is not full, x is not y; stages 1, 2, 4, 6, 8
    Case("lts-f64-64-F2", "wpt", F64, 64, T3, 2, 67, (LT, LT)),
    Case("lts-f64-64-F4", "wpt", F64, 64, T3, 4, 67, (LT, LT)),
    Case("lts-f64-64-F8", "wpt", F64, 64, T3, 8, 67, (LT, LT), forced=True),
    Case("lts-f64-64-F12", "wpt", F64, 64, T3, 12, 67, (LT, LT)),
    Case("lts-f64-64-F16", "wpt", F64, 64, T3, 16, 67, (LT, LT)),
    Case("lts-f64-128", "wpt", F64, 128, T3, 8, 35, (LT, LT)),
    Case("lts-f64-256", "wpt", F64, 256, T3, 8, 19, (LT, LT)),
    Case("lts-f64-512", "wpt", F64, 512, T3, 8, 11, (LT, LT)),
    Case("lts-f32-64-F8", "wpt", F32, 64, T3, 8, 67, (LT, LT), forced=True),
    Case("lts-f32-64-F16", "wpt", F32, 64, T3, 16, 67, (LT, LT)),
    Case("lts-f32-512", "wpt", F32, 512, T3, 8, 11, (LT, LT)),
    # `filt.F <= 16` (wx_lattice_trees_short): 18 taps leave lat_short; `small` holds, the lane tree takes it
    Case("lts-f64-64-F18", "wpt", F64, 64, T3, 18, 67, (("LANETREE",), ("LANETREE",))),
    # just under the batch threshold: 63 < 4096 / 64 -> the lane tree; 7 < 4096 / 512 and no small kernel at 512 -> the fused kernel
    Case("lts-f64-64-B64", "wpt", F64, 64, T3, 8, 64, (LT, LT)),                             # exactly at it
    Case("lts-f64-64-B63", "wpt", F64, 64, T3, 8, 63, (("LANETREE",), ("LANETREE",))),
    Case("lts-f64-512-B7", "wpt", F64, 512, T3, 8, 7, (("FUSED",), ("FUSED",)), forced=True),
    # pyramids of the same shapes: small_pyr, no tail cut
    Case("spyr-f64-64", "dwt", F64, 64, 6, 8, 67, (LT, LT)),
    Case("spyr-f64-512", "dwt", F64, 512, 9, 8, 11, (LT, LT)),
    # lat_short decides for pyramids of 256 / 512 samples (`small` keeps shorter trees on the same kernels either way): exactly at
    # `batch >= 4096 / n` the masked kernel takes the whole pyramid; one signal fewer, the tail is cut and the fused kernels run
    Case("spyr-f64-512-B8", "dwt", F64, 512, 9, 8, 8, (LT, LT)),
    Case("spyr-f64-512-B7", "dwt", F64, 512, 9, 8, 7, (("FUSED", "TAIL"), ("ITAIL", "THRFUSED", "FUSED"))),
    Case("spyr-f32-64", "dwt", F32, 64, 6, 8, 67, (LT, LT)),
    # Float32 full trees
    Case("f32full-256", "wpt", F32, 256, 3, 8, 33, (LT, LT), forced=True),                   # a tree of ones (full_long)
    Case("f32full-128-L3", "wpt", F32, 128, 3, 8, 35, (LT, LT)),                             # `n == 128 && tr.Leff >= 2`: a tree of ones too
    Case("f32full-256-B15", "wpt", F32, 256, 3, 8, 15, (("FUSED",), ("FUSED",))),            # 15 < 4096 / 256
    Case("f32full-128-L1", "wpt", F32, 128, 1, 8, 35, (("LATF32",), ("LATF32",))),           # `n == 128 && tr.Leff >= 2` fails
    Case("f32full-128-F20", "wpt", F32, 128, 3, 20, 35, (("LANETREE",), ("LANETREE",))),     # wx_lattice_f32 declines 20 taps
    # full trees above 8 taps on 64 .. 512 samples: full_long
    Case("full-f64-64-F12", "wpt", F64, 64, 3, 12, 67, (LT, LT)),
    Case("full-f32-64-F12", "wpt", F32, 64, 3, 12, 67, (LT, LT)),
    # Float64 full trees on the lattice
    Case("latg-f64-64", "wpt", F64, 64, 3, 8, 67, (("LATF64",), ("LATF64",)), forced=True, tol=T_LAT),
    Case("latg-f64-512", "wpt", F64, 512, 3, 8, 11, (("LATF64",), ("LATF64",)), tol=T_LAT),
    Case("lat-1024", "wpt", F64, 1024, 4, 8, 5, (("LATF64",), ("LATF64",)), tol=T_LAT),
    Case("lat-2048", "wpt", F64, 2048, 5, 8, 3, (("LATF64",), ("LATF64",)), tol=T_LAT),
    Case("lat-4096-L3", "wpt", F64, 4096, 3, 8, 3, (("LATF64",), ("LATF64",)), tol=T_LAT),
    Case("lat-4096-L8", "wpt", F64, 4096, 8, 8, 3, (("LATF64",), ("LATF64",)), forced=True, modes=(2,), tol=T_LAT),
    Case("lat-4096-L8-F12", "wpt", F64, 4096, 8, 12, 3, (("LATF64",), ("LATF64",)), tol=T_LAT),  # six stages below full depth: no fold
    Case("lat-4096-L12-F12", "wpt", F64, 4096, 12, 12, 3, (("LATF64",), ("LATF64",)), modes=(3,), tol=T_LAT),
    Case("lat-8192-L8", "wpt", F64, 8192, 8, 8, 3, (("LATF64",), ("LATF64",)), tol=T_8K),
    # Haar at a depth the lattice declines (1024 samples: `L + SH < 6` with SH = 2)
    Case("haar-f64-1024-L2", "wpt", F64, 1024, 2, 2, 5, (("HAAR",), ("HAAR",)), forced=True, tol=T_HAAR),
    # y is x: every register route wants dx != dy
    Case("ip-f64-64-tree", "wpt", F64, 64, T3, 8, 1, (("FUSED",), ("FUSED",)), inplace=True),
    Case("ip-f64-512-full", "wpt", F64, 512, 3, 8, 1, (("FUSED",), ("FUSED",)), inplace=True),
    Case("ip-f64-512-dwt", "wpt", F64, 512, ("dwt", 9), 8, 1, (("FUSED", "TAIL"), ("ITAIL", "THRFUSED", "FUSED")), inplace=True),
    # ---- pyramids with the lane-local tail ---------------------------------------------------------------------------------------
    Case("pyr-f64-1024", "dwt", F64, 1024, 10, 8, 5, (("LATTREE", "TAIL"), ("ITAIL", "THRFUSED", "LATTREE")), forced=True, tol=T_PYR),
    Case("pyr-f32-1024", "dwt", F32, 1024, 10, 8, 5, (("LATTREE", "TAIL"), ("ITAIL", "THRFUSED", "FUSED"))),
    # ---- long pyramids (wx_dev_dwt_long / wx_dev_idwt_long) ----------------------------------------------------------------------
    Case("lp-f64-8192-L3", "dwt", F64, 8192, 3, 8, 3, (("TOP",), ("TOP",)), tol=T_8K),  # Lp <= 4: top passes only
    Case("lp-f32-8192-L3", "dwt", F32, 8192, 3, 8, 3, (("TOP",), ("TOP",))),
    Case("lp-f64-65536-L6", "dwt", F64, 65536, 6, 8, 3, (("TOP", "TOP"), ("TOP", "TOP"))),   # Lp - dl <= 2 && Lp <= 8 && (n >> 4) >= 4096
    Case("lp-f64-16384-full", "dwt", F64, 16384, 14, 8, 3, (("TOP", "LATTREE", "TAIL"), ("ITAIL", "LATTREE", "TOP"))),
    Case("lp-f32-16384-full", "dwt", F32, 16384, 14, 8, 3, (("TOP", "LATTREE", "TAIL"), ("ITAIL", "LATTREE", "TOP"))),
    # a filter the lattice declines (pad_front: db2 behind two zero taps): wx_dwt_long_plan falls to the fused kernel at 8192 samples,
    # which finishes the pyramid under the cut tree's status, reading / writing with the long signal's stride
    Case("lp-f64-16384-declined", "dwt", F64, 16384, 14, 6, 3, (("TOP", "FUSED", "TAIL"), ("ITAIL", "FUSED", "TOP")), qmf="pad_front"),
    # ---- full trees on long signals ----------------------------------------------------------------------------------------------
    # at most four levels: one tiled pass; the inverse only where the fused kernel does not take the whole signal (`d0 >= 1`)
    Case("lf-f64-16384-L3", "wpt", F64, 16384, 3, 8, 3, (("TOP",), ("TOP",)), forced=True),
    Case("lf-f64-8192-L3", "wpt", F64, 8192, 3, 8, 3, (("TOP",), ("FUSED",))),
    Case("lf-f32-16384-L3", "wpt", F32, 16384, 3, 8, 3, (("TOP",), ("FUSED",))),
    Case("lf-f64-262144-L6", "wpt", F64, 262144, 6, 8, 3, (("TOP", "TOP", "FUSED"), ("FUSED", "TOP", "TOP"))),   # d0 = 5: two passes
    Case("lf-f64-16384-L9", "wpt", F64, 16384, 9, 8, 3, (("TOP", "LATF64"), ("LATF64", "TOP")), tol=T_LAT),  # L - dl >= 6
    Case("lf-f32-16384-L9", "wpt", F32, 16384, 9, 8, 3, (("TOP", "LATF32"), ("LATF32", "TOP"))),
    Case("lf-f64-16384-declined", "wpt", F64, 16384, 9, 6, 3, (("TOP", "FUSED"), ("FUSED", "TOP")), qmf="pad_front"),   # `lat` fails: FUSED at n2 = 8192
    Case("lf-f64-131072-L11", "wpt", F64, 131072, 11, 8, 3, (("TOP", "TOP", "LATF64"), ("LATF64", "TOP", "TOP")), tol=T_LAT),
    # in place the tiled passes decline (`x != y`): the d0 > 0 block, one tiled level and the fused kernel on sub-signals
    Case("ip-f64-16384-L3", "wpt", F64, 16384, 3, 8, 1, (("L1TILE", "FUSED"), ("FUSED", "L1TILE")), inplace=True),
    # ---- other trees on long signals (wx_dev_wpt_long_tree) ----------------------------------------------------------------------
    Case("lt-f64-8192", "wpt", F64, 8192, T3, 8, 3, (("LAT8KT",), ("LAT8KT",)), tol=T_8K),
    # random trees of full depth: both children of the root split (8192), four of the eight 4096-sample nodes split (32768)
    Case("lt-f64-8192-rand", "wpt", F64, 8192, RT8K, 8, 3, (("LAT8KT",), ("LAT8KT",)), tol=T_8K),
    Case("lt-f64-32768-rand", "wpt", F64, 32768, RT32K, 8, 3, (("TOP",) + LT * 4, LT * 4 + ("TOP",))),
    Case("lt-f64-32768-top", "wpt", F64, 32768, ("nodes", [1, 3, 6]), 8, 3, (("TOP",), ("TOP",))),          # depth <= dl: the tiles suffice
    Case("lt-f64-32768-deep", "wpt", F64, 32768, ("nodes", [1, 3, 6, 12]), 8, 3, (("TOP", "LATTREE"), ("LATTREE", "TOP"))),   # the deep branch is a detail
    Case("lt-f32-16384-deep", "wpt", F32, 16384, ("nodes", [1, 3, 6]), 8, 3, (("TOP", "LATTREE"), ("LATTREE", "TOP"))),
    # (two such levels and a single per-level pass: in place the first level reads a staged copy -- it used to read the array it wrote)
    Case("ip-f64-32768-L3", "wpt", F64, 32768, 3, 8, 1, (("L1TILE", "L1TILE", "FUSED"), ("FUSED", "L1TILE", "L1TILE")), inplace=True),
    Case("ip-f64-16384-L1", "wpt", F64, 16384, 1, 8, 1, (("LEVEL",), ("LEVEL",)), inplace=True),
    Case("ip-f32-32768-tree", "wpt", F32, 32768, T3, 8, 1, (("LEVEL",) * 3, ("LEVEL",) * 3), inplace=True),  # the same in Float32, past its fused kernel
    Case("ip-f64-16384-tree", "wpt", F64, 16384, T3, 8, 1, (("LEVEL",) * 3, ("LEVEL",) * 3), inplace=True),  # longt wants dx != dy
    # ---- wpd / iwpd --------------------------------------------------------------------------------------------------------------
    Case("wpd-f64-64", "wpd", F64, 64, 3, 8, 67, (("LATWPD",), ("LATF64",)), forced=True, tol=T_LAT),
    Case("wpd-f64-1024", "wpd", F64, 1024, 4, 8, 5, (("LATWPD",), ("LATF64",)), tol=T_LAT),
    Case("wpd-f64-4096", "wpd", F64, 4096, 3, 8, 3, (("LATWPD",), ("LATF64",)), tol=T_LAT),
    Case("wpd-f32-128", "wpd", F32, 128, 3, 8, 35, (("LATWPD",), ("LATF32",))),
    Case("wpd-f32-256-B33", "wpd", F32, 256, 3, 8, 33, (("FUSED",), ("LATTREE",))),          # iwpd: the tree of ones, `batch >= 2 * 4096 / n`
    Case("wpd-f32-256-B19", "wpd", F32, 256, 3, 8, 19, (("FUSED",), ("FUSED",))),
    Case("wpd-f64-16384", "wpd", F64, 16384, 3, 8, 3, (("TOPWPD", "FUSED"), ("TOP",))),      # iwpd: `L <= 4 && is > n && !(is & 1)`
    Case("wpd-f64-16384-L9", "wpd", F64, 16384, 9, 8, 3, (("TOPWPD", "FUSED"), ("LATF64", "TOP")), tol=T_LAT),  # iwpd: the densifying copy first
    Case("wpd-f64-24", "wpd", F64, 24, 2, 8, 5, (("LEVEL",) * 2, None)),                     # iwpd wants a dyadic length
    Case("wpd-f64-4", "wpd", F64, 4, 2, 4, 5, (("LEVEL",) * 2, ("LEVEL",) * 2)),             # below wx_fused1d_ok
    Case("lvl-f32-4", "wpt", F32, 4, 2, 4, 5, (("LEVEL",) * 2, ("LEVEL",) * 2)),             # below every fused and register kernel
    Case("wpdt-f64-64", "wpd", F64, 64, 3, 8, 67, (("LATWPD",), ("LATTREE",)), iarg=T3, forced=True),       # col_stride
    Case("wpdt-f64-64-B5", "wpd", F64, 64, 3, 8, 5, (("FUSED",), ("FUSED",)), iarg=T3),      # `batch < per`: the fused kernel with colmap
    Case("gbc-f64-64", "gbc", F64, 64, T3, 8, 5, (None, ("GATHER",))),
    # ---- the thresholded inverse -------------------------------------------------------------------------------------------------
    Case("thr-f64-64-short", "thr", F64, 64, ("dwt", 6), 8, 67, (None, ("THRCOPY", "LATTREE")), th="hard"),
    Case("thr-f64-64-short-soft", "thr", F64, 64, T3, 8, 67, (None, ("THRCOPY", "LATTREE")), th="soft", per=True, row_lo=8),
    Case("thr-f64-1024-tree", "thr", F64, 1024, T3, 8, 5, (None, ("THRFUSED", "LATTREE")), th="soft", per=True, row_lo=128),
    Case("thr-f64-1024-hard", "thr", F64, 1024, T3, 8, 5, (None, ("THRFUSED", "LATTREE")), th="hard"),
    Case("thr-f32-1024-tree", "thr", F32, 1024, T3, 8, 5, (None, ("THRFUSED", "FUSED")), th="hard"),
    Case("thr-f64-1024-tail", "thr", F64, 1024, ("dwt", 10), 8, 5, (None, ("ITAIL", "THRFUSED", "LATTREE")), th="soft", per=True, row_lo=1),
    Case("thr-f64-128-pyr", "thr", F64, 128, ("dwt", 2), 8, 5, (None, ("THRFUSED", "FUSED")), th="hard", per=True),   # `Ld - tail >= 2` fails
    Case("thr-f64-1024-full", "thr", F64, 1024, ("nodes", list(range(1, 16))), 8, 5, (None, ("THRCOPY", "LATF64")), th="soft", row_lo=64, tol=T_LAT),
    Case("thr-f64-1024-full-hard", "thr", F64, 1024, ("nodes", list(range(1, 16))), 8, 5, (None, ("THRCOPY", "LATF64")), th="hard", per=True, tol=T_LAT),
    Case("thr-f64-16384-pyr-soft", "thr", F64, 16384, ("dwt", 14), 8, 3, (None, ("THRCOPY", "LATTREE", "TOP")), th="soft", row_lo=64),
    Case("thr-f32-1024-tree-soft", "thr", F32, 1024, T3, 8, 5, (None, ("THRFUSED", "FUSED")), th="soft", per=True, row_lo=128),
    Case("thr-f64-1024-tail-hard", "thr", F64, 1024, ("dwt", 10), 8, 5, (None, ("ITAIL", "THRFUSED", "LATTREE")), th="hard"),
    Case("thr-f64-16384-pyr", "thr", F64, 16384, ("dwt", 14), 8, 3, (None, ("THRCOPY", "LATTREE", "TOP")), th="hard", per=True, row_lo=256),
]
CASE_BY_ID = {c.id: c for c in CASES_A}
assert len(CASE_BY_ID) == len(CASES_A)

# >>> PINS
PINS = {
    "lane-f64": ([('LANETREE', 0, 3, 64, 5)],
        [('LANETREE', 3, 3, 64, 5)]),
    "lane-f32": ([('LANETREE', 0, 3, 128, 5)],
        [('LANETREE', 3, 3, 128, 5)]),
    "small-f64": ([('SMALLTREE', 0, 3, 256, 5, 1)],
        [('SMALLTREE', 3, 3, 256, 5, 1)]),
    "lts-f64-64-F2": ([('LATTREE', 0, 3, 64, 67)],
        [('LATTREE', 3, 3, 64, 67)]),
    "lts-f64-64-F4": ([('LATTREE', 0, 3, 64, 67)],
        [('LATTREE', 3, 3, 64, 67)]),
    "lts-f64-64-F8": ([('LATTREE', 0, 3, 64, 67)],
        [('LATTREE', 3, 3, 64, 67)]),
    "lts-f64-64-F12": ([('LATTREE', 0, 3, 64, 67)],
        [('LATTREE', 3, 3, 64, 67)]),
    "lts-f64-64-F16": ([('LATTREE', 0, 3, 64, 67)],
        [('LATTREE', 3, 3, 64, 67)]),
    "lts-f64-128": ([('LATTREE', 0, 3, 128, 35)],
        [('LATTREE', 3, 3, 128, 35)]),
    "lts-f64-256": ([('LATTREE', 0, 3, 256, 19)],
        [('LATTREE', 3, 3, 256, 19)]),
    "lts-f64-512": ([('LATTREE', 0, 3, 512, 11)],
        [('LATTREE', 3, 3, 512, 11)]),
    "lts-f32-64-F8": ([('LATTREE', 0, 3, 64, 67)],
        [('LATTREE', 3, 3, 64, 67)]),
    "lts-f32-64-F16": ([('LATTREE', 0, 3, 64, 67)],
        [('LATTREE', 3, 3, 64, 67)]),
    "lts-f32-512": ([('LATTREE', 0, 3, 512, 11)],
        [('LATTREE', 3, 3, 512, 11)]),
    "lts-f64-64-F18": ([('LANETREE', 0, 3, 64, 67)],
        [('LANETREE', 3, 3, 64, 67)]),
    "lts-f64-64-B64": ([('LATTREE', 0, 3, 64, 64)],
        [('LATTREE', 3, 3, 64, 64)]),
    "lts-f64-64-B63": ([('LANETREE', 0, 3, 64, 63)],
        [('LANETREE', 3, 3, 64, 63)]),
    "lts-f64-512-B7": ([('FUSED', 0, 3, 512, 7, 0, 1, 1)],
        [('FUSED', 3, 3, 512, 7, 0, 0, 1)]),
    "spyr-f64-64": ([('LATTREE', 0, 6, 64, 67)],
        [('LATTREE', 6, 6, 64, 67)]),
    "spyr-f64-512": ([('LATTREE', 0, 9, 512, 11)],
        [('LATTREE', 9, 9, 512, 11)]),
    "spyr-f64-512-B8": ([('LATTREE', 0, 9, 512, 8)],
        [('LATTREE', 9, 9, 512, 8)]),
    "spyr-f64-512-B7": ([('FUSED', 0, 3, 512, 7, 0, 1, 1), ('TAIL', 3, 6, 512, 7, 6)],
        [('ITAIL', 9, 6, 512, 7, 6), ('THRFUSED', 3, 3, 512, 7, 0, 0, 1), ('FUSED', 3, 3, 512, 7, 0, 0, 1)]),
    "spyr-f32-64": ([('LATTREE', 0, 6, 64, 67)],
        [('LATTREE', 6, 6, 64, 67)]),
    "f32full-256": ([('LATTREE', 0, 3, 256, 33, 1)],
        [('LATTREE', 3, 3, 256, 33, 1)]),
    "f32full-128-L3": ([('LATTREE', 0, 3, 128, 35, 1)],
        [('LATTREE', 3, 3, 128, 35, 1)]),
    "f32full-256-B15": ([('FUSED', 0, 3, 256, 15, 0, 1)],
        [('FUSED', 3, 3, 256, 15)]),
    "f32full-128-L1": ([('LATF32', 0, 1, 128, 35, 4)],
        [('LATF32', 1, 1, 128, 35, 4)]),
    "f32full-128-F20": ([('LANETREE', 0, 3, 128, 35, 1)],
        [('LANETREE', 3, 3, 128, 35, 1)]),
    "full-f64-64-F12": ([('LATTREE', 0, 3, 64, 67, 1)],
        [('LATTREE', 3, 3, 64, 67, 1)]),
    "full-f32-64-F12": ([('LATTREE', 0, 3, 64, 67, 1)],
        [('LATTREE', 3, 3, 64, 67, 1)]),
    "latg-f64-64": ([('LATF64', 0, 3, 64, 67, 4)],
        [('LATF64', 3, 3, 64, 67, 4)]),
    "latg-f64-512": ([('LATF64', 0, 3, 512, 11, 4)],
        [('LATF64', 3, 3, 512, 11, 4)]),
    "lat-1024": ([('LATF64', 0, 4, 1024, 5, 4)],
        [('LATF64', 4, 4, 1024, 5, 4)]),
    "lat-2048": ([('LATF64', 0, 5, 2048, 3, 4)],
        [('LATF64', 5, 5, 2048, 3, 4)]),
    "lat-4096-L3": ([('LATF64', 0, 3, 4096, 3, 4)],
        [('LATF64', 3, 3, 4096, 3, 4)]),
    "lat-4096-L8": ([('LATF64', 0, 8, 4096, 3, 4)],
        [('LATF64', 8, 8, 4096, 3, 4)]),
    "lat-4096-L8-F12": ([('LATF64', 0, 8, 4096, 3, 6)],
        [('LATF64', 8, 8, 4096, 3, 6)]),
    "lat-4096-L12-F12": ([('LATF64', 0, 12, 4096, 3, 6)],
        [('LATF64', 12, 12, 4096, 3, 6, 1)]),
    "lat-8192-L8": ([('LATF64', 0, 8, 8192, 3, 4)],
        [('LATF64', 8, 8, 8192, 3, 4)]),
    "haar-f64-1024-L2": ([('HAAR', 0, 2, 1024, 5)],
        [('HAAR', 2, 2, 1024, 5)]),
    "ip-f64-64-tree": ([('FUSED', 0, 3, 64, 1, 0, 1, 1)],
        [('FUSED', 3, 3, 64, 1, 0, 0, 1)]),
    "ip-f64-512-full": ([('FUSED', 0, 3, 512, 1, 0, 1)],
        [('FUSED', 3, 3, 512, 1)]),
    "ip-f64-512-dwt": ([('FUSED', 0, 3, 512, 1, 0, 1, 1), ('TAIL', 3, 6, 512, 1, 6)],
        [('ITAIL', 9, 6, 512, 1, 6), ('THRFUSED', 3, 3, 512, 1, 0, 0, 1), ('FUSED', 3, 3, 512, 1, 0, 0, 1)]),
    "pyr-f64-1024": ([('LATTREE', 0, 4, 1024, 5), ('TAIL', 4, 6, 1024, 5, 6)],
        [('ITAIL', 10, 6, 1024, 5, 6), ('THRFUSED', 4, 4, 1024, 5, 0, 0, 1), ('LATTREE', 4, 4, 1024, 5, 0, 0, 1)]),
    "pyr-f32-1024": ([('LATTREE', 0, 4, 1024, 5), ('TAIL', 4, 6, 1024, 5, 6)],
        [('ITAIL', 10, 6, 1024, 5, 6), ('THRFUSED', 4, 4, 1024, 5, 0, 0, 1), ('FUSED', 4, 4, 1024, 5, 0, 0, 1)]),
    "lp-f64-8192-L3": ([('TOP', 0, 3, 8192, 3, 3, 11, 1)],
        [('TOP', 3, 3, 8192, 3, 3, 11, 1)]),
    "lp-f32-8192-L3": ([('TOP', 0, 3, 8192, 3, 3, 11, 1)],
        [('TOP', 3, 3, 8192, 3, 3, 11, 1)]),
    "lp-f64-65536-L6": ([('TOP', 0, 4, 65536, 3, 4, 139, 1, 0, 1), ('TOP', 4, 2, 4096, 3, 2, 3, 1, 1)],
        [('TOP', 6, 2, 4096, 3, 2, 3, 1, 1), ('TOP', 4, 4, 65536, 3, 4, 139, 1, 0, 1)]),
    "lp-f64-16384-full": ([('TOP', 0, 2, 16384, 3, 2, 3, 1, 0, 1), ('LATTREE', 2, 6, 4096, 3, 0, 0, 0, 1, 1), ('TAIL', 8, 6, 16384, 3, 6)],
        [('ITAIL', 14, 6, 16384, 3, 6), ('LATTREE', 8, 6, 4096, 3, 0, 0, 1, 1, 1), ('TOP', 2, 2, 16384, 3, 2, 3, 1, 0, 1)]),
    "lp-f32-16384-full": ([('TOP', 0, 2, 16384, 3, 2, 3, 1, 0, 1), ('LATTREE', 2, 6, 4096, 3, 0, 0, 0, 1, 1), ('TAIL', 8, 6, 16384, 3, 6)],
        [('ITAIL', 14, 6, 16384, 3, 6), ('LATTREE', 8, 6, 4096, 3, 0, 0, 1, 1, 1), ('TOP', 2, 2, 16384, 3, 2, 3, 1, 0, 1)]),
    "lp-f64-16384-declined": ([('TOP', 0, 1, 16384, 3, 1, 1, 1, 0, 1), ('FUSED', 1, 7, 8192, 3, 0, 1, 1, 1), ('TAIL', 8, 6, 16384, 3, 6)],
        [('ITAIL', 14, 6, 16384, 3, 6), ('FUSED', 8, 7, 8192, 3, 0, 0, 1, 1), ('TOP', 1, 1, 16384, 3, 1, 1, 1, 0, 1)]),
    "lf-f64-16384-L3": ([('TOP', 0, 3, 16384, 3, 3, -1)],
        [('TOP', 3, 3, 16384, 3, 3, -1)]),
    "lf-f64-8192-L3": ([('TOP', 0, 3, 8192, 3, 3, -1)],
        [('FUSED', 3, 3, 8192, 3)]),
    "lf-f32-16384-L3": ([('TOP', 0, 3, 16384, 3, 3, -1)],
        [('FUSED', 3, 3, 16384, 3)]),
    "lf-f64-262144-L6": ([('TOP', 0, 4, 262144, 3, 4, -1), ('TOP', 4, 1, 16384, 48, 1, -1), ('FUSED', 5, 1, 8192, 96, 0, 1)],
        [('FUSED', 6, 1, 8192, 96), ('TOP', 5, 1, 16384, 48, 1, -1), ('TOP', 4, 4, 262144, 3, 4, -1)]),
    "lf-f64-16384-L9": ([('TOP', 0, 2, 16384, 3, 2, -1), ('LATF64', 2, 7, 4096, 12, 4)],
        [('LATF64', 9, 7, 4096, 12, 4), ('TOP', 2, 2, 16384, 3, 2, -1)]),
    "lf-f32-16384-L9": ([('TOP', 0, 2, 16384, 3, 2, -1), ('LATF32', 2, 7, 4096, 12, 4)],
        [('LATF32', 9, 7, 4096, 12, 4), ('TOP', 2, 2, 16384, 3, 2, -1)]),
    "lf-f64-16384-declined": ([('TOP', 0, 1, 16384, 3, 1, -1), ('FUSED', 1, 8, 8192, 6, 0, 1)],
        [('FUSED', 9, 8, 8192, 6), ('TOP', 1, 1, 16384, 3, 1, -1)]),
    "lf-f64-131072-L11": ([('TOP', 0, 4, 131072, 3, 4, -1), ('TOP', 4, 1, 8192, 48, 1, -1), ('LATF64', 5, 6, 4096, 96, 4)],
        [('LATF64', 11, 6, 4096, 96, 4), ('TOP', 5, 1, 8192, 48, 1, -1), ('TOP', 4, 4, 131072, 3, 4, -1)]),
    "ip-f64-16384-L3": ([('L1TILE', 0, 1, 16384, 1, 1), ('FUSED', 1, 2, 8192, 2, 0, 1)],
        [('FUSED', 3, 2, 8192, 2), ('L1TILE', 1, 1, 16384, 1, 1)]),
    "lt-f64-8192": ([('LAT8KT', 0, 3, 8192, 3, 2)],
        [('LAT8KT', 3, 3, 8192, 3, 2)]),
    "lt-f64-8192-rand": ([('LAT8KT', 0, 13, 8192, 3, 12, 12)],
        [('LAT8KT', 13, 13, 8192, 3, 12, 12)]),
    "lt-f64-32768-rand": ([('TOP', 0, 3, 32768, 3, 3, 27, 1, 0, 15), ('LATTREE', 3, 12, 4096, 3, 0, 0, 0, 1, 1), ('LATTREE', 3, 12, 4096, 3, 0, 0, 0, 1, 1), ('LATTREE', 3, 12, 4096, 3, 0, 0, 0, 1, 1), ('LATTREE', 3, 12, 4096, 3, 0, 0, 0, 1, 1)],
        [('LATTREE', 15, 12, 4096, 3, 0, 0, 0, 1, 1), ('LATTREE', 15, 12, 4096, 3, 0, 0, 0, 1, 1), ('LATTREE', 15, 12, 4096, 3, 0, 0, 0, 1, 1), ('LATTREE', 15, 12, 4096, 3, 0, 0, 0, 1, 1), ('TOP', 3, 3, 32768, 3, 3, 27, 1, 0, 15)]),
    "lt-f64-32768-top": ([('TOP', 0, 3, 32768, 3, 3, 37, 1)],
        [('TOP', 3, 3, 32768, 3, 3, 37, 1)]),
    "lt-f64-32768-deep": ([('TOP', 0, 3, 32768, 3, 3, 37, 1, 0, 16), ('LATTREE', 3, 1, 4096, 3, 0, 0, 0, 1, 1)],
        [('LATTREE', 4, 1, 4096, 3, 0, 0, 0, 1, 1), ('TOP', 3, 3, 32768, 3, 3, 37, 1, 0, 16)]),
    "lt-f32-16384-deep": ([('TOP', 0, 2, 16384, 3, 2, 5, 1, 0, 4), ('LATTREE', 2, 1, 4096, 3, 0, 0, 0, 1, 1)],
        [('LATTREE', 3, 1, 4096, 3, 0, 0, 0, 1, 1), ('TOP', 2, 2, 16384, 3, 2, 5, 1, 0, 4)]),
    "ip-f64-32768-L3": ([('L1TILE', 0, 1, 32768, 1, 1), ('L1TILE', 1, 1, 16384, 1, 2, 1, 1), ('FUSED', 2, 1, 8192, 4, 0, 1)],
        [('FUSED', 3, 1, 8192, 4), ('L1TILE', 2, 1, 16384, 1, 2, 1, 1), ('L1TILE', 1, 1, 32768, 1, 1)]),
    "ip-f64-16384-L1": ([('LEVEL', 0, 1, 16384, 1)],
        [('LEVEL', 1, 1, 16384, 1)]),
    "ip-f32-32768-tree": ([('LEVEL', 0, 1, 32768, 1, 1), ('LEVEL', 1, 1, 32768, 1, 1), ('LEVEL', 2, 1, 32768, 1, 1)],
        [('LEVEL', 3, 1, 32768, 1, 1), ('LEVEL', 2, 1, 32768, 1, 1), ('LEVEL', 1, 1, 32768, 1, 1)]),
    "ip-f64-16384-tree": ([('LEVEL', 0, 1, 16384, 1, 1), ('LEVEL', 1, 1, 16384, 1, 1), ('LEVEL', 2, 1, 16384, 1, 1)],
        [('LEVEL', 3, 1, 16384, 1, 1), ('LEVEL', 2, 1, 16384, 1, 1), ('LEVEL', 1, 1, 16384, 1, 1)]),
    "wpd-f64-64": ([('LATWPD', 0, 3, 64, 67, 4)],
        [('LATF64', 3, 3, 64, 67, 4, 0, 1)]),
    "wpd-f64-1024": ([('LATWPD', 0, 4, 1024, 5, 4)],
        [('LATF64', 4, 4, 1024, 5, 4, 0, 1)]),
    "wpd-f64-4096": ([('LATWPD', 0, 3, 4096, 3, 4)],
        [('LATF64', 3, 3, 4096, 3, 4, 0, 1)]),
    "wpd-f32-128": ([('LATWPD', 0, 3, 128, 35, 4)],
        [('LATF32', 3, 3, 128, 35, 4, 0, 1)]),
    "wpd-f32-256-B33": ([('FUSED', 0, 3, 256, 33, 1)],
        [('LATTREE', 3, 3, 256, 33, 1, 0, 0, 0, 1)]),
    "wpd-f32-256-B19": ([('FUSED', 0, 3, 256, 19, 1)],
        [('FUSED', 3, 3, 256, 19, 0, 0, 0, 1)]),
    "wpd-f64-16384": ([('TOPWPD', 0, 1, 16384, 3), ('FUSED', 1, 2, 8192, 6, 1, 0, 0, 1, 1)],
        [('TOP', 3, 3, 16384, 3, 3, -1, 0, 1)]),
    "wpd-f64-16384-L9": ([('TOPWPD', 0, 1, 16384, 3), ('FUSED', 1, 8, 8192, 6, 1, 0, 0, 1, 1)],
        [('LATF64', 9, 7, 4096, 12, 4), ('TOP', 2, 2, 16384, 3, 2, -1)]),
    "wpd-f64-24": ([('LEVEL', 0, 1, 24, 5, 0, 1), ('LEVEL', 1, 1, 24, 5, 0, 1)],
        None),
    "wpd-f64-4": ([('LEVEL', 0, 1, 4, 5, 0, 1), ('LEVEL', 1, 1, 4, 5, 0, 1)],
        [('LEVEL', 2, 1, 4, 5, 0, 1), ('LEVEL', 1, 1, 4, 5)]),
    "lvl-f32-4": ([('LEVEL', 0, 1, 4, 5), ('LEVEL', 1, 1, 4, 5)],
        [('LEVEL', 2, 1, 4, 5), ('LEVEL', 1, 1, 4, 5)]),
    "wpdt-f64-64": ([('LATWPD', 0, 3, 64, 67, 4)],
        [('LATTREE', 3, 3, 64, 67, 0, 1, 0, 0, 1)]),
    "wpdt-f64-64-B5": ([('FUSED', 0, 3, 64, 5, 1)],
        [('FUSED', 3, 3, 64, 5, 0, 0, 1, 2)]),
    "gbc-f64-64": (None,
        [('GATHER', 0, 0, 64, 5, 4, 8)]),
    "thr-f64-64-short": (None,
        [('THRCOPY', 6, 0, 64, 67), ('LATTREE', 6, 6, 64, 67)]),
    "thr-f64-64-short-soft": (None,
        [('THRCOPY', 3, 0, 64, 67, 1, 1, 0, 1), ('LATTREE', 3, 3, 64, 67)]),
    "thr-f64-1024-tree": (None,
        [('THRFUSED', 3, 3, 1024, 5, 1, 1, 0, 1), ('LATTREE', 3, 3, 1024, 5, 0, 0, 1)]),
    "thr-f64-1024-hard": (None,
        [('THRFUSED', 3, 3, 1024, 5), ('LATTREE', 3, 3, 1024, 5, 0, 0, 1)]),
    "thr-f32-1024-tree": (None,
        [('THRFUSED', 3, 3, 1024, 5), ('FUSED', 3, 3, 1024, 5, 0, 0, 1)]),
    "thr-f64-1024-tail": (None,
        [('ITAIL', 10, 6, 1024, 5, 6, 1), ('THRFUSED', 4, 4, 1024, 5, 1, 1, 1, 1), ('LATTREE', 4, 4, 1024, 5, 0, 0, 1)]),
    "thr-f64-128-pyr": (None,
        [('THRFUSED', 2, 2, 128, 5, 0, 1), ('FUSED', 2, 2, 128, 5, 0, 0, 1)]),
    "thr-f64-1024-full": (None,
        [('THRCOPY', 4, 0, 1024, 5, 1, 0, 0, 1), ('LATF64', 4, 4, 1024, 5, 4)]),
    "thr-f64-1024-full-hard": (None,
        [('THRCOPY', 4, 0, 1024, 5, 0, 1), ('LATF64', 4, 4, 1024, 5, 4)]),
    "thr-f64-16384-pyr-soft": (None,
        [('THRCOPY', 14, 0, 16384, 3, 1, 0, 0, 1), ('LATTREE', 14, 12, 4096, 3, 0, 0, 0, 1, 1), ('TOP', 2, 2, 16384, 3, 2, 3, 1, 0, 1)]),
    "thr-f32-1024-tree-soft": (None,
        [('THRFUSED', 3, 3, 1024, 5, 1, 1, 0, 1), ('FUSED', 3, 3, 1024, 5, 0, 0, 1)]),
    "thr-f64-1024-tail-hard": (None,
        [('ITAIL', 10, 6, 1024, 5, 6, 1), ('THRFUSED', 4, 4, 1024, 5, 0, 0, 1), ('LATTREE', 4, 4, 1024, 5, 0, 0, 1)]),
    "thr-f64-16384-pyr": (None,
        [('THRCOPY', 14, 0, 16384, 3, 0, 1, 0, 1), ('LATTREE', 14, 12, 4096, 3, 0, 0, 0, 1, 1), ('TOP', 2, 2, 16384, 3, 2, 3, 1, 0, 1)]),
    "wrap-level-wpd": ([('LEVEL', 0, 1, 6144, 343, 0, 1), ('LEVEL', 1, 1, 6144, 343, 0, 1)],
        None),
    "wrap-level-wpt": ([('LEVEL', 0, 1, 8192, 257), ('LEVEL', 1, 1, 8192, 257)],
        [('LEVEL', 2, 1, 8192, 257), ('LEVEL', 1, 1, 8192, 257)]),
    "wrap-gather": (None,
        [('GATHER', 3, 0, 64, 16500, 4, 8), ('LEVEL', 3, 1, 64, 16500, 1), ('LEVEL', 2, 1, 64, 16500, 1), ('LEVEL', 1, 1, 64, 16500, 1)]),
    "wrap-fused": ([('FUSED', 0, 3, 8, 4200, 0, 1)],
        [('FUSED', 3, 3, 8, 4200)]),
    "wrap-top": ([('TOP', 0, 3, 65536, 130, 3, -1)],
        [('TOP', 3, 3, 65536, 130, 3, -1)]),
}
# <<< PINS

# the extras (after route, depth, K, n, signals) that decide a kernel or a branch of it: how many of e0 .. belong to the key of part c
INSTANCE = {"LATF64": 3, "LATWPD": 0, "LATF32": 3, "LATTREE": 5, "LAT8KT": 0, "LANETREE": 1, "SMALLTREE": 1, "HAAR": 0, "TOP": 0,
            "TOPWPD": 0, "FUSED": 5, "L1TILE": 0, "LEVEL": 2, "GATHER": 0, "TAIL": 0, "ITAIL": 0, "THRFUSED": 3, "THRCOPY": 0}


def _reachable():
    """(route, elem_size, inverse, deciding extras), written from the launchers' conditions"""
    R = set()

    def add(route, es, inv, *e):
        for s in (es if isinstance(es, tuple) else (es,)):
            for i in (inv if isinstance(inv, tuple) else (inv,)):
                R.add((route, s, i, tuple(e) + (0,) * (INSTANCE[route] - len(e))))

    both, fi = (8, 4), (0, 1)
    add("LATF64", 8, fi, 4)                                # stages; folded; strided
    add("LATF64", 8, 1, 6, 1)                              # the folded full-depth inverse
    add("LATF64", 8, fi, 6)                                # 12 taps, general kernel (forward; the inverse under mode 3)
    add("LATF64", 8, 1, 4, 0, 1)                           # iwpd of a full tree: the stride of the table
    add("LATWPD", both, 0)
    add("LATF32", 4, fi, 4)
    add("LATF32", 4, 1, 4, 0, 1)
    add("LATTREE", both, fi)                               # a tree, dense
    add("LATTREE", both, fi, 1)                            # the tree of ones
    add("LATTREE", 4, 1, 1, 0, 0, 0, 1)                    # ... with the stride of a packet table (iwpd, Float32 256 samples)
    add("LATTREE", 8, 1, 0, 1, 0, 0, 1)                    # iwpd along a tree: col_stride
    add("LATTREE", 8, 1, 0, 0, 1)                          # threshold or head on the loads
    add("LATTREE", both, fi, 0, 0, 0, 1, 1)                # the 4096-sample node of a long signal
    add("LATTREE", both, 1, 0, 0, 1, 1, 1)                 # ... with the head of the tail
    add("LAT8KT", 8, fi)
    add("LANETREE", both, fi)
    add("LANETREE", 4, fi, 1)
    add("SMALLTREE", 8, fi, 1)
    add("HAAR", 8, fi)
    add("TOP", both, fi)
    add("TOPWPD", 8, 0)
    add("FUSED", 8, 0, 0, 1, 1)                            # forward, in-place kernel, a status
    add("FUSED", 8, 0, 0, 1, 1, 1)                         # ... reading with the long signal's stride (the finisher of wx_dev_dwt_long)
    add("FUSED", 8, 1, 0, 0, 1, 1)                         # its inverse twin (wx_dev_idwt_long)
    add("FUSED", both, 0, 0, 1)                            # forward, in-place kernel, full tree
    add("FUSED", 8, 0, 0, 1, 0, 0, 0)
    add("FUSED", both, 0, 1)                               # wpd layout
    add("FUSED", 8, 0, 1, 0, 0, 1, 1)                      # wpd of a long signal: sub-signals of the table
    add("FUSED", both, 1)                                  # inverse, full tree
    add("FUSED", both, 1, 0, 0, 1)                         # inverse, a status
    add("FUSED", 4, 1, 0, 0, 0, 1)                         # inverse, the stride of a packet table
    add("FUSED", 8, 1, 0, 0, 1, 2)                         # inverse, colmap
    add("L1TILE", 8, fi)
    add("LEVEL", both, fi)
    add("LEVEL", 8, fi, 1)                                 # a status
    add("LEVEL", 4, fi, 1)                                 # (Float32: in place past the fused kernel, the forced run of wrap-gather)
    add("LEVEL", 8, fi, 0, 1)                              # a packet table
    add("GATHER", both, 1)
    add("TAIL", both, 0)
    add("ITAIL", both, 1)
    add("THRFUSED", both, 1, 0, 0, 1)                      # idwt: the head, no threshold
    add("THRFUSED", both, 1, 0, 0, 0)                      # Hard, one threshold
    add("THRFUSED", both, 1, 1, 1, 0)                      # Soft, per signal
    add("THRFUSED", 8, 1, 1, 1, 1)
    add("THRFUSED", 8, 1, 0, 1, 0)
    add("THRCOPY", 8, 1)
    return R


REACHABLE = _reachable()

RECORD = None                                             # a dict: tools/dwt1d_pins.py collects the traces instead of comparing them


def _wt(wx, c):
    if c.qmf:
        import qmf_family
        q = qmf_family.family(wx)[c.qmf]
        assert q.size == c.F
        return wx.OrthoFilter(q, c.qmf)
    return wx.wavelet(getattr(wx.WT, WF[c.F]))


def _tol(c):
    tol = c.tol or TOL[np.dtype(c.dtype)]
    assert tol <= TOL[np.dtype(c.dtype)]
    return tol


def _key(tr):
    out = []
    for t in tr:
        e = [t.e0, t.e1, t.e2, t.e3, t.e4]
        while e and e[-1] == 0:
            e.pop()
        out.append((t.route, t.depth, t.K, t.n, t.signals) + tuple(e))
    return out


def _instances(rows, es, inverse):
    out = set()
    for r in rows:
        e = tuple(r[5:]) + (0,) * 5
        out.add((r[0], es, inverse, e[:INSTANCE[r[0]]]))
    return out


def _need(c, which, tr, tag=""):
    """the trace of a case against c.expect[which] and PINS[c.id][which] (0 = forward, 1 = inverse)"""
    assert tr.dropped == 0
    es = np.dtype(c.dtype).itemsize
    assert all(t.inverse == which and t.elem_size == es for t in tr), (c.id, list(tr))
    got = _key(tr)
    names = tuple(r[0] for r in got)
    if RECORD is not None:
        RECORD.setdefault(c.id + tag, [None, None])[which] = got
        if not tag and names != tuple(c.expect[which]):
            RECORD.setdefault("surprises", {})[c.id + ":" + str(which)] = [list(c.expect[which]), list(names)]
        return
    if not tag:
        assert names == tuple(c.expect[which]), "%s %s: written for %s, took %s" % (c.id, ("forward", "inverse")[which], c.expect[which], got)
        want = [tuple(w) for w in PINS[c.id][which]]
        assert got == want, "%s %s: pinned %s, took %s" % (c.id, ("forward", "inverse")[which], want, got)


def _close(got, exp, tol, what):
    """every signal (last axis) within tol of that signal's own largest magnitude"""
    got = np.asarray(got, dtype=np.float64)
    exp = np.asarray(exp, dtype=np.float64)
    assert got.shape == exp.shape, (what, got.shape, exp.shape)
    ax = tuple(range(got.ndim - 1))
    err = np.abs(got - exp).max(axis=ax)
    den = np.abs(exp).max(axis=ax)
    rel = np.atleast_1d(err / np.where(den > 0, den, 1.0))
    b = int(np.argmax(rel))
    print("%s: worst signal %d, error %.3g (tolerance %.3g)" % (what, b, rel[b], tol))
    if RECORD is not None:
        RECORD.setdefault("err", {})[what] = float(rel[b])
    assert np.isfinite(got).all() and rel[b] <= tol, "%s: signal %d: error %.3g of the signal's maximum (tolerance %.3g)" % (
        what, b, rel[b], tol)


def _tree(wx, n, spec):
    """the int depth of a full tree, or the boolean tree (heap order, n - 1 nodes) of a spec"""
    if spec is None or isinstance(spec, int):
        return spec
    if spec[0] == "dwt":
        return np.asarray(wx.maketree(n, spec[1], "dwt"), dtype=bool)
    if spec[0] == "rand":
        return _rand_tree(n, spec[1], spec[2])
    t = np.zeros(n - 1, dtype=bool)
    t[np.asarray(spec[1]) - 1] = True
    return t


class _mode:
    """wx.set_force_generic(m) for a block"""

    def __init__(self, wx, m):
        self.wx, self.m = wx, m

    def __enter__(self):
        self.wx.set_force_generic(self.m)

    def __exit__(self, *exc):
        self.wx.set_force_generic(0)


def _fwd(wx, c, x, wt, arg):
    if c.op == "wpd":
        return wx.wpdall(x, wt, arg)
    if c.op == "dwt":
        return wx.dwtall(x, wt, arg)
    if c.inplace:
        y = x.clone()
        wx.wpt_(y[:, 0], y[:, 0], wt, arg)
        return y
    return wx.wptall(x, wt, arg)


def _inv(wx, c, xw, wt, arg):
    if c.op == "wpd":
        return wx.iwpdall(xw, wt, arg)
    if c.op == "dwt":
        return wx.idwtall(xw, wt, arg)
    if c.inplace:
        y = xw.clone()
        wx.iwpt_(y[:, 0], y[:, 0], wt, arg)
        return y
    return wx.iwptall(xw, wt, arg)


def _oracle_pair(wx, oracle, c, xh, qmf):
    """(forward reference, the inverse's argument, function of the coefficients that gives the inverse reference)"""
    if c.op == "wpd":
        iarg = _tree(wx, c.n, c.iarg) if c.iarg is not None else c.arg
        return oracle.wpdall(xh, qmf, c.arg), iarg, lambda w: oracle.iwpdall(w, qmf, iarg)
    tree = _tree(wx, c.n, ("dwt", c.arg)) if c.op == "dwt" else _tree(wx, c.n, c.arg)
    return oracle.wptall(xh, qmf, tree), (c.arg if c.op == "dwt" else tree), lambda w: oracle.iwptall(w, qmf, tree)


def _dev(wx, a):
    """numpy (Julia shape) -> a column-major device tensor of its own (jl_empty: what the entry points themselves allocate)"""
    import torch
    a = np.asfortranarray(a)
    t = wx.jl_empty(a.shape, torch.float64 if a.dtype == np.float64 else torch.float32, "cuda")
    t.copy_(wx.to_device(a))
    return t


def _only_generic(tr):
    return len(tr) > 0 and {t.route for t in tr} <= GENERIC


def _threshold(w, th, t, row_lo):
    """Wavelets.Threshold on rows [row_lo, n) of every signal, in the array's own type: HardTH keeps |x| > t, SoftTH shrinks by t"""
    w = np.array(w, order="F")
    t = np.broadcast_to(np.asarray(t, dtype=w.dtype), (w.shape[1],))[None, :]
    v = w[row_lo:]
    if th == "hard":
        v[np.abs(v) <= t] = 0
    else:
        w[row_lo:] = np.sign(v) * np.maximum(np.abs(v) - t, 0).astype(w.dtype)
    return w


def _run_thr(wx, oracle, c, x, wt):
    from waveletsext_jl_amd import denoising as dn
    tol = _tol(c)
    tree = _tree(wx, c.n, c.arg)
    coef = np.asfortranarray(oracle.wptall(x, wt.qmf, tree), dtype=c.dtype)
    rng = np.random.default_rng(77 + c.n)
    t = (0.5 + rng.random(c.B)).astype(c.dtype) if c.per else np.asarray([0.8], dtype=c.dtype)
    th = wx.HardTH() if c.th == "hard" else wx.SoftTH()
    exp = oracle.iwptall(np.asfortranarray(_threshold(coef, c.th, t, c.row_lo), dtype=np.float64), wt.qmf, tree)
    cd = _dev(wx, coef)

    def call():
        return wx.to_numpy(dn._iwpt_thresh(dn.Arg(cd), wt, tree, True, th, t, c.row_lo))

    with wx.dwt1d_trace() as tr:
        got = call()
    _need(c, 1, tr)
    assert got.dtype == c.dtype
    _close(got, exp, tol, c.id + " against threshold + the oracle's inverse")
    with _mode(wx, 1), wx.dwt1d_trace() as trf:
        ref = call()
    assert _only_generic(trf), (c.id, _key(trf))
    _close(got, ref, 1e-13 if c.dtype == F64 else TOL[np.dtype(c.dtype)], c.id + " against one level per launch")


def run_case(wx, oracle, c):
    wt = _wt(wx, c)
    tol = _tol(c)
    agree = 1e-13 if c.dtype == F64 else TOL[np.dtype(c.dtype)]
    rng = np.random.default_rng(7000 + c.n + 3 * c.F + 11 * c.B + sum(map(ord, c.id)))
    xh = np.asfortranarray(rng.standard_normal((c.n, c.B)).astype(c.dtype))
    if c.op == "thr":
        return _run_thr(wx, oracle, c, xh, wt)
    if c.op == "gbc":
        tree = _tree(wx, c.n, c.arg)
        tab = np.asfortranarray(oracle.wpdall(xh, wt.qmf, 3), dtype=c.dtype)
        td = _dev(wx, tab)
        with wx.dwt1d_trace() as tr:
            got = wx.to_numpy(wx.getbasiscoefall(td, tree))
        _need(c, 1, tr)
        for i in range(c.B):
            assert (got[:, i] == oracle.getbasiscoef(np.asfortranarray(tab[:, :, i]), tree)).all(), (c.id, i)
        return
    x = _dev(wx, xh)
    exp, iarg, oinv = _oracle_pair(wx, oracle, c, xh, wt.qmf)
    farg = c.arg if c.op in ("wpd", "dwt") else _tree(wx, c.n, c.arg)
    with wx.dwt1d_trace() as tr:
        got = _fwd(wx, c, x, wt, farg)
    _need(c, 0, tr)
    goth = wx.to_numpy(got)
    assert goth.dtype == c.dtype
    _close(goth, exp, tol, c.id + " forward")
    if c.forced:
        with _mode(wx, 1), wx.dwt1d_trace() as trf:
            ref = wx.to_numpy(_fwd(wx, c, x, wt, farg))
        assert _only_generic(trf), (c.id, _key(trf))
        _close(goth, ref, agree, c.id + " forward against one level per launch")
    for m in c.modes or ():
        with _mode(wx, m), wx.dwt1d_trace() as trm:
            ref = wx.to_numpy(_fwd(wx, c, x, wt, farg))
        _need(c, 0, trm, "@mode%d" % m)
        _mode_check(c, m, trm, 0)
        _close(goth, ref, agree, c.id + " forward against mode %d" % m)
    if c.expect[1] is None:
        return
    # the inverse of the oracle's coefficients, in the case's type
    coef = np.asfortranarray(exp, dtype=c.dtype)
    cd = _dev(wx, coef)
    with wx.dwt1d_trace() as tr:
        back = _inv(wx, c, cd, wt, iarg)
    _need(c, 1, tr)
    backh = wx.to_numpy(back)
    assert backh.dtype == c.dtype
    _close(backh, oinv(coef), tol, c.id + " inverse against the oracle")
    _close(backh, xh, 10 * tol, c.id + " inverse against the signal")
    if c.forced:
        with _mode(wx, 1), wx.dwt1d_trace() as trf:
            ref = wx.to_numpy(_inv(wx, c, cd, wt, iarg))
        assert _only_generic(trf), (c.id, _key(trf))
        _close(backh, ref, agree, c.id + " inverse against one level per launch")
    for m in c.modes or ():
        with _mode(wx, m), wx.dwt1d_trace() as trm:
            ref = wx.to_numpy(_inv(wx, c, cd, wt, iarg))
        _need(c, 1, trm, "@mode%d" % m)
        _mode_check(c, m, trm, 1)
        _close(backh, ref, agree, c.id + " inverse against mode %d" % m)


REGISTER = {"LATF64", "LATWPD", "LATF32", "LATTREE", "LAT8KT", "HAAR"}


def _mode_check(c, m, tr, inverse):
    """mode 2: no register kernels; mode 3: the same routes, the full-depth inverse without the fold"""
    if m == 2:
        assert len(tr) and not ({t.route for t in tr} & REGISTER), (c.id, _key(tr))
    if m == 3:
        assert [t.route for t in tr] == list(c.expect[inverse]) and all(t.e1 == 0 for t in tr if t.route == "LATF64"), (c.id, _key(tr))
        if inverse and RECORD is None:
            assert [(tuple(r) + (0, 0))[6] for r in PINS[c.id][1] if r[0] == "LATF64"] == [1], (c.id, PINS[c.id][1])   # folded in the normal run


@gpu
@pytest.mark.parametrize("cid", [c.id for c in CASES_A])
def test_route_and_parity(wx, oracle, cid):
    run_case(wx, oracle, CASE_BY_ID[cid])


# ---- b. every grid wrap-around loop goes round -------------------------------------------------------------------------------
class Wrap:
    """a part a case with B signals, of which the signals b >= period are copies of signal b mod period; `route`: the route of
    which one launch at least must have a grid smaller than its work items; `items`: work items (workgroups' worth) per signal of
    a launch.  TOP's launcher computes its grid itself (wx_top_grid, not in the row): its items are tiles, and the case holds more
    of them than the largest grid wx_top_grid can return on this device."""

    def __init__(self, cid, op, dtype, n, arg, F, B, route, items, forced=False, iarg=None, inverse=None, period=P):
        self.case = Case(cid, op, dtype, n, arg, F, B, None, iarg=iarg)
        self.route, self.items, self.forced, self.inverse, self.period = route, items, forced, inverse, period


WRAPS = [
    # wx_grid_for: a thread per output pair, 256 per workgroup, at most 4096 workgroups (343 * 3072 / 256 = 4116)
    Wrap("wrap-level-wpd", "wpd", F64, 6144, 2, 8, 343, "LEVEL", 6144 / 2 / 256, inverse=0),
    Wrap("wrap-level-wpt", "wpt", F64, 8192, 2, 8, 257, "LEVEL", 8192 / 2 / 256, forced=True),
    # the leaf gather of iwpd: an element per thread (16500 * 64 / 256 = 4125)
    Wrap("wrap-gather", "wpd", F32, 64, 3, 4, 16500, "GATHER", 64 / 256, forced=True, iarg=T3, inverse=1),
    # wx_fused_grid: a signal per turn, at most 4096 workgroups
    Wrap("wrap-fused", "wpt", F64, 8, 3, 4, 4200, "FUSED", 1),
    # wx_top_grid: `cus * per` persistent workgroups with `per > 8 -> 8`, a tile of at most 4096 input samples per turn
    # (wx_tt_ts: 4096 or 2048): 130 signals of 65536 samples are at least 2080 tiles, more than 8 x 256 CUs; 34 MB
    Wrap("wrap-top", "wpt", F32, 65536, 3, 8, 130, "TOP", 65536 / 4096, period=43),
]
WRAP_BY_ID = {w.case.id: w for w in WRAPS}


def _same_as_original(out, idx, what):
    """bit-identical: signal b against signal b mod P"""
    import torch
    bits = out.view(torch.int64 if out.dtype == torch.float64 else torch.int32)
    assert torch.equal(bits, bits.index_select(bits.ndim - 1, torch.as_tensor(idx, device=out.device))), what


def run_wrap(wx, oracle, w):
    import torch
    c = w.case
    wt = _wt(wx, c)
    tol = TOL[np.dtype(c.dtype)]
    P = w.period
    rng = np.random.default_rng(4242 + c.n)
    xh = np.asfortranarray(rng.standard_normal((c.n, P)).astype(c.dtype))
    idx = np.arange(c.B) % P
    tidx = torch.as_tensor(idx, device="cuda")
    head = Case(c.id, c.op, c.dtype, c.n, c.arg, c.F, P, None, iarg=c.iarg)
    exp, iarg, oinv = _oracle_pair(wx, oracle, head, xh, wt.qmf)
    farg = c.arg if c.op in ("wpd", "dwt") else _tree(wx, c.n, c.arg)
    seen = False

    def spread(a):
        d = wx.to_device(np.asfortranarray(a))
        d = d.index_select(d.ndim - 1, tidx)
        out = wx.jl_empty(tuple(d.shape), d.dtype, "cuda")
        out.copy_(d)
        return out

    def wrapped(tr, inverse):
        rows = [t for t in tr if t.route == w.route]
        if RECORD is not None:
            RECORD.setdefault(c.id, [None, None])[inverse] = _key(tr)
            RECORD.setdefault("grids", {})[c.id + str(inverse)] = [t.grid for t in rows]
        else:
            assert _key(tr) == [tuple(r) for r in PINS[c.id][inverse]], (c.id, inverse, _key(tr))
        if w.route == "TOP":
            import torch
            cap = 8 * torch.cuda.get_device_properties(0).multi_processor_count
            return len(rows) > 0 and all(t.n == c.n and t.signals == c.B for t in rows) and w.items * c.B > cap
        return any(t.grid < w.items * c.B for t in rows)

    if w.inverse != 1:
        x = spread(xh)
        with _mode(wx, 1 if w.forced else 0), wx.dwt1d_trace() as tr:
            got = _fwd(wx, c, x, wt, farg)
        seen |= wrapped(tr, 0)
        _same_as_original(got, idx, c.id + " forward")
        _close(wx.to_numpy(got[..., :P]), exp, tol, c.id + " forward")
    if w.inverse != 0:
        coef = np.asfortranarray(exp, dtype=c.dtype)
        cd = spread(coef)
        with _mode(wx, 1 if w.forced else 0), wx.dwt1d_trace() as tr:
            back = _inv(wx, c, cd, wt, iarg)
        seen |= wrapped(tr, 1)
        _same_as_original(back, idx, c.id + " inverse")
        _close(wx.to_numpy(back[..., :P]), oinv(coef), tol, c.id + " inverse against the oracle")
        _close(wx.to_numpy(back[..., :P]), xh, 10 * tol, c.id + " inverse against the signal")
    assert seen, (c.id, w.route)


@gpu
@pytest.mark.parametrize("wid", [w.case.id for w in WRAPS])
def test_grid_loops_go_round(wx, oracle, wid):
    run_wrap(wx, oracle, WRAP_BY_ID[wid])


# ---- c. the table itself -----------------------------------------------------------------------------------------------------
def test_pins_cover_what_is_reachable(wx):
    """every (route, type, direction, deciding extras) pinned in parts a and b is declared in REACHABLE and the other way round: a
    route or a branch cannot be added to the dispatch (or lose its last case) without this file saying so"""
    cases = dict(CASE_BY_ID)
    cases.update({w.case.id: w.case for w in WRAPS})
    assert {k.split("@")[0] for k in PINS} == set(cases), sorted({k.split("@")[0] for k in PINS} ^ set(cases))
    pinned = set()
    for cid, (f, i) in PINS.items():
        es = np.dtype(cases[cid.split("@")[0]].dtype).itemsize
        pinned |= _instances(f or [], es, 0) | _instances(i or [], es, 1)
    assert pinned == REACHABLE, "declared and not pinned: %s; pinned and not declared: %s" % (
        sorted(REACHABLE - pinned, key=repr), sorted(pinned - REACHABLE, key=repr))
