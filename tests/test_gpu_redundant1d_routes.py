"""GPU parity of the 1-D redundant transforms (csrc/wx_swt1d.hip, wx_haarswt.hip, wx_swtdeep*.hip) on every launch route.

The launchers choose among about twenty kernels by length, depth, type, filter length, container, shift and tree.  Every case
here runs the public entry point on device tensors inside `wx.swt1d_trace()` -- the record the launchers themselves write next to
each launch (csrc/wx_debug.h) -- and fails if the sequence of (route, depth, K, R, OPT) is not the one written out in PINS, then
compares with the CPU oracle.  The oracle always runs in Float64 on the case's own values (also for Float32 cases); every column
of a coefficient table is compared against that column's own maximum at helpers.TOL; inputs are white noise; Float32 cases stop
at depth log2(n) - 2, so that no column degenerates to a multiple of the signal's mean.

  a. one case per route and per template class at the smallest shape that reaches it; where a fused route exists the same call
     is repeated under wx.set_force_generic(1), which must launch FLVL / FG / ILVL / IAC* only and agree to 1e-13 (Float64)
  b. the shift-based inverses for every shift, iswpd along trees with and without a shift
  c. every grid wrap-around loop goes round once: signals b >= 251 are copies of signal b mod 251, so every output must be
     bit-identical to that of its original
  d. (no device) the inverse schedules of part a through wx.swt_inv_plan

Rows per thread of FMRC (k_swt_fwd_multi_rc) and IM (k_swt_inv_multi): REACHED_FMRC / REACHED_IM below, each pinned by a case.
A scan of n in {24, 32, 48, 64, 96, 384, 512, 640, 1024, 2048, 4096} x every valid L x {haar, db2, db4, db7, db10} x both types
with the trace on reaches OPT = 1, 4 and 8 only.  OPT = 2 needs a tile of 128 to 255 elements (four rows per thread would leave
fewer than 64 threads, two do not), which no length of that set has and n = 128 has at every K: the cases sp-*-128-*.  Every
(K, OPT) in {2, 3} x {1, 2, 4, 8} is therefore reachable in the inverse in both types and in the forward in Float64.  Not
reachable within the rules of this file:
  * FMRC with OPT = 1 or 2 in Float32: residue-class tiles need 16 classes of Float32, that is a pass starting at depth 4 or
    below, with n >> 4 = 4 (OPT = 1: n = 64) or 8 to 15 (OPT = 2: n = 128 .. 240) samples per class -- L = 6 of those lengths,
    beyond the depth log2(n) - 2 at which Float32 cases stop.  The Float64 instances of the same templates are pinned.
FHAAR6 / IHAAR6 need L >= 12 and are pinned in test_gpu_bench_geometry.py, where a table of that depth is already paid for."""
import numpy as np
import pytest

from helpers import TOL, random_tree_1d

gpu = pytest.mark.gpu
F64, F32 = np.float64, np.float32
FLEN = {"haar": 2, "db2": 4, "db4": 8, "db7": 14, "db10": 20, "db11": 22}
P = 251                                                   # part c: signals b >= P are copies of signal b mod P
FWD_GENERIC = {"FLVL", "FG"}
INV_GENERIC = {"ILVL", "IACDWT", "IACWPT", "IACWPD"}


class Case:
    """kind: the container and family (dwt / wpt / wpd, ac* = autocorrelation); inv: None = no inverse in this case,
    "avg" = average based, an int = that shift, "pyramid" = iswpd along the pyramid tree of depth L"""

    def __init__(self, cid, kind, dtype, n, L, wname, B=2, inv="avg", forced=False):
        self.id, self.kind, self.dtype, self.n, self.L, self.wname, self.B, self.inv, self.forced = cid, kind, dtype, n, L, wname, B, inv, forced


# ---- a. one case per route and template class ------------------------------------------------------------------------------
CASES_A = [
    # fused sdwt / isdwt in place, one column of LDS: Float32 n = 32768, Float64 n = 16384 (runtime taps with db11)
    Case("sd-f32-32768-L2", "dwt", F32, 32768, 2, "db4", forced=True),
    Case("sd-f32-32768-L13", "dwt", F32, 32768, 13, "db4"),
    Case("sd-f64-16384-db11", "dwt", F64, 16384, 3, "db11", forced=True),
    # between the fused limits: per-level forward with 96 KiB of LDS, tile inverse in the dwt container, per-sample below it
    Case("sd-f64-12288-L2", "dwt", F64, 12288, 2, "db4"),
    Case("sd-f64-12288-L8", "dwt", F64, 12288, 8, "db4"),
    # fused isdwt with one workgroup per CU but no pipeline
    Case("sd-f64-6144-L2", "dwt", F64, 6144, 2, "db4", forced=True),
    Case("sd-f64-6144-L11", "dwt", F64, 6144, 11, "db4"),
    # runtime-tap instances of the two-column fused kernels (inverse: eight per CU, then pipelined)
    Case("sd-f64-64-db11", "dwt", F64, 64, 6, "db11", forced=True),
    Case("sd-f64-4096-db11", "dwt", F64, 4096, 5, "db11", forced=True),
    Case("sd-f64-4096-db4", "dwt", F64, 4096, 5, "db4"),
    Case("sd-f32-8192-haar", "dwt", F32, 8192, 4, "haar"),
    Case("acd-f64-64", "acdwt", F64, 64, 4, "db4", forced=True),
    Case("acd-f64-16384", "acdwt", F64, 16384, 2, "db4"),
    Case("sd-f64-16384-db4", "dwt", F64, 16384, 4, "db4"),
    # filters of more than 20 taps in swpt: no composite passes, no fused inverse, no tile instance
    Case("sp-f64-512-db11", "wpt", F64, 512, 9, "db11"),
    Case("sp-f64-4096-db11", "wpt", F64, 4096, 4, "db11"),
    # db7 at depth: no lane-local instance for 14 taps, composite passes down to residue classes of one sample
    Case("sp-f64-1024-db7-L7", "wpt", F64, 1024, 7, "db7", forced=True),
    Case("sp-f64-1024-db7-L8", "wpt", F64, 1024, 8, "db7"),
    Case("sp-f64-1024-db7-L9", "wpt", F64, 1024, 9, "db7"),
    Case("sp-f64-1024-db7-L10", "wpt", F64, 1024, 10, "db7", forced=True),
    # rows per thread of FMRC / IM (module docstring), Float64
    Case("sp-f64-32-haar-L5", "wpt", F64, 32, 5, "haar", forced=True),
    Case("sp-f64-64-haar-L6", "wpt", F64, 64, 6, "haar", forced=True),
    Case("sp-f64-384-haar-L5", "wpt", F64, 384, 5, "haar"),
    Case("sp-f64-384-haar-L6", "wpt", F64, 384, 6, "haar"),
    Case("sp-f64-512-haar-L9", "wpt", F64, 512, 9, "haar", forced=True),
    Case("sp-f64-4096-haar-L5", "wpt", F64, 4096, 5, "haar"),
    Case("sp-f64-4096-db2-L6", "wpt", F64, 4096, 6, "db2"),
    Case("sp-f64-24-db4-L2", "wpt", F64, 24, 2, "db4"),
    Case("sp-f64-24-db2-L3", "wpt", F64, 24, 3, "db2"),
    Case("sp-f64-384-db4-L2", "wpt", F64, 384, 2, "db4"),
    Case("sp-f64-384-db2-L3", "wpt", F64, 384, 3, "db2"),
    Case("sp-f64-512-db10-L2", "wpt", F64, 512, 2, "db10"),
    Case("sp-f64-512-db2-L3", "wpt", F64, 512, 3, "db2"),
    Case("sp-f64-128-haar-L5", "wpt", F64, 128, 5, "haar"),                   # two rows per thread: tiles of 128 to 255 elements
    Case("sp-f64-128-haar-L6", "wpt", F64, 128, 6, "haar"),
    Case("sp-f64-128-db4-L2", "wpt", F64, 128, 2, "db4"),
    Case("sp-f64-128-db2-L3", "wpt", F64, 128, 3, "db2"),
    # Float32
    Case("sp-f32-384-db4-L6", "wpt", F32, 384, 6, "db4", forced=True),
    Case("sp-f32-4096-db4-L6", "wpt", F32, 4096, 6, "db4"),
    Case("sp-f32-2048-haar-L9", "wpt", F32, 2048, 9, "haar"),
    Case("sp-f32-4096-haar-L9", "wpt", F32, 4096, 9, "haar", B=1),
    Case("sp-f32-24-db4-L2", "wpt", F32, 24, 2, "db4"),
    Case("sp-f32-32-haar-L3", "wpt", F32, 32, 3, "haar"),
    Case("sp-f32-384-db4-L2", "wpt", F32, 384, 2, "db4"),
    Case("sp-f32-384-db2-L3", "wpt", F32, 384, 3, "db2"),
    Case("sp-f32-512-db10-L2", "wpt", F32, 512, 2, "db10"),
    Case("sp-f32-512-db2-L3", "wpt", F32, 512, 3, "db2"),
    Case("sp-f32-128-db4-L2", "wpt", F32, 128, 2, "db4"),
    Case("sp-f32-128-db2-L3", "wpt", F32, 128, 3, "db2"),
    # swpd / acwpd two levels per pass: an even and an odd number of levels (the odd one ends in FLVL)
    Case("pd-f64-64-L4", "wpd", F64, 64, 4, "db4", forced=True),
    Case("pd-f64-64-L3", "wpd", F64, 64, 3, "db4"),
    Case("pd-f32-64-L3", "wpd", F32, 64, 3, "db4"),
    Case("acpd-f64-64-L4", "acwpd", F64, 64, 4, "db4", forced=True),
    Case("acpd-f64-64-L3", "acwpd", F64, 64, 3, "db4"),
    Case("acp-f64-64-L4", "acwpt", F64, 64, 4, "db4"),
    # tile inverse: wpt container and wpd container with a sparse tree, two tap counts (the dwt container: sd-f64-12288-*)
    Case("sp-f64-4096-haar-L1", "wpt", F64, 4096, 1, "haar", forced=True),
    Case("sp-f32-4096-db4-L1", "wpt", F32, 4096, 1, "db4"),
    Case("pd-f64-4096-pyramid-db4", "wpd", F64, 4096, 2, "db4", inv="pyramid", forced=True),
    Case("pd-f64-4096-pyramid-db2", "wpd", F64, 4096, 2, "db2", inv="pyramid"),
    # per-sample inverse, shift based (the average-based one: sd-f64-12288-L8, sp-f64-*-db11)
    Case("sp-f64-64-db4-sm5", "wpt", F64, 64, 3, "db4", inv=5),
    # lane-local deep levels
    Case("sp-f64-1024-db4-L10", "wpt", F64, 1024, 10, "db4", forced=True),
    Case("pd-f64-1024-db4-L7", "wpd", F64, 1024, 7, "db4"),
    # one level per launch from global memory: wpd container with its root-column copy at L = 3, autocorrelation, Float32 swpt
    # on two alternating scratch arrays, lengths that are no power of two
    Case("pd-f64-20488-L3", "wpd", F64, 20488, 3, "db4", inv=None),            # (iswpd by depth wants a dyadic length)
    Case("acpd-f64-20488-L3", "acwpd", F64, 20488, 3, "db4", inv=None),
    Case("acd-f64-20488-L3", "acdwt", F64, 20488, 3, "db4"),
    Case("sp-f32-40968-L3", "wpt", F32, 40968, 3, "db4"),
    Case("sp-f64-20488-L3", "wpt", F64, 20488, 3, "haar"),
    Case("sd-f64-20488-L3", "dwt", F64, 20488, 3, "db4"),
]
CASE_BY_ID = {c.id: c for c in CASES_A}

# (route, depth, K, R, OPT) of every launch, as recorded on an MI355X: case id -> (forward, inverse)
PINS = {
    "sd-f32-32768-L2": ([("FSDIP", 0, 2, 8, 0)],
        [("ISDIP", 2, 2, 0, 0)]),
    "sd-f32-32768-L13": ([("FSDIP", 0, 13, 8, 0)],
        [("ISDIP", 13, 13, 0, 0)]),
    "sd-f64-16384-db11": ([("FSDIP", 0, 3, 0, 0)],
        [("ISDIP", 3, 3, 0, 0)]),
    "sd-f64-12288-L2": ([("FLVL", 0, 1, 0, 0), ("FLVL", 1, 1, 0, 0)],
        [("ITILE", 2, 1, 4, 0), ("ITILE", 1, 1, 4, 0)]),
    "sd-f64-12288-L8": ([("FLVL", 0, 1, 0, 0), ("FLVL", 1, 1, 0, 0), ("FLVL", 2, 1, 0, 0), ("FLVL", 3, 1, 0, 0), ("FLVL", 4, 1, 0, 0), ("FLVL", 5, 1, 0, 0), ("FLVL", 6, 1, 0, 0), ("FLVL", 7, 1, 0, 0)],
        [("ILVL", 8, 1, 0, 0), ("ITILE", 7, 1, 4, 0), ("ITILE", 6, 1, 4, 0), ("ITILE", 5, 1, 4, 0), ("ITILE", 4, 1, 4, 0), ("ITILE", 3, 1, 4, 0), ("ITILE", 2, 1, 4, 0), ("ITILE", 1, 1, 4, 0)]),
    "sd-f64-6144-L2": ([("FSD", 0, 2, 8, 0)],
        [("ISD", 2, 2, 8, 0)]),
    "sd-f64-6144-L11": ([("FSD", 0, 11, 8, 0)],
        [("ISD", 11, 11, 8, 0)]),
    "sd-f64-64-db11": ([("FSD", 0, 6, 0, 0)],
        [("ISD", 6, 6, 0, 0)]),
    "sd-f64-4096-db11": ([("FSD", 0, 5, 0, 0)],
        [("ISD", 5, 5, 0, 1)]),
    "sd-f64-4096-db4": ([("FSD", 0, 5, 8, 0)],
        [("ISD", 5, 5, 8, 1)]),
    "sd-f32-8192-haar": ([("FSD", 0, 4, 2, 0)],
        [("ISD", 4, 4, 2, 1)]),
    "acd-f64-64": ([("FSD", 0, 4, 0, 1)],
        [("IACDWT", 4, 4, 0, 0)]),
    "acd-f64-16384": ([("FSDIP", 0, 2, 0, 1)],
        [("IACDWT", 2, 2, 0, 0)]),
    "sd-f64-16384-db4": ([("FSDIP", 0, 4, 8, 0)],
        [("ISDIP", 4, 4, 0, 0)]),
    "sp-f64-512-db11": ([("FLVL", 0, 1, 0, 0), ("FLVL", 1, 1, 0, 0), ("FLVL", 2, 1, 0, 0), ("FLVL", 3, 1, 0, 0), ("FLVL", 4, 1, 0, 0), ("FLVL", 5, 1, 0, 0), ("FLVL", 6, 1, 0, 0), ("FLVL", 7, 1, 0, 0), ("FLVL", 8, 1, 0, 0)],
        [("ILVL", 9, 1, 0, 0), ("ILVL", 8, 1, 0, 0), ("ILVL", 7, 1, 0, 0), ("ILVL", 6, 1, 0, 0), ("ILVL", 5, 1, 0, 0), ("ILVL", 4, 1, 0, 0), ("ILVL", 3, 1, 0, 0), ("ILVL", 2, 1, 0, 0), ("ILVL", 1, 1, 0, 0)]),
    "sp-f64-4096-db11": ([("FLVL", 0, 1, 0, 0), ("FLVL", 1, 1, 0, 0), ("FLVL", 2, 1, 0, 0), ("FLVL", 3, 1, 0, 0)],
        [("ILVL", 4, 1, 0, 0), ("ILVL", 3, 1, 0, 0), ("ILVL", 2, 1, 0, 0), ("ILVL", 1, 1, 0, 0)]),
    "sp-f64-1024-db7-L7": ([("FM", 0, 2, 0, 0), ("FM", 2, 2, 0, 0), ("FMRC", 4, 2, 16, 4), ("FLVL", 6, 1, 0, 0)],
        [("IM", 7, 2, 32, 8), ("IM", 5, 2, 8, 8), ("IM", 3, 2, 2, 8), ("ILVL", 1, 1, 0, 0)]),
    "sp-f64-1024-db7-L8": ([("FM", 0, 2, 0, 0), ("FM", 2, 2, 0, 0), ("FMRC", 4, 2, 16, 4), ("FMRC", 6, 2, 64, 4)],
        [("IM", 8, 2, 64, 8), ("IM", 6, 2, 16, 8), ("IM", 4, 2, 4, 8), ("IM", 2, 2, 1, 8)]),
    "sp-f64-1024-db7-L9": ([("FM", 0, 2, 0, 0), ("FM", 2, 2, 0, 0), ("FMRC", 4, 2, 16, 4), ("FMRC", 6, 2, 64, 4), ("FLVL", 8, 1, 0, 0)],
        [("IM", 9, 2, 128, 8), ("IM", 7, 2, 32, 8), ("IM", 5, 2, 8, 8), ("IM", 3, 2, 2, 8), ("ILVL", 1, 1, 0, 0)]),
    "sp-f64-1024-db7-L10": ([("FM", 0, 2, 0, 0), ("FM", 2, 2, 0, 0), ("FMRC", 4, 2, 16, 4), ("FMRC", 6, 2, 64, 4), ("FMRC", 8, 2, 128, 4)],
        [("IM", 10, 2, 128, 4), ("IM", 8, 2, 64, 8), ("IM", 6, 2, 16, 8), ("IM", 4, 2, 4, 8), ("IM", 2, 2, 1, 8)]),
    "sp-f64-32-haar-L5": ([("FM", 0, 3, 0, 0), ("FMRC", 3, 2, 8, 1)],
        [("IM", 5, 3, 4, 1), ("IM", 2, 2, 1, 1)]),
    "sp-f64-64-haar-L6": ([("FM", 0, 3, 0, 0), ("FMRC", 3, 3, 8, 1)],
        [("IM", 6, 3, 8, 1), ("IM", 3, 3, 1, 1)]),
    "sp-f64-384-haar-L5": ([("FM", 0, 3, 0, 0), ("FMRC", 3, 2, 8, 4)],
        [("IM", 5, 3, 4, 4), ("IM", 2, 2, 1, 4)]),
    "sp-f64-384-haar-L6": ([("FM", 0, 3, 0, 0), ("FMRC", 3, 3, 8, 4)],
        [("IM", 6, 3, 8, 4), ("IM", 3, 3, 1, 4)]),
    "sp-f64-512-haar-L9": ([("FM", 0, 3, 0, 0), ("FMRC", 3, 3, 8, 4), ("FMRC", 6, 3, 64, 4)],
        [("IM", 9, 3, 64, 8), ("IM", 6, 3, 8, 8), ("IM", 3, 3, 1, 8)]),
    "sp-f64-4096-haar-L5": ([("FM", 0, 3, 0, 0), ("FMRC", 3, 2, 8, 8)],
        [("IM", 5, 3, 4, 8), ("IM", 2, 2, 1, 8)]),
    "sp-f64-4096-db2-L6": ([("FM", 0, 3, 0, 0), ("FMRC", 3, 3, 8, 8)],
        [("IM", 6, 3, 8, 8), ("IM", 3, 3, 1, 8)]),
    "sp-f64-24-db4-L2": ([("FM", 0, 2, 0, 0)],
        [("IM", 2, 2, 1, 1)]),
    "sp-f64-24-db2-L3": ([("FM", 0, 3, 0, 0)],
        [("IM", 3, 3, 1, 1)]),
    "sp-f64-384-db4-L2": ([("FM", 0, 2, 0, 0)],
        [("IM", 2, 2, 1, 4)]),
    "sp-f64-384-db2-L3": ([("FM", 0, 3, 0, 0)],
        [("IM", 3, 3, 1, 4)]),
    "sp-f64-512-db10-L2": ([("FM", 0, 2, 0, 0)],
        [("IM", 2, 2, 1, 8)]),
    "sp-f64-512-db2-L3": ([("FM", 0, 3, 0, 0)],
        [("IM", 3, 3, 1, 8)]),
    "sp-f32-384-db4-L6": ([("FM", 0, 2, 0, 0), ("FM", 2, 2, 0, 0), ("FMRC", 4, 2, 16, 4)],
        [("IM", 6, 2, 16, 4), ("IM", 4, 2, 4, 4), ("IM", 2, 2, 1, 4)]),
    "sp-f32-4096-db4-L6": ([("FM", 0, 2, 0, 0), ("FM", 2, 2, 0, 0), ("FMRC", 4, 2, 16, 8)],
        [("IM", 6, 2, 16, 8), ("IM", 4, 2, 4, 8), ("IM", 2, 2, 1, 8)]),
    "sp-f32-2048-haar-L9": ([("FM", 0, 3, 0, 0), ("FM", 3, 3, 0, 0), ("FMRC", 6, 3, 64, 4)],
        [("IM", 9, 3, 64, 8), ("IM", 6, 3, 8, 8), ("IM", 3, 3, 1, 8)]),
    "sp-f32-4096-haar-L9": ([("FM", 0, 3, 0, 0), ("FM", 3, 3, 0, 0), ("FMRC", 6, 3, 64, 8)],
        [("IM", 9, 3, 64, 8), ("IM", 6, 3, 8, 8), ("IM", 3, 3, 1, 8)]),
    "sp-f32-24-db4-L2": ([("FM", 0, 2, 0, 0)],
        [("IM", 2, 2, 1, 1)]),
    "sp-f32-32-haar-L3": ([("FM", 0, 3, 0, 0)],
        [("IM", 3, 3, 1, 1)]),
    "sp-f32-384-db4-L2": ([("FM", 0, 2, 0, 0)],
        [("IM", 2, 2, 1, 4)]),
    "sp-f32-384-db2-L3": ([("FM", 0, 3, 0, 0)],
        [("IM", 3, 3, 1, 4)]),
    "sp-f32-512-db10-L2": ([("FM", 0, 2, 0, 0)],
        [("IM", 2, 2, 1, 8)]),
    "sp-f32-512-db2-L3": ([("FM", 0, 3, 0, 0)],
        [("IM", 3, 3, 1, 8)]),
    "pd-f64-64-L4": ([("FTWO", 0, 2, 0, 0), ("FTWO", 2, 2, 0, 0)],
        [("IM", 4, 2, 4, 1), ("IM", 2, 2, 1, 1)]),
    "pd-f64-64-L3": ([("FTWO", 0, 2, 0, 0), ("FLVL", 2, 1, 0, 0)],
        [("IM", 3, 2, 2, 1), ("ILVL", 1, 1, 0, 0)]),
    "pd-f32-64-L3": ([("FTWO", 0, 2, 0, 0), ("FLVL", 2, 1, 0, 0)],
        [("IM", 3, 2, 2, 1), ("ILVL", 1, 1, 0, 0)]),
    "acpd-f64-64-L4": ([("FTWO", 0, 2, 0, 1), ("FTWO", 2, 2, 0, 1)],
        [("IACWPD", 4, 4, 0, 0)]),
    "acpd-f64-64-L3": ([("FTWO", 0, 2, 0, 1), ("FLVL", 2, 1, 0, 1)],
        [("IACWPD", 3, 3, 0, 0)]),
    "acp-f64-64-L4": ([("FLVL", 0, 1, 0, 1), ("FLVL", 1, 1, 0, 1), ("FLVL", 2, 1, 0, 1), ("FLVL", 3, 1, 0, 1)],
        [("IACWPT", 4, 4, 0, 0)]),
    "sp-f64-4096-haar-L1": ([("FLVL", 0, 1, 0, 0)],
        [("ITILE", 1, 1, 1, 0)]),
    "sp-f32-4096-db4-L1": ([("FLVL", 0, 1, 0, 0)],
        [("ITILE", 1, 1, 4, 0)]),
    "pd-f64-4096-pyramid-db4": ([("FTWO", 0, 2, 0, 0)],
        [("ITILE", 2, 1, 4, 0), ("ITILE", 1, 1, 4, 0)]),
    "pd-f64-4096-pyramid-db2": ([("FTWO", 0, 2, 0, 0)],
        [("ITILE", 2, 1, 2, 0), ("ITILE", 1, 1, 2, 0)]),
    "sp-f64-64-db4-sm5": ([("FM", 0, 2, 0, 0), ("FLVL", 2, 1, 0, 0)],
        [("ILVL", 3, 1, 0, 1), ("ILVL", 2, 1, 0, 1), ("ILVL", 1, 1, 0, 1)]),
    "sp-f64-1024-db4-L10": ([("FM", 0, 2, 0, 0), ("FM", 2, 2, 0, 0), ("FMRC", 4, 2, 16, 4), ("FDEEP", 6, 4, 0, 0)],
        [("IDEEP", 10, 4, 0, 0), ("IM", 6, 2, 16, 8), ("IM", 4, 2, 4, 8), ("IM", 2, 2, 1, 8)]),
    "pd-f64-1024-db4-L7": ([("FTWO", 0, 2, 0, 0), ("FTWO", 2, 2, 0, 0), ("FTWO", 4, 2, 0, 0), ("FDEEP", 6, 1, 1, 0)],
        [("IM", 7, 2, 32, 8), ("IM", 5, 2, 8, 8), ("IM", 3, 2, 2, 8), ("ILVL", 1, 1, 0, 0)]),
    "pd-f64-20488-L3": ([("FG", 0, 1, 0, 0), ("FG", 1, 1, 0, 0), ("FG", 2, 1, 0, 0)],
        None),
    "acpd-f64-20488-L3": ([("FG", 0, 1, 0, 1), ("FG", 1, 1, 0, 1), ("FG", 2, 1, 0, 1)],
        None),
    "acd-f64-20488-L3": ([("FG", 0, 1, 0, 1), ("FG", 1, 1, 0, 1), ("FG", 2, 1, 0, 1)],
        [("IACDWT", 3, 3, 0, 0)]),
    "sp-f32-40968-L3": ([("FG", 0, 1, 0, 0), ("FG", 1, 1, 0, 0), ("FG", 2, 1, 0, 0)],
        [("ILVL", 3, 1, 0, 0), ("ILVL", 2, 1, 0, 0), ("ILVL", 1, 1, 0, 0)]),
    "sp-f64-20488-L3": ([("FG", 0, 1, 0, 0), ("FG", 1, 1, 0, 0), ("FG", 2, 1, 0, 0)],
        [("ILVL", 3, 1, 0, 0), ("ILVL", 2, 1, 0, 0), ("ILVL", 1, 1, 0, 0)]),
    "sd-f64-20488-L3": ([("FG", 0, 1, 0, 0), ("FG", 1, 1, 0, 0), ("FG", 2, 1, 0, 0)],
        [("ILVL", 3, 1, 0, 0), ("ILVL", 2, 1, 0, 0), ("ILVL", 1, 1, 0, 0)]),
    "iswpd-full-64": (None,
        [("IM", 6, 2, 16, 1), ("IM", 4, 2, 4, 1), ("IM", 2, 2, 1, 1)]),
    "wrap-y-flvl": ([("FLVL", 0, 1, 0, 0)],
        None),
    "wrap-y-ftwo": ([("FTWO", 0, 2, 0, 0), ("FTWO", 2, 2, 0, 0)],
        None),
    "wrap-y-multi": ([("FM", 0, 3, 0, 0), ("FMRC", 3, 2, 8, 1)],
        [("IM", 5, 3, 4, 1), ("IM", 2, 2, 1, 1)]),
    "wrap-z-fg-dwt": ([("FG", 0, 1, 0, 0), ("FG", 1, 1, 0, 0)],
        None),
    "wrap-z-fg-wpd": ([("FG", 0, 1, 0, 0)],
        None),
    "wrap-x-ilvl": (None,
        [("ILVL", 2, 1, 0, 1), ("ILVL", 1, 1, 0, 1)]),
    "wrap-x-acdwt": (None,
        [("IACDWT", 2, 2, 0, 0)]),
    "wrap-x-acwpt": (None,
        [("IACWPT", 2, 2, 0, 0)]),
    "wrap-x-acwpd": (None,
        [("IACWPD", 2, 2, 0, 0)]),
    "wrap-x-itile": (None,
        [("ITILE", 1, 1, 4, 0)]),
    "wrap-x-fsd": ([("FSD", 0, 3, 8, 0)],
        [("ISD", 3, 3, 8, 0)]),
    "sp-f64-128-haar-L5": ([("FM", 0, 3, 0, 0), ("FMRC", 3, 2, 8, 2)],
        [("IM", 5, 3, 4, 2), ("IM", 2, 2, 1, 2)]),
    "sp-f64-128-haar-L6": ([("FM", 0, 3, 0, 0), ("FMRC", 3, 3, 8, 2)],
        [("IM", 6, 3, 8, 2), ("IM", 3, 3, 1, 2)]),
    "sp-f64-128-db4-L2": ([("FM", 0, 2, 0, 0)],
        [("IM", 2, 2, 1, 2)]),
    "sp-f64-128-db2-L3": ([("FM", 0, 3, 0, 0)],
        [("IM", 3, 3, 1, 2)]),
    "sp-f32-128-db4-L2": ([("FM", 0, 2, 0, 0)],
        [("IM", 2, 2, 1, 2)]),
    "sp-f32-128-db2-L3": ([("FM", 0, 3, 0, 0)],
        [("IM", 3, 3, 1, 2)]),
}

# rows per thread that can be reached (module docstring): (element size, K, OPT)
REACHED_FMRC = {(8, k, o) for k in (2, 3) for o in (1, 2, 4, 8)} | {(4, 2, 4), (4, 2, 8), (4, 3, 4), (4, 3, 8)}
REACHED_IM = {(e, k, o) for e in (8, 4) for k in (2, 3) for o in (1, 2, 4, 8)}


def _wt(wx, name):
    return wx.wavelet(name)


def _key(tr):
    return [(t.route, t.depth, t.K, t.R, t.OPT) for t in tr]


def _need(cid, which, tr):
    """the trace of a case against PINS[cid][which] (0 = forward, 1 = inverse)"""
    want = [tuple(w) for w in PINS[cid][which]]
    got = _key(tr)
    assert tr.dropped == 0
    assert got == want, "%s %s: written for %s, took %s" % (cid, ("forward", "inverse")[which], want, got)


def _noise(wx, shape, dtype, seed):
    import torch
    x = wx.jl_empty(shape, torch.float64 if dtype == F64 else torch.float32, "cuda")
    x.normal_(generator=torch.Generator(device="cuda").manual_seed(seed))
    return x


def _close_cols(got, exp, tol, what):
    """every column of every signal within tol of that column's own largest magnitude; arrays (n, columns[, signals])"""
    got = np.asarray(got, dtype=np.float64)
    exp = np.asarray(exp, dtype=np.float64)
    assert got.shape == exp.shape, (what, got.shape, exp.shape)
    err = np.abs(got - exp).max(axis=0)
    den = np.abs(exp).max(axis=0)
    rel = err / np.where(den > 0, den, 1.0)
    k = np.unravel_index(int(np.argmax(rel)), rel.shape) if rel.ndim else ()
    worst = float(rel[k]) if rel.ndim else float(rel)
    assert np.isfinite(got).all() and worst <= tol, "%s: column %s: error %.3g of the column's maximum (tolerance %.3g)" % (
        what, k, worst, tol)


def _stack(fn, X, *a):
    X = np.asarray(X, dtype=np.float64)
    return np.asfortranarray(np.stack([fn(np.asfortranarray(X[..., i]), *a) for i in range(X.shape[-1])], axis=-1))


def _fwd_fn(wx, kind):
    return {"dwt": wx.sdwtall, "wpt": wx.swptall, "wpd": wx.swpdall, "acdwt": wx.acdwtall, "acwpt": wx.acwptall, "acwpd": wx.acwpdall}[kind]


def _ofwd(oracle, kind, x, qmf, L):
    fn = {"dwt": oracle.sdwt, "wpt": oracle.swpt, "wpd": oracle.swpd, "acdwt": oracle.acdwt, "acwpt": oracle.acwpt, "acwpd": oracle.acwpd}[kind]
    return _stack(fn, x, qmf, L)


def _inv(wx, kind, xw, wt, arg=None, sm=None):
    if kind == "dwt":
        return wx.isdwtall(xw, wt, sm)
    if kind == "wpt":
        return wx.iswptall(xw, wt, sm)
    if kind == "wpd":
        return wx.iswpdall(xw, wt, arg, sm)
    if kind == "acdwt":
        return wx.iacdwtall(xw)
    if kind == "acwpt":
        return wx.iacwptall(xw)
    return wx.iacwpdall(xw, arg)


def _oinv(oracle, kind, xw, qmf, arg=None, sm=None):
    if kind == "dwt":
        return _stack(oracle.isdwt, xw, qmf, sm)
    if kind == "wpt":
        return _stack(oracle.iswpt, xw, qmf, sm)
    if kind == "wpd":
        return _stack(oracle.iswpd, xw, qmf, arg, sm)
    if kind == "acdwt":
        return _stack(oracle.iacdwt, xw)
    if kind == "acwpt":
        return _stack(oracle.iacwpt, xw)
    return _stack(oracle.iacwpd, xw, arg)


def _inv_args(wx, c):
    """(tree or depth argument of iswpd / iacwpd, shift) of a case's inverse"""
    arg = None
    if c.kind in ("wpd", "acwpd"):
        arg = wx.maketree(c.n, c.L, "dwt") if c.inv == "pyramid" else (wx.maketree(c.n, c.L, "full") if c.kind == "acwpd" else c.L)
    return arg, (c.inv if isinstance(c.inv, int) else None)


class _forced:
    """wx.set_force_generic(1) for a block: one level per launch"""

    def __init__(self, wx):
        self.wx = wx

    def __enter__(self):
        self.wx.set_force_generic(1)

    def __exit__(self, *exc):
        self.wx.set_force_generic(0)


@gpu
@pytest.mark.parametrize("cid", [c.id for c in CASES_A])
def test_route_and_parity(wx, oracle, cid):
    c = CASE_BY_ID[cid]
    if c.dtype == F32:
        assert c.L <= int(np.log2(c.n)) - 2
    wt = _wt(wx, c.wname)
    tol = TOL[np.dtype(c.dtype)]
    agree = 1e-13 if c.dtype == F64 else tol
    x = _noise(wx, (c.n, c.B), c.dtype, 7000 + c.n + c.L)
    fwd = _fwd_fn(wx, c.kind)
    with wx.swt1d_trace() as tr:
        got = fwd(x, wt, c.L)
    _need(cid, 0, tr)
    xh = wx.to_numpy(x)
    goth = wx.to_numpy(got)
    assert goth.dtype == c.dtype
    exp = _ofwd(oracle, c.kind, xh, wt.qmf, c.L)
    _close_cols(goth, exp, tol, cid + " forward")
    if c.forced:
        with _forced(wx), wx.swt1d_trace() as trf:
            ref = wx.to_numpy(fwd(x, wt, c.L))
        assert {t.route for t in trf} <= FWD_GENERIC, (cid, _key(trf))
        _close_cols(goth, ref, agree, cid + " forward against one level per launch")
    if c.inv is None:
        return
    # the inverse of the oracle's coefficients, in the case's type
    coef = np.asfortranarray(exp, dtype=c.dtype)
    cd = wx.to_device(coef)
    arg, sm = _inv_args(wx, c)
    with wx.swt1d_trace() as tr:
        back = _inv(wx, c.kind, cd, wt, arg, sm)
    _need(cid, 1, tr)
    backh = wx.to_numpy(back)
    assert backh.dtype == c.dtype
    _close_cols(backh, _oinv(oracle, c.kind, coef, wt.qmf, arg, sm), tol, cid + " inverse against the oracle")
    _close_cols(backh, xh, 20 * tol, cid + " inverse against the signal")
    if c.forced:
        with _forced(wx), wx.swt1d_trace() as trf:
            ref = wx.to_numpy(_inv(wx, c.kind, cd, wt, arg, sm))
        assert {t.route for t in trf} <= INV_GENERIC, (cid, _key(trf))
        _close_cols(backh, ref, agree, cid + " inverse against one level per launch")


def test_pins_cover_every_route_and_rows_per_thread():
    """the table itself: every route of csrc/wx_debug.h but the two Haar passes, both types where the route has both, every
    reached (K, OPT) of FMRC and IM, two HF of ITILE in three containers, both ILVL modes, FTWO followed and not followed by FLVL"""
    seen, fmrc, im, tile = set(), set(), set(), set()
    for cid, (f, i) in PINS.items():
        if cid not in CASE_BY_ID:
            continue
        c = CASE_BY_ID[cid]
        es = np.dtype(c.dtype).itemsize
        for (r, d, K, R, OPT) in list(f) + list(i or []):
            seen.add((r, es))
            if r == "FMRC":
                fmrc.add((es, K, OPT))
            if r == "IM":
                im.add((es, K, OPT))
            if r == "ITILE":
                tile.add((c.kind, R))
            if r == "ILVL":
                seen.add(("ILVL-shift" if OPT else "ILVL-average", es))
            if r in ("FSD", "FSDIP", "ISD"):
                seen.add((r + ("-runtime" if R == 0 else "-taps"), es))
            if r == "ISD":
                seen.add(("ISD-pipelined" if OPT else "ISD-plain", es))
    both = ["FG", "FSD", "FSDIP", "FTWO", "FLVL", "FM", "FMRC", "ISD", "ISDIP", "IM", "ITILE", "ILVL"]
    for r in both:
        assert (r, 8) in seen and (r, 4) in seen, r
    for r in ("FDEEP", "IDEEP", "IACDWT", "IACWPT", "IACWPD", "FSD-runtime", "FSD-taps", "FSDIP-runtime", "FSDIP-taps", "ISD-runtime", "ISD-taps",
              "ISD-pipelined", "ISD-plain", "ILVL-shift", "ILVL-average"):
        assert (r, 8) in seen, r
    assert fmrc == REACHED_FMRC, sorted(fmrc ^ REACHED_FMRC)
    assert im == REACHED_IM, sorted(im ^ REACHED_IM)
    assert {k for k, _ in tile} == {"dwt", "wpt", "wpd"} and len({h for _, h in tile}) >= 2, tile
    two = {cid: [r for (r, *_) in PINS[cid][0]] for cid in ("pd-f64-64-L4", "pd-f64-64-L3", "acpd-f64-64-L4", "acpd-f64-64-L3")}
    assert two["pd-f64-64-L4"] == two["acpd-f64-64-L4"] == ["FTWO", "FTWO"]
    assert two["pd-f64-64-L3"] == two["acpd-f64-64-L3"] == ["FTWO", "FLVL"]


@gpu
def test_iswpd_of_a_full_tree_takes_the_fused_iswpt_passes(wx, oracle):
    """a full tree reads only its leaves: the fused iswpt passes at a column offset with the table's signal stride; bit-equal to
    iswptall of the leaf columns"""
    n, L, B = 64, 6, 3
    wt = _wt(wx, "db4")
    x = _noise(wx, (n, B), F64, 7100)
    xh = wx.to_numpy(x)
    coef = _ofwd(oracle, "wpd", xh, wt.qmf, L)
    cd = wx.to_device(coef)
    leaves = wx.to_device(np.asfortranarray(coef[:, (1 << L) - 1:, :]))
    with wx.swt1d_trace() as tr:
        back = wx.iswpdall(cd, wt)
    _need("iswpd-full-64", 1, tr)
    with wx.swt1d_trace() as tr2:
        back2 = wx.iswptall(leaves, wt)
    assert _key(tr2) == _key(tr) and {t.route for t in tr} == {"IM"}, (_key(tr), _key(tr2))
    import torch
    assert torch.equal(back, back2)
    _close_cols(wx.to_numpy(back), _oinv(oracle, "wpd", coef, wt.qmf, None, None), TOL[np.dtype(F64)], "iswpd of a full tree")
    _close_cols(wx.to_numpy(back), xh, 20 * TOL[np.dtype(F64)], "iswpd of a full tree against the signal")


# ---- b. shifts and trees -----------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("n,dtype", [(64, F64), (4096, F64), (4096, F32)], ids=["64-f64", "4096-f64", "4096-f32"])
def test_shift_based_inverse_every_shift(wx, oracle, n, dtype):
    """isdwt and iswpt for every shift at L = 3, on a length whose average-based iswpt is fused (64) and one whose average-based
    levels run out of LDS tiles (4096): with a shift every level is the per-sample kernel"""
    L, B = 3, 2
    wt = _wt(wx, "db4")
    tol = TOL[np.dtype(dtype)]
    x = _noise(wx, (n, B), dtype, 7200 + n)
    xh = wx.to_numpy(x)
    want = [("ILVL", d, 1, 0, 1) for d in (3, 2, 1)]
    for kind, shifts in (("dwt", range(1, 1 << L)), ("wpt", range(1 << L))):
        coef = np.asfortranarray(_ofwd(oracle, kind, xh, wt.qmf, L), dtype=dtype)
        cd = wx.to_device(coef)
        for sm in shifts:
            with wx.swt1d_trace() as tr:
                back = wx.to_numpy(_inv(wx, kind, cd, wt, None, sm))
            assert _key(tr) == want, "%s sm=%d: written for %s, took %s" % (kind, sm, want, _key(tr))
            what = "shift inverse %s n=%d sm=%d" % (kind, n, sm)
            _close_cols(back, _oinv(oracle, kind, coef, wt.qmf, None, sm), tol, what + " against the oracle")
            _close_cols(back, xh, 20 * tol, what + " against the signal")


def _clip(tree, L):
    tree = tree.copy()
    tree[(1 << L) - 1:] = False
    return tree


def _tdepth(tree):
    return max(int(np.floor(np.log2(i + 1))) for i in np.flatnonzero(tree)) + 1


@gpu
def test_iswpd_trees_with_and_without_shift(wx, oracle):
    """iswpd along the pyramid, two random trees and a full tree shallower than the table, average based and with the first and
    the last shift: a sparse tree stays in the wpd container on single levels, and so does the shallow full tree once it has a
    shift (its shifts follow the table's depth, not the tree's)"""
    n, L, B = 64, 4, 2
    rng = np.random.default_rng(7300)
    wt = _wt(wx, "db4")
    tol = TOL[np.dtype(F64)]
    x = _noise(wx, (n, B), F64, 7300)
    xh = wx.to_numpy(x)
    coef = _ofwd(oracle, "wpd", xh, wt.qmf, L)
    cd = wx.to_device(coef)
    trees = [("pyramid", _clip(wx.maketree(n, L, "dwt"), L))]
    for p in (0.7, 0.5):
        t = _clip(random_tree_1d(n, rng, p), L)
        while not (t[0] and t[1:3].any() and not t[:(1 << _tdepth(t)) - 1].all()):          # deeper than one level, and sparse
            t = _clip(random_tree_1d(n, rng, p), L)
        trees.append(("random %.1f" % p, t))
    trees.append(("full depth 2", wx.maketree(n, 2, "full")))
    for name, tree in trees:
        depth = _tdepth(tree)
        for sm in (None, 0, (1 << L) - 1):
            with wx.swt1d_trace() as tr:
                back = wx.to_numpy(wx.iswpdall(cd, wt, tree, sm))
            routes = _key(tr)
            if name == "full depth 2" and sm is None:
                assert routes == [("IM", 2, 2, 1, 1)], routes                                  # leaves only: the iswpt passes
            else:
                want = [("ILVL", d, 1, 0, 0 if sm is None else 1) for d in range(depth, 0, -1)]
                assert routes == want, "%s sm=%s: written for %s, took %s" % (name, sm, want, routes)
            what = "iswpd %s sm=%s" % (name, sm)
            _close_cols(back, _oinv(oracle, "wpd", coef, wt.qmf, tree, sm), tol, what + " against the oracle")
            _close_cols(back, xh, 20 * tol, what + " against the signal")


# ---- c. every wrap-around loop goes round once ------------------------------------------------------------------------------
def _copies(wx, n, B, dtype, seed):
    """(n, B) device signals: white noise for b < P, signal b mod P for the others; and the index b mod P"""
    import torch
    base = _noise(wx, (n, P), dtype, seed)
    idx = torch.arange(B, device="cuda") % P
    x = wx.jl_empty((n, B), base.dtype, "cuda")
    x.copy_(base.index_select(1, idx))
    return x, idx


def _same_as_original(out, idx):
    """every signal's output bit-identical to that of the signal it copies"""
    import torch
    B = out.shape[-1]
    flat = out.reshape(-1, B) if out.dim() > 1 else out
    step = 8192
    for b0 in range(P, B, step):
        sl = slice(b0, min(B, b0 + step))
        if not torch.equal(flat[..., sl], flat.index_select(-1, idx[sl])):
            return False
    return True


def _wrap_check(wx, oracle, cid, kind, dtype, n, L, wname, B, cap, dim, jobs, sigcap, inv=None, sm=None, fwd=True):
    """forward (fwd) and inverse (inv) of B copies: the recorded grid dimension `dim` is the cap, below the `jobs` it serves;
    signals 0, P - 1, sigcap - 1, sigcap (the first signal past the cap) and the last against the oracle"""
    wt = _wt(wx, wname)
    tol = TOL[np.dtype(dtype)]
    assert cap < jobs and P < sigcap < B
    x, idx = _copies(wx, n, B, dtype, 7400 + n + B)
    sel = sorted({0, P - 1, sigcap - 1, sigcap, B - 1})
    xs = wx.to_numpy(x[:, sel])
    if fwd:
        with wx.swt1d_trace() as tr:
            xw = _fwd_fn(wx, kind)(x, wt, L)
        _need(cid, 0, tr)
        assert max(getattr(t, dim) for t in tr) == cap, (cid, list(tr))
        assert _same_as_original(xw, idx), cid + ": a copy's forward output differs from its original's"
        ws = wx.to_numpy(xw[..., sel])
        _close_cols(ws, _ofwd(oracle, kind, xs, wt.qmf, L), tol, cid + " forward")
    else:
        xw = wx.to_device(np.asfortranarray(_ofwd(oracle, kind, wx.to_numpy(x[:, :P]), wt.qmf, L), dtype=dtype)).index_select(-1, idx)
        xw = wx.to_colmajor(xw)
        ws = wx.to_numpy(xw[..., sel])
    if inv is None:
        return
    arg = wx.maketree(n, L, "full") if kind == "acwpd" else None
    with wx.swt1d_trace() as tr:
        back = _inv(wx, kind, xw, wt, arg, sm)
    _need(cid, 1, tr)
    assert max(getattr(t, dim) for t in tr) == cap, (cid, list(tr))
    assert _same_as_original(back, idx), cid + ": a copy's inverse output differs from its original's"
    bs = wx.to_numpy(back[:, sel])
    _close_cols(bs, _oinv(oracle, kind, ws, wt.qmf, arg, sm), tol, cid + " inverse against the oracle")
    _close_cols(bs, xs, 20 * tol, cid + " inverse against the signal")


@gpu
def test_blockidx_y_wraps_forward_level(wx, oracle):
    """sdwt n = 8, L = 1: k_swt_fwd_level with 65543 signals on a grid.y of 65535"""
    _wrap_check(wx, oracle, "wrap-y-flvl", "dwt", F64, 8, 1, "db2", 65543, 65535, "grid_y", 65543, 65535)


@gpu
def test_blockidx_y_wraps_two_level_swpd(wx, oracle):
    """swpd n = 16, L = 4: k_swpd_fwd_two twice, 65543 signals on a grid.y of 65535"""
    _wrap_check(wx, oracle, "wrap-y-ftwo", "wpd", F64, 16, 4, "db2", 65543, 65535, "grid_y", 65543, 65535)


@gpu
def test_blockidx_y_wraps_fused_swpt_passes(wx, oracle):
    """Haar swpt / iswpt n = 32, L = 5: k_swt_fwd_multi, k_swt_fwd_multi_rc and two k_swt_inv_multi passes, 65543 signals"""
    _wrap_check(wx, oracle, "wrap-y-multi", "wpt", F64, 32, 5, "haar", 65543, 65535, "grid_y", 65543, 65535, inv="avg")


@gpu
@pytest.mark.parametrize("kind,L", [("dwt", 2), ("wpd", 1)])
def test_blockidx_z_wraps_global_level(wx, oracle, kind, L):
    """n = 20488 Float64 (no power of two, more than a CU's LDS): k_swt_fwd_level_g with 1031 signals on a grid.z of 1024"""
    _wrap_check(wx, oracle, "wrap-z-fg-" + kind, kind, F64, 20488, L, "db4", 1031, 1024, "grid_z", 1031, 1024)


@gpu
def test_grid_stride_wraps_shift_based_level(wx, oracle):
    """iswpt n = 1024, L = 2, sm = 1, 1030 signals: k_swt_inv_level at depth 1 has 1030 * 2 * 512 > 2^20 samples for 4096 workgroups"""
    assert 1030 * 2 * 512 > 4096 * 256
    _wrap_check(wx, oracle, "wrap-x-ilvl", "wpt", F64, 1024, 2, "db4", 1030, 4096, "grid_x", 1030 * 2 * 512 // 256, 1024, inv=1, sm=1, fwd=False)


@gpu
@pytest.mark.parametrize("kind", ["acdwt", "acwpt", "acwpd"])
def test_grid_stride_wraps_autocorrelation_inverse(wx, oracle, kind):
    """n = 256, L = 2, 4101 signals: 4101 * 256 > 2^20 output samples for the 4096 workgroups of k_iacdwt / k_iacwpt / k_iacwpd"""
    assert 4101 * 256 > 4096 * 256
    _wrap_check(wx, oracle, "wrap-x-" + kind, kind, F64, 256, 2, "db4", 4101, 4096, "grid_x", 4101, 4096, inv="avg", fwd=False)


@gpu
def test_unit_loop_wraps_tile_inverse(wx, oracle):
    """iswpt n = 4096, L = 1, 1030 signals: 2060 tiles of 2048 samples for the 2048 workgroups of k_swt_inv_level_tile"""
    assert 1030 * 4096 // 2048 > 2048
    _wrap_check(wx, oracle, "wrap-x-itile", "wpt", F64, 4096, 1, "db4", 1030, 2048, "grid_x", 1030 * 2, 1024, inv="avg", fwd=False)


@gpu
def test_signal_loop_wraps_fused_sdwt_isdwt(wx, oracle):
    """sdwt / isdwt n = 64, L = 3, 2052 signals: the signal loops of k_sdwt_fused and k_isdwt_avg_fused on 2048 workgroups"""
    _wrap_check(wx, oracle, "wrap-x-fsd", "dwt", F64, 64, 3, "db4", 2052, 2048, "grid_x", 2052, 2048, inv="avg")


# ---- d. the inverse schedule, no device ---------------------------------------------------------------------------------------
def _plan_of(pins):
    """the schedule a pinned inverse trace implies; None for the routes that do not go through the schedule"""
    plan = []
    for (r, d, K, R, OPT) in pins:
        if r == "IM":
            plan.append((d, d - K, R, OPT))
        elif r == "IDEEP":
            plan.append((d, d - K, 64, -1))
        elif r in ("ITILE", "ILVL"):
            plan.append((d, d - 1, 0, 1))
        else:
            return None
    return plan


def test_inverse_schedules_of_part_a(wx):
    checked = 0
    for c in CASES_A:
        if c.inv is None or c.kind.startswith("ac"):
            continue
        want = _plan_of(PINS[c.id][1])
        if want is None:
            continue
        layout, has_tree = c.kind, c.inv == "pyramid"
        if c.kind == "wpd" and not has_tree:
            layout = "wpt"                                                  # a full tree: the iswpt layout at a column offset
        sm = c.inv if isinstance(c.inv, int) else None
        got = wx.swt_inv_plan(layout, c.L, FLEN[c.wname], c.n, np.dtype(c.dtype).itemsize, sm=sm, has_tree=has_tree)
        assert got == want, "%s: schedule %s, the pinned trace implies %s" % (c.id, got, want)
        checked += 1
    assert checked >= 30
    with _forced(wx):
        assert wx.swt_inv_plan("wpt", 5, 2, 32, 8) == [(d, d - 1, 0, 1) for d in range(5, 0, -1)]
    assert wx.swt_inv_plan("wpt", 5, 2, 32, 8) == [(5, 2, 4, 1), (2, 0, 1, 1)]
    # the Haar register pass, as the caller asks for it at the benchmarked geometry
    assert wx.swt_inv_plan("wpt", 12, 2, 16384, 8, haar6=True)[0] == (12, 7, 64, 0)
