"""GPU parity of the 2-D decimated transforms (wpd, wpt, iwpt, iwpd, dwt / idwt of images: csrc/wx_api_2d.hip, wx_dwt2d.hip,
wx_lattice_2d64*, wx_lattice_rows.h, wx_lattice2d.h, wx_pyr2d.hip, wx_dwttail.hip) on every launch route.

One public call ends in one of about a dozen kernel families and, inside them, in one of a few hundred template instances,
chosen by image shape, type, filter length, depth, tree shape, in place or not, and batch parity.  Every case here runs the
public entry point on device tensors inside `wx.dwt2d_trace()` -- the record the launchers themselves write next to each launch
(csrc/wx_debug.h) -- and fails if the sequence of (route, depth, K, extras) is not the one written out in PINS (grids, block sizes
and LDS bytes are recorded but not pinned), then compares with the CPU oracle.  The oracle always runs in Float64 on the case's own
values (also for Float32 cases); every image is compared against that image's own largest magnitude at helpers.TOL (1e-10 / 1e-5),
the Float32 lattice cases (Case.tol) at the 2e-6 (256 x 256 at depth 5, 512 x 512 at depth 6) / 3e-6 (deeper, 1024 x 1024) that
test_gpu_bench_geometry.py holds for the same kernels; inputs are white noise.

  a. test_route_and_parity: one case per route and per reachable template instance, forward and inverse, both types where both
     are built, 1 to 3 images.  A sample of the full trees -- one case at least per fused route and geometry: Q64, LROWS at
     each SH, ROWS with and without in place and register levels, L2DF at 256 / 512 / 1024, L2DC, full trees on tile levels
     (forced=True) -- repeats the call under wx.set_force_generic(1), which must record two-pass levels (TWO) only and agree
     to 1e-13 (Float64) / TOL (Float32).
     set_force_generic is read in wx_api_2d.hip only: trees that are not full and wpd keep their tile levels under it
     (wx_dev_wpt2d: `if (status) {`, wx_dev_wpd2d: `if (wx_launch_level_tile<T>(...)) continue;`), so those cases are not repeated.
  b. test_grid_loops_go_round: every launcher that caps its grid, with more work items than workgroups (asserted from the
     recorded grid): images b >= 251 are copies of image b mod 251, every output image must be bit-identical to that of its
     original, and the first 251 are compared with the oracle.
  c. test_pins_cover_what_the_docstring_declares_reachable: the (route, type, direction, instance) keys pinned in a and b ==
     REACHABLE, which _reachable() writes out by hand from the launchers' switches and the conditions quoted below (it is not
     taken from a record: a reachable instance without a case fails this test).

Routes (csrc/wx_debug.h) and the cases that pin them; NS = lattice stages = F / 2 rounded up to 1, 2, 4, 6, 8, 10:
  Q64W      wpd of 64 x 64 images, F <= 8: q64w-*-F2 .. F8 (NS 1, 2, 4); 10 taps decline: q64w-*-F10 (tile levels, whole image)
  Q64       full trees on 64 x 64, F <= 16: q64-*-F2 .. F16 (NS 1 .. 8), six levels q64-*-F6-L6; iwpd of a full tree reads slice L
            of the table (q64w-*); 18 / 20 taps decline to COL1D + ROWS (q64-*-F18, -F20); y is x still takes it (ip64-*-full)
  Q64TPREP + Q64T   any other tree on 64 x 64 whose root is split, F <= 16, x is not y: q64t-*-F2 .. F16; 18 taps: q64t-*-F18
            (tile levels, then two-pass levels below 8 x 8).  y is x: ip64-*-tree (tile levels), ip64-*-dwt (PYR).
            The pyramid policy (`pyramid && wx_pyr2d_small_ok && !(q64 && (!INVERSE || Ld <= 4 || F > 8))`): forward pyramids
            take Q64T for the levels down to 8 x 8 and TAIL for the rest (dwt64-*-F8-L3 .. L6: 0 .. 3 tail levels); inverse
            pyramids take Q64T up to four levels or above 8 taps (dwt64-*-F8-L3, -L4, dwt64-*-F10-L4, -L6) and PYR otherwise
            (dwt64-*-F8-L5, -L6); 18 taps: PYR both ways (dwt64-*-F18-L6)
  PYR       the whole pyramid of a small image in LDS, compile-time taps 2 .. 8 or runtime: pyr-*-F2 .. F10, 4 x 4 images pyr-*-4x4
  TAIL      lane-local levels below 8 x 8 of a forward pyramid, every F of its switch, 1 to 3 levels: tail-*-F2 .. F20 (128 x 128:
            tile levels by node list, two-pass levels by node list, TAIL; the inverse starts with COPYB)
  L2DF      Float32 256 x 256 / 512 x 512 / 1024 x 1024 (HB 1 / 0 / 2) at depths 5.. / 6.. / 7..: every NS at the base depth
            (E = 0: l2d-256-F*, -B2, l2d-512-F*, -L6, l2d-1024-F*, -L7) and one to three levels deeper (E = 1: l2d-*-deep,
            l2d-256-L8, l2d-512-F4-L9, l2d-1024-F4-L8); even and odd batches of 256 x 256 (l2d-256-B2, -B3: 1 and 2 units), one image
            (l2d-256-B1: `batch < per`, strips).  No case has more than one piece (65534 units: more than 100 MB).
  L2DC      the two-launch form, taken where the fused launcher declines: 256 x 256 forward with deep levels
            (`if constexpr (HB == 1) return 0;`: l2d-256-*-deep, l2d-256-L8) and with 18 / 20 taps (`HB == 1 && NSS == 10`:
            l2d-256-F20)
  COL1D + LROWS   Float64 full trees of 128 / 256 / 512 columns (SH 5 / 4 / 3): every NS at each SH (lrows-128-F*, lrows-256-F*,
            lrows-256-L2, lrows-512-F*, -L6, -W), full depth of 256 x 256 (lrows-256x256-L8); they decline -- ROWS runs -- below
            `L + SH < 6` (lrows-256-L1, -odd), below `SH < wx_rows_minsh(L)` (512 columns, fewer than 6 levels: lrows-512-L5),
            with fewer rows than a wavefront takes (`m < per`: rows-f64-8x128, -8x256) and above 16 taps (lrows-128-F20)
  COL1D + ROWS    k_rows_fused<T, F, INVERSE, V, KI, REGL> with strips (R, S): every wx_rows_geometry outcome per type
            (rows-*-8x8 .. 8x1024), every F (rows-*-16x32-F2 .. F20: V = VW up to 12 taps, V = 1 above), in place (KI = 2) with
            and without register levels for every F <= 8 (rows-*-8x256-F*, rows-*-8x1024-F*, rows-*-8x256, -8x1024),
            a strided input (iwpd reads slice L: rows-*-iwpd-16x32, wpd-*-128x64*), an input one element past a 16-byte boundary
            (off=True: WxIO re-aligns it, the vector instance still runs)
  TILEP / TILE    forward tile level, persistent or not; (by_node, status): wpd (0, 0) every F (wpd-*-128x64*, wpd-*-tile: an
            image of one tile); trees by node list (1, 1) every F with nodes larger than and equal to a tile (tile-*-F*); whole-image
            walk (0, 1) every F with nodes smaller than a tile that cover half of the image (tile-*-walk-F*); random trees
            (tile-*-rand, -deep), full trees whose rows are too long for the strips (tile-*-long)
  ITILEP / ITILE  the inverse mirror, the same cases; ITILEP is Float64 up to 8 taps by node list
  TWO       two-pass level: without a tree (0, 1, 0) under set_force_generic(1), for wpd levels below 8 x 8 (wpd-*-128x64) and on
            sides that are no power of two (wpd-*-24x8); by node list with (1, 1, 1: the root, which copies the other blocks)
            and without copy (1, 0, 1): two-*-24x8, -24x8-tree, -4x4, and below the tile levels of every deep tree
  COPYB     ahead of the two-pass levels of an inverse that ends in tile levels (tail-*, tile-*-rand, -deep, q64t-*-F18)
  GATHER    iwpd along a tree that is not full: q64w-*-tree, wpd-*-128-tree

Not reachable from any public call.  The template instances that earlier versions of this list named are no longer built; the
proofs, with the conditions as they stood, are in profiles/dwt2d_routes.md ("Removed as unreachable"):
  * k_rows_fused: V = 1 up to 12 taps and V = VW above (the launcher answers WX_EUNSUPPORTED for rows, strides or pointers off the
    16-byte vectors: wx_fused1d_ok leaves m a power of two >= 8, wx_rows_geometry ends at `R > VW` / `(R + R / 4) % VW == 0`, WxIO
    re-aligns device pointers, the scratch images come from the allocator), KI = 1, register levels without in place, in place
    without register levels in Float64; KI > 0 or REGL above 8 taps was never instantiated (`filt.F <= 8` in `inplace`).
  * k_dwt2d_level_tile_p above 10 taps and in Float32 at 10 taps (NBP = (80 * 80 + 255) / 256 = 25: `if constexpr (NBP <= 24 && F <=
    10)`); k_idwt2d_level_tile_p in Float32 and above 8 taps (`if constexpr (NBP <= 24 && F <= 8 && sizeof(T) == 8)`).
  * L2DC at 512 x 512 and 1024 x 1024, and in the inverse (k_lat2d_icolT_f32): only the diagnostic knob WX_L2D_FUSED, which is gone,
    reached them; the fused launcher declines only `if constexpr (HB == 1)` forward instances, which take the 256 x 256 forward
    pair (wx_lattice2d_launch_256), and `batch < per`, misaligned pointers and in-place odd batches, which the pair declines too.
  * k_lat2d64_wpd<3>: `wx_lat_stages_of(int ns) { return ns <= 2 ? ns : ((ns + 1) & ~1); }` never returns 3 (6 taps run NS = 4).
Still built though unreachable, because they are paths inside kernels that run (removing them would change those kernels):
  * LROWS in Float32 is compiled out at the call (`if constexpr (sizeof(T) == 8)` in wx_launch_rows); LROWS at 1024 columns:
    `n == 512 ? 3 : (n == 256 ? 4 : (n == 128 ? 5 : -1))`.
  * TILEP with (by_node, status) = (0, 1), the whole-image walk under a tree status without a node list in the persistent kernels:
    `if (!tt.status || by_node)`; (1, 0) in TILE and TILEP: `by_node = tt.status && tt.act && ...`.
  * ITILE / ITILEP without a tree status: `if (!wx_level_tile_ok<T>(m, n, d, filt.F) || !tt.status) return false;`; ITILEP without a
    node list: `if (by_node)`.
  * TWO with a tree status and no node list (0, *, 1), the `status` branch of k_dwt2d_dim1 / _dim2 without `act`: wx_api_2d.hip sets
    `htree` wherever it sets `dstatus`, and wx_dev_wpt2d answers WX_EUNSUPPORTED for a status without it.
Reachable and not pinned here, each for its size: L2DF with more than one piece (a batch of more than 65534 units) and the
host loop `for (int64_t b0 = 0; b0 < batch; b0 += 65535)` of TILE / ITILE (more than 65535 images of at least one tile: 2 GB).
The persistent loop of L2DF, the ticket ring of its second pass, and batches beyond one ring are the subject of
test_gpu_bench_geometry.py and test_gpu_fused2d_stress.py.  Grid loops: the one-wavefront kernels, TAIL, LROWS, TILE / ITILE (up
to 65535 images per launch) and L2DC launch one workgroup per work item (no cap, no loop in the kernel); TWO (without and with a
node list), TILEP, ITILEP, ROWS, PYR, COPYB and GATHER are capped and wrapped in part b."""
import numpy as np
import pytest

from helpers import TOL, random_tree_2d

gpu = pytest.mark.gpu
F64, F32 = np.float64, np.float32
WF = {2: "haar", 4: "db2", 6: "db3", 8: "db4", 10: "db5", 12: "db6", 14: "db7", 16: "db8", 18: "db9", 20: "db10"}
P = 251                                                   # part b: images b >= P are copies of image b mod P


class Case:
    """op: "wpt" (arg = depth of a full tree, or a tree spec), "dwt" (arg = depth of the pyramid, through dwtall / idwtall),
    "wpd" (arg = depth; the inverse is iwpdall along `iarg`, default the full tree of that depth).  A tree spec is ("dwt", L),
    ("nodes", [heap indices of the decomposed nodes]) or ("rand", p, depth, seed).  inplace: one image through wpt_ / iwpt_
    with y is x.  off: the inverse's input starts one element past a 16-byte boundary.  tol: where an existing test holds a
    tighter figure than helpers.TOL for the same kernel."""

    def __init__(self, cid, op, dtype, m, n, arg, F, B=2, forced=False, inplace=False, off=False, iarg=None, tol=None):
        self.id, self.op, self.dtype, self.m, self.n, self.arg, self.F, self.B = cid, op, dtype, m, n, arg, F, B
        self.forced, self.inplace, self.off, self.iarg, self.tol = forced, inplace, off, iarg, tol


def _t(dtype):
    return "f64" if dtype == F64 else "f32"


CASES_A = []
# ---- the one-wavefront 64 x 64 kernels ------------------------------------------------------------------------------------------
for _dt in (F64, F32):
    for _F in (2, 4, 8, 12, 16):                          # lattice stages 1, 2, 4, 6, 8
        CASES_A.append(Case("q64-%s-F%d" % (_t(_dt), _F), "wpt", _dt, 64, 64, 3, _F, B=3, forced=_F == 8))
    CASES_A.append(Case("q64-%s-F6-L6" % _t(_dt), "wpt", _dt, 64, 64, 6, 6, B=2))
    CASES_A.append(Case("q64-%s-F20" % _t(_dt), "wpt", _dt, 64, 64, 2, 20, B=2))          # 10 stages: not built, the LDS strips
    CASES_A.append(Case("q64-%s-F18" % _t(_dt), "wpt", _dt, 64, 64, 2, 18, B=2))
    for _F in (2, 4, 6, 8, 10):                           # wpd in one pass: up to 8 taps
        CASES_A.append(Case("q64w-%s-F%d" % (_t(_dt), _F), "wpd", _dt, 64, 64, 3, _F, B=3))
    CASES_A.append(Case("q64w-%s-tree" % _t(_dt), "wpd", _dt, 64, 64, 3, 8, B=2, iarg=("rand", 0.6, 3, 11)))   # iwpd: gather
    for _F in (2, 4, 8, 12, 16):
        CASES_A.append(Case("q64t-%s-F%d" % (_t(_dt), _F), "wpt", _dt, 64, 64, ("rand", 0.6, 4, 5 + _F), _F, B=3))
    CASES_A.append(Case("q64t-%s-F18" % _t(_dt), "wpt", _dt, 64, 64, ("rand", 0.6, 3, 23), 18, B=2))   # q64 wants F <= 16: tile levels
    # the pyramid policy around 64 x 64
    for _L in (3, 4, 5, 6):
        CASES_A.append(Case("dwt64-%s-F8-L%d" % (_t(_dt), _L), "dwt", _dt, 64, 64, _L, 8, B=3))
    CASES_A.append(Case("dwt64-%s-F10-L6" % _t(_dt), "dwt", _dt, 64, 64, 6, 10, B=3))
    CASES_A.append(Case("dwt64-%s-F10-L4" % _t(_dt), "dwt", _dt, 64, 64, 4, 10, B=2))
    CASES_A.append(Case("dwt64-%s-F18-L6" % _t(_dt), "dwt", _dt, 64, 64, 6, 18, B=2))
    # y is x: the one-wavefront tree kernel declines
    CASES_A.append(Case("ip64-%s-dwt" % _t(_dt), "wpt", _dt, 64, 64, ("dwt", 6), 8, B=1, inplace=True))
    CASES_A.append(Case("ip64-%s-tree" % _t(_dt), "wpt", _dt, 64, 64, ("rand", 0.6, 4, 31), 8, B=1, inplace=True))
    CASES_A.append(Case("ip64-%s-full" % _t(_dt), "wpt", _dt, 64, 64, 3, 8, B=1, inplace=True))
# ---- the LDS pyramid and the lane-local tail ------------------------------------------------------------------------------------
for _dt in (F64, F32):
    for _F in (2, 4, 6, 8, 10):
        CASES_A.append(Case("pyr-%s-F%d" % (_t(_dt), _F), "dwt", _dt, 16, 32, 4, _F, B=3))
    CASES_A.append(Case("pyr-%s-4x4" % _t(_dt), "dwt", _dt, 4, 4, 2, 4, B=3))
    for _F in (2, 4, 6, 8, 10, 12, 14, 16, 18, 20):
        CASES_A.append(Case("tail-%s-F%d" % (_t(_dt), _F), "dwt", _dt, 128, 128, 5 + (_F // 2) % 3, _F, B=2))
# ---- full trees: column pass + row pass -----------------------------------------------------------------------------------------
for _dt in (F64, F32):
    for _n in (8, 16, 32, 64, 128, 256, 512, 1024):       # every wx_rows_geometry outcome, 8 rows: the lattice rows decline
        CASES_A.append(Case("rows-%s-8x%d" % (_t(_dt), _n), "wpt", _dt, 8, _n, 3, 8, B=3, forced=_n in (8, 256, 1024)))
    for _F in (2, 4, 6, 8, 10, 12, 14, 16, 18, 20):
        CASES_A.append(Case("rows-%s-16x32-F%d" % (_t(_dt), _F), "wpt", _dt, 16, 32, 3, _F, B=3, off=_F in (4, 10)))
    for _F in (2, 4, 6):                                  # (8 taps: rows-*-8x256 / 8x1024 above)
        CASES_A.append(Case("rows-%s-8x256-F%d" % (_t(_dt), _F), "wpt", _dt, 8, 256, 2, _F, B=2, off=_F == 4))
        CASES_A.append(Case("rows-%s-8x1024-F%d" % (_t(_dt), _F), "wpt", _dt, 8, 1024, 2, _F, B=2))
    CASES_A.append(Case("rows-%s-iwpd-16x32" % _t(_dt), "wpd", _dt, 16, 32, 3, 8, B=3))    # the inverse reads slice L of the table
# lattice rows (Float64, 128 / 256 / 512 columns) at each SH, every stage count, and the depths at which they decline
for _F in (2, 4, 8, 12, 16, 20):
    CASES_A.append(Case("lrows-128-F%d" % _F, "wpt", F64, 32, 128, 3, _F, B=2, forced=_F == 8))
CASES_A += [
    Case("lrows-256-L2", "wpt", F64, 16, 256, 2, 8, B=3, forced=True),
    Case("lrows-256-L1", "wpt", F64, 16, 256, 1, 8, B=2),                      # L + SH < 6
    Case("lrows-256-odd", "wpt", F64, 32, 256, 1, 6, B=2),
    Case("lrows-512-L6", "wpt", F64, 64, 512, 6, 8, B=2, forced=True),
    Case("lrows-512-L5", "wpt", F64, 64, 512, 5, 8, B=2),                      # SH = 3 from 6 levels on
    Case("lrows-512-W", "wpt", F64, 64, 512, 6, 4, B=1),
    Case("lrows-256x256-L8", "wpt", F64, 256, 256, 8, 8, B=2),
]
for _F in (2, 4, 12, 16):
    CASES_A.append(Case("lrows-256-F%d" % _F, "wpt", F64, 16, 256, 2, _F, B=2))
for _F in (2, 12, 16):
    CASES_A.append(Case("lrows-512-F%d" % _F, "wpt", F64, 64, 512, 6, _F, B=1))
# ---- Float32 lattice: 256 x 256 (odd and even batches), 512 x 512, 1024 x 1024 ------------------------------------------------
CASES_A += [
    Case("l2d-256-B2", "wpt", F32, 256, 256, 5, 8, B=2, forced=True, tol=2e-6),
    Case("l2d-256-B3", "wpt", F32, 256, 256, 5, 8, B=3, tol=2e-6),
    Case("l2d-256-L8", "wpt", F32, 256, 256, 8, 8, B=2, forced=True, tol=3e-6),
    Case("l2d-256-F20", "wpt", F32, 256, 256, 5, 20, B=2, tol=2e-6),
    Case("l2d-256-L4", "wpt", F32, 256, 256, 4, 8, B=2),                       # below the lattice's depths: strips
    Case("l2d-512-L6", "wpt", F32, 512, 512, 6, 8, B=2, forced=True, tol=2e-6),
    Case("l2d-512-F4-L9", "wpt", F32, 512, 512, 9, 4, B=2, tol=3e-6),
    Case("l2d-1024-L7", "wpt", F32, 1024, 1024, 7, 8, B=2, forced=True, tol=3e-6),
    Case("l2d-1024-L3", "wpt", F32, 1024, 1024, 3, 8, B=2),
    Case("l2d-1024-F4-L8", "wpt", F32, 1024, 1024, 8, 4, B=2, tol=3e-6),
    Case("l2d-1024-F20", "wpt", F32, 1024, 1024, 7, 20, B=2, tol=3e-6),
]
for _F in (2, 4, 12, 16):                                 # every stage count of the fused launch (8 and 20 taps above)
    CASES_A.append(Case("l2d-256-F%d" % _F, "wpt", F32, 256, 256, 5, _F, B=2, tol=2e-6))
for _F in (2, 4, 12, 16, 20):
    CASES_A.append(Case("l2d-512-F%d" % _F, "wpt", F32, 512, 512, 6, _F, B=2, tol=2e-6))
for _F in (2, 4, 12, 16):                                 # (8 and 20 taps: l2d-1024-L7, l2d-1024-F20)
    CASES_A.append(Case("l2d-1024-F%d" % _F, "wpt", F32, 1024, 1024, 7, _F, B=2, tol=3e-6))
for _F in (2, 4, 8, 12, 16, 20):                          # one level past the lattice levels: the 8 x 8 node matrices (E = 1)
    CASES_A.append(Case("l2d-256-F%d-deep" % _F, "wpt", F32, 256, 256, 6, _F, B=2, tol=3e-6))
    CASES_A.append(Case("l2d-512-F%d-deep" % _F, "wpt", F32, 512, 512, 7, _F, B=2, tol=3e-6))
    CASES_A.append(Case("l2d-1024-F%d-deep" % _F, "wpt", F32, 1024, 1024, 8, _F, B=2, tol=3e-6))
CASES_A.append(Case("l2d-256-B1", "wpt", F32, 256, 256, 5, 8, B=1))                 # a pair of images per unit: one image takes the strips
# ---- tree-driven levels ------------------------------------------------------------------------------------------------------
_T2 = ("nodes", [1, 3])                                    # the root and its second child (the first would make it a pyramid)
_T3 = ("nodes", [1, 2, 3, 4, 5, 6, 7, 10, 11, 14, 15, 18, 19])     # depth 2: 8 of 16 nodes, half of the image
for _dt in (F64, F32):
    for _F in (2, 4, 6, 8, 10, 12, 14, 16, 18, 20):
        CASES_A.append(Case("tile-%s-F%d" % (_t(_dt), _F), "wpt", _dt, 128, 64 if _dt == F64 else 128, _T2, _F, B=2))   # depth 1: nodes of one tile
    for _F in (2, 4, 6, 8, 10, 12, 14, 16, 18, 20):      # depth 2: nodes smaller than a tile, the level walks the whole image
        CASES_A.append(Case("tile-%s-walk-F%d" % (_t(_dt), _F), "wpt", _dt, 128, 128, _T3, _F, B=2))
    CASES_A.append(Case("tile-%s-rand" % _t(_dt), "wpt", _dt, 256, 128, ("rand", 0.7, 5, 41), 8, B=2))
    CASES_A.append(Case("tile-%s-deep" % _t(_dt), "wpt", _dt, 128, 128, ("rand", 0.8, 7, 43), 4, B=2))   # below 8 x 8: two-pass levels
    CASES_A.append(Case("tile-%s-idwt128" % _t(_dt), "dwt", _dt, 128, 128, 7, 8, B=3))
    CASES_A.append(Case("tile-%s-long" % _t(_dt), "wpt", _dt, 64, 8192, 2, 8, B=1, forced=True))  # full tree, rows too long
    CASES_A.append(Case("two-%s-24x8" % _t(_dt), "wpt", _dt, 24, 8, 3, 8, B=3))                 # no dyadic side: two-pass by node list
    CASES_A.append(Case("two-%s-24x8-tree" % _t(_dt), "wpt", _dt, 24, 8, ("nodes", [1, 3]), 4, B=3))
    CASES_A.append(Case("two-%s-4x4" % _t(_dt), "wpt", _dt, 4, 4, 2, 4, B=3, forced=True))
    # wpd level by level: nodes larger than, equal to and smaller than a tile, then the two-pass levels
    CASES_A.append(Case("wpd-%s-128x64" % _t(_dt), "wpd", _dt, 128, 64, 5, 8, B=2))
    for _F in (2, 4, 6, 10, 12, 14, 16, 18, 20):
        CASES_A.append(Case("wpd-%s-128x64-F%d" % (_t(_dt), _F), "wpd", _dt, 128, 64, 2, _F, B=2))
    CASES_A.append(Case("wpd-%s-tile" % _t(_dt), "wpd", _dt, 64, 32 if _dt == F64 else 64, 2, 10, B=2))
    CASES_A.append(Case("wpd-%s-128-tree" % _t(_dt), "wpd", _dt, 128, 128, 3, 8, B=2, iarg=("rand", 0.6, 3, 47)))
    CASES_A.append(Case("wpd-%s-24x8" % _t(_dt), "wpd", _dt, 24, 8, 2, 4, B=2))
CASE_BY_ID = {c.id: c for c in CASES_A}
assert len(CASE_BY_ID) == len(CASES_A)

# (route, depth, K, e0 ...) of every launch (trailing zeros dropped; e0 ... as tabulated in csrc/wx_debug.h), as recorded on an
# MI355X (tools/dwt2d_pins.py writes this block): case id -> (forward, inverse)
# >>> PINS
PINS = {
    "q64-f64-F2": ([('Q64', 0, 3, 1)],
        [('Q64', 3, 3, 1)]),
    "q64-f64-F4": ([('Q64', 0, 3, 2)],
        [('Q64', 3, 3, 2)]),
    "q64-f64-F8": ([('Q64', 0, 3, 4)],
        [('Q64', 3, 3, 4)]),
    "q64-f64-F12": ([('Q64', 0, 3, 6)],
        [('Q64', 3, 3, 6)]),
    "q64-f64-F16": ([('Q64', 0, 3, 8)],
        [('Q64', 3, 3, 8)]),
    "q64-f64-F6-L6": ([('Q64', 0, 6, 4)],
        [('Q64', 6, 6, 4)]),
    "q64-f64-F20": ([('COL1D', 0, 2, 64, 64), ('ROWS', 0, 2, 20, 1, 0, 0, 32, 32)],
        [('ROWS', 2, 2, 20, 1, 0, 0, 32, 32), ('COL1D', 2, 2, 64, 64)]),
    "q64-f64-F18": ([('COL1D', 0, 2, 64, 64), ('ROWS', 0, 2, 18, 1, 0, 0, 32, 32)],
        [('ROWS', 2, 2, 18, 1, 0, 0, 32, 32), ('COL1D', 2, 2, 64, 64)]),
    "q64w-f64-F2": ([('Q64W', 0, 3, 1)],
        [('Q64', 3, 3, 1)]),
    "q64w-f64-F4": ([('Q64W', 0, 3, 2)],
        [('Q64', 3, 3, 2)]),
    "q64w-f64-F6": ([('Q64W', 0, 3, 4)],
        [('Q64', 3, 3, 4)]),
    "q64w-f64-F8": ([('Q64W', 0, 3, 4)],
        [('Q64', 3, 3, 4)]),
    "q64w-f64-F10": ([('TILEP', 0, 1, 10, 0, 0, 2), ('TILEP', 1, 1, 10, 0, 0, 2), ('TILEP', 2, 1, 10, 0, 0, 2)],
        [('Q64', 3, 3, 6)]),
    "q64w-f64-tree": ([('Q64W', 0, 3, 4)],
        [('GATHER', 0, 0, 8, 4), ('COPYB', 2, 0, 7), ('TWO', 3, 1, 1, 0, 1, 7), ('ITILE', 2, 1, 8, 0, 1, 2), ('ITILEP', 1, 1, 8, 1, 1, 2)]),
    "q64t-f64-F2": ([('Q64TPREP', 0, 4), ('Q64T', 0, 4, 1)],
        [('Q64TPREP', 4, 4), ('Q64T', 4, 4, 1)]),
    "q64t-f64-F4": ([('Q64TPREP', 0, 2), ('Q64T', 0, 2, 2)],
        [('Q64TPREP', 2, 2), ('Q64T', 2, 2, 2)]),
    "q64t-f64-F8": ([('Q64TPREP', 0, 4), ('Q64T', 0, 4, 4)],
        [('Q64TPREP', 4, 4), ('Q64T', 4, 4, 4)]),
    "q64t-f64-F12": ([('Q64TPREP', 0, 4), ('Q64T', 0, 4, 6)],
        [('Q64TPREP', 4, 4), ('Q64T', 4, 4, 6)]),
    "q64t-f64-F16": ([('Q64TPREP', 0, 4), ('Q64T', 0, 4, 8)],
        [('Q64TPREP', 4, 4), ('Q64T', 4, 4, 8)]),
    "q64t-f64-F18": ([('TILE', 0, 1, 18, 1, 1, 2), ('TILE', 1, 1, 18, 0, 1, 2), ('TWO', 2, 1, 1, 0, 1, 5)],
        [('COPYB', 2, 0, 5), ('TWO', 3, 1, 1, 0, 1, 5), ('ITILE', 2, 1, 18, 0, 1, 2), ('ITILE', 1, 1, 18, 1, 1, 2)]),
    "dwt64-f64-F8-L3": ([('Q64TPREP', 0, 3), ('Q64T', 0, 3, 4)],
        [('Q64TPREP', 3, 3), ('Q64T', 3, 3, 4)]),
    "dwt64-f64-F8-L4": ([('Q64TPREP', 0, 3), ('Q64T', 0, 3, 4), ('TAIL', 0, 1, 8, 64)],
        [('Q64TPREP', 4, 4), ('Q64T', 4, 4, 4)]),
    "dwt64-f64-F8-L5": ([('Q64TPREP', 0, 3), ('Q64T', 0, 3, 4), ('TAIL', 0, 2, 8, 64)],
        [('PYR', 5, 5, 8, 6, 6)]),
    "dwt64-f64-F8-L6": ([('Q64TPREP', 0, 3), ('Q64T', 0, 3, 4), ('TAIL', 0, 3, 8, 64)],
        [('PYR', 6, 6, 8, 6, 6)]),
    "dwt64-f64-F10-L6": ([('Q64TPREP', 0, 3), ('Q64T', 0, 3, 6), ('TAIL', 0, 3, 10, 64)],
        [('Q64TPREP', 6, 6), ('Q64T', 6, 6, 6)]),
    "dwt64-f64-F10-L4": ([('Q64TPREP', 0, 3), ('Q64T', 0, 3, 6), ('TAIL', 0, 1, 10, 64)],
        [('Q64TPREP', 4, 4), ('Q64T', 4, 4, 6)]),
    "dwt64-f64-F18-L6": ([('PYR', 0, 6, 0, 6, 6)],
        [('PYR', 6, 6, 0, 6, 6)]),
    "ip64-f64-dwt": ([('PYR', 0, 6, 8, 6, 6)],
        [('PYR', 6, 6, 8, 6, 6)]),
    "ip64-f64-tree": ([('TILEP', 0, 1, 8, 1, 1, 2), ('TILE', 1, 1, 8, 0, 1, 2), ('TWO', 2, 1, 1, 0, 1, 5), ('TWO', 3, 1, 1, 0, 1, 10)],
        [('COPYB', 2, 0, 5), ('TWO', 4, 1, 1, 0, 1, 10), ('TWO', 3, 1, 1, 0, 1, 5), ('ITILE', 2, 1, 8, 0, 1, 2), ('ITILEP', 1, 1, 8, 1, 1, 2)]),
    "ip64-f64-full": ([('Q64', 0, 3, 4)],
        [('Q64', 3, 3, 4)]),
    "q64-f32-F2": ([('Q64', 0, 3, 1)],
        [('Q64', 3, 3, 1)]),
    "q64-f32-F4": ([('Q64', 0, 3, 2)],
        [('Q64', 3, 3, 2)]),
    "q64-f32-F8": ([('Q64', 0, 3, 4)],
        [('Q64', 3, 3, 4)]),
    "q64-f32-F12": ([('Q64', 0, 3, 6)],
        [('Q64', 3, 3, 6)]),
    "q64-f32-F16": ([('Q64', 0, 3, 8)],
        [('Q64', 3, 3, 8)]),
    "q64-f32-F6-L6": ([('Q64', 0, 6, 4)],
        [('Q64', 6, 6, 4)]),
    "q64-f32-F20": ([('COL1D', 0, 2, 64, 64), ('ROWS', 0, 2, 20, 1, 0, 0, 64, 64)],
        [('ROWS', 2, 2, 20, 1, 0, 0, 64, 64), ('COL1D', 2, 2, 64, 64)]),
    "q64-f32-F18": ([('COL1D', 0, 2, 64, 64), ('ROWS', 0, 2, 18, 1, 0, 0, 64, 64)],
        [('ROWS', 2, 2, 18, 1, 0, 0, 64, 64), ('COL1D', 2, 2, 64, 64)]),
    "q64w-f32-F2": ([('Q64W', 0, 3, 1)],
        [('Q64', 3, 3, 1)]),
    "q64w-f32-F4": ([('Q64W', 0, 3, 2)],
        [('Q64', 3, 3, 2)]),
    "q64w-f32-F6": ([('Q64W', 0, 3, 4)],
        [('Q64', 3, 3, 4)]),
    "q64w-f32-F8": ([('Q64W', 0, 3, 4)],
        [('Q64', 3, 3, 4)]),
    "q64w-f32-F10": ([('TILE', 0, 1, 10, 0, 0, 1), ('TILE', 1, 1, 10, 0, 0, 1), ('TILE', 2, 1, 10, 0, 0, 1)],
        [('Q64', 3, 3, 6)]),
    "q64w-f32-tree": ([('Q64W', 0, 3, 4)],
        [('GATHER', 0, 0, 8, 4), ('COPYB', 2, 0, 7), ('TWO', 3, 1, 1, 0, 1, 7), ('ITILE', 2, 1, 8, 0, 1, 2), ('ITILE', 1, 1, 8, 1, 1, 2)]),
    "q64t-f32-F2": ([('Q64TPREP', 0, 4), ('Q64T', 0, 4, 1)],
        [('Q64TPREP', 4, 4), ('Q64T', 4, 4, 1)]),
    "q64t-f32-F4": ([('Q64TPREP', 0, 2), ('Q64T', 0, 2, 2)],
        [('Q64TPREP', 2, 2), ('Q64T', 2, 2, 2)]),
    "q64t-f32-F8": ([('Q64TPREP', 0, 4), ('Q64T', 0, 4, 4)],
        [('Q64TPREP', 4, 4), ('Q64T', 4, 4, 4)]),
    "q64t-f32-F12": ([('Q64TPREP', 0, 4), ('Q64T', 0, 4, 6)],
        [('Q64TPREP', 4, 4), ('Q64T', 4, 4, 6)]),
    "q64t-f32-F16": ([('Q64TPREP', 0, 4), ('Q64T', 0, 4, 8)],
        [('Q64TPREP', 4, 4), ('Q64T', 4, 4, 8)]),
    "q64t-f32-F18": ([('TILE', 0, 1, 18, 1, 1, 1), ('TILE', 1, 1, 18, 0, 1, 1), ('TWO', 2, 1, 1, 0, 1, 5)],
        [('COPYB', 2, 0, 5), ('TWO', 3, 1, 1, 0, 1, 5), ('ITILE', 2, 1, 18, 0, 1, 2), ('ITILE', 1, 1, 18, 1, 1, 2)]),
    "dwt64-f32-F8-L3": ([('Q64TPREP', 0, 3), ('Q64T', 0, 3, 4)],
        [('Q64TPREP', 3, 3), ('Q64T', 3, 3, 4)]),
    "dwt64-f32-F8-L4": ([('Q64TPREP', 0, 3), ('Q64T', 0, 3, 4), ('TAIL', 0, 1, 8, 64)],
        [('Q64TPREP', 4, 4), ('Q64T', 4, 4, 4)]),
    "dwt64-f32-F8-L5": ([('Q64TPREP', 0, 3), ('Q64T', 0, 3, 4), ('TAIL', 0, 2, 8, 64)],
        [('PYR', 5, 5, 8, 6, 6)]),
    "dwt64-f32-F8-L6": ([('Q64TPREP', 0, 3), ('Q64T', 0, 3, 4), ('TAIL', 0, 3, 8, 64)],
        [('PYR', 6, 6, 8, 6, 6)]),
    "dwt64-f32-F10-L6": ([('Q64TPREP', 0, 3), ('Q64T', 0, 3, 6), ('TAIL', 0, 3, 10, 64)],
        [('Q64TPREP', 6, 6), ('Q64T', 6, 6, 6)]),
    "dwt64-f32-F10-L4": ([('Q64TPREP', 0, 3), ('Q64T', 0, 3, 6), ('TAIL', 0, 1, 10, 64)],
        [('Q64TPREP', 4, 4), ('Q64T', 4, 4, 6)]),
    "dwt64-f32-F18-L6": ([('PYR', 0, 6, 0, 6, 6)],
        [('PYR', 6, 6, 0, 6, 6)]),
    "ip64-f32-dwt": ([('PYR', 0, 6, 8, 6, 6)],
        [('PYR', 6, 6, 8, 6, 6)]),
    "ip64-f32-tree": ([('TILEP', 0, 1, 8, 1, 1, 1), ('TILE', 1, 1, 8, 0, 1, 1), ('TWO', 2, 1, 1, 0, 1, 5), ('TWO', 3, 1, 1, 0, 1, 10)],
        [('COPYB', 2, 0, 5), ('TWO', 4, 1, 1, 0, 1, 10), ('TWO', 3, 1, 1, 0, 1, 5), ('ITILE', 2, 1, 8, 0, 1, 2), ('ITILE', 1, 1, 8, 1, 1, 2)]),
    "ip64-f32-full": ([('Q64', 0, 3, 4)],
        [('Q64', 3, 3, 4)]),
    "pyr-f64-F2": ([('PYR', 0, 4, 2, 4, 5)],
        [('PYR', 4, 4, 2, 4, 5)]),
    "pyr-f64-F4": ([('PYR', 0, 4, 4, 4, 5)],
        [('PYR', 4, 4, 4, 4, 5)]),
    "pyr-f64-F6": ([('PYR', 0, 4, 6, 4, 5)],
        [('PYR', 4, 4, 6, 4, 5)]),
    "pyr-f64-F8": ([('PYR', 0, 4, 8, 4, 5)],
        [('PYR', 4, 4, 8, 4, 5)]),
    "pyr-f64-F10": ([('PYR', 0, 4, 0, 4, 5)],
        [('PYR', 4, 4, 0, 4, 5)]),
    "pyr-f64-4x4": ([('PYR', 0, 2, 4, 2, 2)],
        [('PYR', 2, 2, 4, 2, 2)]),
    "tail-f64-F2": ([('TILEP', 0, 1, 2, 1, 1, 8), ('TILEP', 1, 1, 2, 1, 1, 2), ('TWO', 2, 1, 1, 0, 1, 1), ('TWO', 3, 1, 1, 0, 1, 1), ('TAIL', 0, 2, 2, 128)],
        [('COPYB', 2, 0, 1), ('TWO', 6, 1, 1, 0, 1, 1), ('TWO', 5, 1, 1, 0, 1, 1), ('TWO', 4, 1, 1, 0, 1, 1), ('TWO', 3, 1, 1, 0, 1, 1), ('ITILEP', 2, 1, 2, 1, 1, 2), ('ITILEP', 1, 1, 2, 1, 1, 8)]),
    "tail-f64-F4": ([('TILEP', 0, 1, 4, 1, 1, 8), ('TILEP', 1, 1, 4, 1, 1, 2), ('TWO', 2, 1, 1, 0, 1, 1), ('TWO', 3, 1, 1, 0, 1, 1), ('TAIL', 0, 3, 4, 128)],
        [('COPYB', 2, 0, 1), ('TWO', 7, 1, 1, 0, 1, 1), ('TWO', 6, 1, 1, 0, 1, 1), ('TWO', 5, 1, 1, 0, 1, 1), ('TWO', 4, 1, 1, 0, 1, 1), ('TWO', 3, 1, 1, 0, 1, 1), ('ITILEP', 2, 1, 4, 1, 1, 2), ('ITILEP', 1, 1, 4, 1, 1, 8)]),
    "tail-f64-F6": ([('TILEP', 0, 1, 6, 1, 1, 8), ('TILEP', 1, 1, 6, 1, 1, 2), ('TWO', 2, 1, 1, 0, 1, 1), ('TWO', 3, 1, 1, 0, 1, 1), ('TAIL', 0, 1, 6, 128)],
        [('COPYB', 2, 0, 1), ('TWO', 5, 1, 1, 0, 1, 1), ('TWO', 4, 1, 1, 0, 1, 1), ('TWO', 3, 1, 1, 0, 1, 1), ('ITILEP', 2, 1, 6, 1, 1, 2), ('ITILEP', 1, 1, 6, 1, 1, 8)]),
    "tail-f64-F8": ([('TILEP', 0, 1, 8, 1, 1, 8), ('TILEP', 1, 1, 8, 1, 1, 2), ('TWO', 2, 1, 1, 0, 1, 1), ('TWO', 3, 1, 1, 0, 1, 1), ('TAIL', 0, 2, 8, 128)],
        [('COPYB', 2, 0, 1), ('TWO', 6, 1, 1, 0, 1, 1), ('TWO', 5, 1, 1, 0, 1, 1), ('TWO', 4, 1, 1, 0, 1, 1), ('TWO', 3, 1, 1, 0, 1, 1), ('ITILEP', 2, 1, 8, 1, 1, 2), ('ITILEP', 1, 1, 8, 1, 1, 8)]),
    "tail-f64-F10": ([('TILEP', 0, 1, 10, 1, 1, 8), ('TILEP', 1, 1, 10, 1, 1, 2), ('TWO', 2, 1, 1, 0, 1, 1), ('TWO', 3, 1, 1, 0, 1, 1), ('TAIL', 0, 3, 10, 128)],
        [('COPYB', 2, 0, 1), ('TWO', 7, 1, 1, 0, 1, 1), ('TWO', 6, 1, 1, 0, 1, 1), ('TWO', 5, 1, 1, 0, 1, 1), ('TWO', 4, 1, 1, 0, 1, 1), ('TWO', 3, 1, 1, 0, 1, 1), ('ITILE', 2, 1, 10, 1, 1, 2), ('ITILE', 1, 1, 10, 1, 1, 8)]),
    "tail-f64-F12": ([('TILE', 0, 1, 12, 1, 1, 8), ('TILE', 1, 1, 12, 1, 1, 2), ('TWO', 2, 1, 1, 0, 1, 1), ('TWO', 3, 1, 1, 0, 1, 1), ('TAIL', 0, 1, 12, 128)],
        [('COPYB', 2, 0, 1), ('TWO', 5, 1, 1, 0, 1, 1), ('TWO', 4, 1, 1, 0, 1, 1), ('TWO', 3, 1, 1, 0, 1, 1), ('ITILE', 2, 1, 12, 1, 1, 2), ('ITILE', 1, 1, 12, 1, 1, 8)]),
    "tail-f64-F14": ([('TILE', 0, 1, 14, 1, 1, 8), ('TILE', 1, 1, 14, 1, 1, 2), ('TWO', 2, 1, 1, 0, 1, 1), ('TWO', 3, 1, 1, 0, 1, 1), ('TAIL', 0, 2, 14, 128)],
        [('COPYB', 2, 0, 1), ('TWO', 6, 1, 1, 0, 1, 1), ('TWO', 5, 1, 1, 0, 1, 1), ('TWO', 4, 1, 1, 0, 1, 1), ('TWO', 3, 1, 1, 0, 1, 1), ('ITILE', 2, 1, 14, 1, 1, 2), ('ITILE', 1, 1, 14, 1, 1, 8)]),
    "tail-f64-F16": ([('TILE', 0, 1, 16, 1, 1, 8), ('TILE', 1, 1, 16, 1, 1, 2), ('TWO', 2, 1, 1, 0, 1, 1), ('TWO', 3, 1, 1, 0, 1, 1), ('TAIL', 0, 3, 16, 128)],
        [('COPYB', 2, 0, 1), ('TWO', 7, 1, 1, 0, 1, 1), ('TWO', 6, 1, 1, 0, 1, 1), ('TWO', 5, 1, 1, 0, 1, 1), ('TWO', 4, 1, 1, 0, 1, 1), ('TWO', 3, 1, 1, 0, 1, 1), ('ITILE', 2, 1, 16, 1, 1, 2), ('ITILE', 1, 1, 16, 1, 1, 8)]),
    "tail-f64-F18": ([('TILE', 0, 1, 18, 1, 1, 8), ('TILE', 1, 1, 18, 1, 1, 2), ('TWO', 2, 1, 1, 0, 1, 1), ('TWO', 3, 1, 1, 0, 1, 1), ('TAIL', 0, 1, 18, 128)],
        [('COPYB', 2, 0, 1), ('TWO', 5, 1, 1, 0, 1, 1), ('TWO', 4, 1, 1, 0, 1, 1), ('TWO', 3, 1, 1, 0, 1, 1), ('ITILE', 2, 1, 18, 1, 1, 2), ('ITILE', 1, 1, 18, 1, 1, 8)]),
    "tail-f64-F20": ([('TILE', 0, 1, 20, 1, 1, 8), ('TILE', 1, 1, 20, 1, 1, 2), ('TWO', 2, 1, 1, 0, 1, 1), ('TWO', 3, 1, 1, 0, 1, 1), ('TAIL', 0, 2, 20, 128)],
        [('COPYB', 2, 0, 1), ('TWO', 6, 1, 1, 0, 1, 1), ('TWO', 5, 1, 1, 0, 1, 1), ('TWO', 4, 1, 1, 0, 1, 1), ('TWO', 3, 1, 1, 0, 1, 1), ('ITILE', 2, 1, 20, 1, 1, 2), ('ITILE', 1, 1, 20, 1, 1, 8)]),
    "pyr-f32-F2": ([('PYR', 0, 4, 2, 4, 5)],
        [('PYR', 4, 4, 2, 4, 5)]),
    "pyr-f32-F4": ([('PYR', 0, 4, 4, 4, 5)],
        [('PYR', 4, 4, 4, 4, 5)]),
    "pyr-f32-F6": ([('PYR', 0, 4, 6, 4, 5)],
        [('PYR', 4, 4, 6, 4, 5)]),
    "pyr-f32-F8": ([('PYR', 0, 4, 8, 4, 5)],
        [('PYR', 4, 4, 8, 4, 5)]),
    "pyr-f32-F10": ([('PYR', 0, 4, 0, 4, 5)],
        [('PYR', 4, 4, 0, 4, 5)]),
    "pyr-f32-4x4": ([('PYR', 0, 2, 4, 2, 2)],
        [('PYR', 2, 2, 4, 2, 2)]),
    "tail-f32-F2": ([('TILEP', 0, 1, 2, 1, 1, 4), ('TILEP', 1, 1, 2, 1, 1, 1), ('TWO', 2, 1, 1, 0, 1, 1), ('TWO', 3, 1, 1, 0, 1, 1), ('TAIL', 0, 2, 2, 128)],
        [('COPYB', 2, 0, 1), ('TWO', 6, 1, 1, 0, 1, 1), ('TWO', 5, 1, 1, 0, 1, 1), ('TWO', 4, 1, 1, 0, 1, 1), ('TWO', 3, 1, 1, 0, 1, 1), ('ITILE', 2, 1, 2, 1, 1, 2), ('ITILE', 1, 1, 2, 1, 1, 8)]),
    "tail-f32-F4": ([('TILEP', 0, 1, 4, 1, 1, 4), ('TILEP', 1, 1, 4, 1, 1, 1), ('TWO', 2, 1, 1, 0, 1, 1), ('TWO', 3, 1, 1, 0, 1, 1), ('TAIL', 0, 3, 4, 128)],
        [('COPYB', 2, 0, 1), ('TWO', 7, 1, 1, 0, 1, 1), ('TWO', 6, 1, 1, 0, 1, 1), ('TWO', 5, 1, 1, 0, 1, 1), ('TWO', 4, 1, 1, 0, 1, 1), ('TWO', 3, 1, 1, 0, 1, 1), ('ITILE', 2, 1, 4, 1, 1, 2), ('ITILE', 1, 1, 4, 1, 1, 8)]),
    "tail-f32-F6": ([('TILEP', 0, 1, 6, 1, 1, 4), ('TILEP', 1, 1, 6, 1, 1, 1), ('TWO', 2, 1, 1, 0, 1, 1), ('TWO', 3, 1, 1, 0, 1, 1), ('TAIL', 0, 1, 6, 128)],
        [('COPYB', 2, 0, 1), ('TWO', 5, 1, 1, 0, 1, 1), ('TWO', 4, 1, 1, 0, 1, 1), ('TWO', 3, 1, 1, 0, 1, 1), ('ITILE', 2, 1, 6, 1, 1, 2), ('ITILE', 1, 1, 6, 1, 1, 8)]),
    "tail-f32-F8": ([('TILEP', 0, 1, 8, 1, 1, 4), ('TILEP', 1, 1, 8, 1, 1, 1), ('TWO', 2, 1, 1, 0, 1, 1), ('TWO', 3, 1, 1, 0, 1, 1), ('TAIL', 0, 2, 8, 128)],
        [('COPYB', 2, 0, 1), ('TWO', 6, 1, 1, 0, 1, 1), ('TWO', 5, 1, 1, 0, 1, 1), ('TWO', 4, 1, 1, 0, 1, 1), ('TWO', 3, 1, 1, 0, 1, 1), ('ITILE', 2, 1, 8, 1, 1, 2), ('ITILE', 1, 1, 8, 1, 1, 8)]),
    "tail-f32-F10": ([('TILE', 0, 1, 10, 1, 1, 4), ('TILE', 1, 1, 10, 1, 1, 1), ('TWO', 2, 1, 1, 0, 1, 1), ('TWO', 3, 1, 1, 0, 1, 1), ('TAIL', 0, 3, 10, 128)],
        [('COPYB', 2, 0, 1), ('TWO', 7, 1, 1, 0, 1, 1), ('TWO', 6, 1, 1, 0, 1, 1), ('TWO', 5, 1, 1, 0, 1, 1), ('TWO', 4, 1, 1, 0, 1, 1), ('TWO', 3, 1, 1, 0, 1, 1), ('ITILE', 2, 1, 10, 1, 1, 2), ('ITILE', 1, 1, 10, 1, 1, 8)]),
    "tail-f32-F12": ([('TILE', 0, 1, 12, 1, 1, 4), ('TILE', 1, 1, 12, 1, 1, 1), ('TWO', 2, 1, 1, 0, 1, 1), ('TWO', 3, 1, 1, 0, 1, 1), ('TAIL', 0, 1, 12, 128)],
        [('COPYB', 2, 0, 1), ('TWO', 5, 1, 1, 0, 1, 1), ('TWO', 4, 1, 1, 0, 1, 1), ('TWO', 3, 1, 1, 0, 1, 1), ('ITILE', 2, 1, 12, 1, 1, 2), ('ITILE', 1, 1, 12, 1, 1, 8)]),
    "tail-f32-F14": ([('TILE', 0, 1, 14, 1, 1, 4), ('TILE', 1, 1, 14, 1, 1, 1), ('TWO', 2, 1, 1, 0, 1, 1), ('TWO', 3, 1, 1, 0, 1, 1), ('TAIL', 0, 2, 14, 128)],
        [('COPYB', 2, 0, 1), ('TWO', 6, 1, 1, 0, 1, 1), ('TWO', 5, 1, 1, 0, 1, 1), ('TWO', 4, 1, 1, 0, 1, 1), ('TWO', 3, 1, 1, 0, 1, 1), ('ITILE', 2, 1, 14, 1, 1, 2), ('ITILE', 1, 1, 14, 1, 1, 8)]),
    "tail-f32-F16": ([('TILE', 0, 1, 16, 1, 1, 4), ('TILE', 1, 1, 16, 1, 1, 1), ('TWO', 2, 1, 1, 0, 1, 1), ('TWO', 3, 1, 1, 0, 1, 1), ('TAIL', 0, 3, 16, 128)],
        [('COPYB', 2, 0, 1), ('TWO', 7, 1, 1, 0, 1, 1), ('TWO', 6, 1, 1, 0, 1, 1), ('TWO', 5, 1, 1, 0, 1, 1), ('TWO', 4, 1, 1, 0, 1, 1), ('TWO', 3, 1, 1, 0, 1, 1), ('ITILE', 2, 1, 16, 1, 1, 2), ('ITILE', 1, 1, 16, 1, 1, 8)]),
    "tail-f32-F18": ([('TILE', 0, 1, 18, 1, 1, 4), ('TILE', 1, 1, 18, 1, 1, 1), ('TWO', 2, 1, 1, 0, 1, 1), ('TWO', 3, 1, 1, 0, 1, 1), ('TAIL', 0, 1, 18, 128)],
        [('COPYB', 2, 0, 1), ('TWO', 5, 1, 1, 0, 1, 1), ('TWO', 4, 1, 1, 0, 1, 1), ('TWO', 3, 1, 1, 0, 1, 1), ('ITILE', 2, 1, 18, 1, 1, 2), ('ITILE', 1, 1, 18, 1, 1, 8)]),
    "tail-f32-F20": ([('TILE', 0, 1, 20, 1, 1, 4), ('TILE', 1, 1, 20, 1, 1, 1), ('TWO', 2, 1, 1, 0, 1, 1), ('TWO', 3, 1, 1, 0, 1, 1), ('TAIL', 0, 2, 20, 128)],
        [('COPYB', 2, 0, 1), ('TWO', 6, 1, 1, 0, 1, 1), ('TWO', 5, 1, 1, 0, 1, 1), ('TWO', 4, 1, 1, 0, 1, 1), ('TWO', 3, 1, 1, 0, 1, 1), ('ITILE', 2, 1, 20, 1, 1, 2), ('ITILE', 1, 1, 20, 1, 1, 8)]),
    "rows-f64-8x8": ([('COL1D', 0, 3, 8, 8), ('ROWS', 0, 3, 8, 2, 0, 0, 32, 32)],
        [('ROWS', 3, 3, 8, 2, 0, 0, 32, 32), ('COL1D', 3, 3, 8, 8)]),
    "rows-f64-8x16": ([('COL1D', 0, 3, 8, 16), ('ROWS', 0, 3, 8, 2, 0, 0, 32, 32)],
        [('ROWS', 3, 3, 8, 2, 0, 0, 32, 32), ('COL1D', 3, 3, 8, 16)]),
    "rows-f64-8x32": ([('COL1D', 0, 3, 8, 32), ('ROWS', 0, 3, 8, 2, 0, 0, 32, 32)],
        [('ROWS', 3, 3, 8, 2, 0, 0, 32, 32), ('COL1D', 3, 3, 8, 32)]),
    "rows-f64-8x64": ([('COL1D', 0, 3, 8, 64), ('ROWS', 0, 3, 8, 2, 0, 0, 32, 32)],
        [('ROWS', 3, 3, 8, 2, 0, 0, 32, 32), ('COL1D', 3, 3, 8, 64)]),
    "rows-f64-8x128": ([('COL1D', 0, 3, 8, 128), ('ROWS', 0, 3, 8, 2, 0, 0, 32, 32)],
        [('ROWS', 3, 3, 8, 2, 0, 0, 32, 32), ('COL1D', 3, 3, 8, 128)]),
    "rows-f64-8x256": ([('COL1D', 0, 3, 8, 256), ('ROWS', 0, 3, 8, 2, 2, 1, 32, 32)],
        [('ROWS', 3, 3, 8, 2, 2, 1, 32, 32), ('COL1D', 3, 3, 8, 256)]),
    "rows-f64-8x512": ([('COL1D', 0, 3, 8, 512), ('ROWS', 0, 3, 8, 2, 2, 1, 16, 20)],
        [('ROWS', 3, 3, 8, 2, 2, 1, 16, 20), ('COL1D', 3, 3, 8, 512)]),
    "rows-f64-8x1024": ([('COL1D', 0, 3, 8, 1024), ('ROWS', 0, 3, 8, 2, 2, 1, 8, 10)],
        [('ROWS', 3, 3, 8, 2, 2, 1, 8, 10), ('COL1D', 3, 3, 8, 1024)]),
    "rows-f64-16x32-F2": ([('COL1D', 0, 3, 16, 32), ('ROWS', 0, 3, 2, 2, 0, 0, 32, 32)],
        [('ROWS', 3, 3, 2, 2, 0, 0, 32, 32), ('COL1D', 3, 3, 16, 32)]),
    "rows-f64-16x32-F4": ([('COL1D', 0, 3, 16, 32), ('ROWS', 0, 3, 4, 2, 0, 0, 32, 32)],
        [('ROWS', 3, 3, 4, 2, 0, 0, 32, 32), ('COL1D', 3, 3, 16, 32)]),
    "rows-f64-16x32-F6": ([('COL1D', 0, 3, 16, 32), ('ROWS', 0, 3, 6, 2, 0, 0, 32, 32)],
        [('ROWS', 3, 3, 6, 2, 0, 0, 32, 32), ('COL1D', 3, 3, 16, 32)]),
    "rows-f64-16x32-F8": ([('COL1D', 0, 3, 16, 32), ('ROWS', 0, 3, 8, 2, 0, 0, 32, 32)],
        [('ROWS', 3, 3, 8, 2, 0, 0, 32, 32), ('COL1D', 3, 3, 16, 32)]),
    "rows-f64-16x32-F10": ([('COL1D', 0, 3, 16, 32), ('ROWS', 0, 3, 10, 2, 0, 0, 32, 32)],
        [('ROWS', 3, 3, 10, 2, 0, 0, 32, 32), ('COL1D', 3, 3, 16, 32)]),
    "rows-f64-16x32-F12": ([('COL1D', 0, 3, 16, 32), ('ROWS', 0, 3, 12, 2, 0, 0, 32, 32)],
        [('ROWS', 3, 3, 12, 2, 0, 0, 32, 32), ('COL1D', 3, 3, 16, 32)]),
    "rows-f64-16x32-F14": ([('COL1D', 0, 3, 16, 32), ('ROWS', 0, 3, 14, 1, 0, 0, 32, 32)],
        [('ROWS', 3, 3, 14, 1, 0, 0, 32, 32), ('COL1D', 3, 3, 16, 32)]),
    "rows-f64-16x32-F16": ([('COL1D', 0, 3, 16, 32), ('ROWS', 0, 3, 16, 1, 0, 0, 32, 32)],
        [('ROWS', 3, 3, 16, 1, 0, 0, 32, 32), ('COL1D', 3, 3, 16, 32)]),
    "rows-f64-16x32-F18": ([('COL1D', 0, 3, 16, 32), ('ROWS', 0, 3, 18, 1, 0, 0, 32, 32)],
        [('ROWS', 3, 3, 18, 1, 0, 0, 32, 32), ('COL1D', 3, 3, 16, 32)]),
    "rows-f64-16x32-F20": ([('COL1D', 0, 3, 16, 32), ('ROWS', 0, 3, 20, 1, 0, 0, 32, 32)],
        [('ROWS', 3, 3, 20, 1, 0, 0, 32, 32), ('COL1D', 3, 3, 16, 32)]),
    "rows-f64-8x256-F2": ([('COL1D', 0, 2, 8, 256), ('ROWS', 0, 2, 2, 2, 2, 1, 32, 32)],
        [('ROWS', 2, 2, 2, 2, 2, 1, 32, 32), ('COL1D', 2, 2, 8, 256)]),
    "rows-f64-8x1024-F2": ([('COL1D', 0, 2, 8, 1024), ('ROWS', 0, 2, 2, 2, 2, 1, 8, 10)],
        [('ROWS', 2, 2, 2, 2, 2, 1, 8, 10), ('COL1D', 2, 2, 8, 1024)]),
    "rows-f64-8x256-F4": ([('COL1D', 0, 2, 8, 256), ('ROWS', 0, 2, 4, 2, 2, 1, 32, 32)],
        [('ROWS', 2, 2, 4, 2, 2, 1, 32, 32), ('COL1D', 2, 2, 8, 256)]),
    "rows-f64-8x1024-F4": ([('COL1D', 0, 2, 8, 1024), ('ROWS', 0, 2, 4, 2, 2, 1, 8, 10)],
        [('ROWS', 2, 2, 4, 2, 2, 1, 8, 10), ('COL1D', 2, 2, 8, 1024)]),
    "rows-f64-8x256-F6": ([('COL1D', 0, 2, 8, 256), ('ROWS', 0, 2, 6, 2, 2, 1, 32, 32)],
        [('ROWS', 2, 2, 6, 2, 2, 1, 32, 32), ('COL1D', 2, 2, 8, 256)]),
    "rows-f64-8x1024-F6": ([('COL1D', 0, 2, 8, 1024), ('ROWS', 0, 2, 6, 2, 2, 1, 8, 10)],
        [('ROWS', 2, 2, 6, 2, 2, 1, 8, 10), ('COL1D', 2, 2, 8, 1024)]),
    "rows-f64-iwpd-16x32": ([('TWO', 0, 1, 0, 1), ('TWO', 1, 1, 0, 1), ('TWO', 2, 1, 0, 1)],
        [('ROWS', 3, 3, 8, 2, 0, 0, 32, 32), ('COL1D', 3, 3, 16, 32)]),
    "rows-f32-8x8": ([('COL1D', 0, 3, 8, 8), ('ROWS', 0, 3, 8, 4, 0, 0, 64, 64)],
        [('ROWS', 3, 3, 8, 4, 0, 0, 64, 64), ('COL1D', 3, 3, 8, 8)]),
    "rows-f32-8x16": ([('COL1D', 0, 3, 8, 16), ('ROWS', 0, 3, 8, 4, 0, 0, 64, 64)],
        [('ROWS', 3, 3, 8, 4, 0, 0, 64, 64), ('COL1D', 3, 3, 8, 16)]),
    "rows-f32-8x32": ([('COL1D', 0, 3, 8, 32), ('ROWS', 0, 3, 8, 4, 0, 0, 64, 64)],
        [('ROWS', 3, 3, 8, 4, 0, 0, 64, 64), ('COL1D', 3, 3, 8, 32)]),
    "rows-f32-8x64": ([('COL1D', 0, 3, 8, 64), ('ROWS', 0, 3, 8, 4, 0, 0, 64, 64)],
        [('ROWS', 3, 3, 8, 4, 0, 0, 64, 64), ('COL1D', 3, 3, 8, 64)]),
    "rows-f32-8x128": ([('COL1D', 0, 3, 8, 128), ('ROWS', 0, 3, 8, 4, 0, 0, 64, 64)],
        [('ROWS', 3, 3, 8, 4, 0, 0, 64, 64), ('COL1D', 3, 3, 8, 128)]),
    "rows-f32-8x256": ([('COL1D', 0, 3, 8, 256), ('ROWS', 0, 3, 8, 4, 2, 0, 64, 64)],
        [('ROWS', 3, 3, 8, 4, 2, 0, 64, 64), ('COL1D', 3, 3, 8, 256)]),
    "rows-f32-8x512": ([('COL1D', 0, 3, 8, 512), ('ROWS', 0, 3, 8, 4, 2, 0, 32, 32)],
        [('ROWS', 3, 3, 8, 4, 2, 0, 32, 32), ('COL1D', 3, 3, 8, 512)]),
    "rows-f32-8x1024": ([('COL1D', 0, 3, 8, 1024), ('ROWS', 0, 3, 8, 4, 2, 1, 16, 20)],
        [('ROWS', 3, 3, 8, 4, 2, 1, 16, 20), ('COL1D', 3, 3, 8, 1024)]),
    "rows-f32-16x32-F2": ([('COL1D', 0, 3, 16, 32), ('ROWS', 0, 3, 2, 4, 0, 0, 64, 64)],
        [('ROWS', 3, 3, 2, 4, 0, 0, 64, 64), ('COL1D', 3, 3, 16, 32)]),
    "rows-f32-16x32-F4": ([('COL1D', 0, 3, 16, 32), ('ROWS', 0, 3, 4, 4, 0, 0, 64, 64)],
        [('ROWS', 3, 3, 4, 4, 0, 0, 64, 64), ('COL1D', 3, 3, 16, 32)]),
    "rows-f32-16x32-F6": ([('COL1D', 0, 3, 16, 32), ('ROWS', 0, 3, 6, 4, 0, 0, 64, 64)],
        [('ROWS', 3, 3, 6, 4, 0, 0, 64, 64), ('COL1D', 3, 3, 16, 32)]),
    "rows-f32-16x32-F8": ([('COL1D', 0, 3, 16, 32), ('ROWS', 0, 3, 8, 4, 0, 0, 64, 64)],
        [('ROWS', 3, 3, 8, 4, 0, 0, 64, 64), ('COL1D', 3, 3, 16, 32)]),
    "rows-f32-16x32-F10": ([('COL1D', 0, 3, 16, 32), ('ROWS', 0, 3, 10, 4, 0, 0, 64, 64)],
        [('ROWS', 3, 3, 10, 4, 0, 0, 64, 64), ('COL1D', 3, 3, 16, 32)]),
    "rows-f32-16x32-F12": ([('COL1D', 0, 3, 16, 32), ('ROWS', 0, 3, 12, 4, 0, 0, 64, 64)],
        [('ROWS', 3, 3, 12, 4, 0, 0, 64, 64), ('COL1D', 3, 3, 16, 32)]),
    "rows-f32-16x32-F14": ([('COL1D', 0, 3, 16, 32), ('ROWS', 0, 3, 14, 1, 0, 0, 64, 64)],
        [('ROWS', 3, 3, 14, 1, 0, 0, 64, 64), ('COL1D', 3, 3, 16, 32)]),
    "rows-f32-16x32-F16": ([('COL1D', 0, 3, 16, 32), ('ROWS', 0, 3, 16, 1, 0, 0, 64, 64)],
        [('ROWS', 3, 3, 16, 1, 0, 0, 64, 64), ('COL1D', 3, 3, 16, 32)]),
    "rows-f32-16x32-F18": ([('COL1D', 0, 3, 16, 32), ('ROWS', 0, 3, 18, 1, 0, 0, 64, 64)],
        [('ROWS', 3, 3, 18, 1, 0, 0, 64, 64), ('COL1D', 3, 3, 16, 32)]),
    "rows-f32-16x32-F20": ([('COL1D', 0, 3, 16, 32), ('ROWS', 0, 3, 20, 1, 0, 0, 64, 64)],
        [('ROWS', 3, 3, 20, 1, 0, 0, 64, 64), ('COL1D', 3, 3, 16, 32)]),
    "rows-f32-8x256-F2": ([('COL1D', 0, 2, 8, 256), ('ROWS', 0, 2, 2, 4, 2, 0, 64, 64)],
        [('ROWS', 2, 2, 2, 4, 2, 0, 64, 64), ('COL1D', 2, 2, 8, 256)]),
    "rows-f32-8x1024-F2": ([('COL1D', 0, 2, 8, 1024), ('ROWS', 0, 2, 2, 4, 2, 1, 16, 20)],
        [('ROWS', 2, 2, 2, 4, 2, 1, 16, 20), ('COL1D', 2, 2, 8, 1024)]),
    "rows-f32-8x256-F4": ([('COL1D', 0, 2, 8, 256), ('ROWS', 0, 2, 4, 4, 2, 0, 64, 64)],
        [('ROWS', 2, 2, 4, 4, 2, 0, 64, 64), ('COL1D', 2, 2, 8, 256)]),
    "rows-f32-8x1024-F4": ([('COL1D', 0, 2, 8, 1024), ('ROWS', 0, 2, 4, 4, 2, 1, 16, 20)],
        [('ROWS', 2, 2, 4, 4, 2, 1, 16, 20), ('COL1D', 2, 2, 8, 1024)]),
    "rows-f32-8x256-F6": ([('COL1D', 0, 2, 8, 256), ('ROWS', 0, 2, 6, 4, 2, 0, 64, 64)],
        [('ROWS', 2, 2, 6, 4, 2, 0, 64, 64), ('COL1D', 2, 2, 8, 256)]),
    "rows-f32-8x1024-F6": ([('COL1D', 0, 2, 8, 1024), ('ROWS', 0, 2, 6, 4, 2, 1, 16, 20)],
        [('ROWS', 2, 2, 6, 4, 2, 1, 16, 20), ('COL1D', 2, 2, 8, 1024)]),
    "rows-f32-iwpd-16x32": ([('TWO', 0, 1, 0, 1), ('TWO', 1, 1, 0, 1), ('TWO', 2, 1, 0, 1)],
        [('ROWS', 3, 3, 8, 4, 0, 0, 64, 64), ('COL1D', 3, 3, 16, 32)]),
    "lrows-128-F2": ([('COL1D', 0, 3, 32, 128), ('LROWS', 0, 3, 1, 5, 1)],
        [('LROWS', 3, 3, 1, 5, 1), ('COL1D', 3, 3, 32, 128)]),
    "lrows-128-F4": ([('COL1D', 0, 3, 32, 128), ('LROWS', 0, 3, 2, 5, 1)],
        [('LROWS', 3, 3, 2, 5, 1), ('COL1D', 3, 3, 32, 128)]),
    "lrows-128-F8": ([('COL1D', 0, 3, 32, 128), ('LROWS', 0, 3, 4, 5, 1)],
        [('LROWS', 3, 3, 4, 5, 1), ('COL1D', 3, 3, 32, 128)]),
    "lrows-128-F12": ([('COL1D', 0, 3, 32, 128), ('LROWS', 0, 3, 6, 5, 1)],
        [('LROWS', 3, 3, 6, 5, 1), ('COL1D', 3, 3, 32, 128)]),
    "lrows-128-F16": ([('COL1D', 0, 3, 32, 128), ('LROWS', 0, 3, 8, 5, 1)],
        [('LROWS', 3, 3, 8, 5, 1), ('COL1D', 3, 3, 32, 128)]),
    "lrows-128-F20": ([('COL1D', 0, 3, 32, 128), ('ROWS', 0, 3, 20, 1, 0, 0, 32, 32)],
        [('ROWS', 3, 3, 20, 1, 0, 0, 32, 32), ('COL1D', 3, 3, 32, 128)]),
    "lrows-256-L2": ([('COL1D', 0, 2, 16, 256), ('LROWS', 0, 2, 4, 4, 1)],
        [('LROWS', 2, 2, 4, 4, 1), ('COL1D', 2, 2, 16, 256)]),
    "lrows-256-L1": ([('COL1D', 0, 1, 16, 256), ('ROWS', 0, 1, 8, 2, 2, 1, 32, 32)],
        [('ROWS', 1, 1, 8, 2, 2, 1, 32, 32), ('COL1D', 1, 1, 16, 256)]),
    "lrows-256-odd": ([('COL1D', 0, 1, 32, 256), ('ROWS', 0, 1, 6, 2, 2, 1, 32, 32)],
        [('ROWS', 1, 1, 6, 2, 2, 1, 32, 32), ('COL1D', 1, 1, 32, 256)]),
    "lrows-512-L6": ([('COL1D', 0, 6, 64, 512), ('LROWS', 0, 6, 4, 3, 2)],
        [('LROWS', 6, 6, 4, 3, 2), ('COL1D', 6, 6, 64, 512)]),
    "lrows-512-L5": ([('COL1D', 0, 5, 64, 512), ('ROWS', 0, 5, 8, 2, 2, 1, 16, 20)],
        [('ROWS', 5, 5, 8, 2, 2, 1, 16, 20), ('COL1D', 5, 5, 64, 512)]),
    "lrows-512-W": ([('COL1D', 0, 6, 64, 512), ('LROWS', 0, 6, 2, 3, 2)],
        [('LROWS', 6, 6, 2, 3, 2), ('COL1D', 6, 6, 64, 512)]),
    "lrows-256x256-L8": ([('COL1D', 0, 8, 256, 256), ('LROWS', 0, 8, 4, 4, 1)],
        [('LROWS', 8, 8, 4, 4, 1), ('COL1D', 8, 8, 256, 256)]),
    "lrows-256-F2": ([('COL1D', 0, 2, 16, 256), ('LROWS', 0, 2, 1, 4, 1)],
        [('LROWS', 2, 2, 1, 4, 1), ('COL1D', 2, 2, 16, 256)]),
    "lrows-256-F4": ([('COL1D', 0, 2, 16, 256), ('LROWS', 0, 2, 2, 4, 1)],
        [('LROWS', 2, 2, 2, 4, 1), ('COL1D', 2, 2, 16, 256)]),
    "lrows-256-F12": ([('COL1D', 0, 2, 16, 256), ('LROWS', 0, 2, 6, 4, 1)],
        [('LROWS', 2, 2, 6, 4, 1), ('COL1D', 2, 2, 16, 256)]),
    "lrows-256-F16": ([('COL1D', 0, 2, 16, 256), ('LROWS', 0, 2, 8, 4, 1)],
        [('LROWS', 2, 2, 8, 4, 1), ('COL1D', 2, 2, 16, 256)]),
    "lrows-512-F2": ([('COL1D', 0, 6, 64, 512), ('LROWS', 0, 6, 1, 3, 2)],
        [('LROWS', 6, 6, 1, 3, 2), ('COL1D', 6, 6, 64, 512)]),
    "lrows-512-F12": ([('COL1D', 0, 6, 64, 512), ('LROWS', 0, 6, 6, 3, 2)],
        [('LROWS', 6, 6, 6, 3, 2), ('COL1D', 6, 6, 64, 512)]),
    "lrows-512-F16": ([('COL1D', 0, 6, 64, 512), ('LROWS', 0, 6, 8, 3, 2)],
        [('LROWS', 6, 6, 8, 3, 2), ('COL1D', 6, 6, 64, 512)]),
    "l2d-256-B2": ([('L2DF', 0, 5, 4, 1, 0, 1)],
        [('L2DF', 5, 5, 4, 1, 0, 1)]),
    "l2d-256-B3": ([('L2DF', 0, 5, 4, 1, 0, 2)],
        [('L2DF', 5, 5, 4, 1, 0, 2)]),
    "l2d-256-L8": ([('L2DC', 0, 8, 4, 1, 1), ('L2DC', 0, 8, 4, 1, 2)],
        [('L2DF', 8, 8, 4, 1, 1, 1)]),
    "l2d-256-F20": ([('L2DC', 0, 5, 10, 1, 1), ('L2DC', 0, 5, 10, 1, 2)],
        [('L2DF', 5, 5, 10, 1, 0, 1)]),
    "l2d-256-L4": ([('COL1D', 0, 4, 256, 256), ('ROWS', 0, 4, 8, 4, 2, 0, 64, 64)],
        [('ROWS', 4, 4, 8, 4, 2, 0, 64, 64), ('COL1D', 4, 4, 256, 256)]),
    "l2d-512-L6": ([('L2DF', 0, 6, 4, 0, 0, 2)],
        [('L2DF', 6, 6, 4, 0, 0, 2)]),
    "l2d-512-F4-L9": ([('L2DF', 0, 9, 2, 0, 1, 2)],
        [('L2DF', 9, 9, 2, 0, 1, 2)]),
    "l2d-1024-L7": ([('L2DF', 0, 7, 4, 2, 0, 2)],
        [('L2DF', 7, 7, 4, 2, 0, 2)]),
    "l2d-1024-L3": ([('COL1D', 0, 3, 1024, 1024), ('ROWS', 0, 3, 8, 4, 2, 1, 16, 20)],
        [('ROWS', 3, 3, 8, 4, 2, 1, 16, 20), ('COL1D', 3, 3, 1024, 1024)]),
    "l2d-1024-F4-L8": ([('L2DF', 0, 8, 2, 2, 1, 2)],
        [('L2DF', 8, 8, 2, 2, 1, 2)]),
    "l2d-1024-F20": ([('L2DF', 0, 7, 10, 2, 0, 2)],
        [('L2DF', 7, 7, 10, 2, 0, 2)]),
    "l2d-256-F2": ([('L2DF', 0, 5, 1, 1, 0, 1)],
        [('L2DF', 5, 5, 1, 1, 0, 1)]),
    "l2d-256-F4": ([('L2DF', 0, 5, 2, 1, 0, 1)],
        [('L2DF', 5, 5, 2, 1, 0, 1)]),
    "l2d-256-F12": ([('L2DF', 0, 5, 6, 1, 0, 1)],
        [('L2DF', 5, 5, 6, 1, 0, 1)]),
    "l2d-256-F16": ([('L2DF', 0, 5, 8, 1, 0, 1)],
        [('L2DF', 5, 5, 8, 1, 0, 1)]),
    "l2d-512-F2": ([('L2DF', 0, 6, 1, 0, 0, 2)],
        [('L2DF', 6, 6, 1, 0, 0, 2)]),
    "l2d-512-F4": ([('L2DF', 0, 6, 2, 0, 0, 2)],
        [('L2DF', 6, 6, 2, 0, 0, 2)]),
    "l2d-512-F12": ([('L2DF', 0, 6, 6, 0, 0, 2)],
        [('L2DF', 6, 6, 6, 0, 0, 2)]),
    "l2d-512-F16": ([('L2DF', 0, 6, 8, 0, 0, 2)],
        [('L2DF', 6, 6, 8, 0, 0, 2)]),
    "l2d-512-F20": ([('L2DF', 0, 6, 10, 0, 0, 2)],
        [('L2DF', 6, 6, 10, 0, 0, 2)]),
    "l2d-1024-F2": ([('L2DF', 0, 7, 1, 2, 0, 2)],
        [('L2DF', 7, 7, 1, 2, 0, 2)]),
    "l2d-1024-F4": ([('L2DF', 0, 7, 2, 2, 0, 2)],
        [('L2DF', 7, 7, 2, 2, 0, 2)]),
    "l2d-1024-F12": ([('L2DF', 0, 7, 6, 2, 0, 2)],
        [('L2DF', 7, 7, 6, 2, 0, 2)]),
    "l2d-1024-F16": ([('L2DF', 0, 7, 8, 2, 0, 2)],
        [('L2DF', 7, 7, 8, 2, 0, 2)]),
    "l2d-256-F2-deep": ([('L2DC', 0, 6, 1, 1, 1), ('L2DC', 0, 6, 1, 1, 2)],
        [('L2DF', 6, 6, 1, 1, 1, 1)]),
    "l2d-512-F2-deep": ([('L2DF', 0, 7, 1, 0, 1, 2)],
        [('L2DF', 7, 7, 1, 0, 1, 2)]),
    "l2d-1024-F2-deep": ([('L2DF', 0, 8, 1, 2, 1, 2)],
        [('L2DF', 8, 8, 1, 2, 1, 2)]),
    "l2d-256-F4-deep": ([('L2DC', 0, 6, 2, 1, 1), ('L2DC', 0, 6, 2, 1, 2)],
        [('L2DF', 6, 6, 2, 1, 1, 1)]),
    "l2d-512-F4-deep": ([('L2DF', 0, 7, 2, 0, 1, 2)],
        [('L2DF', 7, 7, 2, 0, 1, 2)]),
    "l2d-1024-F4-deep": ([('L2DF', 0, 8, 2, 2, 1, 2)],
        [('L2DF', 8, 8, 2, 2, 1, 2)]),
    "l2d-256-F8-deep": ([('L2DC', 0, 6, 4, 1, 1), ('L2DC', 0, 6, 4, 1, 2)],
        [('L2DF', 6, 6, 4, 1, 1, 1)]),
    "l2d-512-F8-deep": ([('L2DF', 0, 7, 4, 0, 1, 2)],
        [('L2DF', 7, 7, 4, 0, 1, 2)]),
    "l2d-1024-F8-deep": ([('L2DF', 0, 8, 4, 2, 1, 2)],
        [('L2DF', 8, 8, 4, 2, 1, 2)]),
    "l2d-256-F12-deep": ([('L2DC', 0, 6, 6, 1, 1), ('L2DC', 0, 6, 6, 1, 2)],
        [('L2DF', 6, 6, 6, 1, 1, 1)]),
    "l2d-512-F12-deep": ([('L2DF', 0, 7, 6, 0, 1, 2)],
        [('L2DF', 7, 7, 6, 0, 1, 2)]),
    "l2d-1024-F12-deep": ([('L2DF', 0, 8, 6, 2, 1, 2)],
        [('L2DF', 8, 8, 6, 2, 1, 2)]),
    "l2d-256-F16-deep": ([('L2DC', 0, 6, 8, 1, 1), ('L2DC', 0, 6, 8, 1, 2)],
        [('L2DF', 6, 6, 8, 1, 1, 1)]),
    "l2d-512-F16-deep": ([('L2DF', 0, 7, 8, 0, 1, 2)],
        [('L2DF', 7, 7, 8, 0, 1, 2)]),
    "l2d-1024-F16-deep": ([('L2DF', 0, 8, 8, 2, 1, 2)],
        [('L2DF', 8, 8, 8, 2, 1, 2)]),
    "l2d-256-F20-deep": ([('L2DC', 0, 6, 10, 1, 1), ('L2DC', 0, 6, 10, 1, 2)],
        [('L2DF', 6, 6, 10, 1, 1, 1)]),
    "l2d-512-F20-deep": ([('L2DF', 0, 7, 10, 0, 1, 2)],
        [('L2DF', 7, 7, 10, 0, 1, 2)]),
    "l2d-1024-F20-deep": ([('L2DF', 0, 8, 10, 2, 1, 2)],
        [('L2DF', 8, 8, 10, 2, 1, 2)]),
    "l2d-256-B1": ([('COL1D', 0, 5, 256, 256), ('ROWS', 0, 5, 8, 4, 2, 0, 64, 64)],
        [('ROWS', 5, 5, 8, 4, 2, 0, 64, 64), ('COL1D', 5, 5, 256, 256)]),
    "tile-f64-F2": ([('TILEP', 0, 1, 2, 1, 1, 4), ('TILEP', 1, 1, 2, 1, 1, 1)],
        [('ITILEP', 2, 1, 2, 1, 1, 1), ('ITILEP', 1, 1, 2, 1, 1, 4)]),
    "tile-f64-F4": ([('TILEP', 0, 1, 4, 1, 1, 4), ('TILEP', 1, 1, 4, 1, 1, 1)],
        [('ITILEP', 2, 1, 4, 1, 1, 1), ('ITILEP', 1, 1, 4, 1, 1, 4)]),
    "tile-f64-F6": ([('TILEP', 0, 1, 6, 1, 1, 4), ('TILEP', 1, 1, 6, 1, 1, 1)],
        [('ITILEP', 2, 1, 6, 1, 1, 1), ('ITILEP', 1, 1, 6, 1, 1, 4)]),
    "tile-f64-F8": ([('TILEP', 0, 1, 8, 1, 1, 4), ('TILEP', 1, 1, 8, 1, 1, 1)],
        [('ITILEP', 2, 1, 8, 1, 1, 1), ('ITILEP', 1, 1, 8, 1, 1, 4)]),
    "tile-f64-F10": ([('TILEP', 0, 1, 10, 1, 1, 4), ('TILEP', 1, 1, 10, 1, 1, 1)],
        [('ITILE', 2, 1, 10, 1, 1, 1), ('ITILE', 1, 1, 10, 1, 1, 4)]),
    "tile-f64-F12": ([('TILE', 0, 1, 12, 1, 1, 4), ('TILE', 1, 1, 12, 1, 1, 1)],
        [('ITILE', 2, 1, 12, 1, 1, 1), ('ITILE', 1, 1, 12, 1, 1, 4)]),
    "tile-f64-F14": ([('TILE', 0, 1, 14, 1, 1, 4), ('TILE', 1, 1, 14, 1, 1, 1)],
        [('ITILE', 2, 1, 14, 1, 1, 1), ('ITILE', 1, 1, 14, 1, 1, 4)]),
    "tile-f64-F16": ([('TILE', 0, 1, 16, 1, 1, 4), ('TILE', 1, 1, 16, 1, 1, 1)],
        [('ITILE', 2, 1, 16, 1, 1, 1), ('ITILE', 1, 1, 16, 1, 1, 4)]),
    "tile-f64-F18": ([('TILE', 0, 1, 18, 1, 1, 4), ('TILE', 1, 1, 18, 1, 1, 1)],
        [('ITILE', 2, 1, 18, 1, 1, 1), ('ITILE', 1, 1, 18, 1, 1, 4)]),
    "tile-f64-F20": ([('TILE', 0, 1, 20, 1, 1, 4), ('TILE', 1, 1, 20, 1, 1, 1)],
        [('ITILE', 2, 1, 20, 1, 1, 1), ('ITILE', 1, 1, 20, 1, 1, 4)]),
    "tile-f64-walk-F2": ([('TILEP', 0, 1, 2, 1, 1, 8), ('TILEP', 1, 1, 2, 1, 1, 8), ('TILE', 2, 1, 2, 0, 1, 8)],
        [('ITILE', 3, 1, 2, 0, 1, 8), ('ITILEP', 2, 1, 2, 1, 1, 8), ('ITILEP', 1, 1, 2, 1, 1, 8)]),
    "tile-f64-walk-F4": ([('TILEP', 0, 1, 4, 1, 1, 8), ('TILEP', 1, 1, 4, 1, 1, 8), ('TILE', 2, 1, 4, 0, 1, 8)],
        [('ITILE', 3, 1, 4, 0, 1, 8), ('ITILEP', 2, 1, 4, 1, 1, 8), ('ITILEP', 1, 1, 4, 1, 1, 8)]),
    "tile-f64-walk-F6": ([('TILEP', 0, 1, 6, 1, 1, 8), ('TILEP', 1, 1, 6, 1, 1, 8), ('TILE', 2, 1, 6, 0, 1, 8)],
        [('ITILE', 3, 1, 6, 0, 1, 8), ('ITILEP', 2, 1, 6, 1, 1, 8), ('ITILEP', 1, 1, 6, 1, 1, 8)]),
    "tile-f64-walk-F8": ([('TILEP', 0, 1, 8, 1, 1, 8), ('TILEP', 1, 1, 8, 1, 1, 8), ('TILE', 2, 1, 8, 0, 1, 8)],
        [('ITILE', 3, 1, 8, 0, 1, 8), ('ITILEP', 2, 1, 8, 1, 1, 8), ('ITILEP', 1, 1, 8, 1, 1, 8)]),
    "tile-f64-walk-F10": ([('TILEP', 0, 1, 10, 1, 1, 8), ('TILEP', 1, 1, 10, 1, 1, 8), ('TILE', 2, 1, 10, 0, 1, 8)],
        [('ITILE', 3, 1, 10, 0, 1, 8), ('ITILE', 2, 1, 10, 1, 1, 8), ('ITILE', 1, 1, 10, 1, 1, 8)]),
    "tile-f64-walk-F12": ([('TILE', 0, 1, 12, 1, 1, 8), ('TILE', 1, 1, 12, 1, 1, 8), ('TILE', 2, 1, 12, 0, 1, 8)],
        [('ITILE', 3, 1, 12, 0, 1, 8), ('ITILE', 2, 1, 12, 1, 1, 8), ('ITILE', 1, 1, 12, 1, 1, 8)]),
    "tile-f64-walk-F14": ([('TILE', 0, 1, 14, 1, 1, 8), ('TILE', 1, 1, 14, 1, 1, 8), ('TILE', 2, 1, 14, 0, 1, 8)],
        [('ITILE', 3, 1, 14, 0, 1, 8), ('ITILE', 2, 1, 14, 1, 1, 8), ('ITILE', 1, 1, 14, 1, 1, 8)]),
    "tile-f64-walk-F16": ([('TILE', 0, 1, 16, 1, 1, 8), ('TILE', 1, 1, 16, 1, 1, 8), ('TILE', 2, 1, 16, 0, 1, 8)],
        [('ITILE', 3, 1, 16, 0, 1, 8), ('ITILE', 2, 1, 16, 1, 1, 8), ('ITILE', 1, 1, 16, 1, 1, 8)]),
    "tile-f64-walk-F18": ([('TILE', 0, 1, 18, 1, 1, 8), ('TILE', 1, 1, 18, 1, 1, 8), ('TILE', 2, 1, 18, 0, 1, 8)],
        [('ITILE', 3, 1, 18, 0, 1, 8), ('ITILE', 2, 1, 18, 1, 1, 8), ('ITILE', 1, 1, 18, 1, 1, 8)]),
    "tile-f64-walk-F20": ([('TILE', 0, 1, 20, 1, 1, 8), ('TILE', 1, 1, 20, 1, 1, 8), ('TILE', 2, 1, 20, 0, 1, 8)],
        [('ITILE', 3, 1, 20, 0, 1, 8), ('ITILE', 2, 1, 20, 1, 1, 8), ('ITILE', 1, 1, 20, 1, 1, 8)]),
    "tile-f64-rand": ([('TILEP', 0, 1, 8, 1, 1, 16), ('TILEP', 1, 1, 8, 1, 1, 4), ('TILEP', 2, 1, 8, 1, 1, 3), ('TWO', 3, 1, 1, 0, 1, 7), ('TWO', 4, 1, 1, 0, 1, 15)],
        [('COPYB', 3, 0, 7), ('TWO', 5, 1, 1, 0, 1, 15), ('TWO', 4, 1, 1, 0, 1, 7), ('ITILEP', 3, 1, 8, 1, 1, 3), ('ITILEP', 2, 1, 8, 1, 1, 4), ('ITILEP', 1, 1, 8, 1, 1, 16)]),
    "tile-f64-deep": ([('TILEP', 0, 1, 4, 1, 1, 8), ('TILEP', 1, 1, 4, 1, 1, 6), ('TILE', 2, 1, 4, 0, 1, 8), ('TILE', 3, 1, 4, 0, 1, 8), ('TWO', 4, 1, 1, 0, 1, 100), ('TWO', 5, 1, 1, 0, 1, 325), ('TWO', 6, 1, 1, 0, 1, 1023)],
        [('COPYB', 4, 0, 100), ('TWO', 7, 1, 1, 0, 1, 1023), ('TWO', 6, 1, 1, 0, 1, 325), ('TWO', 5, 1, 1, 0, 1, 100), ('ITILE', 4, 1, 4, 0, 1, 8), ('ITILE', 3, 1, 4, 0, 1, 8), ('ITILEP', 2, 1, 4, 1, 1, 6), ('ITILEP', 1, 1, 4, 1, 1, 8)]),
    "tile-f64-idwt128": ([('TILEP', 0, 1, 8, 1, 1, 8), ('TILEP', 1, 1, 8, 1, 1, 2), ('TWO', 2, 1, 1, 0, 1, 1), ('TWO', 3, 1, 1, 0, 1, 1), ('TAIL', 0, 3, 8, 128)],
        [('COPYB', 2, 0, 1), ('TWO', 7, 1, 1, 0, 1, 1), ('TWO', 6, 1, 1, 0, 1, 1), ('TWO', 5, 1, 1, 0, 1, 1), ('TWO', 4, 1, 1, 0, 1, 1), ('TWO', 3, 1, 1, 0, 1, 1), ('ITILEP', 2, 1, 8, 1, 1, 2), ('ITILEP', 1, 1, 8, 1, 1, 8)]),
    "tile-f64-long": ([('TILEP', 0, 1, 8, 1, 1, 256), ('TILE', 1, 1, 8, 0, 1, 256)],
        [('ITILE', 2, 1, 8, 0, 1, 256), ('ITILEP', 1, 1, 8, 1, 1, 256)]),
    "two-f64-24x8": ([('TWO', 0, 1, 1, 1, 1, 1), ('TWO', 1, 1, 1, 0, 1, 4), ('TWO', 2, 1, 1, 0, 1, 16)],
        [('TWO', 3, 1, 1, 0, 1, 16), ('TWO', 2, 1, 1, 0, 1, 4), ('TWO', 1, 1, 1, 0, 1, 1)]),
    "two-f64-24x8-tree": ([('TWO', 0, 1, 1, 1, 1, 1), ('TWO', 1, 1, 1, 0, 1, 1)],
        [('TWO', 2, 1, 1, 0, 1, 1), ('TWO', 1, 1, 1, 0, 1, 1)]),
    "two-f64-4x4": ([('TWO', 0, 1, 1, 1, 1, 1), ('TWO', 1, 1, 1, 0, 1, 4)],
        [('TWO', 2, 1, 1, 0, 1, 4), ('TWO', 1, 1, 1, 0, 1, 1)]),
    "wpd-f64-128x64": ([('TILEP', 0, 1, 8, 0, 0, 4), ('TILEP', 1, 1, 8, 0, 0, 4), ('TILEP', 2, 1, 8, 0, 0, 4), ('TILEP', 3, 1, 8, 0, 0, 4), ('TWO', 4, 1, 0, 1)],
        [('ROWS', 5, 5, 8, 2, 0, 0, 32, 32), ('COL1D', 5, 5, 128, 64)]),
    "wpd-f64-128x64-F2": ([('TILEP', 0, 1, 2, 0, 0, 4), ('TILEP', 1, 1, 2, 0, 0, 4)],
        [('ROWS', 2, 2, 2, 2, 0, 0, 32, 32), ('COL1D', 2, 2, 128, 64)]),
    "wpd-f64-128x64-F4": ([('TILEP', 0, 1, 4, 0, 0, 4), ('TILEP', 1, 1, 4, 0, 0, 4)],
        [('ROWS', 2, 2, 4, 2, 0, 0, 32, 32), ('COL1D', 2, 2, 128, 64)]),
    "wpd-f64-128x64-F6": ([('TILEP', 0, 1, 6, 0, 0, 4), ('TILEP', 1, 1, 6, 0, 0, 4)],
        [('ROWS', 2, 2, 6, 2, 0, 0, 32, 32), ('COL1D', 2, 2, 128, 64)]),
    "wpd-f64-128x64-F10": ([('TILEP', 0, 1, 10, 0, 0, 4), ('TILEP', 1, 1, 10, 0, 0, 4)],
        [('ROWS', 2, 2, 10, 2, 0, 0, 32, 32), ('COL1D', 2, 2, 128, 64)]),
    "wpd-f64-128x64-F12": ([('TILE', 0, 1, 12, 0, 0, 4), ('TILE', 1, 1, 12, 0, 0, 4)],
        [('ROWS', 2, 2, 12, 2, 0, 0, 32, 32), ('COL1D', 2, 2, 128, 64)]),
    "wpd-f64-128x64-F14": ([('TILE', 0, 1, 14, 0, 0, 4), ('TILE', 1, 1, 14, 0, 0, 4)],
        [('ROWS', 2, 2, 14, 1, 0, 0, 32, 32), ('COL1D', 2, 2, 128, 64)]),
    "wpd-f64-128x64-F16": ([('TILE', 0, 1, 16, 0, 0, 4), ('TILE', 1, 1, 16, 0, 0, 4)],
        [('ROWS', 2, 2, 16, 1, 0, 0, 32, 32), ('COL1D', 2, 2, 128, 64)]),
    "wpd-f64-128x64-F18": ([('TILE', 0, 1, 18, 0, 0, 4), ('TILE', 1, 1, 18, 0, 0, 4)],
        [('ROWS', 2, 2, 18, 1, 0, 0, 32, 32), ('COL1D', 2, 2, 128, 64)]),
    "wpd-f64-128x64-F20": ([('TILE', 0, 1, 20, 0, 0, 4), ('TILE', 1, 1, 20, 0, 0, 4)],
        [('ROWS', 2, 2, 20, 1, 0, 0, 32, 32), ('COL1D', 2, 2, 128, 64)]),
    "wpd-f64-tile": ([('TILEP', 0, 1, 10, 0, 0, 1), ('TILEP', 1, 1, 10, 0, 0, 1)],
        [('ROWS', 2, 2, 10, 2, 0, 0, 32, 32), ('COL1D', 2, 2, 64, 32)]),
    "wpd-f64-128-tree": ([('TILEP', 0, 1, 8, 0, 0, 8), ('TILEP', 1, 1, 8, 0, 0, 8), ('TILEP', 2, 1, 8, 0, 0, 8)],
        [('GATHER', 0, 0, 8, 4), ('COPYB', 2, 0, 4), ('TWO', 3, 1, 1, 0, 1, 4), ('ITILEP', 2, 1, 8, 1, 1, 4), ('ITILEP', 1, 1, 8, 1, 1, 8)]),
    "wpd-f64-24x8": ([('TWO', 0, 1, 0, 1), ('TWO', 1, 1, 0, 1)],
        [('TWO', 2, 1, 0, 1), ('TWO', 1, 1, 0, 1)]),
    "tile-f32-F2": ([('TILEP', 0, 1, 2, 1, 1, 4), ('TILEP', 1, 1, 2, 1, 1, 1)],
        [('ITILE', 2, 1, 2, 1, 1, 2), ('ITILE', 1, 1, 2, 1, 1, 8)]),
    "tile-f32-F4": ([('TILEP', 0, 1, 4, 1, 1, 4), ('TILEP', 1, 1, 4, 1, 1, 1)],
        [('ITILE', 2, 1, 4, 1, 1, 2), ('ITILE', 1, 1, 4, 1, 1, 8)]),
    "tile-f32-F6": ([('TILEP', 0, 1, 6, 1, 1, 4), ('TILEP', 1, 1, 6, 1, 1, 1)],
        [('ITILE', 2, 1, 6, 1, 1, 2), ('ITILE', 1, 1, 6, 1, 1, 8)]),
    "tile-f32-F8": ([('TILEP', 0, 1, 8, 1, 1, 4), ('TILEP', 1, 1, 8, 1, 1, 1)],
        [('ITILE', 2, 1, 8, 1, 1, 2), ('ITILE', 1, 1, 8, 1, 1, 8)]),
    "tile-f32-F10": ([('TILE', 0, 1, 10, 1, 1, 4), ('TILE', 1, 1, 10, 1, 1, 1)],
        [('ITILE', 2, 1, 10, 1, 1, 2), ('ITILE', 1, 1, 10, 1, 1, 8)]),
    "tile-f32-F12": ([('TILE', 0, 1, 12, 1, 1, 4), ('TILE', 1, 1, 12, 1, 1, 1)],
        [('ITILE', 2, 1, 12, 1, 1, 2), ('ITILE', 1, 1, 12, 1, 1, 8)]),
    "tile-f32-F14": ([('TILE', 0, 1, 14, 1, 1, 4), ('TILE', 1, 1, 14, 1, 1, 1)],
        [('ITILE', 2, 1, 14, 1, 1, 2), ('ITILE', 1, 1, 14, 1, 1, 8)]),
    "tile-f32-F16": ([('TILE', 0, 1, 16, 1, 1, 4), ('TILE', 1, 1, 16, 1, 1, 1)],
        [('ITILE', 2, 1, 16, 1, 1, 2), ('ITILE', 1, 1, 16, 1, 1, 8)]),
    "tile-f32-F18": ([('TILE', 0, 1, 18, 1, 1, 4), ('TILE', 1, 1, 18, 1, 1, 1)],
        [('ITILE', 2, 1, 18, 1, 1, 2), ('ITILE', 1, 1, 18, 1, 1, 8)]),
    "tile-f32-F20": ([('TILE', 0, 1, 20, 1, 1, 4), ('TILE', 1, 1, 20, 1, 1, 1)],
        [('ITILE', 2, 1, 20, 1, 1, 2), ('ITILE', 1, 1, 20, 1, 1, 8)]),
    "tile-f32-walk-F2": ([('TILEP', 0, 1, 2, 1, 1, 4), ('TILEP', 1, 1, 2, 1, 1, 4), ('TILE', 2, 1, 2, 0, 1, 4)],
        [('ITILE', 3, 1, 2, 0, 1, 8), ('ITILE', 2, 1, 2, 1, 1, 8), ('ITILE', 1, 1, 2, 1, 1, 8)]),
    "tile-f32-walk-F4": ([('TILEP', 0, 1, 4, 1, 1, 4), ('TILEP', 1, 1, 4, 1, 1, 4), ('TILE', 2, 1, 4, 0, 1, 4)],
        [('ITILE', 3, 1, 4, 0, 1, 8), ('ITILE', 2, 1, 4, 1, 1, 8), ('ITILE', 1, 1, 4, 1, 1, 8)]),
    "tile-f32-walk-F6": ([('TILEP', 0, 1, 6, 1, 1, 4), ('TILEP', 1, 1, 6, 1, 1, 4), ('TILE', 2, 1, 6, 0, 1, 4)],
        [('ITILE', 3, 1, 6, 0, 1, 8), ('ITILE', 2, 1, 6, 1, 1, 8), ('ITILE', 1, 1, 6, 1, 1, 8)]),
    "tile-f32-walk-F8": ([('TILEP', 0, 1, 8, 1, 1, 4), ('TILEP', 1, 1, 8, 1, 1, 4), ('TILE', 2, 1, 8, 0, 1, 4)],
        [('ITILE', 3, 1, 8, 0, 1, 8), ('ITILE', 2, 1, 8, 1, 1, 8), ('ITILE', 1, 1, 8, 1, 1, 8)]),
    "tile-f32-walk-F10": ([('TILE', 0, 1, 10, 1, 1, 4), ('TILE', 1, 1, 10, 1, 1, 4), ('TILE', 2, 1, 10, 0, 1, 4)],
        [('ITILE', 3, 1, 10, 0, 1, 8), ('ITILE', 2, 1, 10, 1, 1, 8), ('ITILE', 1, 1, 10, 1, 1, 8)]),
    "tile-f32-walk-F12": ([('TILE', 0, 1, 12, 1, 1, 4), ('TILE', 1, 1, 12, 1, 1, 4), ('TILE', 2, 1, 12, 0, 1, 4)],
        [('ITILE', 3, 1, 12, 0, 1, 8), ('ITILE', 2, 1, 12, 1, 1, 8), ('ITILE', 1, 1, 12, 1, 1, 8)]),
    "tile-f32-walk-F14": ([('TILE', 0, 1, 14, 1, 1, 4), ('TILE', 1, 1, 14, 1, 1, 4), ('TILE', 2, 1, 14, 0, 1, 4)],
        [('ITILE', 3, 1, 14, 0, 1, 8), ('ITILE', 2, 1, 14, 1, 1, 8), ('ITILE', 1, 1, 14, 1, 1, 8)]),
    "tile-f32-walk-F16": ([('TILE', 0, 1, 16, 1, 1, 4), ('TILE', 1, 1, 16, 1, 1, 4), ('TILE', 2, 1, 16, 0, 1, 4)],
        [('ITILE', 3, 1, 16, 0, 1, 8), ('ITILE', 2, 1, 16, 1, 1, 8), ('ITILE', 1, 1, 16, 1, 1, 8)]),
    "tile-f32-walk-F18": ([('TILE', 0, 1, 18, 1, 1, 4), ('TILE', 1, 1, 18, 1, 1, 4), ('TILE', 2, 1, 18, 0, 1, 4)],
        [('ITILE', 3, 1, 18, 0, 1, 8), ('ITILE', 2, 1, 18, 1, 1, 8), ('ITILE', 1, 1, 18, 1, 1, 8)]),
    "tile-f32-walk-F20": ([('TILE', 0, 1, 20, 1, 1, 4), ('TILE', 1, 1, 20, 1, 1, 4), ('TILE', 2, 1, 20, 0, 1, 4)],
        [('ITILE', 3, 1, 20, 0, 1, 8), ('ITILE', 2, 1, 20, 1, 1, 8), ('ITILE', 1, 1, 20, 1, 1, 8)]),
    "tile-f32-rand": ([('TILEP', 0, 1, 8, 1, 1, 8), ('TILEP', 1, 1, 8, 1, 1, 2), ('TWO', 2, 1, 1, 0, 1, 3), ('TWO', 3, 1, 1, 0, 1, 7), ('TWO', 4, 1, 1, 0, 1, 15)],
        [('COPYB', 2, 0, 3), ('TWO', 5, 1, 1, 0, 1, 15), ('TWO', 4, 1, 1, 0, 1, 7), ('TWO', 3, 1, 1, 0, 1, 3), ('ITILE', 2, 1, 8, 1, 1, 4), ('ITILE', 1, 1, 8, 1, 1, 16)]),
    "tile-f32-deep": ([('TILEP', 0, 1, 4, 1, 1, 4), ('TILEP', 1, 1, 4, 1, 1, 3), ('TILE', 2, 1, 4, 0, 1, 4), ('TILE', 3, 1, 4, 0, 1, 4), ('TWO', 4, 1, 1, 0, 1, 100), ('TWO', 5, 1, 1, 0, 1, 325), ('TWO', 6, 1, 1, 0, 1, 1023)],
        [('COPYB', 4, 0, 100), ('TWO', 7, 1, 1, 0, 1, 1023), ('TWO', 6, 1, 1, 0, 1, 325), ('TWO', 5, 1, 1, 0, 1, 100), ('ITILE', 4, 1, 4, 0, 1, 8), ('ITILE', 3, 1, 4, 0, 1, 8), ('ITILE', 2, 1, 4, 1, 1, 6), ('ITILE', 1, 1, 4, 1, 1, 8)]),
    "tile-f32-idwt128": ([('TILEP', 0, 1, 8, 1, 1, 4), ('TILEP', 1, 1, 8, 1, 1, 1), ('TWO', 2, 1, 1, 0, 1, 1), ('TWO', 3, 1, 1, 0, 1, 1), ('TAIL', 0, 3, 8, 128)],
        [('COPYB', 2, 0, 1), ('TWO', 7, 1, 1, 0, 1, 1), ('TWO', 6, 1, 1, 0, 1, 1), ('TWO', 5, 1, 1, 0, 1, 1), ('TWO', 4, 1, 1, 0, 1, 1), ('TWO', 3, 1, 1, 0, 1, 1), ('ITILE', 2, 1, 8, 1, 1, 2), ('ITILE', 1, 1, 8, 1, 1, 8)]),
    "tile-f32-long": ([('TILEP', 0, 1, 8, 1, 1, 128), ('TILE', 1, 1, 8, 0, 1, 128)],
        [('ITILE', 2, 1, 8, 0, 1, 256), ('ITILE', 1, 1, 8, 1, 1, 256)]),
    "two-f32-24x8": ([('TWO', 0, 1, 1, 1, 1, 1), ('TWO', 1, 1, 1, 0, 1, 4), ('TWO', 2, 1, 1, 0, 1, 16)],
        [('TWO', 3, 1, 1, 0, 1, 16), ('TWO', 2, 1, 1, 0, 1, 4), ('TWO', 1, 1, 1, 0, 1, 1)]),
    "two-f32-24x8-tree": ([('TWO', 0, 1, 1, 1, 1, 1), ('TWO', 1, 1, 1, 0, 1, 1)],
        [('TWO', 2, 1, 1, 0, 1, 1), ('TWO', 1, 1, 1, 0, 1, 1)]),
    "two-f32-4x4": ([('TWO', 0, 1, 1, 1, 1, 1), ('TWO', 1, 1, 1, 0, 1, 4)],
        [('TWO', 2, 1, 1, 0, 1, 4), ('TWO', 1, 1, 1, 0, 1, 1)]),
    "wpd-f32-128x64": ([('TILEP', 0, 1, 8, 0, 0, 2), ('TILEP', 1, 1, 8, 0, 0, 2), ('TILEP', 2, 1, 8, 0, 0, 2), ('TILEP', 3, 1, 8, 0, 0, 2), ('TWO', 4, 1, 0, 1)],
        [('ROWS', 5, 5, 8, 4, 0, 0, 64, 64), ('COL1D', 5, 5, 128, 64)]),
    "wpd-f32-128x64-F2": ([('TILEP', 0, 1, 2, 0, 0, 2), ('TILEP', 1, 1, 2, 0, 0, 2)],
        [('ROWS', 2, 2, 2, 4, 0, 0, 64, 64), ('COL1D', 2, 2, 128, 64)]),
    "wpd-f32-128x64-F4": ([('TILEP', 0, 1, 4, 0, 0, 2), ('TILEP', 1, 1, 4, 0, 0, 2)],
        [('ROWS', 2, 2, 4, 4, 0, 0, 64, 64), ('COL1D', 2, 2, 128, 64)]),
    "wpd-f32-128x64-F6": ([('TILEP', 0, 1, 6, 0, 0, 2), ('TILEP', 1, 1, 6, 0, 0, 2)],
        [('ROWS', 2, 2, 6, 4, 0, 0, 64, 64), ('COL1D', 2, 2, 128, 64)]),
    "wpd-f32-128x64-F10": ([('TILE', 0, 1, 10, 0, 0, 2), ('TILE', 1, 1, 10, 0, 0, 2)],
        [('ROWS', 2, 2, 10, 4, 0, 0, 64, 64), ('COL1D', 2, 2, 128, 64)]),
    "wpd-f32-128x64-F12": ([('TILE', 0, 1, 12, 0, 0, 2), ('TILE', 1, 1, 12, 0, 0, 2)],
        [('ROWS', 2, 2, 12, 4, 0, 0, 64, 64), ('COL1D', 2, 2, 128, 64)]),
    "wpd-f32-128x64-F14": ([('TILE', 0, 1, 14, 0, 0, 2), ('TILE', 1, 1, 14, 0, 0, 2)],
        [('ROWS', 2, 2, 14, 1, 0, 0, 64, 64), ('COL1D', 2, 2, 128, 64)]),
    "wpd-f32-128x64-F16": ([('TILE', 0, 1, 16, 0, 0, 2), ('TILE', 1, 1, 16, 0, 0, 2)],
        [('ROWS', 2, 2, 16, 1, 0, 0, 64, 64), ('COL1D', 2, 2, 128, 64)]),
    "wpd-f32-128x64-F18": ([('TILE', 0, 1, 18, 0, 0, 2), ('TILE', 1, 1, 18, 0, 0, 2)],
        [('ROWS', 2, 2, 18, 1, 0, 0, 64, 64), ('COL1D', 2, 2, 128, 64)]),
    "wpd-f32-128x64-F20": ([('TILE', 0, 1, 20, 0, 0, 2), ('TILE', 1, 1, 20, 0, 0, 2)],
        [('ROWS', 2, 2, 20, 1, 0, 0, 64, 64), ('COL1D', 2, 2, 128, 64)]),
    "wpd-f32-tile": ([('TILE', 0, 1, 10, 0, 0, 1), ('TILE', 1, 1, 10, 0, 0, 1)],
        [('Q64', 2, 2, 6)]),
    "wpd-f32-128-tree": ([('TILEP', 0, 1, 8, 0, 0, 4), ('TILEP', 1, 1, 8, 0, 0, 4), ('TILEP', 2, 1, 8, 0, 0, 4)],
        [('GATHER', 0, 0, 8, 4), ('COPYB', 2, 0, 4), ('TWO', 3, 1, 1, 0, 1, 4), ('ITILE', 2, 1, 8, 1, 1, 4), ('ITILE', 1, 1, 8, 1, 1, 8)]),
    "wpd-f32-24x8": ([('TWO', 0, 1, 0, 1), ('TWO', 1, 1, 0, 1)],
        [('TWO', 2, 1, 0, 1), ('TWO', 1, 1, 0, 1)]),
    "wrap-two": ([('TWO', 0, 1, 0, 1)],
        [('TWO', 1, 1, 0, 1)]),
    "wrap-two-act": ([('TWO', 0, 1, 1, 1, 1, 1)],
        [('TWO', 1, 1, 1, 0, 1, 1)]),
    "wrap-tilep": ([('TILEP', 0, 1, 8, 0, 0, 4)],
        None),
    "wrap-itilep": (None,
        [('ITILEP', 2, 1, 8, 1, 1, 1), ('ITILEP', 1, 1, 8, 1, 1, 4)]),
    "wrap-rows": ([('COL1D', 0, 3, 8, 64), ('ROWS', 0, 3, 8, 4, 0, 0, 64, 64)],
        [('ROWS', 3, 3, 8, 4, 0, 0, 64, 64), ('COL1D', 3, 3, 8, 64)]),
    "wrap-pyr": ([('PYR', 0, 4, 4, 4, 4)],
        [('PYR', 4, 4, 4, 4, 4)]),
    "wrap-copyb": (None,
        [('COPYB', 1, 0, 1), ('TWO', 2, 1, 1, 0, 1, 1), ('ITILE', 1, 1, 4, 1, 1, 4)]),
    "wrap-gather": (None,
        [('GATHER', 0, 0, 4, 3), ('COPYB', 1, 0, 1), ('TWO', 2, 1, 1, 0, 1, 1), ('ITILE', 1, 1, 4, 1, 1, 2)]),
}
# <<< PINS

# per route, which extras name the template instance (the others are geometry)
INSTANCE = {"Q64W": 1, "Q64TPREP": 0, "Q64T": 1, "Q64": 1, "PYR": 1, "TAIL": 1, "L2DF": 3, "L2DC": 3, "COL1D": 0, "LROWS": 2, "ROWS": 4,
            "TILE": 3, "TILEP": 3, "ITILE": 3, "ITILEP": 3, "TWO": 3, "COPYB": 0, "GATHER": 0}


def _reachable():
    """What the module docstring declares reachable, written from the launchers' switches and conditions and NOT from a record:
    (route, element size, direction, extras that name the instance).  A dispatch change that adds an instance has to add it
    here and give it a case; tools/dwt2d_pins.py never writes this."""
    FS = (2, 4, 6, 8, 10, 12, 14, 16, 18, 20)               # the taps of the row, tile and tail switches
    NSQ = (1, 2, 4, 6, 8)                                    # lattice stages built for Float64 registers (F <= 16)
    NSL = NSQ + (10,)                                        # ... and for the Float32 2-D lattice (F <= 20)
    both, r = ((8, 0), (8, 1), (4, 0), (4, 1)), set()
    r |= {("Q64W", es, 0, (ns,)) for es in (8, 4) for ns in (1, 2, 4)}                     # F <= 8; 3 stages run as 4
    r |= {(rt, es, d, (ns,)) for rt in ("Q64T", "Q64") for es, d in both for ns in NSQ}
    r |= {("Q64TPREP", es, d, ()) for es, d in both}
    r |= {("PYR", es, d, (ft,)) for es, d in both for ft in (0, 2, 4, 6, 8)}
    r |= {("TAIL", es, 0, (F,)) for es in (8, 4) for F in FS}
    # fused Float32 lattice (NS, HB, E): the inverse takes everything; the forward declines 256 x 256 (HB 1) with node matrices
    # (E = 1) or ten stages, which run as the pair L2DC (NS, HB, pass)
    r |= {("L2DF", 4, 1, (ns, hb, e)) for ns in NSL for hb in (0, 1, 2) for e in (0, 1)}
    r |= {("L2DF", 4, 0, (ns, hb, e)) for ns in NSL for hb in (0, 2) for e in (0, 1)}
    r |= {("L2DF", 4, 0, (ns, 1, 0)) for ns in NSQ}
    r |= {("L2DC", 4, 0, (ns, 1, p)) for ns in NSL for p in (1, 2)}
    r |= {("COL1D", es, d, ()) for es, d in both}
    r |= {("LROWS", 8, d, (ns, sh)) for d in (0, 1) for ns in NSQ for sh in (3, 4, 5)}
    # k_rows_fused (F, V, KI, REGL): vectors up to 12 taps; in place (KI = 2) up to 8 taps -- Float64 always with register levels,
    # Float32 with them from 1024 columns on
    for d in (0, 1):
        for F in FS:
            r |= {("ROWS", 8, d, (F, 2 if F <= 12 else 1, 0, 0)), ("ROWS", 4, d, (F, 4 if F <= 12 else 1, 0, 0))}
            if F <= 8:
                r |= {("ROWS", 8, d, (F, 2, 2, 1)), ("ROWS", 4, d, (F, 4, 2, 0)), ("ROWS", 4, d, (F, 4, 2, 1))}
    # tile levels (F, by_node, status): a whole-image walk under a tree (0, 1) is never persistent; wpd (0, 0) and node lists
    # (1, 1) are persistent up to 10 taps in Float64 and 8 in Float32 (forward), up to 8 taps in Float64 only (inverse)
    for F in FS:
        for es, pmax, ipmax in ((8, 10, 8), (4, 8, 0)):
            r.add(("TILE", es, 0, (F, 0, 1)))
            r |= {("TILEP" if F <= pmax else "TILE", es, 0, (F, 0, 0)), ("TILEP" if F <= pmax else "TILE", es, 0, (F, 1, 1))}
            r.add(("ITILE", es, 1, (F, 0, 1)))
            r.add(("ITILEP" if F <= ipmax else "ITILE", es, 1, (F, 1, 1)))
    # two-pass level (node list, copy_inactive, status): only the root of a forward tree copies the other blocks
    r |= {("TWO", es, d, e) for es, d in both for e in ((0, 1, 0), (1, 0, 1))}
    r |= {("TWO", es, 0, (1, 1, 1)) for es in (8, 4)}
    r |= {(rt, es, 1, ()) for rt in ("COPYB", "GATHER") for es in (8, 4)}
    return r


REACHABLE = _reachable()

RECORD = None                                             # a dict: tools/dwt2d_pins.py collects the traces instead of comparing them


def _wt(wx, F):
    return wx.wavelet(getattr(wx.WT, WF[F]))


def _key(tr):
    out = []
    for t in tr:
        e = [t.e0, t.e1, t.e2, t.e3, t.e4, t.e5]
        while e and e[-1] == 0:
            e.pop()
        out.append((t.route, t.depth, t.K) + tuple(e))
    return out


def _instances(rows, es, inverse):
    out = set()
    for r in rows:
        e = tuple(r[3:]) + (0,) * 6
        out.add((r[0], es, inverse, e[:INSTANCE[r[0]]]))
    return out


def _need(cid, which, tr, dtype):
    """the trace of a case against PINS[cid][which] (0 = forward, 1 = inverse)"""
    assert tr.dropped == 0
    assert all(t.inverse == which and t.elem_size == np.dtype(dtype).itemsize for t in tr), (cid, list(tr))
    got = _key(tr)
    if RECORD is not None:
        RECORD.setdefault(cid, [None, None])[which] = got
        return
    want = [tuple(w) for w in PINS[cid][which]]
    assert got == want, "%s %s: written for %s, took %s" % (cid, ("forward", "inverse")[which], want, got)


def _noise(wx, shape, dtype, seed):
    import torch
    x = wx.jl_empty(shape, torch.float64 if dtype == F64 else torch.float32, "cuda")
    x.normal_(generator=torch.Generator(device="cuda").manual_seed(seed))
    return x


def _off(a):
    """numpy (Julia shape) -> column-major device tensor whose first element sits one element past an aligned allocation"""
    import torch
    a = np.asfortranarray(a)
    flat = torch.empty(a.size + 1, dtype=torch.float64 if a.dtype == np.float64 else torch.float32, device="cuda")
    flat[1:].copy_(torch.from_numpy(np.ascontiguousarray(a.T).reshape(-1)))
    t = flat[1:].view(tuple(reversed(a.shape)))
    return t.permute(*reversed(range(a.ndim)))


def _close_imgs(got, exp, tol, what):
    """every image (last axis) within tol of that image's own largest magnitude"""
    got = np.asarray(got, dtype=np.float64)
    exp = np.asarray(exp, dtype=np.float64)
    assert got.shape == exp.shape, (what, got.shape, exp.shape)
    ax = tuple(range(got.ndim - 1))
    err = np.abs(got - exp).max(axis=ax)
    den = np.abs(exp).max(axis=ax)
    rel = err / np.where(den > 0, den, 1.0)
    b = int(np.argmax(rel))
    if RECORD is not None:
        RECORD.setdefault("err", {})[what] = float(rel[b])
    assert np.isfinite(got).all() and rel[b] <= tol, "%s: image %d: error %.3g of the image's maximum (tolerance %.3g)" % (
        what, b, rel[b], tol)


def _stack(fn, X, *a):
    X = np.asarray(X, dtype=np.float64)
    return np.asfortranarray(np.stack([fn(np.asfortranarray(X[..., i]), *a) for i in range(X.shape[-1])], axis=-1))


def _tree(wx, m, n, spec):
    """the int depth of a full tree, or the boolean quad tree (heap order) of a spec"""
    if spec is None or isinstance(spec, int):
        return spec
    Lmax = wx.maxtransformlevels(min(m, n))
    if spec[0] == "dwt":
        return np.asarray(wx.maketree(m, n, spec[1], "dwt"), dtype=bool)
    if spec[0] == "nodes":
        t = np.zeros((4 ** Lmax - 1) // 3, dtype=bool)
        t[np.asarray(spec[1]) - 1] = True
        return t
    _, p, depth, seed = spec
    t = np.array(random_tree_2d(m, n, np.random.default_rng(seed), p), dtype=bool)
    t[(4 ** depth - 1) // 3:] = False
    return t


class _forced:
    """wx.set_force_generic(1) for a block: one level per launch"""

    def __init__(self, wx):
        self.wx = wx

    def __enter__(self):
        self.wx.set_force_generic(1)

    def __exit__(self, *exc):
        self.wx.set_force_generic(0)


def _fwd(wx, c, x, wt, arg):
    if c.op == "wpd":
        return wx.wpdall(x, wt, arg)
    if c.op == "dwt":
        return wx.dwtall(x, wt, arg)
    if c.inplace:
        y = x.clone()
        wx.wpt_(y[:, :, 0], y[:, :, 0], wt, arg)
        return y
    return wx.wptall(x, wt, arg)


def _inv(wx, c, xw, wt, arg):
    if c.op == "wpd":
        return wx.iwpdall(xw, wt, arg)
    if c.op == "dwt":
        return wx.idwtall(xw, wt, arg)
    if c.inplace:
        y = xw.clone()
        wx.iwpt_(y[:, :, 0], y[:, :, 0], wt, arg)
        return y
    return wx.iwptall(xw, wt, arg)


def _oracle_pair(wx, oracle, c, xh, qmf):
    """(forward reference, the inverse's argument, function of the coefficients that gives the inverse reference)"""
    if c.op == "wpd":
        iarg = _tree(wx, c.m, c.n, c.iarg) if c.iarg is not None else c.arg
        return _stack(oracle.wpd, xh, qmf, c.arg), iarg, lambda w: _stack(oracle.iwpd, w, qmf, iarg)
    tree = _tree(wx, c.m, c.n, ("dwt", c.arg)) if c.op == "dwt" else _tree(wx, c.m, c.n, c.arg)
    return _stack(oracle.wpt, xh, qmf, tree), (c.arg if c.op == "dwt" else tree), lambda w: _stack(oracle.iwpt, w, qmf, tree)


def _only_two_pass(tr):
    return {t.route for t in tr} <= {"TWO"}


def run_case(wx, oracle, c):
    wt = _wt(wx, c.F)
    tol = c.tol or TOL[np.dtype(c.dtype)]
    assert tol <= TOL[np.dtype(c.dtype)]
    agree = 1e-13 if c.dtype == F64 else TOL[np.dtype(c.dtype)]
    x = _noise(wx, (c.m, c.n, c.B), c.dtype, 9000 + c.m + 3 * c.n + c.F)
    xh = wx.to_numpy(x)
    exp, iarg, oinv = _oracle_pair(wx, oracle, c, xh, wt.qmf)
    farg = c.arg if c.op in ("wpd", "dwt") else _tree(wx, c.m, c.n, c.arg)
    with wx.dwt2d_trace() as tr:
        got = _fwd(wx, c, x, wt, farg)
    _need(c.id, 0, tr, c.dtype)
    goth = wx.to_numpy(got)
    assert goth.dtype == c.dtype
    _close_imgs(goth, exp, tol, c.id + " forward")
    if c.forced:
        with _forced(wx), wx.dwt2d_trace() as trf:
            ref = wx.to_numpy(_fwd(wx, c, x, wt, farg))
        assert _only_two_pass(trf) and len(trf), (c.id, _key(trf))
        _close_imgs(goth, ref, agree, c.id + " forward against one level per launch")
    # the inverse of the oracle's coefficients, in the case's type
    coef = np.asfortranarray(exp, dtype=c.dtype)
    cd = _off(coef) if c.off else wx.to_device(coef)
    if c.off:
        assert cd.data_ptr() % 16 in (4, 8)
    with wx.dwt2d_trace() as tr:
        back = _inv(wx, c, cd, wt, iarg)
    _need(c.id, 1, tr, c.dtype)
    backh = wx.to_numpy(back)
    assert backh.dtype == c.dtype
    _close_imgs(backh, oinv(coef), tol, c.id + " inverse against the oracle")
    _close_imgs(backh, xh, 20 * tol, c.id + " inverse against the image")
    if c.forced:
        with _forced(wx), wx.dwt2d_trace() as trf:
            ref = wx.to_numpy(_inv(wx, c, cd, wt, iarg))
        assert _only_two_pass(trf) and len(trf), (c.id, _key(trf))
        _close_imgs(backh, ref, agree, c.id + " inverse against one level per launch")


@gpu
@pytest.mark.parametrize("cid", [c.id for c in CASES_A])
def test_route_and_parity(wx, oracle, cid):
    run_case(wx, oracle, CASE_BY_ID[cid])


# ---- b. every grid wrap-around loop goes round -------------------------------------------------------------------------------
class Wrap:
    """a part a case with B images, of which the images b >= P are copies of image b mod P; `route`: the route of which one
    launch at least must have a grid smaller than its work items, `items`: work items per image of a launch (a function of the
    recorded row)"""

    def __init__(self, cid, op, dtype, m, n, arg, F, B, route, items, forced=False, iarg=None, inverse=None):
        self.case = Case(cid, op, dtype, m, n, arg, F, B=B, iarg=iarg)
        self.route, self.items, self.forced, self.inverse = route, items, forced, inverse


WRAPS = [
    # two-pass level: a thread per output pair, 256 per workgroup, at most 8192 workgroups
    Wrap("wrap-two", "wpt", F32, 64, 64, 1, 8, 1100, "TWO", lambda t: 64 * 64 / 2 / 256, forced=True),
    # the same by node list (a full tree on sides that are no power of two: one node of 24 x 8 per image)
    Wrap("wrap-two-act", "wpt", F32, 24, 8, 1, 4, 22000, "TWO", lambda t: 24 * 8 / 2 / 256),
    # persistent forward tile level: a tile per turn
    Wrap("wrap-tilep", "wpd", F64, 128, 64, 1, 8, 300, "TILEP", lambda t: t.e3, inverse=0),
    # persistent inverse tile level (Float64, up to 8 taps, by node list)
    Wrap("wrap-itilep", "wpt", F64, 128, 64, ("nodes", [1, 3]), 8, 300, "ITILEP", lambda t: t.e3, inverse=1),
    # row strips: a strip of R rows per turn
    Wrap("wrap-rows", "wpt", F32, 8, 64, 3, 8, 1300, "ROWS", lambda t: -(-8 // t.e4)),
    # LDS pyramid: an image per turn
    Wrap("wrap-pyr", "dwt", F64, 16, 16, 4, 4, 2100, "PYR", lambda t: 1),
    # block copy ahead of the small inverse levels, and the leaf gather of iwpd: an element per thread, at most 8192 workgroups
    Wrap("wrap-copyb", "wpt", F32, 128, 64, ("nodes", [1, 3]), 4, 1100, "COPYB", lambda t: 64 * 32 / 256, inverse=1),
    Wrap("wrap-gather", "wpd", F32, 64, 64, 2, 4, 600, "GATHER", lambda t: 64 * 64 / 256, iarg=("nodes", [1, 3]), inverse=1),
]
WRAP_BY_ID = {w.case.id: w for w in WRAPS}


def _copies(wx, c, seed):
    import torch
    x = _noise(wx, (c.m, c.n, c.B), c.dtype, seed)
    idx = torch.arange(c.B, device="cuda") % P
    x.copy_(x[:, :, idx].clone())
    return x, idx.cpu().numpy()


def _same_as_original(out, idx, what):
    """bit-identical: image b against image b mod P, for all b >= P"""
    import torch
    bits = out.view(torch.int64 if out.dtype == torch.float64 else torch.int32)
    assert torch.equal(bits, bits.index_select(bits.ndim - 1, torch.as_tensor(idx, device=out.device))), what


def run_wrap(wx, oracle, w):
    import torch
    c = w.case
    wt = _wt(wx, c.F)
    tol = TOL[np.dtype(c.dtype)]
    x, idx = _copies(wx, c, 4242 + c.m)
    xh = wx.to_numpy(x[:, :, :P])
    head = Case(c.id, c.op, c.dtype, c.m, c.n, c.arg, c.F, B=P, iarg=c.iarg)
    exp, iarg, oinv = _oracle_pair(wx, oracle, head, xh, wt.qmf)
    farg = c.arg if c.op in ("wpd", "dwt") else _tree(wx, c.m, c.n, c.arg)
    seen = False

    def wrapped(tr, inverse):
        rows = [t for t in tr if t.route == w.route]
        if RECORD is not None:
            RECORD.setdefault(c.id, [None, None])[inverse] = _key(tr)
            RECORD.setdefault("grids", {})[c.id + str(inverse)] = [(t.grid_x, t.grid_y, t.grid_z) for t in rows]
        else:
            assert _key(tr) == [tuple(r) for r in PINS[c.id][inverse]], (c.id, inverse, _key(tr))
        return any(t.grid_y == 1 and t.grid_z == 1 and t.grid_x < w.items(t) * c.B for t in rows)

    if w.inverse != 1:
        if w.forced:
            wx.set_force_generic(1)
        try:
            with wx.dwt2d_trace() as tr:
                got = _fwd(wx, c, x, wt, farg)
        finally:
            wx.set_force_generic(0)
        seen |= wrapped(tr, 0)
        _same_as_original(got, idx, c.id + " forward")
        _close_imgs(wx.to_numpy(got[..., :P]), exp, tol, c.id + " forward")
    if w.inverse != 0:
        coef = np.asfortranarray(exp, dtype=c.dtype)
        cd = wx.to_device(coef)
        cd = cd.index_select(cd.ndim - 1, torch.as_tensor(idx, device="cuda"))
        cdj = wx.jl_empty(tuple(cd.shape), cd.dtype, "cuda")
        cdj.copy_(cd)
        if w.forced:
            wx.set_force_generic(1)
        try:
            with wx.dwt2d_trace() as tr:
                back = _inv(wx, c, cdj, wt, iarg)
        finally:
            wx.set_force_generic(0)
        seen |= wrapped(tr, 1)
        _same_as_original(back, idx, c.id + " inverse")
        _close_imgs(wx.to_numpy(back[..., :P]), oinv(coef), tol, c.id + " inverse against the oracle")
        _close_imgs(wx.to_numpy(back[..., :P]), xh, 20 * tol, c.id + " inverse against the image")
    assert seen, (c.id, w.route)


@gpu
@pytest.mark.parametrize("wid", [w.case.id for w in WRAPS])
def test_grid_loops_go_round(wx, oracle, wid):
    run_wrap(wx, oracle, WRAP_BY_ID[wid])


# ---- c. the table itself -----------------------------------------------------------------------------------------------------
def test_pins_cover_what_the_docstring_declares_reachable(wx):
    """every (route, type, instance) pinned in parts a and b is declared in REACHABLE and the other way round: a route or a
    template instance cannot be added to the dispatch (or lose its last case) without this file saying so"""
    cases = dict(CASE_BY_ID)
    cases.update({w.case.id: w.case for w in WRAPS})
    assert set(PINS) == set(cases), sorted(set(PINS) ^ set(cases))
    pinned = set()
    for cid, (f, i) in PINS.items():
        es = np.dtype(cases[cid].dtype).itemsize
        pinned |= _instances(f or [], es, 0) | _instances(i or [], es, 1)
    assert pinned == REACHABLE, "declared and not pinned: %s; pinned and not declared: %s" % (
        sorted(REACHABLE - pinned, key=repr), sorted(pinned - REACHABLE, key=repr))
    assert {r[0] for r in REACHABLE} == set(wx.DWT2D_ROUTES.values())
