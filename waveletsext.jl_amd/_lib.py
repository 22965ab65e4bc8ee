"""ctypes binding of libwaveletsext_hip.so (the C ABI in include/waveletsext_hip.h).

The product path has NO CPU fallback: if the shared library is missing this module raises on
import of the symbol table, and every compute entry point fails with WxError(WX_EHIP) when no
HIP device is visible.
"""
import collections
import contextlib
import ctypes
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
# WX_HIP_LIB: another build of the same library (kernel experiments); the default is the in-tree build
LIB_PATH = os.environ.get("WX_HIP_LIB") or os.path.join(_HERE, "csrc", "libwaveletsext_hip.so")

WX_OK, WX_EASSERT, WX_EARG, WX_EBOUNDS, WX_EHIP, WX_EUNSUPPORTED = 0, -1, -2, -3, -10, -11


class WxError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__("libwaveletsext_hip status %d: %s" % (code, msg))
        self.code = code


_lib = None


def lib():
    """Load the library once (RTLD_GLOBAL is not needed; HIP runtime comes in as a dependency)."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise ImportError(
                "libwaveletsext_hip.so is not built (%s). Run `python -c 'import __graft_entry__ as g; "
                "g.build()'` or `make -C waveletsext.jl_amd/csrc`. There is no CPU fallback." % LIB_PATH)
        _lib = ctypes.CDLL(LIB_PATH)
        _declare(_lib)
    return _lib


_P, _I, _L = ctypes.c_void_p, ctypes.c_int, ctypes.c_int64


def _declare(L):
    L.wx_version.restype = _I
    L.wx_last_error.restype = ctypes.c_char_p
    L.wx_device_count.restype = _I
    L.wx_build_info.restype = ctypes.c_char_p
    L.wx_debug_set_dispatch.argtypes = [_I]           # csrc/wx_debug.h: test-suite hook, not in the public header
    L.wx_debug_set_dispatch.restype = None
    L.wx_debug_red2d_route.argtypes = [_I, _L, _L, _I, _I, _I, _I, _I]
    L.wx_debug_red2d_route.restype = _I
    L.wx_debug_swt1d_trace_begin.argtypes = []
    L.wx_debug_swt1d_trace_begin.restype = None
    L.wx_debug_swt1d_trace_end.argtypes = [_P, _I]
    L.wx_debug_swt1d_trace_end.restype = _I
    L.wx_debug_swt1d_trace_dropped.argtypes = []
    L.wx_debug_swt1d_trace_dropped.restype = _L
    L.wx_debug_dwt2d_trace_begin.argtypes = []
    L.wx_debug_dwt2d_trace_begin.restype = None
    L.wx_debug_dwt2d_trace_end.argtypes = [_P, _I]
    L.wx_debug_dwt2d_trace_end.restype = _I
    L.wx_debug_dwt2d_trace_dropped.argtypes = []
    L.wx_debug_dwt2d_trace_dropped.restype = _L
    L.wx_debug_dwt1d_trace_begin.argtypes = []
    L.wx_debug_dwt1d_trace_begin.restype = None
    L.wx_debug_dwt1d_trace_end.argtypes = [_P, _I]
    L.wx_debug_dwt1d_trace_end.restype = _I
    L.wx_debug_dwt1d_trace_dropped.argtypes = []
    L.wx_debug_dwt1d_trace_dropped.restype = _L
    L.wx_debug_swt_inv_plan.argtypes = [_I, _I, _I, _L, _L, _I, _I, _I, _P]
    L.wx_debug_swt_inv_plan.restype = _I
    L.wx_debug_ldb_chunks.argtypes = [_L, _L, _I]
    L.wx_debug_ldb_chunks.restype = _I
    sigs = {
        # name: argtypes (without the _f64/_f32 suffix)
        "wx_wpd1d": [_P, _P, _L, _I, _L, _P, _I, _P],
        "wx_wpt1d": [_P, _P, _L, _I, _P, _L, _L, _P, _I, _P],
        "wx_iwpt1d": [_P, _P, _L, _I, _P, _L, _L, _P, _I, _P],
        "wx_iwpd1d": [_P, _P, _L, _I, _I, _P, _L, _L, _P, _I, _P],
        "wx_getbasiscoef1d": [_P, _P, _L, _I, _P, _L, _L, _P],
    }
    sigs.update(_EXTRA_SIGS)
    for name, args in sigs.items():
        for suf in ("_f64", "_f32"):
            if hasattr(L, name + suf):
                fn = getattr(L, name + suf)
                fn.argtypes = args
                fn.restype = _I
    for name, args in _PLAIN_SIGS.items():
        if hasattr(L, name):
            fn = getattr(L, name)
            fn.argtypes = args
            fn.restype = _I
    for name in ("wx_siwt_ncols", "wx_siwt_nnodes"):
        if hasattr(L, name):
            getattr(L, name).argtypes = [_I, _I]
            getattr(L, name).restype = _L


# filled in by the other host modules' families (SWT / ACWT / 2-D / JBB)
_EXTRA_SIGS = {
    "wx_wpd2d": [_P, _P, _L, _L, _I, _L, _P, _I, _P],
    "wx_wpt2d": [_P, _P, _L, _L, _I, _P, _L, _L, _P, _I, _P],
    "wx_iwpt2d": [_P, _P, _L, _L, _I, _P, _L, _L, _P, _I, _P],
    "wx_iwpd2d": [_P, _P, _L, _L, _I, _I, _P, _L, _L, _P, _I, _P],
    "wx_sdwt1d": [_P, _P, _L, _I, _L, _P, _I, _P],
    "wx_isdwt1d": [_P, _P, _L, _I, _L, _L, _P, _I, _P],
    "wx_swpt1d": [_P, _P, _L, _I, _L, _P, _I, _P],
    "wx_iswpt1d": [_P, _P, _L, _I, _L, _L, _P, _I, _P],
    "wx_swpd1d": [_P, _P, _L, _I, _L, _P, _I, _P],
    "wx_iswpd1d": [_P, _P, _L, _L, _I, _P, _L, _L, _L, _P, _I, _P],
    "wx_acdwt1d": [_P, _P, _L, _I, _L, _P, _I, _P],
    "wx_iacdwt1d": [_P, _P, _L, _I, _L, _P],
    "wx_acwpt1d": [_P, _P, _L, _I, _L, _P, _I, _P],
    "wx_iacwpt1d": [_P, _P, _L, _I, _L, _P],
    "wx_acwpd1d": [_P, _P, _L, _I, _L, _P, _I, _P],
    "wx_iacwpd1d": [_P, _P, _L, _L, _I, _P, _L, _L, _P],
    "wx_sdwt2d": [_P, _P, _L, _L, _I, _L, _P, _I, _P],
    "wx_swpt2d": [_P, _P, _L, _L, _I, _L, _P, _I, _P],
    "wx_swpd2d": [_P, _P, _L, _L, _I, _L, _P, _I, _P],
    "wx_isdwt2d": [_P, _P, _L, _L, _I, _L, _L, _P, _I, _P],
    "wx_iswpt2d": [_P, _P, _L, _L, _I, _L, _L, _P, _I, _P],
    "wx_iswpd2d": [_P, _P, _L, _L, _L, _I, _P, _L, _L, _L, _P, _I, _P],
    "wx_acdwt2d": [_P, _P, _L, _L, _I, _L, _P, _I, _P],
    "wx_acwpt2d": [_P, _P, _L, _L, _I, _L, _P, _I, _P],
    "wx_acwpd2d": [_P, _P, _L, _L, _I, _L, _P, _I, _P],
    "wx_iacdwt2d": [_P, _P, _L, _L, _I, _L, _P],
    "wx_iacwpt2d": [_P, _P, _L, _L, _I, _L, _P],
    "wx_iacwpd2d": [_P, _P, _L, _L, _L, _I, _P, _L, _L, _P],
    "wx_jbb_costs2d": [_P, _P, _L, _L, _L, _L, _I, _I, ctypes.c_double, _P, _P],
    "wx_getbasiscoef2d": [_P, _P, _L, _L, _I, _P, _L, _L, _P],
    "wx_getbasiscoef1d_trees": [_P, _P, _L, _I, _P, _L, _L, _P],
    "wx_getbasiscoef2d_trees": [_P, _P, _L, _L, _I, _P, _L, _L, _P],
    "wx_wpt1d_trees": [_P, _P, _L, _P, _L, _L, _P, _I, _P],
    "wx_iwpt1d_trees": [_P, _P, _L, _P, _L, _L, _P, _I, _P],
    "wx_iwpd1d_trees": [_P, _P, _L, _I, _P, _L, _L, _P, _I, _P],
    "wx_wpt2d_trees": [_P, _P, _L, _L, _P, _L, _L, _P, _I, _P],
    "wx_iwpt2d_trees": [_P, _P, _L, _L, _P, _L, _L, _P, _I, _P],
    "wx_iwpd2d_trees": [_P, _P, _L, _L, _I, _P, _L, _L, _P, _I, _P],
    "wx_denoise_wpt1d_trees": [_P, _P, _L, _P, _L, _L, _P, _I, _I, ctypes.c_double, _P, _L, _I, _P, _P],
    "wx_iswpd1d_trees": [_P, _P, _L, _L, _P, _L, _L, _L, _P, _I, _P],
    "wx_iacwpd1d_trees": [_P, _P, _L, _L, _P, _L, _L, _P],
    "wx_denoise_swpd1d_trees": [_P, _P, _L, _L, _P, _L, _L, _P, _I, _I, ctypes.c_double, _P, _L, _I, _P, _P],
    "wx_denoise_acwpd1d_trees": [_P, _P, _L, _L, _P, _L, _L, _I, ctypes.c_double, _P, _L, _I, _P, _P],
    "wx_jbb_moments": [_P, _P, _P, _L, _L, _I, _P],
    "wx_jbb_costs": [_P, _P, _L, _L, _L, _I, _I, ctypes.c_double, _P, _P],
    "wx_acwpd_jbb_moments": [_P, _P, _P, _L, _I, _L, _P, _I, _I, _P],
    "wx_siwpd": [_P, _P, _P, _L, _I, _I, _L, _P, _I, _P],
    "wx_siwt_bestbasis": [_P, _P, _I, _I, _L, _P],
    "wx_isiwpd": [_P, _P, _P, _L, _I, _I, _L, _P, _I, _I, _P],
    "wx_ns_dwt1d": [_P, _P, _L, _I, _L, _P, _I, _P],
    "wx_ns_idwt1d": [_P, _P, _L, _I, _L, _P, _I, _P],
    "wx_sft": [_P, _P, _L, _L, _I, _I, _P, _I, _P],
    "wx_sparseform_count": [_P, _L, _I, ctypes.c_double, _P, _P, _P],
    "wx_sparseform_fill": [_P, _L, _I, ctypes.c_double, _P, _P, _P, _P],
    "wx_wavemult_plan_create": [_P, _P, _P, _L, ctypes.POINTER(ctypes.c_void_p), _P],
    "wx_wavemult_apply": [_P, _I, _P, _P, _L, _I, _L, _P, _I, _P],
    "wx_wavemult_product": [_P, _P, _P, _L, _P],
}
_PLAIN_SIGS = {
    "wx_treeselect_f64": [_P, _L, _L, _I, _P],
    "wx_treeselect_f32": [_P, _L, _L, _I, _P],
    "wx_treeselect_gap_f64": [_P, _L, _L, _I, _P, _P],
    "wx_treeselect_gap_f32": [_P, _L, _L, _I, _P, _P],
    "wx_treeselect2d_f64": [_P, _L, _L, _L, _I, _P],
    "wx_treeselect2d_f32": [_P, _L, _L, _L, _I, _P],
    "wx_shutdown": [],
    "wx_wpt_trees_last_route": [],
    "wx_set_host_hugepages": [_I],
    "wx_energy_map_f64": [_P, _L, _L, _L, _P, _I, _P, _P, _P],
    "wx_energy_map_f32": [_P, _L, _L, _L, _P, _I, _P, _P, _P],
    "wx_class_mean_f64": [_P, _L, _L, _P, _I, _P, _P],
    "wx_class_mean_f32": [_P, _L, _L, _P, _I, _P, _P],
    "wx_class_var_f64": [_P, _L, _L, _P, _I, _P, _P, _P],
    "wx_class_var_f32": [_P, _L, _L, _P, _I, _P, _P, _P],
    "wx_class_median_mad_f64": [_P, _L, _L, _P, _I, _P, _P, _P],
    "wx_class_median_mad_f32": [_P, _L, _L, _P, _I, _P, _P, _P],
    "wx_emd_measure_f64": [_P, _L, _L, _P, _I, _P, _P],
    "wx_emd_measure_f32": [_P, _L, _L, _P, _I, _P, _P],
    "wx_pdf_energy_map_f64": [_P, _L, _L, _P, _I, _P, _P],
    "wx_pdf_energy_map_f32": [_P, _L, _L, _P, _I, _P, _P],
    "wx_signature_weights_f64": [_P, _L, _L, _P, _I, _P, _P],
    "wx_signature_weights_f32": [_P, _L, _L, _P, _I, _P, _P],
    "wx_emd_measure_weighted_f64": [_P, _P, _L, _L, _P, _I, _P, _P],
    "wx_emd_measure_weighted_f32": [_P, _P, _L, _L, _P, _I, _P, _P],
    "wx_noisest_f64": [_P, _L, _L, _L, _L, _L, _P, _P],
    "wx_noisest_f32": [_P, _L, _L, _L, _L, _L, _P, _P],
    "wx_threshold_f64": [_P, _P, _L, _L, _L, _I, _P, _L, _L, _P, _P],
    "wx_threshold_f32": [_P, _P, _L, _L, _L, _I, _P, _L, _L, _P, _P],
    "wx_dwt3d_f64": [_P, _P, _L, _L, _L, _I, _L, _P, _I, _P],
    "wx_dwt3d_f32": [_P, _P, _L, _L, _L, _I, _L, _P, _I, _P],
    "wx_idwt3d_f64": [_P, _P, _L, _L, _L, _I, _L, _P, _I, _P],
    "wx_idwt3d_f32": [_P, _P, _L, _L, _L, _I, _L, _P, _I, _P],
    "wx_denoiseall_dwt_f64": [_P, _P, _L, _I, _L, _P, _I, _I, ctypes.c_double, _I, _P, _P],
    "wx_denoiseall_dwt_f32": [_P, _P, _L, _I, _L, _P, _I, _I, ctypes.c_double, _I, _P, _P],
    "wx_denoiseall_sig_f64": [_P, _P, _L, _I, _L, _P, _I, _I, ctypes.c_double, _I, _P, _P],
    "wx_denoiseall_sig_f32": [_P, _P, _L, _I, _L, _P, _I, _I, ctypes.c_double, _I, _P, _P],
    "wx_iwpt1d_thresh_f64": [_P, _P, _L, _I, _P, _L, _L, _P, _I, _I, _P, _L, _L, ctypes.c_double, _P],
    "wx_iwpt1d_thresh_f32": [_P, _P, _L, _I, _P, _L, _L, _P, _I, _I, _P, _L, _L, ctypes.c_double, _P],
    "wx_surethreshold_f64": [_P, _L, _L, _L, _P, _P, _P],
    "wx_surethreshold_f32": [_P, _L, _L, _L, _P, _P, _P],
    "wx_relerrorthreshold_f64": [_P, _L, _L, _L, _P, _I, _P, _P],
    "wx_relerrorthreshold_f32": [_P, _L, _L, _L, _P, _I, _P, _P],
    "wx_surethreshold_trees_f64": [_P, _L, _L, _P, _L, _L, _P, _P],
    "wx_surethreshold_trees_f32": [_P, _L, _L, _P, _L, _L, _P, _P],
    "wx_relerrorthreshold_trees_f64": [_P, _L, _L, _P, _L, _L, _I, _P, _P],
    "wx_relerrorthreshold_trees_f32": [_P, _L, _L, _P, _L, _L, _I, _P, _P],
    "wx_bb_costs_f64": [_P, _P, _L, _L, _L, _I, _I, _P],
    "wx_bb_costs_f32": [_P, _P, _L, _L, _L, _I, _I, _P],
    "wx_bb_costs2d_f64": [_P, _P, _L, _L, _L, _L, _I, _I, _P],
    "wx_bb_costs2d_f32": [_P, _P, _L, _L, _L, _L, _I, _I, _P],
    "wx_lsdb_entropy_f64": [_P, _L, _L, _P, _P],
    "wx_lsdb_entropy_f32": [_P, _L, _L, _P, _P],
    "wx_lsdb_costs_f64": [_P, _L, _L, _L, _I, _P, _P],
    "wx_lsdb_costs_f32": [_P, _L, _L, _L, _I, _P, _P],
    "wx_lsdb_costs2d_f64": [_P, _L, _L, _L, _L, _I, _P, _P],
    "wx_lsdb_costs2d_f32": [_P, _L, _L, _L, _L, _I, _P, _P],
    "wx_treeselect_batch_f64": [_P, _L, _L, _L, _I, _L, _P, _P],
    "wx_treeselect_batch_f32": [_P, _L, _L, _L, _I, _L, _P, _P],
    "wx_wpd_bbtrees_f64": [_P, _L, _L, _L, _P, _I, _I, _P, _P, _P],
    "wx_wpd_bbtrees_f32": [_P, _L, _L, _L, _P, _I, _I, _P, _P, _P],
    "wx_wpd_bb_last_route": [],
    "wx_swpd_bbtrees_f64": [_P, _L, _L, _L, _P, _I, _I, _P, _P, _P],
    "wx_swpd_bbtrees_f32": [_P, _L, _L, _L, _P, _I, _I, _P, _P, _P],
    "wx_acwpd_bbtrees_f64": [_P, _L, _L, _L, _P, _I, _I, _P, _P, _P],
    "wx_red_bb_last_route": [],
    "wx_denoise_swpd1d_sig_trees_f64": [_P, _P, _L, _L, _P, _L, _L, _P, _I, _I, ctypes.c_double, _P, _L, _I, _P, _P],
    "wx_denoise_swpd1d_sig_trees_f32": [_P, _P, _L, _L, _P, _L, _L, _P, _I, _I, ctypes.c_double, _P, _L, _I, _P, _P],
    "wx_denoise_acwpd1d_sig_trees_f64": [_P, _P, _L, _L, _P, _L, _L, _P, _I, _I, ctypes.c_double, _P, _L, _I, _P, _P],
    "wx_wavemult_plan_info": [_P, _P],
    "wx_wavemult_plan_destroy": [_P],
    "wx_comm_unique_id": [_P],
    "wx_comm_init": [_I, _I, _P, ctypes.POINTER(ctypes.c_void_p)],
    "wx_comm_destroy": [_P],
    "wx_allgather_out_f64": [_P, _P, _L, _P, _P],
    "wx_allgather_out_f32": [_P, _P, _L, _P, _P],
    "wx_allgatherv_out_f64": [_P, _P, _P, _I, _P, _P],
    "wx_allgatherv_out_f32": [_P, _P, _P, _I, _P, _P],
    "wx_allreduce_moments_f64": [_P, _L, _P, _P],
    "wx_allreduce_moments_f32": [_P, _L, _P, _P],
}


def check(rc):
    if rc == WX_OK:
        return
    msg = lib().wx_last_error().decode("utf-8", "replace")
    if rc == WX_EASSERT:
        raise AssertionError(msg)
    if rc == WX_EARG:
        from .filters import ArgumentError
        raise ArgumentError(msg)
    if rc == WX_EBOUNDS:
        raise IndexError(msg)
    raise WxError(rc, msg)


def device_count():
    return lib().wx_device_count()


def build_info():
    """what the loaded binary was built from (source digest, commit, compiler, flags): wx_build_info"""
    return lib().wx_build_info().decode("utf-8", "replace")


def shutdown():
    """release the library's cached device scratch (wx_shutdown)"""
    check(lib().wx_shutdown())


def set_host_hugepages(on):
    """MADV_HUGEPAGE advice on host result arrays of 64 MiB and more (on by default; the advice persists on the caller's address range:
    include/waveletsext_hip.h); returns the previous setting (wx_set_host_hugepages)"""
    return bool(lib().wx_set_host_hugepages(1 if on else 0))


def set_force_generic(on):
    lib().wx_debug_set_dispatch(on if on in (2, 3) else (1 if on else 0))


def lattice_fold_matrix(qmf, nf, inverse=True):
    """csrc/wx_debug.h: the (nf, nf) node matrix that folds the deepest log2(nf) levels of the full-depth lattice transform, or
    None when this filter does not fold"""
    import numpy as np
    q = np.ascontiguousarray(qmf, dtype=np.float64)
    m = np.zeros((nf, nf), dtype=np.float64)
    f = lib().wx_debug_lattice_fold
    f.argtypes = [_P, _I, _I, _I, _P]
    f.restype = _I
    got = f(q.ctypes.data, int(q.size), int(nf), 1 if inverse else 0, m.ctypes.data)
    return m if got == nf else None


LatticeFactor = collections.namedtuple("LatticeFactor", "p kap g0 g2")


def lattice_factor(qmf, L, inverse=False, elem_size=8):
    """csrc/wx_debug.h: the launchers' own lattice factorisation of the QMF for a transform of L levels -- the shears p[j], kap[j]
    (F / 2 of them) and the gains g0 = g^(+-L), g2 = g^(-+2) -- or None when it declines (the direct-form kernels run).
    elem_size 8: kernels with Float64 registers; 4: kernels that compute in Float32 and normalise once after L levels, which
    also decline a gain g^(L + 1) below 2^-50 and shears too ill-conditioned for L levels of Float32 (the
    tree-driven Float32 kernels normalise every level and apply the range rule of one level)."""
    import numpy as np
    q = np.ascontiguousarray(qmf, dtype=np.float64)
    p = np.zeros(10, dtype=np.float64)
    kap = np.zeros(10, dtype=np.float64)
    g0, g2 = ctypes.c_double(0.0), ctypes.c_double(0.0)
    f = lib().wx_debug_lattice_factor
    f.argtypes = [_P, _I, _I, _I, _I, _P, _P, _P, _P]
    f.restype = _I
    ok = f(q.ctypes.data, int(q.size), int(L), 1 if inverse else 0, int(elem_size), p.ctypes.data, kap.ctypes.data,
           ctypes.addressof(g0), ctypes.addressof(g2))
    if not ok:
        return None
    ns = q.size // 2
    return LatticeFactor(p[:ns].copy(), kap[:ns].copy(), g0.value, g2.value)


RED2D_ROUTES = {1: "F1", 2: "F2", 3: "F3", 4: "I1", 5: "I2", 6: "I3", 7: "I4"}


def red2d_route(inverse, m, n, L, elem_size, F, ac=False, shift=False):
    """(route, R) that the 2-D redundant transforms take under the current dispatch mode (csrc/wx_debug.h:
    wx_debug_red2d_route): forward, the route of a whole call of L levels; inverse, the route of the level of depth L - 1.
    R is the strip height of that level for F1 / F2 / I1 and 0 otherwise."""
    code = lib().wx_debug_red2d_route(int(bool(inverse)), m, n, L, elem_size, F, int(bool(ac)), int(bool(shift)))
    if code < 0:
        raise ValueError("wx_debug_red2d_route: arguments outside the transforms' domain")
    return RED2D_ROUTES[code & 255], code >> 8


# include/waveletsext_hip.h: wx_wpt_trees_last_route
WPT_TREES_ROUTES = {0: "none", 1: "host trees", 2: "device prep + lds kernel", 3: "device prep + single tree",
                    4: "device trees copied to host", 5: "device prep + gather"}


def wpt_trees_route():
    """which way the last wptall / iwptall / iwpdall / getbasiscoefall / denoiseall / iswpdall / iacwpdall call with one tree per signal went on this thread
    (wx_wpt_trees_last_route): one of WPT_TREES_ROUTES' strings; "none" before the first such call and after one that raised"""
    return WPT_TREES_ROUTES[lib().wx_wpt_trees_last_route()]


def wpd_bb_route():
    """which way the last wpd_bestbasistreeall / bestbasiscoefall call went on this thread (wx_wpd_bb_last_route,
    include/waveletsext_hip.h): 0 = none yet, or that call raised; 1 = the fused kernel; 2 = chunks of signals through the table
    kernels; 3 = nothing to transform (L = 0, no signals)"""
    return int(lib().wx_wpd_bb_last_route())


def red_bb_route():
    """which way the last swpd_bestbasistreeall / acwpd_bestbasistreeall / swpd_denoiseall / acwpd_denoiseall / red_noisestall call went on this thread (wx_red_bb_last_route,
    include/waveletsext_hip.h): 0 = none yet, or that call raised; 1 = the fused kernel; 2 = chunks of signals through the table
    kernels; 3 = nothing to transform (L = 0, no signals)"""
    return int(lib().wx_red_bb_last_route())


def red_bb_grid(n, L, F, elem_size, ac, which, batch):
    """csrc/wx_debug.h: the workgroups the kernel of wx_swpd_bbtrees_* / wx_acwpd_bbtrees_f64 (which = 0) or of
    wx_denoise_swpd1d_sig_trees_* / wx_denoise_acwpd1d_sig_trees_f64 (which = 1) is launched with for this shape, by the functions the
    launch calls; 0 outside the kernel's window.  Needs no device."""
    f = lib().wx_debug_red_bb_grid
    f.argtypes = [_L, _I, _I, _I, _I, _I, _L]
    f.restype = _I
    return int(f(int(n), int(L), int(F), int(elem_size), int(bool(ac)), int(which), int(batch)))


def wpd_bb_grid(n, L, F, elem_size, batch):
    """csrc/wx_debug.h: the workgroups the fused kernel of wx_wpd_bbtrees_* is launched with for this shape, by the function the
    launch calls; 0 outside the kernel's window.  Needs no device."""
    f = lib().wx_debug_wpd_bb_grid
    f.argtypes = [_L, _I, _I, _I, _L]
    f.restype = _I
    return int(f(int(n), int(L), int(F), int(elem_size), int(batch)))


# csrc/wx_debug.h: route ids of the 1-D redundant transforms' launch record
SWT1D_ROUTES = {1: "FG", 2: "FSD", 3: "FSDIP", 4: "FTWO", 5: "FLVL", 6: "FM", 7: "FMRC", 8: "FHAAR6", 9: "FDEEP",
                10: "ISD", 11: "ISDIP", 12: "IM", 13: "IHAAR6", 14: "IDEEP", 15: "ITILE", 16: "ILVL",
                17: "IACDWT", 18: "IACWPT", 19: "IACWPD"}
SWT1D_TRACE_MAX = 1 << 18
Swt1dLaunch = collections.namedtuple("Swt1dLaunch", "route depth K R OPT elem_size block grid_x grid_y grid_z lds")


class Swt1dTrace(list):
    """the list `swt1d_trace` yields; `dropped` = launches past SWT1D_TRACE_MAX, which the record does not hold"""
    dropped = 0


@contextlib.contextmanager
def swt1d_trace():
    """Record every kernel launch of the 1-D redundant transforms made inside the block (csrc/wx_debug.h:
    wx_debug_swt1d_trace_begin / _end; process-global, so one block at a time).  Yields a list that holds one Swt1dLaunch per
    launch, in launch order, once the block has ended."""
    import numpy as np
    L = lib()
    out = Swt1dTrace()
    L.wx_debug_swt1d_trace_begin()
    try:
        yield out
    finally:
        buf = np.empty((SWT1D_TRACE_MAX, len(Swt1dLaunch._fields)), dtype=np.int32)
        got = L.wx_debug_swt1d_trace_end(buf.ctypes.data, SWT1D_TRACE_MAX)
        check(min(got, 0))
        out.dropped = int(L.wx_debug_swt1d_trace_dropped())
        for row in buf[:got].tolist():
            out.append(Swt1dLaunch(SWT1D_ROUTES[row[0]], *row[1:]))


# csrc/wx_debug.h: route ids of the 2-D decimated transforms' launch record
DWT2D_ROUTES = {1: "Q64W", 2: "Q64TPREP", 3: "Q64T", 4: "Q64", 5: "PYR", 6: "TAIL", 7: "L2DF", 8: "L2DC", 9: "COL1D", 10: "LROWS",
                11: "ROWS", 12: "TILE", 13: "TILEP", 14: "ITILE", 15: "ITILEP", 16: "TWO", 17: "COPYB", 18: "GATHER"}
DWT2D_TRACE_MAX = 1 << 16
Dwt2dLaunch = collections.namedtuple("Dwt2dLaunch", "route inverse depth K elem_size block grid_x grid_y grid_z lds e0 e1 e2 e3 e4 e5")


class Dwt2dTrace(list):
    """the list `dwt2d_trace` yields; `dropped` = launches past DWT2D_TRACE_MAX, which the record does not hold"""
    dropped = 0


@contextlib.contextmanager
def dwt2d_trace():
    """Record every kernel launch of the 2-D decimated transforms (wpd, wpt, iwpt, iwpd, dwt / idwt of images) made inside the
    block (csrc/wx_debug.h: wx_debug_dwt2d_trace_begin / _end; process-global, so one block at a time).  Yields a list that
    holds one Dwt2dLaunch per launch, in launch order, once the block has ended; what e0 .. e5 hold for each route is
    tabulated in wx_debug.h."""
    import numpy as np
    L = lib()
    out = Dwt2dTrace()
    L.wx_debug_dwt2d_trace_begin()
    try:
        yield out
    finally:
        buf = np.empty((DWT2D_TRACE_MAX, len(Dwt2dLaunch._fields)), dtype=np.int32)
        got = L.wx_debug_dwt2d_trace_end(buf.ctypes.data, DWT2D_TRACE_MAX)
        check(min(got, 0))
        out.dropped = int(L.wx_debug_dwt2d_trace_dropped())
        for row in buf[:got].tolist():
            out.append(Dwt2dLaunch(DWT2D_ROUTES[row[0]], *row[1:]))


# csrc/wx_debug.h: route ids of the 1-D decimated transforms' launch record
DWT1D_ROUTES = {1: "LATF64", 2: "LATWPD", 3: "LATF32", 4: "LATTREE", 5: "LAT8KT", 6: "LANETREE", 7: "SMALLTREE", 8: "HAAR", 9: "TOP",
                10: "TOPWPD", 11: "FUSED", 12: "L1TILE", 13: "LEVEL", 14: "GATHER", 15: "TAIL", 16: "ITAIL", 17: "THRFUSED", 18: "THRCOPY"}
DWT1D_TRACE_MAX = 1 << 16
Dwt1dLaunch = collections.namedtuple("Dwt1dLaunch", "route inverse elem_size n depth K signals F e0 e1 e2 e3 e4 block grid lds")


class Dwt1dTrace(list):
    """the list `dwt1d_trace` yields; `dropped` = launches past DWT1D_TRACE_MAX, which the record does not hold"""
    dropped = 0


@contextlib.contextmanager
def dwt1d_trace():
    """Record every kernel launch of the 1-D decimated transforms (wpd, wpt, iwpt, iwpd, dwt / idwt of signals, the thresholded
    inverse behind denoise) made inside the block (csrc/wx_debug.h: wx_debug_dwt1d_trace_begin / _end; process-global, so one
    block at a time).  Yields a list that holds one Dwt1dLaunch per launch, in launch order, once the block has ended; what
    e0 .. e4 hold for each route is tabulated in wx_debug.h."""
    import numpy as np
    L = lib()
    out = Dwt1dTrace()
    L.wx_debug_dwt1d_trace_begin()
    try:
        yield out
    finally:
        buf = np.empty((DWT1D_TRACE_MAX, len(Dwt1dLaunch._fields)), dtype=np.int32)
        got = L.wx_debug_dwt1d_trace_end(buf.ctypes.data, DWT1D_TRACE_MAX)
        check(min(got, 0))
        out.dropped = int(L.wx_debug_dwt1d_trace_dropped())
        for row in buf[:got].tolist():
            out.append(Dwt1dLaunch(DWT1D_ROUTES[row[0]], *row[1:]))


def swt_inv_plan(layout, L, F, n, elem_size, sm=None, has_tree=False, haar6=False):
    """[(from, to, R, OPT)] of every pass of the 1-D redundant inverse under the current dispatch mode (csrc/wx_debug.h:
    wx_debug_swt_inv_plan, which runs the launcher's own wx_swt_inv_plan; needs no device).  layout "dwt" / "wpt" / "wpd"."""
    import numpy as np
    out = np.zeros((max(int(L), 1), 4), dtype=np.int32)
    code = {"dwt": 0, "wpt": 1, "wpd": 2}.get(layout, layout)
    got = lib().wx_debug_swt_inv_plan(int(code), int(L), int(F), -1 if sm is None else int(sm), int(n), int(elem_size),
                                      int(bool(has_tree)), int(bool(haar6)), out.ctypes.data)
    check(min(got, 0))
    return [tuple(r) for r in out[:got].tolist()]


def ldb_chunks(nk, N, nc):
    """chunks per class of the LDB class reductions (energy map, class means / variances) over nk coefficients of N signals in nc
    classes (csrc/wx_debug.h: wx_debug_ldb_chunks, which runs the function the launch code calls; needs no device)"""
    got = lib().wx_debug_ldb_chunks(int(nk), int(N), int(nc))
    check(min(got, 0))
    return got
