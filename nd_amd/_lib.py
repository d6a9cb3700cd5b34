"""
nd_amd/_lib.py -- ctypes binding of libnd_amd.so (include/nd_amd.h).

The HIP library is the only compute path of this package.  If it is missing the
import of any op raises; there is no CPU or PyTorch fallback.
"""
import ctypes as C
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
# ND_AMD_LIB points the loader at an alternative build of the same library (tuning experiments)
LIB_PATH = os.environ.get('ND_AMD_LIB') or os.path.join(_HERE, 'libnd_amd.so')

F32, F64 = 0, 1
I64 = 2                 # values of nd_amd_rasterize_polygons
U8, I32 = 3, 4          # with F32, F64 and I64: the map types of the region entries
OK, EINVAL, EWORKSPACE, EHIP, ENOSOLUTION, EUNSUPPORTED = 0, -1, -2, -3, -4, -5
EINTERNAL = -6
MODES = {'reflect': 0, 'constant': 1, 'nearest': 2, 'mirror': 3, 'wrap': 4,
         'grid-constant': 1, 'grid-mirror': 0, 'grid-wrap': 4}
KERNEL_NAMES = {1: 'omnibus_c2_global', 2: 'omnibus_c2_search', 3: 'correlate',
                4: 'nlmeans', 5: 'boxcar_tiled', 6: 'nlmeans_tiled', 7: 'correlate1d',
                8: 'relayout', 9: 'omnibus_c2_dense', 10: 'omnibus_c2_fused', 11: 'omnibus_c2_sample', 12: 'omnibus_c2_exact',
                13: 'coregister_shifts', 14: 'warp_translate', 15: 'rgb_limits', 16: 'rgb_compose',
                17: 'classify_forest', 18: 'classify_kmeans', 19: 'classify_gather', 20: 'class_mean',
                21: 'classify_knn', 22: 'classify_linear', 23: 'kmeans_step', 24: 'feature_moments',
                25: 'gather_rows', 26: 'change_segments', 27: 'rasterize', 28: 'resample', 29: 'speckle', 30: 'regions',
                31: 'zonal', 32: 'temporal'}
LAYOUT_PLANAR, LAYOUT_PIXEL_MAJOR = 0, 1
STRUCT_DIAG, STRUCT_C2, STRUCT_C3 = 0, 1, 2

# every symbol include/nd_amd.h declares
SYMBOLS = ('nd_amd_abi_version', 'nd_amd_last_error',
           'nd_amd_omnibus_c2_workspace_bytes', 'nd_amd_omnibus_c2_uses_wave_search', 'nd_amd_omnibus_c2',
           'nd_amd_omnibus_c2_pixel_major',
           'nd_amd_omnibus_c2_ml_workspace_bytes', 'nd_amd_omnibus_c2_ml',
           'nd_amd_omnibus_c3_workspace_bytes', 'nd_amd_omnibus_c3', 'nd_amd_omnibus_c3_pixel_major',
           'nd_amd_omnibus_diag_workspace_bytes', 'nd_amd_omnibus_diag', 'nd_amd_change_segments',
           'nd_amd_correlate', 'nd_amd_correlate1d', 'nd_amd_correlate1d_yx', 'nd_amd_nlmeans3d',
           'nd_amd_relayout_planar', 'nd_amd_relayout_planar_complex',
           'nd_amd_relayout_pixel_major', 'nd_amd_split_complex', 'nd_amd_merge_complex',
           'nd_amd_timing_enable', 'nd_amd_timing_collect', 'nd_amd_timing_dropped',
           'nd_amd_timing_select',
           'nd_amd_coregister_shifts_workspace_bytes', 'nd_amd_coregister_shifts',
           'nd_amd_warp_translate_workspace_bytes', 'nd_amd_warp_translate',
           'nd_amd_rgb_limits_workspace_bytes', 'nd_amd_rgb_limits', 'nd_amd_rgb_compose',
           'nd_amd_classify_workspace_bytes', 'nd_amd_classify_forest', 'nd_amd_classify_kmeans',
           'nd_amd_classify_select', 'nd_amd_classify_gather', 'nd_amd_class_stats', 'nd_amd_class_fill',
           'nd_amd_classify_knn', 'nd_amd_classify_linear',
           'nd_amd_kmeans_fit_workspace_bytes', 'nd_amd_kmeans_step', 'nd_amd_feature_moments',
           'nd_amd_gather_rows',
           'nd_amd_rasterize_workspace_bytes', 'nd_amd_rasterize_polygons',
           'nd_amd_resample', 'nd_amd_resample_nearest', 'nd_amd_resample_check_table',
           'nd_amd_speckle_lee', 'nd_amd_speckle_multitemporal_workspace_bytes', 'nd_amd_speckle_multitemporal',
           'nd_amd_regions_workspace_bytes', 'nd_amd_label_regions', 'nd_amd_region_sizes', 'nd_amd_sieve_regions',
           'nd_amd_zonal_keys', 'nd_amd_zonal_workspace_bytes', 'nd_amd_zonal_stats', 'nd_amd_zonal_paint',
           'nd_amd_temporal_stats')
CLASSIFY_BLOCK_ROWS, CLASSIFY_MAX_FEATURES = 1024, 1024
CLASSIFY_KNN_MAX_K, CLASSIFY_KNN_MAX_FEATURES, CLASSIFY_KNN_TILE = 32, 128, 8
KMEANS_FIT_MAX_ACC = 4096
RASTERIZE_MAX_CROSSINGS = 256
RESAMPLE_MAX_TAPS = 256
SPECKLE_METHODS = {'lee': 0, 'kuan': 1}
# include/nd_amd.h: ND_AMD_SPECKLE_MAX_W, _MAX_VARIABLES, _HOT_MAX_PLANES, _TILE_Y, _TILE_X, _HOT_TILE_Y
SPECKLE_MAX_W, SPECKLE_MAX_VARIABLES, SPECKLE_HOT_MAX_PLANES = 31, 4, 32
SPECKLE_TILE_Y, SPECKLE_TILE_X, SPECKLE_HOT_TILE_Y = 32, 64, 8
# include/nd_amd.h: ND_AMD_TEMPORAL_REG_MAX_*, _LDS_MAX_*; the forms that nd_amd_temporal_stats_in_form names, an
# entry of temporal.hip for the tests that is in no header (kernels.temporal_stats binds it where `_form` is used)
TEMPORAL_REG_MAX = {F32: 64, F64: 64}
TEMPORAL_LDS_MAX = {F32: 256, F64: 128}
TEMPORAL_FORMS = {'register': 1, 'lds': 2, 'stream': 3}
LINKS = {'none': 0, 'softmax': 1, 'ovr': 2}
LINEAR_OUTPUTS = {'predict': 0, 'decision_function': 1, 'predict_proba': 2}

_lib = None


class NdAmdError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__('libnd_amd error %d: %s' % (code, msg))
        self.code = code


def lib():
    """Load libnd_amd.so (built by `python -m nd_amd.build`)."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise ImportError(
            'nd_amd: %s is missing -- build it with `python -m nd_amd.build` '
            '(hipcc, gfx950).  There is no fallback path.' % LIB_PATH)
    L = C.CDLL(LIB_PATH)
    i64, dbl, vp, i32 = C.c_int64, C.c_double, C.c_void_p, C.c_int
    L.nd_amd_abi_version.restype = i32
    L.nd_amd_abi_version.argtypes = []
    L.nd_amd_last_error.restype = C.c_char_p
    L.nd_amd_last_error.argtypes = []
    L.nd_amd_omnibus_c2_workspace_bytes.restype = C.c_size_t
    L.nd_amd_omnibus_c2_workspace_bytes.argtypes = [i32, i64, i64, i64,
                                                    C.POINTER(C.c_size_t)]
    L.nd_amd_omnibus_c2_uses_wave_search.restype = i32
    L.nd_amd_omnibus_c2_uses_wave_search.argtypes = [i32, i64, i64, dbl, C.c_uint32, i32]
    L.nd_amd_omnibus_c2.restype = i32
    L.nd_amd_omnibus_c2.argtypes = ([vp] * 4 + [i32] + [i64] * 6 + [C.c_uint32, dbl]
                                    + [vp, vp, vp, vp, C.c_size_t, vp])
    L.nd_amd_omnibus_c2_ml_workspace_bytes.restype = C.c_size_t
    L.nd_amd_omnibus_c2_ml_workspace_bytes.argtypes = [i32, i64, i64, i64, i32]
    L.nd_amd_omnibus_c2_ml.restype = i32
    L.nd_amd_omnibus_c2_ml.argtypes = ([vp] * 4 + [i32] + [i64] * 6 + [i32, dbl]
                                       + [vp, vp, vp, vp, C.c_size_t, vp])
    L.nd_amd_omnibus_c2_pixel_major.restype = i32
    L.nd_amd_omnibus_c2_pixel_major.argtypes = ([vp] * 4 + [i32] + [i64] * 3 + [C.POINTER(i64)]
                                                + [C.c_uint32, dbl] + [vp, vp, vp, vp, C.c_size_t, vp])
    L.nd_amd_omnibus_c3_workspace_bytes.restype = C.c_size_t
    L.nd_amd_omnibus_c3_workspace_bytes.argtypes = [i64, i64, i64]
    L.nd_amd_omnibus_c3.restype = i32
    L.nd_amd_omnibus_c3.argtypes = ([C.POINTER(vp), i32] + [i64] * 6 + [C.c_uint32, dbl]
                                    + [vp, vp, vp, vp, C.c_size_t, vp])
    L.nd_amd_omnibus_c3_pixel_major.restype = i32
    L.nd_amd_omnibus_c3_pixel_major.argtypes = ([C.POINTER(vp), i32] + [i64] * 3 + [C.POINTER(i64)]
                                                + [C.c_uint32, dbl] + [vp, vp, vp, vp, C.c_size_t, vp])
    L.nd_amd_omnibus_diag_workspace_bytes.restype = C.c_size_t
    L.nd_amd_omnibus_diag_workspace_bytes.argtypes = [i32, i32, i64, i64, i64]
    L.nd_amd_omnibus_diag.restype = i32
    L.nd_amd_omnibus_diag.argtypes = ([C.POINTER(vp), i32, i32] + [i64] * 6 + [dbl, dbl]
                                      + [vp, vp, vp, vp, C.c_size_t, vp])
    L.nd_amd_change_segments.restype = i32
    L.nd_amd_change_segments.argtypes = ([C.POINTER(vp), i32, i32, i32] + [i64] * 6
                                         + [vp, vp, C.POINTER(vp), vp])
    L.nd_amd_correlate.restype = i32
    L.nd_amd_correlate.argtypes = [vp, vp, i32, C.POINTER(i64), C.POINTER(i64),
                                   C.POINTER(i64), i64, C.POINTER(i64),
                                   C.POINTER(dbl), i32, dbl, vp, C.c_size_t, vp]
    L.nd_amd_correlate1d.restype = i32
    L.nd_amd_correlate1d.argtypes = [vp, vp, i32, C.POINTER(i64), C.POINTER(i64), C.POINTER(i64),
                                     i32, i32, C.POINTER(dbl), i32, dbl, vp]
    L.nd_amd_merge_complex.restype = i32
    L.nd_amd_merge_complex.argtypes = [vp, vp, vp, i32, i64, vp]
    L.nd_amd_split_complex.restype = i32
    L.nd_amd_split_complex.argtypes = [vp, vp, vp, i32, i64, vp]
    L.nd_amd_correlate1d_yx.restype = i32
    L.nd_amd_correlate1d_yx.argtypes = [vp, vp, i32, C.POINTER(i64), C.POINTER(i64), C.POINTER(i64),
                                        i32, C.POINTER(dbl), C.POINTER(dbl), i32, vp]
    L.nd_amd_nlmeans3d.restype = i32
    L.nd_amd_nlmeans3d.argtypes = [vp, vp, i32, C.POINTER(i64), i64, C.POINTER(i64),
                                   C.POINTER(i64), C.POINTER(C.c_uint32),
                                   C.POINTER(C.c_uint32), dbl, dbl, dbl, i32, i32, vp,
                                   C.POINTER(i64), C.POINTER(i64), C.POINTER(i64),
                                   C.POINTER(i64), vp]
    L.nd_amd_relayout_planar.restype = i32
    L.nd_amd_relayout_planar.argtypes = [vp, vp, i32, i64, i64, i64, i64, vp]
    L.nd_amd_relayout_planar_complex.restype = i32
    L.nd_amd_relayout_planar_complex.argtypes = [vp, vp, vp, i32, i64, i64, i64, vp]
    L.nd_amd_relayout_pixel_major.restype = i32
    L.nd_amd_relayout_pixel_major.argtypes = [vp, vp, i32, i64, i64, i64, i64, vp]
    L.nd_amd_timing_enable.restype = i32
    L.nd_amd_timing_enable.argtypes = [i32]
    L.nd_amd_timing_collect.restype = i32
    L.nd_amd_timing_collect.argtypes = [C.POINTER(C.c_int32), C.POINTER(C.c_float), i32,
                                        C.POINTER(i32)]
    L.nd_amd_timing_dropped.restype = i32
    L.nd_amd_timing_dropped.argtypes = []
    L.nd_amd_timing_select.restype = i32
    L.nd_amd_timing_select.argtypes = [C.c_uint64]
    L.nd_amd_coregister_shifts_workspace_bytes.restype = C.c_size_t
    L.nd_amd_coregister_shifts_workspace_bytes.argtypes = [i32, i64, i64, i64, i32]
    L.nd_amd_coregister_shifts.restype = i32
    L.nd_amd_coregister_shifts.argtypes = [vp, i32] + [i64] * 7 + [i32, vp, vp, vp, C.c_size_t, vp]
    L.nd_amd_warp_translate_workspace_bytes.restype = C.c_size_t
    L.nd_amd_warp_translate_workspace_bytes.argtypes = [i32, i32, i64, i64, i64, i32]
    L.nd_amd_warp_translate.restype = i32
    L.nd_amd_warp_translate.argtypes = ([C.POINTER(vp), C.POINTER(vp), i32, i32] + [i64] * 3
                                        + [i32, vp, i64, vp, C.c_size_t, vp])
    L.nd_amd_rgb_limits_workspace_bytes.restype = C.c_size_t
    L.nd_amd_rgb_limits_workspace_bytes.argtypes = [i32, i64]
    L.nd_amd_rgb_limits.restype = i32
    L.nd_amd_rgb_limits.argtypes = ([C.POINTER(vp), C.POINTER(vp), i32, i32] + [i64] * 6 + [dbl, dbl]
                                    + [vp, vp, vp, C.c_size_t, vp])
    L.nd_amd_rgb_compose.restype = i32
    L.nd_amd_rgb_compose.argtypes = ([C.POINTER(vp), C.POINTER(vp), i32, i32] + [i64] * 6
                                     + [vp, C.POINTER(dbl), C.POINTER(dbl), vp, vp, vp])
    pi64 = C.POINTER(i64)
    L.nd_amd_classify_workspace_bytes.restype = C.c_size_t
    L.nd_amd_classify_workspace_bytes.argtypes = [i32]
    table = [C.POINTER(vp), i32, i32, pi64, pi64]
    L.nd_amd_classify_forest.restype = i32
    L.nd_amd_classify_forest.argtypes = table + [vp, i64, vp, vp, i32, vp, i32, vp, vp, vp, vp, vp, C.c_size_t, vp]
    L.nd_amd_classify_kmeans.restype = i32
    L.nd_amd_classify_kmeans.argtypes = table + [vp, i32, vp, vp, vp, vp, C.c_size_t, vp]
    L.nd_amd_classify_knn.restype = i32
    L.nd_amd_classify_knn.argtypes = table + [vp, vp, i32, i32, vp, i32, vp, vp, vp, vp, vp, C.c_size_t, vp]
    L.nd_amd_classify_linear.restype = i32
    L.nd_amd_classify_linear.argtypes = table + [vp, vp, i32, vp, i32, i32, vp, vp, vp, vp, C.c_size_t, vp]
    L.nd_amd_classify_select.restype = i32
    L.nd_amd_classify_select.argtypes = table + [vp, pi64, vp, vp, vp, vp, C.c_size_t, vp]
    L.nd_amd_classify_gather.restype = i32
    L.nd_amd_classify_gather.argtypes = table + [vp, pi64, vp, vp, vp, vp, vp, C.c_size_t, vp]
    L.nd_amd_class_stats.restype = i32
    L.nd_amd_class_stats.argtypes = [vp, i32, pi64, pi64, vp, pi64, i32, vp, vp, vp, vp]
    L.nd_amd_class_fill.restype = i32
    L.nd_amd_class_fill.argtypes = [vp, vp, i32, pi64, pi64, vp, pi64, i32, vp, vp]
    L.nd_amd_kmeans_fit_workspace_bytes.restype = C.c_size_t
    L.nd_amd_kmeans_fit_workspace_bytes.argtypes = [i32, i32, i64]
    L.nd_amd_kmeans_step.restype = i32
    L.nd_amd_kmeans_step.argtypes = table + [vp, i32, vp, vp, vp, vp, vp, vp, vp, vp, C.c_size_t, vp]
    L.nd_amd_feature_moments.restype = i32
    L.nd_amd_feature_moments.argtypes = table + [vp, vp, vp, vp, vp, vp, C.c_size_t, vp]
    L.nd_amd_gather_rows.restype = i32
    L.nd_amd_gather_rows.argtypes = table + [vp, i64, vp, vp, vp, vp, vp, C.c_size_t, vp]
    L.nd_amd_rasterize_workspace_bytes.restype = C.c_size_t
    L.nd_amd_rasterize_workspace_bytes.argtypes = [i64, i64, i64]
    L.nd_amd_rasterize_polygons.restype = i32
    L.nd_amd_rasterize_polygons.argtypes = ([vp] * 7 + [i32, vp] + [i64] * 4 + [vp] + [i64] * 3
                                            + [vp, C.c_size_t, vp])
    grid = [i64, i64, i64, i64, pi64, i64, i64, pi64]     # nplanes, inner, source size and strides, destination
    L.nd_amd_resample.restype = i32
    L.nd_amd_resample.argtypes = [vp, vp, i32] + grid + [vp, vp, vp, i32] * 2 + [dbl, vp]
    L.nd_amd_resample_nearest.restype = i32
    L.nd_amd_resample_nearest.argtypes = [vp, vp, i32] + grid + [vp] * 4 + [vp, vp]
    L.nd_amd_resample_check_table.restype = i32
    L.nd_amd_resample_check_table.argtypes = [vp, vp, i64, i64, i32, vp]
    L.nd_amd_speckle_lee.restype = i32
    L.nd_amd_speckle_lee.argtypes = [vp, vp, i32, i64, i64, i64, pi64, pi64, i32, dbl, i32, vp]
    L.nd_amd_speckle_multitemporal_workspace_bytes.restype = C.c_size_t
    L.nd_amd_speckle_multitemporal_workspace_bytes.argtypes = [i64, i64, i64, i32]
    L.nd_amd_speckle_multitemporal.restype = i32
    L.nd_amd_speckle_multitemporal.argtypes = [C.POINTER(vp), C.POINTER(vp), i32, i32, i64, i64, i64, pi64, pi64,
                                               i32, vp, C.c_size_t, vp]
    L.nd_amd_regions_workspace_bytes.restype = C.c_size_t
    L.nd_amd_regions_workspace_bytes.argtypes = [i64, i64, i64, i32]
    L.nd_amd_label_regions.restype = i32
    L.nd_amd_label_regions.argtypes = [vp, i32, i64, i64, i64, pi64, i32, i32, vp, vp, pi64, vp, pi64, vp,
                                       vp, C.c_size_t, vp]
    L.nd_amd_region_sizes.restype = i32
    L.nd_amd_region_sizes.argtypes = [vp, pi64, i64, i64, i64, vp, vp, i64, vp]
    L.nd_amd_sieve_regions.restype = i32
    L.nd_amd_sieve_regions.argtypes = [vp, vp, i32, i64, i64, i64, pi64, pi64, i32, i32, vp, vp, i64,
                                       vp, C.c_size_t, vp]
    L.nd_amd_zonal_keys.restype = i32
    L.nd_amd_zonal_keys.argtypes = [vp, i32, i64, i64, pi64, vp, i64, vp, vp]
    L.nd_amd_zonal_workspace_bytes.restype = C.c_size_t
    L.nd_amd_zonal_workspace_bytes.argtypes = [i64, i64, i64, i64]
    L.nd_amd_zonal_stats.restype = i32
    L.nd_amd_zonal_stats.argtypes = [vp, i32, i64, i64, i64, pi64, vp, vp, i64] + [vp] * 6 + [vp, C.c_size_t, vp]
    L.nd_amd_zonal_paint.restype = i32
    L.nd_amd_zonal_paint.argtypes = [vp, vp, i64, i64, i64, i64, vp, pi64, vp, pi64, i32, dbl, vp]
    L.nd_amd_temporal_stats.restype = i32
    L.nd_amd_temporal_stats.argtypes = [vp, i32, i64, i64, i64, pi64, i32, i32, C.POINTER(dbl), i32] + [vp] * 14 + [vp]
    v = L.nd_amd_abi_version()
    if v != 1:
        raise ImportError('nd_amd: libnd_amd.so has ABI version %d, expected 1' % v)
    _lib = L
    return L


def check(rc):
    if rc != OK:
        raise NdAmdError(rc, lib().nd_amd_last_error().decode('utf-8', 'replace'))


def i64_array(values):
    return (C.c_int64 * len(values))(*[int(v) for v in values])


def u32_array(values):
    return (C.c_uint32 * len(values))(*[int(v) for v in values])


def timing_enable(capacity):
    check(lib().nd_amd_timing_enable(int(capacity)))


def timing_select(names=None):
    """time only the kernels named (KERNEL_NAMES values); None = all.  Reset by timing_enable."""
    mask = 0
    if names:
        ids = {v: k for k, v in KERNEL_NAMES.items()}
        for n in names:
            mask |= 1 << ids[n]
    check(lib().nd_amd_timing_select(mask))


def timing_dropped():
    """launches that found the timing ring full since the last call (0 = every launch was timed)."""
    return int(lib().nd_amd_timing_dropped())


def timing_collect(max_n=65536):
    """-> list of (kernel name, milliseconds) in launch order; synchronises."""
    ids = (C.c_int32 * max_n)()
    ms = (C.c_float * max_n)()
    n = C.c_int(0)
    check(lib().nd_amd_timing_collect(ids, ms, max_n, C.byref(n)))
    return [(KERNEL_NAMES.get(ids[i], str(ids[i])), float(ms[i])) for i in range(n.value)]
