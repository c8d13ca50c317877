"""ctypes binding of libsunerf_hip.so (C ABI: include/sunerf_hip.h).

The library is built in-tree by ``csrc/build.sh`` (``__graft_entry__.build()``).  There is no CPU fallback: if
the library is missing or a tensor is not on a ROCm device the call raises.
"""
import ctypes
import os

# PyTorch-ROCm bundles its own HIP runtime (torch/lib/libamdhip64.so, SONAME libamdhip64.so.7).  It must be mapped
# BEFORE libsunerf_hip.so so that our library binds to the same runtime instance (streams and device pointers are
# shared with torch); loading ours first would pull in /opt/rocm's copy and every launch fails with
# hipErrorNoDevice (100).
import torch  # noqa: F401  (side effect: loads torch's HIP runtime)

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get('SUNERF_HIP_LIB') or os.path.join(os.path.dirname(_HERE), 'libsunerf_hip.so')

_lib = None

c_f32p = ctypes.c_void_p   # device pointers travel as raw addresses
c_void = ctypes.c_void_p


class GridFrame(ctypes.Structure):
    """``SunerfGridFrame``: origin and the three basis vectors of an affine grid, passed by value."""
    _fields_ = [('origin', ctypes.c_double * 3), ('basis', (ctypes.c_double * 3) * 3)]


_SIGNATURES = {
    'sunerf_abi_version': (ctypes.c_int, []),
    'sunerf_packed_mlp_bytes': (ctypes.c_size_t, [ctypes.c_int, ctypes.c_int]),
    'sunerf_pack_mlp': (ctypes.c_int, [ctypes.POINTER(ctypes.c_void_p), ctypes.POINTER(ctypes.c_void_p), ctypes.c_int,
                                        ctypes.c_int, ctypes.c_int, ctypes.c_int, c_void, c_void]),
    'sunerf_sample_z': (ctypes.c_int, [ctypes.c_int, c_f32p, c_f32p, c_f32p, c_f32p, ctypes.c_int64, ctypes.c_int,
                                        ctypes.c_float, ctypes.c_float, c_f32p, c_void]),
    'sunerf_act_stash_bytes': (ctypes.c_size_t, [ctypes.c_int64, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int]),
    'sunerf_render_workspace_bytes': (ctypes.c_size_t, [ctypes.c_int]),
    'sunerf_emission_render_fwd': (ctypes.c_int, [c_void, ctypes.c_int, ctypes.c_int, ctypes.c_int, c_f32p, c_f32p, c_f32p, c_f32p,
                                                   ctypes.c_int64, ctypes.c_int, c_f32p, c_f32p, c_f32p, c_f32p,
                                                   c_f32p, c_f32p, c_f32p, ctypes.c_float, c_void, ctypes.c_int, c_void, ctypes.c_size_t,
                                                   c_void]),
    'sunerf_packed_mlp_t_bytes': (ctypes.c_size_t, [ctypes.c_int, ctypes.c_int]),
    'sunerf_pack_mlp_t': (ctypes.c_int, [ctypes.POINTER(ctypes.c_void_p), ctypes.c_int, ctypes.c_int, ctypes.c_int,
                                          c_void, c_void]),
    'sunerf_dz_stash_bytes': (ctypes.c_size_t, [ctypes.c_int64, ctypes.c_int, ctypes.c_int, ctypes.c_int]),
    'sunerf_wgrad_workspace_bytes': (ctypes.c_size_t, [ctypes.c_int, ctypes.c_int, ctypes.c_int]),
    'sunerf_emission_integral_fwd': (ctypes.c_int, [c_f32p, c_f32p, c_f32p, ctypes.c_int64, ctypes.c_int, c_f32p, c_f32p, c_f32p,
                                                     c_void]),
    'sunerf_emission_integral_bwd': (ctypes.c_int, [c_f32p, c_f32p, c_f32p, c_f32p, c_f32p, c_f32p, c_f32p, c_f32p, ctypes.c_float,
                                                     ctypes.c_float, ctypes.c_int64, ctypes.c_int, c_f32p, c_void, c_void]),
    'sunerf_mlp_dgrad': (ctypes.c_int, [c_void, ctypes.c_int, ctypes.c_int, c_f32p, c_void, c_void, c_void,
                                         ctypes.c_int64, ctypes.c_int, c_void]),
    'sunerf_mlp_wgrad': (ctypes.c_int, [ctypes.c_int, ctypes.c_int, ctypes.c_int, c_void, c_void, c_void, c_f32p, c_void,
                                         ctypes.c_int64, ctypes.c_int, c_void, ctypes.c_int,
                                         ctypes.POINTER(ctypes.c_void_p), ctypes.POINTER(ctypes.c_void_p), ctypes.c_int,
                                         c_void]),
    'sunerf_bwd_pipe_workspace_bytes': (ctypes.c_size_t, [ctypes.c_int64, ctypes.c_int, ctypes.c_int, ctypes.c_int]),
    'sunerf_mlp_backward_pipe': (ctypes.c_int, [ctypes.c_int, ctypes.c_int, ctypes.c_int, c_void, c_void, c_f32p, c_void,
                                                 ctypes.c_int64, ctypes.c_int, c_void, ctypes.c_size_t,
                                                 ctypes.POINTER(ctypes.c_void_p), ctypes.POINTER(ctypes.c_void_p), ctypes.c_int,
                                                 ctypes.c_int, c_void]),
    'sunerf_bwd_pipe_kernel_time': (ctypes.c_int, [ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_int)]),
    'sunerf_mlp_backward_exact_workspace_bytes': (ctypes.c_size_t, [ctypes.c_int64, ctypes.c_int, ctypes.c_int]),
    'sunerf_mlp_backward_exact': (ctypes.c_int, [ctypes.POINTER(ctypes.c_void_p), ctypes.POINTER(ctypes.c_void_p), ctypes.c_int,
                                                  ctypes.c_int, ctypes.c_int, c_f32p, c_f32p, c_f32p, c_f32p, c_f32p,
                                                  ctypes.c_int64, ctypes.c_int, c_f32p, c_void, ctypes.c_size_t,
                                                  ctypes.POINTER(ctypes.c_void_p), ctypes.POINTER(ctypes.c_void_p), ctypes.c_int,
                                                  c_void]),
    'sunerf_mlp_backward_exact_chunked_workspace_bytes': (ctypes.c_size_t, [ctypes.c_int, ctypes.c_int]),
    'sunerf_mlp_backward_exact_chunked': (ctypes.c_int, [ctypes.POINTER(ctypes.c_void_p), ctypes.POINTER(ctypes.c_void_p),
                                                          ctypes.c_int, ctypes.c_int, ctypes.c_int, c_f32p, c_f32p, c_f32p, c_f32p,
                                                          c_f32p, ctypes.c_int64, ctypes.c_int, c_f32p, c_void, ctypes.c_size_t,
                                                          ctypes.POINTER(ctypes.c_void_p), ctypes.POINTER(ctypes.c_void_p),
                                                          ctypes.c_int, c_void]),
    'sunerf_mlp_input_grad_exact_workspace_bytes': (ctypes.c_size_t, [ctypes.c_int, ctypes.c_int]),
    'sunerf_mlp_input_grad_exact': (ctypes.c_int, [ctypes.POINTER(ctypes.c_void_p), ctypes.POINTER(ctypes.c_void_p), ctypes.c_int,
                                                    ctypes.c_int, ctypes.c_int, c_f32p, c_f32p, c_f32p, c_f32p, c_f32p,
                                                    ctypes.c_int64, ctypes.c_int, c_f32p, c_void, ctypes.c_size_t,
                                                    ctypes.POINTER(ctypes.c_void_p), ctypes.POINTER(ctypes.c_void_p), ctypes.c_int,
                                                    c_f32p, c_f32p, c_f32p, c_f32p, c_f32p, c_void]),
    'sunerf_dt_integral_fwd': (ctypes.c_int, [c_f32p, c_f32p, c_f32p, c_f32p, c_f32p, ctypes.c_int, c_f32p, c_f32p, c_f32p,
                                               c_f32p, ctypes.c_float, ctypes.c_float, ctypes.c_float, ctypes.c_float,
                                               ctypes.c_int64, ctypes.c_int, c_f32p, c_f32p, c_f32p, c_f32p, c_f32p, c_f32p,
                                               c_void]),
    'sunerf_dt_integral_bwd': (ctypes.c_int, [c_f32p, c_f32p, c_f32p, c_f32p, c_f32p, ctypes.c_int, c_f32p, c_f32p, c_f32p,
                                               c_f32p, ctypes.c_float, ctypes.c_float, ctypes.c_float, ctypes.c_float,
                                               ctypes.c_int64, ctypes.c_int, c_f32p, c_f32p, c_f32p, c_f32p, c_f32p, c_void,
                                               c_void]),
    'sunerf_dem_integral': (ctypes.c_int, [c_f32p, c_f32p, c_f32p, c_f32p, c_f32p, ctypes.c_int, ctypes.c_float, ctypes.c_float,
                                            c_f32p, ctypes.c_float, ctypes.c_float, ctypes.c_int64, ctypes.c_int, c_f32p, c_f32p,
                                            c_f32p, c_f32p, c_void]),
    'sunerf_dem_invert': (ctypes.c_int, [c_f32p, c_f32p, c_void, c_void, c_f32p, c_f32p, ctypes.c_int, ctypes.c_int,
                                          ctypes.c_double, ctypes.c_double, ctypes.c_double, ctypes.c_int, ctypes.c_double,
                                          ctypes.c_int, ctypes.c_int64, ctypes.c_int, ctypes.c_int, c_f32p, c_f32p, c_f32p,
                                          c_f32p, c_f32p, c_void, c_void]),
    'sunerf_hier_resample': (ctypes.c_int, [c_f32p, c_f32p, c_f32p, ctypes.c_int, ctypes.c_int64, ctypes.c_int,
                                             ctypes.c_int, c_f32p, c_f32p, c_void]),
    'sunerf_mlp_points_fwd': (ctypes.c_int, [c_void, ctypes.c_int, ctypes.c_int, ctypes.c_int, c_f32p, ctypes.c_int64, c_f32p,
                                              c_void, ctypes.c_int, c_void, ctypes.c_size_t, c_void]),
    'sunerf_sample_pdf': (ctypes.c_int, [c_f32p, c_f32p, c_f32p, ctypes.c_int, ctypes.c_int64, ctypes.c_int, ctypes.c_int,
                                          c_f32p, c_void]),
    'sunerf_observer_rays': (ctypes.c_int, [c_void, c_void, ctypes.c_int, ctypes.c_int, ctypes.c_int64, ctypes.c_int64,
                                             ctypes.POINTER(ctypes.c_float), ctypes.c_float, c_f32p, c_f32p, c_f32p, c_void]),
    'sunerf_view_desc_bytes': (ctypes.c_size_t, []),
    'sunerf_build_ray_pool': (ctypes.c_int, [c_void, ctypes.c_int, ctypes.c_int64, c_void, ctypes.c_int64, ctypes.c_int,
                                              ctypes.c_int, ctypes.c_uint64, ctypes.c_uint64, ctypes.c_int64, ctypes.c_int64,
                                              c_f32p, c_f32p, c_f32p, c_f32p, c_void]),
    'sunerf_observer_desc_bytes': (ctypes.c_size_t, []),
    'sunerf_synchronic_map': (ctypes.c_int, [c_void, ctypes.c_int, ctypes.c_int, c_void, ctypes.c_int, c_void, ctypes.c_int,
                                              ctypes.c_int, ctypes.c_int, ctypes.c_double, c_f32p, c_void, c_void, c_void]),
    'sunerf_map_fill_workspace_bytes': (ctypes.c_size_t, [ctypes.c_int]),
    'sunerf_map_fill': (ctypes.c_int, [c_f32p, ctypes.c_int, ctypes.c_int64, ctypes.c_int, ctypes.c_double, c_void, c_void,
                                        ctypes.c_size_t, c_void]),
    'sunerf_reproject_views': (ctypes.c_int, [c_f32p, ctypes.c_int, c_void, ctypes.c_int, c_void, ctypes.c_int, ctypes.c_double,
                                               c_void, ctypes.c_int, ctypes.c_int64, ctypes.c_float, c_f32p, c_void, c_void]),
    'sunerf_column_rays': (ctypes.c_int, [c_void, c_void, ctypes.c_int, ctypes.c_int, ctypes.c_int64, ctypes.c_int64,
                                           ctypes.c_float, c_f32p, c_f32p, c_f32p, c_void]),
    'sunerf_column_stats': (ctypes.c_int, [c_f32p, c_f32p, c_f32p, ctypes.c_int64, ctypes.c_int, ctypes.c_float, c_f32p, c_f32p,
                                            c_f32p, c_f32p, c_void]),
    'sunerf_simple_star_field': (ctypes.c_int, [c_f32p, c_f32p, c_f32p, ctypes.c_int64, ctypes.c_int, ctypes.c_float,
                                                 ctypes.c_float, ctypes.c_float, ctypes.c_float, ctypes.c_float, c_f32p,
                                                 c_void]),
    'sunerf_simple_star_field_dev': (ctypes.c_int, [c_f32p, c_f32p, c_f32p, ctypes.c_int64, ctypes.c_int, c_f32p,
                                                     ctypes.c_float, c_f32p, c_void]),
    'sunerf_simple_star_bwd_workspace_bytes': (ctypes.c_size_t, []),
    'sunerf_simple_star_bwd': (ctypes.c_int, [c_f32p, c_f32p, c_f32p, ctypes.c_int64, ctypes.c_int, c_f32p, ctypes.c_float,
                                               c_f32p, c_void, ctypes.c_size_t, c_f32p, ctypes.c_int, c_void]),
    'sunerf_dt_integral_bwd_full': (ctypes.c_int, [c_f32p, c_f32p, c_f32p, c_f32p, c_f32p, ctypes.c_int, c_f32p, c_f32p, c_f32p,
                                                    c_f32p, ctypes.c_float, ctypes.c_float, ctypes.c_float, ctypes.c_float,
                                                    ctypes.c_int64, ctypes.c_int, c_f32p, c_f32p, c_f32p, c_f32p, c_f32p,
                                                    c_f32p, c_f32p, c_void, c_void]),
    'sunerf_mhd_frame_bytes': (ctypes.c_size_t, []),
    'sunerf_mhd_field': (ctypes.c_int, [c_f32p, c_f32p, c_f32p, c_f32p, ctypes.c_int64, ctypes.c_int, c_void, c_void, ctypes.c_int,
                                         ctypes.c_int, c_f32p, c_void, c_void]),
    'sunerf_mhd_field_points': (ctypes.c_int, [c_f32p, ctypes.c_int64, c_void, c_void, ctypes.c_int, ctypes.c_int, c_f32p, c_void,
                                                c_void]),
    'sunerf_thomson_integral_fwd': (ctypes.c_int, [c_f32p, ctypes.c_int, ctypes.c_float, c_f32p, c_f32p, c_f32p, c_f32p, c_f32p,
                                                    c_f32p, ctypes.c_int64, ctypes.c_int, c_f32p, c_f32p, c_f32p, c_f32p,
                                                    c_f32p, c_void]),
    'sunerf_thomson_integral_bwd': (ctypes.c_int, [c_f32p, ctypes.c_int, ctypes.c_float, c_f32p, c_f32p, c_f32p, c_f32p, c_f32p,
                                                    c_f32p, ctypes.c_int64, ctypes.c_int, c_f32p, c_f32p, c_f32p, c_f32p,
                                                    c_f32p, c_f32p, c_void, c_void]),
    'sunerf_train_workspace_bytes': (ctypes.c_size_t, []),
    'sunerf_training_loss': (ctypes.c_int, [c_f32p, c_f32p, c_f32p, ctypes.c_int64, c_f32p, ctypes.c_int64,
                                             ctypes.POINTER(ctypes.c_void_p), ctypes.POINTER(ctypes.c_int64), ctypes.c_int,
                                             ctypes.c_int, ctypes.c_float, ctypes.c_float, ctypes.c_float, ctypes.c_float,
                                             c_f32p, c_f32p, c_f32p, c_void, ctypes.c_size_t, c_void]),
    'sunerf_clip_adam_step': (ctypes.c_int, [c_f32p, c_f32p, c_f32p, c_f32p, ctypes.c_int64, ctypes.c_double,
                                              ctypes.c_double, ctypes.c_double, ctypes.c_double, ctypes.c_float,
                                              ctypes.c_float, ctypes.c_int64, c_f32p, c_f32p, c_void, ctypes.c_size_t,
                                              c_void, c_void]),
    'sunerf_image_metrics_workspace_bytes': (ctypes.c_size_t, [ctypes.c_int64, ctypes.c_int, ctypes.c_int]),
    'sunerf_image_metrics': (ctypes.c_int, [c_f32p, c_f32p, ctypes.c_int64, ctypes.c_int, ctypes.c_int, ctypes.c_double, c_void,
                                             c_void, ctypes.c_size_t, c_void]),
    'sunerf_grid_points': (ctypes.c_int, [ctypes.c_int, c_void, c_void, c_void, ctypes.c_int, ctypes.c_int, ctypes.c_int, GridFrame,
                                           ctypes.c_double, ctypes.c_float, ctypes.c_int64, ctypes.c_int64, c_f32p, c_f32p,
                                           c_void]),
    'sunerf_field_quantities': (ctypes.c_int, [ctypes.c_int, c_f32p, ctypes.c_int, c_f32p, ctypes.c_int64, ctypes.c_float,
                                                ctypes.c_float, ctypes.c_float, ctypes.c_float, c_f32p, ctypes.c_int, c_f32p,
                                                c_f32p, c_f32p, c_f32p, c_f32p, c_f32p, c_f32p, c_void]),
    'sunerf_volume_metrics_workspace_bytes': (ctypes.c_size_t, [ctypes.c_int64]),
    'sunerf_volume_metrics': (ctypes.c_int, [c_f32p, c_f32p, ctypes.c_int, ctypes.c_int, ctypes.c_int, c_void, c_void, c_void,
                                              c_void, c_void, ctypes.c_size_t, c_void]),
    'sunerf_grid_field_desc_bytes': (ctypes.c_size_t, []),
    'sunerf_grid_field_fwd': (ctypes.c_int, [c_void, c_f32p, c_f32p, c_f32p, c_f32p, ctypes.c_int64, ctypes.c_int, c_f32p,
                                              ctypes.c_int, c_f32p, c_void, c_f32p, c_void]),
    'sunerf_grid_field_bwd_workspace_bytes': (ctypes.c_size_t, [ctypes.c_int64, ctypes.c_int]),
    'sunerf_grid_field_bwd': (ctypes.c_int, [c_void, c_f32p, c_void, c_f32p, c_void, c_void, ctypes.c_int64, c_void,
                                              ctypes.c_size_t, c_f32p, ctypes.c_int, c_void]),
}

EXPORTED_SYMBOLS = tuple(_SIGNATURES)

# The extension table (include/sunerf_hip_ext.h): entry points added beside the table above, which stays as it is and keeps
# its version.  The same library holds both.
_EXT_SIGNATURES = {
    'sunerf_ext_abi_version': (ctypes.c_int, []),
    'sunerf_dynamic_grid_fwd': (ctypes.c_int, [c_void, c_void, ctypes.c_int, ctypes.c_int, c_f32p, c_f32p, c_f32p, c_f32p, c_f32p,
                                                ctypes.c_int64, ctypes.c_int, c_f32p, ctypes.c_int, c_f32p, c_void, c_f32p,
                                                c_void]),
    'sunerf_dynamic_grid_bwd_workspace_bytes': (ctypes.c_size_t, [ctypes.c_int64, ctypes.c_int]),
    'sunerf_dynamic_grid_bwd': (ctypes.c_int, [c_void, ctypes.c_int, c_f32p, c_void, c_f32p, c_void, c_void, ctypes.c_int64,
                                                c_void, ctypes.c_size_t, c_f32p, ctypes.c_int, c_void]),
}

EXTENSION_SYMBOLS = tuple(_EXT_SIGNATURES)
EXT_ABI_VERSION = 1

# The response-set table (include/sunerf_hip_response.h): the DT integral against any instrument's channels.  A third table
# beside the two above, which stay as they are and keep their versions.
_RS_HEAD = [c_f32p, c_f32p, c_f32p, c_f32p, c_f32p, ctypes.c_int, ctypes.c_int, ctypes.c_int, c_void, c_f32p, c_f32p, c_f32p,
            c_f32p, c_f32p, ctypes.c_float, ctypes.c_float, ctypes.c_float, ctypes.c_float, ctypes.c_int64, ctypes.c_int]
_RESPONSE_SIGNATURES = {
    'sunerf_response_abi_version': (ctypes.c_int, []),
    'sunerf_dt_response_bwd_lds_bytes': (ctypes.c_size_t, [ctypes.c_int, ctypes.c_int, ctypes.c_int]),
    'sunerf_dt_response_fwd': (ctypes.c_int, _RS_HEAD + [c_f32p, c_f32p, c_f32p, c_f32p, c_f32p, c_f32p, c_void]),
    'sunerf_dt_response_bwd': (ctypes.c_int, _RS_HEAD + [c_f32p, c_f32p, c_f32p, c_f32p, c_f32p, c_void, c_void]),
    'sunerf_dt_response_bwd_full': (ctypes.c_int, _RS_HEAD + [c_f32p, c_f32p, c_f32p, c_f32p, c_f32p, c_f32p, c_f32p, c_void,
                                                              c_void]),
}

RESPONSE_SYMBOLS = tuple(_RESPONSE_SIGNATURES)
RESPONSE_ABI_VERSION = 1

# The image-preparation table (include/sunerf_hip_prep.h): spline prefilter, affine resample, exact order statistics.  A fourth
# table beside the three above, which stay as they are and keep their versions.
_PREP_SIGNATURES = {
    'sunerf_prep_abi_version': (ctypes.c_int, []),
    'sunerf_prep_workspace_bytes': (ctypes.c_size_t, [ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int]),
    'sunerf_prep_spline_prefilter': (ctypes.c_int, [c_f32p, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int, c_void, c_void,
                                                     c_void, ctypes.c_size_t, c_void]),
    'sunerf_prep_affine_resample': (ctypes.c_int, [c_void, c_void, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int]
                                    + [ctypes.c_double] * 7 + [c_void, ctypes.c_int, ctypes.c_int, ctypes.c_int, c_f32p, c_void]),
    'sunerf_prep_order_statistics': (ctypes.c_int, [c_f32p, ctypes.c_int, ctypes.c_int64, c_void, ctypes.c_int, c_f32p, c_void,
                                                     c_void, ctypes.c_size_t, c_void]),
}

PREP_SYMBOLS = tuple(_PREP_SIGNATURES)
PREP_ABI_VERSION = 1

# The instrument table (include/sunerf_hip_instrument.h): PSF-and-bin correlation, detector noise, the Philox generator.  A fifth
# table beside the four above, which stay as they are and keep their versions.
_INSTRUMENT_SIGNATURES = {
    'sunerf_instrument_abi_version': (ctypes.c_int, []),
    'sunerf_instrument_correlate_bin': (ctypes.c_int, [c_f32p, ctypes.c_int, ctypes.c_int, ctypes.c_int, c_void, ctypes.c_int,
                                                        ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int,
                                                        ctypes.c_double, ctypes.c_int, c_f32p, c_void]),
    'sunerf_instrument_philox': (ctypes.c_int, [c_void, ctypes.c_int64, ctypes.c_uint32, ctypes.c_uint32, c_void, c_void]),
    'sunerf_instrument_noise': (ctypes.c_int, [c_f32p, ctypes.c_int, ctypes.c_int, ctypes.c_int, c_void, ctypes.c_uint64,
                                                ctypes.c_int64, ctypes.c_int, c_f32p, c_f32p, c_void, c_void]),
}

INSTRUMENT_SYMBOLS = tuple(_INSTRUMENT_SIGNATURES)
INSTRUMENT_ABI_VERSION = 1

# The patch table (include/sunerf_hip_patch.h): the adjoint of the PSF-and-bin correlation and the records of a batch of patches.
# A sixth table beside the five above, which stay as they are and keep their versions.
_PATCH_SIGNATURES = {
    'sunerf_patch_abi_version': (ctypes.c_int, []),
    'sunerf_patch_correlate_bin_adjoint': (ctypes.c_int, [c_f32p, ctypes.c_int, ctypes.c_int, ctypes.c_int, c_void, ctypes.c_int,
                                                           ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int,
                                                           ctypes.c_double, ctypes.c_int, c_f32p, c_void]),
    'sunerf_patch_records': (ctypes.c_int, [c_void, ctypes.c_int, c_void, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int,
                                             ctypes.c_int, ctypes.c_int, c_f32p, c_f32p, c_f32p, c_f32p, c_void]),
}

PATCH_SYMBOLS = tuple(_PATCH_SIGNATURES)
PATCH_ABI_VERSION = 1

# The likelihood table (include/sunerf_hip_likelihood.h): the Gaussian noise likelihood of the detector model as the training loss,
# with per-row calibration gains.  A seventh table beside the six above, which stay as they are and keep their versions.
_LIKELIHOOD_SIGNATURES = {
    'sunerf_likelihood_abi_version': (ctypes.c_int, []),
    'sunerf_likelihood_workspace_bytes': (ctypes.c_size_t, [ctypes.c_int]),
    'sunerf_likelihood_loss': (ctypes.c_int, [c_f32p, c_f32p, c_f32p, c_f32p, ctypes.c_int64, ctypes.c_int, c_f32p, c_void, c_f32p,
                                               ctypes.c_int, ctypes.c_int, c_f32p, ctypes.c_int64,
                                               ctypes.POINTER(ctypes.c_void_p), ctypes.POINTER(ctypes.c_int64), ctypes.c_int,
                                               ctypes.c_float, ctypes.c_float, c_f32p, c_f32p, c_void, c_void, c_f32p, c_void,
                                               ctypes.c_size_t, c_void]),
}

LIKELIHOOD_SYMBOLS = tuple(_LIKELIHOOD_SIGNATURES)
LIKELIHOOD_ABI_VERSION = 1

# The structural-loss table (include/sunerf_hip_ssim_loss.h): D-SSIM of a batch of patches with its gradient.  An eighth table
# beside the seven above, which stay as they are and keep their versions.
_SSIM_LOSS_SIGNATURES = {
    'sunerf_ssim_loss_abi_version': (ctypes.c_int, []),
    'sunerf_ssim_loss_workspace_bytes': (ctypes.c_size_t, [ctypes.c_int64, ctypes.c_int]),
    'sunerf_ssim_loss': (ctypes.c_int, [c_f32p, c_f32p, c_f32p, ctypes.c_int64, ctypes.c_int, ctypes.c_int, ctypes.c_int,
                                         ctypes.c_double, ctypes.c_double, ctypes.c_double, ctypes.c_int, c_f32p, c_f32p, c_void,
                                         c_void, c_void, ctypes.c_size_t, c_void]),
}

SSIM_LOSS_SYMBOLS = tuple(_SSIM_LOSS_SIGNATURES)
SSIM_LOSS_ABI_VERSION = 1

# The deconvolution table (include/sunerf_hip_deconvolve.h): Richardson-Lucy against the PSF-and-bin kernel, the iterations
# enqueued by one call.  A ninth table beside the eight above, which stay as they are and keep their versions.
_DECONVOLVE_SIGNATURES = {
    'sunerf_deconvolve_abi_version': (ctypes.c_int, []),
    'sunerf_deconvolve_workspace_bytes': (ctypes.c_size_t, [ctypes.c_int] * 6),
    'sunerf_deconvolve_richardson_lucy': (ctypes.c_int, [c_f32p, c_f32p, c_void, c_f32p, c_void, ctypes.c_int, ctypes.c_int,
                                                          ctypes.c_int, c_void, ctypes.c_int, ctypes.c_int, ctypes.c_int,
                                                          ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_double, ctypes.c_int,
                                                          ctypes.c_int, ctypes.c_double, c_f32p, c_void, c_void, c_void]),
}

DECONVOLVE_SYMBOLS = tuple(_DECONVOLVE_SIGNATURES)
DECONVOLVE_ABI_VERSION = 1

# The PSF-gradient table (include/sunerf_hip_psf_grad.h): the derivative of the PSF-and-bin correlation with respect to its taps.
# A tenth table beside the nine above, which stay as they are and keep their versions.
_PSF_GRAD_SIGNATURES = {
    'sunerf_psf_grad_abi_version': (ctypes.c_int, []),
    'sunerf_psf_grad_workspace_bytes': (ctypes.c_size_t, [ctypes.c_int] * 7),
    'sunerf_psf_grad_taps': (ctypes.c_int, [c_f32p, c_f32p] + [ctypes.c_int] * 9 + [ctypes.c_double, ctypes.c_int, c_void, c_void,
                                                                                     c_void]),
}

PSF_GRAD_SYMBOLS = tuple(_PSF_GRAD_SIGNATURES)
PSF_GRAD_ABI_VERSION = 1

# The despiking table (include/sunerf_hip_despike.h): cosmic-ray hits and hot pixels found by an iterated masked median and filled.
# An eleventh table beside the ten above, which stay as they are and keep their versions.
_DESPIKE_SIGNATURES = {
    'sunerf_despike_abi_version': (ctypes.c_int, []),
    'sunerf_despike_workspace_bytes': (ctypes.c_size_t, [ctypes.c_int] * 4),
    'sunerf_despike': (ctypes.c_int, [c_f32p, c_void, c_void] + [ctypes.c_int] * 6 + [ctypes.c_double, ctypes.c_double, ctypes.c_int,
                                      ctypes.c_int, c_f32p, c_void, c_void, c_void, c_void]),
}

DESPIKE_SYMBOLS = tuple(_DESPIKE_SIGNATURES)
DESPIKE_ABI_VERSION = 1

# The co-alignment table (include/sunerf_hip_coalign.h): the six sums of a masked zero-mean normalised cross-correlation for every
# integer shift of a window.  A twelfth table beside the eleven above, which stay as they are and keep their versions.
_COALIGN_SIGNATURES = {
    'sunerf_coalign_abi_version': (ctypes.c_int, []),
    'sunerf_coalign_workspace_bytes': (ctypes.c_size_t, [ctypes.c_int] * 5),
    'sunerf_coalign_shift_sums': (ctypes.c_int, [c_f32p, c_f32p, c_void, c_void] + [ctypes.c_int] * 5 + [c_void, c_void, c_void]),
}

COALIGN_SYMBOLS = tuple(_COALIGN_SIGNATURES)
COALIGN_ABI_VERSION = 1

# The stacking table (include/sunerf_hip_stack.h): an order statistic or the mean of every pixel over a stack of frames, after an
# optional clipping against the pixel's own median.  A thirteenth table beside the twelve above, which stay as they are and keep
# their versions.
_STACK_SIGNATURES = {
    'sunerf_stack_abi_version': (ctypes.c_int, []),
    'sunerf_stack_combine': (ctypes.c_int, [c_f32p, c_void, c_void] + [ctypes.c_int] * 5 + [ctypes.c_double] + [ctypes.c_int] * 3
                             + [ctypes.c_double] + [ctypes.c_int] * 3 + [c_f32p, c_void, c_void, c_void, c_void]),
}

STACK_SYMBOLS = tuple(_STACK_SIGNATURES)
STACK_ABI_VERSION = 1

# The noise-gating table (include/sunerf_hip_noise_gate.h): an image sequence in overlapping apodised blocks, every Fourier
# coefficient of a block kept, dropped or attenuated by the block's own expected noise power.  A fourteenth table beside the
# thirteen above, which stay as they are and keep their versions.
_NOISE_GATE_SIGNATURES = {
    'sunerf_noise_gate_abi_version': (ctypes.c_int, []),
    'sunerf_noise_gate': (ctypes.c_int, [c_f32p, c_void, c_void, c_void] + [ctypes.c_int] * 7 + [ctypes.c_double]
                          + [c_f32p, c_void, c_void]),
}

NOISE_GATE_SYMBOLS = tuple(_NOISE_GATE_SIGNATURES)
NOISE_GATE_ABI_VERSION = 1

# The registration table (include/sunerf_hip_register.h): the frames of a sequence, each with its own observer, grid and time,
# resampled onto one reference observer, grid and time through the sphere and a differential rotation law.  A fifteenth table
# beside the fourteen above, which stay as they are and keep their versions.
_REGISTER_SIGNATURES = {
    'sunerf_register_abi_version': (ctypes.c_int, []),
    'sunerf_register_frame_desc_bytes': (ctypes.c_size_t, []),
    'sunerf_register_frames': (ctypes.c_int, [c_void] + [ctypes.c_int] * 3 + [c_f32p, c_void, c_void] + [ctypes.c_int] * 2
                               + [ctypes.c_double] * 4 + [ctypes.c_int, ctypes.c_float, ctypes.c_int]
                               + [c_f32p, c_void, c_void, c_void, c_void]),
}

REGISTER_SYMBOLS = tuple(_REGISTER_SIGNATURES)
REGISTER_ABI_VERSION = 1

# The enhancement table (include/sunerf_hip_enhance.h): multi-scale Gaussian normalisation, ring statistics and the normalising
# radial graded filter.  A sixteenth table beside the fifteen above, which stay as they are and keep their versions.
_ENHANCE_SIGNATURES = {
    'sunerf_enhance_abi_version': (ctypes.c_int, []),
    'sunerf_enhance_mgn_workspace_bytes': (ctypes.c_size_t, [ctypes.c_int] * 3),
    'sunerf_enhance_mgn': (ctypes.c_int, [c_f32p, c_void] + [ctypes.c_int] * 3 + [c_void, c_void, ctypes.c_int, ctypes.c_double]
                           + [ctypes.c_float] * 3 + [c_f32p] * 6 + [c_void, c_void, ctypes.c_size_t, c_void]),
    'sunerf_enhance_radial_statistics': (ctypes.c_int, [c_f32p, c_void] + [ctypes.c_int] * 3 + [ctypes.c_double] * 2
                                         + [c_void, ctypes.c_int, ctypes.c_int] + [c_void] * 6),
    'sunerf_enhance_nrgf': (ctypes.c_int, [c_f32p, c_void] + [ctypes.c_int] * 3 + [ctypes.c_double] * 2
                            + [c_void, ctypes.c_int, ctypes.c_int, ctypes.c_float, ctypes.c_int] + [c_void] * 5 + [c_f32p, c_void, c_void]),
}

ENHANCE_SYMBOLS = tuple(_ENHANCE_SIGNATURES)
ENHANCE_ABI_VERSION = 1


class SunerfHipError(RuntimeError):
    pass


def load():
    """Loads the library once; raises (never falls back) when it is absent."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise SunerfHipError(
                f'{LIB_PATH} not found: build it with 2024-hl-spi3s-sunerf_amd/csrc/build.sh '
                '(or __graft_entry__.build()); there is no CPU fallback for the render path')
        lib = ctypes.CDLL(LIB_PATH)
        for name, (res, args) in _SIGNATURES.items():
            fn = getattr(lib, name)
            fn.restype = res
            fn.argtypes = args
        if lib.sunerf_abi_version() != 9:
            raise SunerfHipError('libsunerf_hip.so ABI version mismatch')
        for name, (res, args) in _EXT_SIGNATURES.items():
            fn = getattr(lib, name)
            fn.restype = res
            fn.argtypes = args
        if lib.sunerf_ext_abi_version() != EXT_ABI_VERSION:
            raise SunerfHipError('libsunerf_hip.so extension ABI version mismatch')
        for name, (res, args) in _RESPONSE_SIGNATURES.items():
            fn = getattr(lib, name)
            fn.restype = res
            fn.argtypes = args
        if lib.sunerf_response_abi_version() != RESPONSE_ABI_VERSION:
            raise SunerfHipError('libsunerf_hip.so response-set ABI version mismatch')
        for name, (res, args) in _PREP_SIGNATURES.items():
            fn = getattr(lib, name)
            fn.restype = res
            fn.argtypes = args
        if lib.sunerf_prep_abi_version() != PREP_ABI_VERSION:
            raise SunerfHipError('libsunerf_hip.so image-preparation ABI version mismatch')
        for name, (res, args) in _INSTRUMENT_SIGNATURES.items():
            fn = getattr(lib, name)
            fn.restype = res
            fn.argtypes = args
        if lib.sunerf_instrument_abi_version() != INSTRUMENT_ABI_VERSION:
            raise SunerfHipError('libsunerf_hip.so instrument ABI version mismatch')
        for name, (res, args) in _PATCH_SIGNATURES.items():
            fn = getattr(lib, name)
            fn.restype = res
            fn.argtypes = args
        if lib.sunerf_patch_abi_version() != PATCH_ABI_VERSION:
            raise SunerfHipError('libsunerf_hip.so patch ABI version mismatch')
        for name, (res, args) in _LIKELIHOOD_SIGNATURES.items():
            fn = getattr(lib, name)
            fn.restype = res
            fn.argtypes = args
        if lib.sunerf_likelihood_abi_version() != LIKELIHOOD_ABI_VERSION:
            raise SunerfHipError('libsunerf_hip.so likelihood ABI version mismatch')
        for name, (res, args) in _SSIM_LOSS_SIGNATURES.items():
            fn = getattr(lib, name)
            fn.restype = res
            fn.argtypes = args
        if lib.sunerf_ssim_loss_abi_version() != SSIM_LOSS_ABI_VERSION:
            raise SunerfHipError('libsunerf_hip.so structural-loss ABI version mismatch')
        for name, (res, args) in _DECONVOLVE_SIGNATURES.items():
            fn = getattr(lib, name)
            fn.restype = res
            fn.argtypes = args
        if lib.sunerf_deconvolve_abi_version() != DECONVOLVE_ABI_VERSION:
            raise SunerfHipError('libsunerf_hip.so deconvolution ABI version mismatch')
        for name, (res, args) in _PSF_GRAD_SIGNATURES.items():
            fn = getattr(lib, name)
            fn.restype = res
            fn.argtypes = args
        if lib.sunerf_psf_grad_abi_version() != PSF_GRAD_ABI_VERSION:
            raise SunerfHipError('libsunerf_hip.so PSF-gradient ABI version mismatch')
        for name, (res, args) in _DESPIKE_SIGNATURES.items():
            fn = getattr(lib, name)
            fn.restype = res
            fn.argtypes = args
        if lib.sunerf_despike_abi_version() != DESPIKE_ABI_VERSION:
            raise SunerfHipError('libsunerf_hip.so despiking ABI version mismatch')
        for name, (res, args) in _COALIGN_SIGNATURES.items():
            fn = getattr(lib, name)
            fn.restype = res
            fn.argtypes = args
        if lib.sunerf_coalign_abi_version() != COALIGN_ABI_VERSION:
            raise SunerfHipError('libsunerf_hip.so co-alignment ABI version mismatch')
        for name, (res, args) in _STACK_SIGNATURES.items():
            fn = getattr(lib, name)
            fn.restype = res
            fn.argtypes = args
        if lib.sunerf_stack_abi_version() != STACK_ABI_VERSION:
            raise SunerfHipError('libsunerf_hip.so stacking ABI version mismatch')
        for name, (res, args) in _NOISE_GATE_SIGNATURES.items():
            fn = getattr(lib, name)
            fn.restype = res
            fn.argtypes = args
        if lib.sunerf_noise_gate_abi_version() != NOISE_GATE_ABI_VERSION:
            raise SunerfHipError('libsunerf_hip.so noise-gating ABI version mismatch')
        for name, (res, args) in _REGISTER_SIGNATURES.items():
            fn = getattr(lib, name)
            fn.restype = res
            fn.argtypes = args
        if lib.sunerf_register_abi_version() != REGISTER_ABI_VERSION:
            raise SunerfHipError('libsunerf_hip.so registration ABI version mismatch')
        for name, (res, args) in _ENHANCE_SIGNATURES.items():
            fn = getattr(lib, name)
            fn.restype = res
            fn.argtypes = args
        if lib.sunerf_enhance_abi_version() != ENHANCE_ABI_VERSION:
            raise SunerfHipError('libsunerf_hip.so enhancement ABI version mismatch')
        _lib = lib
    return _lib


_ERRORS = {-1: 'bad argument (null pointer or non-positive size)',
           -2: 'unsupported configuration (d_filter / n_layers / sample count outside the compiled set)',
           -3: 'workspace too small'}


def check(status, what):
    if status == 0:
        return
    if status in (-1, -2, -3):
        raise ValueError(f'{what}: {_ERRORS[status]}')
    raise SunerfHipError(f'{what}: HIP error {status}')


def call(device, name, *args):
    """Runs C-ABI entry point ``name`` with ``device`` current (the library sizes its grids from hipGetDevice() and a
    kernel can only be launched into a stream of the current device: a module on cuda:1 while cuda:0 is current would
    otherwise fail or use the wrong CU count) and raises on a non-zero status."""
    fn = getattr(load(), name)
    with torch.cuda.device(device):
        status = fn(*args)
    check(status, name)
