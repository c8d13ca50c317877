"""ctypes binding of libsunerf_hip.so (C ABI: include/sunerf_hip.h and the feature headers beside it).

The library is built in-tree by ``csrc/build.sh`` (``__graft_entry__.build()``).  There is no CPU fallback: if
the library is missing or a tensor is not on a ROCm device the call raises.
"""
import ctypes
import os
from typing import NamedTuple

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


class Table(NamedTuple):
    """One entry-point table of the C ABI: a header under ``include/``, its version function and the signatures it declares.
    ``label`` is what the version-mismatch message calls the table (with its trailing space; empty for the core table)."""
    name: str
    header: str
    label: str
    version_symbol: str
    version: int
    signatures: dict            # symbol -> (restype, argtypes), in the header's order


_RS_HEAD = [c_f32p, c_f32p, c_f32p, c_f32p, c_f32p, ctypes.c_int, ctypes.c_int, ctypes.c_int, c_void, c_f32p, c_f32p, c_f32p,
            c_f32p, c_f32p, ctypes.c_float, ctypes.c_float, ctypes.c_float, ctypes.c_float, ctypes.c_int64, ctypes.c_int]

# Every table lives in the same library and keeps its own version: a new feature adds a table (one entry here, one header, one
# source name in csrc/build.sh) and leaves the others as they are.
TABLES = (
    # The core table: the render path, the MLP forward and backward, the fields, maps, metrics and the static grid.
    Table('core', 'sunerf_hip.h', '', 'sunerf_abi_version', 9, {
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
    }),
    # The extension table: the voxel grid with a time axis.
    Table('ext', 'sunerf_hip_ext.h', 'extension ', 'sunerf_ext_abi_version', 1, {
        'sunerf_ext_abi_version': (ctypes.c_int, []),
        'sunerf_dynamic_grid_fwd': (ctypes.c_int, [c_void, c_void, ctypes.c_int, ctypes.c_int, c_f32p, c_f32p, c_f32p, c_f32p, c_f32p,
                                                    ctypes.c_int64, ctypes.c_int, c_f32p, ctypes.c_int, c_f32p, c_void, c_f32p,
                                                    c_void]),
        'sunerf_dynamic_grid_bwd_workspace_bytes': (ctypes.c_size_t, [ctypes.c_int64, ctypes.c_int]),
        'sunerf_dynamic_grid_bwd': (ctypes.c_int, [c_void, ctypes.c_int, c_f32p, c_void, c_f32p, c_void, c_void, ctypes.c_int64,
                                                    c_void, ctypes.c_size_t, c_f32p, ctypes.c_int, c_void]),
    }),
    # The response-set table: the DT integral against any instrument's channels.
    Table('response', 'sunerf_hip_response.h', 'response-set ', 'sunerf_response_abi_version', 1, {
        'sunerf_response_abi_version': (ctypes.c_int, []),
        'sunerf_dt_response_bwd_lds_bytes': (ctypes.c_size_t, [ctypes.c_int, ctypes.c_int, ctypes.c_int]),
        'sunerf_dt_response_fwd': (ctypes.c_int, _RS_HEAD + [c_f32p, c_f32p, c_f32p, c_f32p, c_f32p, c_f32p, c_void]),
        'sunerf_dt_response_bwd': (ctypes.c_int, _RS_HEAD + [c_f32p, c_f32p, c_f32p, c_f32p, c_f32p, c_void, c_void]),
        'sunerf_dt_response_bwd_full': (ctypes.c_int, _RS_HEAD + [c_f32p, c_f32p, c_f32p, c_f32p, c_f32p, c_f32p, c_f32p, c_void,
                                                                  c_void]),
    }),
    # The image-preparation table: spline prefilter, affine resample, exact order statistics.
    Table('prep', 'sunerf_hip_prep.h', 'image-preparation ', 'sunerf_prep_abi_version', 1, {
        'sunerf_prep_abi_version': (ctypes.c_int, []),
        'sunerf_prep_workspace_bytes': (ctypes.c_size_t, [ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int]),
        'sunerf_prep_spline_prefilter': (ctypes.c_int, [c_f32p, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int, c_void, c_void,
                                                         c_void, ctypes.c_size_t, c_void]),
        'sunerf_prep_affine_resample': (ctypes.c_int, [c_void, c_void, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int]
                                        + [ctypes.c_double] * 7 + [c_void, ctypes.c_int, ctypes.c_int, ctypes.c_int, c_f32p, c_void]),
        'sunerf_prep_order_statistics': (ctypes.c_int, [c_f32p, ctypes.c_int, ctypes.c_int64, c_void, ctypes.c_int, c_f32p, c_void,
                                                         c_void, ctypes.c_size_t, c_void]),
    }),
    # The instrument table: PSF-and-bin correlation, detector noise, the Philox generator.
    Table('instrument', 'sunerf_hip_instrument.h', 'instrument ', 'sunerf_instrument_abi_version', 1, {
        'sunerf_instrument_abi_version': (ctypes.c_int, []),
        'sunerf_instrument_correlate_bin': (ctypes.c_int, [c_f32p, ctypes.c_int, ctypes.c_int, ctypes.c_int, c_void, ctypes.c_int,
                                                            ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int,
                                                            ctypes.c_double, ctypes.c_int, c_f32p, c_void]),
        'sunerf_instrument_philox': (ctypes.c_int, [c_void, ctypes.c_int64, ctypes.c_uint32, ctypes.c_uint32, c_void, c_void]),
        'sunerf_instrument_noise': (ctypes.c_int, [c_f32p, ctypes.c_int, ctypes.c_int, ctypes.c_int, c_void, ctypes.c_uint64,
                                                    ctypes.c_int64, ctypes.c_int, c_f32p, c_f32p, c_void, c_void]),
    }),
    # The patch table: the adjoint of the PSF-and-bin correlation and the records of a batch of patches.
    Table('patch', 'sunerf_hip_patch.h', 'patch ', 'sunerf_patch_abi_version', 1, {
        'sunerf_patch_abi_version': (ctypes.c_int, []),
        'sunerf_patch_correlate_bin_adjoint': (ctypes.c_int, [c_f32p, ctypes.c_int, ctypes.c_int, ctypes.c_int, c_void, ctypes.c_int,
                                                               ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int,
                                                               ctypes.c_double, ctypes.c_int, c_f32p, c_void]),
        'sunerf_patch_records': (ctypes.c_int, [c_void, ctypes.c_int, c_void, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int,
                                                 ctypes.c_int, ctypes.c_int, c_f32p, c_f32p, c_f32p, c_f32p, c_void]),
    }),
    # The likelihood table: the Gaussian noise likelihood of the detector model as the training loss, with per-row calibration
    # gains.
    Table('likelihood', 'sunerf_hip_likelihood.h', 'likelihood ', 'sunerf_likelihood_abi_version', 1, {
        'sunerf_likelihood_abi_version': (ctypes.c_int, []),
        'sunerf_likelihood_workspace_bytes': (ctypes.c_size_t, [ctypes.c_int]),
        'sunerf_likelihood_loss': (ctypes.c_int, [c_f32p, c_f32p, c_f32p, c_f32p, ctypes.c_int64, ctypes.c_int, c_f32p, c_void, c_f32p,
                                                   ctypes.c_int, ctypes.c_int, c_f32p, ctypes.c_int64,
                                                   ctypes.POINTER(ctypes.c_void_p), ctypes.POINTER(ctypes.c_int64), ctypes.c_int,
                                                   ctypes.c_float, ctypes.c_float, c_f32p, c_f32p, c_void, c_void, c_f32p, c_void,
                                                   ctypes.c_size_t, c_void]),
    }),
    # The structural-loss table: D-SSIM of a batch of patches with its gradient.
    Table('ssim_loss', 'sunerf_hip_ssim_loss.h', 'structural-loss ', 'sunerf_ssim_loss_abi_version', 1, {
        'sunerf_ssim_loss_abi_version': (ctypes.c_int, []),
        'sunerf_ssim_loss_workspace_bytes': (ctypes.c_size_t, [ctypes.c_int64, ctypes.c_int]),
        'sunerf_ssim_loss': (ctypes.c_int, [c_f32p, c_f32p, c_f32p, ctypes.c_int64, ctypes.c_int, ctypes.c_int, ctypes.c_int,
                                             ctypes.c_double, ctypes.c_double, ctypes.c_double, ctypes.c_int, c_f32p, c_f32p, c_void,
                                             c_void, c_void, ctypes.c_size_t, c_void]),
    }),
    # The deconvolution table: Richardson-Lucy against the PSF-and-bin kernel, the iterations enqueued by one call.
    Table('deconvolve', 'sunerf_hip_deconvolve.h', 'deconvolution ', 'sunerf_deconvolve_abi_version', 1, {
        'sunerf_deconvolve_abi_version': (ctypes.c_int, []),
        'sunerf_deconvolve_workspace_bytes': (ctypes.c_size_t, [ctypes.c_int] * 6),
        'sunerf_deconvolve_richardson_lucy': (ctypes.c_int, [c_f32p, c_f32p, c_void, c_f32p, c_void, ctypes.c_int, ctypes.c_int,
                                                              ctypes.c_int, c_void, ctypes.c_int, ctypes.c_int, ctypes.c_int,
                                                              ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_double, ctypes.c_int,
                                                              ctypes.c_int, ctypes.c_double, c_f32p, c_void, c_void, c_void]),
    }),
    # The PSF-gradient table: the derivative of the PSF-and-bin correlation with respect to its taps.
    Table('psf_grad', 'sunerf_hip_psf_grad.h', 'PSF-gradient ', 'sunerf_psf_grad_abi_version', 1, {
        'sunerf_psf_grad_abi_version': (ctypes.c_int, []),
        'sunerf_psf_grad_workspace_bytes': (ctypes.c_size_t, [ctypes.c_int] * 7),
        'sunerf_psf_grad_taps': (ctypes.c_int, [c_f32p, c_f32p] + [ctypes.c_int] * 9 + [ctypes.c_double, ctypes.c_int, c_void, c_void,
                                                                                         c_void]),
    }),
    # The despiking table: cosmic-ray hits and hot pixels found by an iterated masked median and filled.
    Table('despike', 'sunerf_hip_despike.h', 'despiking ', 'sunerf_despike_abi_version', 1, {
        'sunerf_despike_abi_version': (ctypes.c_int, []),
        'sunerf_despike_workspace_bytes': (ctypes.c_size_t, [ctypes.c_int] * 4),
        'sunerf_despike': (ctypes.c_int, [c_f32p, c_void, c_void] + [ctypes.c_int] * 6 + [ctypes.c_double, ctypes.c_double, ctypes.c_int,
                                          ctypes.c_int, c_f32p, c_void, c_void, c_void, c_void]),
    }),
    # The co-alignment table: the six sums of a masked zero-mean normalised cross-correlation for every integer shift of a window.
    Table('coalign', 'sunerf_hip_coalign.h', 'co-alignment ', 'sunerf_coalign_abi_version', 1, {
        'sunerf_coalign_abi_version': (ctypes.c_int, []),
        'sunerf_coalign_workspace_bytes': (ctypes.c_size_t, [ctypes.c_int] * 5),
        'sunerf_coalign_shift_sums': (ctypes.c_int, [c_f32p, c_f32p, c_void, c_void] + [ctypes.c_int] * 5 + [c_void, c_void, c_void]),
    }),
    # The stacking table: an order statistic or the mean of every pixel over a stack of frames, after an optional clipping against
    # the pixel's own median.
    Table('stack', 'sunerf_hip_stack.h', 'stacking ', 'sunerf_stack_abi_version', 1, {
        'sunerf_stack_abi_version': (ctypes.c_int, []),
        'sunerf_stack_combine': (ctypes.c_int, [c_f32p, c_void, c_void] + [ctypes.c_int] * 5 + [ctypes.c_double] + [ctypes.c_int] * 3
                                 + [ctypes.c_double] + [ctypes.c_int] * 3 + [c_f32p, c_void, c_void, c_void, c_void]),
    }),
    # The noise-gating table: an image sequence in overlapping apodised blocks, every Fourier coefficient of a block kept, dropped
    # or attenuated by the block's own expected noise power.
    Table('noise_gate', 'sunerf_hip_noise_gate.h', 'noise-gating ', 'sunerf_noise_gate_abi_version', 1, {
        'sunerf_noise_gate_abi_version': (ctypes.c_int, []),
        'sunerf_noise_gate': (ctypes.c_int, [c_f32p, c_void, c_void, c_void] + [ctypes.c_int] * 7 + [ctypes.c_double]
                              + [c_f32p, c_void, c_void]),
    }),
    # The registration table: the frames of a sequence, each with its own observer, grid and time, resampled onto one reference
    # observer, grid and time through the sphere and a differential rotation law.
    Table('register', 'sunerf_hip_register.h', 'registration ', 'sunerf_register_abi_version', 1, {
        'sunerf_register_abi_version': (ctypes.c_int, []),
        'sunerf_register_frame_desc_bytes': (ctypes.c_size_t, []),
        'sunerf_register_frames': (ctypes.c_int, [c_void] + [ctypes.c_int] * 3 + [c_f32p, c_void, c_void] + [ctypes.c_int] * 2
                                   + [ctypes.c_double] * 4 + [ctypes.c_int, ctypes.c_float, ctypes.c_int]
                                   + [c_f32p, c_void, c_void, c_void, c_void]),
    }),
    # The enhancement table: multi-scale Gaussian normalisation, ring statistics and the normalising radial graded filter.
    Table('enhance', 'sunerf_hip_enhance.h', 'enhancement ', 'sunerf_enhance_abi_version', 1, {
        'sunerf_enhance_abi_version': (ctypes.c_int, []),
        'sunerf_enhance_mgn_workspace_bytes': (ctypes.c_size_t, [ctypes.c_int] * 3),
        'sunerf_enhance_mgn': (ctypes.c_int, [c_f32p, c_void] + [ctypes.c_int] * 3 + [c_void, c_void, ctypes.c_int, ctypes.c_double]
                               + [ctypes.c_float] * 3 + [c_f32p] * 6 + [c_void, c_void, ctypes.c_size_t, c_void]),
        'sunerf_enhance_radial_statistics': (ctypes.c_int, [c_f32p, c_void] + [ctypes.c_int] * 3 + [ctypes.c_double] * 2
                                             + [c_void, ctypes.c_int, ctypes.c_int] + [c_void] * 6),
        'sunerf_enhance_nrgf': (ctypes.c_int, [c_f32p, c_void] + [ctypes.c_int] * 3 + [ctypes.c_double] * 2
                                + [c_void, ctypes.c_int, ctypes.c_int, ctypes.c_float, ctypes.c_int] + [c_void] * 5 + [c_f32p, c_void, c_void]),
    }),
)


# The second registry: ``TABLES`` is frozen at its sixteen tables, by count, names and contents (tests/test_abi_tables_host.py), so
# a table added after them is entered here.  ``load()`` binds and version-checks it after ``TABLES``; ``symbols(name)`` and
# ``signature(symbol)`` answer for it; ``symbols()`` without a name stays the sixteen.
ADDED_TABLES = (
    # The polarimetry table: polariser exposures to Stokes planes, tB and pB; the polarisation-ratio depth of a (tB, pB) pair.
    Table('polarimetry', 'sunerf_hip_polarimetry.h', 'polarimetry ', 'sunerf_polarimetry_abi_version', 1, {
        'sunerf_polarimetry_abi_version': (ctypes.c_int, []),
        'sunerf_polarimetry_stokes': (ctypes.c_int, [c_f32p, c_void] + [ctypes.POINTER(ctypes.c_double)] * 4 + [c_void, c_void]
                                      + [ctypes.c_int] * 4 + [ctypes.c_double] * 2 + [c_f32p] * 7 + [c_void, c_void, c_void]),
        'sunerf_polarimetry_ratio_depth': (ctypes.c_int, [c_f32p] * 6 + [ctypes.c_int64, ctypes.c_double] + [c_f32p] * 5
                                           + [c_void, c_void]),
    }),
)


def symbols(table=None):
    """The entry-point names of every table of ``TABLES`` in table order, or of the table called ``table`` alone, which may be one of
    ``ADDED_TABLES``."""
    if table is None:
        return tuple(name for t in TABLES for name in t.signatures)
    return tuple(name for t in TABLES + ADDED_TABLES if table == t.name for name in t.signatures)


def signature(name):
    """``(restype, argtypes)`` of the entry point ``name``, whichever table declares it."""
    for t in TABLES + ADDED_TABLES:
        if name in t.signatures:
            return t.signatures[name]
    raise KeyError(name)


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
        for t in TABLES + ADDED_TABLES:
            for name, (res, args) in t.signatures.items():
                fn = getattr(lib, name)
                fn.restype = res
                fn.argtypes = args
            if getattr(lib, t.version_symbol)() != t.version:
                raise SunerfHipError(f'libsunerf_hip.so {t.label}ABI version mismatch')
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
