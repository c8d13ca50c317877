/* Response-set entry points of libsunerf_hip.so: the density / temperature integral of sunerf_hip.h (sunerf_dt_integral_*)
 * against any instrument's channels.  A third table beside sunerf_hip.h and sunerf_hip_ext.h, which stay as they are and keep
 * their versions; the same library holds all three.  Same conventions: row-major fp32 device tensors unless stated, `stream` a
 * hipStream_t (NULL: the default stream), status 0 on success, SUNERF_E_BADARG (-1), SUNERF_E_UNSUPPORTED (-2) or a positive
 * hipError_t; argument errors are found before anything touches a device.  The Python binding is sunerf_hip/lib.py:
 * _RESPONSE_SIGNATURES; the host-side object is sunerf_hip/response.py: ResponseSet.  DESIGN.md section 8m. */
#ifndef SUNERF_HIP_RESPONSE_H
#define SUNERF_HIP_RESPONSE_H

#include "sunerf_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Version of THIS table; sunerf_hip/lib.py refuses a library that answers anything else. */
#define SUNERF_RESPONSE_ABI_VERSION 1
int sunerf_response_abi_version(void);

/* ------------------------------------------------------------------------------------------------------------
 * A response set: n_channels = M channels (1 <= M <= 64), channel m with
 *   codes[m]   [M] fp32: a positive integer below 2^24 (exact in fp32), unique in the set.  It is what a ray's `wavelengths`
 *              row carries for that channel: for an AIA-only set the wavelength in Angstrom, as in sunerf_dt_integral_*
 *   offsets    [M + 1] int32: channel m owns nodes offsets[m] .. offsets[m + 1] - 1 of logt / resp; offsets[0] = 0,
 *              offsets[M] = n_nodes_total <= 4096, at least 2 nodes per channel
 *   logt       [n_nodes_total]: the channel's own log10 T grid, strictly increasing, finite; non-uniform grids and grids of
 *              different lengths are fine
 *   resp       [n_nodes_total]: its temperature response on that grid, exposure time or gain already folded in
 * all four DEVICE arrays.  The grids are validated by the caller (ResponseSet does it on the host) and TRUSTED by the kernels:
 * offsets that are not increasing, or that point past n_nodes_total, read out of bounds.
 *
 * R_m(logT) = linear interpolation on the channel's grid in the interval i = the largest i <= n_m - 2 with x_i <= logT
 * (searchsorted(right) - 1, clamped), y_i + (logT - x_i) * (y_{i+1} - y_i) / (x_{i+1} - x_i) in fp32 -- what
 * sunerf_dt_integral_* computes on its (7,101) table -- and 0 with slope 0 outside [x_0, x_{n_m - 1}].
 *
 * The three integral entry points take the arguments of their sunerf_dt_integral_* counterparts and compute what those compute
 * (sunerf_hip.h), the two (7,101) table pointers replaced by the set:
 *   wavelengths [N, W], 1 <= W <= 8: per ray the codes of its columns.  An entry <= 0 is an absent column; so is a positive
 *              code that the set does not hold: image 0, no gradient.
 *   log_abs    [M] in set order; g_log_abs [M] likewise.
 * Outputs as there: image [N, W], weights / reg_q [N, S] and the optional height_map / absorption_map [N], regularization
 * [N, S]; g_raw [N, S, 2] written once per sample without atomics (reruns are bit-identical), g_absmax the bit pattern of
 * max |g_raw|.  g_log_abs and g_vol_c are sums of per-workgroup partial sums added with float atomics in whatever order the
 * workgroups finish: the free-order contract of sunerf_dt_integral_bwd -- equal between reruns to rounding, not by bits.
 * On a set that holds the seven AIA rows, every other output equals that of sunerf_dt_integral_* bit for bit.
 *
 * The backward keeps exp(-A) of 8 rays in LDS, strided by the call's W:
 *   sunerf_dt_response_bwd_lds_bytes(S, W, n_nodes_total) = (200 + 2 n_nodes_total + 8 S W) * 4 bytes
 * (head: offsets, codes, the scalar sums; the two node tables; the slabs); a call that needs more than 160 KiB answers
 * SUNERF_E_UNSUPPORTED before any launch, nothing written.
 *
 * Checked in this order, sizes and limits before anything touches a device:
 *   n_rays < 0, n_samples < 3, n_channels < 1, n_nodes_total < 2 n_channels               : SUNERF_E_BADARG
 *   n_channels > 64, n_nodes_total > 4096, n_wavelengths < 1 or > 8                       : SUNERF_E_UNSUPPORTED
 *   n_rays == 0: the forward returns 0 and reads no pointer.  The backward needs g_log_abs, g_vol_c and g_absmax
 *     (SUNERF_E_BADARG when one is NULL), zeroes g_log_abs [M], g_vol_c and g_absmax and returns 0
 *   a NULL input, set array or required output                                            : SUNERF_E_BADARG
 *   (backward) the LDS limit                                                              : SUNERF_E_UNSUPPORTED
 * ---------------------------------------------------------------------------------------------------------- */
size_t sunerf_dt_response_bwd_lds_bytes(int n_samples, int n_wavelengths, int n_nodes_total);
int sunerf_dt_response_fwd(const float* raw, const float* z_vals, const float* rays_o, const float* rays_d,
                           const float* wavelengths, int n_wavelengths, int n_channels, int n_nodes_total, const int* offsets,
                           const float* codes, const float* logt, const float* resp, const float* log_abs, const float* vol_c,
                           float base_log_density, float base_log_temperature, float pixel_intensity_factor, float reg_radius,
                           int64_t n_rays, int n_samples, float* image, float* weights, float* reg_q, float* height_map,
                           float* absorption_map, float* regularization, void* stream);
int sunerf_dt_response_bwd(const float* raw, const float* z_vals, const float* rays_o, const float* rays_d,
                           const float* wavelengths, int n_wavelengths, int n_channels, int n_nodes_total, const int* offsets,
                           const float* codes, const float* logt, const float* resp, const float* log_abs, const float* vol_c,
                           float base_log_density, float base_log_temperature, float pixel_intensity_factor, float reg_radius,
                           int64_t n_rays, int n_samples, const float* g_image, const float* g_reg, float* g_raw,
                           float* g_log_abs, float* g_vol_c, void* g_absmax, void* stream);
/* also the gradients arriving at weights and the regularizing quantity (either may be NULL): sunerf_dt_integral_bwd_full */
int sunerf_dt_response_bwd_full(const float* raw, const float* z_vals, const float* rays_o, const float* rays_d,
                                const float* wavelengths, int n_wavelengths, int n_channels, int n_nodes_total,
                                const int* offsets, const float* codes, const float* logt, const float* resp,
                                const float* log_abs, const float* vol_c, float base_log_density, float base_log_temperature,
                                float pixel_intensity_factor, float reg_radius, int64_t n_rays, int n_samples,
                                const float* g_image, const float* g_reg, const float* g_weights, const float* g_reg_q,
                                float* g_raw, float* g_log_abs, float* g_vol_c, void* g_absmax, void* stream);

#ifdef __cplusplus
}
#endif
#endif
