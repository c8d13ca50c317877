/* Image-preparation entry points of libsunerf_hip.so: a detector image becomes a view -- spline prefilter, affine resample
 * (roll to north, recentre, one plate scale) with the scaling / norm / clip epilogue, and exact order statistics for the
 * percentile clip.  A fourth table beside sunerf_hip.h, sunerf_hip_ext.h and sunerf_hip_response.h, which stay as they are and
 * keep their versions; the same library holds all four.  Same conventions: row-major device tensors, `stream` a hipStream_t
 * (NULL: the default stream), status 0 on success, SUNERF_E_BADARG (-1), SUNERF_E_UNSUPPORTED (-2), SUNERF_E_WORKSPACE (-3) or
 * a positive hipError_t; argument errors are found before anything touches a device.  The Python binding is
 * sunerf_hip/lib.py: _PREP_SIGNATURES; the host side is sunerf_hip/prep.py.  DESIGN.md section 8n.
 *
 * Semantics: scipy.ndimage.affine_transform(order = 0 .. 5, mode = 'constant', cval = missing, prefilter = True) of scipy 1.15,
 * restated in fp64 and rounded to fp32 once.  No floating-point atomics anywhere: reruns are bit-identical, and a plane alone
 * gives the bits it gives inside a batch of planes. */
#ifndef SUNERF_HIP_PREP_H
#define SUNERF_HIP_PREP_H

#include "sunerf_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Version of THIS table; sunerf_hip/lib.py refuses a library that answers anything else. */
#define SUNERF_PREP_ABI_VERSION 1
int sunerf_prep_abi_version(void);

#define SUNERF_PREP_MAX_ORDER 5
#define SUNERF_PREP_MAX_RANKS 8
/* A line is filtered in segments of SUNERF_PREP_SEGMENT samples, each by one thread that starts its recursions a horizon early
 * on the mirrored line (prep.SEGMENT / prep.HORIZON of the binding; the horizons per order are 0, 0, 23, 30, 39, 47). */
#define SUNERF_PREP_SEGMENT 128

/* stages of sunerf_prep_workspace_bytes */
#define SUNERF_PREP_STAGE_PREFILTER 0
#define SUNERF_PREP_STAGE_ORDER_STATISTICS 1
/* flags of sunerf_prep_affine_resample */
#define SUNERF_PREP_CLIP_RANGE 1      /* clamp the interpolated value to the plane's [lo, hi] (params 0, 1)           */
#define SUNERF_PREP_NORM 2            /* (v - vmin) / (vmax - vmin) (params 3, 4)                                     */
#define SUNERF_PREP_NORM_CLIP 4       /* ... clamped to [0, 1]                                                        */
#define SUNERF_PREP_CLIP_NEGATIVE 8   /* v < 0 -> 0                                                                   */
#define SUNERF_PREP_PROPAGATE 16      /* NaN where a tap read a pixel whose mask byte is set (needs nonfinite_mask)   */
#define SUNERF_PREP_PARAMS 6          /* doubles per plane: lo, hi, factor, vmin, vmax, reserved                      */

/* Bytes of workspace a stage needs, 0 when it needs none or the shape is refused:
 *   SUNERF_PREP_STAGE_PREFILTER        (n_planes, height, width, param = order): n_planes * height * width * 8 when order >= 2 and
 *                                      height >= 2 (the pass along x writes there, the pass along y reads it), else 0
 *   SUNERF_PREP_STAGE_ORDER_STATISTICS (n_planes, height * width = values per plane, param = n_ranks):
 *                                      n_planes * n_ranks * 16 + n_planes * G * (n_ranks * 256 + 1) * 4,
 *                                      G = min(128, ceil(values / 4096)) workgroups per plane */
size_t sunerf_prep_workspace_bytes(int stage, int n_planes, int height, int width, int param);

/* Spline coefficients of `image` [n_planes, height, width] fp32 -> `coefficients` [n_planes, height, width] fp64: the recursive
 * prefilter of scipy.ndimage.spline_filter(order, mode = 'mirror'), along x and then along y; orders 0 and 1 and lines of
 * length 1 are not filtered (the value as fp64).  A non-finite pixel enters as 0; `nonfinite_mask` [n_planes, height, width]
 * uint8 (may be NULL) receives 1 there and 0 elsewhere.  `workspace`: sunerf_prep_workspace_bytes(PREFILTER, ...) bytes,
 * 8-byte aligned, nothing assumed about its contents; may be NULL when that is 0.
 * Checked in this order: order outside 0 .. 5: UNSUPPORTED; n_planes, height or width 0 and none negative: 0, nothing read or
 * written; a negative count, a NULL image or coefficients, a NULL workspace that is needed: BADARG; workspace_bytes too small:
 * WORKSPACE. */
int sunerf_prep_spline_prefilter(const float* image, int n_planes, int height, int width, int order, double* coefficients,
                                 uint8_t* nonfinite_mask, void* workspace, size_t workspace_bytes, void* stream);

/* out [n_planes, out_height, out_width] fp32 from `coefficients` [n_planes, height, width] fp64.  Output pixel (r, c), 0-based,
 * has the source coordinate (in fp64, in this order of operations, no fused multiply-add)
 *   y = (offset_y + m_yy * r) + m_yx * c,   x = (offset_x + m_xy * r) + m_xx * c
 * and the value `missing` when y leaves [0, height - 1] or x leaves [0, width - 1], else the sum over the (order + 1)^2 taps with
 * scipy's B-spline weights, taps past the edge at their mirrored index.  Then per plane p, with params [n_planes, 6] fp64 (device)
 * = lo, hi, factor, vmin, vmax, reserved, in fp64: CLIP_RANGE clamps to [lo, hi]; v *= factor; NORM takes (v - vmin) / (vmax -
 * vmin), NORM_CLIP clamps that to [0, 1]; CLIP_NEGATIVE sets v < 0 to 0; the value is rounded to fp32 once; a non-finite result
 * becomes 0; PROPAGATE then makes it NaN where a tap read a pixel with nonfinite_mask [n_planes, height, width] set.
 * Checked in this order: order outside 0 .. 5, unknown flag bits: UNSUPPORTED; n_planes, out_height or out_width 0 and no count
 * negative: 0, nothing read or written; a negative count, height or width 0, a NULL coefficients, params or out, PROPAGATE
 * without a mask: BADARG. */
int sunerf_prep_affine_resample(const double* coefficients, const uint8_t* nonfinite_mask, int n_planes, int height, int width,
                                int order, double m_yy, double m_yx, double m_xy, double m_xx, double offset_y, double offset_x,
                                double missing, const double* params, int flags, int out_height, int out_width, float* out,
                                void* stream);

/* Exact order statistics: values [n_planes, n_ranks] fp32 = the element of rank ranks [n_planes, n_ranks] (int64, device, 0-based)
 * of plane p of x [n_planes, n_values] in ascending order, NaNs left out; nan_count [n_planes] int64 = the number left out.  A
 * rank outside [0, n_values - nan_count) gives NaN.  -0.0 sorts below +0.0.  A radix select over the order-preserving integer
 * image of the floats, 8 bits per pass: integer histograms per workgroup (LDS atomics) go to the workspace and are added in a
 * fixed order.  `workspace`: sunerf_prep_workspace_bytes(ORDER_STATISTICS, n_planes, n_values as height * width, n_ranks)
 * bytes, 8-byte aligned, nothing assumed about its contents.
 * Checked in this order: n_ranks outside 1 .. 8: UNSUPPORTED; n_planes or n_values 0 and neither negative: 0, nothing read or
 * written; a negative count, a NULL pointer: BADARG; workspace_bytes too small: WORKSPACE. */
int sunerf_prep_order_statistics(const float* x, int n_planes, int64_t n_values, const int64_t* ranks, int n_ranks, float* values,
                                 int64_t* nan_count, void* workspace, size_t workspace_bytes, void* stream);

#ifdef __cplusplus
}
#endif
#endif
