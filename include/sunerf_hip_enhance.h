/* Enhancement entry points of libsunerf_hip.so: multi-scale Gaussian normalisation (MGN, Morgan & Druckmuller 2014) for EUV frames
 * and the normalising radial graded filter (NRGF, Morgan, Habbal & Woo 2006) with the ring statistics it stands on, for anything
 * off the limb.  The kernels behind sunerf_hip/enhance.py.  A sixteenth table beside sunerf_hip.h, sunerf_hip_ext.h,
 * sunerf_hip_response.h, sunerf_hip_prep.h, sunerf_hip_instrument.h, sunerf_hip_patch.h, sunerf_hip_likelihood.h,
 * sunerf_hip_ssim_loss.h, sunerf_hip_deconvolve.h, sunerf_hip_psf_grad.h, sunerf_hip_despike.h, sunerf_hip_coalign.h,
 * sunerf_hip_stack.h, sunerf_hip_noise_gate.h and sunerf_hip_register.h, which stay as they are and keep their versions; the
 * same library holds all sixteen.  Same conventions as sunerf_hip.h: row-major device tensors, `stream` a hipStream_t (NULL: the
 * default stream) and the last argument, status 0 on success, SUNERF_E_BADARG (-1), SUNERF_E_UNSUPPORTED (-2),
 * SUNERF_E_WORKSPACE (-3) or a positive hipError_t; argument errors are found before anything touches a device.  The Python
 * binding is sunerf_hip/lib.py: _ENHANCE_SIGNATURES; the host side is sunerf_hip/enhance.py.  DESIGN.md section 8ab.
 *
 * No floating-point atomics anywhere (minimum, maximum and the counters are integer atomics): reruns are bit-identical, and no
 * output depends on what it or the workspace held before the call.  Everything is enqueued on `stream`; nothing is read back.
 *
 * VALIDITY.  A pixel is invalid when it is not finite or when its byte in `bad` (same shape as the image, or NULL) is not 0.
 * An invalid pixel enters no sum, and every output is NaN there.  Planes are independent. */
#ifndef SUNERF_HIP_ENHANCE_H
#define SUNERF_HIP_ENHANCE_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* Version of THIS table; sunerf_hip/lib.py refuses a library that answers anything else. */
#define SUNERF_ENHANCE_ABI_VERSION 1
int sunerf_enhance_abi_version(void);

#define SUNERF_ENHANCE_MAX_SCALES 8
#define SUNERF_ENHANCE_MAX_RADIUS 128
#define SUNERF_ENHANCE_MGN_STATE 3    /* int64 per plane: n_invalid, n_below (valid x < lo), n_above (valid x > hi)          */
#define SUNERF_ENHANCE_NRGF_STATE 3   /* int64 per plane: n_invalid, n_outside, n_degenerate, a pixel counted once, in this order */
#define SUNERF_ENHANCE_MAX_RINGS 4096
#define SUNERF_ENHANCE_MAX_SEGMENTS 360
#define SUNERF_ENHANCE_MAX_BINS 65536
/* tiles of the two convolution passes: a row-pass workgroup forms 4 rows x 512 columns (each lane 8 adjacent columns), a
 * column-pass workgroup 128 rows x 32 columns (each lane 16 adjacent rows) */
#define SUNERF_ENHANCE_ROW_TILE_Y 4
#define SUNERF_ENHANCE_ROW_TILE_X 512
#define SUNERF_ENHANCE_COL_TILE_Y 128
#define SUNERF_ENHANCE_COL_TILE_X 32
/* outside */
#define SUNERF_ENHANCE_OUTSIDE_KEEP 0
#define SUNERF_ENHANCE_OUTSIDE_MISSING 1

/* ---- MGN ------------------------------------------------------------------------------------------------------------------
 *   image  fp32 [n_planes][height][width]; bad uint8, same shape, or NULL                          (device)
 *   sigma  fp64 [n_scales], weights fp32 [n_scales] or NULL (all 1)                                 (HOST)
 *   lo, hi, floor   fp32 [n_planes] or NULL, each on its own                                       (device)
 *   out    fp32 [n_planes][height][width]; lo_out, hi_out fp32 [n_planes]; state int64 [n_planes][3]   written, every element
 *   workspace: sunerf_enhance_mgn_workspace_bytes(n_planes, height, width) bytes, 256-aligned: four fp32 planes per image plane
 *   (the cleaned image, the row sums, the row sums of the mask, r) and 32 bytes per plane.
 *
 * Per scale i: R_i = (int)(truncate sigma_i + 0.5); w_j = exp(-j j / (2 sigma_i sigma_i)) for |j| <= R_i formed in fp64 and rounded
 * to fp32 once (R_i = 0: the one weight 1).  With m the validity mask and edge replication (a replicated tap is as valid as the
 * pixel it replicates), G_i[f] = (sum_y w sum_x w f m) / (sum_y w sum_x w m): rows first, each tap sum accumulated in fp32 by fused
 * multiply-adds in ascending tap order.  In a plane without an invalid pixel (decided on the device from n_invalid, a branch that
 * is uniform over a workgroup) the mask sums are not formed and the numerator is multiplied by fp32(1 / (sum_j w_j)^2), that sum
 * taken in fp64 over the rounded weights.
 *   lo, hi: the caller's, else the minimum and maximum of the plane's valid pixels (a zero is +0; NaN when none is valid).
 *   floor:  the caller's (data units), else 2^-16 max(|lo|, |hi|).  f2 = fp32(floor floor).
 *   r_i = x - G_i[x];  v_i = G_i[r_i r_i] (r squared in fp32 as it is loaded);  s_i = sqrt(v_i + f2);
 *   t_i = atan(k r_i / s_i), 0 where s_i == 0;  a = sum_i weights_i t_i in ascending i, fp32.
 *   g = clamp((x - lo) / (hi - lo), 0, 1) ^ fp32(1 / gamma), 0 where hi <= lo;  out = h g + fp32((1 - h) / n_scales) a.
 * A plane without a valid pixel is NaN throughout and so are its lo and hi.  Values whose squares leave fp32's range are the
 * caller's to rescale.
 *
 * Checked in this order: n_scales outside 1 .. 8: UNSUPPORTED; a NULL sigma, a sigma or truncate that is negative or not finite:
 * BADARG; an R_i above 128: UNSUPPORTED; n_planes, height or width 0 while none is negative: 0, nothing read or written; a
 * negative count, n_planes above 65535, height above 4 x 65535, a k, h or weight that is not finite, a gamma that is not finite
 * and above 0; a NULL image, out, lo_out, hi_out, state or workspace; an image, out, lo, hi, floor, lo_out or hi_out not aligned
 * to 4 bytes, a state not aligned to 8, a workspace not aligned to 256: BADARG; workspace_bytes too small: WORKSPACE. */
size_t sunerf_enhance_mgn_workspace_bytes(int n_planes, int height, int width); /* 0 for a count below 1 */
int sunerf_enhance_mgn(const float* image, const uint8_t* bad, int n_planes, int height, int width, const double* sigma,
                       const float* weights, int n_scales, double truncate, float k, float gamma, float h, const float* lo,
                       const float* hi, const float* floor, float* out, float* lo_out, float* hi_out, int64_t* state,
                       void* workspace, size_t workspace_bytes, void* stream);

/* ---- radial statistics ------------------------------------------------------------------------------------------------------
 *   edges  fp64 [n_rings + 1], >= 0 and strictly ascending (the caller's to see to; any table is read inside its bounds) (device)
 *   count  int64, mean, std, min, max fp64: [n_planes][n_rings][n_segments]                      written, every element
 * Geometry in fp64, every operation rounded on its own (no fused multiply-add): dy = y - cy, dx = x - cx, d2 = dy dy + dx dx;
 * pixel (y, x) lies in ring i iff edges[i] edges[i] <= d2 < edges[i+1] edges[i+1] (no root is taken); with n_segments > 1 in
 * segment min((int)floor((atan2(dy, dx) + pi) / (2 pi) n_segments), n_segments - 1).  Per plane, ring and segment over the valid
 * pixels: count; mean = sum / count; std = sqrt(sum (x - mean)^2 / count) (two passes, population); min; max -- the last four
 * NaN where count == 0.  One workgroup per ring and plane walks the ring's rows in ascending order; the order of every sum is
 * fixed by the shape alone.
 *
 * Checked in this order: n_rings outside 1 .. 4096, n_segments outside 1 .. 360, n_rings n_segments above 65536: UNSUPPORTED;
 * n_planes, height or width 0 while none is negative: 0; a negative count, n_planes above 65535, a cy or cx that is not finite
 * or beyond 2^30 in magnitude (the two pixels by which a row's intervals are widened have to outweigh the rounding of the root),
 * a NULL image, edges, count, mean, std, min or max, an image not aligned to 4 bytes or another of them not aligned to 8: BADARG. */
int sunerf_enhance_radial_statistics(const float* image, const uint8_t* bad, int n_planes, int height, int width, double cy,
                                     double cx, const double* edges, int n_rings, int n_segments, int64_t* count, double* mean,
                                     double* std, double* min, double* max, void* stream);

/* ---- NRGF -------------------------------------------------------------------------------------------------------------------
 *   compute != 0: count, mean, std, min, max [n_planes][n_rings] are written as by sunerf_enhance_radial_statistics with
 *   n_segments = 1 and then used; compute == 0: count, mean and std are the caller's and only read (min, max may be NULL).
 *   out fp32 [n_planes][height][width], state int64 [n_planes][3]                                written, every element
 * One lane per pixel finds its ring b by bisection on edges^2.  An invalid pixel: NaN (n_invalid).  Else a pixel outside
 * [edges[0], edges[n_rings]): its input value (outside = KEEP) or `missing` (n_outside).  Else, where count_b < 2 or std_b == 0
 * (or std_b is NaN): 0 (n_degenerate).  Else fp32((x - mean_b) / std_b), the difference and the quotient in fp64.
 *
 * Checked in this order: n_rings outside 1 .. 4096, an outside other than those above: UNSUPPORTED; n_planes, height or width 0
 * while none is negative: 0; a negative count, n_planes above 65535, a cy or cx that is not finite or beyond 2^30 in magnitude, a
 * NULL image, edges, count, mean, std, out or state, with compute a NULL min or max, an image or out not aligned to 4 bytes or another of them not aligned
 * to 8: BADARG. */
int sunerf_enhance_nrgf(const float* image, const uint8_t* bad, int n_planes, int height, int width, double cy, double cx,
                        const double* edges, int n_rings, int outside, float missing, int compute, int64_t* count, double* mean,
                        double* std, double* min, double* max, float* out, int64_t* state, void* stream);

#ifdef __cplusplus
}
#endif
#endif
