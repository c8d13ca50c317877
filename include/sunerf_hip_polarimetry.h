/* White-light polarimetry entry points of libsunerf_hip.so: the exposures of a coronagraph through a linear polariser turned into
 * the Stokes planes and the total and polarised brightness (tB, pB) that ThompsonScattering renders and trains on, and the
 * polarisation-ratio method (Moran & Davis 2004) that turns a (tB, pB) pair into the distance of the scattering electrons from the
 * plane of the sky through the Thomson-scattering formulas of Howard & Tappin 2009.  A table beside the sixteen of sunerf_hip.h ..
 * sunerf_hip_enhance.h, which stay as they are and keep their versions; the same library holds all of them.  Same conventions as
 * sunerf_hip_stack.h: row-major device tensors, `stream` a hipStream_t (NULL: the default stream) and the last argument, status 0 on
 * success, SUNERF_E_BADARG (-1), SUNERF_E_UNSUPPORTED (-2) or a positive hipError_t; argument errors are found before anything
 * touches a device; nothing is allocated and nothing waits.  The Python binding is sunerf_hip/lib.py: ADDED_TABLES; the host side is
 * sunerf_hip/polarimetry.py.  DESIGN.md section 8af.
 *
 * No floating-point atomics anywhere and no sum of floating-point numbers across threads: reruns are bit-identical, and a pixel or
 * ray alone gives the bits it gives inside a batch.  All arithmetic is IEEE fp64 on the (double) inputs with every operation rounded
 * on its own (no fused multiply-add), in the order written; a result is rounded to fp32 once.  There is no workspace. */
#ifndef SUNERF_HIP_POLARIMETRY_H
#define SUNERF_HIP_POLARIMETRY_H

#include "sunerf_hip_patch.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Version of THIS table; sunerf_hip/lib.py refuses a library that answers anything else. */
#define SUNERF_POLARIMETRY_ABI_VERSION 1
int sunerf_polarimetry_abi_version(void);

#define SUNERF_POLARIMETRY_MIN_FRAMES 3
#define SUNERF_POLARIMETRY_MAX_FRAMES 8
#define SUNERF_POLARIMETRY_COUNTS 4 /* int64 per plane: pixels DETERMINED, UNDETERMINED, CENTRE, pixels that lost a sample */

/* status of a pixel (uint8) */
#define SUNERF_POLARIMETRY_DETERMINED 0
#define SUNERF_POLARIMETRY_UNDETERMINED 1 /* fewer than 3 valid samples, or a pivot of the solve at or below 2^-40 of its diagonal */
#define SUNERF_POLARIMETRY_CENTRE 2       /* solved, and dx = dy = 0: I, Q, U, chi2 and sigma_tb stand, pb, pb_cross and sigma_pb are NaN */

/* One call, one kernel, one lane per pixel: the weighted least-squares fit of (I, Q, U) to n_frames exposures through a linear
 * polariser.
 *
 *   frames      fp32 [n_frames, n_planes, height, width]     may hold NaN and +-inf
 *   bad         uint8, shape of frames, or NULL               not 0: the sample is not valid
 *   cos2, sin2  HOST fp64 [n_frames]                          cosine and sine of TWICE the polariser angle of frame k
 *   throughput  HOST fp64 [n_frames]                          t_k > 0
 *   efficiency  HOST fp64 [n_frames]                          e_k > 0 (1: an ideal polariser)
 *   a, b        fp64 [n_planes] each, or both NULL            variance of a sample y: a + b * (y > 0 ? y : 0); both NULL: weight 1
 *   cy, cx      the Sun's centre in pixels (row, column), anywhere, also outside the frame
 *   stokes      fp32 [3, n_planes, height, width] or NULL    I, Q, U in the image frame (Q > 0: along the columns' axis)
 *   tb, pb      fp32 [n_planes, height, width], written      every element
 *   pb_cross, chi2, sigma_tb, sigma_pb   fp32 like tb, or NULL
 *   status      uint8 [n_planes, height, width] or NULL
 *   counts      int64 [n_planes, SUNERF_POLARIMETRY_COUNTS] or NULL, written (zeroed by the call, then integer adds)
 *
 * The model of a sample is y_k = g_k0 I + g_k1 Q + g_k2 U with, formed on the host,
 *   g_k0 = 0.5 * t_k,   h = g_k0 * e_k,   g_k1 = h * cos2_k,   g_k2 = h * sin2_k.
 * Pixels are independent.  Sample k of pixel (c, row, col) is y = (double) frames[k, c, row, col]; it is valid when y is finite, bad
 * is NULL or 0 there and, with a noise model, v = a[c] + b[c] * (y > 0 ? y : 0) satisfies 0 < v < inf; its weight is w = 1 / v
 * (1 without a noise model).  Over the valid samples in ascending k, every sum starting from 0.0:
 *   p_i = w * g_ki (i = 0, 1, 2);   m00 += p_0 * g_k0;  m01 += p_0 * g_k1;  m02 += p_0 * g_k2;  m11 += p_1 * g_k1;  m12 += p_1 * g_k2;
 *   m22 += p_2 * g_k2;   r_i += p_i * y.
 * The solve is LDL^T without pivoting, eps = 2^-40:
 *   d0 = m00;                               UNDETERMINED unless d0 > eps * m00 (that is, unless m00 > 0)
 *   l10 = m01 / d0;   l20 = m02 / d0;
 *   d1 = m11 - l10 * m01;                   UNDETERMINED unless d1 > eps * m11
 *   t21 = m12 - l20 * m01;   l21 = t21 / d1;
 *   d2 = (m22 - l20 * m02) - l21 * t21;     UNDETERMINED unless d2 > eps * m22
 *   z0 = r_0;   z1 = r_1 - l10 * z0;   z2 = (r_2 - l20 * z0) - l21 * z1;
 *   U = z2 / d2;   Q = z1 / d1 - l21 * U;   I = (z0 / d0 - l10 * Q) - l20 * U.
 * A pixel with fewer than 3 valid samples is UNDETERMINED before any of this ("unless x > y" is also what a NaN fails).
 *   chi2 = sum over the valid samples in ascending k of (w * e) * e,  e = y - ((g_k0 * I + g_k1 * Q) + g_k2 * U).
 * The rotation into the tangential / radial frame of the Sun, dx = (double) col - cx, dy = (double) row - cy:
 *   n = dx * dx + dy * dy;   C2 = (dx * dx - dy * dy) / n;   S2 = (2 * (dx * dy)) / n;
 *   tb = I;   pb = -(Q * C2 + U * S2);   pb_cross = Q * S2 - U * C2;             n == 0: CENTRE.
 * With a noise model the covariance of (I, Q, U) is the inverse of the normal matrix, taken from the factors:
 *   g = l10 * l21 - l20;   c22 = 1 / d2;   c12 = -l21 / d2;   c11 = 1 / d1 + (l21 * l21) / d2;
 *   c00 = (1 / d0 + (l10 * l10) / d1) + (g * g) / d2;
 *   sigma_tb = sqrt(c00);   sigma_pb = sqrt((c11 * (C2 * C2) + 2 * (c12 * (C2 * S2))) + c22 * (S2 * S2)).
 * Without one both are NaN.  An UNDETERMINED pixel has NaN in every image output.  status is UNDETERMINED, else CENTRE, else
 * DETERMINED, and counts[c] = the pixels of plane c with each of the three, and those with at least one sample that is not valid.
 *
 * Checked in this order: n_frames above SUNERF_POLARIMETRY_MAX_FRAMES: UNSUPPORTED; n_planes, height or width 0 while no count is
 * negative and n_frames >= SUNERF_POLARIMETRY_MIN_FRAMES: 0, nothing read or written; a negative count, n_frames below
 * SUNERF_POLARIMETRY_MIN_FRAMES, cy or cx not finite, a NULL frames, cos2, sin2, throughput, efficiency, tb or pb, one of a and b
 * NULL and the other not, a cos2 or sin2 that is not finite, a throughput or efficiency that is not a finite number above 0, an a,
 * b or counts not aligned to 8 bytes, an image output or status that overlaps frames or bad: BADARG.  That the outputs do not
 * overlap each other, a, b or counts is the caller's to see to. */
int sunerf_polarimetry_stokes(const float* frames, const uint8_t* bad, const double* cos2, const double* sin2, const double* throughput,
                              const double* efficiency, const double* a, const double* b, int n_frames, int n_planes, int height,
                              int width, double cy, double cx, float* stokes, float* tb, float* pb, float* pb_cross, float* chi2,
                              float* sigma_tb, float* sigma_pb, uint8_t* status, int64_t* counts, void* stream);

/* Below this impact parameter, in solar radii, the ratio I_P / I_tot of one electron is not monotone along the line of sight (it
 * rises first from the plane of the sky: 1.247 at u = 0, less for u > 0), and the ratio has two roots on either side. */
#define SUNERF_POLARIMETRY_MIN_IMPACT 1.25
#define SUNERF_POLARIMETRY_STEPS 64 /* bisection steps, always all of them */

/* status of a ray (uint8) */
#define SUNERF_POLARIMETRY_OK 0
#define SUNERF_POLARIMETRY_ABOVE 1      /* ratio above f(0): x = 0 (noise does this) */
#define SUNERF_POLARIMETRY_BELOW 2      /* ratio below f(x_max), negative pb included: x = x_max */
#define SUNERF_POLARIMETRY_CLOSE 3      /* impact parameter below SUNERF_POLARIMETRY_MIN_IMPACT solar radii, the disc included */
#define SUNERF_POLARIMETRY_DEGENERATE 4 /* d = 0, or an o or d that is not finite */
#define SUNERF_POLARIMETRY_INVALID 5    /* tb or pb not finite, or tb <= 0 */

/* One call, one kernel, one lane per ray: the distance x >= 0 from the point of the ray closest to the Sun at which ONE electron
 * scatters light with the polarisation ratio pb / tb.
 *
 *   tb, pb                fp32 [n]
 *   rays_o, rays_d        fp32 [n, 3]     x(z) = o + d z, as the render kernels take them
 *   solar_radius          fp32 [1]        R, in the rays' length unit; the buffers sunerf_thomson_integral_fwd reads
 *   limb_darkening_coeff  fp32 [1]        u
 *   x_max_factor          the bracket is [0, x_max_factor * b], b the ray's impact parameter
 *   depth, status         fp32, uint8 [n], written
 *   z_front, z_back, radius, slope   fp32 [n] or NULL
 *
 * Per ray, with o, d, tb, pb converted to double:
 *   l2 = (dx * dx + dy * dy) + dz * dz;   l = sqrt(l2);   z0 = -((ox * dx + oy * dy) + oz * dz) / l2;
 *   (cx, cy, cz) = o x d;   b2 = ((cx * cx + cy * cy) + cz * cz) / l2;   b = sqrt(b2)          (the p2 of sunerf_thomson_integral_fwd)
 *   f(x) = I_P / I_tot of csrc/thomson_math.h at r2 = b2 + x * x, r = sqrt(r2), p2 = b2 -- the text the Thomson integral evaluates.
 * Status, the first that applies: INVALID (tb or pb not finite, or not tb > 0); DEGENERATE (l2, z0 or b2 not finite, or not l2 > 0);
 * CLOSE (not b >= SUNERF_POLARIMETRY_MIN_IMPACT * R, or not R > 0): every output NaN for these three.  Else with q = pb / tb and
 * x_max = x_max_factor * b: ABOVE when q > f(0), x = 0; BELOW when q < f(x_max), x = x_max; else OK: lo = 0, hi = x_max and
 * SUNERF_POLARIMETRY_STEPS times m = 0.5 * (lo + hi), then lo = m when f(m) > q, else hi = m; x = 0.5 * (lo + hi).
 *   depth = x;   z_front = z0 - x / l;   z_back = z0 + x / l;   radius = sqrt(b2 + x * x);
 *   h = b / 4096;   slope = x < h ? (f(x + h) - f(x)) / h : (f(x + h) - f(x - h)) / (2 * h).
 *
 * Checked in this order: n below 0: BADARG; n == 0: 0, nothing read or written; x_max_factor that is not a finite number above 0, a
 * NULL tb, pb, rays_o, rays_d, solar_radius, limb_darkening_coeff, depth or status: BADARG. */
int sunerf_polarimetry_ratio_depth(const float* tb, const float* pb, const float* rays_o, const float* rays_d, const float* solar_radius,
                                   const float* limb_darkening_coeff, int64_t n, double x_max_factor, float* depth, float* z_front,
                                   float* z_back, float* radius, float* slope, uint8_t* status, void* stream);

#ifdef __cplusplus
}
#endif
#endif
