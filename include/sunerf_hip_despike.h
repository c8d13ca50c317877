/* Despiking entry points of libsunerf_hip.so: cosmic-ray hits and hot pixels found by an iterated, masked sliding-window median
 * test and replaced by the median of their clean neighbours -- the step in front of sunerf_hip_prep.h, whose spline prefilter
 * spreads a hit over its neighbourhood, and of sunerf_hip_deconvolve.h, which sharpens one into a point source.  An eleventh
 * table beside sunerf_hip.h, sunerf_hip_ext.h, sunerf_hip_response.h, sunerf_hip_prep.h, sunerf_hip_instrument.h,
 * sunerf_hip_patch.h, sunerf_hip_likelihood.h, sunerf_hip_ssim_loss.h, sunerf_hip_deconvolve.h and sunerf_hip_psf_grad.h, which stay
 * as they are and keep their versions; the same library holds all eleven.  Same conventions as sunerf_hip_deconvolve.h: row-major
 * device tensors, `stream` a hipStream_t (NULL: the default stream) and the last argument, status 0 on success, SUNERF_E_BADARG
 * (-1), SUNERF_E_UNSUPPORTED (-2) or a positive hipError_t; argument errors are found before anything touches a device.  The Python
 * binding is sunerf_hip/lib.py: _DESPIKE_SIGNATURES; the host side is sunerf_hip/despike.py.  DESIGN.md section 8v.
 *
 * No floating-point atomics anywhere and no sum of floating-point numbers across threads: reruns are bit-identical, and a plane
 * alone gives the bits it gives inside a batch of planes.  The decision arithmetic is IEEE fp64 with every operation rounded on its
 * own (no fused multiply-add), in the order written, and uses + - * max and comparisons only. */
#ifndef SUNERF_HIP_DESPIKE_H
#define SUNERF_HIP_DESPIKE_H

#include "sunerf_hip_patch.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Version of THIS table; sunerf_hip/lib.py refuses a library that answers anything else. */
#define SUNERF_DESPIKE_ABI_VERSION 1
int sunerf_despike_abi_version(void);

#define SUNERF_DESPIKE_MAX_RADIUS 3      /* windows of 3 x 3, 5 x 5 and 7 x 7 */
#define SUNERF_DESPIKE_MAX_ITERATIONS 64
#define SUNERF_DESPIKE_MAX_MIN_VALID 48  /* the neighbours of the largest window */
#define SUNERF_DESPIKE_STATE 6 /* doubles per plane: n_spike, n_invalid, n_unfilled, passes, converged, 0 */

/* mask bits (uint8) */
#define SUNERF_DESPIKE_SPIKE 1    /* flagged by a detection pass */
#define SUNERF_DESPIKE_INVALID 2  /* non-finite on entry, or the caller's `bad` */
#define SUNERF_DESPIKE_UNFILLED 4 /* flagged, and fewer than min_valid clean neighbours to fill it from: clean is NaN there */

/* mode: the scale of the test */
#define SUNERF_DESPIKE_MODE_MODEL 0 /* var = a + b max(med, 0): the instrument's noise model */
#define SUNERF_DESPIKE_MODE_MAD 1   /* s = max(1.4826 mad, floor): the neighbours' own scatter */

/* flags */
#define SUNERF_DESPIKE_TWO_SIDED 1 /* flag negative outliers too */
#define SUNERF_DESPIKE_FILL_NAN 2  /* flagged pixels become NaN instead of the median */

/* Bytes of the workspace: the second mask buffer (n_planes * height * width bytes, rounded up to a multiple of 8) and
 * SUNERF_DESPIKE_MAX_ITERATIONS + 2 counters of 4 bytes per plane.  0 for a count below 1 or a radius outside
 * [1, SUNERF_DESPIKE_MAX_RADIUS].  Nothing of what the workspace held is read; one workspace serves one stream. */
size_t sunerf_despike_workspace_bytes(int n_planes, int height, int width, int radius);

/* Up to max_iterations detection passes and one fill, all enqueued by this one call: the host does not wait between passes, and a
 * plane stops on the device at its first pass that flags nothing.
 *
 *   image   fp32 [n_planes, height, width]          the observed planes; may hold NaN and +-inf
 *   bad     uint8, shape of image, or NULL          not 0: the pixel is INVALID from the start
 *   params  fp64 [n_planes, 4] = a, b, floor, 0     a, b >= 0: variance = a + b * signal (MODEL); floor: the least scale (MAD)
 *   clean   fp32, shape of image, written           every element; may not overlap image
 *   mask    uint8, shape of image, written          every element: the SUNERF_DESPIKE_* bits
 *   state   fp64 [n_planes, SUNERF_DESPIKE_STATE], written: n_spike, n_invalid, n_unfilled (pixels that carry the bit), passes
 *           (the detection passes that flagged something), converged (1.0: a pass flagged nothing), 0.0
 *   workspace  sunerf_despike_workspace_bytes(n_planes, height, width, radius) bytes
 *
 * Planes are independent.  Mask 0 holds INVALID where image is not finite or bad is not 0.  N(p) of a pixel p under a mask: the
 * pixels of the (2 radius + 1)^2 window around p that lie inside the frame (nothing is padded), are not p, and carry no bit in
 * that mask; n = |N(p)|.  med(p) = 0.5 * ((double) lo + (double) hi) with lo, hi the order statistics of ranks (n - 1) / 2 and
 * n / 2 (integer division, rank 0 the smallest) of the values of N(p).  mad(p) = the same rule over |(double) v - med(p)|, v in
 * N(p), in fp64.  With x = (double) image[p] and d = x - med(p),
 *   MODEL:  var = a + b * (med > 0 ? med : 0);   hit = d > 0 && d * d > (t * t) * var      TWO_SIDED: d != 0 && d * d > (t * t) * var
 *   MAD:    s = 1.4826 * mad;  s = s > floor ? s : floor;   hit = d > t * s                TWO_SIDED: |d| > t * s
 * with t = grow_sigma if one of the 8 neighbours of p inside the frame carries SPIKE in the mask read, else n_sigma.
 * Detection pass k (k = 0 ...) reads mask k and writes mask k + 1 = mask k plus SPIKE on every p that carries no bit in mask k,
 * has n >= min_valid and is a hit.  A plane's passes end after the first that adds nothing, or after max_iterations.
 * The fill reads the last mask; neighbours are always values of image, never filled ones.  A pixel without a bit: clean = image,
 * bit for bit.  A pixel with SPIKE or INVALID: clean = (float) med(p) if n >= min_valid, else NaN and UNFILLED is added to its
 * mask; under FILL_NAN clean = NaN and UNFILLED is never set.  max_iterations == 0 is the fill alone.
 *
 * Checked in this order: radius above SUNERF_DESPIKE_MAX_RADIUS, max_iterations above SUNERF_DESPIKE_MAX_ITERATIONS, min_valid above
 * SUNERF_DESPIKE_MAX_MIN_VALID, a mode other than the two, a flag bit other than the two: UNSUPPORTED; n_planes, height or width 0
 * while no count is negative and radius >= 1: 0, nothing read or written; a negative count, radius, min_valid below 1,
 * max_iterations below 0, n_sigma or grow_sigma that is not a finite number above 0, a NULL image, params, clean, mask, state or
 * workspace (the workspace's size is never 0 here), a params, state or workspace not aligned to 8 bytes, a clean that overlaps
 * image: BADARG. */
int sunerf_despike(const float* image, const uint8_t* bad, const double* params, int n_planes, int height, int width, int radius,
                   int mode, int flags, double n_sigma, double grow_sigma, int min_valid, int max_iterations, float* clean,
                   uint8_t* mask, double* state, void* workspace, void* stream);

#ifdef __cplusplus
}
#endif
#endif
