/* Stacking entry points of libsunerf_hip.so: a per-pixel statistic over a stack of up to 64 frames of one detector -- an order
 * statistic (median, percentile, rank) or the mean, after an optional iterated clipping of outliers against the pixel's own
 * median.  The reduction behind sunerf_hip/stack.py: multi-frame rejection of cosmic-ray hits, the low-percentile background of a
 * coronagraph sequence, the robust stack of a burst.  A thirteenth table beside sunerf_hip.h, sunerf_hip_ext.h,
 * sunerf_hip_response.h, sunerf_hip_prep.h, sunerf_hip_instrument.h, sunerf_hip_patch.h, sunerf_hip_likelihood.h,
 * sunerf_hip_ssim_loss.h, sunerf_hip_deconvolve.h, sunerf_hip_psf_grad.h, sunerf_hip_despike.h and sunerf_hip_coalign.h, which stay
 * as they are and keep their versions; the same library holds all thirteen.  Same conventions as sunerf_hip_coalign.h: row-major
 * device tensors, `stream` a hipStream_t (NULL: the default stream) and the last argument, status 0 on success, SUNERF_E_BADARG
 * (-1), SUNERF_E_UNSUPPORTED (-2) or a positive hipError_t; argument errors are found before anything touches a device.  The Python
 * binding is sunerf_hip/lib.py: _STACK_SIGNATURES; the host side is sunerf_hip/stack.py.  DESIGN.md section 8y.
 *
 * No floating-point atomics anywhere and no sum of floating-point numbers across threads: reruns are bit-identical, and a pixel
 * alone gives the bits it gives inside a frame.  All arithmetic is IEEE fp64 on (double) v with every operation rounded on its own
 * (no fused multiply-add), in the order written; the result is rounded to fp32 once.  There is no workspace. */
#ifndef SUNERF_HIP_STACK_H
#define SUNERF_HIP_STACK_H

#include "sunerf_hip_patch.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Version of THIS table; sunerf_hip/lib.py refuses a library that answers anything else. */
#define SUNERF_STACK_ABI_VERSION 1
int sunerf_stack_abi_version(void);

#define SUNERF_STACK_MAX_FRAMES 64
#define SUNERF_STACK_MAX_ITERATIONS 16
#define SUNERF_STACK_STATE 4 /* int64 per plane: samples rejected, samples invalid, pixels with a NaN result, passes */

/* mask values (uint8): 0 for a survivor */
#define SUNERF_STACK_REJECTED 1 /* valid, and outside the interval the clipping left */
#define SUNERF_STACK_INVALID 2  /* not finite, or the caller's `bad` */

/* method: the statistic over the survivors */
#define SUNERF_STACK_MEAN 0
#define SUNERF_STACK_MEDIAN 1
#define SUNERF_STACK_PERCENTILE 2 /* of q in [0, 100], linear between the two neighbouring order statistics */
#define SUNERF_STACK_RANK 3       /* the order statistic `rank`: 0 the smallest, -1 the largest */

/* mode: the scale of the clipping test */
#define SUNERF_STACK_MODE_MODEL 0 /* var = a + b max(m, 0): the instrument's noise model at the median */
#define SUNERF_STACK_MODE_MAD 1   /* s = max(1.4826 MAD, floor): the survivors' own scatter */

/* flags */
#define SUNERF_STACK_TWO_SIDED 1 /* reject negative outliers too */

/* One call, one kernel, one lane per pixel.
 *
 *   frames  fp32 [n_frames, n_planes, height, width]     may hold NaN and +-inf
 *   bad     uint8, shape of frames, or NULL               not 0: the sample is INVALID
 *   params  fp64 [n_planes, 4] = a, b, floor, 0           a, b >= 0: variance = a + b * signal (MODEL); floor: the least scale (MAD)
 *   image   fp32 [n_planes, height, width], written       every element
 *   count   uint8 [n_planes, height, width], written      every element: the survivors n of the pixel
 *   mask    uint8, shape of frames, written, or NULL      every element: 0, SUNERF_STACK_REJECTED or SUNERF_STACK_INVALID
 *   state   int64 [n_planes, SUNERF_STACK_STATE], written  per plane: the samples REJECTED, the samples INVALID, the pixels whose
 *           image is NaN, the largest number of passes over its pixels that rejected something
 *
 * Pixels are independent.  Sample t of pixel (c, y, x) is v_t = frames[t, c, y, x]; it is valid when v_t is finite and bad is NULL
 * or 0 there.  The valid samples sorted ascending by value are the sequence s; the survivors are at every moment a run
 * s_lo .. s_hi-1 of it, at first all of it.  A pass over a pixel with n = hi - lo survivors:
 *   m = 0.5 * ((double) s_[lo + (n - 1) / 2] + (double) s_[lo + n / 2])                       (integer division)
 *   MODEL:  L = (n_sigma * n_sigma) * (a + b * (m > 0 ? m : 0));  with d = (double) v - m a survivor v fails when
 *           d > 0 && d * d > L,   under TWO_SIDED also when d < 0 && d * d > L
 *   MAD:    MAD = 0.5 * (e_[(n - 1) / 2] + e_[n / 2]) with e the values |(double) v - m| of the survivors sorted ascending;
 *           s = 1.4826 * MAD;  s = s > floor ? s : floor;  L = n_sigma * s;  a survivor fails when
 *           d > L,   under TWO_SIDED also when -d > L
 *   Every survivor that fails leaves at once (the tests are monotone in v: those that fail are a tail of the run at either end, and
 *   equal values share one fate).
 * At most `iterations` passes run over a pixel; they end before a pass that would find n < clip_min, and after the first pass in
 * which nothing fails.  The pixel's passes are those in which something failed.
 *
 * The statistic over the n survivors r_i = s_[lo + i], in fp64, then rounded to fp32:
 *   MEAN        ((((double) r_0 + r_1) + r_2) + ... + r_[n-1]) / n                              in that ascending order
 *   MEDIAN      0.5 * ((double) r_[(n - 1) / 2] + (double) r_[n / 2])
 *   PERCENTILE  p = q / 100.0 * (n - 1);  l = floor(p);  l >= n - 1: r_l;  else r_l + (p - l) * ((double) r_[l+1] - (double) r_l)
 *   RANK        rank >= 0: r_[min(rank, n - 1)];  rank < 0: r_[max(n + rank, 0)]
 * and NaN where n < min_valid (min_valid >= 1: a pixel without survivors is always NaN).  count = n.  mask[t] = INVALID for a sample
 * that is not valid, REJECTED for a valid one with v < r_0 or v > r_[n-1] (every valid one when n = 0), else 0.
 *
 * Checked in this order: n_frames above SUNERF_STACK_MAX_FRAMES, iterations above SUNERF_STACK_MAX_ITERATIONS, a method or a mode
 * other than those above, a flag bit other than TWO_SIDED: UNSUPPORTED; n_planes, height or width 0 while no count is negative and
 * n_frames >= 1: 0, nothing read or written; a negative count, n_frames below 1, iterations below 0, clip_min below 2, min_valid
 * below 1, n_sigma that is not a finite number above 0, q that is not in [0, 100] (PERCENTILE only), a NULL frames, params, image,
 * count or state, a params or state not aligned to 8 bytes, an image, count or mask that overlaps frames or bad (the kernel reads
 * both while it writes the three; the samples a second time for the mask): BADARG.  That the outputs do not overlap each other,
 * params or state is the caller's to see to. */
int sunerf_stack_combine(const float* frames, const uint8_t* bad, const double* params, int n_frames, int n_planes, int height,
                         int width, int method, double q, int rank, int mode, int flags, double n_sigma, int iterations, int clip_min,
                         int min_valid, float* image, uint8_t* count, uint8_t* mask, int64_t* state, void* stream);

#ifdef __cplusplus
}
#endif
#endif
