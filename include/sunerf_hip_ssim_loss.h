/* Structural-loss entry points of libsunerf_hip.so: D-SSIM of a batch of detector-pixel patches with its gradient, the term that
 * stands beside the pixel loss of a patch batch.  An eighth table beside sunerf_hip.h, sunerf_hip_ext.h, sunerf_hip_response.h,
 * sunerf_hip_prep.h, sunerf_hip_instrument.h, sunerf_hip_patch.h and sunerf_hip_likelihood.h, which stay as they are and keep
 * their versions; the same library holds all eight.  Same conventions as sunerf_hip_likelihood.h: row-major device tensors,
 * `stream` a hipStream_t (NULL: the default stream) and the last argument, status 0 on success, SUNERF_E_BADARG (-1),
 * SUNERF_E_UNSUPPORTED (-2), SUNERF_E_WORKSPACE (-3) or a positive hipError_t; argument errors are found before anything touches
 * a device.  The Python binding is sunerf_hip/lib.py: _SSIM_LOSS_SIGNATURES; the host side is sunerf_hip/ssim_loss.py.  DESIGN.md
 * section 8r.
 *
 * No floating-point atomics anywhere: reruns are bit-identical.  All arithmetic is IEEE fp64 with every operation rounded on its
 * own (no fused multiply-add); the fp32 gradients are rounded once, at the store. */
#ifndef SUNERF_HIP_SSIM_LOSS_H
#define SUNERF_HIP_SSIM_LOSS_H

#include "sunerf_hip_likelihood.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Version of THIS table; sunerf_hip/lib.py refuses a library that answers anything else. */
#define SUNERF_SSIM_LOSS_ABI_VERSION 1
int sunerf_ssim_loss_abi_version(void);

#define SUNERF_SSIM_LOSS_MAX_PATCH 64        /* P: the side of a patch in detector pixels     */
#define SUNERF_SSIM_LOSS_MIN_WINDOW 3        /* w: odd, 3 .. 11                               */
#define SUNERF_SSIM_LOSS_MAX_WINDOW 11
#define SUNERF_SSIM_LOSS_MAX_CHANNELS 64     /* C                                             */

/* Bytes of the reduction workspace for n patches of C channels: a ticket line of 64 bytes and 4 fp64 words per patch and
 * channel.  0 for n below 1, C outside [1, 64] or a size that does not fit.  ZERO-INITIALISED once by the caller (the kernel leaves
 * its ticket zeroed and needs nothing else of what the workspace held); one workspace serves one stream. */
size_t sunerf_ssim_loss_workspace_bytes(int64_t n, int C);

/* D-SSIM of the coarse and of the fine image of a patch batch against the target, and both gradients, in one launch.
 *
 *   coarse, fine, target  fp32 [n P P, C], channel last: element (k, r, q, c) at ((k P + r) P + q) C + c -- the rows a patch
 *                         batch's pixel loss receives; no permuted copy is made on the way in or out
 *   window      w, odd, 3 .. 11, w <= P <= 64; N = w^2
 *   data_range  R > 0, finite: C1 = (0.01 R)^2, C2 = (0.03 R)^2
 *   use_asinh   not 0: both images pass s(v) = asinh(v / vmax / a) / asinh(1 / a) first (fp64), R then refers to s(v)
 *
 * A PLANE is one channel of one patch of one of the two images, together with the same channel of the target: 2 P^2 values;
 * there are 2 n C planes.  Per plane and per fully inside window (there are (P - w + 1)^2), with sums over the window's N pixels:
 *   mu_x = sum x / N, mu_y = sum y / N, var_x = (sum x^2 - N mu_x^2) / (N - 1), var_y alike, cov = (sum x y - N mu_x mu_y) / (N - 1)
 *   A1 = 2 mu_x mu_y + C1, A2 = 2 cov + C2, B1 = mu_x^2 + mu_y^2 + C1, B2 = var_x + var_y + C2, S = A1 A2 / (B1 B2)
 * ssim(plane) is the mean of S over the windows: skimage.metrics.structural_similarity(y, x, win_size=w, data_range=R) of the
 * patch.  A plane is VALID when all its 2 P^2 values are finite; an invalid plane adds nothing and its gradient is 0.
 * dssim(image) = 1 - the mean of ssim over the image's valid planes, 0 when it has none.
 *
 *   g_coarse, g_fine  fp32 [n P P, C]: d ssim(plane) / d x of every pixel (NOT negated, NOT divided by the number of valid
 *                     planes: d dssim / d x = -g / (the image's number of valid planes)), every element written
 *   plane_ssim        fp64 [2, n, C]: ssim of the coarse planes, then of the fine planes; NaN for an invalid plane
 *   stats             fp64 [4]: dssim(coarse), dssim(fine), the number of valid planes and the number of invalid planes, both
 *                     counted over the 2 n C planes of the two images: a channel whose fine values hold a NaN while its coarse
 *                     and target values are finite is one valid and one invalid plane; a non-finite target makes two invalid
 *
 * A plane's ssim and gradient do not depend on the batch it is in or on its place there.  The sums of stats are taken in one
 * fixed order (per workgroup in channel order, the workgroups' partials in index order by the workgroup that takes the last
 * ticket).
 *
 * Checked in this order: window even or outside 3 .. 11, P below window or above 64, C outside 1 .. 64, data_range not > 0 or not
 * finite, use_asinh with a vmax or a that is not > 0 and finite: UNSUPPORTED; n == 0: 0, nothing read or written; n below 0, a
 * NULL among the three inputs, the four outputs and the workspace, a plane_ssim, stats or workspace not aligned to 8 bytes:
 * BADARG; workspace_bytes below the query's answer: WORKSPACE. */
int sunerf_ssim_loss(const float* coarse, const float* fine, const float* target, int64_t n, int P, int C, int window,
                     double data_range, double vmax, double a, int use_asinh, float* g_coarse, float* g_fine,
                     double* plane_ssim, double* stats, void* workspace, size_t workspace_bytes, void* stream);

#ifdef __cplusplus
}
#endif
#endif
