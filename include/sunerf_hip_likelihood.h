/* Likelihood entry points of libsunerf_hip.so: the Gaussian noise likelihood of the detector model of sunerf_hip_instrument.h as
 * the training loss, with one trainable calibration gain per table row.  A seventh table beside sunerf_hip.h, sunerf_hip_ext.h,
 * sunerf_hip_response.h, sunerf_hip_prep.h, sunerf_hip_instrument.h and sunerf_hip_patch.h, which stay as they are and keep their
 * versions; the same library holds all seven.  Same conventions as sunerf_hip_patch.h: row-major device tensors, `stream` a
 * hipStream_t (NULL: the default stream) and the last argument, status 0 on success, SUNERF_E_BADARG (-1), SUNERF_E_UNSUPPORTED
 * (-2), SUNERF_E_WORKSPACE (-3) or a positive hipError_t; argument errors are found before anything touches a device.  The Python
 * binding is sunerf_hip/lib.py: _LIKELIHOOD_SIGNATURES; the host side is sunerf_hip/likelihood.py.  DESIGN.md section 8q.
 *
 * No floating-point atomics anywhere: reruns are bit-identical.  All arithmetic is IEEE fp64 with every operation rounded on its
 * own (no fused multiply-add); fp32 outputs are rounded once, at the store. */
#ifndef SUNERF_HIP_LIKELIHOOD_H
#define SUNERF_HIP_LIKELIHOOD_H

#include "sunerf_hip_instrument.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Version of THIS table; sunerf_hip/lib.py refuses a library that answers anything else. */
#define SUNERF_LIKELIHOOD_ABI_VERSION 1
int sunerf_likelihood_abi_version(void);

#define SUNERF_LIKELIHOOD_MAX_ROWS 64            /* rows of the table: the channels of a response set                  */
#define SUNERF_LIKELIHOOD_MAX_FINITE_CHECK 8     /* further tensors that only take part in the NaN / Inf count         */
#define SUNERF_LIKELIHOOD_OBSERVED 0             /* variance from the target: the classical chi-square, fixed weights  */
#define SUNERF_LIKELIHOOD_MODEL 1                /* variance from the prediction: the Gaussian negative log-likelihood */

/* Bytes of the reduction workspace for a table of n_rows rows: a ticket and 128 block partials of 5 n_rows + 3 fp64 words.
 * 0 for n_rows outside [1, SUNERF_LIKELIHOOD_MAX_ROWS].  ZERO-INITIALISED once by the caller (the kernel leaves its ticket
 * zeroed and needs nothing else of what the workspace held); one workspace serves one stream. */
size_t sunerf_likelihood_workspace_bytes(int n_rows);

/* Replaces the loss section of the reference's training steps, sunerf/model/sunerf.py:105-125 (EmissionSuNeRFModule: finite
 * asserts, 2 x MSE of the asinh-scaled images, regularization.mean(), psnr) and sunerf/model/sunerf.py:187-191
 * (DensityTemperatureSuNeRFModule: the same with a plain MSE), by the negative log-likelihood the detector model implies.
 *
 *   coarse_image, fine_image, target_image  fp32 [n_rays, n_columns]: the slots
 *   codes       fp32 [n_rays, n_columns], or NULL: every slot is row 0 (one channel)
 *   row_codes   fp32 [n_rows]: the code of every table row (positive, exact in fp32, no two alike)
 *   noise       fp64 [n_rows, 8]: unit U, exposure E, dn_per_photon G, read_noise R, extra_var, floor, 0, 0 per row -- the first
 *               four as the instrument's noise kernel takes them; extra_var a variance in DN^2 (1 / 12 for a quantising
 *               detector), floor a standard deviation in image units
 *   log_gain    fp32 [n_rows]
 *   regularization  fp32 [n_reg] (n_reg may be 0, the pointer then NULL)
 *   finite_check_host[n_finite_check <= 8]  HOST arrays of further device tensors and their sizes: counted, nothing else
 *
 * Per slot, with r the row whose code the slot carries, g = exp(log_gain[r]), p the prediction (coarse or fine), t the target,
 *   m = g p,   var(x) = (max(x, 0) U E G + R^2 + extra_var) / (U E)^2      [sqrt(var(t)) is Instrument.errors(t)]
 *   mode OBSERVED:  s2 = var(t) + floor^2,  term = (m - t)^2 / s2
 *   mode MODEL:     s2 = var(m) + floor^2,  term = (m - t)^2 / s2 + ln s2;  d s2 / d m = G / (U E) where m > 0, else 0
 * A slot is MASKED -- it adds nothing and its gradient is 0 -- when its code is not > 0 (NaN included), when its target is not
 * finite, or when its positive code is no row of the table; the last kind is counted in stats[7], whatever its target holds.  A
 * non-finite coarse or fine value at an unmasked slot is counted in stats[5] (and reaches the sums by IEEE rules), as are
 * non-finite elements of regularization and of the finite_check tensors.
 *
 *   g_coarse, g_fine  fp32 [n_rays, n_columns]: d term / d p = (d term / d m) g, every element written, NOT divided by the
 *                     number of valid slots: the caller multiplies by lambda_image / n_valid (stats[6], on the device)
 *   g_log_gain        fp64 [n_rows]: sum over the row's valid slots of (d term_c / d m_c) m_c + (d term_f / d m_f) m_f
 *   channel_stats     fp64 [n_rows, 4]: valid slots, sum of coarse terms, sum of fine terms, sum of (g fine - t)^2
 *   stats             fp32 [8]: [0] lambda_image (mean_valid(term_c) + mean_valid(term_f)) + lambda_regularization mean(reg),
 *                     [1] the coarse mean, [2] the fine mean, [3] mean(reg), [4] -10 log10 of the mean over valid slots of
 *                     (g fine - t)^2, [5] the non-finite count, [6] n_valid, [7] the unknown-code count
 * With no valid slot the means and stats[4] are 0, the loss is lambda_regularization mean(reg) and every gradient is 0.
 * Sums are taken per row in a fixed order (workgroup partials added in workgroup order) and over the rows in row order.
 *
 * Checked in this order: n_rows above 64, n_finite_check above 8, a mode other than the two: UNSUPPORTED; n_rays or n_columns 0
 * while neither is negative, n_rows >= 1, n_reg >= 0 and n_finite_check >= 0: 0, nothing read or written; n_rays, n_columns or
 * n_rows below 1, a negative n_reg or n_finite_check, n_rays n_columns above 2^63 - 1, a NULL among coarse_image, fine_image,
 * target_image, row_codes, noise, log_gain, g_coarse, g_fine, g_log_gain, channel_stats, stats and workspace, a NULL
 * regularization with n_reg > 0, a noise, g_log_gain, channel_stats or workspace not aligned to 8 bytes, a NULL or negative
 * entry of the finite-check lists: BADARG; workspace_bytes below the query's answer: WORKSPACE. */
int sunerf_likelihood_loss(const float* coarse_image, const float* fine_image, const float* target_image, const float* codes,
                           int64_t n_rays, int n_columns, const float* row_codes, const double* noise, const float* log_gain,
                           int n_rows, int mode, const float* regularization, int64_t n_reg,
                           const float* const* finite_check_host, const int64_t* finite_check_sizes_host, int n_finite_check,
                           float lambda_image, float lambda_regularization, float* g_coarse, float* g_fine, double* g_log_gain,
                           double* channel_stats, float* stats, void* workspace, size_t workspace_bytes, void* stream);

#ifdef __cplusplus
}
#endif
#endif
