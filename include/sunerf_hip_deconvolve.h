/* Deconvolution entry points of libsunerf_hip.so: Richardson-Lucy against the PSF-and-bin kernel of sunerf_hip_instrument.h -- the
 * classical way from a detector image back to the frame it was observed from, the baseline beside training through the
 * instrument.  A ninth table beside sunerf_hip.h, sunerf_hip_ext.h, sunerf_hip_response.h, sunerf_hip_prep.h,
 * sunerf_hip_instrument.h, sunerf_hip_patch.h, sunerf_hip_likelihood.h and sunerf_hip_ssim_loss.h, which stay as they are and keep
 * their versions; the same library holds all nine.  Same conventions as sunerf_hip_patch.h: row-major device tensors, `stream` a
 * hipStream_t (NULL: the default stream) and the last argument, status 0 on success, SUNERF_E_BADARG (-1), SUNERF_E_UNSUPPORTED
 * (-2) or a positive hipError_t; argument errors are found before anything touches a device.  The Python binding is
 * sunerf_hip/lib.py: _DECONVOLVE_SIGNATURES; the host side is sunerf_hip/deconvolve.py.  DESIGN.md section 8s.
 *
 * No floating-point atomics anywhere: reruns are bit-identical, and a plane alone gives the bits it gives inside a batch of
 * planes.  All arithmetic is IEEE fp64 with every operation rounded on its own (no fused multiply-add), in the order written. */
#ifndef SUNERF_HIP_DECONVOLVE_H
#define SUNERF_HIP_DECONVOLVE_H

#include "sunerf_hip_patch.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Version of THIS table; sunerf_hip/lib.py refuses a library that answers anything else. */
#define SUNERF_DECONVOLVE_ABI_VERSION 1
int sunerf_deconvolve_abi_version(void);

#define SUNERF_DECONVOLVE_MAX_ITERATIONS 10000
#define SUNERF_DECONVOLVE_STATE 4 /* doubles per plane: deviance, n_valid, iterations_applied, stopped */

/* Bytes of the reduction workspace: one (deviance, n_valid) pair of fp64 per tile of the forward correlation, n_planes times
 * ceil((height / bin) / T) * ceil((width / bin) / T) pairs with T the tile of sunerf_hip_instrument.h for (kh, kw, bin).  0 for
 * a count below 1 or a kernel or bin outside the limits.  Nothing of what the workspace held is read; one workspace serves one
 * stream. */
size_t sunerf_deconvolve_workspace_bytes(int n_planes, int height, int width, int kh, int kw, int bin);

/* Shifted-Poisson Richardson-Lucy (Snyder et al. 1993: the EM iteration for Poisson counts plus Gaussian read noise), up to
 * n_iterations updates of u in place, all enqueued by this one call: the host does not wait between iterations.
 *
 *   u       fp32 [n_planes, height, width]             the latent image, image units: the start on entry, the iterate on return
 *   d       fp32 [n_planes, height / bin, width / bin] the detector image, image units
 *   bad     uint8, shape of d, or NULL                 not 0: the pixel takes no part
 *   norm    fp32, shape of u                           A^T of (valid as 1.0f / 0.0f): sunerf_patch_correlate_bin_adjoint of the mask
 *   params  fp64 [n_planes, 2] = c, v                  photons per image unit; read variance in photons^2
 *   K, n_kernels, kh, kw, bin, anchor_y, anchor_x, scale, boundary: the operator A of sunerf_instrument_correlate_bin, same limits
 *   ratio   fp32, shape of d                           scratch, every element written (the ratio of the last pass that ran)
 *   state   fp64 [n_planes, 4], written                deviance, n_valid, iterations_applied, stopped (0.0 or 1.0)
 *
 * Per plane, off = v / c.  A PASS computes, per detector pixel (R, C),
 *   valid = isfinite(d) && !(bad != NULL && bad[R, C])
 *   e     = scale * acc          acc: the fp64 sum of sunerf_instrument_correlate_bin over u, in that header's order (the first
 *                                product starts the sum), NOT rounded to fp32
 *   den   = e + off
 *   num   = valid ? (double) d + off : 0;   num = num > 0 ? num : 0
 *   ratio = (valid && den > 0) ? num / den : 0, rounded to fp32
 *   term  = (valid && den > 0) ? 2 * ((L - N) + (N > 0 ? N * log(N / L) : 0)) : 0   with L = c * den, N = c * num
 * and the plane's deviance = the sum of the terms, n_valid = the number of valid pixels.  The terms are added in ONE order that
 * depends on the plane's shape and on (kh, kw, bin) alone: inside a tile of T x T detector pixels of 256 threads, a thread's
 * pixels (t, t + 256, ... of the tile, row-major) ascending, the 64 threads of a wave by a butterfly (distance 32, 16, ... 1),
 * the four waves ascending; then the plane's tiles: 256 chains take the tiles q, q + 256, ... (row-major) ascending and are
 * folded in halves (chain q takes chain q + 128, then q + 64, ... 1).  log is the device's fp64 function.
 * If stop > 0 and deviance <= stop * n_valid the plane is STOPPED: stopped = 1, and no later pass or update touches the plane's u
 * or state -- they are those of the iterate whose deviance is reported.
 * An UPDATE follows every pass but the last, for the planes that are not stopped; it counts in iterations_applied:
 *   t  = scale * acc_adj         acc_adj: the fp64 sum of sunerf_patch_correlate_bin_adjoint over the fp32 ratio, in that
 *                                header's order
 *   u' = norm > 0 ? (float) (((double) u * t) / (double) norm) : u
 * The call runs n_iterations + 1 passes and up to n_iterations updates: the last pass describes the last iterate.
 * n_iterations == 0 is one pass and no update: u keeps its bits and state describes u as given.  With K >= 0 and u > 0 on
 * entry every iterate is >= 0.  Where norm is 0 (no valid detector pixel reads the pixel) u keeps its bits.
 *
 * Checked in this order (the instrument table's): kh or kw above 96, bin above 8, a boundary other than the two: UNSUPPORTED;
 * n_planes, height / bin or width / bin 0 while no count is negative and kh, kw, bin >= 1: 0, nothing read or written; a negative
 * count, kh, kw or bin below 1, n_kernels neither 1 nor n_planes, an anchor outside [0, kh) x [0, kw), n_iterations outside
 * [0, SUNERF_DECONVOLVE_MAX_ITERATIONS], a stop that is NaN or negative, a NULL u, d, norm, params, K, ratio, state or workspace
 * (the workspace's size is never 0 here), a params, K, state or workspace not aligned to 8 bytes: BADARG. */
int sunerf_deconvolve_richardson_lucy(float* u, const float* d, const uint8_t* bad, const float* norm, const double* params,
                                      int n_planes, int height, int width, const double* K, int n_kernels, int kh, int kw, int bin,
                                      int anchor_y, int anchor_x, double scale, int boundary, int n_iterations, double stop,
                                      float* ratio, double* state, void* workspace, void* stream);

#ifdef __cplusplus
}
#endif
#endif
