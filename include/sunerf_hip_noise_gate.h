/* Noise-gating entry points of libsunerf_hip.so: an image sequence of one detector is cut into overlapping apodised blocks of
 * bt x 16 x 16 samples (t, y, x), every block is Fourier-transformed, every coefficient that does not stand out of the block's own
 * expected noise power is dropped (or attenuated), and the blocks are transformed back and overlap-added (DeForest 2017).  The
 * kernel behind sunerf_hip/noise_gate.py.  A fourteenth table beside sunerf_hip.h, sunerf_hip_ext.h, sunerf_hip_response.h,
 * sunerf_hip_prep.h, sunerf_hip_instrument.h, sunerf_hip_patch.h, sunerf_hip_likelihood.h, sunerf_hip_ssim_loss.h,
 * sunerf_hip_deconvolve.h, sunerf_hip_psf_grad.h, sunerf_hip_despike.h, sunerf_hip_coalign.h and sunerf_hip_stack.h, which stay as
 * they are and keep their versions; the same library holds all fourteen.  Same conventions as sunerf_hip_stack.h: row-major device
 * tensors, `stream` a hipStream_t (NULL: the default stream) and the last argument, status 0 on success, SUNERF_E_BADARG (-1),
 * SUNERF_E_UNSUPPORTED (-2) or a positive hipError_t; argument errors are found before anything touches a device.  The Python
 * binding is sunerf_hip/lib.py: _NOISE_GATE_SIGNATURES; the host side is sunerf_hip/noise_gate.py.  DESIGN.md section 8z.
 *
 * No floating-point atomics anywhere: the blocks are enqueued as 4 x 4 x 4 (bt = 1: 4 x 4) passes of blocks that do not overlap,
 * in a fixed order on the stream; the first pass stores, the others add.  Reruns are bit-identical and `out` does not depend on
 * what it held.  The transforms are fp32, every operation rounded on its own (no fused multiply-add); the sums that decide (the
 * block's mean, its noise power, |F|^2 against the threshold) are fp64.  There is no workspace. */
#ifndef SUNERF_HIP_NOISE_GATE_H
#define SUNERF_HIP_NOISE_GATE_H

#include "sunerf_hip_patch.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Version of THIS table; sunerf_hip/lib.py refuses a library that answers anything else. */
#define SUNERF_NOISE_GATE_ABI_VERSION 1
int sunerf_noise_gate_abi_version(void);

#define SUNERF_NOISE_GATE_BLOCK 16 /* samples of a block along y and along x */
#define SUNERF_NOISE_GATE_STATE 4  /* int64 per plane: invalid samples, blocks with a valid sample, their non-DC coefficients
                                      with a factor above 0, their non-DC coefficients */

/* mode: the factor of a coefficient k != 0 with power |F_k|^2 under the expected noise power P_k */
#define SUNERF_NOISE_GATE_MODE_GATE 0   /* 1 where |F_k|^2 >= gamma^2 P_k, else 0 */
#define SUNERF_NOISE_GATE_MODE_WIENER 1 /* max(0, 1 - gamma^2 P_k / |F_k|^2), 0 where |F_k| = 0 */

/* flags */
#define SUNERF_NOISE_GATE_FILL_INVALID 1 /* an invalid sample gets the gated estimate instead of NaN */

/* One call, 64 kernels (bt = 1: 16), one workgroup per 16 x 16 x 16 samples: 16 / bt blocks that are neighbours along x.
 *
 *   frames    fp32 [n_frames, n_planes, height, width]      may hold NaN and +-inf
 *   bad       uint8, shape of frames, or NULL                not 0: the sample is invalid
 *   params    fp64 [n_planes, 4] = a, b, 0, 0                a, b >= 0: the variance of a sample I is a + b max(I, 0)
 *   spectrum  fp32 [n_planes, bt, 16, 16] or NULL            S_k >= 0 in DFT layout (k_t, k_y, k_x): P_k = P S_k; NULL: S = 1
 *   out       fp32, shape of frames, written                 every element
 *   state     int64 [n_planes, SUNERF_NOISE_GATE_STATE], written
 *
 * Planes are independent.  bt is 1, 4, 8 or 16; an axis of N > 1 samples of the block has the window
 * w(k) = sin^2(pi (k + 1/2) / N) and the stride s = N / 4, an axis of N = 1 the window 1 and the stride 1.  Along an image axis of
 * n samples the blocks begin at -(N - s), -(N - s) + s, ... while below n, so that 4 blocks cover every sample and the squares of
 * their windows sum to 1.5 there.  A block reads index i outside [0, n) at the symmetric fold: m = i mod 2n, m < n ? m : 2n - 1 - m.
 *
 * A sample is valid when it is finite and bad is NULL or 0 there.  Per block with at least one valid sample: the invalid samples
 * take (float) mean, the fp64 mean of the block's valid samples; W = w_t w_y w_x; F = the unnormalised DFT of W I;
 * P = sum over the valid samples of W^2 (a + b max(I, 0)); T_k = ((gamma gamma) P) S_c(k); f_k by `mode` from |F_c(k)|^2 and T_k,
 * f_0 = 1.  c(k) is k itself for 0 < k_x < 8, -k for k_x > 8, and of the pair (k, -k) with k_x = 0 or 8 the one whose
 * (k_t, k_y) comes first in row-major order: k and -k share one factor, and only those elements of `spectrum` are read.  The block
 * contributes W Re(IDFT(f F)) (normalised), and out is the sum of the contributions at every sample inside the image divided by
 * 1.5^(number of block axes with N > 1).  A block without a valid sample contributes nothing.  Where the input sample is invalid,
 * out is NaN, or that sum under FILL_INVALID.  state counts per plane the invalid samples and, over the blocks with a valid
 * sample, the blocks, the coefficients k != 0 with f_k > 0 and the coefficients k != 0 (k and -k both count).
 *
 * Checked in this order: bt not in {1, 4, 8, 16}, a mode other than those above, a flag bit other than FILL_INVALID: UNSUPPORTED;
 * n_frames, n_planes, height or width 0 while none is negative: 0, nothing read or written; a negative count, gamma that is not a
 * finite number above 0, a NULL frames, params, out or state, a params or state not aligned to 8 bytes, a frames, spectrum or
 * out not aligned to 4, an out that overlaps frames, bad, params or spectrum: BADARG.  That state overlaps nothing is the
 * caller's to see to. */
int sunerf_noise_gate(const float* frames, const uint8_t* bad, const double* params, const float* spectrum, int n_frames, int n_planes,
                      int height, int width, int bt, int mode, int flags, double gamma, float* out, int64_t* state, void* stream);

#ifdef __cplusplus
}
#endif
#endif
