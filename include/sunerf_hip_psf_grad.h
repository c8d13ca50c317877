/* PSF-gradient entry points of libsunerf_hip.so: the derivative of the PSF-and-bin correlation of sunerf_hip_instrument.h with
 * respect to its taps -- the one reduction that makes the point-spread function a trainable part of the instrument chain
 * (sunerf_hip/psf_fit.py).  A tenth table beside sunerf_hip.h, sunerf_hip_ext.h, sunerf_hip_response.h, sunerf_hip_prep.h,
 * sunerf_hip_instrument.h, sunerf_hip_patch.h, sunerf_hip_likelihood.h, sunerf_hip_ssim_loss.h and sunerf_hip_deconvolve.h, which
 * stay as they are and keep their versions; the same library holds all ten.  Same conventions as sunerf_hip_patch.h: row-major
 * device tensors, `stream` a hipStream_t (NULL: the default stream) and the last argument, status 0 on success, SUNERF_E_BADARG
 * (-1), SUNERF_E_UNSUPPORTED (-2) or a positive hipError_t; argument errors are found before anything touches a device.  The
 * Python binding is sunerf_hip/lib.py: _PSF_GRAD_SIGNATURES; the host side is sunerf_hip/psf_fit.py.  DESIGN.md section 8t.
 *
 * No floating-point atomics anywhere: reruns are bit-identical.  All arithmetic is IEEE fp64 with every operation rounded on its
 * own (no fused multiply-add), in the order written below. */
#ifndef SUNERF_HIP_PSF_GRAD_H
#define SUNERF_HIP_PSF_GRAD_H

#include "sunerf_hip_patch.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Version of THIS table; sunerf_hip/lib.py refuses a library that answers anything else. */
#define SUNERF_PSF_GRAD_ABI_VERSION 1
int sunerf_psf_grad_abi_version(void);

#define SUNERF_PSF_GRAD_MAX_RUNS 512  /* partial sums per tap, over all kernel indices together, unless n_kernels is larger */
#define SUNERF_PSF_GRAD_CHUNK 1024    /* taps of one workgroup at most */

/* Bytes of the reduction workspace: n_kernels * n_runs * kh * kw fp64 partial sums, with
 *   items  = (n_planes / n_kernels) * ceil((height / bin) / T) * ceil((width / bin) / T)     the (plane, tile) pairs of one kernel
 *            index, T the tile of sunerf_hip_instrument.h for (kh, kw, bin): min(32, (127 - max(kh, kw)) / bin + 1)
 *   n_runs = min(items, max(1, SUNERF_PSF_GRAD_MAX_RUNS / n_kernels))
 * so at most max(n_kernels, 512) * kh * kw * 8 bytes whatever the frame: 4.5 MB for a shared 33 x 33 kernel, 37.7 MB for a shared
 * 96 x 96 one.  0 for a count below 1, an n_kernels that does not divide n_planes, a frame without a detector pixel
 * (height / bin or width / bin 0) or a kernel or bin outside the limits.  Nothing of what the workspace held is read; one
 * workspace serves one stream. */
size_t sunerf_psf_grad_workspace_bytes(int n_planes, int height, int width, int n_kernels, int kh, int kw, int bin);

/* The gradient of the strided correlation with respect to its taps.
 *
 *   in     fp32 [n_planes, height, width]              the planes the correlation read
 *   g_out  fp32 [n_planes, height / bin, width / bin]  the cotangent of its output
 *   g_K    fp64 [n_kernels, kh, kw]                    written, every element
 *
 *   g_K[k, i, j] = scale * sum over the planes p with p % n_kernels == k, and over R, C of
 *                  (double) g_out[p, R, C] * (double) in_b[p, R bin + i - anchor_y, C bin + j - anchor_x]
 *
 * with in_b = in under the boundary rule of sunerf_hip_instrument.h (BOUNDARY_NEAREST: the index clamped to the frame;
 * BOUNDARY_ZERO: 0 outside it, and the product with that 0 is formed all the same).  This is the exact derivative of the sum of the
 * correlation of that header with respect to K, before that function rounds to fp32.  n_kernels may be any divisor of n_planes:
 * 1 (a shared kernel), n_planes (one per plane) or C with the planes laid out [n, C] (one per channel over a batch of windows).
 * Limits: kh, kw <= 96, bin <= 8.
 *
 * Order.  Every product of two fp32 values is exact in fp64; the additions and the final multiplication by scale round, once each.
 * The order of the additions depends on the arguments alone:
 *   taps   = kh kw;  chunks = ceil(taps / 1024);  chunk_taps = ceil(taps / chunks)
 *   for nt = 1 .. 4 with G = ceil(chunk_taps / nt) <= 256:  S_r = min(T, 256 / G),  S_c = max(1, min(4, T, (256 / G) / S_r));
 *   of these the nt with the smallest nt / (S_r S_c) is taken, the largest such nt; S = S_r S_c slices, L = ceil(T / S_c).
 *   Slice s = sc S_r + sr holds, of a tile whose n_r x n_c detector pixels lie inside the frame, the rows sr, sr + S_r, ... < n_r
 *   and the columns sc L .. min((sc + 1) L, n_c) - 1.
 *   items, n_runs as above; item q of kernel index k is tile q % tiles (row-major over the plane's tiles of T x T detector pixels)
 *   of plane k + (q / tiles) n_kernels; run r holds the items floor(r items / n_runs) .. floor((r + 1) items / n_runs) - 1.
 * (1) For a tap, a run and a slice, one sum starts at +0.0 and takes, item by item ascending, the products of the slice's
 *     detector pixels, row by row ascending and inside a row column by column ascending.
 * (2) The run's partial is the sum of its slices, slice 0 first, then + slice 1, ... + slice S - 1.
 * (3) The tap's sum is the run's partials, run 0 first, then + run 1, ...; g_K = scale * that sum.
 * Non-finite values propagate by IEEE rules: a NaN in g_out[p] reaches every tap of kernel index p % n_kernels and no other.
 * With g_out all zeros and in finite every g_K is scale * +0.0.
 *
 * Checked in this order (the instrument table's): kh or kw above 96, bin above 8, a boundary other than the two: UNSUPPORTED;
 * n_planes, height / bin or width / bin 0 while no count is negative and kh, kw, bin >= 1: 0, nothing read or written; a negative
 * count, kh, kw or bin below 1, n_kernels below 1 or no divisor of n_planes, an anchor outside [0, kh) x [0, kw), a NULL in, g_out,
 * g_K or workspace (the workspace's size is never 0 here), a g_K or workspace not aligned to 8 bytes: BADARG. */
int sunerf_psf_grad_taps(const float* in, const float* g_out, int n_planes, int height, int width, int n_kernels, int kh, int kw,
                         int bin, int anchor_y, int anchor_x, double scale, int boundary, double* g_K, void* workspace, void* stream);

#ifdef __cplusplus
}
#endif
#endif
