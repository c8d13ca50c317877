/* Patch entry points of libsunerf_hip.so: what training THROUGH the instrument needs beside the forward model of
 * sunerf_hip_instrument.h -- the adjoint (transpose) of the PSF-and-bin correlation, and one launch that writes a batch of
 * detector-pixel patches as the rays of their sub-pixel windows (halo included) with their targets.  A sixth table beside
 * sunerf_hip.h, sunerf_hip_ext.h, sunerf_hip_response.h, sunerf_hip_prep.h and sunerf_hip_instrument.h, which stay as they are and
 * keep their versions; the same library holds all six.  Same conventions as sunerf_hip_instrument.h: row-major device tensors,
 * `stream` a hipStream_t (NULL: the default stream), status 0 on success, SUNERF_E_BADARG (-1), SUNERF_E_UNSUPPORTED (-2) or a
 * positive hipError_t; argument errors are found before anything touches a device.  The Python binding is sunerf_hip/lib.py:
 * _PATCH_SIGNATURES; the host side is sunerf_hip/patch.py and sunerf_hip/instrument.py.  DESIGN.md section 8p.
 *
 * No floating-point atomics anywhere: reruns are bit-identical, and a plane alone gives the bits it gives inside a batch of
 * planes.  The arithmetic of the adjoint is IEEE fp64 with every operation rounded on its own (no fused multiply-add), in the
 * order written, and one rounding to fp32 at the end. */
#ifndef SUNERF_HIP_PATCH_H
#define SUNERF_HIP_PATCH_H

#include "sunerf_hip_instrument.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Version of THIS table; sunerf_hip/lib.py refuses a library that answers anything else. */
#define SUNERF_PATCH_ABI_VERSION 1
int sunerf_patch_abi_version(void);

/* The adjoint works on square tiles of T x T INPUT pixels (pixels of g_in), T = 32, 256 threads with four pixels each.  LDS holds
 * the kernel, kh x bin x ceil(kw / bin) fp64 words (at most 96 x 103 = 77 KiB, 72 KiB at bin 1), the slice of g_out whose taps
 * reach the tile, at most ((T + kh - 2) / bin + 1) x ((T + kw - 2) / bin + 1) fp32 words (127 x 127 = 63 KiB at bin 1, 64 x 64 at
 * bin 2), and one row of zeros for each: at most 137 KiB of the 160 KiB of a compute unit. */
#define SUNERF_PATCH_TILE 32

/* The exact transpose of sunerf_instrument_correlate_bin for the same n_planes, height, width, K, n_kernels, kh, kw, bin, anchor,
 * scale and boundary (same limits: kh, kw <= SUNERF_INSTRUMENT_MAX_KERNEL, bin <= SUNERF_INSTRUMENT_MAX_BIN, n_kernels 1 or
 * n_planes): g_in [n_planes, height, width] fp32, every element written, from g_out [n_planes, height / bin, width / bin] fp32,
 *   g_in[p, y, x] = scale * sum K[p or 0, i, j] * (double) g_out[p, R, C]
 * over every (R, C, i, j) whose tap of the forward reads (y, x): the row R bin + i - anchor_y -- clamped to [0, height) under
 * BOUNDARY_NEAREST, discarded when outside it under BOUNDARY_ZERO -- equals y, and likewise the column C bin + j - anchor_x and x.
 * The sum is taken in fp64 in ONE order: i ascending, inside it j ascending, inside it R ascending, inside it C ascending; each
 * product is rounded, then added; the sum starts from +0.0, is multiplied by `scale`, then rounded to fp32.  Trailing rows and
 * columns of the input that fill no detector pixel still receive the gradient of the taps that read them; under BOUNDARY_NEAREST
 * an edge or corner pixel collects every tap that was clamped onto it.  Non-finite g_out propagates by IEEE rules through every
 * term that holds it.
 * Checked in this order (the forward's): kh or kw above 96, bin above 8, a boundary other than the two: UNSUPPORTED; n_planes,
 * height / bin or width / bin 0 while no count is negative and kh, kw, bin >= 1: 0, nothing read or written; a negative count, kh,
 * kw or bin below 1, n_kernels neither 1 nor n_planes, an anchor outside [0, kh) x [0, kw), a NULL g_out, K or g_in, a K not
 * aligned to 8 bytes: BADARG. */
int sunerf_patch_correlate_bin_adjoint(const float* g_out, int n_planes, int height, int width, const double* K, int n_kernels,
                                       int kh, int kw, int bin, int anchor_y, int anchor_x, double scale, int boundary,
                                       float* g_in, void* stream);

/* One view of a patch set: a detector image and the EXTENDED sub-pixel axes of its frame.  With `bin` sub-pixels per detector
 * pixel and axis and a kh x kw correlation kernel of anchor (ay, ax), entry m of tx is the angle of sub-pixel column m - ax of the
 * detector frame, m in [0, (width - 1) bin + kw); ty likewise with ay, kh and height.  Entries past the frame's edge are real
 * angles: the window of a patch at the edge is rendered, not padded.  Modelled on SunerfViewDesc (sunerf_hip.h). */
#define SUNERF_PATCH_VIEW_DESC_BYTES 216
typedef struct SunerfPatchViewDesc {
  const double* tx;          /* DEVICE: extended column angles [(width - 1) bin + kw]                                   */
  const double* ty;          /* DEVICE: extended row angles [(height - 1) bin + kh]                                     */
  const float* image;        /* DEVICE: [n_planes, height, width], the present channels only                            */
  int32_t height, width;     /* detector pixels of the view                                                             */
  float c2w[12];             /* rows of pose_spherical(...)[:3, :4]                                                     */
  float time;                /* normalised observation time                                                             */
  int32_t n_planes;
  int32_t plane[SUNERF_OBS_MAX_CHANNELS];      /* per output channel: its plane of `image`, or -1 (absent: target 0, wavelength 0) */
  float wavelength[SUNERF_OBS_MAX_CHANNELS];   /* per output channel: the value written for a present channel                */
} SunerfPatchViewDesc;

/* A batch of patches in one launch.  views: DEVICE table of n_views descriptors (the caller keeps every pointer in it valid);
 * patches: DEVICE int32 [n_patches, 3] = (view, R0, C0), the view's number and the first detector row and column of a patch of
 * P x P detector pixels.  With hw = (P - 1) bin + kh and ww = (P - 1) bin + kw, patch k writes
 *   rays       [k, wy, wx, 2, 3]  origin and direction of the ray with angles (tx[C0 bin + wx], ty[R0 bin + wy]) of its view: the
 *                                 arithmetic of csrc/ray_math.h, so the bits sunerf_observer_rays gives for the same angles
 *   time       [(k hw + wy) ww + wx]               the view's time
 *   wavelength [((k hw + wy) ww + wx), c]          the view's wavelength of channel c, 0 for an absent one (may be NULL)
 *   target     [k, c, py, px] = image[plane[c], R0 + py, C0 + px], 0 for an absent channel
 * rays [n_patches, hw, ww, 2, 3], time [n_patches hw ww, 1], target [n_patches, n_channels, P, P], wavelength
 * [n_patches hw ww, n_channels], all fp32.  A triple whose view is outside [0, n_views) or whose patch does not lie inside its view
 * (a corrupt list) gives all-zero records.
 * Checked in this order: kh or kw above 96, bin above 8: UNSUPPORTED; n_patches 0 while no count is negative and P, bin, kh, kw
 * >= 1: 0, nothing read or written; a negative n_patches, n_views < 1, P, bin, kh or kw below 1, n_channels outside
 * [1, SUNERF_OBS_MAX_CHANNELS], n_patches hw ww or n_patches n_channels P P above 2^31 - 1, a NULL views, patches, rays, time or
 * target: BADARG. */
int sunerf_patch_records(const SunerfPatchViewDesc* views, int n_views, const int32_t* patches, int n_patches, int n_channels,
                         int P, int bin, int kh, int kw, float* rays, float* time, float* target, float* wavelength, void* stream);

#ifdef __cplusplus
}
#endif
#endif
