/* Co-alignment entry points of libsunerf_hip.so: for every integer shift of a window, the six sums a zero-mean normalised
 * cross-correlation (ZNCC) of an image with a template is made of, over the pixels valid in both -- the reduction behind
 * sunerf_hip/coalign.py, which finds a view's pointing offset to a fraction of a pixel and moves its crpix by it.  A twelfth table
 * beside sunerf_hip.h, sunerf_hip_ext.h, sunerf_hip_response.h, sunerf_hip_prep.h, sunerf_hip_instrument.h, sunerf_hip_patch.h,
 * sunerf_hip_likelihood.h, sunerf_hip_ssim_loss.h, sunerf_hip_deconvolve.h, sunerf_hip_psf_grad.h and sunerf_hip_despike.h, which stay
 * as they are and keep their versions; the same library holds all twelve.  Same conventions as sunerf_hip_psf_grad.h: row-major
 * device tensors, `stream` a hipStream_t (NULL: the default stream) and the last argument, status 0 on success, SUNERF_E_BADARG
 * (-1), SUNERF_E_UNSUPPORTED (-2) or a positive hipError_t; argument errors are found before anything touches a device.  The Python
 * binding is sunerf_hip/lib.py: _COALIGN_SIGNATURES; the host side is sunerf_hip/coalign.py.  DESIGN.md section 8x.
 *
 * No floating-point atomics anywhere: reruns are bit-identical.  All arithmetic is IEEE fp64 with every operation rounded on its
 * own (no fused multiply-add), in the order written below. */
#ifndef SUNERF_HIP_COALIGN_H
#define SUNERF_HIP_COALIGN_H

#include "sunerf_hip_patch.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Version of THIS table; sunerf_hip/lib.py refuses a library that answers anything else. */
#define SUNERF_COALIGN_ABI_VERSION 1
int sunerf_coalign_abi_version(void);

#define SUNERF_COALIGN_MAX_SHIFT 32  /* per axis: at most 65 x 65 = 4225 shifts */
#define SUNERF_COALIGN_SUMS 6        /* per shift: n, Sa, Sb, Saa, Sbb, Sab */
#define SUNERF_COALIGN_TILE 32       /* template pixels per side of a tile */
#define SUNERF_COALIGN_CHUNK 1024    /* shifts of one workgroup at most */
#define SUNERF_COALIGN_MAX_RUNS 256  /* partial sums per shift, over all planes together, unless n_planes is larger */

/* Bytes of the reduction workspace: n_planes * n_runs * S * 6 fp64 partial sums, with
 *   S      = (2 max_dy + 1) (2 max_dx + 1)                                     the shifts
 *   tiles  = ceil(height / 32) * ceil(width / 32)                              the template tiles of one plane
 *   n_runs = min(tiles, max(1, SUNERF_COALIGN_MAX_RUNS / n_planes))
 * so at most max(n_planes, 256) * S * 48 bytes whatever the frame: 3.6 MB at max_dy = max_dx = 8, 51.9 MB at the limit of 32 (a
 * partial sum per tile of a 1024 x 1024 plane would be 208 MB there).  0 for a count below 1 or a max_dy, max_dx outside
 * [0, SUNERF_COALIGN_MAX_SHIFT].  Nothing of what the workspace held is read; one workspace serves one stream. */
size_t sunerf_coalign_workspace_bytes(int n_planes, int height, int width, int max_dy, int max_dx);

/* The six sums of every shift.
 *
 *   image         fp32 [n_planes, height, width]
 *   templ         fp32 [n_planes, height, width]
 *   bad_image     uint8, shape of image, or NULL        not 0: the pixel takes part in no sum
 *   bad_template  uint8, shape of templ, or NULL        likewise
 *   sums          fp64 [n_planes, 2 max_dy + 1, 2 max_dx + 1, 6], written, every element
 *
 * Planes are independent.  For the shift (dy, dx) = (i - max_dy, j - max_dx) of element [p, i, j] the pair set is every (r, c) with
 * (r, c) and (r + dy, c + dx) inside the frame, a = image[p, r + dy, c + dx] and b = templ[p, r, c] both finite (NaN and +-inf are
 * not) and neither pixel flagged in its bad_* plane.  Over that set, in this order:
 *   n (the count, as a double), sum a, sum b, sum a a, sum b b, sum a b
 * with a and b converted to fp64 first.  A shift without a pair gives six +0.0; max_dy >= height or max_dx >= width is legal and
 * gives such shifts.  The shift (dy, dx) at which the sums peak means: the image's content sits dy rows and dx columns further along
 * than the template's.
 *
 * Order.  Every product of two fp32 values is exact in fp64, and so is a product with a validity of 0.0 or 1.0; only the additions
 * round.  A pixel that is not valid is staged as the value +0.0 with validity 0.0, a valid one with validity 1.0, and a term is
 *   n: va vb    sum a: a vb    sum b: b va    sum a a: (a a) vb    sum b b: (b b) va    sum a b: a b
 * so a pair outside the set adds +-0.0, which changes no sum that began at +0.0.  The order of the additions depends on the arguments
 * alone:
 *   S = S_y S_x;  chunks = ceil(S / 1024);  chunk_shifts = ceil(S / chunks);  shift s = i S_x + j
 *   for nt = 1 .. 4 with G = ceil(chunk_shifts / nt) <= 256:  R = min(32, 256 / G),  C = max(1, min(4, (256 / G) / R));
 *   of these the nt with the smallest nt / (R C) is taken, the largest such nt; R C slices, L = ceil(32 / C).
 *   Slice q = qc R + qr holds, of a tile whose n_r x n_c template pixels lie inside the frame, the rows qr, qr + R, ... < n_r and the
 *   columns qc L .. min((qc + 1) L, n_c) - 1.
 *   tiles, n_runs as above; tile t of a plane is row-major over the plane's tiles of 32 x 32 template pixels; run u holds the tiles
 *   floor(u tiles / n_runs) .. floor((u + 1) tiles / n_runs) - 1.
 * (1) For a sum of a shift, a run and a slice, one sum starts at +0.0 and takes, tile by tile ascending, the terms of the slice's
 *     template pixels, row by row ascending and inside a row column by column ascending.
 * (2) The run's partial is the sum of its slices, slice 0 first, then + slice 1, ... + slice R C - 1.
 * (3) The result is the run's partials, run 0 first, then + run 1, ...
 *
 * Checked in this order: max_dy or max_dx above SUNERF_COALIGN_MAX_SHIFT: UNSUPPORTED; n_planes, height or width 0 while no count
 * and neither max_dy nor max_dx is negative: 0, nothing read or written; a negative n_planes, height, width, max_dy or max_dx, a NULL
 * image, templ, sums or workspace (the workspace's size is never 0 here), a sums or workspace not aligned to 8 bytes, a sums that
 * overlaps image, templ, bad_image or bad_template: BADARG. */
int sunerf_coalign_shift_sums(const float* image, const float* templ, const unsigned char* bad_image, const unsigned char* bad_template,
                              int n_planes, int height, int width, int max_dy, int max_dx, double* sums, void* workspace,
                              void* stream);

#ifdef __cplusplus
}
#endif
#endif
