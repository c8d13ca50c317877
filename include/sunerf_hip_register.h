/* Registration entry points of libsunerf_hip.so: the frames of an image sequence, each with its own observer, pixel grid and time,
 * are resampled onto ONE reference observer, grid and time under the assumption that what they show lies on the sphere
 * r = radius and turns with a three-term differential rotation law.  After the call pixel (y, x) of every frame shows the same
 * piece of the Sun, which is what sunerf_stack_combine and sunerf_noise_gate assume.  The kernel behind sunerf_hip/register.py.
 * A fifteenth table beside sunerf_hip.h, sunerf_hip_ext.h, sunerf_hip_response.h, sunerf_hip_prep.h, sunerf_hip_instrument.h,
 * sunerf_hip_patch.h, sunerf_hip_likelihood.h, sunerf_hip_ssim_loss.h, sunerf_hip_deconvolve.h, sunerf_hip_psf_grad.h,
 * sunerf_hip_despike.h, sunerf_hip_coalign.h, sunerf_hip_stack.h and sunerf_hip_noise_gate.h, which stay as they are and keep
 * their versions; the same library holds all fifteen.  Same conventions as sunerf_hip.h: row-major device tensors, `stream` a
 * hipStream_t (NULL: the default stream) and the last argument, status 0 on success, SUNERF_E_BADARG (-1), SUNERF_E_UNSUPPORTED
 * (-2) or a positive hipError_t; argument errors are found before anything touches a device.  The Python binding is
 * sunerf_hip/lib.py: _REGISTER_SIGNATURES; the host side is sunerf_hip/register.py.  DESIGN.md section 8aa.
 *
 * No floating-point atomics anywhere (the four counters of a frame are integer atomics): reruns are bit-identical, and no output
 * depends on what it held before the call.  The geometry is fp64, every operation rounded on its own (no fused multiply-add),
 * in the order written below; the value is prep's tap sum in fp64, rounded to fp32 once.  There is no workspace. */
#ifndef SUNERF_HIP_REGISTER_H
#define SUNERF_HIP_REGISTER_H

#include "sunerf_hip_prep.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Version of THIS table; sunerf_hip/lib.py refuses a library that answers anything else. */
#define SUNERF_REGISTER_ABI_VERSION 1
int sunerf_register_abi_version(void);

#define SUNERF_REGISTER_TILE 16  /* output pixels of a workgroup along y and along x */
#define SUNERF_REGISTER_STATE 4  /* int64 per frame: pixels with status ON_DISK, OFF_DISK, BEHIND, OUTSIDE, in this order */
/* the edge rule: a coordinate this far outside [0, n - 1] is taken to lie on the border (2^-20 pixel) */
#define SUNERF_REGISTER_EDGE_EPS 9.5367431640625e-07

/* status of an output pixel: exactly one of these, decided in the order of the steps below */
#define SUNERF_REGISTER_ON_DISK 1   /* the line of sight meets the sphere; the value was sampled                               */
#define SUNERF_REGISTER_OFF_DISK 2  /* it does not.  off_disk = MISSING: the value is `missing`; off_disk = CLOSEST: the value */
                                    /* was sampled at the point of closest approach (never `missing` with this status)         */
#define SUNERF_REGISTER_BEHIND 4    /* on the disk, but the rotated point is behind the limb of the frame: `missing`            */
#define SUNERF_REGISTER_OUTSIDE 8   /* the point is outside the frame's pixel grid (or the frame is unusable): `missing`        */

/* off_disk */
#define SUNERF_REGISTER_OFF_DISK_MISSING 0
#define SUNERF_REGISTER_OFF_DISK_CLOSEST 1
/* flags */
#define SUNERF_REGISTER_PROPAGATE 1 /* NaN where a tap read a pixel whose byte in the frame's mask is set (frames without a mask: no effect) */

/* One frame of the sequence; the table of n_frames of them is in device memory.  Frames may differ in shape and observer. */
typedef struct SunerfRegisterFrameDesc {
  const double* coefficients; /* [n_planes][height][width] fp64 of sunerf_prep_spline_prefilter at the call's order     */
  const uint8_t* mask;        /* [n_planes][height][width] or NULL: not 0 = a flagged pixel (PROPAGATE)                 */
  const double* tx;           /* [width]  angles of the pixel columns, strictly monotone                               */
  const double* ty;           /* [height] angles of the pixel rows, strictly monotone                                  */
  int32_t height, width;
  float c2w[12];              /* rows 0 .. 2 of the camera-to-world pose, row-major [3][4]                              */
  double dt;                  /* t_k - t_ref                                                                           */
  double shift_y, shift_x;    /* pointing offset in pixels of this frame, added to the coordinate                      */
} SunerfRegisterFrameDesc;
size_t sunerf_register_frame_desc_bytes(void); /* sizeof(SunerfRegisterFrameDesc) = 112 */

/* One launch for all frames, one workgroup per 16 x 16 output pixels of one frame, one lane per pixel: the geometry and the
 * 2 (order + 1) weights are formed once and reused over the planes.
 *
 *   frames   SunerfRegisterFrameDesc [n_frames]                      (device)
 *   c2w_ref  fp32 [12], tx_ref fp64 [out_width], ty_ref fp64 [out_height]   the reference observer (device)
 *   out      fp32  [n_frames][n_planes][out_height][out_width]       written, every element
 *   status   uint8 [n_frames][out_height][out_width]                 written, every element
 *   coords   fp64  [n_frames][2][out_height][out_width] or NULL      written, every element: cy, cx
 *   state    int64 [n_frames][SUNERF_REGISTER_STATE]                 written
 *
 * Output pixel (r, c) of frame k, all in fp64 (c2w promoted), sums of three left to right:
 *  1. Tx = tx_ref[c], Ty = ty_ref[r]; e = (sin Tx, -(sin Ty) cos Tx, -(cos Tx) cos Ty); d_i = (c2w_ref[4i] e_0 + c2w_ref[4i+1] e_1)
 *     + c2w_ref[4i+2] e_2, o_i = c2w_ref[4i+3]; v = o x d; m = radius radius - ((v_0 v_0 + v_1 v_1) + v_2 v_2); od = o . d.
 *     On the disk iff m > 0 and od < 0 (the expressions of sunerf_reproject_views).
 *  2. On the disk s = -od - sqrt(m); off it with CLOSEST s = -od (the point of closest approach to the centre, which is the
 *     tangent point at the limb: the map is continuous there); off it with MISSING the pixel is OFF_DISK.  p_i = o_i + d_i s.
 *  3. rho = sqrt((p_0 p_0 + p_1 p_1) + p_2 p_2), lat = atan2(-p_2, hypot(p_0, p_1)), lon = atan2(-p_0, p_1); sl = sin lat,
 *     s2 = sl sl, w = (A + B s2) + C (s2 s2), lon_k = lon + w dt; q = (rho (-(cos lat) sin lon_k), rho ((cos lat) cos lon_k),
 *     rho (-sl)): the plasma seen at lon at the reference time sat at lon_k when frame k was taken.  A, B, C are radians per
 *     unit of dt relative to the frame of the poses.
 *  4. With o' the position of frame k: an on-disk pixel with q . o' - radius radius <= 0 is BEHIND.
 *  5. cam = c2w_k[:3,:3]^-1 (q - o') by cofactors; Tx' = atan2(cam_0, hypot(cam_1, cam_2)), Ty' = atan2(-cam_1, -cam_2);
 *     cx = axis(tx_k, width, Tx') + shift_x, cy = axis(ty_k, height, Ty') + shift_y.  axis: on n >= 2 centres the interval
 *     [lo, lo + 1] found by bisection (the outermost interval for an angle beyond the ends), lo + (t - a_lo) / (a_lo+1 - a_lo);
 *     on one centre 0 when t equals it, else NaN.
 *  6. A coordinate in [-EDGE_EPS, 0) becomes 0, one in (n - 1, n - 1 + EDGE_EPS] becomes n - 1; a coordinate that is then outside
 *     [0, n - 1], or NaN, makes the pixel OUTSIDE, as does a frame with a NULL coefficients or a height or width below 1.
 *  7. Else the pixel is ON_DISK, or OFF_DISK when it came through CLOSEST, and per plane its value is the sum over the
 *     (order + 1)^2 taps as the affine resample of sunerf_hip_prep.h forms it (rows outermost, (coefficient wy) wx, mirrored
 *     indices, scipy's B-spline weights), rounded to fp32 once; with PROPAGATE NaN when a tap read a flagged pixel of that plane.
 * `coords` holds cy, cx after step 6 for a sampled pixel, after step 5 for an OUTSIDE pixel whose frame is usable, else NaN.
 * `state` counts the pixels of each status per frame.  `missing` may be any value, NaN included.
 *
 * Checked in this order: order outside 0 .. 5, an off_disk other than those above, a flag bit other than PROPAGATE: UNSUPPORTED;
 * n_frames, out_height or out_width 0 while no count is negative: 0, nothing read or written; a negative count, n_planes 0,
 * n_frames above 65535, out_height above 16 x 65535, a radius that is not a finite number above 0, an A, B or C that is not finite, a NULL frames, c2w_ref,
 * tx_ref, ty_ref, out, status or state, a frames, tx_ref, ty_ref, coords or state not aligned to 8 bytes, a c2w_ref or out not
 * aligned to 4: BADARG.  The descriptors are read on the device only; that no output overlaps an input or another output is the
 * caller's to see to. */
int sunerf_register_frames(const SunerfRegisterFrameDesc* frames, int n_frames, int n_planes, int order, const float* c2w_ref,
                           const double* tx_ref, const double* ty_ref, int out_height, int out_width, double radius, double A,
                           double B, double C, int off_disk, float missing, int flags, float* out, uint8_t* status, double* coords,
                           int64_t* state, void* stream);

#ifdef __cplusplus
}
#endif
#endif
