/* Extension entry points of libsunerf_hip.so: additions that leave the table of sunerf_hip.h (and its version) as it is.
 * Same conventions as there: row-major fp32 device tensors unless stated, `stream` a hipStream_t (NULL: the default stream),
 * status 0 on success, SUNERF_E_BADARG (-1), SUNERF_E_UNSUPPORTED (-2), SUNERF_E_WORKSPACE (-3) or a positive hipError_t;
 * argument errors are found before anything touches a device.  The Python binding is sunerf_hip/lib.py: _EXT_SIGNATURES. */
#ifndef SUNERF_HIP_EXT_H
#define SUNERF_HIP_EXT_H

#include "sunerf_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Version of THIS table; sunerf_hip/lib.py refuses a library that answers anything else. */
#define SUNERF_EXT_ABI_VERSION 1
int sunerf_ext_abi_version(void);

/* ------------------------------------------------------------------------------------------------------------
 * Voxel-grid field with a time axis: values [T][n0][n1][n2][C] fp32 on frame_times [T] (fp64
 * normalised times, strictly increasing and finite, T >= 2); every frame lives on the one grid of the descriptor, 1 <= C <= 4.
 * The static field of sunerf_hip.h (SunerfGridFieldDesc, sunerf_grid_field_*) blended linearly between its two neighbouring
 * frames, as MHDModel blends two simulation frames in time (sunerf/model/mhd_model.py:112-124), and fitted through the
 * adjoint: time-dependent tomography.
 *
 * One sample at the point p [model units, fp32] and the time t [fp32] of its ray:
 *   space : exactly as sunerf_grid_field_fwd locates it (the same code, csrc/grid_locate.h): coordinates, cell, the six
 *           weights and the inside test of sunerf_hip.h
 *   time  : t promoted to fp64; j = searchsorted(frame_times, t, 'left') - 1 clipped to [0, T - 2],
 *           s = (t - tau_j) / (tau_{j+1} - tau_j); the weights wt_lo = (float)(1 - s), wt_hi = (float)s
 *           SUNERF_TIME_CLAMP: t <= tau_0 is j = 0, s = 0 and t >= tau_{T-1} is j = T - 2, s = 1, set, not computed
 *           SUNERF_TIME_FILL : t outside [tau_0, tau_{T-1}] answers the fill
 *           a NaN time answers the fill in both modes
 *   value : raw[c] = wt_lo * tri(frame j)[c] + wt_hi * tri(frame j + 1)[c] in fp32, tri the nested trilinear expression of the
 *           static kernel: at t == tau_f the answer is that of sunerf_grid_field_fwd on values[f], as numbers
 *   outside in space or time, or a NaN: raw[c] = fill[c], no gradient
 *
 * sunerf_dynamic_grid_fwd: ray mode (points == NULL): rays_o / rays_d [N,3], z_vals [N,S], ray_times [N] -> raw [N,S,C] at
 *   the samples o + d z (multiply, then add, in fp32); points mode: points [M,4] = (x, y, z, t), point_stride == 4,
 *   n_rays = M, n_samples = 1 -> raw [M,C]; rays_o, rays_d, z_vals and ray_times are not read then.  frame_times [T] fp64 is
 *   a DEVICE array, values [T][n0][n1][n2][C].  cells [N S] int32 and weights [N S][8] fp32 (both or neither), for the backward:
 *   cells = j * n_cells + the static field's cell id (n_cells = the number of cells of the grid), outside (T - 1) * n_cells;
 *   weights = the six spatial weights [3][2], then wt_lo, wt_hi (outside: zeros).
 * sunerf_dynamic_grid_bwd: g_values[f][node][c] (+)= sum over samples of wt(sample, f) w(sample, node) g_raw[sample][c].
 *   g_raw [n_total][C], cells [n_total], weights [n_total][8] as the forward left them; perm [n_total] int64: a stable
 *   ascending sort of `cells`; seg_start [(T - 1) * n_cells + 1] int64: the first sorted position of every id.  g_values
 *   [T][n0][n1][n2][C].  No floating-point atomics: one thread per (frame, node) adds interval f - 1 (wt_hi) and then interval
 *   f (wt_lo), in each the segments of the node's adjacent cells in the static kernel's order; segments longer than 64 samples
 *   go through per-wave partial sums in `workspace` [sunerf_dynamic_grid_bwd_workspace_bytes(n_total, C) bytes =
 *   ceil(n_total / 64) * 2 * 16 * C * 4]: reruns are bit-identical.  accumulate != 0 adds onto g_values.  n_total == 0:
 *   g_values is zeroed (accumulate == 0) or left alone, and no other pointer is read.
 * Checked in this order, before anything touches a device: the descriptor and the sizes (as sunerf_grid_field_*; n_frames
 * < 2, a time_mode that is neither, points with n_samples != 1 or point_stride != 4: -1; (T - 1) * n_cells >= 2^31 - 1: -2),
 * then the empty batch (0), then null pointers (-1) and the workspace (-3).  `grid` is a HOST pointer (its axis pointers are
 * device arrays); its n_channels is C.
 * ---------------------------------------------------------------------------------------------------------- */
#define SUNERF_TIME_CLAMP 0
#define SUNERF_TIME_FILL  1
int sunerf_dynamic_grid_fwd(const SunerfGridFieldDesc* grid, const double* frame_times, int n_frames, int time_mode,
                            const float* values, const float* rays_o, const float* rays_d, const float* z_vals,
                            const float* ray_times, int64_t n_rays, int n_samples, const float* points, int point_stride,
                            float* raw, int* cells, float* weights, void* stream);
size_t sunerf_dynamic_grid_bwd_workspace_bytes(int64_t n_total, int n_channels);
int sunerf_dynamic_grid_bwd(const SunerfGridFieldDesc* grid, int n_frames, const float* g_raw, const int* cells,
                            const float* weights, const int64_t* perm, const int64_t* seg_start, int64_t n_total,
                            void* workspace, size_t workspace_bytes, float* g_values, int accumulate, void* stream);

#ifdef __cplusplus
}
#endif
#endif
