// The ray of one pixel (restates get_rays, sunerf/data/ray_sampling.py:7-36), shared by rays.hip (frame tiles) and
// observations.hip (training pools) so that both produce the same bits for the same pixel.
//   direction = (sin Tx, -sin Ty cos Tx, -cos Tx cos Ty)      evaluated in fp64, rounded to fp32 (np.stack(..., dtype=float32))
//   rays_d[r] = sum_c direction[c] * c2w[r][c]               fp32 products, summed left to right (np.sum over 3 elements)
//   rays_o    = c2w[:3, 3]
#pragma once
#include <hip/hip_runtime.h>

// c2w: 12 floats = rows of the 3x4 pose.  o, d: 3 floats each.
__device__ __forceinline__ void sunerf_pixel_ray(double Tx, double Ty, const float* c2w, float* o, float* d) {
  const double sx = sin(Tx), cx = cos(Tx), sy = sin(Ty), cy = cos(Ty);
  const float d0 = (float)sx, d1 = (float)(-sy * cx), d2 = (float)(-cx * cy);
#pragma unroll
  for (int r = 0; r < 3; ++r) {
    d[r] = (d0 * c2w[4 * r + 0] + d1 * c2w[4 * r + 1]) + d2 * c2w[4 * r + 2];
    o[r] = c2w[4 * r + 3];
  }
}
