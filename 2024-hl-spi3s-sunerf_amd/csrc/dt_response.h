// AIA temperature response R_w(log T) of the density / temperature path, shared by the line-of-sight integral (dt.hip) and
// the per-voxel emissivity (volume.hip) so that a voxel and the integral evaluate the same function.
//
// R_w = linear interpolation of the (7, 101) response table (x exposure time), 0 outside the table (Interp1D(..., extrap=0),
// restated from its documented semantics), density_temperature.py:245-256.
#pragma once
#include <hip/hip_runtime.h>

constexpr int NCH = 7;
constexpr int NTAB = NCH * 101;

__device__ __forceinline__ int channel_of(float wl) {
  const float w[NCH] = {94.f, 131.f, 171.f, 193.f, 211.f, 304.f, 335.f};
#pragma unroll
  for (int c = 0; c < NCH; ++c) if (wl == w[c]) return c;
  return -1;
}

// linear interpolation on the 101-point grid; returns value and slope (both 0 outside [x0, x100])
__device__ __forceinline__ void response(const float* lt, const float* rs, float x, float& val, float& slope) {
  val = 0.f; slope = 0.f;
  if (!(x >= lt[0] && x <= lt[100])) return;
  int i = (int)((x - lt[0]) * 20.f);              // grid step 0.05
  i = max(0, min(99, i));
  while (i < 99 && lt[i + 1] <= x) ++i;            // searchsorted(right=True) - 1, clamped to the last interval
  while (i > 0 && lt[i] > x) --i;
  const float x0 = lt[i], x1 = lt[i + 1], y0 = rs[i], y1 = rs[i + 1];
  slope = (y1 - y0) / (x1 - x0);
  val = y0 + (x - x0) * (y1 - y0) / (x1 - x0);
}
