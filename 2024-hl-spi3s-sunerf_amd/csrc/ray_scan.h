// Scans and sums over the 32 lanes that own one ray (lane n = sample 32 c + n of chunk c): what the line-of-sight integrals
// (dt_sweep.h, dem.hip, thomson.hip) carry along a ray.  Fixed shuffle order: reruns give the same bits.
#pragma once
#include <hip/hip_runtime.h>

__device__ __forceinline__ float scan_up32(float v, int n) {      // inclusive prefix sum over the 32 lanes of a ray
#pragma unroll
  for (int d = 1; d < 32; d <<= 1) {
    const float o = __shfl_up(v, d, 32);
    if (n >= d) v += o;
  }
  return v;
}
__device__ __forceinline__ float scan_down32(float v, int n) {    // inclusive suffix sum
#pragma unroll
  for (int d = 1; d < 32; d <<= 1) {
    const float o = __shfl_down(v, d, 32);
    if (n + d < 32) v += o;
  }
  return v;
}
__device__ __forceinline__ float sum32(float v) {
#pragma unroll
  for (int d = 16; d >= 1; d >>= 1) v += __shfl_xor(v, d, 32);
  return v;
}
