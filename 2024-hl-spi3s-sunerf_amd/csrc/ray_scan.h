// Scans and sums over the 32 lanes that own one ray (lane n = sample 32 c + n of chunk c): what the line-of-sight integrals
// (emission_sweep.h, dt_sweep.h, dem.hip, thomson.hip) carry along a ray, and the small reductions their kernels end with.
// Fixed shuffle order: reruns give the same bits.
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
__device__ __forceinline__ float scan_mul_up32(float v, int n) {  // inclusive prefix product
#pragma unroll
  for (int d = 1; d < 32; d <<= 1) {
    const float o = __shfl_up(v, d, 32);
    if (n >= d) v *= o;
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

// ---- over the 64 lanes of a wave (float and double): the order 32..1 is part of the result's bits ----
// (what a workgroup and a grid do with the wave totals -- the waves in wave order, the LDS tree, the ticket -- is ordered_sum.h's)
template <class T>
__device__ __forceinline__ T sum64(T v) {
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) v += __shfl_xor(v, d, 64);
  return v;
}
__device__ __forceinline__ float max64(float v) {
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) v = fmaxf(v, __shfl_xor(v, d, 64));
  return v;
}

// ---- batch maximum to one word: ONE atomic per workgroup (atomics on one address serialise in L2) ----
// In two halves around the caller's __syncthreads(): batch_max_stage() before it, batch_max_publish<WAVES>() after it.
// `wave_max`: one LDS float per wave, the caller's (static or a slice of its dynamic LDS).
__device__ __forceinline__ void batch_max_stage(float local_max, float* wave_max, int tid) {
  local_max = max64(local_max);
  if ((tid & 63) == 0) wave_max[tid >> 6] = local_max;
}
// the bit pattern of a non-negative float orders like an unsigned integer; zero, inf and NaN are not published
template <int WAVES>
__device__ __forceinline__ void batch_max_publish(const float* wave_max, int tid, unsigned* absmax_bits) {
  if (tid == 0) {
    float m = wave_max[0];
#pragma unroll
    for (int w = 1; w < WAVES; ++w) m = fmaxf(m, wave_max[w]);
    if (m > 0.f && m < INFINITY) atomicMax(absmax_bits, __float_as_uint(m));
  }
}

// trapezoid weight of point j on the grid z[0..S-2]: (dz_{j-1} + dz_j) / 2 with the missing neighbours of the two ends dropped
// (S by reference keeps dt_bwd_kernel's instruction streams as they were: DESIGN.md section 8ac)
__device__ __forceinline__ float trapezoid_weight(int j, float zm, float z0, float zp, const int& S) {
  float w = 0.f;
  if (j >= 1) w += z0 - zm;
  if (j <= S - 3) w += zp - z0;
  return 0.5f * w;
}

// |o + d z| (base_tracing.py:102), summed as (x^2 + y^2) + z^2
__device__ __forceinline__ float sample_radius(float ox, float oy, float oz, float dx, float dy, float dz, float z) {
  const float px = ox + dx * z, py = oy + dy * z, pz = oz + dz * z;
  return sqrtf((px * px + py * py) + pz * pz);
}
