// The emission / absorption integral along a ray (EmissionRadiativeTransfer.raw2outputs, emission.py:14-54): the step that
// the epilogue fused behind the MLP (render_fwd.hip) and integral_fwd_kernel (render_bwd.hip) take per 32-sample chunk.
// Sweep 1 of integral_bwd_kernel (render_bwd.hip) is the same arithmetic in that kernel's own text: called from there the
// step cost it a register and 3 % of its time.
//
//   dist_i = (z_i - z_{i-1}) |d|, the first one duplicated              (emission.py:19-26)
//   a_i    = exp(-relu(r1_i) dist_i)
//   T_i    = prod_{k < i} (a_k + 1e-10)                                 exclusive; chunk-wise scan with a scalar carry
//   em_i   = (exp(r0_i) dist_i) T_i,   image = sum_i em_i,   weights_i = em_i / (image + 1e-10)
//
// Layout: 32 lanes per ray, lane n = sample 32 c + n of chunk c.  The expressions and their order are fixed (the build uses
// -ffp-contract=off): the two callers give the same bits on the same raw (tests/test_gpu_emission_integral.py).
#pragma once
#include "ray_scan.h"

struct EmissionCarry {
  float T = 1.f;      // product of (a + 1e-10) over all previous samples of the ray
  float z = 0.f;      // z of the previous chunk's last sample
};
struct EmissionStep {
  float dist, a, em;  // em = 0 on lanes past the ray's end; dist and a are computed there too (on the last sample's z), unread
};

// One chunk.  `z`: this lane's z (lanes past S: any finite value, callers give the last sample's), `first`: z_1 - z_0, read by
// sample 0 only (the caller knows where its z live: registers in the fused kernel, memory in the stand-alone ones).
__device__ __forceinline__ EmissionStep emission_step(EmissionCarry& k, float z, float first, float r0, float r1, float dnorm,
                                                      int i, int n, bool valid) {
  float zprev = __shfl_up(z, 1, 32);
  if (n == 0) zprev = k.z;
  const float dzv = (i == 0) ? first : (z - zprev);
  EmissionStep o;
  o.dist = dzv * dnorm;
  o.a = expf(-fmaxf(r1, 0.f) * o.dist);
  const float pr = scan_mul_up32(valid ? (o.a + 1e-10f) : 1.f, n);
  float excl = __shfl_up(pr, 1, 32);
  if (n == 0) excl = 1.f;
  o.em = valid ? (expf(r0) * o.dist) * (k.T * excl) : 0.f;
  k.T *= __shfl(pr, 31, 32);
  k.z = __shfl(z, 31, 32);
  return o;
}

// weights = em / (sum em + 1e-10) (emission.py:49-50) on one ray's row: every lane finalises the un-normalised em it stored itself
__device__ __forceinline__ void emission_normalise(float* w, int S, int n, float denom) {
  const int n_chunks = (S + 31) >> 5;
  for (int c = 0; c < n_chunks; ++c) {
    const int i = 32 * c + n;
    if (i < S) w[i] = w[i] / denom;
  }
}
