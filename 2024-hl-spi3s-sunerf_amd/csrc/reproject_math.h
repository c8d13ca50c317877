// The pinhole geometry that reprojection.hip and register.hip share (DESIGN.md sections 8g and 8aa): the fractional pixel of an
// angle on a monotone axis of pixel centres and the inverse rotation of a pose by cofactors.  All fp64; -ffp-contract=off gives
// the operations in the order they stand here.
#pragma once
#include <hip/hip_runtime.h>

namespace {

__device__ __forceinline__ double quiet_nan() { return __longlong_as_double(0x7ff8000000000000ll); }

// fractional pixel coordinate of angle t on an axis of n pixel centres (monotone; n >= 1)
__device__ __forceinline__ double axis_coord(const double* axis, int n, double t) {
  if (n == 1) return t == axis[0] ? 0. : quiet_nan();
  const bool ascending = axis[n - 1] > axis[0];
  int lo = 0, hi = n - 1;
  while (hi - lo > 1) {
    const int mid = (lo + hi) >> 1;
    const double a = axis[mid];
    if (ascending ? a <= t : a >= t) lo = mid; else hi = mid;
  }
  const double a0 = axis[lo], a1 = axis[lo + 1];
  return (double)lo + (t - a0) / (a1 - a0);
}

// cam = c2w[:3,:3]^-1 q by cofactors in fp64.  The fp32 pose is orthonormal to 1e-7 only: its transpose would put a pixel's own
// surface point 1e-5 pixels beside the pixel.  Rows a, b, c: the inverse's columns are b x c, c x a, a x b over det = a . (b x c).
__device__ __forceinline__ void inverse_rotate(const float* c2w, const double* q, double* cam) {
  const double a[3] = {(double)c2w[0], (double)c2w[1], (double)c2w[2]}, b[3] = {(double)c2w[4], (double)c2w[5], (double)c2w[6]},
               c[3] = {(double)c2w[8], (double)c2w[9], (double)c2w[10]};
  const double bc[3] = {b[1] * c[2] - b[2] * c[1], b[2] * c[0] - b[0] * c[2], b[0] * c[1] - b[1] * c[0]};
  const double ca[3] = {c[1] * a[2] - c[2] * a[1], c[2] * a[0] - c[0] * a[2], c[0] * a[1] - c[1] * a[0]};
  const double ab[3] = {a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0]};
  const double det = (a[0] * bc[0] + a[1] * bc[1]) + a[2] * bc[2];
#pragma unroll
  for (int i = 0; i < 3; ++i) cam[i] = ((bc[i] * q[0] + ca[i] * q[1]) + ab[i] * q[2]) / det;
}

}  // namespace
