// The arithmetic of prep.hip that is the same on the host and on the device: the spline poles and horizons, the mirror rule, the
// recursive filter of one line, scipy's B-spline weights and the tap sum of one output pixel.  All fp64, written so that
// -ffp-contract=off gives the operations in the order they stand here.
#pragma once
#include <math.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define PREP_HD __host__ __device__ __forceinline__
#else
#define PREP_HD inline
#endif

constexpr int PREP_MAX_ORDER = 5;
constexpr int PREP_SEGMENT = 128;        // outputs of one line that one thread filters
constexpr int PREP_LINES = 64;           // lines of a tile: one per lane of a wave
constexpr int PREP_MAX_HALO = 60;        // the largest sum of a row of PREP_HORIZON

// Horizon of every pole: the smallest K with |z|^K < 1e-17.  A recursion that starts K samples early with any bounded state
// carries less than 1e-17 of the line's maximum of that state into the first sample that is kept.  The first column is what
// the binding exports as prep.HORIZON (the largest pole's).
constexpr int PREP_HORIZON[PREP_MAX_ORDER + 1][2] = {{0, 0}, {0, 0}, {23, 0}, {30, 0}, {39, 10}, {47, 13}};

PREP_HD int prep_n_poles(int order) { return order < 2 ? 0 : (order < 4 ? 1 : 2); }
PREP_HD int prep_halo(int order) { return PREP_HORIZON[order][0] + PREP_HORIZON[order][1]; }

// scipy/ndimage/src/ni_splines.c: get_filter_poles (the same expressions; sqrt is correctly rounded on both sides)
inline void prep_poles(int order, double z[2]) {
  z[0] = z[1] = 0.;
  switch (order) {
    case 2: z[0] = sqrt(8.0) - 3.0; break;
    case 3: z[0] = sqrt(3.0) - 2.0; break;
    case 4:
      z[0] = sqrt(664.0 - sqrt(438976.0)) + sqrt(304.0) - 19.0;
      z[1] = sqrt(664.0 + sqrt(438976.0)) - sqrt(304.0) - 19.0;
      break;
    case 5:
      z[0] = sqrt(67.5 - sqrt(4436.25)) + sqrt(26.25) - 6.5;
      z[1] = sqrt(67.5 + sqrt(4436.25)) - sqrt(26.25) - 6.5;
      break;
    default: break;
  }
}
// ni_splines.c: filter_gain
inline double prep_gain(int order) {
  double z[2], gain = 1.0;
  prep_poles(order, z);
  for (int k = 0; k < prep_n_poles(order); ++k) gain *= (1.0 - z[k]) * (1.0 - 1.0 / z[k]);
  return gain;
}

// index of the mirrored signal (... 2 1 | 0 1 2 ... n-1 | n-2 ...) for any i, n >= 1
PREP_HD int prep_mirror(int64_t i, int n) {
  if (n <= 1) return 0;
  const int64_t period = 2 * (int64_t)n - 2;
  i %= period;
  if (i < 0) i += period;
  return (int)(i < n ? i : period - i);
}

// One line of `len` samples at T[0], T[stride], ... (already multiplied by the gain), filtered in place pole by pole with
// scipy's two recurrences (ni_splines.c: _apply_filter).  The causal state before T[0] is taken as 0 and the anticausal start is
// scipy's mirror formula: both are wrong by a bounded amount that the horizon removes from the samples that are kept.
PREP_HD void prep_filter_line(double* T, int stride, int len, int n_poles, double z0, double z1) {
  for (int k = 0; k < n_poles; ++k) {
    const double z = k == 0 ? z0 : z1;
    double c = T[0];
    for (int p = 1; p < len; ++p) {
      c = T[(int64_t)p * stride] + z * c;
      T[(int64_t)p * stride] = c;
    }
    c = (z * T[(int64_t)(len - 2) * stride] + c) * z / (z * z - 1.0);
    T[(int64_t)(len - 1) * stride] = c;
    for (int p = len - 2; p >= 0; --p) {
      c = z * (c - T[(int64_t)p * stride]);
      T[(int64_t)p * stride] = c;
    }
  }
}

// ni_splines.c: get_spline_interpolation_weights -- order + 1 weights of the taps start .. start + order around x
PREP_HD void prep_weights(double x, int order, double* w) {
  x -= floor((order & 1) ? x : x + 0.5);
  double y = x, z = 1.0 - x, t;
  switch (order) {
    case 1:
      w[0] = 1.0 - x;
      break;
    case 2:
      w[1] = 0.75 - x * x;
      y = 0.5 - x;
      w[0] = 0.5 * y * y;
      break;
    case 3:
      w[1] = (y * y * (y - 2.0) * 3.0 + 4.0) / 6.0;
      w[2] = (z * z * (z - 2.0) * 3.0 + 4.0) / 6.0;
      w[0] = z * z * z / 6.0;
      break;
    case 4:
      t = x * x;
      w[2] = t * (t * 0.25 - 0.625) + 115.0 / 192.0;
      y = 1.0 + x;
      w[1] = y * (y * (y * (5.0 - y) / 6.0 - 1.25) + 5.0 / 24.0) + 55.0 / 96.0;
      z = 1.0 - x;
      w[3] = z * (z * (z * (5.0 - z) / 6.0 - 1.25) + 5.0 / 24.0) + 55.0 / 96.0;
      y = 0.5 - x;
      t = y * y;
      w[0] = t * t / 24.0;
      break;
    case 5:
      t = y * y;
      w[2] = t * (t * (0.25 - y / 12.0) - 0.5) + 0.55;
      t = z * z;
      w[3] = t * (t * (0.25 - z / 12.0) - 0.5) + 0.55;
      y += 1.0;
      w[1] = y * (y * (y * (y * (y / 24.0 - 0.375) + 1.25) - 1.75) + 0.625) + 0.425;
      z += 1.0;
      w[4] = z * (z * (z * (z * (z / 24.0 - 0.375) + 1.25) - 1.75) + 0.625) + 0.425;
      z = 1.0 - x;
      t = z * z;
      w[0] = t * t * z / 120.0;
      break;
    default: break;
  }
  if (order >= 1) {
    double last = 1.0;
#pragma unroll
    for (int i = 0; i < order; ++i) last -= w[i];
    w[order] = last;
  }
}

PREP_HD int64_t prep_start(double c, int order) {
  return (int64_t)floor((order & 1) ? c : c + 0.5) - order / 2;
}

// The value of one output pixel whose source coordinate is (cy, cx) (0-based, row and column) on `coef` [H][W], as
// scipy.ndimage.affine_transform(mode='constant') forms it: `outside` when a coordinate leaves [0, n-1], else the sum over the
// (order+1)^2 taps, rows outermost, of (coef * wy) * wx, taps past the edge taken at their mirrored index.  `hit` says whether
// a tap read a pixel whose mask byte is set (mask may be null).
template <int order>
PREP_HD double prep_sample(const double* coef, const uint8_t* mask, int H, int W, double cy, double cx, bool* outside,
                           bool* hit) {
  *hit = false;
  *outside = cy < 0.0 || cy > (double)(H - 1) || cx < 0.0 || cx > (double)(W - 1) || cy != cy || cx != cx;
  if (*outside) return 0.0;
  const int64_t sy = prep_start(cy, order), sx = prep_start(cx, order);
  double wy[PREP_MAX_ORDER + 1], wx[PREP_MAX_ORDER + 1];
  int ix[PREP_MAX_ORDER + 1];
  if (order > 0) {
    prep_weights(cy, order, wy);
    prep_weights(cx, order, wx);
  }
#pragma unroll
  for (int j = 0; j <= order; ++j) ix[j] = prep_mirror(sx + j, W);
  double t = 0.0;
#pragma unroll
  for (int i = 0; i <= order; ++i) {
    const int64_t row = (int64_t)prep_mirror(sy + i, H) * W;
#pragma unroll
    for (int j = 0; j <= order; ++j) {
      double c = coef[row + ix[j]];
      if (mask && mask[row + ix[j]]) *hit = true;
      if (order > 0) {
        c *= wy[i];
        c *= wx[j];
      }
      t += c;
    }
  }
  return t;
}

// Order-preserving image of an fp32 bit pattern: a < b as floats <=> key(a) < key(b) as unsigned (-0.0 below +0.0)
PREP_HD uint32_t prep_key(uint32_t bits) { return (bits & 0x80000000u) ? ~bits : (bits | 0x80000000u); }
PREP_HD uint32_t prep_unkey(uint32_t key) { return (key & 0x80000000u) ? (key ^ 0x80000000u) : ~key; }
PREP_HD bool prep_is_nan_bits(uint32_t bits) { return (bits & 0x7fffffffu) > 0x7f800000u; }
