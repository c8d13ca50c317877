// Where a sample lies on a grid of sunerf_hip/volume.py: coordinates, cell, the three pairs of weights and the inside test
// (include/sunerf_hip.h: SunerfGridFieldDesc).  Shared by the static field (grid_field.hip) and the field with a time axis
// (dynamic_grid.hip), so that both locate a sample with the same code.
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>

#include "../../include/sunerf_hip.h"

namespace {

constexpr double GF_TWO_PI = 6.283185307179586;

__host__ __device__ inline int gf_cells_lon(const SunerfGridFieldDesc& g) {
  return g.lon_mode == SUNERF_GRID_LON_OPEN ? g.n[1] : g.n[1] - 1;
}

// searchsorted(a, u, 'left') - 1 clipped to [0, n - 2]: a[i] < u <= a[i + 1] inside the axis
__device__ __forceinline__ int gf_cell(const double* a, int n, double u) {
  int lo = 0, hi = n;
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if (a[mid] < u) lo = mid + 1; else hi = mid;
  }
  const int i = lo - 1;
  return i < 0 ? 0 : (i > n - 2 ? n - 2 : i);
}

// Cell i[3] and weights (wl = 1 - t, wh = t per axis) of the point p [model units]; false: outside the grid or a NaN coordinate.
__device__ __forceinline__ bool gf_locate(const SunerfGridFieldDesc& g, float px, float py, float pz, int i[3], float wl[3],
                                          float wh[3]) {
  const double X = (double)px * g.Rs_per_ds, Y = (double)py * g.Rs_per_ds, Z = (double)pz * g.Rs_per_ds;
  double u[3];
  bool periodic = false;
  if (g.kind == SUNERF_GRID_AFFINE) {
    const double dx = X - g.origin[0], dy = Y - g.origin[1], dz = Z - g.origin[2];
#pragma unroll
    for (int m = 0; m < 3; ++m) u[m] = (g.inverse[m][0] * dx + g.inverse[m][1] * dy) + g.inverse[m][2] * dz;
  } else {
    // inverse of X = r (-cos b sin l, cos b cos l, -sin b) (sunerf_grid_points): b = asin(-Z / r), l = atan2(-X, Y)
    const double r = sqrt((X * X + Y * Y) + Z * Z);
    double s = -Z / r;
    if (s > 1.0) s = 1.0;
    if (s < -1.0) s = -1.0;                                  // (a NaN stays a NaN)
    u[0] = asin(s);
    double l = atan2(-X, Y);
    l = l - GF_TWO_PI * floor((l - g.lo[1]) / GF_TWO_PI);    // into [lon[0], lon[0] + 2 pi)
    if (l < g.lo[1]) l += GF_TWO_PI;
    if (l >= g.lo[1] + GF_TWO_PI) l -= GF_TWO_PI;
    u[1] = l;
    u[2] = r;
    periodic = g.lon_mode != SUNERF_GRID_LON_PATCH;
  }
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    if (k == 1 && periodic) {
      if (!(u[1] == u[1])) return false;
    } else if (!(u[k] >= g.lo[k] && u[k] <= g.hi[k])) {
      return false;
    }
  }
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    const double* a = g.axis[k];
    const int n = g.n[k];
    double t;
    if (k == 1 && g.lon_mode == SUNERF_GRID_LON_OPEN && g.kind == SUNERF_GRID_SPHERICAL && u[1] > g.hi[1]) {
      i[1] = n - 1;                                           // the wrap cell: last node -> first node + 2 pi
      t = (u[1] - g.hi[1]) / ((g.lo[1] + GF_TWO_PI) - g.hi[1]);
    } else {
      i[k] = gf_cell(a, n, u[k]);
      const double a0 = a[i[k]], a1 = a[i[k] + 1];
      t = (u[k] - a0) / (a1 - a0);
    }
    wl[k] = (float)(1.0 - t);
    wh[k] = (float)t;
  }
  return true;
}

// status of a descriptor, before anything touches the device
int check_desc(const SunerfGridFieldDesc* g) {
  if (!g) return SUNERF_E_BADARG;
  if (g->n_channels < 1) return SUNERF_E_BADARG;
  if (g->n_channels > SUNERF_GRID_FIELD_MAX_CHANNELS) return SUNERF_E_UNSUPPORTED;
  if (g->kind != SUNERF_GRID_AFFINE && g->kind != SUNERF_GRID_SPHERICAL) return SUNERF_E_BADARG;
  if (g->lon_mode < SUNERF_GRID_LON_PATCH || g->lon_mode > SUNERF_GRID_LON_OPEN) return SUNERF_E_BADARG;
  if (g->kind == SUNERF_GRID_AFFINE && g->lon_mode != SUNERF_GRID_LON_PATCH) return SUNERF_E_BADARG;
  for (int k = 0; k < 3; ++k)
    if (g->n[k] < 2) return SUNERF_E_BADARG;                            // a plane, an axis of one node: no cell
  if (!(g->Rs_per_ds > 0.0)) return SUNERF_E_BADARG;
  const int64_t cells = (int64_t)(g->n[0] - 1) * gf_cells_lon(*g) * (g->n[2] - 1);
  if (cells >= 0x7fffffff) return SUNERF_E_UNSUPPORTED;                 // cell ids are int32, one more for the sentinel
  return 0;
}
}  // namespace
