// Heliographic analyses: radial columns cast outward from the solar surface, one per (latitude,
// longitude), and the column statistics the fused emission integral does not produce.
//
// The stash scripts of the reference's sunerf/evaluation/stash/ (topographical_map.py:36-66, topographical_profile.py:33-58,
// topographical_slice.py:119-140, eruption_profile.py:76-101) all build the points u(lat, lon) r_j of a fixed radial grid
// r_j on the host and reduce the fine model's output along each column.  Here a column is a ray of the fused render kernel:
//   rays_o = 0,  rays_d = fp32(u),  z_j = r_j / Rs_per_ds,  u(b, l) = (-cos b sin l, cos b cos l, -sin b)
// with b, l the latitude / longitude of SuNeRFLoader.render_observer_image: u is the unit vector towards the observer that
// pose_spherical(-l, b, d) places (train/coordinate_transformation.py:36-54), so the column lies straight below it.
//
// column_rays_kernel  : one thread per column; u in fp64, rounded to fp32; 28 bytes written per column.
// column_stats_kernel : one wave64 per column; reads raw (S, 2) and the shared z row, reduces in fp32.
#include "sunerf_common.h"
#include "ray_scan.h"
#include "../../include/sunerf_hip.h"

namespace {

struct ColumnRayArgs {
  const double* lat; const double* lon;
  int per_column, n_lon;
  int64_t col_begin, n_cols;
  float* rays_o; float* rays_d;
  float* times; float time_value;
};

__global__ __launch_bounds__(256) void column_rays_kernel(ColumnRayArgs a) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= a.n_cols) return;
  const int64_t p = a.col_begin + i;
  const double b = a.per_column ? a.lat[p] : a.lat[p / a.n_lon];    // grid: row 0 = first latitude (south)
  const double l = a.per_column ? a.lon[p] : a.lon[p % a.n_lon];    //       column 0 = first longitude
  const double cb = cos(b), sb = sin(b), cl = cos(l), sl = sin(l);
  a.rays_d[i * 3 + 0] = (float)(-cb * sl);
  a.rays_d[i * 3 + 1] = (float)(cb * cl);
  a.rays_d[i * 3 + 2] = (float)(-sb);
#pragma unroll
  for (int r = 0; r < 3; ++r) a.rays_o[i * 3 + r] = 0.f;
  if (a.times) a.times[i] = a.time_value;
}

constexpr int CS_THREADS = 256;            // 4 columns per workgroup
constexpr int CS_COLS = CS_THREADS / 64;

struct ColumnStatArgs {
  const float* raw; const float* z; const float* rays_d;
  int64_t n_cols; int S;
  float height_scale;
  float* emission_height; float* emission_column;
  float* emission; float* absorption;
};

__global__ __launch_bounds__(CS_THREADS) void column_stats_kernel(ColumnStatArgs a) {
  const int lane = threadIdx.x & 63;
  const int64_t col = (int64_t)blockIdx.x * CS_COLS + (threadIdx.x >> 6);
  if (col >= a.n_cols) return;                                       // the whole wave leaves together
  const float dx = a.rays_d[col * 3 + 0], dy = a.rays_d[col * 3 + 1], dz = a.rays_d[col * 3 + 2];
  const float dnorm = sqrtf((dx * dx + dy * dy) + dz * dz);          // the integral's |rays_d| (emission.py:26)
  const int S = a.S;
  const float* raw = a.raw + col * (int64_t)S * 2;
  float s_e = 0.f, s_re = 0.f, s_col = 0.f;
  for (int j = lane; j < S; j += 64) {
    const float zj = a.z[j];
    const float dzv = (j == 0) ? (a.z[1] - zj) : (zj - a.z[j - 1]);  // first interval duplicated (emission.py:21-22)
    const float dr = dzv * dnorm;
    const float e = expf(raw[2 * j]);                                // topographical_profile.py:55
    s_e += e;
    s_re += (zj * dnorm) * e;                                        // |p_j| = z_j |u| (the column starts at the centre)
    s_col += e * dr;
    if (a.emission) {
      const int64_t o = col * S + j;
      a.emission[o] = e;
      a.absorption[o] = 1.f - expf(-fmaxf(raw[2 * j + 1], 0.f) * dr);   // eruption_profile.py:93
    }
  }
  s_e = sum64(s_e); s_re = sum64(s_re); s_col = sum64(s_col);
  if (lane == 0) {
    a.emission_height[col] = a.height_scale * (s_re / s_e);            // topographical_profile.py:57
    a.emission_column[col] = s_col;
  }
}

}  // namespace

extern "C" int sunerf_column_rays(const double* lat, const double* lon, int per_column, int n_lon, int64_t col_begin,
                                  int64_t n_cols, float time_value, float* rays_o, float* rays_d, float* times, void* stream) {
  if (n_cols < 0 || col_begin < 0 || n_lon < 1) return SUNERF_E_BADARG;
  if (n_cols == 0) return 0;
  if (!lat || !lon || !rays_o || !rays_d) return SUNERF_E_BADARG;
  ColumnRayArgs a;
  a.lat = lat; a.lon = lon; a.per_column = per_column != 0; a.n_lon = n_lon; a.col_begin = col_begin; a.n_cols = n_cols;
  a.rays_o = rays_o; a.rays_d = rays_d; a.times = times; a.time_value = time_value;
  SUNERF_CLEAR_ERROR();
  hipLaunchKernelGGL(column_rays_kernel, dim3((unsigned)((n_cols + 255) / 256)), dim3(256), 0, (hipStream_t)stream, a);
  SUNERF_CHECK_LAUNCH();
  return 0;
}

extern "C" int sunerf_column_stats(const float* raw, const float* z_row, const float* rays_d, int64_t n_cols, int n_samples,
                                   float height_scale, float* emission_height, float* emission_column, float* emission,
                                   float* absorption, void* stream) {
  if (n_cols < 0 || n_samples < 2) return SUNERF_E_BADARG;
  if (n_cols == 0) return 0;
  if (!raw || !z_row || !rays_d || !emission_height || !emission_column) return SUNERF_E_BADARG;
  if ((emission == nullptr) != (absorption == nullptr)) return SUNERF_E_BADARG;
  ColumnStatArgs a;
  a.raw = raw; a.z = z_row; a.rays_d = rays_d; a.n_cols = n_cols; a.S = n_samples; a.height_scale = height_scale;
  a.emission_height = emission_height; a.emission_column = emission_column; a.emission = emission; a.absorption = absorption;
  SUNERF_CLEAR_ERROR();
  hipLaunchKernelGGL(column_stats_kernel, dim3((unsigned)((n_cols + CS_COLS - 1) / CS_COLS)), dim3(CS_THREADS), 0,
                     (hipStream_t)stream, a);
  SUNERF_CHECK_LAUNCH();
  return 0;
}
