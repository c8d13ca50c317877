// Voxel-grid field with a time axis: values on the nodes of a grid at T frame times, gathered at the samples of a ray batch
// (or at free-standing points) at the time of their ray, and fitted through the adjoint scatter
// (include/sunerf_hip_ext.h: sunerf_dynamic_grid_*).
//
// The static field of grid_field.hip blended linearly between its two neighbouring frames, as MHDModel blends two simulation
// frames (sunerf/model/mhd_model.py:112-124).  A sample is located in space by the code of the static field (grid_locate.h)
// and in time by the same bisection on the fp64 frame times (dg_time); the temporal weights are rounded once, like the spatial
// ones.
//
// Forward: one lane per sample (index = ray * S + sample), 16 gathers of C values: the static kernel's nested trilinear
// expression on frame j and on frame j + 1, then wt_lo * lower + wt_hi * upper.  With `cells` / `weights` given it leaves
// id = j * n_cells + spatial cell and the eight weights (six spatial, two temporal) for the backward.
//
// The pieces of the forward, the backward's two kernels and their launcher are grid_gather.h with NT = 2, shared with
// grid_field.hip.
#include <hip/hip_runtime.h>
#include <math.h>

#include "../../include/sunerf_hip_ext.h"
#include "grid_gather.h"

namespace {

struct DgArgs : GgFwdArgs {                                         // values [T][n0][n1][n2][C]; points [M, 4]
  const double* frame_times; int T; int time_mode;
  const float* ray_times;                                           // ray mode
  int ncells;                                                       // cells of the grid; ids are interval * ncells + cell
};

// Interval j and weights (wt_lo = 1 - s, wt_hi = s) of the time t; false: a NaN, or outside the frames under SUNERF_TIME_FILL.
__device__ __forceinline__ bool dg_time(const double* tau, int T, int mode, float t, int& j, float& wt_lo, float& wt_hi) {
  const double td = (double)t;
  if (!(td == td)) return false;
  const double first = tau[0], last = tau[T - 1];
  if (td <= first) {
    if (td < first && mode == SUNERF_TIME_FILL) return false;
    j = 0; wt_lo = 1.f; wt_hi = 0.f;
    return true;
  }
  if (td >= last) {
    if (td > last && mode == SUNERF_TIME_FILL) return false;
    j = T - 2; wt_lo = 0.f; wt_hi = 1.f;
    return true;
  }
  j = gf_cell(tau, T, td);
  const double t0 = tau[j], t1 = tau[j + 1];
  const double s = (td - t0) / (t1 - t0);
  wt_lo = (float)(1.0 - s);
  wt_hi = (float)s;
  return true;
}

template <int C, bool RAYS>
__global__ __launch_bounds__(GF_THREADS) void dg_fwd_kernel(DgArgs a) {
  const int64_t idx = (int64_t)blockIdx.x * GF_THREADS + threadIdx.x;
  if (idx >= a.n * a.S) return;
  float p[3];
  const int64_t row = gg_point<RAYS>(a, idx, 4, p);
  const float t = RAYS ? a.ray_times[row] : a.points[row * 4 + 3];
  int i[3], j = 0;
  float wl[3], wh[3], wt_lo = 0.f, wt_hi = 0.f;
  const SunerfGridFieldDesc& g = a.g;
  float out[C];
  const bool inside = dg_time(a.frame_times, a.T, a.time_mode, t, j, wt_lo, wt_hi) && gf_locate(g, p[0], p[1], p[2], i, wl, wh);
  if (!inside) {
#pragma unroll
    for (int c = 0; c < C; ++c) out[c] = g.fill[c];
    if (a.cells) gg_write_sentinel<2>(a, idx, (a.T - 1) * a.ncells);
  } else {
    const int64_t frame = (int64_t)g.n[0] * g.n[1] * g.n[2] * C;
    float lower[C], upper[C];
    gg_trilinear<C>(g, a.values + (int64_t)j * frame, i, wl, wh, lower);
    gg_trilinear<C>(g, a.values + (int64_t)(j + 1) * frame, i, wl, wh, upper);
#pragma unroll
    for (int c = 0; c < C; ++c) out[c] = wt_lo * lower[c] + wt_hi * upper[c];
    if (a.cells) gg_write_index<2>(a, idx, j * a.ncells + gg_cell_id(g, i), wl, wh, wt_lo, wt_hi);
  }
#pragma unroll
  for (int c = 0; c < C; ++c) a.raw[idx * C + c] = out[c];
}

// status of the frame count and the id range of a checked descriptor; *ncells: the cells of the grid
int check_frames(const SunerfGridFieldDesc* g, int n_frames, int* ncells) {
  if (n_frames < 2) return SUNERF_E_BADARG;
  const int64_t cells = (int64_t)(g->n[0] - 1) * gf_cells_lon(*g) * (g->n[2] - 1);
  if ((int64_t)(n_frames - 1) * cells >= 0x7fffffff) return SUNERF_E_UNSUPPORTED;   // ids are int32, one more for the sentinel
  *ncells = (int)cells;
  return 0;
}

}  // namespace

extern "C" int sunerf_ext_abi_version(void) { return SUNERF_EXT_ABI_VERSION; }

extern "C" int sunerf_dynamic_grid_fwd(const SunerfGridFieldDesc* grid, const double* frame_times, int n_frames, int time_mode,
                                       const float* values, const float* rays_o, const float* rays_d, const float* z_vals,
                                       const float* ray_times, int64_t n_rays, int n_samples, const float* points,
                                       int point_stride, float* raw, int* cells, float* weights, void* stream) {
  int ncells = 0;
  int st = check_desc(grid);
  if (st) return st;
  if (n_frames < 2 || (time_mode != SUNERF_TIME_CLAMP && time_mode != SUNERF_TIME_FILL)) return SUNERF_E_BADARG;
  if (n_rays < 0 || n_samples < 1) return SUNERF_E_BADARG;
  if (points && (n_samples != 1 || point_stride != 4)) return SUNERF_E_BADARG;
  st = check_frames(grid, n_frames, &ncells);
  if (st) return st;
  if (n_rays == 0) return 0;
  if (!values || !raw || !frame_times || !grid->axis[0] || !grid->axis[1] || !grid->axis[2]) return SUNERF_E_BADARG;
  if (!points && (!rays_o || !rays_d || !z_vals || !ray_times)) return SUNERF_E_BADARG;
  if ((cells == nullptr) != (weights == nullptr)) return SUNERF_E_BADARG;
  const int64_t blocks = gg_fwd_blocks(n_rays, n_samples);
  if (blocks < 0) return SUNERF_E_UNSUPPORTED;
  const DgArgs a = {{*grid, values, rays_o, rays_d, z_vals, points, point_stride, n_rays, n_samples, raw, cells, weights},
                    frame_times, n_frames, time_mode, ray_times, ncells};
  SUNERF_CLEAR_ERROR();
  gg_for_channels(grid->n_channels, [&](auto c) {
    auto kernel = points ? dg_fwd_kernel<decltype(c)::value, false> : dg_fwd_kernel<decltype(c)::value, true>;
    hipLaunchKernelGGL(kernel, dim3((unsigned)blocks), dim3(GF_THREADS), 0, (hipStream_t)stream, a);
  });
  SUNERF_CHECK_LAUNCH();
  return 0;
}

extern "C" size_t sunerf_dynamic_grid_bwd_workspace_bytes(int64_t n_total, int n_channels) {
  return gg_workspace_bytes(n_total, n_channels, 2);
}

extern "C" int sunerf_dynamic_grid_bwd(const SunerfGridFieldDesc* grid, int n_frames, const float* g_raw, const int* cells,
                                       const float* weights, const int64_t* perm, const int64_t* seg_start, int64_t n_total,
                                       void* workspace, size_t workspace_bytes, float* g_values, int accumulate,
                                       void* stream) {
  int ncells = 0;
  int st = check_desc(grid);
  if (!st) st = check_frames(grid, n_frames, &ncells);
  if (st) return st;
  return gg_backward<2>(grid, n_frames, g_raw, cells, weights, perm, seg_start, n_total, workspace, workspace_bytes, g_values,
                        accumulate, (hipStream_t)stream);
}
