// Voxel-grid field: values on the nodes of a grid, gathered at the samples of a ray batch (or at free-standing points) and
// fitted through the adjoint scatter (include/sunerf_hip.h: sunerf_grid_field_*).
//
// Generalises the trilinear gather of MHDModel, sunerf/model/mhd_model.py:45-75 (scipy RegularGridInterpolator per variable on
// the CPU; csrc/mhd.hip is its device form for PSI's layout), to any grid of sunerf_hip/volume.py -- the cube of the reference's
// sunerf/evaluation/stash/voxel_volume.py:30-44 included -- with 1 to 4 channels per node, and adds the gradient w.r.t. the
// node values, which neither has.
//
// Forward: one lane per sample, the samples of a ray in neighbouring lanes (index = ray * S + sample, as mhd.hip), so that the
// 8 gathers of a wave walk through neighbouring cells.  The sample's grid coordinates, its cell and its three pairs of
// weights are formed in fp64 from the fp32 point (as thomson.hip forms its geometry) and rounded once to fp32 (grid_locate.h);
// the interpolation is fp32.  A cell is found by bisection on the fp64 axis (at most ceil(log2 n) probes of an array that stays
// in cache): the rule of numpy.searchsorted(axis, u, 'left') - 1 clipped to [0, n - 2], for uniform and non-uniform axes alike.
// With `cells` / `weights` given, the forward also leaves every sample's flattened cell id and its six weights for the backward.
//
// The pieces of the forward, the backward's two kernels and their launcher are grid_gather.h with NT = 1, shared with
// dynamic_grid.hip.
#include <hip/hip_runtime.h>
#include <math.h>

#include "../../include/sunerf_hip.h"
#include "grid_gather.h"

namespace {

template <int C, bool RAYS>
__global__ __launch_bounds__(GF_THREADS) void gf_fwd_kernel(GgFwdArgs a) {
  const int64_t idx = (int64_t)blockIdx.x * GF_THREADS + threadIdx.x;
  if (idx >= a.n * a.S) return;
  float p[3];
  gg_point<RAYS>(a, idx, a.stride, p);
  int i[3];
  float wl[3], wh[3];
  const SunerfGridFieldDesc& g = a.g;
  float out[C];
  if (!gf_locate(g, p[0], p[1], p[2], i, wl, wh)) {
#pragma unroll
    for (int c = 0; c < C; ++c) out[c] = g.fill[c];
    if (a.cells) gg_write_sentinel<1>(a, idx, (g.n[0] - 1) * gf_cells_lon(g) * (g.n[2] - 1));
  } else {
    gg_trilinear<C>(g, a.values, i, wl, wh, out);
    if (a.cells) gg_write_index<1>(a, idx, gg_cell_id(g, i), wl, wh);
  }
#pragma unroll
  for (int c = 0; c < C; ++c) a.raw[idx * C + c] = out[c];
}

}  // namespace

extern "C" size_t sunerf_grid_field_desc_bytes(void) { return sizeof(SunerfGridFieldDesc); }

extern "C" int sunerf_grid_field_fwd(const SunerfGridFieldDesc* grid, const float* values, const float* rays_o,
                                     const float* rays_d, const float* z_vals, int64_t n_rays, int n_samples,
                                     const float* points, int point_stride, float* raw, int* cells, float* weights,
                                     void* stream) {
  const int st = check_desc(grid);
  if (st) return st;
  if (n_rays < 0 || n_samples < 1) return SUNERF_E_BADARG;
  if (points && (n_samples != 1 || (point_stride != 3 && point_stride != 4))) return SUNERF_E_BADARG;
  if (n_rays == 0) return 0;
  if (!values || !raw || !grid->axis[0] || !grid->axis[1] || !grid->axis[2]) return SUNERF_E_BADARG;
  if (!points && (!rays_o || !rays_d || !z_vals)) return SUNERF_E_BADARG;
  if ((cells == nullptr) != (weights == nullptr)) return SUNERF_E_BADARG;
  const int64_t blocks = gg_fwd_blocks(n_rays, n_samples);
  if (blocks < 0) return SUNERF_E_UNSUPPORTED;
  const GgFwdArgs a = {*grid, values, rays_o, rays_d, z_vals, points, point_stride, n_rays, n_samples, raw, cells, weights};
  SUNERF_CLEAR_ERROR();
  gg_for_channels(grid->n_channels, [&](auto c) {
    auto kernel = points ? gf_fwd_kernel<decltype(c)::value, false> : gf_fwd_kernel<decltype(c)::value, true>;
    hipLaunchKernelGGL(kernel, dim3((unsigned)blocks), dim3(GF_THREADS), 0, (hipStream_t)stream, a);
  });
  SUNERF_CHECK_LAUNCH();
  return 0;
}

extern "C" size_t sunerf_grid_field_bwd_workspace_bytes(int64_t n_total, int n_channels) {
  return gg_workspace_bytes(n_total, n_channels, 1);
}

extern "C" int sunerf_grid_field_bwd(const SunerfGridFieldDesc* grid, const float* g_raw, const int* cells,
                                     const float* weights, const int64_t* perm, const int64_t* seg_start, int64_t n_total,
                                     void* workspace, size_t workspace_bytes, float* g_values, int accumulate, void* stream) {
  const int st = check_desc(grid);
  if (st) return st;
  return gg_backward<1>(grid, 1, g_raw, cells, weights, perm, seg_start, n_total, workspace, workspace_bytes, g_values,
                        accumulate, (hipStream_t)stream);
}
