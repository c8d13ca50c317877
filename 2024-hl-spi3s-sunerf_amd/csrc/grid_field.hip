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
// weights are formed in fp64 from the fp32 point (as thomson.hip forms its geometry) and rounded once to fp32; the
// interpolation is fp32.  A cell is found by bisection on the fp64 axis (at most ceil(log2 n) probes of an array that stays
// in cache): the rule of numpy.searchsorted(axis, u, 'left') - 1 clipped to [0, n - 2], for uniform and non-uniform axes alike.
// With `cells` / `weights` given, the forward also leaves every sample's flattened cell id and its six weights for the backward.
//
// Backward: no floating-point atomics.  The caller sorts the cell ids (stable) and hands the permutation and the start of
// every cell's segment in it.  A node's gradient is the sum over its (up to 8) adjacent cells, in a fixed order, of the
// samples of that cell's segment, in the permutation's order: one thread per node (gf_node_kernel).  A segment longer than
// GF_CHUNK samples is not walked by that one thread: the sorted positions are cut at the multiples of GF_CHUNK, one wave
// per piece sums the piece's samples of a long cell with a fixed butterfly (gf_chunk_kernel), and the node thread adds the
// pieces in position order.  A piece holds the samples of at most two long cells -- the one its first position belongs to
// (slot 0) and the one its last position belongs to (slot 1) -- because a long segment cannot lie strictly inside a piece.
// Every sum has a fixed order: reruns are bit-identical.
#include <hip/hip_runtime.h>
#include <math.h>

#include "sunerf_common.h"
#include "../../include/sunerf_hip.h"
#include "grid_locate.h"

namespace {

constexpr int GF_THREADS = 256;
constexpr int GF_CHUNK = 64;                 // sorted positions per piece of a long segment = one wave

struct GfArgs {
  SunerfGridFieldDesc g;
  const float* values;
  const float* rays_o; const float* rays_d; const float* z_vals;    // ray mode
  const float* points; int stride;                                  // points mode: [M, stride], stride 3 or 4
  int64_t n; int S;                                                 // rays x samples, or points x 1
  float* raw; int* cells; float* weights;
};

template <int C, bool RAYS>
__global__ __launch_bounds__(GF_THREADS) void gf_fwd_kernel(GfArgs a) {
  const int64_t idx = (int64_t)blockIdx.x * GF_THREADS + threadIdx.x;
  if (idx >= a.n * a.S) return;
  float x, y, z;
  if (RAYS) {
    const int64_t ray = idx / a.S;
    const float zz = a.z_vals[idx];
    x = a.rays_o[ray * 3 + 0] + a.rays_d[ray * 3 + 0] * zz;       // sampling.py:100; -ffp-contract=off: multiply, then add
    y = a.rays_o[ray * 3 + 1] + a.rays_d[ray * 3 + 1] * zz;
    z = a.rays_o[ray * 3 + 2] + a.rays_d[ray * 3 + 2] * zz;
  } else {
    const float* p = a.points + idx * a.stride;
    x = p[0]; y = p[1]; z = p[2];
  }
  int i[3];
  float wl[3], wh[3];
  const SunerfGridFieldDesc& g = a.g;
  float out[C];
  if (!gf_locate(g, x, y, z, i, wl, wh)) {
#pragma unroll
    for (int c = 0; c < C; ++c) out[c] = g.fill[c];
    if (a.cells) {
      a.cells[idx] = (g.n[0] - 1) * gf_cells_lon(g) * (g.n[2] - 1);    // the sentinel: sorts behind every cell
#pragma unroll
      for (int k = 0; k < 3; ++k) { a.weights[idx * 6 + 2 * k] = 0.f; a.weights[idx * 6 + 2 * k + 1] = 0.f; }
    }
  } else {
    const int n1 = g.n[1], n2 = g.n[2];
    const int j1 = i[1] + 1 == n1 ? 0 : i[1] + 1;                       // (n1 only in the wrap cell)
    const int64_t r00 = (((int64_t)i[0] * n1 + i[1]) * n2 + i[2]) * C;  // (node 0, node 1) rows; + C: the next radius / z node
    const int64_t r01 = (((int64_t)i[0] * n1 + j1) * n2 + i[2]) * C;
    const int64_t r10 = (((int64_t)(i[0] + 1) * n1 + i[1]) * n2 + i[2]) * C;
    const int64_t r11 = (((int64_t)(i[0] + 1) * n1 + j1) * n2 + i[2]) * C;
    const float* v = a.values;
#pragma unroll
    for (int c = 0; c < C; ++c) {
      const float a00 = wl[2] * v[r00 + c] + wh[2] * v[r00 + C + c], a01 = wl[2] * v[r01 + c] + wh[2] * v[r01 + C + c];
      const float a10 = wl[2] * v[r10 + c] + wh[2] * v[r10 + C + c], a11 = wl[2] * v[r11 + c] + wh[2] * v[r11 + C + c];
      out[c] = wl[0] * (wl[1] * a00 + wh[1] * a01) + wh[0] * (wl[1] * a10 + wh[1] * a11);
    }
    if (a.cells) {
      a.cells[idx] = (i[0] * gf_cells_lon(g) + i[1]) * (n2 - 1) + i[2];
#pragma unroll
      for (int k = 0; k < 3; ++k) { a.weights[idx * 6 + 2 * k] = wl[k]; a.weights[idx * 6 + 2 * k + 1] = wh[k]; }
    }
  }
#pragma unroll
  for (int c = 0; c < C; ++c) a.raw[idx * C + c] = out[c];
}

struct GfBwdArgs {
  int n[3], nc[3];
  int wrap;                          // open periodic longitude: cell nc[1] - 1 joins node n[1] - 1 to node 0
  int ncells;
  const float* g_raw; const int* cells; const float* weights;
  const int64_t* perm; const int64_t* seg;
  int64_t total;
  float* part;                       // [pieces][2 slots][8 corners][C]
  float* g_values; int accumulate;
};

// weight of corner (d0, d1, d2) of sample s: d = 1 is the upper node of the axis
__device__ __forceinline__ float gf_corner_weight(const float* w, int64_t s, int d0, int d1, int d2) {
  return (w[s * 6 + d0] * w[s * 6 + 2 + d1]) * w[s * 6 + 4 + d2];
}

template <int C>
__global__ __launch_bounds__(GF_THREADS) void gf_chunk_kernel(GfBwdArgs a) {
  const int64_t q = ((int64_t)blockIdx.x * GF_THREADS + threadIdx.x) / GF_CHUNK;
  const int lane = threadIdx.x & (GF_CHUNK - 1);
  const int64_t first = q * GF_CHUNK;
  if (first >= a.total) return;                                        // (the whole wave)
  const int64_t left = a.total - first;
  const int last_lane = left >= GF_CHUNK ? GF_CHUNK - 1 : (int)left - 1;
  const bool valid = lane <= last_lane;
  const int64_t s = valid ? a.perm[first + lane] : 0;
  const int cell = valid ? a.cells[s] : a.ncells;
  const int cf = __shfl(cell, 0), cl = __shfl(cell, last_lane);
  for (int slot = 0; slot < 2; ++slot) {                               // wave-uniform control flow throughout
    const int target = slot ? cl : cf;
    if (slot == 1 && cl == cf) break;
    if (target >= a.ncells) continue;                                  // samples outside the grid
    if (a.seg[target + 1] - a.seg[target] <= GF_CHUNK) continue;       // a short segment: the node thread walks it
    float v[8 * C];
    const bool mine = cell == target;
    float g[C];
#pragma unroll
    for (int c = 0; c < C; ++c) g[c] = mine ? a.g_raw[s * C + c] : 0.f;
#pragma unroll
    for (int corner = 0; corner < 8; ++corner) {
      const float w = mine ? gf_corner_weight(a.weights, s, corner >> 2, (corner >> 1) & 1, corner & 1) : 0.f;
#pragma unroll
      for (int c = 0; c < C; ++c) v[corner * C + c] = w * g[c];
    }
#pragma unroll
    for (int m = GF_CHUNK / 2; m >= 1; m >>= 1) {
#pragma unroll
      for (int k = 0; k < 8 * C; ++k) v[k] += __shfl_xor(v[k], m);
    }
    if (lane == 0) {
      float* dst = a.part + (q * 2 + slot) * 8 * C;
#pragma unroll
      for (int k = 0; k < 8 * C; ++k) dst[k] = v[k];
    }
  }
}

template <int C>
__global__ __launch_bounds__(GF_THREADS) void gf_node_kernel(GfBwdArgs a) {
  const int64_t node = (int64_t)blockIdx.x * GF_THREADS + threadIdx.x;
  if (node >= (int64_t)a.n[0] * a.n[1] * a.n[2]) return;
  const int j2 = (int)(node % a.n[2]);
  const int64_t rest = node / a.n[2];
  const int j1 = (int)(rest % a.n[1]), j0 = (int)(rest / a.n[1]);
  float acc[C];
#pragma unroll
  for (int c = 0; c < C; ++c) acc[c] = 0.f;
  for (int d0 = 0; d0 < 2; ++d0) {
    const int c0 = j0 - d0;
    if (c0 < 0 || c0 >= a.nc[0]) continue;
    for (int d1 = 0; d1 < 2; ++d1) {
      int c1 = j1 - d1;
      if (c1 < 0) {
        if (!a.wrap) continue;
        c1 = a.nc[1] - 1;
      }
      if (c1 >= a.nc[1]) continue;
      for (int d2 = 0; d2 < 2; ++d2) {
        const int c2 = j2 - d2;
        if (c2 < 0 || c2 >= a.nc[2]) continue;
        const int cell = (c0 * a.nc[1] + c1) * a.nc[2] + c2;
        const int64_t begin = a.seg[cell], end = a.seg[cell + 1];
        if (end - begin <= GF_CHUNK) {
          for (int64_t p = begin; p < end; ++p) {
            const int64_t s = a.perm[p];
            const float w = gf_corner_weight(a.weights, s, d0, d1, d2);
#pragma unroll
            for (int c = 0; c < C; ++c) acc[c] += w * a.g_raw[s * C + c];
          }
        } else {
          const int corner = d0 * 4 + d1 * 2 + d2;
          for (int64_t q = begin / GF_CHUNK; q <= (end - 1) / GF_CHUNK; ++q) {
            const int slot = begin <= q * GF_CHUNK ? 0 : 1;             // the piece's first position is this cell's, or not
            const float* src = a.part + ((q * 2 + slot) * 8 + corner) * C;
#pragma unroll
            for (int c = 0; c < C; ++c) acc[c] += src[c];
          }
        }
      }
    }
  }
#pragma unroll
  for (int c = 0; c < C; ++c) {
    float* dst = a.g_values + node * C + c;
    *dst = a.accumulate ? *dst + acc[c] : acc[c];
  }
}

template <int C>
void launch_fwd(const GfArgs& a, unsigned blocks, hipStream_t stream) {
  if (a.points)
    hipLaunchKernelGGL((gf_fwd_kernel<C, false>), dim3(blocks), dim3(GF_THREADS), 0, stream, a);
  else
    hipLaunchKernelGGL((gf_fwd_kernel<C, true>), dim3(blocks), dim3(GF_THREADS), 0, stream, a);
}

template <int C>
void launch_bwd(const GfBwdArgs& a, unsigned chunk_blocks, unsigned node_blocks, hipStream_t stream) {
  if (chunk_blocks) hipLaunchKernelGGL((gf_chunk_kernel<C>), dim3(chunk_blocks), dim3(GF_THREADS), 0, stream, a);
  hipLaunchKernelGGL((gf_node_kernel<C>), dim3(node_blocks), dim3(GF_THREADS), 0, stream, a);
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
  const int64_t blocks = (n_rays * n_samples + GF_THREADS - 1) / GF_THREADS;
  if (blocks > 0x7fffffff) return SUNERF_E_UNSUPPORTED;
  GfArgs a = {};
  a.g = *grid; a.values = values; a.rays_o = rays_o; a.rays_d = rays_d; a.z_vals = z_vals; a.points = points;
  a.stride = point_stride; a.n = n_rays; a.S = n_samples; a.raw = raw; a.cells = cells; a.weights = weights;
  SUNERF_CLEAR_ERROR();
  switch (grid->n_channels) {
    case 1: launch_fwd<1>(a, (unsigned)blocks, (hipStream_t)stream); break;
    case 2: launch_fwd<2>(a, (unsigned)blocks, (hipStream_t)stream); break;
    case 3: launch_fwd<3>(a, (unsigned)blocks, (hipStream_t)stream); break;
    default: launch_fwd<4>(a, (unsigned)blocks, (hipStream_t)stream); break;
  }
  SUNERF_CHECK_LAUNCH();
  return 0;
}

extern "C" size_t sunerf_grid_field_bwd_workspace_bytes(int64_t n_total, int n_channels) {
  if (n_total <= 0 || n_channels < 1) return 0;
  return (size_t)((n_total + GF_CHUNK - 1) / GF_CHUNK) * 2 * 8 * (size_t)n_channels * sizeof(float);
}

extern "C" int sunerf_grid_field_bwd(const SunerfGridFieldDesc* grid, const float* g_raw, const int* cells,
                                     const float* weights, const int64_t* perm, const int64_t* seg_start, int64_t n_total,
                                     void* workspace, size_t workspace_bytes, float* g_values, int accumulate, void* stream) {
  const int st = check_desc(grid);
  if (st) return st;
  if (n_total < 0) return SUNERF_E_BADARG;
  if (!g_values) return SUNERF_E_BADARG;
  const int64_t nodes = (int64_t)grid->n[0] * grid->n[1] * grid->n[2];
  if (n_total == 0) {
    if (!accumulate) {
      hipError_t e = hipMemsetAsync(g_values, 0, (size_t)nodes * grid->n_channels * sizeof(float), (hipStream_t)stream);
      if (e != hipSuccess) return (int)e;
    }
    return 0;
  }
  if (!g_raw || !cells || !weights || !perm || !seg_start || !workspace) return SUNERF_E_BADARG;
  if (workspace_bytes < sunerf_grid_field_bwd_workspace_bytes(n_total, grid->n_channels)) return SUNERF_E_WORKSPACE;
  const int64_t chunk_blocks = ((n_total + GF_CHUNK - 1) / GF_CHUNK * GF_CHUNK + GF_THREADS - 1) / GF_THREADS;
  const int64_t node_blocks = (nodes + GF_THREADS - 1) / GF_THREADS;
  if (chunk_blocks > 0x7fffffff || node_blocks > 0x7fffffff) return SUNERF_E_UNSUPPORTED;
  GfBwdArgs a = {};
  for (int k = 0; k < 3; ++k) { a.n[k] = grid->n[k]; a.nc[k] = grid->n[k] - 1; }
  a.nc[1] = gf_cells_lon(*grid);
  a.wrap = grid->lon_mode == SUNERF_GRID_LON_OPEN;
  a.ncells = a.nc[0] * a.nc[1] * a.nc[2];
  a.g_raw = g_raw; a.cells = cells; a.weights = weights; a.perm = perm; a.seg = seg_start; a.total = n_total;
  a.part = (float*)workspace; a.g_values = g_values; a.accumulate = accumulate;
  SUNERF_CLEAR_ERROR();
  switch (grid->n_channels) {
    case 1: launch_bwd<1>(a, (unsigned)chunk_blocks, (unsigned)node_blocks, (hipStream_t)stream); break;
    case 2: launch_bwd<2>(a, (unsigned)chunk_blocks, (unsigned)node_blocks, (hipStream_t)stream); break;
    case 3: launch_bwd<3>(a, (unsigned)chunk_blocks, (unsigned)node_blocks, (hipStream_t)stream); break;
    default: launch_bwd<4>(a, (unsigned)chunk_blocks, (unsigned)node_blocks, (hipStream_t)stream); break;
  }
  SUNERF_CHECK_LAUNCH();
  return 0;
}
