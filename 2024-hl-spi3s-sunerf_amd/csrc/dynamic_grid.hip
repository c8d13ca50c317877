// Voxel-grid field with a time axis: values on the nodes of a grid at T frame times, gathered at the samples of a ray batch
// (or at free-standing points) at the time of their ray, and fitted through the adjoint scatter
// (include/sunerf_hip_ext.h: sunerf_dynamic_grid_*).
//
// The static field of grid_field.hip blended linearly between its two neighbouring frames, as MHDModel blends two simulation
// frames (sunerf/model/mhd_model.py:112-124).  A sample is located in space by the code of the static field (grid_locate.h)
// and in time by the same bisection on the fp64 frame times; the temporal weights are rounded once, like the spatial ones.
//
// Forward: one lane per sample (index = ray * S + sample), 16 gathers of C values: the static kernel's nested trilinear
// expression on frame j and on frame j + 1, then wt_lo * lower + wt_hi * upper.  With `cells` / `weights` given it leaves
// id = j * n_cells + spatial cell and the eight weights (six spatial, two temporal) for the backward.
//
// Backward: the sorted inverted index of grid_field.hip over the ids (interval, cell); no floating-point atomics.  One thread
// per (frame f, node) adds interval f - 1 (upper temporal weight) and then interval f (lower), in each the node's up to 8
// adjacent cells in the static kernel's order and each segment in the permutation's order.  A segment longer than DG_CHUNK
// goes through the piece kernel: one wave per 64 sorted positions, two slots per piece (the id of its first position and the id
// of its last), a fixed butterfly over the 16 C partial sums (2 frames x 8 corners x C); the node thread adds the pieces in
// position order.  Every sum has one order: reruns are bit-identical.
#include <hip/hip_runtime.h>
#include <math.h>

#include "sunerf_common.h"
#include "../../include/sunerf_hip_ext.h"
#include "grid_locate.h"

namespace {

constexpr int DG_THREADS = 256;
constexpr int DG_CHUNK = 64;                 // sorted positions per piece of a long segment = one wave

struct DgArgs {
  SunerfGridFieldDesc g;
  const double* frame_times; int T; int time_mode;
  const float* values;                                              // [T][n0][n1][n2][C]
  const float* rays_o; const float* rays_d; const float* z_vals; const float* ray_times;    // ray mode
  const float* points;                                              // points mode: [M, 4]
  int64_t n; int S;                                                 // rays x samples, or points x 1
  int ncells;                                                       // cells of the grid; ids are interval * ncells + cell
  float* raw; int* cells; float* weights;
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
__global__ __launch_bounds__(DG_THREADS) void dg_fwd_kernel(DgArgs a) {
  const int64_t idx = (int64_t)blockIdx.x * DG_THREADS + threadIdx.x;
  if (idx >= a.n * a.S) return;
  float x, y, z, t;
  if (RAYS) {
    const int64_t ray = idx / a.S;
    const float zz = a.z_vals[idx];
    x = a.rays_o[ray * 3 + 0] + a.rays_d[ray * 3 + 0] * zz;       // sampling.py:100; -ffp-contract=off: multiply, then add
    y = a.rays_o[ray * 3 + 1] + a.rays_d[ray * 3 + 1] * zz;
    z = a.rays_o[ray * 3 + 2] + a.rays_d[ray * 3 + 2] * zz;
    t = a.ray_times[ray];
  } else {
    const float* p = a.points + idx * 4;
    x = p[0]; y = p[1]; z = p[2]; t = p[3];
  }
  int i[3], j = 0;
  float wl[3], wh[3], wt_lo = 0.f, wt_hi = 0.f;
  const SunerfGridFieldDesc& g = a.g;
  float out[C];
  const bool inside = dg_time(a.frame_times, a.T, a.time_mode, t, j, wt_lo, wt_hi) && gf_locate(g, x, y, z, i, wl, wh);
  if (!inside) {
#pragma unroll
    for (int c = 0; c < C; ++c) out[c] = g.fill[c];
    if (a.cells) {
      a.cells[idx] = (a.T - 1) * a.ncells;                              // the sentinel: sorts behind every id
#pragma unroll
      for (int k = 0; k < 8; ++k) a.weights[idx * 8 + k] = 0.f;
    }
  } else {
    const int n1 = g.n[1], n2 = g.n[2];
    const int j1 = i[1] + 1 == n1 ? 0 : i[1] + 1;                       // (n1 only in the wrap cell)
    const int64_t r00 = (((int64_t)i[0] * n1 + i[1]) * n2 + i[2]) * C;  // (node 0, node 1) rows; + C: the next radius / z node
    const int64_t r01 = (((int64_t)i[0] * n1 + j1) * n2 + i[2]) * C;
    const int64_t r10 = (((int64_t)(i[0] + 1) * n1 + i[1]) * n2 + i[2]) * C;
    const int64_t r11 = (((int64_t)(i[0] + 1) * n1 + j1) * n2 + i[2]) * C;
    const int64_t frame = (int64_t)g.n[0] * n1 * n2 * C;
    float tri[2][C];
#pragma unroll
    for (int f = 0; f < 2; ++f) {
      const float* v = a.values + (int64_t)(j + f) * frame;
#pragma unroll
      for (int c = 0; c < C; ++c) {
        const float a00 = wl[2] * v[r00 + c] + wh[2] * v[r00 + C + c], a01 = wl[2] * v[r01 + c] + wh[2] * v[r01 + C + c];
        const float a10 = wl[2] * v[r10 + c] + wh[2] * v[r10 + C + c], a11 = wl[2] * v[r11 + c] + wh[2] * v[r11 + C + c];
        tri[f][c] = wl[0] * (wl[1] * a00 + wh[1] * a01) + wh[0] * (wl[1] * a10 + wh[1] * a11);
      }
    }
#pragma unroll
    for (int c = 0; c < C; ++c) out[c] = wt_lo * tri[0][c] + wt_hi * tri[1][c];
    if (a.cells) {
      a.cells[idx] = j * a.ncells + ((i[0] * gf_cells_lon(g) + i[1]) * (n2 - 1) + i[2]);
#pragma unroll
      for (int k = 0; k < 3; ++k) { a.weights[idx * 8 + 2 * k] = wl[k]; a.weights[idx * 8 + 2 * k + 1] = wh[k]; }
      a.weights[idx * 8 + 6] = wt_lo;
      a.weights[idx * 8 + 7] = wt_hi;
    }
  }
#pragma unroll
  for (int c = 0; c < C; ++c) a.raw[idx * C + c] = out[c];
}

struct DgBwdArgs {
  int n[3], nc[3];
  int wrap;                          // open periodic longitude: cell nc[1] - 1 joins node n[1] - 1 to node 0
  int ncells;                        // cells of the grid
  int T;
  int nids;                          // (T - 1) * ncells: the sentinel
  const float* g_raw; const int* cells; const float* weights;
  const int64_t* perm; const int64_t* seg;
  int64_t total;
  float* part;                       // [pieces][2 slots][2 frames][8 corners][C]
  float* g_values; int accumulate;
};

// weight of corner (dt, d0, d1, d2) of sample s: d = 1 is the upper node of the axis, dt = 1 the upper frame of the interval
__device__ __forceinline__ float dg_corner_weight(const float* w, int64_t s, int dt, int d0, int d1, int d2) {
  return ((w[s * 8 + d0] * w[s * 8 + 2 + d1]) * w[s * 8 + 4 + d2]) * w[s * 8 + 6 + dt];
}

template <int C>
__global__ __launch_bounds__(DG_THREADS) void dg_chunk_kernel(DgBwdArgs a) {
  const int64_t q = ((int64_t)blockIdx.x * DG_THREADS + threadIdx.x) / DG_CHUNK;
  const int lane = threadIdx.x & (DG_CHUNK - 1);
  const int64_t first = q * DG_CHUNK;
  if (first >= a.total) return;                                        // (the whole wave)
  const int64_t left = a.total - first;
  const int last_lane = left >= DG_CHUNK ? DG_CHUNK - 1 : (int)left - 1;
  const bool valid = lane <= last_lane;
  const int64_t s = valid ? a.perm[first + lane] : 0;
  const int id = valid ? a.cells[s] : a.nids;
  const int cf = __shfl(id, 0), cl = __shfl(id, last_lane);
  for (int slot = 0; slot < 2; ++slot) {                               // wave-uniform control flow throughout
    const int target = slot ? cl : cf;
    if (slot == 1 && cl == cf) break;
    if (target < 0 || target >= a.nids) continue;                      // samples outside the grid or the frames
    if (a.seg[target + 1] - a.seg[target] <= DG_CHUNK) continue;       // a short segment: the node thread walks it
    float v[16 * C];
    const bool mine = id == target;
    float g[C];
#pragma unroll
    for (int c = 0; c < C; ++c) g[c] = mine ? a.g_raw[s * C + c] : 0.f;
#pragma unroll
    for (int k = 0; k < 16; ++k) {                                     // k = dt * 8 + corner
      const float w = mine ? dg_corner_weight(a.weights, s, k >> 3, (k >> 2) & 1, (k >> 1) & 1, k & 1) : 0.f;
#pragma unroll
      for (int c = 0; c < C; ++c) v[k * C + c] = w * g[c];
    }
#pragma unroll
    for (int m = DG_CHUNK / 2; m >= 1; m >>= 1) {
#pragma unroll
      for (int k = 0; k < 16 * C; ++k) v[k] += __shfl_xor(v[k], m);
    }
    if (lane == 0) {
      float* dst = a.part + (q * 2 + slot) * 16 * C;
#pragma unroll
      for (int k = 0; k < 16 * C; ++k) dst[k] = v[k];
    }
  }
}

template <int C>
__global__ __launch_bounds__(DG_THREADS) void dg_node_kernel(DgBwdArgs a) {
  const int64_t tid = (int64_t)blockIdx.x * DG_THREADS + threadIdx.x;
  const int64_t nodes = (int64_t)a.n[0] * a.n[1] * a.n[2];
  if (tid >= nodes * a.T) return;
  const int f = (int)(tid / nodes);
  const int64_t node = tid % nodes;
  const int j2 = (int)(node % a.n[2]);
  const int64_t rest = node / a.n[2];
  const int j1 = (int)(rest % a.n[1]), j0 = (int)(rest / a.n[1]);
  float acc[C];
#pragma unroll
  for (int c = 0; c < C; ++c) acc[c] = 0.f;
  for (int dt = 1; dt >= 0; --dt) {                                    // interval f - 1 (this frame is its upper), then f
    const int interval = f - dt;
    if (interval < 0 || interval > a.T - 2) continue;
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
          const int id = interval * a.ncells + ((c0 * a.nc[1] + c1) * a.nc[2] + c2);
          const int64_t begin = a.seg[id], end = a.seg[id + 1];
          if (end - begin <= DG_CHUNK) {
            for (int64_t p = begin; p < end; ++p) {
              const int64_t s = a.perm[p];
              const float w = dg_corner_weight(a.weights, s, dt, d0, d1, d2);
#pragma unroll
              for (int c = 0; c < C; ++c) acc[c] += w * a.g_raw[s * C + c];
            }
          } else {
            const int k = dt * 8 + d0 * 4 + d1 * 2 + d2;
            for (int64_t q = begin / DG_CHUNK; q <= (end - 1) / DG_CHUNK; ++q) {
              const int slot = begin <= q * DG_CHUNK ? 0 : 1;           // the piece's first position is this id's, or not
              const float* src = a.part + ((q * 2 + slot) * 16 + k) * C;
#pragma unroll
              for (int c = 0; c < C; ++c) acc[c] += src[c];
            }
          }
        }
      }
    }
  }
#pragma unroll
  for (int c = 0; c < C; ++c) {
    float* dst = a.g_values + tid * C + c;
    *dst = a.accumulate ? *dst + acc[c] : acc[c];
  }
}

// status of the frame count and the id range of a checked descriptor; *ncells: the cells of the grid
int check_frames(const SunerfGridFieldDesc* g, int n_frames, int* ncells) {
  if (n_frames < 2) return SUNERF_E_BADARG;
  const int64_t cells = (int64_t)(g->n[0] - 1) * gf_cells_lon(*g) * (g->n[2] - 1);
  if ((int64_t)(n_frames - 1) * cells >= 0x7fffffff) return SUNERF_E_UNSUPPORTED;   // ids are int32, one more for the sentinel
  *ncells = (int)cells;
  return 0;
}

template <int C>
void launch_fwd(const DgArgs& a, unsigned blocks, hipStream_t stream) {
  if (a.points)
    hipLaunchKernelGGL((dg_fwd_kernel<C, false>), dim3(blocks), dim3(DG_THREADS), 0, stream, a);
  else
    hipLaunchKernelGGL((dg_fwd_kernel<C, true>), dim3(blocks), dim3(DG_THREADS), 0, stream, a);
}

template <int C>
void launch_bwd(const DgBwdArgs& a, unsigned chunk_blocks, unsigned node_blocks, hipStream_t stream) {
  if (chunk_blocks) hipLaunchKernelGGL((dg_chunk_kernel<C>), dim3(chunk_blocks), dim3(DG_THREADS), 0, stream, a);
  hipLaunchKernelGGL((dg_node_kernel<C>), dim3(node_blocks), dim3(DG_THREADS), 0, stream, a);
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
  const int64_t blocks = (n_rays * n_samples + DG_THREADS - 1) / DG_THREADS;
  if (blocks > 0x7fffffff) return SUNERF_E_UNSUPPORTED;
  DgArgs a = {};
  a.g = *grid; a.frame_times = frame_times; a.T = n_frames; a.time_mode = time_mode; a.values = values;
  a.rays_o = rays_o; a.rays_d = rays_d; a.z_vals = z_vals; a.ray_times = ray_times; a.points = points;
  a.n = n_rays; a.S = n_samples; a.ncells = ncells; a.raw = raw; a.cells = cells; a.weights = weights;
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

extern "C" size_t sunerf_dynamic_grid_bwd_workspace_bytes(int64_t n_total, int n_channels) {
  if (n_total <= 0 || n_channels < 1) return 0;
  return (size_t)((n_total + DG_CHUNK - 1) / DG_CHUNK) * 2 * 16 * (size_t)n_channels * sizeof(float);
}

extern "C" int sunerf_dynamic_grid_bwd(const SunerfGridFieldDesc* grid, int n_frames, const float* g_raw, const int* cells,
                                       const float* weights, const int64_t* perm, const int64_t* seg_start, int64_t n_total,
                                       void* workspace, size_t workspace_bytes, float* g_values, int accumulate,
                                       void* stream) {
  int ncells = 0;
  int st = check_desc(grid);
  if (!st) st = check_frames(grid, n_frames, &ncells);
  if (st) return st;
  if (n_total < 0) return SUNERF_E_BADARG;
  if (!g_values) return SUNERF_E_BADARG;
  const int64_t nodes = (int64_t)grid->n[0] * grid->n[1] * grid->n[2];
  if (n_total == 0) {
    if (!accumulate) {
      hipError_t e = hipMemsetAsync(g_values, 0, (size_t)n_frames * nodes * grid->n_channels * sizeof(float), (hipStream_t)stream);
      if (e != hipSuccess) return (int)e;
    }
    return 0;
  }
  if (!g_raw || !cells || !weights || !perm || !seg_start || !workspace) return SUNERF_E_BADARG;
  if (workspace_bytes < sunerf_dynamic_grid_bwd_workspace_bytes(n_total, grid->n_channels)) return SUNERF_E_WORKSPACE;
  const int64_t chunk_blocks = ((n_total + DG_CHUNK - 1) / DG_CHUNK * DG_CHUNK + DG_THREADS - 1) / DG_THREADS;
  const int64_t node_blocks = (nodes * n_frames + DG_THREADS - 1) / DG_THREADS;
  if (chunk_blocks > 0x7fffffff || node_blocks > 0x7fffffff) return SUNERF_E_UNSUPPORTED;
  DgBwdArgs a = {};
  for (int k = 0; k < 3; ++k) { a.n[k] = grid->n[k]; a.nc[k] = grid->n[k] - 1; }
  a.nc[1] = gf_cells_lon(*grid);
  a.wrap = grid->lon_mode == SUNERF_GRID_LON_OPEN;
  a.ncells = ncells; a.T = n_frames; a.nids = (n_frames - 1) * ncells;
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
