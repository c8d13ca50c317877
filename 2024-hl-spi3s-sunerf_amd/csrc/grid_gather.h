// The trilinear gather of a voxel-grid field and its adjoint scatter, once for the static field (grid_field.hip, NT = 1) and the
// field with a time axis (dynamic_grid.hip, NT = 2): NT is the number of frames a sample touches, C the channels per node (1 to
// 4).  DESIGN.md sections 8j and 8l.
//
// Forward (the kernels stay with their entry points; one lane per sample, index = ray * S + sample): gg_point forms the sample,
// grid_locate.h finds its cell and its three pairs of weights, gg_trilinear is the nested fp32 expression on one frame -- called
// once by the static kernel, on frames j and j + 1 by the dynamic one, which then forms wt_lo * lower + wt_hi * upper -- and
// gg_write_index leaves id = interval * n_cells + cell (interval 0 for NT = 1) and the 4 + 2 NT weights of the sample (wl, wh
// per axis, then per frame) for the backward; gg_write_sentinel, for a sample outside, the number of ids and zero weights.
//
// Backward: no floating-point atomics.  The caller sorts the ids (stable) and hands the permutation and the start of every
// id's segment in it.  One thread per (frame f, node) (gg_node_kernel) adds, for NT = 2, interval f - 1 (the frame is its upper
// one) and then interval f, for NT = 1 the one interval; in each the node's (up to 8) adjacent cells in the order d0, d1, d2,
// each segment in the permutation's order.  A segment longer than GF_CHUNK samples is not walked by that one thread: the sorted
// positions are cut at the multiples of GF_CHUNK, one wave per piece sums the piece's samples of a long segment with a fixed
// butterfly over its 8 NT C partial sums (gg_chunk_kernel), and the node thread adds the pieces in position order.  A piece
// holds the samples of at most two long segments -- the one its first position belongs to (slot 0) and the one its last
// position belongs to (slot 1) -- because a long segment cannot lie strictly inside a piece.  Every sum has a fixed order:
// reruns are bit-identical.
#pragma once
#include <type_traits>

#include "sunerf_common.h"
#include "grid_locate.h"

namespace {

constexpr int GF_THREADS = 256;
constexpr int GF_CHUNK = 64;                 // sorted positions per piece of a long segment = one wave

// ---- forward -------------------------------------------------------------------------------------------------------------------
struct GgFwdArgs {
  SunerfGridFieldDesc g;
  const float* values;                                              // [n0][n1][n2][C], NT = 2: [T] of them
  const float* rays_o; const float* rays_d; const float* z_vals;    // ray mode
  const float* points; int stride;                                  // points mode: [M, stride]
  int64_t n; int S;                                                 // rays x samples, or points x 1
  float* raw; int* cells; float* weights;
};

// The point p of sample idx: o + d z of its ray, or the row idx of `points`.  Returns the ray, or the row.
template <bool RAYS>
__device__ __forceinline__ int64_t gg_point(const GgFwdArgs& a, int64_t idx, int stride, float p[3]) {
  if (RAYS) {
    const int64_t ray = idx / a.S;
    const float zz = a.z_vals[idx];
#pragma unroll
    for (int k = 0; k < 3; ++k) p[k] = a.rays_o[ray * 3 + k] + a.rays_d[ray * 3 + k] * zz;    // sampling.py:100; -ffp-contract=off: multiply, then add
    return ray;
  }
  const float* row = a.points + idx * stride;
  p[0] = row[0]; p[1] = row[1]; p[2] = row[2];
  return idx;
}

// out[c] of the frame v [n0][n1][n2][C] in the cell i with the weights (wl, wh) of gf_locate
template <int C>
__device__ __forceinline__ void gg_trilinear(const SunerfGridFieldDesc& g, const float* v, const int i[3], const float wl[3],
                                             const float wh[3], float out[C]) {
  const int n1 = g.n[1], n2 = g.n[2];
  const int j1 = i[1] + 1 == n1 ? 0 : i[1] + 1;                       // (n1 only in the wrap cell)
  const int64_t r00 = (((int64_t)i[0] * n1 + i[1]) * n2 + i[2]) * C;  // (node 0, node 1) rows; + C: the next radius / z node
  const int64_t r01 = (((int64_t)i[0] * n1 + j1) * n2 + i[2]) * C;
  const int64_t r10 = (((int64_t)(i[0] + 1) * n1 + i[1]) * n2 + i[2]) * C;
  const int64_t r11 = (((int64_t)(i[0] + 1) * n1 + j1) * n2 + i[2]) * C;
#pragma unroll
  for (int c = 0; c < C; ++c) {
    const float a00 = wl[2] * v[r00 + c] + wh[2] * v[r00 + C + c], a01 = wl[2] * v[r01 + c] + wh[2] * v[r01 + C + c];
    const float a10 = wl[2] * v[r10 + c] + wh[2] * v[r10 + C + c], a11 = wl[2] * v[r11 + c] + wh[2] * v[r11 + C + c];
    out[c] = wl[0] * (wl[1] * a00 + wh[1] * a01) + wh[0] * (wl[1] * a10 + wh[1] * a11);
  }
}

__device__ __forceinline__ int gg_cell_id(const SunerfGridFieldDesc& g, const int i[3]) {
  return (i[0] * gf_cells_lon(g) + i[1]) * (g.n[2] - 1) + i[2];
}

// The id and the 4 + 2 NT weights of the inside sample idx; wt: the NT = 2 frame pair.
template <int NT>
__device__ __forceinline__ void gg_write_index(const GgFwdArgs& a, int64_t idx, int id, const float wl[3], const float wh[3],
                                               float wt_lo = 0.f, float wt_hi = 0.f) {
  constexpr int W = 4 + 2 * NT;
#pragma unroll
  for (int k = 0; k < 3; ++k) { a.weights[idx * W + 2 * k] = wl[k]; a.weights[idx * W + 2 * k + 1] = wh[k]; }
  if constexpr (NT == 2) { a.weights[idx * W + 6] = wt_lo; a.weights[idx * W + 7] = wt_hi; }
  a.cells[idx] = id;
}

// A sample outside: the sentinel id, which sorts behind every other, and all-zero weights.
template <int NT>
__device__ __forceinline__ void gg_write_sentinel(const GgFwdArgs& a, int64_t idx, int sentinel) {
  constexpr int W = 4 + 2 * NT;
  a.cells[idx] = sentinel;
#pragma unroll
  for (int k = 0; k < W; ++k) a.weights[idx * W + k] = 0.f;
}

// ---- backward ------------------------------------------------------------------------------------------------------------------
struct GgBwdArgs {
  int n[3], nc[3];
  int wrap;                          // open periodic longitude: cell nc[1] - 1 joins node n[1] - 1 to node 0
  int ncells;                        // cells of the grid
  int T;                             // frames (NT = 1: one)
  int nids;                          // intervals * ncells: the sentinel
  const float* g_raw; const int* cells; const float* weights;
  const int64_t* perm; const int64_t* seg;
  int64_t total;
  float* part;                       // [pieces][2 slots][NT frames][8 corners][C]
  float* g_values; int accumulate;
};

// weight of corner (dt, d0, d1, d2) of sample s: d = 1 is the upper node of the axis, dt = 1 the upper frame of the interval
template <int NT>
__device__ __forceinline__ float gg_corner_weight(const float* w, int64_t s, int dt, int d0, int d1, int d2) {
  constexpr int W = 4 + 2 * NT;
  const float space = (w[s * W + d0] * w[s * W + 2 + d1]) * w[s * W + 4 + d2];
  if constexpr (NT == 2) return space * w[s * W + 6 + dt];
  else return space;
}

template <int C, int NT>
__global__ __launch_bounds__(GF_THREADS) void gg_chunk_kernel(GgBwdArgs a) {
  constexpr int K = 8 * NT;                                            // k = dt * 8 + corner
  const int64_t q = ((int64_t)blockIdx.x * GF_THREADS + threadIdx.x) / GF_CHUNK;
  const int lane = threadIdx.x & (GF_CHUNK - 1);
  const int64_t first = q * GF_CHUNK;
  if (first >= a.total) return;                                        // (the whole wave)
  const int64_t left = a.total - first;
  const int last_lane = left >= GF_CHUNK ? GF_CHUNK - 1 : (int)left - 1;
  const bool valid = lane <= last_lane;
  const int64_t s = valid ? a.perm[first + lane] : 0;
  const int id = valid ? a.cells[s] : a.nids;
  const int cf = __shfl(id, 0), cl = __shfl(id, last_lane);
  for (int slot = 0; slot < 2; ++slot) {                               // wave-uniform control flow throughout
    const int target = slot ? cl : cf;
    if (slot == 1 && cl == cf) break;
    if (target < 0 || target >= a.nids) continue;                      // samples outside the grid or the frames
    if (a.seg[target + 1] - a.seg[target] <= GF_CHUNK) continue;       // a short segment: the node thread walks it
    float v[K * C];
    const bool mine = id == target;
    float g[C];
#pragma unroll
    for (int c = 0; c < C; ++c) g[c] = mine ? a.g_raw[s * C + c] : 0.f;
#pragma unroll
    for (int k = 0; k < K; ++k) {
      const float w = mine ? gg_corner_weight<NT>(a.weights, s, k >> 3, (k >> 2) & 1, (k >> 1) & 1, k & 1) : 0.f;
#pragma unroll
      for (int c = 0; c < C; ++c) v[k * C + c] = w * g[c];
    }
#pragma unroll
    for (int m = GF_CHUNK / 2; m >= 1; m >>= 1) {
#pragma unroll
      for (int k = 0; k < K * C; ++k) v[k] += __shfl_xor(v[k], m);
    }
    if (lane == 0) {
      float* dst = a.part + (q * 2 + slot) * K * C;
#pragma unroll
      for (int k = 0; k < K * C; ++k) dst[k] = v[k];
    }
  }
}

template <int C, int NT>
__global__ __launch_bounds__(GF_THREADS) void gg_node_kernel(GgBwdArgs a) {
  const int64_t tid = (int64_t)blockIdx.x * GF_THREADS + threadIdx.x;
  const int64_t nodes = (int64_t)a.n[0] * a.n[1] * a.n[2];
  if (tid >= nodes * a.T) return;
  int f = 0;
  int64_t node = tid;
  if constexpr (NT == 2) { f = (int)(tid / nodes); node = tid % nodes; }
  const int j2 = (int)(node % a.n[2]);
  const int64_t rest = node / a.n[2];
  const int j1 = (int)(rest % a.n[1]), j0 = (int)(rest / a.n[1]);
  float acc[C];
#pragma unroll
  for (int c = 0; c < C; ++c) acc[c] = 0.f;
  for (int dt = NT - 1; dt >= 0; --dt) {                               // NT = 2: interval f - 1 (this frame is its upper), then f
    int interval = 0;
    if constexpr (NT == 2) {
      interval = f - dt;
      if (interval < 0 || interval > a.T - 2) continue;
    }
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
          if (end - begin <= GF_CHUNK) {
            for (int64_t p = begin; p < end; ++p) {
              const int64_t s = a.perm[p];
              const float w = gg_corner_weight<NT>(a.weights, s, dt, d0, d1, d2);
#pragma unroll
              for (int c = 0; c < C; ++c) acc[c] += w * a.g_raw[s * C + c];
            }
          } else {
            const int k = dt * 8 + d0 * 4 + d1 * 2 + d2;
            for (int64_t q = begin / GF_CHUNK; q <= (end - 1) / GF_CHUNK; ++q) {
              const int slot = begin <= q * GF_CHUNK ? 0 : 1;           // the piece's first position is this id's, or not
              const float* src = a.part + ((q * 2 + slot) * 8 * NT + k) * C;
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

// ---- host ----------------------------------------------------------------------------------------------------------------------
// f(std::integral_constant<int, C>) for the channel count of a checked descriptor
template <class F>
void gg_for_channels(int n_channels, F&& f) {
  switch (n_channels) {
    case 1: f(std::integral_constant<int, 1>()); break;
    case 2: f(std::integral_constant<int, 2>()); break;
    case 3: f(std::integral_constant<int, 3>()); break;
    default: f(std::integral_constant<int, 4>()); break;
  }
}

// blocks of GF_THREADS over the samples of a forward, or -1: more than a launch takes
inline int64_t gg_fwd_blocks(int64_t n_rays, int n_samples) {
  const int64_t blocks = (n_rays * n_samples + GF_THREADS - 1) / GF_THREADS;
  return blocks > 0x7fffffff ? -1 : blocks;
}

inline size_t gg_workspace_bytes(int64_t n_total, int n_channels, int NT) {
  if (n_total <= 0 || n_channels < 1) return 0;
  return (size_t)((n_total + GF_CHUNK - 1) / GF_CHUNK) * 2 * 8 * NT * (size_t)n_channels * sizeof(float);
}

// The backward of a checked descriptor (NT = 2: and a checked n_frames; NT = 1: n_frames is 1), from the sizes on.
template <int NT>
int gg_backward(const SunerfGridFieldDesc* grid, int n_frames, const float* g_raw, const int* cells, const float* weights,
                const int64_t* perm, const int64_t* seg_start, int64_t n_total, void* workspace, size_t workspace_bytes,
                float* g_values, int accumulate, hipStream_t stream) {
  if (n_total < 0) return SUNERF_E_BADARG;
  if (!g_values) return SUNERF_E_BADARG;
  const int64_t nodes = (int64_t)grid->n[0] * grid->n[1] * grid->n[2];
  if (n_total == 0) {
    if (!accumulate) {
      hipError_t e = hipMemsetAsync(g_values, 0, (size_t)n_frames * nodes * grid->n_channels * sizeof(float), stream);
      if (e != hipSuccess) return (int)e;
    }
    return 0;
  }
  if (!g_raw || !cells || !weights || !perm || !seg_start || !workspace) return SUNERF_E_BADARG;
  if (workspace_bytes < gg_workspace_bytes(n_total, grid->n_channels, NT)) return SUNERF_E_WORKSPACE;
  const int64_t chunk_blocks = ((n_total + GF_CHUNK - 1) / GF_CHUNK * GF_CHUNK + GF_THREADS - 1) / GF_THREADS;
  const int64_t node_blocks = (nodes * n_frames + GF_THREADS - 1) / GF_THREADS;
  if (chunk_blocks > 0x7fffffff || node_blocks > 0x7fffffff) return SUNERF_E_UNSUPPORTED;
  GgBwdArgs a = {};
  for (int k = 0; k < 3; ++k) { a.n[k] = grid->n[k]; a.nc[k] = grid->n[k] - 1; }
  a.nc[1] = gf_cells_lon(*grid);
  a.wrap = grid->lon_mode == SUNERF_GRID_LON_OPEN;
  a.ncells = a.nc[0] * a.nc[1] * a.nc[2];
  a.T = n_frames; a.nids = (n_frames - NT + 1) * a.ncells;             // one interval, or T - 1
  a.g_raw = g_raw; a.cells = cells; a.weights = weights; a.perm = perm; a.seg = seg_start; a.total = n_total;
  a.part = (float*)workspace; a.g_values = g_values; a.accumulate = accumulate;
  SUNERF_CLEAR_ERROR();
  gg_for_channels(grid->n_channels, [&](auto c) {
    constexpr int C = decltype(c)::value;
    hipLaunchKernelGGL((gg_chunk_kernel<C, NT>), dim3((unsigned)chunk_blocks), dim3(GF_THREADS), 0, stream, a);
    hipLaunchKernelGGL((gg_node_kernel<C, NT>), dim3((unsigned)node_blocks), dim3(GF_THREADS), 0, stream, a);
  });
  SUNERF_CHECK_LAUNCH();
  return 0;
}

}  // namespace
