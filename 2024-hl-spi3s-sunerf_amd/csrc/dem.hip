// Line-of-sight differential emission measure of the density / temperature model: DEM(log T) per ray on a caller-given
// log T grid, total emission measure, emission-measure-weighted log T and column density.
//
// Restates the forward of the DT integral (dt_sweep.h forward_sweep; density_temperature.py:237-265) with the response folded
// out: with rho = exp(relu(raw0 + base_rho)), logT = relu(raw1 + base_T) and, for the quadrature points j = 0..S-2,
//   q_j = trapezoid weight of z_j on the grid z_0..z_{S-2}
//   t_j = exp(-A_{j+1}),  A = cumulative_trapezoid(rho relu(log_abs), z)            (the render's own index shift, :261-263)
//   m_j = [r_in <= |o + d z_j| <= r_out]
//   v_j = q_j t_j m_j rho_j^2
// every v_j is deposited onto the two nodes around logT_j with linear ("hat") weights,
//   i = clamp(searchsorted(nodes, logT_j, right) - 1, 0, K-2),  f = (logT_j - x_i) / (x_{i+1} - x_i)
//   dem[i] += v_j (1 - f),  dem[i+1] += v_j f          only if x_0 <= logT_j <= x_{K-1}  (Interp1D's extrap = 0)
// so that, on the response table's own grid, sum_k dem_k R_w[k] is the render's pixel / (vol_c pixel_intensity_factor):
// a piecewise-linear R_w is the same hat functions.  em = sum v_j, logt_mean = sum v_j logT_j / em, column = sum q_j m_j rho_j.
//
// Layout: 32 lanes per ray, lane n of chunk c owns quadrature point j = 32 c + n (coalesced reads of raw / z); the optical
// depth is a 32-lane scan with a scalar carry from chunk to chunk, as in dt.hip.  The bins live in registers: lane n owns
// nodes n, n + 32, n + 64, n + 96.  The 32 (i, v(1-f), v f) triples of a chunk are walked in sample order by shuffle and a
// lane adds a triple's halves when it owns node i / i + 1: no atomics, no LDS per sample, one fixed summation order, so
// reruns and any position of a ray in a batch give the same bits.  The nodes (K <= 128) sit in LDS for the binary search.
#include "sunerf_common.h"
#include "ray_scan.h"
#include "../../include/sunerf_hip.h"

namespace {

constexpr int DEM_THREADS = 256;
constexpr int DEM_RAYS = DEM_THREADS / 32;    // rays per workgroup
constexpr int DEM_MAX_NODES = 128;
constexpr int DEM_SLOTS = DEM_MAX_NODES / 32;  // nodes per lane

struct DemArgs {
  const float* raw;       // (N,S,2)
  const float* z_vals;    // (N,S)
  const float* rays_o;    // (N,3) or null without a radius mask
  const float* rays_d;
  const float* nodes;     // (K,) strictly increasing
  const float* log_abs;   // (1,) or null
  float base_rho, base_t, r_in, r_out;
  int64_t n_rays;
  int S, K, masked;
  float* dem;             // (N,K) or null
  float* em;              // (N,)
  float* logt_mean;       // (N,) or null
  float* column;          // (N,) or null
};

__global__ __launch_bounds__(DEM_THREADS) void dem_integral_kernel(DemArgs a) {
  __shared__ float nodes[DEM_MAX_NODES];
  const int tid = threadIdx.x, n = tid & 31, sub = tid >> 5;
  if (tid < a.K) nodes[tid] = a.nodes[tid];
  __syncthreads();
  const int64_t ray = (int64_t)blockIdx.x * DEM_RAYS + sub;
  if (ray >= a.n_rays) return;                     // (a whole 32-lane group leaves: the shuffles are 32 wide)
  const int S = a.S, K = a.K, P = S - 1, n_chunks = (P + 31) >> 5;
  const float* z = a.z_vals + ray * S;
  const float* r = a.raw + ray * S * 2;
  const float kappa = a.log_abs ? fmaxf(a.log_abs[0], 0.f) : 0.f;
  float ox = 0.f, oy = 0.f, oz = 0.f, dx = 0.f, dy = 0.f, dz = 0.f;
  if (a.masked) {
    ox = a.rays_o[ray * 3 + 0]; oy = a.rays_o[ray * 3 + 1]; oz = a.rays_o[ray * 3 + 2];
    dx = a.rays_d[ray * 3 + 0]; dy = a.rays_d[ray * 3 + 1]; dz = a.rays_d[ray * 3 + 2];
  }
  const float x_lo = nodes[0], x_hi = nodes[K - 1];
  float bins[DEM_SLOTS];
#pragma unroll
  for (int k = 0; k < DEM_SLOTS; ++k) bins[k] = 0.f;
  float em = 0.f, wt = 0.f, col = 0.f, A_c = 0.f;
  for (int c = 0; c < n_chunks; ++c) {
    const int j = 32 * c + n;
    const bool valid = j < P;
    const int jj = valid ? j : P - 1;                                // (jj + 1 <= S - 1: every read stays inside the ray)
    const float zj = z[jj], zm = z[jj >= 1 ? jj - 1 : 0], zp = z[jj + 1];
    const f32x2 rr = *(const f32x2*)(r + 2 * jj);
    const float rho = expf(fmaxf(rr[0] + a.base_rho, 0.f));
    const float logt = fmaxf(rr[1] + a.base_t, 0.f);
    const float q = trapezoid_weight(jj, zm, zj, zp, S);              // of point j on the grid z[0..S-2]
    // t_j = exp(-A_{j+1}), A_{j+1} = A_j + ((ab_{j+1} + ab_j) * (z_{j+1} - z_j)) / 2
    float t = 1.f;
    if (kappa > 0.f) {                                               // (uniform: one scalar for the whole launch)
      const float rho_n = expf(fmaxf(r[2 * (jj + 1)] + a.base_rho, 0.f));
      const float inc = valid ? (rho_n * kappa + rho * kappa) * (zp - zj) / 2.f : 0.f;
      const float A = A_c + scan_up32(inc, n);
      t = expf(-A);
      A_c = __shfl(A, 31, 32);
    }
    bool inside = valid;
    if (a.masked) {
      const float rad = sample_radius(ox, oy, oz, dx, dy, dz, zj);
      inside = valid && rad >= a.r_in && rad <= a.r_out;              // a NaN radius fails both
    }
    const float v = inside ? q * t * (rho * rho) : 0.f;
    em += v;
    wt += v * logt;
    col += inside ? q * rho : 0.f;
    // ---- deposit
    int i = -2;                                                      // no lane owns node -2 or -1
    float lo_part = 0.f, hi_part = 0.f;
    if (inside && logt >= x_lo && logt <= x_hi) {
      int lo = 0, hi = K;                                            // number of nodes <= logt
      while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (nodes[mid] <= logt) lo = mid + 1; else hi = mid;
      }
      i = max(0, min(K - 2, lo - 1));
      const float x0 = nodes[i], x1 = nodes[i + 1];
      const float f = (logt - x0) / (x1 - x0);
      lo_part = v * (1.f - f);
      hi_part = v * f;
    }
    if (a.dem) {
      for (int s = 0; s < 32; ++s) {
        const int is = __shfl(i, s, 32);
        const float ls = __shfl(lo_part, s, 32), hs = __shfl(hi_part, s, 32);
        // nodes i and i + 1 belong to different lanes: this lane takes at most one half of the triple.  d = distance of the
        // half's node from this lane's first node: a multiple of 32 in [0, 96] when the lane owns it (is = -2: never)
        const int d_lo = is - n;
        const bool low = (d_lo & 31) == 0;
        const int d = low ? d_lo : d_lo + 1;
        const float val = low ? ls : hs;
#pragma unroll
        for (int k = 0; k < DEM_SLOTS; ++k) bins[k] += d == 32 * k ? val : 0.f;
      }
    }
  }
  em = sum32(em); wt = sum32(wt); col = sum32(col);
  if (a.dem) {
#pragma unroll
    for (int k = 0; k < DEM_SLOTS; ++k)
      if (n + 32 * k < K) a.dem[ray * K + n + 32 * k] = bins[k];
  }
  if (n == 0) {
    a.em[ray] = em;
    if (a.logt_mean) a.logt_mean[ray] = wt / em;                      // em = 0: NaN
    if (a.column) a.column[ray] = col;
  }
}

}  // namespace

extern "C" int sunerf_dem_integral(const float* raw, const float* z_vals, const float* rays_o, const float* rays_d,
                                   const float* logt_nodes, int n_nodes, float base_log_density, float base_log_temperature,
                                   const float* log_abs, float r_in, float r_out, int64_t n_rays, int n_samples, float* dem,
                                   float* em, float* logt_mean, float* column, void* stream) {
  if (n_rays < 0 || n_samples < 2 || n_nodes < 2) return SUNERF_E_BADARG;
  if (n_nodes > DEM_MAX_NODES) return SUNERF_E_UNSUPPORTED;
  if (n_rays == 0) return 0;
  const bool masked = !(r_in <= 0.f && r_out == INFINITY);
  if (!raw || !z_vals || !logt_nodes || !em || (masked && (!rays_o || !rays_d))) return SUNERF_E_BADARG;
  DemArgs a = {};
  a.raw = raw; a.z_vals = z_vals; a.rays_o = rays_o; a.rays_d = rays_d; a.nodes = logt_nodes; a.log_abs = log_abs;
  a.base_rho = base_log_density; a.base_t = base_log_temperature; a.r_in = r_in; a.r_out = r_out; a.n_rays = n_rays;
  a.S = n_samples; a.K = n_nodes; a.masked = masked ? 1 : 0; a.dem = dem; a.em = em; a.logt_mean = logt_mean; a.column = column;
  SUNERF_CLEAR_ERROR();
  hipLaunchKernelGGL(dem_integral_kernel, dim3((unsigned)((n_rays + DEM_RAYS - 1) / DEM_RAYS)), dim3(DEM_THREADS), 0,
                     (hipStream_t)stream, a);
  SUNERF_CHECK_LAUNCH();
  return 0;
}
