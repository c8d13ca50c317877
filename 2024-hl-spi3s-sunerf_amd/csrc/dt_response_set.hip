// Density / temperature radiative-transfer integral against a RESPONSE SET: the three kernels of dt.hip (forward, backward,
// backward with the gradients of weights / regularizing quantity) for any instrument's channels instead of the seven AIA rows
// of dt_response.h.  C ABI: include/sunerf_hip_response.h; DESIGN.md section 8m.
//
// A response set is M channels, each a positive integer code (what a ray's `wavelengths` row carries), its own strictly
// increasing log T grid of n_m >= 2 nodes and its response on it: offsets[M + 1] into the concatenated logt[] / resp[].  Per
// ray the W <= 8 columns are resolved against codes[M]; a column <= 0 or with a code the set does not hold is absent (image 0,
// no gradient), the documented semantics of dt.hip's channel_of().
//
// Everything else IS dt.hip: 32 lanes per ray, 32-sample chunks with scalar carries, exp(-A) slabs in dynamic LDS, one write
// of g_raw per sample, per-workgroup LDS sums and then float atomics for the scalar gradients -- and the per-sample arithmetic
// (rho, logT, the trapezoid increments, the scans, the channel loop, g0 / g1) written as dt.hip writes it, in its order, so
// that on the AIA set the outputs are those of sunerf_dt_integral_* bit for bit (tests/test_gpu_response_set.py).  What
// differs: the interval of a sample is found by binary search on the channel's own grid (dt_response.h indexes the 0.05-dex
// grid directly), the tables are staged in LDS at the set's size, and the backward's slab is strided by the call's W, not by
// the maximum.
#include "sunerf_common.h"
#include "../../include/sunerf_hip_response.h"

namespace {

constexpr int RS_THREADS = 256;
constexpr int RS_RAYS = RS_THREADS / 32;      // rays per workgroup (and per step of its walk over the batch)
constexpr int RS_MAX_GRID = 1024;             // backward: workgroups of the grid
constexpr int RS_MAXW = 8;                    // columns of a wavelengths row
constexpr int RS_MAXM = 64;                   // channels of a set
constexpr int RS_MAX_NODES = 4096;            // nodes of a set, all channels together
// LDS floats before the node tables: offsets[65] | codes[64] | g_kappa[64] g_vol | wave maxima[4], rounded up to 16 bytes
constexpr int RS_OFF = 0, RS_CODES = RS_OFF + RS_MAXM + 1, RS_ACC = RS_CODES + RS_MAXM, RS_WMAX = RS_ACC + RS_MAXM + 1;
constexpr int RS_HEAD = (RS_WMAX + RS_THREADS / 64 + 3) & ~3;

struct RsArgs {
  const float* raw;          // (N,S,2) MLP output
  const float* z_vals;       // (N,S)
  const float* rays_o;       // (N,3)
  const float* rays_d;
  const float* wavelengths;  // (N,W) channel code, <= 0: absent
  int M, n_nodes;
  const int* offsets;        // (M+1,)
  const float* codes;        // (M,)
  const float* table_logt;   // (n_nodes,)
  const float* table_resp;   // (n_nodes,), response x exposure time
  const float* log_abs;      // (M,) in set order
  const float* vol_c;        // (1,)
  float base_rho, base_t, pixel_factor, reg_radius;
  int64_t n_rays;
  int S, W;
  // forward outputs
  float* image;              // (N,W)
  float* weights;            // (N,S)
  float* reg_q;              // (N,S)  relu(inf0)
  float* height_map;         // (N,) or null
  float* absorption_map;     // (N,) or null
  float* regularization;     // (N,S) or null
  // backward
  const float* g_image;      // (N,W)
  const float* g_reg;        // (N,S) or null
  float* g_raw;              // (N,S,2)
  float* g_log_abs;          // (M,) accumulated
  float* g_vol_c;            // (1,) accumulated
  unsigned* g_absmax_bits;
  const float* g_weights;    // (N,S) or null (EXTRA backward only)
  const float* g_reg_q;      // (N,S) or null (EXTRA backward only)
};

__device__ __forceinline__ float scan_up32(float v, int n) {      // inclusive prefix sum over the 32 lanes of a ray
#pragma unroll
  for (int d = 1; d < 32; d <<= 1) {
    const float o = __shfl_up(v, d, 32);
    if (n >= d) v += o;
  }
  return v;
}
__device__ __forceinline__ float scan_down32(float v, int n) {    // inclusive suffix sum
#pragma unroll
  for (int d = 1; d < 32; d <<= 1) {
    const float o = __shfl_down(v, d, 32);
    if (n + d < 32) v += o;
  }
  return v;
}
__device__ __forceinline__ float sum32(float v) {
#pragma unroll
  for (int d = 16; d >= 1; d >>= 1) v += __shfl_xor(v, d, 32);
  return v;
}

// the set in LDS: lds[RS_OFF..] offsets (as int bits), lds[RS_CODES..] codes, then logt[n_nodes] | resp[n_nodes]
__device__ __forceinline__ void stage_set(const RsArgs& a, float* lds, int tid) {
  int* offs = (int*)(lds + RS_OFF);
  for (int i = tid; i <= a.M; i += RS_THREADS) offs[i] = a.offsets[i];
  for (int i = tid; i < a.M; i += RS_THREADS) lds[RS_CODES + i] = a.codes[i];
  float* tab = lds + RS_HEAD;
  for (int i = tid; i < a.n_nodes; i += RS_THREADS) { tab[i] = a.table_logt[i]; tab[a.n_nodes + i] = a.table_resp[i]; }
}

// linear interpolation on a grid of n nodes; returns value and slope (both 0 outside [x_0, x_{n-1}]).  The interval is the
// largest i <= n - 2 with x_i <= x (searchsorted(right=True) - 1, clamped to the last interval): what dt_response.h's
// response() finds on its uniform grid; the expression below is its expression.
__device__ __forceinline__ void response(const float* lt, const float* rs, int n, float x, float& val, float& slope) {
  val = 0.f; slope = 0.f;
  if (!(x >= lt[0] && x <= lt[n - 1])) return;
  int i = 0, hi = n - 2;
  while (i < hi) {
    const int mid = (i + hi + 1) >> 1;
    if (lt[mid] <= x) i = mid; else hi = mid - 1;
  }
  const float x0 = lt[i], x1 = lt[i + 1], y0 = rs[i], y1 = rs[i + 1];
  slope = (y1 - y0) / (x1 - x0);
  val = y0 + (x - x0) * (y1 - y0) / (x1 - x0);
}

// channel set-up of one ray (lane-uniform): row of the set, first node and node count, absorption coefficient.  Lane n looks
// at codes n and n + 32; the codes of a set are unique, so the maximum over the 32 lanes is the one match or -1.
struct Channels {
  int ch[RS_MAXW], first[RS_MAXW], count[RS_MAXW];
  float kappa[RS_MAXW];
  __device__ __forceinline__ void init(const RsArgs& a, const float* lds, int64_t ray, int n) {
    const int* offs = (const int*)(lds + RS_OFF);
    const float c0 = n < a.M ? lds[RS_CODES + n] : 0.f, c1 = n + 32 < a.M ? lds[RS_CODES + n + 32] : 0.f;
#pragma unroll
    for (int w = 0; w < RS_MAXW; ++w) {
      int m = -1;
      if (w < a.W) {
        const float wl = a.wavelengths[ray * a.W + w];
        if (wl > 0.f) m = wl == c0 ? n : (wl == c1 ? n + 32 : -1);
#pragma unroll
        for (int d = 16; d >= 1; d >>= 1) m = max(m, __shfl_xor(m, d, 32));
      }
      ch[w] = m;
      first[w] = m >= 0 ? offs[m] : 0;
      count[w] = m >= 0 ? offs[m + 1] - offs[m] : 0;
      kappa[w] = m >= 0 ? fmaxf(a.log_abs[m], 0.f) : 0.f;
    }
  }
};

// One forward sweep along the ray (dt.hip: forward_sweep).  `ea` (backward only) receives exp(-A_{j+1}) at [j * W + w].
template <bool KEEP>
__device__ __forceinline__ void forward_sweep(const RsArgs& a, const float* tab, const Channels& C, const float* r, const float* z,
                                              int n, float* ea, float trap[RS_MAXW]) {
  const int S = a.S, n_chunks = (S + 31) >> 5;
  float A_c[RS_MAXW], ab_c[RS_MAXW], e_c[RS_MAXW], T_c[RS_MAXW];
#pragma unroll
  for (int w = 0; w < RS_MAXW; ++w) { A_c[w] = ab_c[w] = e_c[w] = T_c[w] = 0.f; trap[w] = 0.f; }
  float z_c1 = 0.f, z_c2 = 0.f;
  for (int c = 0; c < n_chunks; ++c) {
    const int i = 32 * c + n;
    const bool valid = i < S;
    const int ii = valid ? i : S - 1;
    const float zi = z[ii];
    const f32x2 rr = *(const f32x2*)(r + 2 * ii);
    float zp = __shfl_up(zi, 1, 32);
    if (n == 0) zp = z_c1;
    float zpp = __shfl_up(zp, 1, 32);
    if (n == 0) zpp = z_c2;
    const float rho = expf(fmaxf(rr[0] + a.base_rho, 0.f));
    const float logt = fmaxf(rr[1] + a.base_t, 0.f);
#pragma unroll
    for (int w = 0; w < RS_MAXW; ++w) {
      if (w >= a.W) break;
      float R = 0.f, dR;
      if (C.ch[w] >= 0) response(tab + C.first[w], tab + a.n_nodes + C.first[w], C.count[w], logt, R, dR);
      const float ab = rho * C.kappa[w], e = rho * rho * R;
      float abp = __shfl_up(ab, 1, 32), ep = __shfl_up(e, 1, 32);
      if (n == 0) { abp = ab_c[w]; ep = e_c[w]; }
      const float inc = (valid && i >= 1) ? (ab + abp) * (zi - zp) / 2.f : 0.f;     // ((y1 + y0) * dx) / 2
      const float A = A_c[w] + scan_up32(inc, n);
      const float ex = expf(-A);
      if (KEEP && valid && i >= 1) ea[(size_t)(i - 1) * a.W + w] = ex;
      const float T = (valid && i >= 1) ? ex * ep : 0.f;                            // term_{i-1}
      float Tp = __shfl_up(T, 1, 32);
      if (n == 0) Tp = T_c[w];
      if (valid && i >= 2) trap[w] += (T + Tp) * (zp - zpp);
      A_c[w] = __shfl(A, 31, 32); ab_c[w] = __shfl(ab, 31, 32); e_c[w] = __shfl(e, 31, 32); T_c[w] = __shfl(T, 31, 32);
    }
    z_c2 = __shfl(zp, 31, 32);
    z_c1 = __shfl(zi, 31, 32);
  }
#pragma unroll
  for (int w = 0; w < RS_MAXW; ++w) trap[w] = sum32(trap[w]);
}

__global__ __launch_bounds__(RS_THREADS) void dt_response_fwd_kernel(RsArgs a) {
  extern __shared__ __attribute__((aligned(16))) float lds[];      // head | logt | resp
  const float* tab = lds + RS_HEAD;
  const int tid = threadIdx.x, n = tid & 31, sub = tid >> 5;
  stage_set(a, lds, tid);
  __syncthreads();
  const int64_t ray = (int64_t)blockIdx.x * RS_RAYS + sub;
  if (ray >= a.n_rays) return;                     // (a whole 32-lane group leaves: the shuffles are 32 wide)
  const int S = a.S, n_chunks = (S + 31) >> 5;
  const float* z = a.z_vals + ray * S;
  const float* r = a.raw + ray * S * 2;
  Channels C;
  C.init(a, lds, ray, n);
  float trap[RS_MAXW];
  forward_sweep<false>(a, tab, C, r, z, n, nullptr, trap);
  if (n < a.W) {
    float t = 0.f;
#pragma unroll
    for (int w = 0; w < RS_MAXW; ++w) if (w == n) t = trap[w];
    a.image[ray * a.W + n] = t / 2.f * a.vol_c[0] * a.pixel_factor;              // trapezoid: sum((y1 + y0) * dx) / 2
  }
  // weights = relu(inf0) / (sum + 1e-10), maps, regularization (density_temperature.py:268-274)
  const float ox = a.rays_o[ray * 3 + 0], oy = a.rays_o[ray * 3 + 1], oz = a.rays_o[ray * 3 + 2];
  const float dx = a.rays_d[ray * 3 + 0], dy = a.rays_d[ray * 3 + 1], dz = a.rays_d[ray * 3 + 2];
  float sum = 0.f;
  for (int c = 0; c < n_chunks; ++c) {
    const int i = 32 * c + n;
    if (i < S) sum += fmaxf(r[2 * i] + a.base_rho, 0.f);
  }
  const float denom = sum32(sum) + 1e-10f;
  float hm = 0.f, am = 0.f;
  for (int c = 0; c < n_chunks; ++c) {
    const int i = 32 * c + n;
    if (i >= S) continue;
    const float q = fmaxf(r[2 * i] + a.base_rho, 0.f);
    const float w = q / denom;
    a.weights[ray * S + i] = w;
    a.reg_q[ray * S + i] = q;
    if (a.regularization || a.height_map) {
      const float zi = z[i];
      const float px = ox + dx * zi, py = oy + dy * zi, pz = oz + dz * zi;
      const float pd = sqrtf((px * px + py * py) + pz * pz);
      hm += w * pd;
      if (a.regularization) a.regularization[ray * S + i] = fmaxf(pd - a.reg_radius, 0.f) * fmaxf(q, 0.f);
    }
    am += 1.f - q;
  }
  hm = sum32(hm); am = sum32(am);
  if (n == 0) {
    if (a.height_map) a.height_map[ray] = hm;
    if (a.absorption_map) a.absorption_map[ray] = am;
  }
}

// backward (dt.hip: dt_integral_bwd_kernel): a forward sweep keeps exp(-A_{j+1}) of every column in LDS ([ray][j][column],
// W columns); the reverse sweep forms the suffix sums and from them the gradients of the two raw outputs of every sample,
// summed over the columns in the lane (no atomics).  log_abs / vol_c gradients: per-ray lane sums -> workgroup sums in LDS ->
// at most M + 1 atomic adds per workgroup.  EXTRA: also the gradients arriving at weights and the regularizing quantity.
template <bool EXTRA>
__global__ __launch_bounds__(RS_THREADS) void dt_response_bwd_kernel(RsArgs a) {
  // head (offsets, codes, g_kappa[64] g_vol, wave maxima) | logt | resp | [RS_RAYS][S][W] exp(-A).  All of it dynamic (no
  // static __shared__): the launcher's 160 KiB check then sees the whole allocation.
  extern __shared__ __attribute__((aligned(16))) float lds[];
  const float* tab = lds + RS_HEAD;
  float* acc = lds + RS_ACC;
  float* wave_max = lds + RS_WMAX;
  const int tid = threadIdx.x, n = tid & 31, sub = tid >> 5;
  stage_set(a, lds, tid);
  if (tid <= RS_MAXM) acc[tid] = 0.f;
  __syncthreads();
  float local_max = 0.f;
  // a workgroup walks over groups of RS_RAYS rays (grid <= RS_MAX_GRID) and sends its sums ONCE
  const int64_t n_groups = (a.n_rays + RS_RAYS - 1) / RS_RAYS;
  for (int64_t grp = blockIdx.x; grp < n_groups; grp += gridDim.x) {
  const int64_t ray_raw = grp * RS_RAYS + sub;
  const bool ray_ok = ray_raw < a.n_rays;
  const int64_t ray = ray_ok ? ray_raw : a.n_rays - 1;
  const int S = a.S, n_chunks = (S + 31) >> 5;
  float* ea = lds + RS_HEAD + 2 * a.n_nodes + (size_t)sub * S * a.W;
  const float* z = a.z_vals + ray * S;
  const float* r = a.raw + ray * S * 2;
  Channels C;
  C.init(a, lds, ray, n);
  float trap[RS_MAXW];
  forward_sweep<true>(a, tab, C, r, z, n, ea, trap);
  float g_trap[RS_MAXW], g_kappa[RS_MAXW], G_c[RS_MAXW];
  const float Cf = a.vol_c[0] * a.pixel_factor;
#pragma unroll
  for (int w = 0; w < RS_MAXW; ++w) {
    g_trap[w] = (ray_ok && w < a.W) ? a.g_image[ray * a.W + w] * Cf : 0.f;
    g_kappa[w] = 0.f;
    G_c[w] = 0.f;
  }
  const float ox = a.rays_o[ray * 3 + 0], oy = a.rays_o[ray * 3 + 1], oz = a.rays_o[ray * 3 + 2];
  const float dx = a.rays_d[ray * 3 + 0], dy = a.rays_d[ray * 3 + 1], dz = a.rays_d[ray * 3 + 2];
  // trapezoid weight of term_j on the grid z[0..S-2]:  wt_j = (dz_{j-1} + dz_j) / 2 with missing neighbours dropped
  auto wt = [&](int j, float zm, float z0, float zp1) {
    float w = 0.f;
    if (j >= 1) w += z0 - zm;
    if (j <= S - 3) w += zp1 - z0;
    return 0.5f * w;
  };
  float inv_denom = 0.f, gw_dot_w = 0.f;
  if (EXTRA && a.g_weights) {
    float sum = 0.f;
    for (int c = 0; c < n_chunks; ++c) {
      const int i = 32 * c + n;
      if (i < S) sum += fmaxf(r[2 * i] + a.base_rho, 0.f);
    }
    const float denom = sum32(sum) + 1e-10f;
    float dot = 0.f;
    for (int c = 0; c < n_chunks; ++c) {
      const int i = 32 * c + n;
      if (i < S) dot += a.g_weights[ray * S + i] * (fmaxf(r[2 * i] + a.base_rho, 0.f) / denom);
    }
    gw_dot_w = sum32(dot);
    inv_denom = 1.f / denom;
  }
  for (int c = n_chunks - 1; c >= 0; --c) {
    const int k = 32 * c + n;
    const bool valid = k < S;
    const int kk = valid ? k : S - 1;
    const float zk = z[kk], zm = z[kk >= 1 ? kk - 1 : 0], zp1 = z[kk + 1 < S ? kk + 1 : S - 1];
    const f32x2 rr = *(const f32x2*)(r + 2 * kk);
    const float inf0 = rr[0] + a.base_rho, inf1 = rr[1] + a.base_t;
    const float rho = expf(fmaxf(inf0, 0.f)), logt = fmaxf(inf1, 0.f);
    const float wk = wt(kk, zm, zk, zp1);
    // lane 0 also needs dL/dA of the sample below its chunk (k - 1): its term is recomputed here
    const bool below = n == 0 && k >= 1;
    float rho_b = 0.f, logt_b = 0.f, w_b = 0.f;
    if (below) {
      const f32x2 rb = *(const f32x2*)(r + 2 * (k - 1));
      rho_b = expf(fmaxf(rb[0] + a.base_rho, 0.f));
      logt_b = fmaxf(rb[1] + a.base_t, 0.f);
      w_b = wt(k - 1, z[k >= 2 ? k - 2 : 0], zm, zk);
    }
    float g0 = 0.f, g1 = 0.f;
#pragma unroll
    for (int w = 0; w < RS_MAXW; ++w) {
      if (w >= a.W) break;
      float R = 0.f, dR = 0.f;
      if (C.ch[w] >= 0) response(tab + C.first[w], tab + a.n_nodes + C.first[w], C.count[w], logt, R, dR);
      const bool has_term = valid && k <= S - 2;
      const float eak = has_term ? ea[(size_t)k * a.W + w] : 0.f;
      const float gA = has_term ? -g_trap[w] * wk * (eak * rho * rho * R) : 0.f;       // dL/dA_k = -g_term_k * term_k
      const float G = G_c[w] + scan_down32(gA, n);                                      // G_k = sum_{j >= k} dL/dA_j
      float gA_b = __shfl_up(gA, 1, 32);                                                 // dL/dA_{k-1}
      if (n == 0) {
        gA_b = 0.f;
        if (below) {
          float Rb = 0.f, dRb;
          if (C.ch[w] >= 0) response(tab + C.first[w], tab + a.n_nodes + C.first[w], C.count[w], logt_b, Rb, dRb);
          gA_b = -g_trap[w] * w_b * (ea[(size_t)(k - 1) * a.W + w] * rho_b * rho_b * Rb);
        }
      }
      if (valid) {
        float g_ab = 0.f;
        if (k <= S - 2) g_ab += 0.5f * (zp1 - zk) * G;
        if (k >= 1) g_ab += 0.5f * (zk - zm) * (G + gA_b);                               // G_{k-1}
        const float g_e = has_term ? g_trap[w] * wk * eak : 0.f;
        const float g_rho = g_ab * C.kappa[w] + g_e * 2.f * rho * R;
        g_kappa[w] += g_ab * rho;
        if (inf0 > 0.f) g0 += g_rho * rho;
        if (inf1 > 0.f) g1 += g_e * rho * rho * dR;
      }
      G_c[w] = __shfl(G, 0, 32);
    }
    if (valid && ray_ok) {
      // regularization_k = relu(|p_k| - R) * relu(relu(inf0))
      const float gr = a.g_reg ? a.g_reg[ray * S + k] : 0.f;
      if (gr != 0.f && inf0 > 0.f) {
        const float px = ox + dx * zk, py = oy + dy * zk, pz = oz + dz * zk;
        g0 += gr * fmaxf(sqrtf((px * px + py * py) + pz * pz) - a.reg_radius, 0.f);
      }
      if (EXTRA && inf0 > 0.f) {
        if (a.g_reg_q) g0 += a.g_reg_q[ray * S + k];
        if (a.g_weights) g0 += (a.g_weights[ray * S + k] - gw_dot_w) * inv_denom;
      }
      const f32x2 gg = {g0, g1};
      *(f32x2*)(a.g_raw + ((size_t)ray * S + k) * 2) = gg;
      local_max = fmaxf(local_max, fmaxf(fabsf(g0), fabsf(g1)));
    }
  }
  // ---- parameter gradients: log_abs (through kappa = relu(log_abs)) and vol_c ----
  float g_vol = 0.f;
#pragma unroll
  for (int w = 0; w < RS_MAXW; ++w) {
    const float gk = sum32(g_kappa[w]);
    if (n == 0 && ray_ok && w < a.W && C.ch[w] >= 0) {
      if (a.log_abs[C.ch[w]] > 0.f && gk != 0.f) atomicAdd(acc + C.ch[w], gk);
      g_vol += a.g_image[ray * a.W + w] * (0.5f * trap[w]) * a.pixel_factor;
    }
  }
  if (n == 0 && g_vol != 0.f) atomicAdd(acc + RS_MAXM, g_vol);
  }
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) local_max = fmaxf(local_max, __shfl_xor(local_max, d));
  if ((tid & 63) == 0) wave_max[tid >> 6] = local_max;
  __syncthreads();
  if (tid < a.M && acc[tid] != 0.f) atomicAdd(a.g_log_abs + tid, acc[tid]);
  if (tid == RS_MAXM && acc[RS_MAXM] != 0.f) atomicAdd(a.g_vol_c, acc[RS_MAXM]);
  if (tid == 0) {
    float m = wave_max[0];
#pragma unroll
    for (int w = 1; w < RS_THREADS / 64; ++w) m = fmaxf(m, wave_max[w]);
    if (m > 0.f && m < INFINITY) atomicMax(a.g_absmax_bits, __float_as_uint(m));
  }
}

// sizes and limits, then the empty batch (returns 1: "nothing to launch"), then the pointers every entry point reads
int check_common(const RsArgs& a) {
  if (a.n_rays < 0 || a.S < 3 || a.M < 1 || a.n_nodes < 2 * a.M) return SUNERF_E_BADARG;
  if (a.M > RS_MAXM || a.n_nodes > RS_MAX_NODES || a.W < 1 || a.W > RS_MAXW) return SUNERF_E_UNSUPPORTED;
  if (a.n_rays == 0) return 1;
  if (!a.raw || !a.z_vals || !a.rays_o || !a.rays_d || !a.wavelengths || !a.offsets || !a.codes || !a.table_logt ||
      !a.table_resp || !a.log_abs || !a.vol_c)
    return SUNERF_E_BADARG;
  return 0;
}

size_t bwd_lds_bytes(int S, int W, int n_nodes) {
  return ((size_t)RS_HEAD + 2 * (size_t)n_nodes + (size_t)RS_RAYS * S * W) * sizeof(float);
}

template <bool EXTRA>
int launch_bwd(const RsArgs& a, void* g_absmax, hipStream_t st) {
  // dynamic LDS is the whole allocation; refused before anything is queued, the outputs untouched
  const size_t lds = bwd_lds_bytes(a.S, a.W, a.n_nodes);
  if (a.n_rays > 0 && lds > 160 * 1024) return SUNERF_E_UNSUPPORTED;
  hipError_t e;
  if ((char*)a.g_vol_c == (char*)a.g_log_abs + a.M * sizeof(float) && (char*)g_absmax == (char*)a.g_vol_c + sizeof(float)) {
    // the three small outputs in one buffer (what the Python wrapper passes): one clear instead of three
    if ((e = hipMemsetAsync(a.g_log_abs, 0, (a.M + 2) * sizeof(float), st)) != hipSuccess) return (int)e;
  } else {
    if ((e = hipMemsetAsync(g_absmax, 0, 4, st)) != hipSuccess) return (int)e;
    if ((e = hipMemsetAsync(a.g_log_abs, 0, a.M * sizeof(float), st)) != hipSuccess) return (int)e;
    if ((e = hipMemsetAsync(a.g_vol_c, 0, sizeof(float), st)) != hipSuccess) return (int)e;
  }
  if (a.n_rays == 0) return 0;
  if (lds > 64 * 1024) {
    e = hipFuncSetAttribute((const void*)dt_response_bwd_kernel<EXTRA>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    if (e != hipSuccess) return (int)e;
  }
  SUNERF_CLEAR_ERROR();
  int64_t groups = (a.n_rays + RS_RAYS - 1) / RS_RAYS;
  if (groups > RS_MAX_GRID) groups = RS_MAX_GRID;
  hipLaunchKernelGGL(dt_response_bwd_kernel<EXTRA>, dim3((unsigned)groups), dim3(RS_THREADS), lds, st, a);
  SUNERF_CHECK_LAUNCH();
  return 0;
}

template <bool EXTRA>
int run_bwd(const RsArgs& a, void* g_absmax, void* stream) {
  const int rc = check_common(a);
  if (rc < 0) return rc;
  // an empty batch has null (N,...) tensors; its call only clears the scalar outputs
  if (!a.g_log_abs || !a.g_vol_c || !g_absmax || (a.n_rays > 0 && (!a.g_image || !a.g_raw))) return SUNERF_E_BADARG;
  return launch_bwd<EXTRA>(a, g_absmax, (hipStream_t)stream);
}

RsArgs common_args(const float* raw, const float* z_vals, const float* rays_o, const float* rays_d, const float* wavelengths,
                   int n_wavelengths, int n_channels, int n_nodes_total, const int* offsets, const float* codes,
                   const float* logt, const float* resp, const float* log_abs, const float* vol_c, float base_log_density,
                   float base_log_temperature, float pixel_intensity_factor, float reg_radius, int64_t n_rays, int n_samples) {
  RsArgs a = {};
  a.raw = raw; a.z_vals = z_vals; a.rays_o = rays_o; a.rays_d = rays_d; a.wavelengths = wavelengths; a.W = n_wavelengths;
  a.M = n_channels; a.n_nodes = n_nodes_total; a.offsets = offsets; a.codes = codes; a.table_logt = logt; a.table_resp = resp;
  a.log_abs = log_abs; a.vol_c = vol_c; a.base_rho = base_log_density; a.base_t = base_log_temperature;
  a.pixel_factor = pixel_intensity_factor; a.reg_radius = reg_radius; a.n_rays = n_rays; a.S = n_samples;
  return a;
}

}  // namespace

extern "C" int sunerf_response_abi_version(void) { return SUNERF_RESPONSE_ABI_VERSION; }

extern "C" size_t sunerf_dt_response_bwd_lds_bytes(int n_samples, int n_wavelengths, int n_nodes_total) {
  if (n_samples < 0 || n_wavelengths < 0 || n_nodes_total < 0) return 0;
  return bwd_lds_bytes(n_samples, n_wavelengths, n_nodes_total);
}

extern "C" int sunerf_dt_response_fwd(const float* raw, const float* z_vals, const float* rays_o, const float* rays_d,
                                      const float* wavelengths, int n_wavelengths, int n_channels, int n_nodes_total,
                                      const int* offsets, const float* codes, const float* logt, const float* resp,
                                      const float* log_abs, const float* vol_c, float base_log_density,
                                      float base_log_temperature, float pixel_intensity_factor, float reg_radius,
                                      int64_t n_rays, int n_samples, float* image, float* weights, float* reg_q,
                                      float* height_map, float* absorption_map, float* regularization, void* stream) {
  RsArgs a = common_args(raw, z_vals, rays_o, rays_d, wavelengths, n_wavelengths, n_channels, n_nodes_total, offsets, codes, logt,
                         resp, log_abs, vol_c, base_log_density, base_log_temperature, pixel_intensity_factor, reg_radius, n_rays,
                         n_samples);
  a.image = image; a.weights = weights; a.reg_q = reg_q; a.height_map = height_map; a.absorption_map = absorption_map;
  a.regularization = regularization;
  const int rc = check_common(a);
  if (rc) return rc < 0 ? rc : 0;
  if (!image || !weights || !reg_q) return SUNERF_E_BADARG;
  const size_t lds = ((size_t)RS_HEAD + 2 * (size_t)n_nodes_total) * sizeof(float);      // <= 33 KiB
  SUNERF_CLEAR_ERROR();
  hipLaunchKernelGGL(dt_response_fwd_kernel, dim3((unsigned)((n_rays + RS_RAYS - 1) / RS_RAYS)), dim3(RS_THREADS), lds,
                     (hipStream_t)stream, a);
  SUNERF_CHECK_LAUNCH();
  return 0;
}

extern "C" int sunerf_dt_response_bwd(const float* raw, const float* z_vals, const float* rays_o, const float* rays_d,
                                      const float* wavelengths, int n_wavelengths, int n_channels, int n_nodes_total,
                                      const int* offsets, const float* codes, const float* logt, const float* resp,
                                      const float* log_abs, const float* vol_c, float base_log_density,
                                      float base_log_temperature, float pixel_intensity_factor, float reg_radius,
                                      int64_t n_rays, int n_samples, const float* g_image, const float* g_reg, float* g_raw,
                                      float* g_log_abs, float* g_vol_c, void* g_absmax, void* stream) {
  RsArgs a = common_args(raw, z_vals, rays_o, rays_d, wavelengths, n_wavelengths, n_channels, n_nodes_total, offsets, codes, logt,
                         resp, log_abs, vol_c, base_log_density, base_log_temperature, pixel_intensity_factor, reg_radius, n_rays,
                         n_samples);
  a.g_image = g_image; a.g_reg = g_reg; a.g_raw = g_raw; a.g_log_abs = g_log_abs; a.g_vol_c = g_vol_c;
  a.g_absmax_bits = (unsigned*)g_absmax;
  return run_bwd<false>(a, g_absmax, stream);
}

extern "C" int sunerf_dt_response_bwd_full(const float* raw, const float* z_vals, const float* rays_o, const float* rays_d,
                                           const float* wavelengths, int n_wavelengths, int n_channels, int n_nodes_total,
                                           const int* offsets, const float* codes, const float* logt, const float* resp,
                                           const float* log_abs, const float* vol_c, float base_log_density,
                                           float base_log_temperature, float pixel_intensity_factor, float reg_radius,
                                           int64_t n_rays, int n_samples, const float* g_image, const float* g_reg,
                                           const float* g_weights, const float* g_reg_q, float* g_raw, float* g_log_abs,
                                           float* g_vol_c, void* g_absmax, void* stream) {
  RsArgs a = common_args(raw, z_vals, rays_o, rays_d, wavelengths, n_wavelengths, n_channels, n_nodes_total, offsets, codes, logt,
                         resp, log_abs, vol_c, base_log_density, base_log_temperature, pixel_intensity_factor, reg_radius, n_rays,
                         n_samples);
  a.g_image = g_image; a.g_reg = g_reg; a.g_raw = g_raw; a.g_log_abs = g_log_abs; a.g_vol_c = g_vol_c;
  a.g_absmax_bits = (unsigned*)g_absmax; a.g_weights = g_weights; a.g_reg_q = g_reg_q;
  return run_bwd<true>(a, g_absmax, stream);
}
