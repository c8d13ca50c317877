// The density / temperature radiative-transfer integral, forward and backward, ONCE: the kernel bodies and the backward
// launcher of dt.hip (the seven AIA rows of dt_response.h) and of dt_response_set.hip (any instrument's response set).
//
//   rho = exp(relu(raw0 + base_rho));  logT = relu(raw1 + base_T);  kappa_w = relu(log_abs[w])
//   A_j   = cumulative_trapezoid(rho kappa_w, z)_j                         j = 0..S-2   (density_temperature.py:261)
//   I_w   = trapezoid(exp(-A_j) rho_j^2 R_w(logT_j), z_j; j = 0..S-2) * vol_c * pixel_intensity_factor   (:263-265)
//   weights = relu(inf0) / (sum + 1e-10);  regularizing quantity = relu(inf0)
//
// Layout: 32 lanes per ray, one sample per lane and 32-sample chunk (coalesced reads of raw / z, coalesced writes), the
// channels looped inside.  Everything sequential along the ray in the reference -- the running optical depth
// (cumulative_trapezoid), the trapezoid sum of the attenuated emission and, in the backward pass, the suffix sums of the
// optical-depth gradients -- is a chunk-wise scan over the 32 lanes with a scalar carry from chunk to chunk, like the
// emission integral (emission_sweep.h). (The first version walked the samples with ONE thread per ray and
// channel: 1.2 ms for the backward of 8192 rays x 256 samples x 7 channels, 10 % of a config-5 training step.)
//
// What the two files differ in is a SET POLICY, a struct of static members that each of them defines:
//   Args                         the kernel argument struct: DtSweepArgs, then the set's tables (at the end: the order of the
//                                kernel arguments moves the backward kernels by about 1 % either way)
//   MAXW                         columns of a `wavelengths` row at most: sizes the per-column registers and the channel loops
//   Channels                     lane-uniform set-up of one ray's columns: ch[MAXW] (row of the set or -1), kappa[MAXW], whatever
//                                lookup() needs, and init(a, lds, ray, n)
//   lookup(a, C, w, tab, logt, R, dR)   R_w(logT) and its slope for a present column
//   stride(a)                    floats from sample to sample of a ray's exp(-A) slab
//   stage(a, lds, tid)           copies the tables (and what init() reads) to LDS
//   tab(lds), acc(lds), wave_max(lds), slab(a, lds)   the LDS layout; acc holds n_abs(a) <= VOL log_abs sums and, at [VOL], vol_c's
//   n_abs(a), VOL
//   bwd_lds_bytes(a)             (host) dynamic LDS of the backward kernel
// The arithmetic below is the same for both, expression by expression (the build uses -ffp-contract=off), so on the AIA set the
// response-set entry points give the bits of the AIA ones (tests/test_gpu_response_set.py).
#pragma once
#include "sunerf_common.h"
#include "ray_scan.h"
#include "../../include/sunerf_hip.h"

constexpr int DT_THREADS = 256;
constexpr int DT_RAYS = DT_THREADS / 32;      // rays per workgroup (and per step of its walk over the batch)
constexpr int DT_MAX_GRID = 1024;             // backward: workgroups of the grid

struct DtSweepArgs {
  const float* raw;          // (N,S,2) MLP output
  const float* z_vals;       // (N,S)
  const float* rays_o;       // (N,3)
  const float* rays_d;
  const float* wavelengths;  // (N,W) channel wavelength in Angstrom / channel code, <= 0: absent
  const float* log_abs;      // one per channel of the set, in set order
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
  float* g_log_abs;          // as log_abs, accumulated
  float* g_vol_c;            // (1,) accumulated
  unsigned* g_absmax_bits;
  const float* g_weights;    // (N,S) or null (EXTRA backward only)
  const float* g_reg_q;      // (N,S) or null (EXTRA backward only)
};

// One forward sweep along the ray: per channel the optical depth A_i = cumulative_trapezoid(rho kappa, z) and the trapezoid
// sum of term_j = exp(-A_{j+1}) rho_j^2 R(logT_j), j = 0..S-2 (density_temperature.py:261-265).  `ea` (backward only):
// receives exp(-A_{j+1}) at [j * stride + w].  Returns the trapezoid sums (x 2, as the reference's running sum) in trap[].
template <class Set, bool KEEP>
__device__ __forceinline__ void forward_sweep(const typename Set::Args& a, const float* tab, const typename Set::Channels& C,
                                              const float* r, const float* z, int n, float* ea, int stride, float trap[Set::MAXW]) {
  constexpr int MAXW = Set::MAXW;
  const int S = a.S, n_chunks = (S + 31) >> 5;
  float A_c[MAXW], ab_c[MAXW], e_c[MAXW], T_c[MAXW];
#pragma unroll
  for (int w = 0; w < MAXW; ++w) { A_c[w] = ab_c[w] = e_c[w] = T_c[w] = 0.f; trap[w] = 0.f; }
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
    for (int w = 0; w < MAXW; ++w) {
      if (w >= a.W) break;
      float R = 0.f, dR;
      if (C.ch[w] >= 0) Set::lookup(a, C, w, tab, logt, R, dR);
      const float ab = rho * C.kappa[w], e = rho * rho * R;
      float abp = __shfl_up(ab, 1, 32), ep = __shfl_up(e, 1, 32);
      if (n == 0) { abp = ab_c[w]; ep = e_c[w]; }
      const float inc = (valid && i >= 1) ? (ab + abp) * (zi - zp) / 2.f : 0.f;     // ((y1 + y0) * dx) / 2
      const float A = A_c[w] + scan_up32(inc, n);
      const float ex = expf(-A);
      if (KEEP && valid && i >= 1) ea[(size_t)(i - 1) * stride + w] = ex;
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
  for (int w = 0; w < MAXW; ++w) trap[w] = sum32(trap[w]);
}

// the forward kernel's body; `lds` is what Set::stage() fills (static for the AIA tables, dynamic for a response set: each
// file's __global__ declares its own)
template <class Set>
__device__ __forceinline__ void dt_forward(const typename Set::Args& a, float* lds) {
  constexpr int MAXW = Set::MAXW;
  const float* tab = Set::tab(lds);
  const int tid = threadIdx.x, n = tid & 31, sub = tid >> 5;
  Set::stage(a, lds, tid);
  __syncthreads();
  const int64_t ray = (int64_t)blockIdx.x * DT_RAYS + sub;
  if (ray >= a.n_rays) return;                     // (a whole 32-lane group leaves: the shuffles are 32 wide)
  const int S = a.S, n_chunks = (S + 31) >> 5;
  const float* z = a.z_vals + ray * S;
  const float* r = a.raw + ray * S * 2;
  typename Set::Channels C;
  C.init(a, lds, ray, n);
  float trap[MAXW];
  forward_sweep<Set, false>(a, tab, C, r, z, n, nullptr, 0, trap);
  if (n < a.W) {
    float t = 0.f;
#pragma unroll
    for (int w = 0; w < MAXW; ++w) if (w == n) t = trap[w];
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
      const float pd = sample_radius(ox, oy, oz, dx, dy, dz, z[i]);
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

// backward: a forward sweep keeps exp(-A_{j+1}) of every column in LDS ([ray][j][column]); the reverse sweep forms the
// suffix sums G_k = sum_{j >= k} dL/dA_j chunk by chunk (descending) and from them the gradients of the two raw outputs of
// every sample, summed over the columns in the lane (no atomics).  log_abs / vol_c gradients: per-ray lane sums ->
// workgroup sums in LDS -> at most n_abs + 1 atomic adds per workgroup.
// EXTRA: also the gradients arriving at the two other outputs of raw2outputs (density_temperature.py:267-271),
//   q = relu(inf0):              g_inf0 += g_q [inf0 > 0]
//   w = q / (sum_s q + 1e-10):   g_inf0 += [inf0 > 0] (g_w - sum_s g_w w) / (sum_s q + 1e-10)
// with the two per-ray sums taken by the ray's own 32 lanes before the reverse sweep (the sum of q in the forward kernel's
// order).  EXTRA = false is the kernel of sunerf_dt_integral_bwd as it always was.
// The kernel itself, not a body behind per-file wrappers: called through a wrapper the same text compiled to up to 240 more
// instructions per kernel.  LDS: tables, accumulators, wave maxima and slabs, all of it dynamic (no
// static __shared__): the launcher's 160 KiB check then sees the whole allocation.
template <class Set, bool EXTRA>
__global__ __launch_bounds__(DT_THREADS) void dt_bwd_kernel(typename Set::Args a) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  constexpr int MAXW = Set::MAXW;
  const int stride = Set::stride(a);      // read once and handed to the sweep: asked for at the store, a run-time stride cost the
                                          // sweep an integer multiply per column and chunk
  const float* tab = Set::tab(lds);
  float* acc = Set::acc(lds);
  float* wave_max = Set::wave_max(lds);
  const int tid = threadIdx.x, n = tid & 31, sub = tid >> 5;
  Set::stage(a, lds, tid);
  if (tid <= Set::VOL) acc[tid] = 0.f;
  __syncthreads();
  float local_max = 0.f;
  // a workgroup walks over groups of DT_RAYS rays (grid <= DT_MAX_GRID) and sends its sums ONCE: n_abs + 1 atomic adds and one
  // atomic max per workgroup instead of per ray group / per wave
  const int64_t n_groups = (a.n_rays + DT_RAYS - 1) / DT_RAYS;
  for (int64_t grp = blockIdx.x; grp < n_groups; grp += gridDim.x) {
  const int64_t ray_raw = grp * DT_RAYS + sub;
  const bool ray_ok = ray_raw < a.n_rays;
  const int64_t ray = ray_ok ? ray_raw : a.n_rays - 1;
  const int S = a.S, n_chunks = (S + 31) >> 5;
  float* ea = Set::slab(a, lds) + (size_t)sub * S * stride;
  const float* z = a.z_vals + ray * S;
  const float* r = a.raw + ray * S * 2;
  typename Set::Channels C;
  C.init(a, lds, ray, n);
  float trap[MAXW];
  forward_sweep<Set, true>(a, tab, C, r, z, n, ea, stride, trap);
  float g_trap[MAXW], g_kappa[MAXW], G_c[MAXW];
  const float Cf = a.vol_c[0] * a.pixel_factor;
#pragma unroll
  for (int w = 0; w < MAXW; ++w) {
    g_trap[w] = (ray_ok && w < a.W) ? a.g_image[ray * a.W + w] * Cf : 0.f;
    g_kappa[w] = 0.f;
    G_c[w] = 0.f;
  }
  const float ox = a.rays_o[ray * 3 + 0], oy = a.rays_o[ray * 3 + 1], oz = a.rays_o[ray * 3 + 2];
  const float dx = a.rays_d[ray * 3 + 0], dy = a.rays_d[ray * 3 + 1], dz = a.rays_d[ray * 3 + 2];
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
    const float wk = trapezoid_weight(kk, zm, zk, zp1, S);      // of term_k on the grid z[0..S-2]
    // lane 0 also needs dL/dA of the sample below its chunk (k - 1): its term is recomputed here
    const bool below = n == 0 && k >= 1;
    float rho_b = 0.f, logt_b = 0.f, w_b = 0.f;
    if (below) {
      const f32x2 rb = *(const f32x2*)(r + 2 * (k - 1));
      rho_b = expf(fmaxf(rb[0] + a.base_rho, 0.f));
      logt_b = fmaxf(rb[1] + a.base_t, 0.f);
      w_b = trapezoid_weight(k - 1, z[k >= 2 ? k - 2 : 0], zm, zk, S);
    }
    float g0 = 0.f, g1 = 0.f;
#pragma unroll
    for (int w = 0; w < MAXW; ++w) {
      if (w >= a.W) break;
      float R = 0.f, dR = 0.f;
      if (C.ch[w] >= 0) Set::lookup(a, C, w, tab, logt, R, dR);
      const bool has_term = valid && k <= S - 2;
      const float eak = has_term ? ea[(size_t)k * stride + w] : 0.f;
      const float gA = has_term ? -g_trap[w] * wk * (eak * rho * rho * R) : 0.f;       // dL/dA_k = -g_term_k * term_k
      const float G = G_c[w] + scan_down32(gA, n);                                      // G_k = sum_{j >= k} dL/dA_j
      float gA_b = __shfl_up(gA, 1, 32);                                                 // dL/dA_{k-1}
      if (n == 0) {
        gA_b = 0.f;
        if (below) {
          float Rb = 0.f, dRb;
          if (C.ch[w] >= 0) Set::lookup(a, C, w, tab, logt_b, Rb, dRb);
          gA_b = -g_trap[w] * w_b * (ea[(size_t)(k - 1) * stride + w] * rho_b * rho_b * Rb);
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
        g0 += gr * fmaxf(sample_radius(ox, oy, oz, dx, dy, dz, zk) - a.reg_radius, 0.f);
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
  for (int w = 0; w < MAXW; ++w) {
    const float gk = sum32(g_kappa[w]);
    if (n == 0 && ray_ok && w < a.W && C.ch[w] >= 0) {
      if (a.log_abs[C.ch[w]] > 0.f && gk != 0.f) atomicAdd(acc + C.ch[w], gk);
      g_vol += a.g_image[ray * a.W + w] * (0.5f * trap[w]) * a.pixel_factor;
    }
  }
  if (n == 0 && g_vol != 0.f) atomicAdd(acc + Set::VOL, g_vol);
  }
  batch_max_stage(local_max, wave_max, tid);
  __syncthreads();
  if (tid < Set::n_abs(a) && acc[tid] != 0.f) atomicAdd(a.g_log_abs + tid, acc[tid]);
  if (tid == Set::VOL && acc[Set::VOL] != 0.f) atomicAdd(a.g_vol_c, acc[Set::VOL]);
  batch_max_publish<DT_THREADS / 64>(wave_max, tid, a.g_absmax_bits);
}

// launches the backward kernel; the entry point has checked the arguments
template <class Set, bool EXTRA>
int dt_launch_bwd(const typename Set::Args& a, hipStream_t st) {
  // dynamic LDS is the whole allocation (the kernels declare no static __shared__) and must fit the 160 KiB of a CU.
  // Refused before anything is queued, the outputs untouched.
  const size_t lds = Set::bwd_lds_bytes(a);
  if (a.n_rays > 0 && lds > 160 * 1024) return SUNERF_E_UNSUPPORTED;
  const size_t n_abs = Set::n_abs(a);
  hipError_t e;
  if ((char*)a.g_vol_c == (char*)a.g_log_abs + n_abs * sizeof(float) &&
      (char*)a.g_absmax_bits == (char*)a.g_vol_c + sizeof(float)) {
    // the three small outputs in one buffer (what the Python wrapper passes): one clear instead of three
    if ((e = hipMemsetAsync(a.g_log_abs, 0, (n_abs + 2) * sizeof(float), st)) != hipSuccess) return (int)e;
  } else {
    if ((e = hipMemsetAsync(a.g_absmax_bits, 0, 4, st)) != hipSuccess) return (int)e;
    if ((e = hipMemsetAsync(a.g_log_abs, 0, n_abs * sizeof(float), st)) != hipSuccess) return (int)e;
    if ((e = hipMemsetAsync(a.g_vol_c, 0, sizeof(float), st)) != hipSuccess) return (int)e;
  }
  if (a.n_rays == 0) return 0;
  if (lds > 64 * 1024) {
    e = hipFuncSetAttribute((const void*)dt_bwd_kernel<Set, EXTRA>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    if (e != hipSuccess) return (int)e;
  }
  SUNERF_CLEAR_ERROR();
  int64_t groups = (a.n_rays + DT_RAYS - 1) / DT_RAYS;
  if (groups > DT_MAX_GRID) groups = DT_MAX_GRID;
  hipLaunchKernelGGL((dt_bwd_kernel<Set, EXTRA>), dim3((unsigned)groups), dim3(DT_THREADS), lds, st, a);
  SUNERF_CHECK_LAUNCH();
  return 0;
}
