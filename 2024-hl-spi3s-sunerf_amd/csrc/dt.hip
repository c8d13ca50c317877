// Density / temperature radiative-transfer integral (run_density_temperature.py path), forward and backward.
//
// Replaces DensityTemperatureRadiativeTransfer.raw2outputs / regularization, sunerf/rendering/density_temperature.py:192-274,
// the "+ base" of NeRF_DT.forward (sunerf/model/model.py:181-185) and the epilogues of base_tracing.py:99-110 for the DT
// subclass.  The MLP itself runs in the fused render kernel (render_fwd.hip) whose raw (N,S,2) output is the input here.
//
//   rho = exp(relu(raw0 + base_rho));  logT = relu(raw1 + base_T);  kappa_w = relu(log_abs[w])
//   A_j   = cumulative_trapezoid(rho kappa_w, z)_j                         j = 0..S-2   (density_temperature.py:261)
//   I_w   = trapezoid(exp(-A_j) rho_j^2 R_w(logT_j), z_j; j = 0..S-2) * vol_c * pixel_intensity_factor   (:263-265)
//   weights = relu(inf0) / (sum + 1e-10);  regularizing quantity = relu(inf0)
// R_w = linear interpolation of the AIA temperature response (x exposure time), 0 outside the table (Interp1D(...,
// extrap=0), restated from its documented semantics: parity unpinned for that sub-step) and 0 for an absent channel
// (wavelength entry <= 0).  The reference's per-wavelength Python loop with two host syncs per channel
// (density_temperature.py:245-256) becomes one launch.
//
// The integral itself (layout, sweeps, kernel bodies, backward launcher) is dt_sweep.h, shared with dt_response_set.hip; this
// file holds the AIA set policy -- the seven rows of dt_response.h -- the forward kernel and the entry points.
#include "dt_sweep.h"
#include "ordered_sum.h"
#include "dt_response.h"     // NCH, NTAB, channel_of(), response(): shared with volume.hip

namespace {

struct DtArgs : DtSweepArgs {
  const float* table_logt;   // (7,101) fp32
  const float* table_resp;   // (7,101) fp32, response x exposure time; log_abs is (7,) in the order 94,131,171,193,211,304,335
};

struct AiaSet {
  using Args = DtArgs;
  static constexpr int MAXW = NCH;
  // channel set-up of one ray (lane-uniform): table rows, absorption coefficient
  struct Channels {
    int ch[NCH];
    float kappa[NCH];
    __device__ __forceinline__ void init(const DtArgs& a, const float*, int64_t ray, int) {
#pragma unroll
      for (int w = 0; w < NCH; ++w) {
        ch[w] = w < a.W ? channel_of(a.wavelengths[ray * a.W + w]) : -1;
        kappa[w] = ch[w] >= 0 ? fmaxf(a.log_abs[ch[w]], 0.f) : 0.f;
      }
    }
  };
  static __device__ __forceinline__ void lookup(const DtArgs&, const Channels& C, int w, const float* tab, float logt, float& R,
                                                float& dR) {
    response(tab + C.ch[w] * 101, tab + NTAB + C.ch[w] * 101, logt, R, dR);
  }
  static __device__ __forceinline__ int stride(const DtArgs&) { return NCH; }
  // LDS floats: tables[2 NTAB] | g_kappa[7] g_vol | wave maxima[4] | [DT_RAYS][S][NCH] exp(-A); the forward has the tables only
  static constexpr int VOL = NCH, HEAD = 2 * NTAB + 8 + DT_THREADS / 64;
  static __host__ __device__ __forceinline__ int n_abs(const DtArgs&) { return NCH; }
  static __device__ __forceinline__ void stage(const DtArgs& a, float* lds, int tid) {
    for (int i = tid; i < NTAB; i += DT_THREADS) { lds[i] = a.table_logt[i]; lds[NTAB + i] = a.table_resp[i]; }
  }
  static __device__ __forceinline__ const float* tab(const float* lds) { return lds; }
  static __device__ __forceinline__ float* acc(float* lds) { return lds + 2 * NTAB; }
  static __device__ __forceinline__ float* wave_max(float* lds) { return lds + 2 * NTAB + 8; }
  static __device__ __forceinline__ float* slab(const DtArgs&, float* lds) { return lds + HEAD; }
  // S <= 705 fits the 160 KiB of a CU
  static size_t bwd_lds_bytes(const DtArgs& a) { return ((size_t)HEAD + (size_t)DT_RAYS * a.S * NCH) * sizeof(float); }
};

__global__ __launch_bounds__(DT_THREADS) void dt_integral_fwd_kernel(DtArgs a) {
  __shared__ float lds[2 * NTAB];
  dt_forward<AiaSet>(a, lds);
}

int check_common(const DtArgs& a) {
  if (a.n_rays == 0 && a.S >= 3 && a.W >= 1 && a.W <= NCH) return 0;
  if (!a.raw || !a.z_vals || !a.rays_o || !a.rays_d || !a.wavelengths || !a.table_logt || !a.table_resp || !a.log_abs || !a.vol_c)
    return SUNERF_E_BADARG;
  if (a.n_rays < 0 || a.S < 3) return SUNERF_E_BADARG;
  if (a.W < 1 || a.W > NCH) return SUNERF_E_UNSUPPORTED;
  return 0;
}

DtArgs common_args(const float* raw, const float* z_vals, const float* rays_o, const float* rays_d, const float* wavelengths,
                   int n_wavelengths, const float* table_logt, const float* table_resp, const float* log_abs, const float* vol_c,
                   float base_log_density, float base_log_temperature, float pixel_intensity_factor, float reg_radius,
                   int64_t n_rays, int n_samples) {
  DtArgs a = {};
  a.raw = raw; a.z_vals = z_vals; a.rays_o = rays_o; a.rays_d = rays_d; a.wavelengths = wavelengths; a.W = n_wavelengths;
  a.table_logt = table_logt; a.table_resp = table_resp; a.log_abs = log_abs; a.vol_c = vol_c; a.base_rho = base_log_density;
  a.base_t = base_log_temperature; a.pixel_factor = pixel_intensity_factor; a.reg_radius = reg_radius; a.n_rays = n_rays;
  a.S = n_samples;
  return a;
}

template <bool EXTRA>
int run_bwd(const DtArgs& a, void* stream) {
  if (int rc = check_common(a)) return rc;
  // an empty batch has null (N,...) tensors; its call only clears the scalar outputs
  if (!a.g_log_abs || !a.g_vol_c || !a.g_absmax_bits || (a.n_rays > 0 && (!a.g_image || !a.g_raw))) return SUNERF_E_BADARG;
  return dt_launch_bwd<AiaSet, EXTRA>(a, (hipStream_t)stream);
}

}  // namespace

namespace {

// SimpleStar.forward, sunerf/model/stellar_model.py:53-102 (Pascoe et al. 2019 eq. 4 and 6), at the sample points
// o + d z of sampling.py:100: the analytic density / temperature field that stands in for a trained NeRF_DT when synthetic
// observations are rendered (evaluation/image_render.py:236-268).  raw = (ln rho, log10 T).
struct StarArgs {
  const float* rays_o; const float* rays_d; const float* z_vals;
  int64_t n_rays; int S;
  float rho_0, h0, T0, Rs, t_photosphere;
  const float* params;       // device (Rs, h0, T0, rho_0) or null: then the four host floats above
  float* raw;
};

// one sample of the field: the radius, ln rho and log10 T, with the reference's masks (radius <= 1, > 1, <= Rs, > Rs)
struct StarSample {
  float radius, temp;
  float ln_rho, log_t;
};

__device__ __forceinline__ StarSample star_sample(const float* rays_o, const float* rays_d, int64_t ray, float z, float rho_0,
                                                  float h0, float T0, float Rs, float t_photosphere) {
  const float x = rays_o[ray * 3 + 0] + rays_d[ray * 3 + 0] * z;
  const float y = rays_o[ray * 3 + 1] + rays_d[ray * 3 + 1] * z;
  const float w = rays_o[ray * 3 + 2] + rays_d[ray * 3 + 2] * z;
  const float radius = sqrtf((x * x + y * y) + w * w);
  float rho = rho_0, temp = t_photosphere;
  if (radius > 1.f) {
    rho = rho_0 * expf((1.f / h0) * (1.f / radius - 1.f));
    temp = radius <= Rs ? (radius - 1.f) * ((T0 - t_photosphere) / (Rs - 1.f)) + t_photosphere : T0;
  }
  // a NaN radius (missed-sphere rays of SphericalSampler) fails every comparison of the reference's masks and leaves the
  // zero-initialised rho / temp: log(0) = -inf
  if (!(radius == radius)) { rho = 0.f; temp = 0.f; }
  StarSample s;
  s.radius = radius; s.temp = temp; s.ln_rho = logf(rho); s.log_t = log10f(temp);
  return s;
}

// PARAMS: the four stellar parameters come from a device array (the trainable ones, read after every optimiser step without a
// host round trip); same fp32 arithmetic either way
template <bool PARAMS>
__global__ __launch_bounds__(256) void simple_star_kernel(StarArgs a) {
  const int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= a.n_rays * a.S) return;
  float rho_0 = a.rho_0, h0 = a.h0, T0 = a.T0, Rs = a.Rs;
  if (PARAMS) { Rs = a.params[0]; h0 = a.params[1]; T0 = a.params[2]; rho_0 = a.params[3]; }
  const StarSample s = star_sample(a.rays_o, a.rays_d, idx / a.S, a.z_vals[idx], rho_0, h0, T0, Rs, a.t_photosphere);
  a.raw[idx * 2 + 0] = s.ln_rho;
  a.raw[idx * 2 + 1] = s.log_t;
}

// Backward of the field w.r.t. the four stellar parameters, given g_raw = dL / d(ln rho, log10 T) at every sample.  The masks
// carry no gradient (the reference's masked assignments, stellar_model.py:53-102); per sample, with L = log10 T:
//   every non-NaN radius: d ln rho / d rho_0 = 1 / rho_0
//   radius > 1:           d ln rho / d h0    = -(1/r - 1) / h0^2
//   1 < r <= Rs:          dL / dT0 = (r - 1) / ((Rs - 1) T ln 10),  dL / dRs = -(r - 1)(T0 - t_ph) / ((Rs - 1)^2 T ln 10)
//   r > Rs:               dL / dT0 = 1 / (T0 ln 10)
// so four sums over the samples carry everything, the parameter factors applied once at the end (rho_0 ~ 3e8: divided after
// summing):  A = sum g0,  B = sum_{r>1} g0 (1 - 1/r),  C = sum_{ramp} g1 (r - 1) / T,  D = sum_{r>Rs} g1.
// Pass 1: grid-stride over the samples, fp64 sums per lane -> per workgroup (fixed shuffle / LDS tree) -> partials[block][4].
// Pass 2: one workgroup adds the partials in a fixed order and writes (or adds) the four gradients.  No float atomics: the
// result does not depend on scheduling, and the grid depends on N*S only.
constexpr int STAR_BWD_THREADS = 256;
constexpr int STAR_BWD_MAX_GRID = 1024;
constexpr int STAR_BWD_WAVES = STAR_BWD_THREADS / 64;

// the four sums of every wave by sum64, parked for ordered_sum.h's wave-order stage (one barrier for all four: the caller's)
__device__ __forceinline__ void star_park_totals(const double (&acc)[4], double* red) {
  double totals[4];
#pragma unroll
  for (int k = 0; k < 4; ++k) totals[k] = sum64(acc[k]);
  park_wave_totals(totals, red);
}

__global__ __launch_bounds__(STAR_BWD_THREADS) void simple_star_bwd_partial_kernel(StarArgs a, const float* g_raw,
                                                                                    double* partials) {
  const float Rs = a.params[0], h0 = a.params[1], T0 = a.params[2], rho_0 = a.params[3];
  const int64_t total = a.n_rays * a.S;
  double acc[4] = {0., 0., 0., 0.};
  for (int64_t idx = (int64_t)blockIdx.x * STAR_BWD_THREADS + threadIdx.x; idx < total;
       idx += (int64_t)gridDim.x * STAR_BWD_THREADS) {
    const StarSample s = star_sample(a.rays_o, a.rays_d, idx / a.S, a.z_vals[idx], rho_0, h0, T0, Rs, a.t_photosphere);
    if (!(s.radius == s.radius)) continue;              // NaN radius: exactly no contribution
    const f32x2 g = *(const f32x2*)(g_raw + idx * 2);
    const double r = s.radius;
    acc[0] += g[0];
    if (s.radius > 1.f) {
      acc[1] += (double)g[0] * (1. - 1. / r);
      if (s.radius <= Rs) acc[2] += (double)g[1] * (r - 1.) / (double)s.temp;
      else acc[3] += g[1];
    }
  }
  __shared__ double red[STAR_BWD_WAVES * 4];
  star_park_totals(acc, red);
  __syncthreads();
  if (threadIdx.x < 4) partials[(size_t)blockIdx.x * 4 + threadIdx.x] = sum_in_wave_order<STAR_BWD_WAVES, 4>(red, threadIdx.x);
}

__global__ __launch_bounds__(STAR_BWD_THREADS) void simple_star_bwd_finish_kernel(StarArgs a, const double* partials,
                                                                                   int n_partials, float* g_params,
                                                                                   int accumulate) {
  double acc[4] = {0., 0., 0., 0.};
  for (int b = threadIdx.x; b < n_partials; b += STAR_BWD_THREADS) {
#pragma unroll
    for (int k = 0; k < 4; ++k) acc[k] += partials[(size_t)b * 4 + k];
  }
  __shared__ double red[STAR_BWD_WAVES * 4];
  star_park_totals(acc, red);
  __syncthreads();
  if (threadIdx.x != 0) return;
  double S[4];
#pragma unroll
  for (int k = 0; k < 4; ++k) S[k] = sum_in_wave_order<STAR_BWD_WAVES, 4>(red, k);
  const double Rs = a.params[0], h0 = a.params[1], T0 = a.params[2], rho_0 = a.params[3], tph = a.t_photosphere;
  const double ln10 = 2.302585092994045684;
  // the ramp sums vanish when no sample lies on it: no 0 / 0 for Rs == 1
  const double ramp = S[2] != 0. ? S[2] / ((Rs - 1.) * ln10) : 0.;
  const double g[4] = {S[2] != 0. ? -ramp * (T0 - tph) / (Rs - 1.) : 0.,      // Rs
                       S[1] / (h0 * h0),                                          // h0
                       ramp + (S[3] != 0. ? S[3] / (T0 * ln10) : 0.),             // T0
                       S[0] / rho_0};                                             // rho_0
#pragma unroll
  for (int k = 0; k < 4; ++k) g_params[k] = accumulate ? (float)((double)g_params[k] + g[k]) : (float)g[k];
}

int star_args(StarArgs& a, const float* rays_o, const float* rays_d, const float* z_vals, int64_t n_rays, int n_samples) {
  if (n_rays < 0 || n_samples < 1) return SUNERF_E_BADARG;
  a.rays_o = rays_o; a.rays_d = rays_d; a.z_vals = z_vals; a.n_rays = n_rays; a.S = n_samples;
  if (n_rays == 0) return 0;
  if (!rays_o || !rays_d || !z_vals) return SUNERF_E_BADARG;
  return 0;
}

}  // namespace

extern "C" int sunerf_simple_star_field(const float* rays_o, const float* rays_d, const float* z_vals, int64_t n_rays,
                                        int n_samples, float rho_0, float h0, float T0, float Rs, float t_photosphere,
                                        float* raw, void* stream) {
  StarArgs a = {};
  if (int rc = star_args(a, rays_o, rays_d, z_vals, n_rays, n_samples)) return rc;
  if (n_rays == 0) return 0;
  if (!raw) return SUNERF_E_BADARG;
  a.rho_0 = rho_0; a.h0 = h0; a.T0 = T0; a.Rs = Rs; a.t_photosphere = t_photosphere; a.raw = raw;
  const int64_t total = n_rays * n_samples;
  SUNERF_CLEAR_ERROR();
  hipLaunchKernelGGL(simple_star_kernel<false>, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, (hipStream_t)stream, a);
  SUNERF_CHECK_LAUNCH();
  return 0;
}

extern "C" int sunerf_simple_star_field_dev(const float* rays_o, const float* rays_d, const float* z_vals, int64_t n_rays,
                                            int n_samples, const float* params, float t_photosphere, float* raw,
                                            void* stream) {
  StarArgs a = {};
  if (int rc = star_args(a, rays_o, rays_d, z_vals, n_rays, n_samples)) return rc;
  if (n_rays == 0) return 0;
  if (!params || !raw) return SUNERF_E_BADARG;
  a.params = params; a.t_photosphere = t_photosphere; a.raw = raw;
  const int64_t total = n_rays * n_samples;
  SUNERF_CLEAR_ERROR();
  hipLaunchKernelGGL(simple_star_kernel<true>, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, (hipStream_t)stream, a);
  SUNERF_CHECK_LAUNCH();
  return 0;
}

extern "C" size_t sunerf_simple_star_bwd_workspace_bytes(void) {
  return (size_t)STAR_BWD_MAX_GRID * 4 * sizeof(double);
}

extern "C" int sunerf_simple_star_bwd(const float* rays_o, const float* rays_d, const float* z_vals, int64_t n_rays,
                                      int n_samples, const float* params, float t_photosphere, const float* g_raw,
                                      void* workspace, size_t workspace_bytes, float* g_params, int accumulate, void* stream) {
  StarArgs a = {};
  if (int rc = star_args(a, rays_o, rays_d, z_vals, n_rays, n_samples)) return rc;
  if (!params || !g_params || !workspace || (n_rays > 0 && !g_raw)) return SUNERF_E_BADARG;
  if (workspace_bytes < sunerf_simple_star_bwd_workspace_bytes()) return SUNERF_E_WORKSPACE;
  a.params = params; a.t_photosphere = t_photosphere;
  const int64_t total = n_rays * n_samples;
  int64_t grid = (total + STAR_BWD_THREADS - 1) / STAR_BWD_THREADS;
  if (grid > STAR_BWD_MAX_GRID) grid = STAR_BWD_MAX_GRID;
  hipStream_t st = (hipStream_t)stream;
  SUNERF_CLEAR_ERROR();
  if (grid > 0)
    hipLaunchKernelGGL(simple_star_bwd_partial_kernel, dim3((unsigned)grid), dim3(STAR_BWD_THREADS), 0, st, a, g_raw,
                       (double*)workspace);
  hipLaunchKernelGGL(simple_star_bwd_finish_kernel, dim3(1), dim3(STAR_BWD_THREADS), 0, st, a, (const double*)workspace,
                     (int)grid, g_params, accumulate);
  SUNERF_CHECK_LAUNCH();
  return 0;
}

extern "C" int sunerf_dt_integral_fwd(const float* raw, const float* z_vals, const float* rays_o, const float* rays_d,
                                      const float* wavelengths, int n_wavelengths, const float* table_logt,
                                      const float* table_resp, const float* log_abs, const float* vol_c, float base_log_density,
                                      float base_log_temperature, float pixel_intensity_factor, float reg_radius,
                                      int64_t n_rays, int n_samples, float* image, float* weights, float* reg_q,
                                      float* height_map, float* absorption_map, float* regularization, void* stream) {
  DtArgs a = common_args(raw, z_vals, rays_o, rays_d, wavelengths, n_wavelengths, table_logt, table_resp, log_abs, vol_c,
                         base_log_density, base_log_temperature, pixel_intensity_factor, reg_radius, n_rays, n_samples);
  a.image = image; a.weights = weights; a.reg_q = reg_q; a.height_map = height_map; a.absorption_map = absorption_map;
  a.regularization = regularization;
  if (int rc = check_common(a)) return rc;
  if (n_rays == 0) return 0;
  if (!image || !weights || !reg_q) return SUNERF_E_BADARG;
  SUNERF_CLEAR_ERROR();
  hipLaunchKernelGGL(dt_integral_fwd_kernel, dim3((unsigned)((n_rays + DT_RAYS - 1) / DT_RAYS)), dim3(DT_THREADS), 0,
                     (hipStream_t)stream, a);
  SUNERF_CHECK_LAUNCH();
  return 0;
}

extern "C" int sunerf_dt_integral_bwd(const float* raw, const float* z_vals, const float* rays_o, const float* rays_d,
                                      const float* wavelengths, int n_wavelengths, const float* table_logt,
                                      const float* table_resp, const float* log_abs, const float* vol_c, float base_log_density,
                                      float base_log_temperature, float pixel_intensity_factor, float reg_radius,
                                      int64_t n_rays, int n_samples, const float* g_image, const float* g_reg, float* g_raw,
                                      float* g_log_abs, float* g_vol_c, void* g_absmax, void* stream) {
  DtArgs a = common_args(raw, z_vals, rays_o, rays_d, wavelengths, n_wavelengths, table_logt, table_resp, log_abs, vol_c,
                         base_log_density, base_log_temperature, pixel_intensity_factor, reg_radius, n_rays, n_samples);
  a.g_image = g_image; a.g_reg = g_reg; a.g_raw = g_raw; a.g_log_abs = g_log_abs; a.g_vol_c = g_vol_c;
  a.g_absmax_bits = (unsigned*)g_absmax;
  return run_bwd<false>(a, stream);
}

extern "C" int sunerf_dt_integral_bwd_full(const float* raw, const float* z_vals, const float* rays_o, const float* rays_d,
                                           const float* wavelengths, int n_wavelengths, const float* table_logt,
                                           const float* table_resp, const float* log_abs, const float* vol_c,
                                           float base_log_density, float base_log_temperature, float pixel_intensity_factor,
                                           float reg_radius, int64_t n_rays, int n_samples, const float* g_image,
                                           const float* g_reg, const float* g_weights, const float* g_reg_q, float* g_raw,
                                           float* g_log_abs, float* g_vol_c, void* g_absmax, void* stream) {
  DtArgs a = common_args(raw, z_vals, rays_o, rays_d, wavelengths, n_wavelengths, table_logt, table_resp, log_abs, vol_c,
                         base_log_density, base_log_temperature, pixel_intensity_factor, reg_radius, n_rays, n_samples);
  a.g_image = g_image; a.g_reg = g_reg; a.g_raw = g_raw; a.g_log_abs = g_log_abs; a.g_vol_c = g_vol_c;
  a.g_absmax_bits = (unsigned*)g_absmax; a.g_weights = g_weights; a.g_reg_q = g_reg_q;
  return run_bwd<true>(a, stream);
}
