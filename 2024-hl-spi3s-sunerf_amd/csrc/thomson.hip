// White-light Thomson-scattering integral (total and polarised brightness), forward and backward.
//
// Replaces ThompsonScattering.raw2outputs, sunerf/rendering/thompson.py:17-109 (Howard & Tappin 2009, eqs. 23, 24, 29),
// with the defects of the reference resolved: the radius of a sample is that of its three spatial
// coordinates, and the geometry is evaluated in fp64.  Per ray (o, d, l = |d|) and sample j = 0..S-1:
//
//   x_j = o + d z_j,  r_j = |x_j|,  R = solar_radius,  D_j = (z_j - z_{j-1}) l  (D_0 = D_1; none for S = 1)
//   rho_j = exp(kappa raw_j[0])                      (kappa = ln 10 for a NeRF: 10 ** raw; 1 for a field answering ln rho)
//   s = sin(Omega) = R / r,  c = cos(Omega),  L = ln((1 + s) / c) = atanh(s)
//   A = c s^2                      B = -(1/8) (1 - 3 s^2 - (c^2 / s)(1 + 3 s^2) L)
//   C = 4/3 - c - c^3/3            D = (1/8) (5 + s^2 - (c^2 / s)(5 - s^2) L)
//   sin^2(chi) = |o x d|^2 / (l^2 r^2),   u = limb_darkening_coeff
//   I_T = (1-u) C + u D,   I_P = sin^2(chi) ((1-u) A + u B),   I_tot = 2 I_T - I_P
//   |I_tot|, |I_P|, both 0 where r <= R or a value is not finite (nan_to_num, thompson.py:76-80)
//   Seams: the limb is inside (r == R by bits gives 0, as does one fp32 step of z further in; one step out gives the limb
//   values); d = 0 makes sin^2(chi) = 0 / 0, so both intensities are 0, as are all line elements; a ray through the centre has
//   |o x d| = 0 and I_P = 0 exactly; a sample at the origin (R / r = inf) is inside; repeated z give D_j = 0.
//
//   pixel_B = C_0 (sum rho |I_tot| D, sum rho |I_P| D),  pixel_density = sum rho D,  M = sum rho
//   distance_from_sun = sum rho r / (M + 1e-10),  distance_from_obs = sum rho z l / (M + 1e-10),  weights = rho / (M + 1e-10)
//
// Numerics: A..D are differences that cancel to O(s^2) far from the Sun (C ~ s^2, B ~ D ~ 2/3 s^2), so in fp32 the relative
// error grows as 2^-24 / s^2 (8 % at 215 solar radii).  The sample point, its radius and A..D are evaluated in fp64 from the
// fp32 inputs (C in the cancellation-free form (1 - c)(4 + c + c^2) / 3 with 1 - c = s^2 / (1 + c), L as log1p, c^2 as
// (r^2 - R^2) / r^2): the residual relative error is ~1e-16 / s^2.  The sums stay fp32 (positive terms).
//
// Layout as dt.hip: 32 lanes per ray, one sample per lane and 32-sample chunk (coalesced reads of raw / z, coalesced writes),
// per-ray sums over the ray's own lanes (butterfly), no float atomics: reruns are bit-identical.  The backward also writes
// the bit pattern of max |g_raw| (one integer atomic max per workgroup) that the MLP backward takes as its gradient scale.
#include "sunerf_common.h"
#include "ray_scan.h"
#include "thomson_math.h"
#include "../../include/sunerf_hip.h"

namespace {

constexpr int TH_THREADS = 256;
constexpr int TH_RAYS = TH_THREADS / 32;      // rays per workgroup (and per step of its walk over the batch)
constexpr int TH_MAX_GRID = 1024;             // backward: workgroups of the grid (one atomic max each)

struct ThomsonArgs {
  const float* raw;          // (N,S,C) channel 0 = log density (log10 rho for a NeRF, ln rho for a field)
  const float* z_vals;       // (N,S)
  const float* rays_o;       // (N,3)
  const float* rays_d;       // (N,3)
  const float* solar_radius; // (1,)  the module's buffers, read on the device
  const float* limb;         // (1,)
  const float* c0;           // (1,)
  float kappa;
  int64_t n_rays;
  int S, C;
  // forward outputs
  float* pixel_b;            // (N,2)
  float* pixel_density;      // (N,)
  float* dist_sun;           // (N,)
  float* dist_obs;           // (N,)
  float* weights;            // (N,S)
  // backward: gradients of the five outputs, each optional
  const float* g_pixel_b;    // (N,2)
  const float* g_density;    // (N,)
  const float* g_dist_sun;   // (N,)
  const float* g_dist_obs;   // (N,)
  const float* g_weights;    // (N,S)
  float* g_raw;              // (N,S,C)
  unsigned* g_absmax_bits;   // (1,) or null
};

// lane-uniform quantities of one ray
struct Ray {
  double ox, oy, oz, dx, dy, dz;
  double p2;                 // |o x d|^2 / l^2: squared impact parameter, sin^2(chi) = p2 / r^2
  float len;                 // l = |d| (fp32, as the reference's torch.norm)
  __device__ __forceinline__ void init(const ThomsonArgs& a, int64_t ray) {
    const float* o = a.rays_o + ray * 3;
    const float* d = a.rays_d + ray * 3;
    ox = o[0]; oy = o[1]; oz = o[2];
    dx = d[0]; dy = d[1]; dz = d[2];
    len = sqrtf((d[0] * d[0] + d[1] * d[1]) + d[2] * d[2]);
    const double cx = oy * dz - oz * dy, cy = oz * dx - ox * dz, cz = ox * dy - oy * dx;
    p2 = (cx * cx + cy * cy + cz * cz) / (dx * dx + dy * dy + dz * dz);
  }
};

struct Sample {
  float r;                   // |x_j|
  float i_tot, i_p;          // |I_tot|, |I_P| (0 inside the Sun / where not finite)
};

// radius of the sample at z and, when WANT_I, the two scattering intensities per electron
template <bool WANT_I>
__device__ __forceinline__ Sample sample_geometry(const Ray& ry, float z, double R, double u) {
  const double zz = z;
  const double px = ry.ox + ry.dx * zz, py = ry.oy + ry.dy * zz, pz = ry.oz + ry.dz * zz;
  const double r2 = px * px + py * py + pz * pz;
  const double r = sqrt(r2);
  Sample o;
  o.r = (float)r;
  o.i_tot = o.i_p = 0.f;
  // inside / on the Sun, or a NaN point.  (On the limb itself c = 0 and (c^2 / s) L below is 0 * inf: the finite check at the
  // end would zero r == R as well, so `>` and `>=` compute the same here; the comparison states the contract.)
  if (!WANT_I || !(r > R)) return o;
  const ThomsonIntensity e = thomson_intensity(r2, r, R, u, ry.p2);   // thomson_math.h: A..D, I_T, I_P, I_tot in fp64
  const float ft = (float)fabs(e.i_tot), fp = (float)fabs(e.i_p);
  if (isfinite(ft) && isfinite(fp)) { o.i_tot = ft; o.i_p = fp; }
  return o;
}

// line element of sample i: (z_i - z_{i-1}) l, the first one repeated; 0 when the ray has one sample
__device__ __forceinline__ float line_element(const float* z, int i, int S, float len) {
  if (S < 2) return 0.f;
  return (i >= 1 ? z[i] - z[i - 1] : z[1] - z[0]) * len;
}

__global__ __launch_bounds__(TH_THREADS) void thomson_integral_fwd_kernel(ThomsonArgs a) {
  const int tid = threadIdx.x, n = tid & 31, sub = tid >> 5;
  const int64_t ray = (int64_t)blockIdx.x * TH_RAYS + sub;
  if (ray >= a.n_rays) return;                     // (a whole 32-lane group leaves: the shuffles are 32 wide)
  const int S = a.S, n_chunks = (S + 31) >> 5;
  const double R = a.solar_radius[0], u = a.limb[0];
  const float c0 = a.c0[0];
  Ray ry;
  ry.init(a, ray);
  const float* z = a.z_vals + ray * S;
  const float* raw = a.raw + ray * S * a.C;
  float tb = 0.f, pb = 0.f, den = 0.f, m = 0.f, nsun = 0.f, nobs = 0.f;
  for (int c = 0; c < n_chunks; ++c) {
    const int i = 32 * c + n;
    if (i >= S) break;
    const float zi = z[i];
    const float rho = expf(a.kappa * raw[(size_t)i * a.C]);
    const Sample g = sample_geometry<true>(ry, zi, R, u);
    if (S >= 2) {
      const float dl = line_element(z, i, S, ry.len);
      tb += rho * g.i_tot * dl;
      pb += rho * g.i_p * dl;
      den += rho * dl;
    }
    m += rho;
    nsun += rho * g.r;
    nobs += rho * (zi * ry.len);
  }
  tb = sum32(tb); pb = sum32(pb); den = sum32(den);
  m = sum32(m); nsun = sum32(nsun); nobs = sum32(nobs);
  const float denom = m + 1e-10f;
  for (int c = 0; c < n_chunks; ++c) {
    const int i = 32 * c + n;
    if (i >= S) break;
    a.weights[ray * S + i] = expf(a.kappa * raw[(size_t)i * a.C]) / denom;
  }
  if (n == 0) {
    const f32x2 b = {c0 * tb, c0 * pb};
    *(f32x2*)(a.pixel_b + ray * 2) = b;
    a.pixel_density[ray] = den;
    a.dist_sun[ray] = nsun / denom;
    a.dist_obs[ray] = nobs / denom;
  }
}

// dL/drho_j = C_0 (g_tB |I_tot| + g_pB |I_P|) D_j + g_den D_j + (g_sun r_j + g_obs z_j l + g_w_j) / M'
//             - (g_sun N_sun + g_obs N_obs + sum_k g_w_k rho_k) / M'^2,          M' = M + 1e-10,  g_raw_j[0] = kappa rho_j dL/drho_j
// The per-ray sums of the ratio outputs (M, N_sun, N_obs, sum g_w rho) take a first sweep when one of their gradients is given.
__global__ __launch_bounds__(TH_THREADS) void thomson_integral_bwd_kernel(ThomsonArgs a) {
  __shared__ float wave_max[TH_THREADS / 64];
  const int tid = threadIdx.x, n = tid & 31, sub = tid >> 5;
  const int S = a.S, n_chunks = (S + 31) >> 5;
  const double R = a.solar_radius[0], u = a.limb[0];
  const float c0 = a.c0[0];
  const bool ratios = a.g_dist_sun || a.g_dist_obs || a.g_weights;
  const bool want_i = a.g_pixel_b != nullptr;
  const bool need_r = want_i || a.g_dist_sun;
  float local_max = 0.f;
  const int64_t n_groups = (a.n_rays + TH_RAYS - 1) / TH_RAYS;
  for (int64_t grp = blockIdx.x; grp < n_groups; grp += gridDim.x) {
    const int64_t ray = grp * TH_RAYS + sub;
    if (ray >= a.n_rays) continue;       // the 32 lanes of a ray stay together; no block-wide barrier inside the walk
    Ray ry;
    ry.init(a, ray);
    const float* z = a.z_vals + ray * S;
    const float* raw = a.raw + ray * S * a.C;
    const float g_tb = want_i ? a.g_pixel_b[ray * 2] * c0 : 0.f;
    const float g_pb = want_i ? a.g_pixel_b[ray * 2 + 1] * c0 : 0.f;
    const float g_den = a.g_density ? a.g_density[ray] : 0.f;
    const float g_sun = a.g_dist_sun ? a.g_dist_sun[ray] : 0.f;
    const float g_obs = a.g_dist_obs ? a.g_dist_obs[ray] : 0.f;
    float inv = 0.f, shift = 0.f;
    if (ratios) {
      float m = 0.f, nsun = 0.f, nobs = 0.f, gwr = 0.f;
      for (int c = 0; c < n_chunks; ++c) {
        const int i = 32 * c + n;
        if (i >= S) break;
        const float rho = expf(a.kappa * raw[(size_t)i * a.C]);
        m += rho;
        if (a.g_dist_sun) nsun += rho * sample_geometry<false>(ry, z[i], R, u).r;
        if (a.g_dist_obs) nobs += rho * (z[i] * ry.len);
        if (a.g_weights) gwr += a.g_weights[ray * S + i] * rho;
      }
      m = sum32(m); nsun = sum32(nsun); nobs = sum32(nobs); gwr = sum32(gwr);
      const float denom = m + 1e-10f;
      inv = 1.f / denom;
      shift = (g_sun * nsun + g_obs * nobs + gwr) / (denom * denom);
    }
    for (int c = 0; c < n_chunks; ++c) {
      const int i = 32 * c + n;
      if (i >= S) break;
      const float zi = z[i];
      const float rho = expf(a.kappa * raw[(size_t)i * a.C]);
      float g = 0.f;
      if (need_r || S >= 2) {
        const Sample s = want_i ? sample_geometry<true>(ry, zi, R, u)
                                : (need_r ? sample_geometry<false>(ry, zi, R, u) : Sample{0.f, 0.f, 0.f});
        if (S >= 2) {
          const float dl = line_element(z, i, S, ry.len);
          g += (g_tb * s.i_tot + g_pb * s.i_p + g_den) * dl;
        }
        if (ratios) g += g_sun * s.r * inv;
      }
      if (ratios) {
        g += g_obs * (zi * ry.len) * inv;
        if (a.g_weights) g += a.g_weights[ray * S + i] * inv;
        g -= shift;
      }
      const float g0 = a.kappa * rho * g;
      float* out = a.g_raw + ((size_t)ray * S + i) * a.C;
      if (a.C == 2) {
        const f32x2 gg = {g0, 0.f};
        *(f32x2*)out = gg;
      } else {
        out[0] = g0;
      }
      local_max = fmaxf(local_max, fabsf(g0));
    }
  }
  batch_max_stage(local_max, wave_max, tid);
  __syncthreads();
  if (a.g_absmax_bits) batch_max_publish<TH_THREADS / 64>(wave_max, tid, a.g_absmax_bits);   // (null: the caller wants no maximum)
}

int check_inputs(const ThomsonArgs& a) {
  if (a.n_rays < 0 || a.S < 1 || (a.C != 1 && a.C != 2)) return SUNERF_E_BADARG;
  if (!a.solar_radius || !a.limb || !a.c0) return SUNERF_E_BADARG;
  if (a.n_rays > 0 && (!a.raw || !a.z_vals || !a.rays_o || !a.rays_d)) return SUNERF_E_BADARG;
  return 0;
}

ThomsonArgs make_args(const float* raw, int n_channels, float kappa, const float* z_vals, const float* rays_o,
                      const float* rays_d, const float* solar_radius, const float* limb_darkening_coeff, const float* c0,
                      int64_t n_rays, int n_samples) {
  ThomsonArgs a = {};
  a.raw = raw; a.C = n_channels; a.kappa = kappa; a.z_vals = z_vals; a.rays_o = rays_o; a.rays_d = rays_d;
  a.solar_radius = solar_radius; a.limb = limb_darkening_coeff; a.c0 = c0; a.n_rays = n_rays; a.S = n_samples;
  return a;
}

}  // namespace

extern "C" int sunerf_thomson_integral_fwd(const float* raw, int n_channels, float kappa, const float* z_vals,
                                           const float* rays_o, const float* rays_d, const float* solar_radius,
                                           const float* limb_darkening_coeff, const float* c0, int64_t n_rays, int n_samples,
                                           float* pixel_b, float* pixel_density, float* distance_from_sun,
                                           float* distance_from_obs, float* weights, void* stream) {
  ThomsonArgs a = make_args(raw, n_channels, kappa, z_vals, rays_o, rays_d, solar_radius, limb_darkening_coeff, c0, n_rays,
                            n_samples);
  a.pixel_b = pixel_b; a.pixel_density = pixel_density; a.dist_sun = distance_from_sun; a.dist_obs = distance_from_obs;
  a.weights = weights;
  if (int rc = check_inputs(a)) return rc;
  if (n_rays > 0 && (!pixel_b || !pixel_density || !distance_from_sun || !distance_from_obs || !weights)) return SUNERF_E_BADARG;
  if (n_rays == 0) return 0;
  SUNERF_CLEAR_ERROR();
  hipLaunchKernelGGL(thomson_integral_fwd_kernel, dim3((unsigned)((n_rays + TH_RAYS - 1) / TH_RAYS)), dim3(TH_THREADS), 0,
                     (hipStream_t)stream, a);
  SUNERF_CHECK_LAUNCH();
  return 0;
}

extern "C" int sunerf_thomson_integral_bwd(const float* raw, int n_channels, float kappa, const float* z_vals,
                                           const float* rays_o, const float* rays_d, const float* solar_radius,
                                           const float* limb_darkening_coeff, const float* c0, int64_t n_rays, int n_samples,
                                           const float* g_pixel_b, const float* g_pixel_density,
                                           const float* g_distance_from_sun, const float* g_distance_from_obs,
                                           const float* g_weights, float* g_raw, void* g_absmax, void* stream) {
  ThomsonArgs a = make_args(raw, n_channels, kappa, z_vals, rays_o, rays_d, solar_radius, limb_darkening_coeff, c0, n_rays,
                            n_samples);
  a.g_pixel_b = g_pixel_b; a.g_density = g_pixel_density; a.g_dist_sun = g_distance_from_sun;
  a.g_dist_obs = g_distance_from_obs; a.g_weights = g_weights; a.g_raw = g_raw; a.g_absmax_bits = (unsigned*)g_absmax;
  if (int rc = check_inputs(a)) return rc;
  if (n_rays > 0 && !g_raw) return SUNERF_E_BADARG;
  hipStream_t st = (hipStream_t)stream;
  if (g_absmax) {
    hipError_t e = hipMemsetAsync(g_absmax, 0, 4, st);
    if (e != hipSuccess) return (int)e;
  }
  if (n_rays == 0) return 0;
  SUNERF_CLEAR_ERROR();
  int64_t groups = (n_rays + TH_RAYS - 1) / TH_RAYS;
  if (groups > TH_MAX_GRID) groups = TH_MAX_GRID;
  hipLaunchKernelGGL(thomson_integral_bwd_kernel, dim3((unsigned)groups), dim3(TH_THREADS), 0, st, a);
  SUNERF_CHECK_LAUNCH();
  return 0;
}
