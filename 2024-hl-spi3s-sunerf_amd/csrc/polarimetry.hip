// White-light polarimetry (include/sunerf_hip_polarimetry.h): polariser exposures to Stokes planes, tB and
// pB, and the polarisation-ratio depth of a (tB, pB) pair.  Two kernels, each one lane per pixel or ray: consecutive lanes take
// consecutive pixels of a plane, so each of the n_frames loads of a wave is one coalesced row of 256 bytes.
//
// stokes: the samples of a pixel live in registers.  The kernel is written for SUNERF_POLARIMETRY_MAX_FRAMES = 8 samples with every
// loop over them unrolled and `k < n_frames` as a predicate: no loop indexes its registers, nothing goes to scratch.  A register past
// the last frame loads the last frame again (the same line) and is not valid.  The design rows g_k come in the kernel's argument
// block (scalar registers): the device does no trigonometry.  The 3 x 3 normal equations are solved by LDL^T with + - * / alone, in
// the order the header writes out, so the fp64 restatement of the tests gives the same values.
//
// ratio_depth: 64 bisection steps through thomson_math.h, the text thomson.hip evaluates at every sample; a fixed count without an
// early exit, so a wave does not diverge inside the loop and reruns are bit-identical.
//
// Counts are integers, summed per workgroup in LDS and added to the plane's row with integer atomics; there is no floating-point
// atomic and no floating-point sum across threads.  -ffp-contract=off and no explicit fma: every operation is rounded on its own.
#include "sunerf_common.h"
#include "thomson_math.h"
#include "../../include/sunerf_hip_polarimetry.h"

namespace {

constexpr int PL_THREADS = 256;          // pixels of one plane, or rays, per workgroup
constexpr int PL_MAX = SUNERF_POLARIMETRY_MAX_FRAMES;
constexpr double PL_EPS = 0x1p-40;

struct StokesArgs {
  double g[PL_MAX][3];          // the design rows, formed on the host
  double cy, cx;
  int n_frames, n_planes, width;
  int64_t plane_px, chunks_per_plane, n_chunks;
};

struct StokesOut {
  float *stokes, *tb, *pb, *pb_cross, *chi2, *sigma_tb, *sigma_pb;
  uint8_t* status;
  unsigned long long* counts;
};

__global__ __launch_bounds__(PL_THREADS) void stokes_kernel(const float* __restrict__ frames, const uint8_t* __restrict__ bad,
                                                            const double* __restrict__ va, const double* __restrict__ vb,
                                                            StokesOut o, StokesArgs a) {
  __shared__ unsigned tally[SUNERF_POLARIMETRY_COUNTS];
  const double inf = __builtin_inf();
  const float nanf_ = __builtin_nanf("");
  const int64_t frame_px = a.plane_px * a.n_planes;
  const bool model = va != nullptr;
  for (int64_t chunk = blockIdx.x; chunk < a.n_chunks; chunk += gridDim.x) {
    const int64_t plane = chunk / a.chunks_per_plane;
    const int64_t in_plane = (chunk - plane * a.chunks_per_plane) * PL_THREADS + threadIdx.x;
    if (threadIdx.x < SUNERF_POLARIMETRY_COUNTS) tally[threadIdx.x] = 0;
    __syncthreads();
    if (in_plane < a.plane_px) {
      const int64_t px = plane * a.plane_px + in_plane;
      const int last_frame = a.n_frames - 1;
      unsigned flagged = 0;
      if (bad) {
#pragma unroll
        for (int k = 0; k < PL_MAX; ++k) flagged |= (unsigned)(bad[(k < last_frame ? k : last_frame) * frame_px + px] != 0) << k;
      }
      float v[PL_MAX];
#pragma unroll
      for (int k = 0; k < PL_MAX; ++k) v[k] = frames[(k < last_frame ? k : last_frame) * frame_px + px];
      const double pa = model ? va[plane] : 0.0, pb_ = model ? vb[plane] : 0.0;

      double w[PL_MAX];
      int n_valid = 0;
      double m00 = 0.0, m01 = 0.0, m02 = 0.0, m11 = 0.0, m12 = 0.0, m22 = 0.0, r0 = 0.0, r1 = 0.0, r2 = 0.0;
#pragma unroll
      for (int k = 0; k < PL_MAX; ++k) {
        const double y = (double)v[k];
        bool valid = k < a.n_frames && fabs(y) < inf && !(flagged >> k & 1);
        double wk = 1.0;
        if (model) {
          const double var = pa + pb_ * (y > 0.0 ? y : 0.0);
          valid = valid && var > 0.0 && var < inf;
          wk = 1.0 / var;
        }
        w[k] = valid ? wk : 0.0;
        if (valid) {
          const double p0 = wk * a.g[k][0], p1 = wk * a.g[k][1], p2 = wk * a.g[k][2];
          m00 += p0 * a.g[k][0]; m01 += p0 * a.g[k][1]; m02 += p0 * a.g[k][2];
          m11 += p1 * a.g[k][1]; m12 += p1 * a.g[k][2];
          m22 += p2 * a.g[k][2];
          r0 += p0 * y; r1 += p1 * y; r2 += p2 * y;
          ++n_valid;
        }
      }

      // LDL^T in the header's order; a quotient by a pivot that fails its test is formed and not used
      const double d0 = m00;
      const double l10 = m01 / d0, l20 = m02 / d0;
      const double d1 = m11 - l10 * m01;
      const double t21 = m12 - l20 * m01, l21 = t21 / d1;
      const double d2 = (m22 - l20 * m02) - l21 * t21;
      const bool solved = n_valid >= SUNERF_POLARIMETRY_MIN_FRAMES && d0 > PL_EPS * m00 && d1 > PL_EPS * m11 && d2 > PL_EPS * m22;
      const double z0 = r0, z1 = r1 - l10 * z0, z2 = (r2 - l20 * z0) - l21 * z1;
      const double U = z2 / d2;
      const double Q = z1 / d1 - l21 * U;
      const double I = (z0 / d0 - l10 * Q) - l20 * U;

      double chi = 0.0;
#pragma unroll
      for (int k = 0; k < PL_MAX; ++k) {
        const double e = (double)v[k] - ((a.g[k][0] * I + a.g[k][1] * Q) + a.g[k][2] * U);
        chi = w[k] != 0.0 ? chi + (w[k] * e) * e : chi;          // (a valid sample has w > 0: 0 < var < inf)
      }

      const int64_t row = in_plane / a.width;
      const double dx = (double)(in_plane - row * a.width) - a.cx, dy = (double)row - a.cy;
      const double nn = dx * dx + dy * dy;
      const bool centre = nn == 0.0;
      const double C2 = (dx * dx - dy * dy) / nn, S2 = (2.0 * (dx * dy)) / nn;
      const double pbv = -(Q * C2 + U * S2), cross = Q * S2 - U * C2;
      const double gg = l10 * l21 - l20;
      const double c22 = 1.0 / d2, c12 = -l21 / d2, c11 = 1.0 / d1 + (l21 * l21) / d2;
      const double c00 = (1.0 / d0 + (l10 * l10) / d1) + (gg * gg) / d2;
      const double s_tb = sqrt(c00), s_pb = sqrt((c11 * (C2 * C2) + 2.0 * (c12 * (C2 * S2))) + c22 * (S2 * S2));

      const bool rot = solved && !centre;
      if (o.stokes) {
        o.stokes[px] = solved ? (float)I : nanf_;
        o.stokes[frame_px + px] = solved ? (float)Q : nanf_;
        o.stokes[2 * frame_px + px] = solved ? (float)U : nanf_;
      }
      o.tb[px] = solved ? (float)I : nanf_;
      o.pb[px] = rot ? (float)pbv : nanf_;
      if (o.pb_cross) o.pb_cross[px] = rot ? (float)cross : nanf_;
      if (o.chi2) o.chi2[px] = solved ? (float)chi : nanf_;
      if (o.sigma_tb) o.sigma_tb[px] = (solved && model) ? (float)s_tb : nanf_;
      if (o.sigma_pb) o.sigma_pb[px] = (rot && model) ? (float)s_pb : nanf_;
      const int st = !solved ? SUNERF_POLARIMETRY_UNDETERMINED : (centre ? SUNERF_POLARIMETRY_CENTRE : SUNERF_POLARIMETRY_DETERMINED);
      if (o.status) o.status[px] = (uint8_t)st;
      if (o.counts) {
        atomicAdd(&tally[st], 1u);
        if (n_valid < a.n_frames) atomicAdd(&tally[3], 1u);
      }
    }
    __syncthreads();
    if (o.counts && threadIdx.x < SUNERF_POLARIMETRY_COUNTS && tally[threadIdx.x])
      atomicAdd(o.counts + plane * SUNERF_POLARIMETRY_COUNTS + threadIdx.x, (unsigned long long)tally[threadIdx.x]);
    // (the threads that read the tally are the ones that clear it for the next chunk)
  }
}

struct DepthArgs {
  const float *tb, *pb, *rays_o, *rays_d, *solar_radius, *limb;
  int64_t n;
  double x_max_factor;
  float *depth, *z_front, *z_back, *radius, *slope;
  uint8_t* status;
};

// I_P / I_tot of one electron at the signed distance x from the closest-approach point of a line of sight with squared impact
// parameter b2
__device__ __forceinline__ double ratio_at(double x, double b2, double R, double u) {
  const double r2 = b2 + x * x;
  const ThomsonIntensity e = thomson_intensity(r2, sqrt(r2), R, u, b2);
  return e.i_p / e.i_tot;
}

__global__ __launch_bounds__(PL_THREADS) void ratio_depth_kernel(DepthArgs a) {
  const double inf = __builtin_inf();
  const float nanf_ = __builtin_nanf("");
  const double R = a.solar_radius[0], u = a.limb[0];
  for (int64_t i = (int64_t)blockIdx.x * PL_THREADS + threadIdx.x; i < a.n; i += (int64_t)gridDim.x * PL_THREADS) {
    const double tb = a.tb[i], pb = a.pb[i];
    const double ox = a.rays_o[3 * i], oy = a.rays_o[3 * i + 1], oz = a.rays_o[3 * i + 2];
    const double dx = a.rays_d[3 * i], dy = a.rays_d[3 * i + 1], dz = a.rays_d[3 * i + 2];
    const double l2 = (dx * dx + dy * dy) + dz * dz, l = sqrt(l2);
    const double z0 = -((ox * dx + oy * dy) + oz * dz) / l2;
    const double cx = oy * dz - oz * dy, cy = oz * dx - ox * dz, cz = ox * dy - oy * dx;
    const double b2 = ((cx * cx + cy * cy) + cz * cz) / l2, b = sqrt(b2);
    int st = SUNERF_POLARIMETRY_OK;
    if (!(fabs(tb) < inf) || !(fabs(pb) < inf) || !(tb > 0.0)) st = SUNERF_POLARIMETRY_INVALID;
    else if (!(l2 > 0.0) || !(l2 < inf) || !(fabs(z0) < inf) || !(b2 < inf)) st = SUNERF_POLARIMETRY_DEGENERATE;
    else if (!(b >= SUNERF_POLARIMETRY_MIN_IMPACT * R) || !(R > 0.0)) st = SUNERF_POLARIMETRY_CLOSE;
    float out_x = nanf_, out_f = nanf_, out_b = nanf_, out_r = nanf_, out_s = nanf_;
    if (st == SUNERF_POLARIMETRY_OK) {
      const double q = pb / tb, x_max = a.x_max_factor * b;
      double x;
      if (q > ratio_at(0.0, b2, R, u)) {
        st = SUNERF_POLARIMETRY_ABOVE;
        x = 0.0;
      } else if (q < ratio_at(x_max, b2, R, u)) {
        st = SUNERF_POLARIMETRY_BELOW;
        x = x_max;
      } else {
        double lo = 0.0, hi = x_max;
#pragma unroll 1
        for (int step = 0; step < SUNERF_POLARIMETRY_STEPS; ++step) {
          const double m = 0.5 * (lo + hi);
          const bool up = ratio_at(m, b2, R, u) > q;
          lo = up ? m : lo;
          hi = up ? hi : m;
        }
        x = 0.5 * (lo + hi);
      }
      const double h = b / 4096.0;
      const double f1 = ratio_at(x + h, b2, R, u);
      const bool one_sided = x < h;
      const double f0 = ratio_at(one_sided ? x : x - h, b2, R, u);
      const double slope = one_sided ? (f1 - f0) / h : (f1 - f0) / (2.0 * h);
      out_x = (float)x;
      out_f = (float)(z0 - x / l);
      out_b = (float)(z0 + x / l);
      out_r = (float)sqrt(b2 + x * x);
      out_s = (float)slope;
    }
    a.depth[i] = out_x;
    a.status[i] = (uint8_t)st;
    if (a.z_front) a.z_front[i] = out_f;
    if (a.z_back) a.z_back[i] = out_b;
    if (a.radius) a.radius[i] = out_r;
    if (a.slope) a.slope[i] = out_s;
  }
}

bool overlaps(const void* r, size_t r_bytes, const void* w, size_t w_bytes) {
  return r && w && (uintptr_t)w < (uintptr_t)r + r_bytes && (uintptr_t)r < (uintptr_t)w + w_bytes;
}

}  // namespace

extern "C" int sunerf_polarimetry_abi_version(void) { return SUNERF_POLARIMETRY_ABI_VERSION; }

extern "C" int sunerf_polarimetry_stokes(const float* frames, const uint8_t* bad, const double* cos2, const double* sin2,
                                         const double* throughput, const double* efficiency, const double* a, const double* b,
                                         int n_frames, int n_planes, int height, int width, double cy, double cx, float* stokes,
                                         float* tb, float* pb, float* pb_cross, float* chi2, float* sigma_tb, float* sigma_pb,
                                         uint8_t* status, int64_t* counts, void* stream) {
  if (n_frames > SUNERF_POLARIMETRY_MAX_FRAMES) return SUNERF_E_UNSUPPORTED;
  if (n_planes >= 0 && height >= 0 && width >= 0 && n_frames >= SUNERF_POLARIMETRY_MIN_FRAMES && (n_planes == 0 || height == 0 || width == 0))
    return 0;
  if (n_planes < 0 || height < 0 || width < 0 || n_frames < SUNERF_POLARIMETRY_MIN_FRAMES) return SUNERF_E_BADARG;
  if (!is_finite(cy) || !is_finite(cx)) return SUNERF_E_BADARG;
  if (!frames || !cos2 || !sin2 || !throughput || !efficiency || !tb || !pb) return SUNERF_E_BADARG;
  if ((a == nullptr) != (b == nullptr)) return SUNERF_E_BADARG;
  for (int k = 0; k < n_frames; ++k) {
    if (!is_finite(cos2[k]) || !is_finite(sin2[k]) || !finite_positive(throughput[k]) || !finite_positive(efficiency[k])) return SUNERF_E_BADARG;
  }
  if ((uintptr_t)a % sizeof(double) || (uintptr_t)b % sizeof(double) || (uintptr_t)counts % sizeof(int64_t)) return SUNERF_E_BADARG;
  const int64_t plane_px = (int64_t)height * width;
  const size_t px = (size_t)n_planes * plane_px, samples = px * n_frames;
  const struct { const void* p; size_t bytes; } in[2] = {{frames, samples * sizeof(float)}, {bad, samples}},
      out[8] = {{stokes, 3 * px * sizeof(float)}, {tb, px * sizeof(float)}, {pb, px * sizeof(float)}, {pb_cross, px * sizeof(float)},
                {chi2, px * sizeof(float)}, {sigma_tb, px * sizeof(float)}, {sigma_pb, px * sizeof(float)}, {status, px}};
  for (const auto& r : in)
    for (const auto& w : out)
      if (overlaps(r.p, r.bytes, w.p, w.bytes)) return SUNERF_E_BADARG;

  StokesArgs s = {};
  for (int k = 0; k < n_frames; ++k) {
    const double g0 = 0.5 * throughput[k], h = g0 * efficiency[k];
    s.g[k][0] = g0; s.g[k][1] = h * cos2[k]; s.g[k][2] = h * sin2[k];
  }
  s.cy = cy; s.cx = cx;
  s.n_frames = n_frames; s.n_planes = n_planes; s.width = width;
  s.plane_px = plane_px;
  s.chunks_per_plane = (plane_px + PL_THREADS - 1) / PL_THREADS;
  s.n_chunks = s.chunks_per_plane * n_planes;
  StokesOut o = {stokes, tb, pb, pb_cross, chi2, sigma_tb, sigma_pb, status, (unsigned long long*)counts};
  hipStream_t st = (hipStream_t)stream;
  SUNERF_CLEAR_ERROR();
  if (counts) {
    hipError_t e = hipMemsetAsync(counts, 0, (size_t)n_planes * SUNERF_POLARIMETRY_COUNTS * sizeof(int64_t), st);
    if (e != hipSuccess) return (int)e;
  }
  hipLaunchKernelGGL(stokes_kernel, dim3(grid_of(s.n_chunks)), dim3(PL_THREADS), 0, st, frames, bad, a, b, o, s);
  SUNERF_CHECK_LAUNCH();
  return 0;
}

extern "C" int sunerf_polarimetry_ratio_depth(const float* tb, const float* pb, const float* rays_o, const float* rays_d,
                                              const float* solar_radius, const float* limb_darkening_coeff, int64_t n,
                                              double x_max_factor, float* depth, float* z_front, float* z_back, float* radius,
                                              float* slope, uint8_t* status, void* stream) {
  if (n < 0) return SUNERF_E_BADARG;
  if (n == 0) return 0;
  if (!finite_positive(x_max_factor)) return SUNERF_E_BADARG;
  if (!tb || !pb || !rays_o || !rays_d || !solar_radius || !limb_darkening_coeff || !depth || !status) return SUNERF_E_BADARG;
  DepthArgs a = {tb, pb, rays_o, rays_d, solar_radius, limb_darkening_coeff, n, x_max_factor, depth, z_front, z_back, radius, slope, status};
  SUNERF_CLEAR_ERROR();
  hipLaunchKernelGGL(ratio_depth_kernel, dim3(grid_of((n + PL_THREADS - 1) / PL_THREADS)), dim3(PL_THREADS), 0, (hipStream_t)stream, a);
  SUNERF_CHECK_LAUNCH();
  return 0;
}
