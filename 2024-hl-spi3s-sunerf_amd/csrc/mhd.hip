// MHD simulation cube as the field behind the density / temperature integral (include/sunerf_hip.h: sunerf_mhd_field*).
//
// Replaces MHDModel.forward, sunerf/model/mhd_model.py:76-142: per unique time the reference re-reads two HDF5 files per
// frame and builds a scipy RegularGridInterpolator per variable on the CPU (:45-75, :114-138).  Here the frames a batch
// needs are resident on the device (sunerf/model/mhd_model.py uploads them) and every point finds its frame pair itself.
//
// Layout: a frame is one float2 (rho, T) per node in [i_phi][i_theta][i_r] order (r fastest), so one trilinear
// interpolation is 8 gathers of 8 bytes (corners (i_r, i_r + 1) adjacent) and rho and T come from the same lines.
// A sample's cell is found per axis by a uniform bucket table (host-built: the cell of each bucket's lower edge) plus a
// short walk to the cell numpy.searchsorted(grid, x) - 1 (clipped to [0, n - 2]) gives, as scipy does; PSI's r grid is
// strongly clustered near 1 solar radius, which is what the table absorbs.  The walk is bounded by the nodes per bucket.
//
// Launch: one lane per sample, the samples of a ray in neighbouring lanes (index = ray * S + sample), so that the gathers
// of a wave walk through neighbouring cells of one ray and share cache lines.
#include <hip/hip_runtime.h>
#include <math.h>

#include "sunerf_common.h"
#include "../../include/sunerf_hip.h"

namespace {

constexpr int MHD_THREADS = 256;
constexpr float MHD_FILL = 1e-10f;          // fill_value of mhd_model.py:45 / :108 and the clamp of data < 0 (:64)

struct MhdArgs {
  const float* rays_o; const float* rays_d; const float* z_vals; const float* times;   // rays mode
  const float* points;                                                                  // points mode: [M,4]
  int64_t n; int S;                                                                     // rays x samples, or points x 1
  const SunerfMhdFrame* frames; const int* slot; int ffirst, flast;
  float* raw; int* status;
};

// cell i of `x` on axis k: g[i] < x <= g[i + 1], clipped to [0, n - 2] (searchsorted(grid, x, 'left') - 1)
__device__ __forceinline__ int find_cell(const SunerfMhdFrame& fr, int k, float x) {
  const float* g = fr.axis[k];
  const int last = fr.n[k] - 2;
  int b = (int)((x - fr.lo[k]) * fr.inv_width[k]);      // x is inside [lo, hi] here: b >= 0 up to rounding
  b = b < 0 ? 0 : (b >= fr.nb[k] ? fr.nb[k] - 1 : b);
  int i = fr.bucket[k][b];
  while (i < last && g[i + 1] < x) ++i;
  while (i > 0 && g[i] >= x) --i;                         // the bucket index may round one bucket high
  return i;
}

// (rho, T) of one frame at (phi, theta, r): RegularGridInterpolator(method='linear', bounds_error=False, fill_value=1e-10)
__device__ __forceinline__ float2 frame_value(const SunerfMhdFrame& fr, float phi, float th, float r) {
  const float c[3] = {phi, th, r};
  if (!(c[0] >= fr.lo[0] && c[0] <= fr.hi[0] && c[1] >= fr.lo[1] && c[1] <= fr.hi[1] && c[2] >= fr.lo[2] && c[2] <= fr.hi[2]))
    return make_float2(MHD_FILL, MHD_FILL);               // (NaN coordinates are handled by the caller)
  int i[3];
  float w[3];
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    i[k] = find_cell(fr, k, c[k]);
    const float g0 = fr.axis[k][i[k]], g1 = fr.axis[k][i[k] + 1];
    w[k] = (c[k] - g0) / (g1 - g0);
  }
  const int nt = fr.n[1], nr = fr.n[2];
  const float2* d = reinterpret_cast<const float2*>(fr.data);
  const int64_t b00 = ((int64_t)i[0] * nt + i[1]) * nr + i[2];   // (phi, theta)
  const int64_t b01 = b00 + nr;                                   // (phi, theta + 1)
  const int64_t b10 = b00 + (int64_t)nt * nr;                     // (phi + 1, theta)
  const int64_t b11 = b10 + nr;
  const float2 v000 = d[b00], v001 = d[b00 + 1], v010 = d[b01], v011 = d[b01 + 1];
  const float2 v100 = d[b10], v101 = d[b10 + 1], v110 = d[b11], v111 = d[b11 + 1];
  const float ur = 1.f - w[2], ut = 1.f - w[1], up = 1.f - w[0];
  float2 out;
  {
    const float a00 = ur * v000.x + w[2] * v001.x, a01 = ur * v010.x + w[2] * v011.x;
    const float a10 = ur * v100.x + w[2] * v101.x, a11 = ur * v110.x + w[2] * v111.x;
    out.x = up * (ut * a00 + w[1] * a01) + w[0] * (ut * a10 + w[1] * a11);
  }
  {
    const float a00 = ur * v000.y + w[2] * v001.y, a01 = ur * v010.y + w[2] * v011.y;
    const float a10 = ur * v100.y + w[2] * v101.y, a11 = ur * v110.y + w[2] * v111.y;
    out.y = up * (ut * a00 + w[1] * a01) + w[0] * (ut * a10 + w[1] * a11);
  }
  return out;
}

// slot of frame f, or -1 (not resident / outside [ffirst, flast])
__device__ __forceinline__ int frame_slot(const MhdArgs& a, float f) {
  if (!(f >= (float)a.ffirst && f <= (float)a.flast)) return -1;
  return a.slot[(int)f - a.ffirst];
}

template <bool RAYS>
__global__ __launch_bounds__(MHD_THREADS) void mhd_field_kernel(MhdArgs a) {
  const int64_t idx = (int64_t)blockIdx.x * MHD_THREADS + threadIdx.x;
  if (idx >= a.n * a.S) return;
  float x, y, z, t;
  if (RAYS) {
    const int64_t ray = idx / a.S;
    const float zz = a.z_vals[idx];
    x = a.rays_o[ray * 3 + 0] + a.rays_d[ray * 3 + 0] * zz;       // sampling.py:100, never written to memory
    y = a.rays_o[ray * 3 + 1] + a.rays_d[ray * 3 + 1] * zz;
    z = a.rays_o[ray * 3 + 2] + a.rays_d[ray * 3 + 2] * zz;
    t = a.times[ray];
  } else {
    const float4 p = reinterpret_cast<const float4*>(a.points)[idx];
    x = p.x; y = p.y; z = p.z; t = p.w;
  }
  // mhd_model.py:100-103 (the product and sum roundings of torch's x**2 + y**2 + z**2; -ffp-contract=off)
  const float r = sqrtf((x * x + y * y) + z * z);
  const float th = acosf(z / r);
  float phi = atan2f(y, x);
  if (phi < 0.f) phi += 6.283185307179586f;
  // mhd_model.py:121-124: f = t (flast - ffirst) + ffirst, w = f - int(f), floor / ceil
  const float f = t * (float)(a.flast - a.ffirst) + (float)a.ffirst;
  const float w = f - truncf(f);
  const int s1 = frame_slot(a, floorf(f)), s2 = frame_slot(a, ceilf(f));
  float2 out;
  if (!(t == t)) {
    out = make_float2(__int_as_float(0x7fc00000), __int_as_float(0x7fc00000));
  } else if (s1 < 0 || s2 < 0) {
    out = make_float2(__int_as_float(0x7fc00000), __int_as_float(0x7fc00000));
    *a.status = 1;                                                  // defensive: the host makes the frames resident first
  } else if (!(r == r && th == th && phi == phi)) {
    out = make_float2(__int_as_float(0x7fc00000), __int_as_float(0x7fc00000));   // scipy: NaN coordinate -> NaN
  } else {
    const float2 v1 = frame_value(a.frames[s1], phi, th, r);
    const float2 v2 = frame_value(a.frames[s2], phi, th, r);
    // mhd_model.py:137-138: the blend and the product in fp32; the logarithms in fp64, rounded once, so that they are the
    // correctly rounded fp32 values (device logf is within 1 ulp, and the fill ln(1e-10) = -23.02585 then misses by 1.9e-6)
    const float u = 1.f - w;
    out.x = (float)log((double)(u * v1.x + w * v2.x));
    out.y = (float)log10((double)(1e6f * (u * v1.y + w * v2.y)));
  }
  reinterpret_cast<float2*>(a.raw)[idx] = out;
}

int launch(const MhdArgs& a, void* stream) {
  const int64_t total = a.n * a.S;
  SUNERF_CLEAR_ERROR();
  if (a.points)
    hipLaunchKernelGGL(mhd_field_kernel<false>, dim3((unsigned)((total + MHD_THREADS - 1) / MHD_THREADS)), dim3(MHD_THREADS), 0,
                       (hipStream_t)stream, a);
  else
    hipLaunchKernelGGL(mhd_field_kernel<true>, dim3((unsigned)((total + MHD_THREADS - 1) / MHD_THREADS)), dim3(MHD_THREADS), 0,
                       (hipStream_t)stream, a);
  SUNERF_CHECK_LAUNCH();
  return 0;
}

}  // namespace

extern "C" size_t sunerf_mhd_frame_bytes(void) { return sizeof(SunerfMhdFrame); }

extern "C" int sunerf_mhd_field(const float* rays_o, const float* rays_d, const float* z_vals, const float* times, int64_t n_rays,
                                int n_samples, const SunerfMhdFrame* frames, const int* slot, int ffirst, int flast, float* raw,
                                int* status, void* stream) {
  if (n_rays < 0 || n_samples < 1 || flast < ffirst) return SUNERF_E_BADARG;
  if (n_rays == 0) return 0;
  if (!rays_o || !rays_d || !z_vals || !times || !frames || !slot || !raw || !status) return SUNERF_E_BADARG;
  if ((n_rays * n_samples + MHD_THREADS - 1) / MHD_THREADS > 0x7fffffff) return SUNERF_E_UNSUPPORTED;
  MhdArgs a = {};
  a.rays_o = rays_o; a.rays_d = rays_d; a.z_vals = z_vals; a.times = times; a.n = n_rays; a.S = n_samples;
  a.frames = frames; a.slot = slot; a.ffirst = ffirst; a.flast = flast; a.raw = raw; a.status = status;
  return launch(a, stream);
}

extern "C" int sunerf_mhd_field_points(const float* points, int64_t n_points, const SunerfMhdFrame* frames, const int* slot,
                                       int ffirst, int flast, float* raw, int* status, void* stream) {
  if (n_points < 0 || flast < ffirst) return SUNERF_E_BADARG;
  if (n_points == 0) return 0;
  if (!points || !frames || !slot || !raw || !status) return SUNERF_E_BADARG;
  if ((n_points + MHD_THREADS - 1) / MHD_THREADS > 0x7fffffff) return SUNERF_E_UNSUPPORTED;
  MhdArgs a = {};
  a.points = points; a.n = n_points; a.S = 1;
  a.frames = frames; a.slot = slot; a.ffirst = ffirst; a.flast = flast; a.raw = raw; a.status = status;
  return launch(a, stream);
}
