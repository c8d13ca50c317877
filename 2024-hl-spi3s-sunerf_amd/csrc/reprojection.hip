// Reprojection baseline: views -> synchronic heliographic map -> views of new observers, under the
// assumption that all emission comes from the sphere r = radius.
//
// Replaces sunerf/baseline/reprojection.py: create_heliographic_map :52-95 (reproject_and_coadd with reproject_interp, mean of
// the covering views, nan_to_num with the nanmean), transform :98-125 and load_views :128-168 (reproject_to per observer).
// Conventions, formulas and argument rules: include/sunerf_hip.h.  All geometry is fp64; the only fp32 values are the taps
// read and the results stored.
//   synchronic_map_kernel   one thread per map pixel, 256 consecutive longitudes of one row per workgroup, a loop over the
//                           views; the descriptors reach LDS once per workgroup, kViewChunk at a time.  Reads of the source
//                           planes are the scattered side (as in build_ray_pool_kernel); stores run along the longitude.
//   map_fill_*_kernel       per channel: fp64 partial sums per workgroup, added in a fixed order by every workgroup of the
//                           second launch, which then replaces the NaNs of its share.
//   reproject_views_kernel  one thread per output pixel of a batch of observers; the block's descriptors are staged in LDS,
//                           the [pixel][channel] rows leave through LDS as 16-byte-per-lane stores.
// No atomics anywhere: the same inputs give the same bytes.  The only data-dependent loops are the binary searches (bounded by
// the axis length), the view loop and the walk over the observers of one block (bounded by its 256 pixels).
#include "sunerf_common.h"
#include "ordered_sum.h"
#include "reproject_math.h"
#include "../../include/sunerf_hip.h"

namespace {

constexpr int kBlock = 256;
constexpr int kViewChunk = 8;        // view descriptors staged per pass: 8 x 232 B
constexpr int kObsStage = 8;         // observer descriptors staged per workgroup: 8 x 80 B
constexpr int kFillBlocks = 128;     // workgroups (= partial sums) per channel of the fill
constexpr int kMaxC = SUNERF_OBS_MAX_CHANNELS;
constexpr double kTwoPi = 6.283185307179586476925286766559;

// one tap of a view's (downscaled) plane: the pool kernel's block mean
__device__ __forceinline__ double view_tap(const float* plane, int64_t src_w, int f, int row, int col) {
  const float* src = plane + (int64_t)row * f * src_w + (int64_t)col * f;
  if (f == 1) return (double)src[0];
  double sum = 0.;
  for (int y = 0; y < f; ++y)
    for (int x = 0; x < f; ++x) sum += (double)src[y * src_w + x];
  return (double)(float)(sum / (double)(f * f));
}

struct Bilinear {
  int y0, y1, x0, x1;
  double w00, w01, w10, w11;
  bool inside;
};

__device__ __forceinline__ Bilinear bilinear_weights(double y, double x, int ny, int nx) {
  Bilinear b;
  b.inside = y >= 0. && y <= (double)(ny - 1) && x >= 0. && x <= (double)(nx - 1);      // false for NaN coordinates
  const double fy = b.inside ? floor(y) : 0., fx = b.inside ? floor(x) : 0.;
  b.y0 = (int)fy; b.x0 = (int)fx;
  b.y1 = b.y0 + 1 < ny ? b.y0 + 1 : ny - 1;
  b.x1 = b.x0 + 1 < nx ? b.x0 + 1 : nx - 1;
  const double wy = y - fy, wx = x - fx;
  b.w00 = (1. - wy) * (1. - wx); b.w01 = (1. - wy) * wx; b.w10 = wy * (1. - wx); b.w11 = wy * wx;
  return b;
}

__device__ __forceinline__ double weighted(const Bilinear& b, double t00, double t01, double t10, double t11) {
  return ((b.w00 * t00 + b.w01 * t01) + b.w10 * t10) + b.w11 * t11;
}

// n_words 32-bit words from global memory to LDS, the whole workgroup taking part
__device__ __forceinline__ void stage_words(uint32_t* dst, const uint32_t* src, int n_words) {
  for (int i = threadIdx.x; i < n_words; i += kBlock) dst[i] = src[i];
}

// ---------------------------------------------------------------------------------------------------------------- map
struct MapArgs {
  const SunerfViewDesc* views; int n_views, C;
  const double* lat; const double* lon; int n_lon, row_begin, n_rows;
  double R;
  float* map; int32_t* footprint; double* coords;
};

__global__ __launch_bounds__(kBlock) void synchronic_map_kernel(MapArgs a) {
  __shared__ __attribute__((aligned(16))) SunerfViewDesc s_view[kViewChunk];
  const int row = blockIdx.y;                                   // row of the slab
  const int col = blockIdx.x * kBlock + threadIdx.x;
  const bool live = col < a.n_lon;
  double p[3] = {0., 0., 0.};
  if (live) {
    const double b = a.lat[a.row_begin + row], l = a.lon[col];
    const double cb = cos(b);
    p[0] = a.R * (-cb * sin(l)); p[1] = a.R * (cb * cos(l)); p[2] = a.R * (-sin(b));
  }
  double sum[kMaxC];
  int cnt[kMaxC];
#pragma unroll
  for (int c = 0; c < kMaxC; ++c) { sum[c] = 0.; cnt[c] = 0; }
  double cx = quiet_nan(), cy = quiet_nan(), cm = quiet_nan();

  for (int v0 = 0; v0 < a.n_views; v0 += kViewChunk) {
    const int nv = a.n_views - v0 < kViewChunk ? a.n_views - v0 : kViewChunk;
    __syncthreads();                                            // the previous chunk is no longer read
    stage_words(reinterpret_cast<uint32_t*>(s_view), reinterpret_cast<const uint32_t*>(a.views + v0),
                nv * (int)(sizeof(SunerfViewDesc) / 4));
    __syncthreads();
    if (!live) continue;
    for (int k = 0; k < nv; ++k) {
      const SunerfViewDesc& v = s_view[k];
      double o[3], q[3], cam[3];
#pragma unroll
      for (int r = 0; r < 3; ++r) { o[r] = (double)v.c2w[4 * r + 3]; q[r] = p[r] - o[r]; }
      const double margin = ((p[0] * o[0] + p[1] * o[1]) + p[2] * o[2]) - a.R * a.R;
      inverse_rotate(v.c2w, q, cam);
      double x = quiet_nan(), y = quiet_nan();
      const bool usable = v.per_pixel == 0 && v.height >= 1 && v.width >= 1;
      if (usable) {
        const double Tx = atan2(cam[0], hypot(cam[1], cam[2]));
        const double Ty = atan2(-cam[1], -cam[2]);
        x = axis_coord(v.tx, v.width, Tx);
        y = axis_coord(v.ty, v.height, Ty);
      }
      if (a.coords) { cx = x; cy = y; cm = margin; }
      if (!(margin > 0.) || !usable) continue;
      const Bilinear b = bilinear_weights(y, x, v.height, v.width);
      if (!b.inside) continue;
      const int f = v.downscale;
      const int64_t src_w = (int64_t)v.width * f, plane_size = (int64_t)v.height * f * src_w;
#pragma unroll
      for (int c = 0; c < kMaxC; ++c) {
        if (c >= a.C) continue;
        const int pl = v.plane[c];
        if (pl < 0 || pl >= v.n_planes) continue;
        const float* plane = v.image + pl * plane_size;
        const double s = weighted(b, view_tap(plane, src_w, f, b.y0, b.x0), view_tap(plane, src_w, f, b.y0, b.x1),
                                  view_tap(plane, src_w, f, b.y1, b.x0), view_tap(plane, src_w, f, b.y1, b.x1));
        if (s == s) { sum[c] += s; cnt[c] += 1; }
      }
    }
  }
  if (!live) return;
  const int64_t slab = (int64_t)a.n_rows * a.n_lon, at = (int64_t)row * a.n_lon + col;
#pragma unroll
  for (int c = 0; c < kMaxC; ++c) {
    if (c >= a.C) continue;
    a.map[c * slab + at] = cnt[c] > 0 ? (float)(sum[c] / (double)cnt[c]) : __int_as_float(0x7fc00000);
    a.footprint[c * slab + at] = cnt[c];
  }
  if (a.coords) {
    a.coords[at] = cx; a.coords[slab + at] = cy; a.coords[2 * slab + at] = cm;
  }
}

// --------------------------------------------------------------------------------------------------------------- fill
struct FillArgs {
  float* map; int64_t n_pixels; int mode; double value;
  double* stats; double* partial;       // partial [C][kFillBlocks][2]
};

// sum over the workgroup of (s, n) by ordered_sum.h's halving tree: the result in red[0] / red[kBlock] for every thread.  Each
// kernel runs it once on an array of its own: no barrier of the caller's.
__device__ __forceinline__ void tree_sum2(double* red, double s, double n) {
  const double v[2] = {s, n};
  lds_tree<kBlock>(red, v, add_values());
}

__global__ __launch_bounds__(kBlock) void map_fill_partial_kernel(FillArgs a) {
  __shared__ double red[2 * kBlock];
  const int c = blockIdx.y;
  const float* m = a.map + (int64_t)c * a.n_pixels;
  double s = 0., n = 0.;
  for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < a.n_pixels; i += (int64_t)kFillBlocks * kBlock) {
    const float v = m[i];
    if (v == v) { s += (double)v; n += 1.; }
  }
  tree_sum2(red, s, n);
  if (threadIdx.x == 0) {
    double* out = a.partial + ((int64_t)c * kFillBlocks + blockIdx.x) * 2;
    out[0] = red[0]; out[1] = red[kBlock];
  }
}

__global__ __launch_bounds__(kBlock) void map_fill_finish_kernel(FillArgs a) {
  __shared__ double red[2 * kBlock];
  const int c = blockIdx.y, t = threadIdx.x;
  const double* part = a.partial + (int64_t)c * kFillBlocks * 2;
  tree_sum2(red, t < kFillBlocks ? part[2 * t] : 0., t < kFillBlocks ? part[2 * t + 1] : 0.);
  const double count = red[kBlock];
  const double mean = count > 0. ? red[0] / count : quiet_nan();
  if (blockIdx.x == 0 && t == 0) { a.stats[2 * c] = mean; a.stats[2 * c + 1] = count; }
  if (a.mode == 0) return;
  const float fill = (float)(a.mode == 1 ? mean : a.value);
  float* m = a.map + (int64_t)c * a.n_pixels;
  for (int64_t i = (int64_t)blockIdx.x * kBlock + t; i < a.n_pixels; i += (int64_t)kFillBlocks * kBlock) {
    const float v = m[i];
    if (v != v) m[i] = fill;
  }
}

// ---------------------------------------------------------------------------------------------------------- reproject
struct ViewsArgs {
  const float* map; int C;
  const double* lat; int n_lat; const double* lon; int n_lon;
  double R;
  const SunerfObserverDesc* obs; int n_obs; int64_t n_pixels;
  float off_disk; float* out; double* coords;
};

__global__ __launch_bounds__(kBlock) void reproject_views_kernel(ViewsArgs a) {
  __shared__ __attribute__((aligned(16))) float s_out[kBlock * kMaxC];      // [256][C]
  __shared__ __attribute__((aligned(16))) SunerfObserverDesc s_obs[kObsStage];
  __shared__ int s_first;
  const int t = threadIdx.x, C = a.C;
  const int64_t first = (int64_t)blockIdx.x * kBlock;
  const int64_t i = first + t;
  if (t == 0) {                                   // last observer whose first pixel is <= the block's first pixel
    int lo = 0, hi = a.n_obs - 1;
    while (lo < hi) {
      const int mid = (lo + hi + 1) >> 1;
      if (a.obs[mid].pix_offset <= first) lo = mid; else hi = mid - 1;
    }
    s_first = lo;
  }
  __syncthreads();
  const int k0 = s_first;
  const int staged = a.n_obs - k0 < kObsStage ? a.n_obs - k0 : kObsStage;
  stage_words(reinterpret_cast<uint32_t*>(s_obs), reinterpret_cast<const uint32_t*>(a.obs + k0),
              staged * (int)(sizeof(SunerfObserverDesc) / 4));
  __syncthreads();
  if (i < a.n_pixels) {
    int k = k0;                                   // the pixel's observer: a walk of at most this block's 256 pixels
    while (k + 1 < a.n_obs && (k + 1 - k0 < staged ? s_obs[k + 1 - k0].pix_offset : a.obs[k + 1].pix_offset) <= i) ++k;
    const SunerfObserverDesc& ob = k - k0 < staged ? s_obs[k - k0] : a.obs[k];
    const int64_t local = i - ob.pix_offset;
    double x = quiet_nan(), y = quiet_nan(), mrel = quiet_nan();
    bool on_disk = false;
    if (local >= 0 && local < (int64_t)ob.height * ob.width) {
      const int row = (int)(local / ob.width), col = (int)(local - (int64_t)row * ob.width);
      const double Tx = ob.tx[col], Ty = ob.ty[row];
      const double sx = sin(Tx), cx = cos(Tx), sy = sin(Ty), cy = cos(Ty);
      const double dc[3] = {sx, -sy * cx, -cx * cy};
      double o[3], d[3];
#pragma unroll
      for (int r = 0; r < 3; ++r) {
        d[r] = ((double)ob.c2w[4 * r] * dc[0] + (double)ob.c2w[4 * r + 1] * dc[1]) + (double)ob.c2w[4 * r + 2] * dc[2];
        o[r] = (double)ob.c2w[4 * r + 3];
      }
      const double c0 = o[1] * d[2] - o[2] * d[1], c1 = o[2] * d[0] - o[0] * d[2], c2 = o[0] * d[1] - o[1] * d[0];
      const double R2 = a.R * a.R;
      const double m = R2 - ((c0 * c0 + c1 * c1) + c2 * c2);
      const double od = (o[0] * d[0] + o[1] * d[1]) + o[2] * d[2];
      mrel = m / R2;
      on_disk = m > 0. && od < 0.;
      if (on_disk) {
        const double s = -od - sqrt(m);
        const double px = o[0] + d[0] * s, py = o[1] + d[1] * s, pz = o[2] + d[2] * s;
        const double lat = atan2(-pz, hypot(px, py));
        double lon = atan2(-px, py);
        const double lon0 = a.lon[0];
        lon -= kTwoPi * floor((lon - lon0) / kTwoPi);
        if (lon < lon0) lon += kTwoPi;
        if (lon >= lon0 + kTwoPi) lon -= kTwoPi;
        x = axis_coord(a.lon, a.n_lon, lon);
        y = axis_coord(a.lat, a.n_lat, lat);
      }
    }
    if (a.coords) { a.coords[i] = x; a.coords[a.n_pixels + i] = y; a.coords[2 * a.n_pixels + i] = mrel; }
    const Bilinear b = bilinear_weights(y, x, a.n_lat, a.n_lon);
    const int64_t plane_size = (int64_t)a.n_lat * a.n_lon;
    for (int c = 0; c < C; ++c) {
      float value = on_disk ? __int_as_float(0x7fc00000) : a.off_disk;
      if (on_disk && b.inside) {
        const float* m = a.map + c * plane_size;
        value = (float)weighted(b, (double)m[(int64_t)b.y0 * a.n_lon + b.x0], (double)m[(int64_t)b.y0 * a.n_lon + b.x1],
                                (double)m[(int64_t)b.y1 * a.n_lon + b.x0], (double)m[(int64_t)b.y1 * a.n_lon + b.x1]);
      }
      s_out[t * C + c] = value;
    }
  }
  __syncthreads();
  const int64_t left = a.n_pixels - first;
  const int n = (left < kBlock ? (int)left : kBlock) * C;        // floats of this block
  float* dst = a.out + first * C;
  for (int v = t * 4; v < n; v += kBlock * 4) {
    if (v + 4 <= n) {
      *reinterpret_cast<f32x4*>(dst + v) = *reinterpret_cast<const f32x4*>(s_out + v);
    } else {
      for (int e = v; e < n; ++e) dst[e] = s_out[e];
    }
  }
}

}  // namespace

extern "C" size_t sunerf_observer_desc_bytes(void) { return sizeof(SunerfObserverDesc); }

extern "C" int sunerf_synchronic_map(const SunerfViewDesc* views, int n_views, int n_channels, const double* lat, int n_lat,
                                     const double* lon, int n_lon, int row_begin, int n_rows, double radius, float* map,
                                     int32_t* footprint, double* coords, void* stream) {
  if (!views || !lat || !lon || n_views < 1 || n_lat < 1 || n_lon < 1) return SUNERF_E_BADARG;
  if (n_channels < 1 || n_channels > SUNERF_OBS_MAX_CHANNELS || !finite_positive(radius)) return SUNERF_E_BADARG;
  if (row_begin < 0 || n_rows < 0 || row_begin > n_lat || n_rows > n_lat - row_begin) return SUNERF_E_BADARG;
  if (coords && n_views != 1) return SUNERF_E_BADARG;
  if (n_rows == 0) return 0;
  if (!map || !footprint || n_rows > 65535) return SUNERF_E_BADARG;      // grid y: callers tile taller slabs
  MapArgs a;
  a.views = views; a.n_views = n_views; a.C = n_channels; a.lat = lat; a.lon = lon; a.n_lon = n_lon;
  a.row_begin = row_begin; a.n_rows = n_rows; a.R = radius; a.map = map; a.footprint = footprint; a.coords = coords;
  SUNERF_CLEAR_ERROR();
  hipLaunchKernelGGL(synchronic_map_kernel, dim3((unsigned)((n_lon + kBlock - 1) / kBlock), (unsigned)n_rows), dim3(kBlock), 0,
                     (hipStream_t)stream, a);
  SUNERF_CHECK_LAUNCH();
  return 0;
}

extern "C" size_t sunerf_map_fill_workspace_bytes(int n_channels) {
  if (n_channels < 1 || n_channels > SUNERF_OBS_MAX_CHANNELS) return 0;
  return (size_t)n_channels * kFillBlocks * 2 * sizeof(double);
}

extern "C" int sunerf_map_fill(float* map, int n_channels, int64_t n_pixels, int mode, double value, double* stats,
                               void* workspace, size_t workspace_bytes, void* stream) {
  if (!map || !stats || !workspace || n_pixels < 1 || mode < 0 || mode > 2) return SUNERF_E_BADARG;
  if (n_channels < 1 || n_channels > SUNERF_OBS_MAX_CHANNELS) return SUNERF_E_BADARG;
  if ((uintptr_t)stats % sizeof(double) || (uintptr_t)workspace % sizeof(double)) return SUNERF_E_BADARG;
  if (workspace_bytes < sunerf_map_fill_workspace_bytes(n_channels)) return SUNERF_E_WORKSPACE;
  FillArgs a;
  a.map = map; a.n_pixels = n_pixels; a.mode = mode; a.value = value; a.stats = stats; a.partial = (double*)workspace;
  hipStream_t st = (hipStream_t)stream;
  SUNERF_CLEAR_ERROR();
  hipLaunchKernelGGL(map_fill_partial_kernel, dim3(kFillBlocks, (unsigned)n_channels), dim3(kBlock), 0, st, a);
  SUNERF_CHECK_LAUNCH();
  hipLaunchKernelGGL(map_fill_finish_kernel, dim3(kFillBlocks, (unsigned)n_channels), dim3(kBlock), 0, st, a);
  SUNERF_CHECK_LAUNCH();
  return 0;
}

extern "C" int sunerf_reproject_views(const float* map, int n_channels, const double* lat, int n_lat, const double* lon,
                                      int n_lon, double radius, const SunerfObserverDesc* observers, int n_observers,
                                      int64_t n_pixels, float off_disk, float* out, double* coords, void* stream) {
  if (!map || !lat || !lon || !observers || n_lat < 1 || n_lon < 1 || n_observers < 1 || n_pixels < 1) return SUNERF_E_BADARG;
  if (n_channels < 1 || n_channels > SUNERF_OBS_MAX_CHANNELS || !finite_positive(radius)) return SUNERF_E_BADARG;
  if (!out || ((uintptr_t)out & 15u) || (n_pixels + kBlock - 1) / kBlock > 0x7fffffff) return SUNERF_E_BADARG;
  ViewsArgs a;
  a.map = map; a.C = n_channels; a.lat = lat; a.n_lat = n_lat; a.lon = lon; a.n_lon = n_lon; a.R = radius;
  a.obs = observers; a.n_obs = n_observers; a.n_pixels = n_pixels; a.off_disk = off_disk; a.out = out; a.coords = coords;
  SUNERF_CLEAR_ERROR();
  hipLaunchKernelGGL(reproject_views_kernel, dim3((unsigned)((n_pixels + kBlock - 1) / kBlock)), dim3(kBlock), 0,
                     (hipStream_t)stream, a);
  SUNERF_CHECK_LAUNCH();
  return 0;
}
