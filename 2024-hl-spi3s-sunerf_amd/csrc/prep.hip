// A detector image becomes a view: spline prefilter, affine resample with the scaling / norm / clip epilogue, exact order
// statistics for the percentile clip (include/sunerf_hip_prep.h).
//
// Replaces the host-side arithmetic of the reference's loaders (sunerf/data/prep/{sdo,stereo,so,psi}.py, sunerf/data/utils.py:
// loadMapStack): Map.rotate(recenter, scale, missing, order), the crop, the exposure scaling, the linear norm, the clips.  The
// semantics are scipy.ndimage.affine_transform(mode='constant', prefilter=True) of scipy 1.15, restated in fp64 (prep_math.h).
//
// 1. Prefilter.  A line is cut into segments of PREP_SEGMENT samples.  The poles are small (|z| <= 0.431), so a segment's causal
//    recursion may start a horizon early on the mirrored line with state 0, and its anticausal recursion the same horizon late:
//    what is left of the wrong start is below 1e-17 of the line's maximum when the first kept sample is reached.  That gives
//    lines x segments independent threads instead of one thread per line.  A workgroup takes a tile of PREP_LINES lines x one
//    segment: all 256 threads stage segment + 2 halo samples of every line in LDS as fp64 (already multiplied by the gain;
//    coalesced along x in both passes), wave 0 filters one line per lane in place (LDS image [position][line]: the lanes of a
//    step touch consecutive doubles), all threads write the kept samples back.  Pass 1 runs along x from the fp32 image into
//    the workspace, pass 2 along y from the workspace into the coefficients.
// 2. Resample.  One thread per output pixel: fp64 source coordinate, (order+1)^2 taps, epilogue, one rounding to fp32.
// 3. Order statistics.  Radix select, 8 bits per pass: per pass one launch histograms the digit of every value that still
//    matches a rank's prefix (integer LDS atomics, one histogram per workgroup and rank written to the workspace) and one launch
//    adds the workgroups' histograms in a fixed order and extends the prefix.
// No floating-point atomics; nothing depends on the launch geometry, which is a function of one plane's shape alone.
#include "sunerf_common.h"
#include "prep_math.h"
#include "../../include/sunerf_hip_prep.h"

static_assert(PREP_SEGMENT == SUNERF_PREP_SEGMENT && PREP_MAX_ORDER == SUNERF_PREP_MAX_ORDER, "header and kernels disagree");

namespace {

constexpr int PF_THREADS = 256;
constexpr int PF_LS = PREP_LINES + 1;          // doubles between two positions of the LDS image

struct PrefilterArgs {
  const float* image;        // pass along x: [C][H][W] fp32
  const double* src;         // pass along y: [C][H][W] fp64
  double* dst;
  uint8_t* mask;             // pass along x only; may be null
  int n_planes, height, width;
  int n_poles, halo;         // 0 poles: the line is copied
  double z0, z1, gain;
  int n_groups, n_segments;  // tiles of a plane: groups of PREP_LINES lines x segments of a line
};

template <bool ALONG_X>
__global__ __launch_bounds__(PF_THREADS) void prep_prefilter_kernel(PrefilterArgs a) {
  extern __shared__ __attribute__((aligned(16))) double tile[];      // [len][PF_LS]
  const int t = threadIdx.x;
  const int n_lines = ALONG_X ? a.height : a.width;        // lines of a plane
  const int n = ALONG_X ? a.width : a.height;              // samples of a line
  const int len = PREP_SEGMENT + 2 * a.halo;
  const int64_t plane_px = (int64_t)a.height * a.width;
  const int64_t tiles_per_plane = (int64_t)a.n_groups * a.n_segments;
  const int64_t n_tiles = tiles_per_plane * a.n_planes;
  for (int64_t tile_id = blockIdx.x; tile_id < n_tiles; tile_id += gridDim.x) {
    const int64_t plane = tile_id / tiles_per_plane;
    const int in_plane = (int)(tile_id - plane * tiles_per_plane);
    const int line0 = (in_plane / a.n_segments) * PREP_LINES;
    const int first = (in_plane % a.n_segments) * PREP_SEGMENT;       // first kept sample
    const int64_t base = plane * plane_px;

    for (int i = t; i < PREP_LINES * len; i += PF_THREADS) {
      int line, pos;
      if (ALONG_X) { line = i / len; pos = i - line * len; } else { pos = i / PREP_LINES; line = i - pos * PREP_LINES; }
      double v = 0.0;
      if (line0 + line < n_lines) {
        const int s = prep_mirror((int64_t)first - a.halo + pos, n);
        if (ALONG_X) {
          const float f = a.image[base + (int64_t)(line0 + line) * a.width + s];
          const bool finite = fabsf(f) <= 3.4028234663852886e38f;      // false for NaN and +-inf
          v = finite ? (double)f : 0.0;
          const int kept = first + pos - a.halo;
          if (a.mask && pos >= a.halo && pos < a.halo + PREP_SEGMENT && kept < n)
            a.mask[base + (int64_t)(line0 + line) * a.width + kept] = finite ? 0 : 1;
        } else {
          v = a.src[base + (int64_t)s * a.width + line0 + line];
        }
        v *= a.gain;
      }
      tile[pos * PF_LS + line] = v;
    }
    __syncthreads();
    if (t < PREP_LINES && a.n_poles > 0) prep_filter_line(tile + t, PF_LS, len, a.n_poles, a.z0, a.z1);
    __syncthreads();
    for (int i = t; i < PREP_LINES * PREP_SEGMENT; i += PF_THREADS) {
      int line, p;
      if (ALONG_X) { line = i / PREP_SEGMENT; p = i - line * PREP_SEGMENT; } else { p = i / PREP_LINES; line = i - p * PREP_LINES; }
      if (line0 + line < n_lines && first + p < n) {
        const int64_t g = ALONG_X ? (int64_t)(line0 + line) * a.width + first + p : (int64_t)(first + p) * a.width + line0 + line;
        a.dst[base + g] = tile[(a.halo + p) * PF_LS + line];
      }
    }
    __syncthreads();                                 // the tile is overwritten by the next one
  }
}

// ---- resample -------------------------------------------------------------------------------------------------------------------
constexpr int RS_THREADS = 256;

struct ResampleArgs {
  const double* coef;
  const uint8_t* mask;
  int n_planes, height, width, out_height, out_width;
  double m_yy, m_yx, m_xy, m_xx, off_y, off_x, missing;
  const double* params;
  int flags;
  float* out;
};

template <int ORDER>
__global__ __launch_bounds__(RS_THREADS) void prep_resample_kernel(ResampleArgs a) {
  const int64_t out_px = (int64_t)a.out_height * a.out_width;
  const int64_t total = out_px * a.n_planes;
  const int64_t in_px = (int64_t)a.height * a.width;
  for (int64_t i = (int64_t)blockIdx.x * RS_THREADS + threadIdx.x; i < total; i += (int64_t)gridDim.x * RS_THREADS) {
    const int64_t plane = i / out_px;
    const int64_t q = i - plane * out_px;
    const int r = (int)(q / a.out_width), c = (int)(q - (int64_t)r * a.out_width);
    const double cy = (a.off_y + a.m_yy * (double)r) + a.m_yx * (double)c;
    const double cx = (a.off_x + a.m_xy * (double)r) + a.m_xx * (double)c;
    bool outside, hit;
    const uint8_t* mask = (a.flags & SUNERF_PREP_PROPAGATE) ? a.mask + plane * in_px : nullptr;
    double v = prep_sample<ORDER>(a.coef + plane * in_px, mask, a.height, a.width, cy, cx, &outside, &hit);
    if (outside) v = a.missing;
    const double* p = a.params + plane * SUNERF_PREP_PARAMS;
    if (a.flags & SUNERF_PREP_CLIP_RANGE) v = v < p[0] ? p[0] : (v > p[1] ? p[1] : v);
    v = v * p[2];
    if (a.flags & SUNERF_PREP_NORM) {
      v = (v - p[3]) / (p[4] - p[3]);
      if (a.flags & SUNERF_PREP_NORM_CLIP) v = v < 0.0 ? 0.0 : (v > 1.0 ? 1.0 : v);
    }
    if ((a.flags & SUNERF_PREP_CLIP_NEGATIVE) && v < 0.0) v = 0.0;
    float f = (float)v;
    if (!(fabsf(f) <= 3.4028234663852886e38f)) f = 0.f;
    if (hit) f = __uint_as_float(0x7fc00000u);
    a.out[i] = f;
  }
}

// ---- order statistics -----------------------------------------------------------------------------------------------------------
constexpr int OS_THREADS = 256;
constexpr int OS_CHUNK = 4096;            // values per workgroup at least
constexpr int OS_MAX_GROUPS = 128;        // workgroups per plane at most

struct OsState {                          // per (plane, rank), 16 bytes
  uint32_t prefix;                        // the digits found so far, in place
  uint32_t ok;                            // the rank lies inside [0, n_valid)
  int64_t remaining;                      // rank among the values that match the prefix
};

struct OsArgs {
  const float* x;
  int n_planes, n_ranks, n_groups;
  int64_t n_values;
  const int64_t* ranks;
  float* values;
  int64_t* nan_count;
  OsState* state;                         // [n_planes][n_ranks]
  uint32_t* hist;                         // [n_planes][n_groups][n_ranks][256]
  uint32_t* nans;                         // [n_planes][n_groups]
  int pass;                               // 0 .. 3, most significant digit first
};

int os_groups(int64_t n_values) {
  const int64_t g = (n_values + OS_CHUNK - 1) / OS_CHUNK;
  return (int)(g < 1 ? 1 : (g > OS_MAX_GROUPS ? OS_MAX_GROUPS : g));
}

// one workgroup per (plane, group): the digit histogram of the group's share of the plane, per rank.  Pass 0 has one prefix
// (none) for all ranks: only rank 0's histogram is formed, and read for every rank.
__global__ __launch_bounds__(OS_THREADS) void prep_os_histogram_kernel(OsArgs a) {
  __shared__ uint32_t hist[SUNERF_PREP_MAX_RANKS][256];
  __shared__ uint32_t nan_total;
  __shared__ uint32_t prefix[SUNERF_PREP_MAX_RANKS];
  __shared__ uint32_t live[SUNERF_PREP_MAX_RANKS];
  const int t = threadIdx.x;
  const int shift = 24 - 8 * a.pass;
  const int n_hist = a.pass == 0 ? 1 : a.n_ranks;
  const int64_t n_work = (int64_t)a.n_planes * a.n_groups;
  const int64_t share = (a.n_values + a.n_groups - 1) / a.n_groups;
  for (int64_t w = blockIdx.x; w < n_work; w += gridDim.x) {
    const int64_t plane = w / a.n_groups;
    const int group = (int)(w - plane * a.n_groups);
    for (int r = 0; r < n_hist; ++r) hist[r][t] = 0;
    if (t == 0) nan_total = 0;
    if (t < n_hist) {
      const OsState s = a.pass == 0 ? OsState{0u, 1u, 0} : a.state[plane * a.n_ranks + t];
      prefix[t] = s.prefix;
      live[t] = s.ok;
    }
    __syncthreads();
    const int64_t begin = group * share;
    const int64_t end = begin + share < a.n_values ? begin + share : a.n_values;
    const float* x = a.x + plane * a.n_values;
    uint32_t my_nans = 0;
    for (int64_t i = begin + t; i < end; i += OS_THREADS) {
      const uint32_t bits = __float_as_uint(x[i]);
      if (prep_is_nan_bits(bits)) {
        ++my_nans;
        continue;
      }
      const uint32_t key = prep_key(bits);
      const uint32_t digit = (key >> shift) & 255u;
      if (a.pass == 0) {
        atomicAdd(&hist[0][digit], 1u);
      } else {
        const uint32_t head = key >> (shift + 8);
        for (int r = 0; r < n_hist; ++r)
          if (live[r] && head == (prefix[r] >> (shift + 8))) atomicAdd(&hist[r][digit], 1u);
      }
    }
    if (a.pass == 0 && my_nans) atomicAdd(&nan_total, my_nans);
    __syncthreads();
    uint32_t* out = a.hist + (plane * a.n_groups + group) * (int64_t)a.n_ranks * 256;
    for (int r = 0; r < n_hist; ++r) out[r * 256 + t] = hist[r][t];
    if (a.pass == 0 && t == 0) a.nans[plane * a.n_groups + group] = nan_total;
    __syncthreads();
  }
}

// one workgroup per (plane, rank): adds the groups' histograms (group 0 first), finds the digit that holds the rank
__global__ __launch_bounds__(OS_THREADS) void prep_os_select_kernel(OsArgs a) {
  __shared__ unsigned long long count[256];
  const int t = threadIdx.x;
  const int shift = 24 - 8 * a.pass;
  const int64_t n_work = (int64_t)a.n_planes * a.n_ranks;
  for (int64_t w = blockIdx.x; w < n_work; w += gridDim.x) {
    const int64_t plane = w / a.n_ranks;
    const int r = (int)(w - plane * a.n_ranks);
    const int hr = a.pass == 0 ? 0 : r;
    unsigned long long sum = 0;
    for (int g = 0; g < a.n_groups; ++g) sum += a.hist[((plane * a.n_groups + g) * a.n_ranks + hr) * 256 + t];
    count[t] = sum;
    __syncthreads();
    if (t == 0) {
      OsState s;
      if (a.pass == 0) {
        int64_t n_nan = 0;
        for (int g = 0; g < a.n_groups; ++g) n_nan += a.nans[plane * a.n_groups + g];
        const int64_t n_valid = a.n_values - n_nan;
        if (r == 0) a.nan_count[plane] = n_nan;
        s.prefix = 0;
        s.remaining = a.ranks[w];
        s.ok = (s.remaining >= 0 && s.remaining < n_valid) ? 1u : 0u;
      } else {
        s = a.state[w];
      }
      if (s.ok) {
        int64_t rem = s.remaining;
        int digit = 0;
        for (; digit < 255; ++digit) {
          const int64_t here = (int64_t)count[digit];
          if (rem < here) break;
          rem -= here;
        }
        s.remaining = rem;
        s.prefix |= (uint32_t)digit << shift;
      }
      a.state[w] = s;
      if (a.pass == 3) a.values[w] = __uint_as_float(s.ok ? prep_unkey(s.prefix) : 0x7fc00000u);
    }
    __syncthreads();
  }
}

size_t prefilter_workspace(int n_planes, int height, int width, int order) {
  if (order < 2 || height < 2) return 0;
  return (size_t)n_planes * (size_t)height * (size_t)width * sizeof(double);
}

size_t os_workspace(int n_planes, int64_t n_values, int n_ranks) {
  const size_t g = (size_t)os_groups(n_values);
  return (size_t)n_planes * n_ranks * sizeof(OsState) + (size_t)n_planes * g * ((size_t)n_ranks * 256 + 1) * sizeof(uint32_t);
}

template <bool ALONG_X>
int launch_prefilter(const PrefilterArgs& a, hipStream_t st) {
  const size_t lds = (size_t)(PREP_SEGMENT + 2 * a.halo) * PF_LS * sizeof(double);
  hipError_t e = hipFuncSetAttribute((const void*)prep_prefilter_kernel<ALONG_X>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
  if (e != hipSuccess) return (int)e;
  const int64_t n_tiles = (int64_t)a.n_groups * a.n_segments * a.n_planes;
  SUNERF_CLEAR_ERROR();
  hipLaunchKernelGGL(prep_prefilter_kernel<ALONG_X>, dim3(grid_of(n_tiles)), dim3(PF_THREADS), lds, st, a);
  SUNERF_CHECK_LAUNCH();
  return 0;
}

}  // namespace

extern "C" int sunerf_prep_abi_version(void) { return SUNERF_PREP_ABI_VERSION; }

extern "C" size_t sunerf_prep_workspace_bytes(int stage, int n_planes, int height, int width, int param) {
  if (n_planes <= 0 || height <= 0 || width <= 0) return 0;
  if (stage == SUNERF_PREP_STAGE_PREFILTER) {
    if (param < 0 || param > SUNERF_PREP_MAX_ORDER) return 0;
    return prefilter_workspace(n_planes, height, width, param);
  }
  if (stage == SUNERF_PREP_STAGE_ORDER_STATISTICS) {
    if (param < 1 || param > SUNERF_PREP_MAX_RANKS) return 0;
    return os_workspace(n_planes, (int64_t)height * width, param);
  }
  return 0;
}

extern "C" int sunerf_prep_spline_prefilter(const float* image, int n_planes, int height, int width, int order, double* coefficients,
                                            uint8_t* nonfinite_mask, void* workspace, size_t workspace_bytes, void* stream) {
  if (order < 0 || order > SUNERF_PREP_MAX_ORDER) return SUNERF_E_UNSUPPORTED;
  if (n_planes >= 0 && height >= 0 && width >= 0 && (n_planes == 0 || height == 0 || width == 0)) return 0;
  if (n_planes < 0 || height < 0 || width < 0 || !image || !coefficients) return SUNERF_E_BADARG;
  const size_t need = prefilter_workspace(n_planes, height, width, order);
  if (need && (!workspace || (uintptr_t)workspace % sizeof(double))) return SUNERF_E_BADARG;
  if ((uintptr_t)coefficients % sizeof(double)) return SUNERF_E_BADARG;
  if (workspace_bytes < need) return SUNERF_E_WORKSPACE;
  hipStream_t st = (hipStream_t)stream;
  double z[2];
  prep_poles(order, z);
  const bool along_y = need != 0;
  PrefilterArgs a;
  a.image = image; a.src = nullptr; a.dst = along_y ? (double*)workspace : coefficients; a.mask = nonfinite_mask;
  a.n_planes = n_planes; a.height = height; a.width = width;
  const bool filter_x = order >= 2 && width >= 2;
  a.n_poles = filter_x ? prep_n_poles(order) : 0;
  a.halo = filter_x ? prep_halo(order) : 0;
  a.z0 = z[0]; a.z1 = z[1]; a.gain = filter_x ? prep_gain(order) : 1.0;
  a.n_groups = (height + PREP_LINES - 1) / PREP_LINES;
  a.n_segments = (width + PREP_SEGMENT - 1) / PREP_SEGMENT;
  int status = launch_prefilter<true>(a, st);
  if (status) return status;
  if (along_y) {
    a.image = nullptr; a.src = (const double*)workspace; a.dst = coefficients; a.mask = nullptr;
    a.n_poles = prep_n_poles(order); a.halo = prep_halo(order); a.gain = prep_gain(order);
    a.n_groups = (width + PREP_LINES - 1) / PREP_LINES;
    a.n_segments = (height + PREP_SEGMENT - 1) / PREP_SEGMENT;
    status = launch_prefilter<false>(a, st);
  }
  return status;
}

extern "C" int sunerf_prep_affine_resample(const double* coefficients, const uint8_t* nonfinite_mask, int n_planes, int height,
                                           int width, int order, double m_yy, double m_yx, double m_xy, double m_xx,
                                           double offset_y, double offset_x, double missing, const double* params, int flags,
                                           int out_height, int out_width, float* out, void* stream) {
  if (order < 0 || order > SUNERF_PREP_MAX_ORDER || (flags & ~31)) return SUNERF_E_UNSUPPORTED;
  const bool negative = n_planes < 0 || height < 0 || width < 0 || out_height < 0 || out_width < 0;
  if (!negative && (n_planes == 0 || out_height == 0 || out_width == 0)) return 0;
  if (negative || height == 0 || width == 0 || !coefficients || !params || !out) return SUNERF_E_BADARG;
  if ((flags & SUNERF_PREP_PROPAGATE) && !nonfinite_mask) return SUNERF_E_BADARG;
  if ((uintptr_t)coefficients % sizeof(double) || (uintptr_t)params % sizeof(double)) return SUNERF_E_BADARG;
  ResampleArgs a;
  a.coef = coefficients; a.mask = nonfinite_mask; a.n_planes = n_planes; a.height = height; a.width = width;
  a.out_height = out_height; a.out_width = out_width;
  a.m_yy = m_yy; a.m_yx = m_yx; a.m_xy = m_xy; a.m_xx = m_xx; a.off_y = offset_y; a.off_x = offset_x; a.missing = missing;
  a.params = params; a.flags = flags; a.out = out;
  const int64_t total = (int64_t)n_planes * out_height * out_width;
  const dim3 grid(grid_of((total + RS_THREADS - 1) / RS_THREADS)), block(RS_THREADS);
  hipStream_t st = (hipStream_t)stream;
  SUNERF_CLEAR_ERROR();
  switch (order) {
    case 0: hipLaunchKernelGGL(prep_resample_kernel<0>, grid, block, 0, st, a); break;
    case 1: hipLaunchKernelGGL(prep_resample_kernel<1>, grid, block, 0, st, a); break;
    case 2: hipLaunchKernelGGL(prep_resample_kernel<2>, grid, block, 0, st, a); break;
    case 3: hipLaunchKernelGGL(prep_resample_kernel<3>, grid, block, 0, st, a); break;
    case 4: hipLaunchKernelGGL(prep_resample_kernel<4>, grid, block, 0, st, a); break;
    default: hipLaunchKernelGGL(prep_resample_kernel<5>, grid, block, 0, st, a); break;
  }
  SUNERF_CHECK_LAUNCH();
  return 0;
}

extern "C" int sunerf_prep_order_statistics(const float* x, int n_planes, int64_t n_values, const int64_t* ranks, int n_ranks,
                                            float* values, int64_t* nan_count, void* workspace, size_t workspace_bytes,
                                            void* stream) {
  if (n_ranks < 1 || n_ranks > SUNERF_PREP_MAX_RANKS) return SUNERF_E_UNSUPPORTED;
  if (n_planes >= 0 && n_values >= 0 && (n_planes == 0 || n_values == 0)) return 0;
  if (n_planes < 0 || n_values < 0 || !x || !ranks || !values || !nan_count || !workspace) return SUNERF_E_BADARG;
  if ((uintptr_t)workspace % sizeof(int64_t) || (uintptr_t)ranks % sizeof(int64_t) || (uintptr_t)nan_count % sizeof(int64_t))
    return SUNERF_E_BADARG;
  if (workspace_bytes < os_workspace(n_planes, n_values, n_ranks)) return SUNERF_E_WORKSPACE;
  OsArgs a;
  a.x = x; a.n_planes = n_planes; a.n_ranks = n_ranks; a.n_groups = os_groups(n_values); a.n_values = n_values;
  a.ranks = ranks; a.values = values; a.nan_count = nan_count;
  a.state = (OsState*)workspace;
  a.hist = (uint32_t*)((char*)workspace + (size_t)n_planes * n_ranks * sizeof(OsState));
  a.nans = a.hist + (size_t)n_planes * a.n_groups * n_ranks * 256;
  hipStream_t st = (hipStream_t)stream;
  for (int pass = 0; pass < 4; ++pass) {
    a.pass = pass;
    SUNERF_CLEAR_ERROR();
    hipLaunchKernelGGL(prep_os_histogram_kernel, dim3(grid_of((int64_t)n_planes * a.n_groups)), dim3(OS_THREADS), 0, st, a);
    SUNERF_CHECK_LAUNCH();
    hipLaunchKernelGGL(prep_os_select_kernel, dim3(grid_of((int64_t)n_planes * n_ranks)), dim3(OS_THREADS), 0, st, a);
    SUNERF_CHECK_LAUNCH();
  }
  return 0;
}
