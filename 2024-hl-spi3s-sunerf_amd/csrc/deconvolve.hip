// Richardson-Lucy deconvolution of detector images against the instrument's PSF-and-bin kernel (include/sunerf_hip_deconvolve.h,
// DESIGN.md section 8s): the classical baseline beside training through the instrument.  One entry point enqueues, per iteration,
//
// 1. the RATIO kernel: the strided correlation of instrument.hip (same tile rule, LDS staging, boundary handling, taps by scalar
//    load, up to four outputs per thread) whose epilogue keeps the fp64 sum, forms ratio = (d + off) / (A u + off) and the
//    pixel's term of the Poisson deviance, and reduces the terms of the tile in a fixed order (a butterfly inside each wave, the
//    four waves in index order) into ONE partial per tile, indexed by the tile's number: the sum does not depend on the grid;
// 2. the CONTROL kernel: one workgroup per plane adds the plane's partials in a fixed order, writes the plane's state and decides
//    whether the plane stops -- on the device, so that the host never waits between iterations;
// 3. the UPDATE kernel: the gather-form adjoint of patch.hip (same tiles of 32 x 32 input pixels, LDS layout and order of
//    summation) whose epilogue is u' = u * (A^T ratio) / norm, in place: a thread reads and writes only its own pixels of u.
//
// A stopped plane's workgroups return at once from all three.  The device functions of instrument.hip and patch.hip are restated
// here with their comments cut down to what differs: those files explain the loops.
// No floating-point atomics; -ffp-contract=off and no explicit fma: every operation is rounded on its own, as the header says.
#include "sunerf_common.h"
#include "../../include/sunerf_hip_deconvolve.h"

namespace {

constexpr int RL_THREADS = 256;
constexpr int RL_WAVES = RL_THREADS / 64;
constexpr int RL_MAX_WORDS = 127 * 127;        // LDS words of the largest input tile of the ratio kernel
constexpr int RL_TILE = SUNERF_PATCH_TILE;     // input pixels per side of an update tile
constexpr int RL_NM = RL_TILE * RL_TILE / RL_THREADS;

static_assert(SUNERF_INSTRUMENT_TILE * SUNERF_INSTRUMENT_TILE == 4 * RL_THREADS, "four outputs per thread at most");
static_assert(SUNERF_INSTRUMENT_TILE - 1 + SUNERF_INSTRUMENT_MAX_KERNEL == 127, "the largest tile is 127 words wide");
static_assert(RL_TILE * RL_TILE == RL_NM * RL_THREADS, "whole pixels per thread");

typedef __attribute__((address_space(3))) double LdsF64;
typedef __attribute__((address_space(3))) float LdsF32;

struct RlArgs {
  int n_planes, height, width, out_h, out_w;
  int n_kernels, kh, kw, bin, ay, ax;
  int tile, tiles_y, tiles_x;          // the ratio kernel's tiles of detector pixels
  int up_tiles_y, up_tiles_x;          // the update kernel's tiles of input pixels
  double scale, stop;
};

int corr_tile(int kh, int kw, int bin) {
  const int k = kh > kw ? kh : kw;
  const int t = (127 - k) / bin + 1;
  return t < SUNERF_INSTRUMENT_TILE ? t : SUNERF_INSTRUMENT_TILE;
}

__device__ __forceinline__ bool plane_stopped(const double* state, int64_t plane, int pass) {
  return pass > 0 && state[plane * SUNERF_DECONVOLVE_STATE + 3] != 0.0;      // pass 0 finds the state unwritten
}

// ---- ratio ----------------------------------------------------------------------------------------------------------------------
template <bool NEAREST, int NM>
__global__ __launch_bounds__(RL_THREADS) void deconvolve_ratio_kernel(const float* __restrict__ u, const float* __restrict__ d,
                                                                      const uint8_t* __restrict__ bad, const double* __restrict__ params,
                                                                      const double* __restrict__ K, float* __restrict__ ratio,
                                                                      const double* __restrict__ state, double* __restrict__ partials,
                                                                      int pass, RlArgs a) {
  extern __shared__ float tile[];                // [lh][lw]
  __shared__ double wave_sum[2 * RL_WAVES];
  const int t = threadIdx.x;
  const int T = a.tile;
  const int lh = (T - 1) * a.bin + a.kh, lw = (T - 1) * a.bin + a.kw;
  const int64_t in_px = (int64_t)a.height * a.width, out_px = (int64_t)a.out_h * a.out_w;
  const int64_t tiles_per_plane = (int64_t)a.tiles_y * a.tiles_x;
  const int64_t n_tiles = tiles_per_plane * a.n_planes;
  for (int64_t tile_id = blockIdx.x; tile_id < n_tiles; tile_id += gridDim.x) {
    const int64_t plane = tile_id / tiles_per_plane;
    if (plane_stopped(state, plane, pass)) continue;          // the whole workgroup: the plane is the tile's
    const int in_plane = (int)(tile_id - plane * tiles_per_plane);
    const int r0 = (in_plane / a.tiles_x) * T, c0 = (in_plane % a.tiles_x) * T;
    const int y0 = r0 * a.bin - a.ay, x0 = c0 * a.bin - a.ax;
    const float* src = u + plane * in_px;
    for (int i = t; i < lh * lw; i += RL_THREADS) {
      const int ly = i / lw;
      int y = y0 + ly, x = x0 + (i - ly * lw);
      float v = 0.f;
      if (NEAREST) {
        y = y < 0 ? 0 : (y >= a.height ? a.height - 1 : y);
        x = x < 0 ? 0 : (x >= a.width ? a.width - 1 : x);
        v = src[(int64_t)y * a.width + x];
      } else if (y >= 0 && y < a.height && x >= 0 && x < a.width) {
        v = src[(int64_t)y * a.width + x];
      }
      tile[i] = v;
    }
    __syncthreads();
    int base[NM];
    bool live[NM];
    double acc[NM];
#pragma unroll
    for (int m = 0; m < NM; ++m) {
      const int o = t + RL_THREADS * m;
      const int r = o / T, c = o - r * T;
      live[m] = o < T * T && r0 + r < a.out_h && c0 + c < a.out_w;
      base[m] = live[m] ? (r * a.bin) * lw + c * a.bin : 0;
      acc[m] = -0.0;
    }
    const double* taps = K + (a.n_kernels == 1 ? (int64_t)0 : plane) * a.kh * a.kw;      // wave-uniform
    for (int i = 0; i < a.kh; ++i) {
      const float* row = tile + i * lw;
#pragma unroll 8
      for (int j = 0; j < a.kw; ++j) {
        const double w = taps[i * a.kw + j];
#pragma unroll
        for (int m = 0; m < NM; ++m) acc[m] = acc[m] + w * (double)row[base[m] + j];
      }
    }
    const double c_ph = params[2 * plane], off = params[2 * plane + 1] / c_ph;            // wave-uniform
    double dev = 0.0, count = 0.0;               // the thread's terms, m ascending
#pragma unroll
    for (int m = 0; m < NM; ++m) {
      if (live[m]) {
        const int o = t + RL_THREADS * m;
        const int r = o / T, c = o - r * T;
        const int64_t px = plane * out_px + (int64_t)(r0 + r) * a.out_w + c0 + c;
        const float obs = d[px];
        const bool valid = isfinite(obs) && !(bad && bad[px]);
        const double den = a.scale * acc[m] + off;
        double num = valid ? (double)obs + off : 0.0;
        num = num > 0.0 ? num : 0.0;
        const bool fit = valid && den > 0.0;
        ratio[px] = fit ? (float)(num / den) : 0.f;
        if (fit) {
          const double L = c_ph * den, N = c_ph * num;
          dev = dev + 2.0 * ((L - N) + (N > 0.0 ? N * log(N / L) : 0.0));
        }
        if (valid) count = count + 1.0;
      }
    }
#pragma unroll
    for (int step = 32; step >= 1; step >>= 1) {          // every lane ends with the wave's sum, formed in one order
      dev = dev + __shfl_xor(dev, step);
      count = count + __shfl_xor(count, step);
    }
    if ((t & 63) == 0) {
      wave_sum[2 * (t >> 6)] = dev;
      wave_sum[2 * (t >> 6) + 1] = count;
    }
    __syncthreads();
    if (t == 0) {
      double s = wave_sum[0], n = wave_sum[1];
#pragma unroll
      for (int w = 1; w < RL_WAVES; ++w) {
        s = s + wave_sum[2 * w];
        n = n + wave_sum[2 * w + 1];
      }
      partials[2 * tile_id] = s;
      partials[2 * tile_id + 1] = n;
    }
    __syncthreads();                             // the tile and the waves' sums are overwritten by the next tile
  }
}

// ---- control --------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(RL_THREADS) void deconvolve_control_kernel(const double* __restrict__ partials, double* __restrict__ state,
                                                                        int64_t tiles_per_plane, double stop, int pass, int last) {
  __shared__ double sum[2 * RL_THREADS];
  const int t = threadIdx.x;
  const int64_t plane = blockIdx.x;
  if (plane_stopped(state, plane, pass)) return;
  const double* p = partials + 2 * plane * tiles_per_plane;
  double s = 0.0, n = 0.0;                       // partials t, t + 256, ... in that order
  for (int64_t i = t; i < tiles_per_plane; i += RL_THREADS) {
    s = s + p[2 * i];
    n = n + p[2 * i + 1];
  }
  sum[2 * t] = s;
  sum[2 * t + 1] = n;
  for (int half = RL_THREADS / 2; half >= 1; half >>= 1) {
    __syncthreads();
    if (t < half) {
      sum[2 * t] = sum[2 * t] + sum[2 * (t + half)];
      sum[2 * t + 1] = sum[2 * t + 1] + sum[2 * (t + half) + 1];
    }
  }
  if (t == 0) {
    double* st = state + plane * SUNERF_DECONVOLVE_STATE;
    const double deviance = sum[0], n_valid = sum[1];
    double applied = pass > 0 ? st[2] : 0.0;
    const bool stopped = stop > 0.0 && deviance <= stop * n_valid;
    if (!stopped && !last) applied = applied + 1.0;          // the update that follows this pass
    st[0] = deviance; st[1] = n_valid; st[2] = applied; st[3] = stopped ? 1.0 : 0.0;
  }
}

// ---- update ---------------------------------------------------------------------------------------------------------------------
__host__ __device__ __forceinline__ int floor_div(int a, int b) {      // b > 0
  const int q = a / b;
  return (a % b != 0 && a < 0) ? q - 1 : q;
}
__host__ __device__ __forceinline__ int ceil_div(int a, int b) { return -floor_div(-a, b); }

__device__ __forceinline__ int tap_word(int i, int j, int bin, int kwb) { return (i * bin + j % bin) * kwb + j / bin; }

// every term of one pixel that taps were clamped onto (BOUNDARY_NEAREST, a pixel on the edge): patch.hip's adjoint_pixel_clamped
__device__ __forceinline__ double update_pixel_clamped(const LdsF64* taps, const LdsF32* slice, const RlArgs& a, int kwb, int y, int x, int r_lo,
                                                       int r_hi, int c_lo, int c_hi) {
  const int bin = a.bin, n_c = c_hi - c_lo + 1;
  const bool top = y == 0, bottom = y == a.height - 1, left = x == 0, right = x == a.width - 1;
  const int ty = y + a.ay, tx = x + a.ax;
  double acc = 0.0;
  int qy = ty / bin, ry = ty - qy * bin;
  for (int i = 0; i < a.kh; ++i) {
    int ra = top ? 0 : qy + (ry > 0), rb = bottom ? a.out_h - 1 : qy;
    ra = ra < r_lo ? r_lo : ra; rb = rb > r_hi ? r_hi : rb;
    if (ra <= rb) {
      int qx = tx / bin, rx = tx - qx * bin;
      int word = i * bin * kwb, jm = 0;
      for (int j = 0; j < a.kw; ++j) {
        int ca = left ? 0 : qx + (rx > 0), cb = right ? a.out_w - 1 : qx;
        ca = ca < c_lo ? c_lo : ca; cb = cb > c_hi ? c_hi : cb;
        if (ca <= cb) {
          const double w = taps[word];
          for (int R = ra; R <= rb; ++R) {
            const LdsF32* grow = slice + (R - r_lo) * n_c - c_lo;
            for (int C = ca; C <= cb; ++C) acc = acc + w * (double)grow[C];
          }
        }
        if (--rx < 0) { rx += bin; --qx; }
        word += kwb;
        if (++jm == bin) { jm = 0; word -= bin * kwb - 1; }
      }
    }
    if (--ry < 0) { ry += bin; --qy; }
  }
  return acc;
}

template <bool NEAREST>
__global__ __launch_bounds__(RL_THREADS) void deconvolve_update_kernel(const float* __restrict__ ratio, const double* __restrict__ K,
                                                                       const float* __restrict__ norm, const double* __restrict__ state,
                                                                       float* __restrict__ u, RlArgs a) {
  extern __shared__ __attribute__((aligned(8))) unsigned char lds[];
  const int bin = a.bin;
  const int kwb = (a.kw + bin - 1) / bin;
  const int sw = (RL_TILE + a.kw - 2) / bin + 1;
  LdsF64* taps = (LdsF64*)lds;                                        // [kh][bin][kwb]: tap_word
  LdsF64* zero_taps = taps + a.kh * bin * kwb;                        // [kwb] of 0.0
  LdsF32* zero_row = (LdsF32*)(zero_taps + kwb);                      // [sw] of 0.f
  LdsF32* slice = zero_row + sw;                                      // [n_r][n_c] of the tile at hand
  const int t = threadIdx.x;
  const int lx = t % RL_TILE, ly = t / RL_TILE;
  for (int i = t; i < kwb; i += RL_THREADS) zero_taps[i] = 0.0;
  for (int i = t; i < sw; i += RL_THREADS) zero_row[i] = 0.f;
  const int64_t in_px = (int64_t)a.height * a.width, out_px = (int64_t)a.out_h * a.out_w;
  const int64_t tiles_per_plane = (int64_t)a.up_tiles_y * a.up_tiles_x;
  const int64_t n_tiles = tiles_per_plane * a.n_planes;
  int64_t staged = -1;
  for (int64_t tile_id = blockIdx.x; tile_id < n_tiles; tile_id += gridDim.x) {
    const int64_t plane = tile_id / tiles_per_plane;
    if (plane_stopped(state, plane, 1)) continue;                     // the control pass before this launch wrote the state
    const int in_plane = (int)(tile_id - plane * tiles_per_plane);
    const int y0 = (in_plane / a.up_tiles_x) * RL_TILE, x0 = (in_plane % a.up_tiles_x) * RL_TILE;
    const int y_last = (y0 + RL_TILE < a.height ? y0 + RL_TILE : a.height) - 1;
    const int x_last = (x0 + RL_TILE < a.width ? x0 + RL_TILE : a.width) - 1;
    int r_lo = ceil_div(y0 + a.ay - (a.kh - 1), bin), r_hi = floor_div(y_last + a.ay, bin);
    int c_lo = ceil_div(x0 + a.ax - (a.kw - 1), bin), c_hi = floor_div(x_last + a.ax, bin);
    r_lo = r_lo < 0 ? 0 : r_lo; r_hi = r_hi > a.out_h - 1 ? a.out_h - 1 : r_hi;
    c_lo = c_lo < 0 ? 0 : c_lo; c_hi = c_hi > a.out_w - 1 ? a.out_w - 1 : c_hi;
    const int n_r = r_hi - r_lo + 1, n_c = c_hi - c_lo + 1;           // either may be <= 0: no tap reaches the tile
    const int64_t kernel = a.n_kernels == 1 ? (int64_t)0 : plane;
    if (kernel != staged) {
      const double* src = K + kernel * a.kh * a.kw;
      for (int i = t; i < a.kh * a.kw; i += RL_THREADS) taps[tap_word(i / a.kw, i % a.kw, bin, kwb)] = src[i];
      staged = kernel;
    }
    if (n_r > 0 && n_c > 0) {
      const float* src = ratio + plane * out_px;
      for (int i = t; i < n_r * n_c; i += RL_THREADS) {
        const int r = i / n_c;
        slice[i] = src[(int64_t)(r_lo + r) * a.out_w + c_lo + (i - r * n_c)];
      }
    }
    __syncthreads();
    const int x = x0 + lx;
    if (x < a.width) {
      double acc[RL_NM];
      bool clamped[RL_NM];
#pragma unroll
      for (int m = 0; m < RL_NM; ++m) {
        const int y = y0 + ly + (RL_THREADS / RL_TILE) * m;
        acc[m] = 0.0;
        clamped[m] = NEAREST && y < a.height && (x == 0 || x == a.width - 1 || y == 0 || y == a.height - 1);
      }
      if (n_r > 0 && n_c > 0) {
        {
          const int tx = x + a.ax, j0 = tx % bin, C0 = tx / bin;
          const int b_min = C0 - c_hi > 0 ? C0 - c_hi : 0;
          int b_max = j0 < a.kw ? (a.kw - 1 - j0) / bin : -1;
          b_max = b_max < C0 - c_lo ? b_max : C0 - c_lo;
          int i0[RL_NM], R0[RL_NM], s_min[RL_NM], s_max[RL_NM];
          int s_begin = 0x7fffffff, s_end = -1;
#pragma unroll
          for (int m = 0; m < RL_NM; ++m) {
            const int y = y0 + ly + (RL_THREADS / RL_TILE) * m;
            const int ty = y + a.ay;
            i0[m] = ty % bin; R0[m] = ty / bin;
            s_min[m] = R0[m] - r_hi > 0 ? R0[m] - r_hi : 0;
            s_max[m] = i0[m] < a.kh ? (a.kh - 1 - i0[m]) / bin : -1;
            s_max[m] = s_max[m] < R0[m] - r_lo ? s_max[m] : R0[m] - r_lo;
            if (y >= a.height || clamped[m]) { s_min[m] = 1; s_max[m] = 0; }
            if (s_min[m] <= s_max[m]) {
              s_begin = s_begin < s_min[m] ? s_begin : s_min[m];
              s_end = s_end > s_max[m] ? s_end : s_max[m];
            }
          }
          for (int s = s_begin; s <= s_end; ++s) {
            const LdsF64* kq[RL_NM];
            const LdsF32* gq[RL_NM];
#pragma unroll
            for (int m = 0; m < RL_NM; ++m) {
              const bool live = s >= s_min[m] && s <= s_max[m];
              kq[m] = live ? taps + ((i0[m] + s * bin) * bin + j0) * kwb : zero_taps;
              gq[m] = live ? slice + (R0[m] - s - r_lo) * n_c + (C0 - c_lo) : zero_row + (sw - 1);
            }
#pragma unroll 4
            for (int b = b_min; b <= b_max; ++b) {
#pragma unroll
              for (int m = 0; m < RL_NM; ++m) acc[m] = acc[m] + kq[m][b] * (double)gq[m][-b];
            }
          }
        }
        if (NEAREST) {
#pragma unroll 1
          for (int m = 0; m < RL_NM; ++m) {
            const int y = y0 + ly + (RL_THREADS / RL_TILE) * m;
            if (clamped[m]) acc[m] = update_pixel_clamped(taps, slice, a, kwb, y, x, r_lo, r_hi, c_lo, c_hi);
          }
        }
      }
#pragma unroll
      for (int m = 0; m < RL_NM; ++m) {
        const int y = y0 + ly + (RL_THREADS / RL_TILE) * m;
        if (y < a.height) {
          const int64_t px = plane * in_px + (int64_t)y * a.width + x;
          const float nm = norm[px];
          if (nm > 0.f) u[px] = (float)(((double)u[px] * (a.scale * acc[m])) / (double)nm);
        }
      }
    }
    __syncthreads();                             // the slice (and a per-plane kernel) is overwritten by the next tile
  }
}

unsigned grid_of(int64_t work) {
  const int64_t cap = (int64_t)1 << 20;
  return (unsigned)(work < 1 ? 1 : (work < cap ? work : cap));
}

struct RlBuffers {
  float* u; const float* d; const uint8_t* bad; const float* norm; const double* params; const double* K;
  float* ratio; double* state; double* partials;
};

template <bool NEAREST>
void launch_ratio(int nm, dim3 grid, size_t lds, hipStream_t st, const RlBuffers& b, int pass, const RlArgs& a) {
#define RL_RATIO(NM)                                                                                                              \
  hipLaunchKernelGGL((deconvolve_ratio_kernel<NEAREST, NM>), grid, dim3(RL_THREADS), lds, st, (const float*)b.u, b.d, b.bad, b.params, b.K, \
                     b.ratio, (const double*)b.state, b.partials, pass, a)
  switch (nm) {
    case 1: RL_RATIO(1); break;
    case 2: RL_RATIO(2); break;
    case 3: RL_RATIO(3); break;
    default: RL_RATIO(4); break;
  }
#undef RL_RATIO
}

template <bool NEAREST>
int run(const RlBuffers& b, const RlArgs& a, int n_iterations, hipStream_t st) {
  const int lh = (a.tile - 1) * a.bin + a.kh, lw = (a.tile - 1) * a.bin + a.kw;
  const size_t ratio_lds = (size_t)lh * lw * sizeof(float);
  const int nm = (a.tile * a.tile + RL_THREADS - 1) / RL_THREADS;
  const int64_t tiles_per_plane = (int64_t)a.tiles_y * a.tiles_x;
  const dim3 ratio_grid(grid_of(tiles_per_plane * a.n_planes));
  const int sh = (RL_TILE + a.kh - 2) / a.bin + 1, sw = (RL_TILE + a.kw - 2) / a.bin + 1;
  const int kwb = (a.kw + a.bin - 1) / a.bin;
  const size_t update_lds = ((size_t)a.kh * a.bin * kwb + kwb) * sizeof(double) + ((size_t)sh * sw + sw) * sizeof(float);
  const dim3 update_grid(grid_of((int64_t)a.up_tiles_y * a.up_tiles_x * a.n_planes));
  if (n_iterations > 0 && update_lds > 64 * 1024) {
    hipError_t e = hipFuncSetAttribute((const void*)deconvolve_update_kernel<NEAREST>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)update_lds);
    if (e != hipSuccess) return (int)e;
  }
  SUNERF_CLEAR_ERROR();
  for (int pass = 0; pass <= n_iterations; ++pass) {          // pass n_iterations describes the last iterate: no update follows it
    const int last = pass == n_iterations;
    launch_ratio<NEAREST>(nm, ratio_grid, ratio_lds, st, b, pass, a);
    hipLaunchKernelGGL(deconvolve_control_kernel, dim3((unsigned)a.n_planes), dim3(RL_THREADS), 0, st, (const double*)b.partials, b.state,
                       tiles_per_plane, a.stop, pass, last);
    if (!last)
      hipLaunchKernelGGL(deconvolve_update_kernel<NEAREST>, update_grid, dim3(RL_THREADS), update_lds, st, (const float*)b.ratio, b.K, b.norm,
                         (const double*)b.state, b.u, a);
    SUNERF_CHECK_LAUNCH();
  }
  return 0;
}

bool within_limits(int kh, int kw, int bin) {
  return kh <= SUNERF_INSTRUMENT_MAX_KERNEL && kw <= SUNERF_INSTRUMENT_MAX_KERNEL && bin <= SUNERF_INSTRUMENT_MAX_BIN;
}

int64_t ratio_tiles(int height, int width, int kh, int kw, int bin) {
  const int tile = corr_tile(kh, kw, bin);
  return (int64_t)((height / bin + tile - 1) / tile) * ((width / bin + tile - 1) / tile);
}

}  // namespace

extern "C" int sunerf_deconvolve_abi_version(void) { return SUNERF_DECONVOLVE_ABI_VERSION; }

extern "C" size_t sunerf_deconvolve_workspace_bytes(int n_planes, int height, int width, int kh, int kw, int bin) {
  if (n_planes < 1 || height < 1 || width < 1 || kh < 1 || kw < 1 || bin < 1 || !within_limits(kh, kw, bin)) return 0;
  return (size_t)n_planes * (size_t)ratio_tiles(height, width, kh, kw, bin) * 2 * sizeof(double);
}

extern "C" int sunerf_deconvolve_richardson_lucy(float* u, const float* d, const uint8_t* bad, const float* norm, const double* params,
                                                 int n_planes, int height, int width, const double* K, int n_kernels, int kh, int kw,
                                                 int bin, int anchor_y, int anchor_x, double scale, int boundary, int n_iterations,
                                                 double stop, float* ratio, double* state, void* workspace, void* stream) {
  if (!within_limits(kh, kw, bin)) return SUNERF_E_UNSUPPORTED;
  if (boundary != SUNERF_INSTRUMENT_BOUNDARY_ZERO && boundary != SUNERF_INSTRUMENT_BOUNDARY_NEAREST) return SUNERF_E_UNSUPPORTED;
  const bool bad_count = n_planes < 0 || height < 0 || width < 0 || kh < 1 || kw < 1 || bin < 1;
  if (!bad_count && (n_planes == 0 || height / bin == 0 || width / bin == 0)) return 0;
  if (bad_count || (n_kernels != 1 && n_kernels != n_planes)) return SUNERF_E_BADARG;
  if (anchor_y < 0 || anchor_y >= kh || anchor_x < 0 || anchor_x >= kw) return SUNERF_E_BADARG;
  if (n_iterations < 0 || n_iterations > SUNERF_DECONVOLVE_MAX_ITERATIONS || !(stop >= 0.0)) return SUNERF_E_BADARG;
  if (!u || !d || !norm || !params || !K || !ratio || !state || !workspace) return SUNERF_E_BADARG;      // the size is non-zero here
  if ((uintptr_t)params % sizeof(double) || (uintptr_t)K % sizeof(double) || (uintptr_t)state % sizeof(double) ||
      (uintptr_t)workspace % sizeof(double))
    return SUNERF_E_BADARG;
  RlArgs a;
  a.n_planes = n_planes; a.height = height; a.width = width; a.out_h = height / bin; a.out_w = width / bin;
  a.n_kernels = n_kernels; a.kh = kh; a.kw = kw; a.bin = bin; a.ay = anchor_y; a.ax = anchor_x;
  a.tile = corr_tile(kh, kw, bin);
  a.tiles_y = (a.out_h + a.tile - 1) / a.tile; a.tiles_x = (a.out_w + a.tile - 1) / a.tile;
  a.up_tiles_y = (height + RL_TILE - 1) / RL_TILE; a.up_tiles_x = (width + RL_TILE - 1) / RL_TILE;
  a.scale = scale; a.stop = stop;
  const int lh = (a.tile - 1) * bin + kh, lw = (a.tile - 1) * bin + kw;
  if (lh * lw > RL_MAX_WORDS) return SUNERF_E_UNSUPPORTED;          // cannot happen inside the limits above
  const RlBuffers b{u, d, bad, norm, params, K, ratio, state, (double*)workspace};
  hipStream_t st = (hipStream_t)stream;
  if (boundary == SUNERF_INSTRUMENT_BOUNDARY_NEAREST) return run<true>(b, a, n_iterations, st);
  return run<false>(b, a, n_iterations, st);
}
