// A rendered frame becomes a detector image: strided correlation with the PSF-and-bin kernel, photon and read noise,
// digitisation, saturation (include/sunerf_hip_instrument.h).
//
// 1. Correlation.  A workgroup takes a tile of T x T detector pixels of one plane, T = min(32, (127 - max(kh, kw)) / bin + 1):
//    all 256 threads stage the input tile with its halo, ((T - 1) bin + kh) x ((T - 1) bin + kw) fp32 words (at most 127 x 127 =
//    63 KiB), in LDS -- the boundary rule is applied there, once per staged word -- and every thread then owns up to four output
//    pixels (output t + 256 m of the tile, row-major) and walks the taps in the header's order, row by row.  The tap K[i][j] is
//    the same for every lane: its address is built from blockIdx and the loop counters only, so it is fetched by a scalar load
//    into SGPRs, once per wave, and the inner loop is one LDS read, one convert, one fp64 multiply and one fp64 add per output.
// 2. Noise.  One thread per element; the generator is Philox4x32-10 keyed by the seed and counted by the element's index, so the
//    value of an element does not depend on the launch geometry, on its neighbours or on how a frame is cut into calls.
// No floating-point atomics; -ffp-contract=off and no explicit fma: every operation is rounded on its own, as the header says.
#include "sunerf_common.h"
#include "../../include/sunerf_hip_instrument.h"

namespace {

constexpr int CB_THREADS = 256;
constexpr int CB_MAX_WORDS = 127 * 127;        // LDS words of the largest input tile

static_assert(SUNERF_INSTRUMENT_TILE * SUNERF_INSTRUMENT_TILE == 4 * CB_THREADS, "four outputs per thread at most");
static_assert(SUNERF_INSTRUMENT_TILE - 1 + SUNERF_INSTRUMENT_MAX_KERNEL == 127, "the largest tile is 127 words wide");

struct CorrArgs {
  int n_planes, height, width, out_h, out_w;
  int n_kernels, kh, kw, bin, ay, ax;
  int tile, tiles_y, tiles_x;
  double scale;
};

int corr_tile(int kh, int kw, int bin) {
  const int k = kh > kw ? kh : kw;
  const int t = (127 - k) / bin + 1;
  return t < SUNERF_INSTRUMENT_TILE ? t : SUNERF_INSTRUMENT_TILE;
}

template <bool NEAREST, int NM>
__global__ __launch_bounds__(CB_THREADS) void instrument_correlate_kernel(const float* __restrict__ in, const double* __restrict__ K,
                                                                          float* __restrict__ out, CorrArgs a) {
  extern __shared__ float tile[];                // [lh][lw]
  const int t = threadIdx.x;
  const int T = a.tile;
  const int lh = (T - 1) * a.bin + a.kh, lw = (T - 1) * a.bin + a.kw;
  const int64_t in_px = (int64_t)a.height * a.width, out_px = (int64_t)a.out_h * a.out_w;
  const int64_t tiles_per_plane = (int64_t)a.tiles_y * a.tiles_x;
  const int64_t n_tiles = tiles_per_plane * a.n_planes;
  for (int64_t tile_id = blockIdx.x; tile_id < n_tiles; tile_id += gridDim.x) {
    const int64_t plane = tile_id / tiles_per_plane;
    const int in_plane = (int)(tile_id - plane * tiles_per_plane);
    const int r0 = (in_plane / a.tiles_x) * T, c0 = (in_plane % a.tiles_x) * T;       // first output pixel of the tile
    const int y0 = r0 * a.bin - a.ay, x0 = c0 * a.bin - a.ax;                         // input pixel of LDS word (0, 0)
    const float* src = in + plane * in_px;
    for (int i = t; i < lh * lw; i += CB_THREADS) {
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
      const int o = t + CB_THREADS * m;
      const int r = o / T, c = o - r * T;
      live[m] = o < T * T && r0 + r < a.out_h && c0 + c < a.out_w;
      base[m] = live[m] ? (r * a.bin) * lw + c * a.bin : 0;          // a dead slot reads word (i, j): inside the tile
      acc[m] = -0.0;                              // -0.0 + x == x for every x: the first product starts the sum
    }
    const double* taps = K + (a.n_kernels == 1 ? (int64_t)0 : plane) * a.kh * a.kw;      // wave-uniform
    for (int i = 0; i < a.kh; ++i) {
      const float* row = tile + i * lw;
#pragma unroll 8
      for (int j = 0; j < a.kw; ++j) {          // unrolled: eight taps per scalar load, eight LDS reads in flight per output
        const double w = taps[i * a.kw + j];
#pragma unroll
        for (int m = 0; m < NM; ++m) acc[m] = acc[m] + w * (double)row[base[m] + j];
      }
    }
#pragma unroll
    for (int m = 0; m < NM; ++m) {
      if (live[m]) {
        const int o = t + CB_THREADS * m;
        const int r = o / T, c = o - r * T;
        out[plane * out_px + (int64_t)(r0 + r) * a.out_w + c0 + c] = (float)(a.scale * acc[m]);
      }
    }
    __syncthreads();                             // the tile is overwritten by the next one
  }
}

// ---- Philox4x32-10 --------------------------------------------------------------------------------------------------------------
struct Block4 {
  uint32_t w[4];
};

__device__ __forceinline__ Block4 philox4x32_10(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0, uint32_t k1) {
#pragma unroll
  for (int round = 0; round < 10; ++round) {
    const uint64_t p0 = (uint64_t)0xD2511F53u * c0, p1 = (uint64_t)0xCD9E8D57u * c2;
    const uint32_t n0 = (uint32_t)(p1 >> 32) ^ c1 ^ k0, n2 = (uint32_t)(p0 >> 32) ^ c3 ^ k1;
    c0 = n0; c1 = (uint32_t)p1; c2 = n2; c3 = (uint32_t)p0;
    k0 += 0x9E3779B9u; k1 += 0xBB67AE85u;
  }
  return Block4{{c0, c1, c2, c3}};
}

constexpr int PX_THREADS = 256;

__global__ __launch_bounds__(PX_THREADS) void instrument_philox_kernel(const uint32_t* __restrict__ ctr, int64_t n, uint32_t k0, uint32_t k1,
                                                                       uint32_t* __restrict__ out) {
  for (int64_t i = (int64_t)blockIdx.x * PX_THREADS + threadIdx.x; i < n; i += (int64_t)gridDim.x * PX_THREADS) {
    const Block4 b = philox4x32_10(ctr[4 * i], ctr[4 * i + 1], ctr[4 * i + 2], ctr[4 * i + 3], k0, k1);
    for (int k = 0; k < 4; ++k) out[4 * i + k] = b.w[k];
  }
}

// ---- noise ----------------------------------------------------------------------------------------------------------------------
constexpr int NZ_THREADS = 256;

__device__ __forceinline__ double uniform53(uint32_t hi, uint32_t lo) {          // (0, 1], exact
  return ((double)(hi >> 5) * 67108864.0 + (double)(lo >> 6) + 1.0) * 1.1102230246251565e-16;
}

struct Draw {
  double ua, ub;
};

__device__ __forceinline__ Draw draw(uint64_t e, uint32_t j, uint32_t s, uint64_t seed) {
  const Block4 b = philox4x32_10((uint32_t)e, (uint32_t)(e >> 32), j, s, (uint32_t)seed, (uint32_t)(seed >> 32));
  return Draw{uniform53(b.w[0], b.w[1]), uniform53(b.w[2], b.w[3])};
}

__device__ double poisson(double lam, uint64_t e, uint64_t seed) {
  if (lam < 10.0) {
    const double u = draw(e, 0u, 0u, seed).ua;
    double k = 0.0, p = exp(-lam), s = p;
    while (u > s && k < 200.0) {
      k += 1.0;
      p = p * (lam / k);
      s = s + p;
    }
    return k;
  }
  const double slam = sqrt(lam), loglam = log(lam);
  const double b = 0.931 + 2.53 * slam;
  const double a = -0.059 + 0.02483 * b;
  const double invalpha = 1.1239 + 1.1328 / (b - 3.4);
  const double vr = 0.9277 - 3.6224 / (b - 2.0);
  for (uint32_t j = 0; j < SUNERF_INSTRUMENT_MAX_ROUNDS; ++j) {
    const Draw d = draw(e, j, 0u, seed);
    const double U = d.ua - 0.5, V = d.ub;
    const double us = 0.5 - fabs(U);
    const double k = floor(((2.0 * a) / us + b) * U + lam + 0.43);
    if (us >= 0.07 && V <= vr) return k;
    if (k < 0.0 || (us < 0.013 && V > us)) continue;
    if ((log(V) + log(invalpha)) - log(a / (us * us) + b) <= (-lam + k * loglam) - lgamma(k + 1.0)) return k;
  }
  return rint(lam);
}

struct NoiseArgs {
  int64_t total, plane_px, index_offset;
  uint64_t seed;
  int flags;
};

__global__ __launch_bounds__(NZ_THREADS) void instrument_noise_kernel(const float* __restrict__ expected, const double* __restrict__ params,
                                                                      float* __restrict__ image, float* __restrict__ sigma,
                                                                      uint8_t* __restrict__ saturated, NoiseArgs a) {
  for (int64_t i = (int64_t)blockIdx.x * NZ_THREADS + threadIdx.x; i < a.total; i += (int64_t)gridDim.x * NZ_THREADS) {
    const double* p = params + (i / a.plane_px) * SUNERF_INSTRUMENT_PARAMS;
    const double unit = p[0], exposure = p[1], g = p[2], read_noise = p[3], pedestal = p[4], saturation = p[5];
    double v = (double)expected[i] * unit;
    v = v < 0.0 ? 0.0 : v;
    const double lam = (v * exposure) / g;
    float img = __uint_as_float(0x7fc00000u), sig = img;
    uint8_t sat = 0;
    if (fabs(lam) <= 4503599627370496.0) {          // finite and <= 2^52 (false for NaN)
      const uint64_t e = (uint64_t)(a.index_offset + i);
      const double n = (a.flags & SUNERF_INSTRUMENT_POISSON) ? poisson(lam, e, a.seed) : lam;
      double dn = n * g + pedestal;
      if (a.flags & SUNERF_INSTRUMENT_READ) {
        const Draw d = draw(e, 0u, 1u, a.seed);
        const double z = sqrt(-2.0 * log(d.ua)) * cos(6.283185307179586 * d.ub);
        dn = dn + read_noise * z;
      }
      if (a.flags & SUNERF_INSTRUMENT_QUANTISE) dn = rint(dn);
      if (a.flags & SUNERF_INSTRUMENT_SATURATE) {
        sat = dn >= saturation ? 1 : 0;
        dn = sat ? saturation : dn;
      }
      img = (float)(((dn - pedestal) / exposure) / unit);
      const double q = (a.flags & SUNERF_INSTRUMENT_QUANTISE) ? 1.0 / 12.0 : 0.0;
      sig = (float)((sqrt((lam * (g * g) + read_noise * read_noise) + q) / exposure) / unit);
    }
    image[i] = img;
    if (sigma) sigma[i] = sig;
    if (saturated) saturated[i] = sat;
  }
}

unsigned grid_of(int64_t work) {
  const int64_t cap = (int64_t)1 << 20;
  return (unsigned)(work < 1 ? 1 : (work < cap ? work : cap));
}

template <bool NEAREST>
void launch_correlate(int nm, dim3 grid, size_t lds, hipStream_t st, const float* in, const double* K, float* out, const CorrArgs& a) {
  switch (nm) {
    case 1: hipLaunchKernelGGL((instrument_correlate_kernel<NEAREST, 1>), grid, dim3(CB_THREADS), lds, st, in, K, out, a); break;
    case 2: hipLaunchKernelGGL((instrument_correlate_kernel<NEAREST, 2>), grid, dim3(CB_THREADS), lds, st, in, K, out, a); break;
    case 3: hipLaunchKernelGGL((instrument_correlate_kernel<NEAREST, 3>), grid, dim3(CB_THREADS), lds, st, in, K, out, a); break;
    default: hipLaunchKernelGGL((instrument_correlate_kernel<NEAREST, 4>), grid, dim3(CB_THREADS), lds, st, in, K, out, a); break;
  }
}

}  // namespace

extern "C" int sunerf_instrument_abi_version(void) { return SUNERF_INSTRUMENT_ABI_VERSION; }

extern "C" int sunerf_instrument_correlate_bin(const float* in, int n_planes, int height, int width, const double* K, int n_kernels,
                                               int kh, int kw, int bin, int anchor_y, int anchor_x, double scale, int boundary,
                                               float* out, void* stream) {
  if (kh > SUNERF_INSTRUMENT_MAX_KERNEL || kw > SUNERF_INSTRUMENT_MAX_KERNEL || bin > SUNERF_INSTRUMENT_MAX_BIN) return SUNERF_E_UNSUPPORTED;
  if (boundary != SUNERF_INSTRUMENT_BOUNDARY_ZERO && boundary != SUNERF_INSTRUMENT_BOUNDARY_NEAREST) return SUNERF_E_UNSUPPORTED;
  const bool bad_count = n_planes < 0 || height < 0 || width < 0 || kh < 1 || kw < 1 || bin < 1;
  if (!bad_count && (n_planes == 0 || height / bin == 0 || width / bin == 0)) return 0;
  if (bad_count || (n_kernels != 1 && n_kernels != n_planes)) return SUNERF_E_BADARG;
  if (anchor_y < 0 || anchor_y >= kh || anchor_x < 0 || anchor_x >= kw) return SUNERF_E_BADARG;
  if (!in || !K || !out || (uintptr_t)K % sizeof(double)) return SUNERF_E_BADARG;
  CorrArgs a;
  a.n_planes = n_planes; a.height = height; a.width = width; a.out_h = height / bin; a.out_w = width / bin;
  a.n_kernels = n_kernels; a.kh = kh; a.kw = kw; a.bin = bin; a.ay = anchor_y; a.ax = anchor_x;
  a.tile = corr_tile(kh, kw, bin);
  a.tiles_y = (a.out_h + a.tile - 1) / a.tile; a.tiles_x = (a.out_w + a.tile - 1) / a.tile;
  a.scale = scale;
  const int lh = (a.tile - 1) * bin + kh, lw = (a.tile - 1) * bin + kw;
  if (lh * lw > CB_MAX_WORDS) return SUNERF_E_UNSUPPORTED;          // cannot happen inside the limits above
  const size_t lds = (size_t)lh * lw * sizeof(float);
  const int nm = (a.tile * a.tile + CB_THREADS - 1) / CB_THREADS;
  const dim3 grid(grid_of((int64_t)a.tiles_y * a.tiles_x * n_planes));
  hipStream_t st = (hipStream_t)stream;
  SUNERF_CLEAR_ERROR();
  if (boundary == SUNERF_INSTRUMENT_BOUNDARY_NEAREST) launch_correlate<true>(nm, grid, lds, st, in, K, out, a);
  else launch_correlate<false>(nm, grid, lds, st, in, K, out, a);
  SUNERF_CHECK_LAUNCH();
  return 0;
}

extern "C" int sunerf_instrument_philox(const uint32_t* ctr, int64_t n, uint32_t key0, uint32_t key1, uint32_t* out, void* stream) {
  if (n == 0) return 0;
  if (n < 0 || !ctr || !out) return SUNERF_E_BADARG;
  SUNERF_CLEAR_ERROR();
  hipLaunchKernelGGL(instrument_philox_kernel, dim3(grid_of((n + PX_THREADS - 1) / PX_THREADS)), dim3(PX_THREADS), 0, (hipStream_t)stream,
                     ctr, n, key0, key1, out);
  SUNERF_CHECK_LAUNCH();
  return 0;
}

extern "C" int sunerf_instrument_noise(const float* expected, int n_planes, int height, int width, const double* params, uint64_t seed,
                                       int64_t index_offset, int flags, float* image, float* sigma, uint8_t* saturated, void* stream) {
  if (flags & ~15) return SUNERF_E_UNSUPPORTED;
  if (n_planes >= 0 && height >= 0 && width >= 0 && (n_planes == 0 || height == 0 || width == 0)) return 0;
  if (n_planes < 0 || height < 0 || width < 0 || index_offset < 0) return SUNERF_E_BADARG;
  if (!expected || !params || !image || (uintptr_t)params % sizeof(double)) return SUNERF_E_BADARG;
  NoiseArgs a;
  a.plane_px = (int64_t)height * width; a.total = a.plane_px * n_planes; a.index_offset = index_offset; a.seed = seed; a.flags = flags;
  SUNERF_CLEAR_ERROR();
  hipLaunchKernelGGL(instrument_noise_kernel, dim3(grid_of((a.total + NZ_THREADS - 1) / NZ_THREADS)), dim3(NZ_THREADS), 0,
                     (hipStream_t)stream, expected, params, image, sigma, saturated, a);
  SUNERF_CHECK_LAUNCH();
  return 0;
}
