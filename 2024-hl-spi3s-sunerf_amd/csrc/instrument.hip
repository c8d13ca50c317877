// A rendered frame becomes a detector image: strided correlation with the PSF-and-bin kernel, photon and read noise,
// digitisation, saturation (include/sunerf_hip_instrument.h).
//
// 1. Correlation.  The tile rule, the staging under the boundary rule and the tap loop are corr_bin.h's, which explains them; the
//    kernel here is the loop over tiles and the store.
// 2. Noise.  One thread per element; the generator is Philox4x32-10 keyed by the seed and counted by the element's index, so the
//    value of an element does not depend on the launch geometry, on its neighbours or on how a frame is cut into calls.
// No floating-point atomics; -ffp-contract=off and no explicit fma: every operation is rounded on its own, as the header says.
#include "corr_bin.h"
#include "../../include/sunerf_hip_instrument.h"

namespace {

template <bool NEAREST, int NM>
__global__ __launch_bounds__(CB_THREADS) void instrument_correlate_kernel(const float* __restrict__ in, const double* __restrict__ K,
                                                                          float* __restrict__ out, CorrBinArgs a) {
  extern __shared__ float tile[];                // [lh][lw]
  const int64_t out_px = (int64_t)a.out_h * a.out_w;
  const int64_t tiles_per_plane = (int64_t)a.tiles_y * a.tiles_x;
  const int64_t n_tiles = tiles_per_plane * a.n_planes;
  for (int64_t tile_id = blockIdx.x; tile_id < n_tiles; tile_id += gridDim.x) {
    const int64_t plane = tile_id / tiles_per_plane;
    const int in_plane = (int)(tile_id - plane * tiles_per_plane);
    const int r0 = (in_plane / a.tiles_x) * a.tile, c0 = (in_plane % a.tiles_x) * a.tile;      // first output pixel of the tile
    corr_stage_tile<NEAREST>(tile, in, a, plane, r0, c0);
    __syncthreads();
    double acc[NM];
    corr_sum_taps<NM>(tile, plane_taps(K, a, plane), a, r0, c0, acc);
#pragma unroll
    for (int m = 0; m < NM; ++m) {
      const CorrOutput o = corr_output(a, r0, c0, m);
      if (o.live) out[plane * out_px + (int64_t)(r0 + o.r) * a.out_w + c0 + o.c] = (float)(a.scale * acc[m]);
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

template <bool NEAREST>
void launch_correlate(int nm, dim3 grid, size_t lds, hipStream_t st, const float* in, const double* K, float* out, const CorrBinArgs& a) {
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
  bool empty;
  const int status = corr_bin_check(n_planes, height, width, n_kernels, kh, kw, bin, anchor_y, anchor_x, boundary, &empty);
  if (status != 0 || empty) return status;
  if (!in || !K || !out || (uintptr_t)K % sizeof(double)) return SUNERF_E_BADARG;
  const CorrBinArgs a = corr_bin_args(n_planes, height, width, n_kernels, kh, kw, bin, anchor_y, anchor_x, scale);
  if (corr_tile_words(a) > CB_MAX_WORDS) return SUNERF_E_UNSUPPORTED;          // cannot happen inside the limits above
  const size_t lds = (size_t)corr_tile_words(a) * sizeof(float);
  const int nm = corr_outputs_per_thread(a);
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
