// Richardson-Lucy deconvolution of detector images against the instrument's PSF-and-bin kernel (include/sunerf_hip_deconvolve.h,
// DESIGN.md section 8s): the classical baseline beside training through the instrument.  One entry point enqueues, per iteration,
//
// 1. the RATIO kernel: the strided correlation of instrument.hip (same tile rule, LDS staging, boundary handling, taps by scalar
//    load, up to four outputs per thread) whose epilogue keeps the fp64 sum, forms ratio = (d + off) / (A u + off) and the
//    pixel's term of the Poisson deviance, and reduces the terms of the tile in a fixed order (sum64's order inside each
//    wave, then ordered_sum.h's wave-order stage) into ONE partial per tile, indexed by the tile's number: the sum does not depend on
//    the grid;
// 2. the CONTROL kernel: one workgroup per plane adds the plane's partials in a fixed order, writes the plane's state and decides
//    whether the plane stops -- on the device, so that the host never waits between iterations;
// 3. the UPDATE kernel: the gather-form adjoint of patch.hip (same tiles of 32 x 32 input pixels, LDS layout and order of
//    summation) whose epilogue is u' = u * (A^T ratio) / norm, in place: a thread reads and writes only its own pixels of u.
//
// A stopped plane's workgroups return at once from all three.  The loops of the two correlations are corr_bin.h's, shared with
// instrument.hip and patch.hip: the kernels here are their loops over tiles, the stopped-plane test and the epilogues.
// No floating-point atomics; -ffp-contract=off and no explicit fma: every operation is rounded on its own, as the header says.
#include "corr_bin.h"
#include "ordered_sum.h"
#include "../../include/sunerf_hip_deconvolve.h"

namespace {

constexpr int RL_WAVES = CB_THREADS / 64;

__device__ __forceinline__ bool plane_stopped(const double* state, int64_t plane, int pass) {
  return pass > 0 && state[plane * SUNERF_DECONVOLVE_STATE + 3] != 0.0;      // pass 0 finds the state unwritten
}

// ---- ratio ----------------------------------------------------------------------------------------------------------------------
template <bool NEAREST, int NM>
__global__ __launch_bounds__(CB_THREADS) void deconvolve_ratio_kernel(const float* __restrict__ u, const float* __restrict__ d,
                                                                      const uint8_t* __restrict__ bad, const double* __restrict__ params,
                                                                      const double* __restrict__ K, float* __restrict__ ratio,
                                                                      const double* __restrict__ state, double* __restrict__ partials,
                                                                      int pass, CorrBinArgs a) {
  extern __shared__ float tile[];                // [lh][lw]
  __shared__ double wave_sum[2 * RL_WAVES];
  const int t = threadIdx.x;
  const int64_t out_px = (int64_t)a.out_h * a.out_w;
  const int64_t tiles_per_plane = (int64_t)a.tiles_y * a.tiles_x;
  const int64_t n_tiles = tiles_per_plane * a.n_planes;
  for (int64_t tile_id = blockIdx.x; tile_id < n_tiles; tile_id += gridDim.x) {
    const int64_t plane = tile_id / tiles_per_plane;
    if (plane_stopped(state, plane, pass)) continue;          // the whole workgroup: the plane is the tile's
    const int in_plane = (int)(tile_id - plane * tiles_per_plane);
    const int r0 = (in_plane / a.tiles_x) * a.tile, c0 = (in_plane % a.tiles_x) * a.tile;
    corr_stage_tile<NEAREST>(tile, u, a, plane, r0, c0);
    __syncthreads();
    double acc[NM];
    corr_sum_taps<NM>(tile, plane_taps(K, a, plane), a, r0, c0, acc);
    const double c_ph = params[2 * plane], off = params[2 * plane + 1] / c_ph;            // wave-uniform
    double dev = 0.0, count = 0.0;               // the thread's terms, m ascending
#pragma unroll
    for (int m = 0; m < NM; ++m) {
      const CorrOutput o = corr_output(a, r0, c0, m);
      if (o.live) {
        const int64_t px = plane * out_px + (int64_t)(r0 + o.r) * a.out_w + c0 + o.c;
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
    // sum64's order for both values, in ONE loop: two sum64 calls compile to two shuffle chains one after the other, which cost
    // 1 % of an iteration; here a level's shuffles of both values are in flight together
#pragma unroll
    for (int step = 32; step >= 1; step >>= 1) {
      dev = dev + __shfl_xor(dev, step);
      count = count + __shfl_xor(count, step);
    }
    const double totals[2] = {dev, count};
    park_wave_totals(totals, wave_sum);
    __syncthreads();
    if (t == 0) {
      partials[2 * tile_id] = sum_in_wave_order<RL_WAVES, 2>(wave_sum, 0);
      partials[2 * tile_id + 1] = sum_in_wave_order<RL_WAVES, 2>(wave_sum, 1);
    }
    __syncthreads();                             // the tile and the waves' sums are overwritten by the next tile
  }
}

// ---- control --------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(CB_THREADS) void deconvolve_control_kernel(const double* __restrict__ partials, double* __restrict__ state,
                                                                        int64_t tiles_per_plane, double stop, int pass, int last) {
  __shared__ double sum[2 * CB_THREADS];
  const int t = threadIdx.x;
  const int64_t plane = blockIdx.x;
  if (plane_stopped(state, plane, pass)) return;
  const double* p = partials + 2 * plane * tiles_per_plane;
  double s = 0.0, n = 0.0;                       // partials t, t + 256, ... in that order
  for (int64_t i = t; i < tiles_per_plane; i += CB_THREADS) {
    s = s + p[2 * i];
    n = n + p[2 * i + 1];
  }
  const double v[2] = {s, n};
  lds_tree<CB_THREADS>(sum, v, add_values());          // (run once, on an array of its own: no barrier of the caller's)
  if (t == 0) {
    double* st = state + plane * SUNERF_DECONVOLVE_STATE;
    const double deviance = sum[0], n_valid = sum[CB_THREADS];
    double applied = pass > 0 ? st[2] : 0.0;
    const bool stopped = stop > 0.0 && deviance <= stop * n_valid;
    if (!stopped && !last) applied = applied + 1.0;          // the update that follows this pass
    st[0] = deviance; st[1] = n_valid; st[2] = applied; st[3] = stopped ? 1.0 : 0.0;
  }
}

// ---- update ---------------------------------------------------------------------------------------------------------------------
template <bool NEAREST>
__global__ __launch_bounds__(CB_THREADS) void deconvolve_update_kernel(const float* __restrict__ ratio, const double* __restrict__ K,
                                                                       const float* __restrict__ norm, const double* __restrict__ state,
                                                                       float* __restrict__ u, CorrBinArgs a) {
  extern __shared__ __attribute__((aligned(8))) unsigned char lds[];
  const AdjointLds L = adjoint_lds(lds, a);
  const int64_t in_px = (int64_t)a.height * a.width;
  const int64_t tiles_per_plane = (int64_t)a.adj_tiles_y * a.adj_tiles_x;
  const int64_t n_tiles = tiles_per_plane * a.n_planes;
  int64_t staged = -1;
  for (int64_t tile_id = blockIdx.x; tile_id < n_tiles; tile_id += gridDim.x) {
    const int64_t plane = tile_id / tiles_per_plane;
    if (plane_stopped(state, plane, 1)) continue;                     // the control pass before this launch wrote the state
    const int in_plane = (int)(tile_id - plane * tiles_per_plane);
    const int y0 = (in_plane / a.adj_tiles_x) * CB_TILE, x0 = (in_plane % a.adj_tiles_x) * CB_TILE;
    const AdjointSlice s = adjoint_stage_tile(L, ratio, K, a, plane, staged, y0, x0);
    __syncthreads();
    const int x = adjoint_column(x0);
    if (x < a.width) {
      double acc[CB_NM];
      adjoint_sum_tile<NEAREST>(L, s, a, y0, x, acc);
#pragma unroll
      for (int m = 0; m < CB_NM; ++m) {
        const int y = adjoint_row(y0, m);
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

struct RlBuffers {
  float* u; const float* d; const uint8_t* bad; const float* norm; const double* params; const double* K;
  float* ratio; double* state; double* partials;
};

template <bool NEAREST>
void launch_ratio(int nm, dim3 grid, size_t lds, hipStream_t st, const RlBuffers& b, int pass, const CorrBinArgs& a) {
#define RL_RATIO(NM)                                                                                                              \
  hipLaunchKernelGGL((deconvolve_ratio_kernel<NEAREST, NM>), grid, dim3(CB_THREADS), lds, st, (const float*)b.u, b.d, b.bad, b.params, b.K, \
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
int run(const RlBuffers& b, const CorrBinArgs& a, int n_iterations, double stop, hipStream_t st) {
  const size_t ratio_lds = (size_t)corr_tile_words(a) * sizeof(float), update_lds = adjoint_lds_bytes(a);
  const int nm = corr_outputs_per_thread(a);
  const int64_t tiles_per_plane = (int64_t)a.tiles_y * a.tiles_x;
  const dim3 ratio_grid(grid_of(tiles_per_plane * a.n_planes));
  const dim3 update_grid(grid_of((int64_t)a.adj_tiles_y * a.adj_tiles_x * a.n_planes));
  if (n_iterations > 0) {
    const int e = adjoint_lds_opt_in((const void*)deconvolve_update_kernel<NEAREST>, update_lds);
    if (e != 0) return e;
  }
  SUNERF_CLEAR_ERROR();
  for (int pass = 0; pass <= n_iterations; ++pass) {          // pass n_iterations describes the last iterate: no update follows it
    const int last = pass == n_iterations;
    launch_ratio<NEAREST>(nm, ratio_grid, ratio_lds, st, b, pass, a);
    hipLaunchKernelGGL(deconvolve_control_kernel, dim3((unsigned)a.n_planes), dim3(CB_THREADS), 0, st, (const double*)b.partials, b.state,
                       tiles_per_plane, stop, pass, last);
    if (!last)
      hipLaunchKernelGGL(deconvolve_update_kernel<NEAREST>, update_grid, dim3(CB_THREADS), update_lds, st, (const float*)b.ratio, b.K, b.norm,
                         (const double*)b.state, b.u, a);
    SUNERF_CHECK_LAUNCH();
  }
  return 0;
}

}  // namespace

extern "C" int sunerf_deconvolve_abi_version(void) { return SUNERF_DECONVOLVE_ABI_VERSION; }

extern "C" size_t sunerf_deconvolve_workspace_bytes(int n_planes, int height, int width, int kh, int kw, int bin) {
  if (n_planes < 1 || height < 1 || width < 1 || kh < 1 || kw < 1 || bin < 1 || !corr_bin_within_limits(kh, kw, bin)) return 0;
  const CorrBinArgs a = corr_bin_args(n_planes, height, width, 1, kh, kw, bin, 0, 0, 1.0);          // one (deviance, n_valid) pair per ratio tile
  return (size_t)n_planes * ((size_t)a.tiles_y * a.tiles_x) * 2 * sizeof(double);
}

extern "C" int sunerf_deconvolve_richardson_lucy(float* u, const float* d, const uint8_t* bad, const float* norm, const double* params,
                                                 int n_planes, int height, int width, const double* K, int n_kernels, int kh, int kw,
                                                 int bin, int anchor_y, int anchor_x, double scale, int boundary, int n_iterations,
                                                 double stop, float* ratio, double* state, void* workspace, void* stream) {
  bool empty;
  const int status = corr_bin_check(n_planes, height, width, n_kernels, kh, kw, bin, anchor_y, anchor_x, boundary, &empty);
  if (status != 0 || empty) return status;
  if (n_iterations < 0 || n_iterations > SUNERF_DECONVOLVE_MAX_ITERATIONS || !(stop >= 0.0)) return SUNERF_E_BADARG;
  if (!u || !d || !norm || !params || !K || !ratio || !state || !workspace) return SUNERF_E_BADARG;      // the size is non-zero here
  if ((uintptr_t)params % sizeof(double) || (uintptr_t)K % sizeof(double) || (uintptr_t)state % sizeof(double) ||
      (uintptr_t)workspace % sizeof(double))
    return SUNERF_E_BADARG;
  const CorrBinArgs a = corr_bin_args(n_planes, height, width, n_kernels, kh, kw, bin, anchor_y, anchor_x, scale);
  if (corr_tile_words(a) > CB_MAX_WORDS) return SUNERF_E_UNSUPPORTED;          // cannot happen inside the limits above
  const RlBuffers b{u, d, bad, norm, params, K, ratio, state, (double*)workspace};
  hipStream_t st = (hipStream_t)stream;
  if (boundary == SUNERF_INSTRUMENT_BOUNDARY_NEAREST) return run<true>(b, a, n_iterations, stop, st);
  return run<false>(b, a, n_iterations, stop, st);
}
