// Training through the instrument (include/sunerf_hip_patch.h): the adjoint of the PSF-and-bin correlation
// of instrument.hip, and the records of a batch of detector-pixel patches.
//
// 1. Adjoint, gather form.  The tiles, the LDS layout, the four chains per lane and the clamped pixels are corr_bin.h's, which
//    explains them; the kernel here is the loop over tiles and the store.
// 2. Records.  One thread per ray of a window, then one per target element; ray_math.h gives the ray, so a window's rays are
//    the bits sunerf_observer_rays gives for the same angles.
// No floating-point atomics; -ffp-contract=off and no explicit fma: every operation is rounded on its own, as the header says.
#include "corr_bin.h"
#include "ray_math.h"
#include "../../include/sunerf_hip_patch.h"

namespace {

static_assert(sizeof(SunerfPatchViewDesc) == SUNERF_PATCH_VIEW_DESC_BYTES, "the header states the size of a descriptor");

template <bool NEAREST>
__global__ __launch_bounds__(CB_THREADS) void patch_adjoint_kernel(const float* __restrict__ g_out, const double* __restrict__ K,
                                                                   float* __restrict__ g_in, CorrBinArgs a) {
  extern __shared__ __attribute__((aligned(8))) unsigned char lds[];
  const AdjointLds L = adjoint_lds(lds, a);
  const int64_t in_px = (int64_t)a.height * a.width;
  const int64_t tiles_per_plane = (int64_t)a.adj_tiles_y * a.adj_tiles_x;
  const int64_t n_tiles = tiles_per_plane * a.n_planes;
  int64_t staged = -1;                                                // the kernel in L.taps
  for (int64_t tile_id = blockIdx.x; tile_id < n_tiles; tile_id += gridDim.x) {
    const int64_t plane = tile_id / tiles_per_plane;
    const int in_plane = (int)(tile_id - plane * tiles_per_plane);
    const int y0 = (in_plane / a.adj_tiles_x) * CB_TILE, x0 = (in_plane % a.adj_tiles_x) * CB_TILE;
    const AdjointSlice s = adjoint_stage_tile(L, g_out, K, a, plane, staged, y0, x0);
    __syncthreads();
    const int x = adjoint_column(x0);
    if (x < a.width) {
      double acc[CB_NM];
      adjoint_sum_tile<NEAREST>(L, s, a, y0, x, acc);
#pragma unroll
      for (int m = 0; m < CB_NM; ++m) {
        const int y = adjoint_row(y0, m);
        if (y < a.height) g_in[plane * in_px + (int64_t)y * a.width + x] = (float)(a.scale * acc[m]);
      }
    }
    __syncthreads();                             // the slice (and a per-plane kernel) is overwritten by the next tile
  }
}

// ---- records --------------------------------------------------------------------------------------------------------------------
constexpr int PR_THREADS = 256;

struct RecArgs {
  const SunerfPatchViewDesc* views; int n_views;
  const int32_t* patches; int n_patches;
  int C, P, bin, hw, ww;
  float* rays; float* time; float* target; float* wavelength;
};

// the view of patch k if the patch lies inside it, else NULL
__device__ __forceinline__ const SunerfPatchViewDesc* patch_view(const RecArgs& a, int k, int& R0, int& C0) {
  const int v = a.patches[3 * k];
  R0 = a.patches[3 * k + 1]; C0 = a.patches[3 * k + 2];
  if (v < 0 || v >= a.n_views) return nullptr;
  const SunerfPatchViewDesc* view = a.views + v;
  if (R0 < 0 || C0 < 0 || R0 > view->height - a.P || C0 > view->width - a.P) return nullptr;
  return view;
}

__global__ __launch_bounds__(PR_THREADS) void patch_records_kernel(RecArgs a) {
  const int64_t stride = (int64_t)gridDim.x * PR_THREADS, first = (int64_t)blockIdx.x * PR_THREADS + threadIdx.x;
  const int64_t window = (int64_t)a.hw * a.ww, n_rays = window * a.n_patches;
  for (int64_t r = first; r < n_rays; r += stride) {
    const int k = (int)(r / window);
    const int in_window = (int)(r - k * window);
    const int wy = in_window / a.ww, wx = in_window - wy * a.ww;
    int R0, C0;
    const SunerfPatchViewDesc* v = patch_view(a, k, R0, C0);
    float o[3] = {0.f, 0.f, 0.f}, d[3] = {0.f, 0.f, 0.f}, time = 0.f;
    if (v) {
      sunerf_pixel_ray(v->tx[(int64_t)C0 * a.bin + wx], v->ty[(int64_t)R0 * a.bin + wy], v->c2w, o, d);
      time = v->time;
    }
#pragma unroll
    for (int e = 0; e < 3; ++e) { a.rays[r * 6 + e] = o[e]; a.rays[r * 6 + 3 + e] = d[e]; }
    a.time[r] = time;
    if (a.wavelength)
      for (int c = 0; c < a.C; ++c) {
        const int pl = v ? v->plane[c] : -1;
        a.wavelength[r * a.C + c] = (pl >= 0 && pl < v->n_planes) ? v->wavelength[c] : 0.f;
      }
  }
  const int64_t pp = (int64_t)a.P * a.P, n_targets = pp * a.C * a.n_patches;
  for (int64_t e = first; e < n_targets; e += stride) {
    const int k = (int)(e / (pp * a.C));
    const int rest = (int)(e - k * pp * a.C);
    const int c = rest / (int)pp, px = rest - c * (int)pp;
    const int py = px / a.P;
    int R0, C0;
    const SunerfPatchViewDesc* v = patch_view(a, k, R0, C0);
    const int pl = v ? v->plane[c] : -1;
    float value = 0.f;
    if (pl >= 0 && pl < v->n_planes)
      value = v->image[((int64_t)pl * v->height + R0 + py) * v->width + C0 + (px - py * a.P)];
    a.target[e] = value;
  }
}

template <bool NEAREST>
int launch_adjoint(dim3 grid, size_t lds_bytes, hipStream_t st, const float* g_out, const double* K, float* g_in, const CorrBinArgs& a) {
  const int e = adjoint_lds_opt_in((const void*)patch_adjoint_kernel<NEAREST>, lds_bytes);
  if (e != 0) return e;
  SUNERF_CLEAR_ERROR();
  hipLaunchKernelGGL(patch_adjoint_kernel<NEAREST>, grid, dim3(CB_THREADS), lds_bytes, st, g_out, K, g_in, a);
  SUNERF_CHECK_LAUNCH();
  return 0;
}

}  // namespace

extern "C" int sunerf_patch_abi_version(void) { return SUNERF_PATCH_ABI_VERSION; }

extern "C" int sunerf_patch_correlate_bin_adjoint(const float* g_out, int n_planes, int height, int width, const double* K, int n_kernels,
                                                  int kh, int kw, int bin, int anchor_y, int anchor_x, double scale, int boundary,
                                                  float* g_in, void* stream) {
  bool empty;
  const int status = corr_bin_check(n_planes, height, width, n_kernels, kh, kw, bin, anchor_y, anchor_x, boundary, &empty);
  if (status != 0 || empty) return status;
  if (!g_out || !K || !g_in || (uintptr_t)K % sizeof(double)) return SUNERF_E_BADARG;
  const CorrBinArgs a = corr_bin_args(n_planes, height, width, n_kernels, kh, kw, bin, anchor_y, anchor_x, scale);
  const size_t lds_bytes = adjoint_lds_bytes(a);
  const dim3 grid(grid_of((int64_t)a.adj_tiles_y * a.adj_tiles_x * n_planes));
  hipStream_t st = (hipStream_t)stream;
  if (boundary == SUNERF_INSTRUMENT_BOUNDARY_NEAREST) return launch_adjoint<true>(grid, lds_bytes, st, g_out, K, g_in, a);
  return launch_adjoint<false>(grid, lds_bytes, st, g_out, K, g_in, a);
}

extern "C" int sunerf_patch_records(const SunerfPatchViewDesc* views, int n_views, const int32_t* patches, int n_patches, int n_channels,
                                    int P, int bin, int kh, int kw, float* rays, float* time, float* target, float* wavelength,
                                    void* stream) {
  if (!corr_bin_within_limits(kh, kw, bin)) return SUNERF_E_UNSUPPORTED;
  const bool bad_count = n_patches < 0 || P < 1 || bin < 1 || kh < 1 || kw < 1;
  if (!bad_count && n_patches == 0) return 0;
  if (bad_count || n_views < 1 || n_channels < 1 || n_channels > SUNERF_OBS_MAX_CHANNELS) return SUNERF_E_BADARG;
  const int64_t hw = (int64_t)(P - 1) * bin + kh, ww = (int64_t)(P - 1) * bin + kw;
  if (hw > 0x7fffffff || ww > 0x7fffffff || hw * ww > 0x7fffffff / n_patches) return SUNERF_E_BADARG;
  if ((int64_t)P * P > 0x7fffffff / ((int64_t)n_patches * n_channels)) return SUNERF_E_BADARG;
  if (!views || !patches || !rays || !time || !target) return SUNERF_E_BADARG;
  RecArgs a;
  a.views = views; a.n_views = n_views; a.patches = patches; a.n_patches = n_patches;
  a.C = n_channels; a.P = P; a.bin = bin; a.hw = (int)hw; a.ww = (int)ww;
  a.rays = rays; a.time = time; a.target = target; a.wavelength = wavelength;
  const int64_t n_rays = hw * ww * n_patches;
  SUNERF_CLEAR_ERROR();
  hipLaunchKernelGGL(patch_records_kernel, dim3(grid_of((n_rays + PR_THREADS - 1) / PR_THREADS)), dim3(PR_THREADS), 0,
                     (hipStream_t)stream, a);
  SUNERF_CHECK_LAUNCH();
  return 0;
}
