// Training through the instrument (include/sunerf_hip_patch.h): the adjoint of the PSF-and-bin correlation
// of instrument.hip, and the records of a batch of detector-pixel patches.
//
// 1. Adjoint, gather form.  A workgroup takes a tile of T x T INPUT pixels of one plane (T = 32); a thread owns four of them (column
//    t % 32, rows t / 32 + 8 m) and sums, in the header's order, every term K[i][j] * g_out[R][C] whose forward tap read its pixel.
//    For a pixel that no tap was clamped onto, row i of the kernel meets row y only through R = (y + ay - i) / bin, so only the
//    rows i = (y + ay) mod bin, + bin, + 2 bin, ... contribute, one R each (R falls by one per step), and likewise the columns:
//    the loops step by bin instead of testing every tap, and the four pixels of a thread, which share their column, walk one
//    column range side by side -- four independent chains of fp64 adds per lane.  A pixel on an edge under BOUNDARY_NEAREST also
//    collects the taps that were clamped onto it: it is summed on its own, every tap walked and R, C running over ranges.  The
//    tap index depends on the lane (through y, x mod bin and through the edge rule), so K cannot come from scalar loads as in the
//    forward: the plane's kernel is staged in LDS (fp64, regrouped by j mod bin so that a pixel's taps lie side by side) beside
//    the slice of g_out that the tile's taps reach (fp32).  Every range lies inside that slice by construction; the loops clamp
//    to it all the same, so no LDS address depends on that argument.
// 2. Records.  One thread per ray of a window, then one per target element; ray_math.h gives the ray, so a window's rays are
//    the bits sunerf_observer_rays gives for the same angles.
// No floating-point atomics; -ffp-contract=off and no explicit fma: every operation is rounded on its own, as the header says.
#include "sunerf_common.h"
#include "ray_math.h"
#include "../../include/sunerf_hip_patch.h"

namespace {

constexpr int PA_THREADS = 256;
constexpr int PA_TILE = SUNERF_PATCH_TILE;
constexpr int PA_NM = PA_TILE * PA_TILE / PA_THREADS;      // pixels per thread

static_assert(PA_TILE * PA_TILE == PA_NM * PA_THREADS, "whole pixels per thread");
static_assert(PA_TILE + SUNERF_INSTRUMENT_MAX_KERNEL - 1 == 127, "the largest slice is 127 words wide");
static_assert(sizeof(SunerfPatchViewDesc) == SUNERF_PATCH_VIEW_DESC_BYTES, "the header states the size of a descriptor");

// LDS pointers carry their address space in their type: a pointer chosen between two LDS rows stays an LDS pointer (ds_read), where
// a plain pointer falls back to flat loads
typedef __attribute__((address_space(3))) double LdsF64;
typedef __attribute__((address_space(3))) float LdsF32;

struct AdjArgs {
  int n_planes, height, width, out_h, out_w;
  int n_kernels, kh, kw, bin, ay, ax;
  int tiles_y, tiles_x;
  double scale;
};

__host__ __device__ __forceinline__ int floor_div(int a, int b) {      // b > 0
  const int q = a / b;
  return (a % b != 0 && a < 0) ? q - 1 : q;
}
__host__ __device__ __forceinline__ int ceil_div(int a, int b) { return -floor_div(-a, b); }

// LDS word of tap (i, j): the row's taps are grouped by j mod bin, so that the taps one pixel meets (j = j0, j0 + bin, ...) lie side
// by side and the inner loop walks both of its operands by constant steps
__device__ __forceinline__ int tap_word(int i, int j, int bin, int kwb) { return (i * bin + j % bin) * kwb + j / bin; }

// Every term of one pixel that taps were clamped onto (BOUNDARY_NEAREST, a pixel on the edge).  Row i of the kernel meets the pixel
// through the detector rows ceil((y + ay - i) / bin) .. floor(same): one row, or none, inside the plane; 0 .. floor on row 0 and
// ceil .. H / bin - 1 on the last row, where the clamped taps gather.  Quotient and remainder of (y + ay - i) / bin are carried
// from tap to tap (no division in the loops), and so is the LDS word of the tap.
__device__ __forceinline__ double adjoint_pixel_clamped(const LdsF64* taps, const LdsF32* slice, const AdjArgs& a, int kwb, int y, int x, int r_lo,
                                        int r_hi, int c_lo, int c_hi) {
  const int bin = a.bin, n_c = c_hi - c_lo + 1;
  const bool top = y == 0, bottom = y == a.height - 1, left = x == 0, right = x == a.width - 1;
  const int ty = y + a.ay, tx = x + a.ax;
  double acc = 0.0;
  int qy = ty / bin, ry = ty - qy * bin;          // ty - i = qy bin + ry, 0 <= ry < bin
  for (int i = 0; i < a.kh; ++i) {
    int ra = top ? 0 : qy + (ry > 0), rb = bottom ? a.out_h - 1 : qy;
    ra = ra < r_lo ? r_lo : ra; rb = rb > r_hi ? r_hi : rb;
    if (ra <= rb) {
      int qx = tx / bin, rx = tx - qx * bin;
      int word = i * bin * kwb, jm = 0;           // tap_word(i, j): j = jd bin + jm, word = (i bin + jm) kwb + jd
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
__global__ __launch_bounds__(PA_THREADS) void patch_adjoint_kernel(const float* __restrict__ g_out, const double* __restrict__ K,
                                                                   float* __restrict__ g_in, AdjArgs a) {
  extern __shared__ __attribute__((aligned(8))) unsigned char lds[];
  const int bin = a.bin;
  const int kwb = (a.kw + bin - 1) / bin;                             // taps of a row that one pixel can meet, at most
  const int sw = (PA_TILE + a.kw - 2) / bin + 1;                      // columns of the largest slice
  LdsF64* taps = (LdsF64*)lds;                                        // [kh][bin][kwb]: tap_word
  LdsF64* zero_taps = taps + a.kh * bin * kwb;                        // [kwb] of 0.0
  LdsF32* zero_row = (LdsF32*)(zero_taps + kwb);                      // [sw] of 0.f
  LdsF32* slice = zero_row + sw;                                      // [n_r][n_c] of the tile at hand
  const int t = threadIdx.x;
  const int lx = t % PA_TILE, ly = t / PA_TILE;                       // the thread's pixels: column lx, rows ly + 8 m
  for (int i = t; i < kwb; i += PA_THREADS) zero_taps[i] = 0.0;
  for (int i = t; i < sw; i += PA_THREADS) zero_row[i] = 0.f;
  const int64_t in_px = (int64_t)a.height * a.width, out_px = (int64_t)a.out_h * a.out_w;
  const int64_t tiles_per_plane = (int64_t)a.tiles_y * a.tiles_x;
  const int64_t n_tiles = tiles_per_plane * a.n_planes;
  int64_t staged = -1;                                                // the kernel in `taps`
  for (int64_t tile_id = blockIdx.x; tile_id < n_tiles; tile_id += gridDim.x) {
    const int64_t plane = tile_id / tiles_per_plane;
    const int in_plane = (int)(tile_id - plane * tiles_per_plane);
    const int y0 = (in_plane / a.tiles_x) * PA_TILE, x0 = (in_plane % a.tiles_x) * PA_TILE;
    const int y_last = (y0 + PA_TILE < a.height ? y0 + PA_TILE : a.height) - 1;
    const int x_last = (x0 + PA_TILE < a.width ? x0 + PA_TILE : a.width) - 1;
    // the detector pixels whose taps reach the tile: R bin in [y0 + ay - (kh - 1), y_last + ay]
    int r_lo = ceil_div(y0 + a.ay - (a.kh - 1), bin), r_hi = floor_div(y_last + a.ay, bin);
    int c_lo = ceil_div(x0 + a.ax - (a.kw - 1), bin), c_hi = floor_div(x_last + a.ax, bin);
    r_lo = r_lo < 0 ? 0 : r_lo; r_hi = r_hi > a.out_h - 1 ? a.out_h - 1 : r_hi;
    c_lo = c_lo < 0 ? 0 : c_lo; c_hi = c_hi > a.out_w - 1 ? a.out_w - 1 : c_hi;
    const int n_r = r_hi - r_lo + 1, n_c = c_hi - c_lo + 1;           // either may be <= 0: no tap reaches the tile
    const int64_t kernel = a.n_kernels == 1 ? (int64_t)0 : plane;
    if (kernel != staged) {
      const double* src = K + kernel * a.kh * a.kw;
      for (int i = t; i < a.kh * a.kw; i += PA_THREADS) taps[tap_word(i / a.kw, i % a.kw, bin, kwb)] = src[i];
      staged = kernel;
    }
    if (n_r > 0 && n_c > 0) {
      const float* src = g_out + plane * out_px;
      for (int i = t; i < n_r * n_c; i += PA_THREADS) {
        const int r = i / n_c;
        slice[i] = src[(int64_t)(r_lo + r) * a.out_w + c_lo + (i - r * n_c)];
      }
    }
    __syncthreads();
    const int x = x0 + lx;
    if (x < a.width) {
      double acc[PA_NM];
      bool clamped[PA_NM];                                            // a pixel that taps were clamped onto: on the edge under NEAREST
#pragma unroll
      for (int m = 0; m < PA_NM; ++m) {
        const int y = y0 + ly + (PA_THREADS / PA_TILE) * m;
        acc[m] = 0.0;
        clamped[m] = NEAREST && y < a.height && (x == 0 || x == a.width - 1 || y == 0 || y == a.height - 1);
      }
      if (n_r > 0 && n_c > 0) {
        {
          // The pixels that no tap was clamped onto.  The thread's pixels share their column, so the taps j = j0 + b bin they meet and the detector columns C0 - b are
          // theirs in common: b runs over one range.  Step s of the rows takes tap row i0 + s bin and detector row R0 - s of
          // each pixel; a pixel for which that step does not exist reads rows of zeros instead -- its sum takes + 0.0 * 0.0, which
          // changes no sum that began at +0.0 (such a sum is never -0.0) -- so the four chains run side by side, unpredicated.
          const int tx = x + a.ax, j0 = tx % bin, C0 = tx / bin;
          const int b_min = C0 - c_hi > 0 ? C0 - c_hi : 0;
          int b_max = j0 < a.kw ? (a.kw - 1 - j0) / bin : -1;
          b_max = b_max < C0 - c_lo ? b_max : C0 - c_lo;
          int i0[PA_NM], R0[PA_NM], s_min[PA_NM], s_max[PA_NM];
          int s_begin = 0x7fffffff, s_end = -1;
#pragma unroll
          for (int m = 0; m < PA_NM; ++m) {
            const int y = y0 + ly + (PA_THREADS / PA_TILE) * m;
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
            const LdsF64* kq[PA_NM];
            const LdsF32* gq[PA_NM];
#pragma unroll
            for (int m = 0; m < PA_NM; ++m) {
              const bool live = s >= s_min[m] && s <= s_max[m];
              kq[m] = live ? taps + ((i0[m] + s * bin) * bin + j0) * kwb : zero_taps;
              gq[m] = live ? slice + (R0[m] - s - r_lo) * n_c + (C0 - c_lo) : zero_row + (sw - 1);
            }
#pragma unroll 4
            for (int b = b_min; b <= b_max; ++b) {
#pragma unroll
              for (int m = 0; m < PA_NM; ++m) acc[m] = acc[m] + kq[m][b] * (double)gq[m][-b];
            }
          }
        }
        if (NEAREST) {
#pragma unroll 1
          for (int m = 0; m < PA_NM; ++m) {
            const int y = y0 + ly + (PA_THREADS / PA_TILE) * m;
            if (clamped[m]) acc[m] = adjoint_pixel_clamped(taps, slice, a, kwb, y, x, r_lo, r_hi, c_lo, c_hi);
          }
        }
      }
#pragma unroll
      for (int m = 0; m < PA_NM; ++m) {
        const int y = y0 + ly + (PA_THREADS / PA_TILE) * m;
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

unsigned grid_of(int64_t work) {
  const int64_t cap = (int64_t)1 << 20;
  return (unsigned)(work < 1 ? 1 : (work < cap ? work : cap));
}

template <bool NEAREST>
int launch_adjoint(dim3 grid, size_t lds_bytes, hipStream_t st, const float* g_out, const double* K, float* g_in, const AdjArgs& a) {
  if (lds_bytes > 64 * 1024) {
    hipError_t e = hipFuncSetAttribute((const void*)patch_adjoint_kernel<NEAREST>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_bytes);
    if (e != hipSuccess) return (int)e;
  }
  SUNERF_CLEAR_ERROR();
  hipLaunchKernelGGL(patch_adjoint_kernel<NEAREST>, grid, dim3(PA_THREADS), lds_bytes, st, g_out, K, g_in, a);
  SUNERF_CHECK_LAUNCH();
  return 0;
}

}  // namespace

extern "C" int sunerf_patch_abi_version(void) { return SUNERF_PATCH_ABI_VERSION; }

extern "C" int sunerf_patch_correlate_bin_adjoint(const float* g_out, int n_planes, int height, int width, const double* K, int n_kernels,
                                                  int kh, int kw, int bin, int anchor_y, int anchor_x, double scale, int boundary,
                                                  float* g_in, void* stream) {
  if (kh > SUNERF_INSTRUMENT_MAX_KERNEL || kw > SUNERF_INSTRUMENT_MAX_KERNEL || bin > SUNERF_INSTRUMENT_MAX_BIN) return SUNERF_E_UNSUPPORTED;
  if (boundary != SUNERF_INSTRUMENT_BOUNDARY_ZERO && boundary != SUNERF_INSTRUMENT_BOUNDARY_NEAREST) return SUNERF_E_UNSUPPORTED;
  const bool bad_count = n_planes < 0 || height < 0 || width < 0 || kh < 1 || kw < 1 || bin < 1;
  if (!bad_count && (n_planes == 0 || height / bin == 0 || width / bin == 0)) return 0;
  if (bad_count || (n_kernels != 1 && n_kernels != n_planes)) return SUNERF_E_BADARG;
  if (anchor_y < 0 || anchor_y >= kh || anchor_x < 0 || anchor_x >= kw) return SUNERF_E_BADARG;
  if (!g_out || !K || !g_in || (uintptr_t)K % sizeof(double)) return SUNERF_E_BADARG;
  AdjArgs a;
  a.n_planes = n_planes; a.height = height; a.width = width; a.out_h = height / bin; a.out_w = width / bin;
  a.n_kernels = n_kernels; a.kh = kh; a.kw = kw; a.bin = bin; a.ay = anchor_y; a.ax = anchor_x;
  a.tiles_y = (height + PA_TILE - 1) / PA_TILE; a.tiles_x = (width + PA_TILE - 1) / PA_TILE;
  a.scale = scale;
  const int sh = (PA_TILE + kh - 2) / bin + 1, sw = (PA_TILE + kw - 2) / bin + 1;      // rows and columns of the largest slice
  const int kwb = (kw + bin - 1) / bin;
  const size_t lds_bytes = ((size_t)kh * bin * kwb + kwb) * sizeof(double) + ((size_t)sh * sw + sw) * sizeof(float);
  const dim3 grid(grid_of((int64_t)a.tiles_y * a.tiles_x * n_planes));
  hipStream_t st = (hipStream_t)stream;
  if (boundary == SUNERF_INSTRUMENT_BOUNDARY_NEAREST) return launch_adjoint<true>(grid, lds_bytes, st, g_out, K, g_in, a);
  return launch_adjoint<false>(grid, lds_bytes, st, g_out, K, g_in, a);
}

extern "C" int sunerf_patch_records(const SunerfPatchViewDesc* views, int n_views, const int32_t* patches, int n_patches, int n_channels,
                                    int P, int bin, int kh, int kw, float* rays, float* time, float* target, float* wavelength,
                                    void* stream) {
  if (kh > SUNERF_INSTRUMENT_MAX_KERNEL || kw > SUNERF_INSTRUMENT_MAX_KERNEL || bin > SUNERF_INSTRUMENT_MAX_BIN) return SUNERF_E_UNSUPPORTED;
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
