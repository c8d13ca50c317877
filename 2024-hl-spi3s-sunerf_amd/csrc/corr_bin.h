// The PSF-and-bin correlation and its adjoint, once (DESIGN.md sections 8o, 8p, 8s): the geometry, the argument check and the device
// loops shared by instrument.hip (the correlation), patch.hip (its adjoint) and deconvolve.hip (Richardson-Lucy on top of both).  A
// kernel of those files keeps its loop over tiles and its epilogue; what it sums, and in which order, is written here.
//
// 1. Correlation.  A workgroup takes a tile of T x T detector pixels of one plane, T = min(32, (127 - max(kh, kw)) / bin + 1):
//    all 256 threads stage the input tile with its halo, ((T - 1) bin + kh) x ((T - 1) bin + kw) fp32 words (at most 127 x 127 =
//    63 KiB), in LDS -- the boundary rule is applied there, once per staged word -- and every thread then owns up to four output
//    pixels (output t + 256 m of the tile, row-major) and walks the taps in the header's order, row by row.  The tap K[i][j] is
//    the same for every lane: its address is built from blockIdx and the loop counters only, so it is fetched by a scalar load
//    into SGPRs, once per wave, and the inner loop is one LDS read, one convert, one fp64 multiply and one fp64 add per output.
// 2. Adjoint, gather form.  A workgroup takes a tile of T x T INPUT pixels of one plane (T = 32); a thread owns four of them (column
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
// 3. Tap gradient (psf_grad.hip).  It takes the correlation's tiles, its argument check and corr_stage_tile from
//    here and keeps its own loop (threads own taps, not outputs) in its file.
// No floating-point atomics; -ffp-contract=off and no explicit fma: every operation is rounded on its own, as the headers say.
#pragma once
#include "sunerf_common.h"
#include "../../include/sunerf_hip_patch.h"      // SUNERF_PATCH_TILE; it includes sunerf_hip_instrument.h: the limits, the boundaries

constexpr int CB_THREADS = 256;
constexpr int CB_MAX_WORDS = 127 * 127;        // LDS words of the largest input tile of the correlation
constexpr int CB_TILE = SUNERF_PATCH_TILE;     // input pixels per side of a tile of the adjoint
constexpr int CB_NM = CB_TILE * CB_TILE / CB_THREADS;      // pixels per thread of the adjoint

static_assert(SUNERF_INSTRUMENT_TILE * SUNERF_INSTRUMENT_TILE == 4 * CB_THREADS, "four outputs per thread at most");
static_assert(SUNERF_INSTRUMENT_TILE - 1 + SUNERF_INSTRUMENT_MAX_KERNEL == 127, "the largest tile is 127 words wide");
static_assert(CB_TILE + SUNERF_INSTRUMENT_MAX_KERNEL - 1 == 127, "the largest slice is 127 words wide");
static_assert(CB_TILE * CB_TILE == CB_NM * CB_THREADS, "whole pixels per thread");

// LDS pointers carry their address space in their type: a pointer chosen between two LDS rows stays an LDS pointer (ds_read), where
// a plain pointer falls back to flat loads
typedef __attribute__((address_space(3))) double LdsF64;
typedef __attribute__((address_space(3))) float LdsF32;

struct CorrBinArgs {
  int n_planes, height, width, out_h, out_w;
  int n_kernels, kh, kw, bin, ay, ax;
  int tile, tiles_y, tiles_x;          // the correlation's tiles of detector pixels
  int adj_tiles_y, adj_tiles_x;        // the adjoint's tiles of input pixels
  double scale;
};

// ---- host -----------------------------------------------------------------------------------------------------------------------
static inline int corr_tile(int kh, int kw, int bin) {
  const int k = kh > kw ? kh : kw;
  const int t = (127 - k) / bin + 1;
  return t < SUNERF_INSTRUMENT_TILE ? t : SUNERF_INSTRUMENT_TILE;
}

static inline bool corr_bin_within_limits(int kh, int kw, int bin) {
  return kh <= SUNERF_INSTRUMENT_MAX_KERNEL && kw <= SUNERF_INSTRUMENT_MAX_KERNEL && bin <= SUNERF_INSTRUMENT_MAX_BIN;
}

// The check the four entry points share, in the order their headers state: limits and an unknown boundary, then the empty call
// (*empty is set: the caller returns 0), then counts, n_kernels and anchors.  The caller's own checks follow a 0 with *empty false.
// `any_divisor`: n_kernels may be any divisor of n_planes (psf_grad.hip: plane p takes kernel p % n_kernels), not 1 or n_planes only.
static inline int corr_bin_check(int n_planes, int height, int width, int n_kernels, int kh, int kw, int bin, int anchor_y, int anchor_x,
                                 int boundary, bool* empty, bool any_divisor = false) {
  *empty = false;
  if (!corr_bin_within_limits(kh, kw, bin)) return SUNERF_E_UNSUPPORTED;
  if (boundary != SUNERF_INSTRUMENT_BOUNDARY_ZERO && boundary != SUNERF_INSTRUMENT_BOUNDARY_NEAREST) return SUNERF_E_UNSUPPORTED;
  const bool bad_count = n_planes < 0 || height < 0 || width < 0 || kh < 1 || kw < 1 || bin < 1;
  if (!bad_count && (n_planes == 0 || height / bin == 0 || width / bin == 0)) {
    *empty = true;
    return 0;
  }
  if (bad_count) return SUNERF_E_BADARG;
  if (any_divisor ? (n_kernels < 1 || n_planes % n_kernels != 0) : (n_kernels != 1 && n_kernels != n_planes)) return SUNERF_E_BADARG;
  if (anchor_y < 0 || anchor_y >= kh || anchor_x < 0 || anchor_x >= kw) return SUNERF_E_BADARG;
  return 0;
}

static inline CorrBinArgs corr_bin_args(int n_planes, int height, int width, int n_kernels, int kh, int kw, int bin, int anchor_y,
                                        int anchor_x, double scale) {
  CorrBinArgs a;
  a.n_planes = n_planes; a.height = height; a.width = width; a.out_h = height / bin; a.out_w = width / bin;
  a.n_kernels = n_kernels; a.kh = kh; a.kw = kw; a.bin = bin; a.ay = anchor_y; a.ax = anchor_x;
  a.tile = corr_tile(kh, kw, bin);
  a.tiles_y = (a.out_h + a.tile - 1) / a.tile; a.tiles_x = (a.out_w + a.tile - 1) / a.tile;
  a.adj_tiles_y = (height + CB_TILE - 1) / CB_TILE; a.adj_tiles_x = (width + CB_TILE - 1) / CB_TILE;
  a.scale = scale;
  return a;
}

// LDS words of the correlation's input tile: at most CB_MAX_WORDS inside the limits
static inline int corr_tile_words(const CorrBinArgs& a) { return ((a.tile - 1) * a.bin + a.kh) * ((a.tile - 1) * a.bin + a.kw); }
// outputs per thread of the correlation: the NM its kernels are compiled for
static inline int corr_outputs_per_thread(const CorrBinArgs& a) { return (a.tile * a.tile + CB_THREADS - 1) / CB_THREADS; }

// LDS bytes of the adjoint: the kernel regrouped, a row of zero taps, a row of zeros and the largest slice
static inline size_t adjoint_lds_bytes(const CorrBinArgs& a) {
  const int sh = (CB_TILE + a.kh - 2) / a.bin + 1, sw = (CB_TILE + a.kw - 2) / a.bin + 1;      // rows and columns of the largest slice
  const int kwb = (a.kw + a.bin - 1) / a.bin;
  return ((size_t)a.kh * a.bin * kwb + kwb) * sizeof(double) + ((size_t)sh * sw + sw) * sizeof(float);
}

// above 64 KiB of dynamic LDS a kernel has to be opted in
static inline int adjoint_lds_opt_in(const void* kernel, size_t lds_bytes) {
  if (lds_bytes > 64 * 1024) {
    hipError_t e = hipFuncSetAttribute(kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_bytes);
    if (e != hipSuccess) return (int)e;
  }
  return 0;
}

// ---- correlation ----------------------------------------------------------------------------------------------------------------
// the taps of a plane: wave-uniform
__device__ __forceinline__ const double* plane_taps(const double* K, const CorrBinArgs& a, int64_t plane) {
  return K + (a.n_kernels == 1 ? (int64_t)0 : plane) * a.kh * a.kw;
}

// Stages the input tile [lh][lw] of the outputs from (r0, c0) on, halo included, under the boundary rule.  A barrier follows.
template <bool NEAREST>
__device__ __forceinline__ void corr_stage_tile(float* tile, const float* in, const CorrBinArgs& a, int64_t plane, int r0, int c0) {
  const int lh = (a.tile - 1) * a.bin + a.kh, lw = (a.tile - 1) * a.bin + a.kw;
  const int y0 = r0 * a.bin - a.ay, x0 = c0 * a.bin - a.ax;                           // input pixel of LDS word (0, 0)
  const float* src = in + plane * ((int64_t)a.height * a.width);
  for (int i = threadIdx.x; i < lh * lw; i += CB_THREADS) {
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
}

// output m of the thread: output t + 256 m of the tile, row-major; r, c inside the tile
struct CorrOutput {
  int r, c;
  bool live;
};
__device__ __forceinline__ CorrOutput corr_output(const CorrBinArgs& a, int r0, int c0, int m) {
  const int T = a.tile, o = threadIdx.x + CB_THREADS * m;
  const int r = o / T, c = o - r * T;
  return CorrOutput{r, c, o < T * T && r0 + r < a.out_h && c0 + c < a.out_w};
}

// the fp64 sums of the thread's NM outputs over the staged tile, taps in the header's order
template <int NM>
__device__ __forceinline__ void corr_sum_taps(const float* tile, const double* taps, const CorrBinArgs& a, int r0, int c0, double (&acc)[NM]) {
  const int lw = (a.tile - 1) * a.bin + a.kw;
  int base[NM];
#pragma unroll
  for (int m = 0; m < NM; ++m) {
    const CorrOutput o = corr_output(a, r0, c0, m);
    base[m] = o.live ? (o.r * a.bin) * lw + o.c * a.bin : 0;          // a dead slot reads word (i, j): inside the tile
    acc[m] = -0.0;                                // -0.0 + x == x for every x: the first product starts the sum
  }
  for (int i = 0; i < a.kh; ++i) {
    const float* row = tile + i * lw;
#pragma unroll 8
    for (int j = 0; j < a.kw; ++j) {            // unrolled: eight taps per scalar load, eight LDS reads in flight per output
      const double w = taps[i * a.kw + j];
#pragma unroll
      for (int m = 0; m < NM; ++m) acc[m] = acc[m] + w * (double)row[base[m] + j];
    }
  }
}

// ---- adjoint --------------------------------------------------------------------------------------------------------------------
__host__ __device__ __forceinline__ int floor_div(int a, int b) {      // b > 0
  const int q = a / b;
  return (a % b != 0 && a < 0) ? q - 1 : q;
}
__host__ __device__ __forceinline__ int ceil_div(int a, int b) { return -floor_div(-a, b); }

// LDS word of tap (i, j): the row's taps are grouped by j mod bin, so that the taps one pixel meets (j = j0, j0 + bin, ...) lie side
// by side and the inner loop walks both of its operands by constant steps
__device__ __forceinline__ int tap_word(int i, int j, int bin, int kwb) { return (i * bin + j % bin) * kwb + j / bin; }

struct AdjointLds {
  LdsF64* taps;            // [kh][bin][kwb]: tap_word
  LdsF64* zero_taps;       // [kwb] of 0.0
  LdsF32* zero_row;        // [sw] of 0.f
  LdsF32* slice;           // [n_r][n_c] of the tile at hand
  int kwb, sw;             // taps of a row that one pixel can meet, at most; columns of the largest slice
};

// carves up the dynamic LDS (adjoint_lds_bytes, 8-byte aligned) and fills the rows of zeros; the first tile's barrier covers the fill
__device__ __forceinline__ AdjointLds adjoint_lds(unsigned char* lds, const CorrBinArgs& a) {
  AdjointLds L;
  L.kwb = (a.kw + a.bin - 1) / a.bin;
  L.sw = (CB_TILE + a.kw - 2) / a.bin + 1;
  L.taps = (LdsF64*)lds;
  L.zero_taps = L.taps + a.kh * a.bin * L.kwb;
  L.zero_row = (LdsF32*)(L.zero_taps + L.kwb);
  L.slice = L.zero_row + L.sw;
  for (int i = threadIdx.x; i < L.kwb; i += CB_THREADS) L.zero_taps[i] = 0.0;
  for (int i = threadIdx.x; i < L.sw; i += CB_THREADS) L.zero_row[i] = 0.f;
  return L;
}

// the thread's pixels of the tile from (y0, x0) on: column t % 32, rows t / 32 + 8 m
__device__ __forceinline__ int adjoint_column(int x0) { return x0 + threadIdx.x % CB_TILE; }
__device__ __forceinline__ int adjoint_row(int y0, int m) { return y0 + threadIdx.x / CB_TILE + (CB_THREADS / CB_TILE) * m; }

// the detector pixels whose taps reach a tile; n_r or n_c may be <= 0: no tap reaches the tile
struct AdjointSlice {
  int r_lo, r_hi, c_lo, c_hi, n_r, n_c;
};

// Stages what the tile from (y0, x0) on needs: the plane's kernel, unless `staged` says it is there, and the slice of g_out.  A
// barrier follows.
__device__ __forceinline__ AdjointSlice adjoint_stage_tile(const AdjointLds& L, const float* g_out, const double* K, const CorrBinArgs& a,
                                                           int64_t plane, int64_t& staged, int y0, int x0) {
  const int bin = a.bin, t = threadIdx.x;
  const int y_last = (y0 + CB_TILE < a.height ? y0 + CB_TILE : a.height) - 1;
  const int x_last = (x0 + CB_TILE < a.width ? x0 + CB_TILE : a.width) - 1;
  // the detector pixels whose taps reach the tile: R bin in [y0 + ay - (kh - 1), y_last + ay]
  AdjointSlice s;
  s.r_lo = ceil_div(y0 + a.ay - (a.kh - 1), bin); s.r_hi = floor_div(y_last + a.ay, bin);
  s.c_lo = ceil_div(x0 + a.ax - (a.kw - 1), bin); s.c_hi = floor_div(x_last + a.ax, bin);
  s.r_lo = s.r_lo < 0 ? 0 : s.r_lo; s.r_hi = s.r_hi > a.out_h - 1 ? a.out_h - 1 : s.r_hi;
  s.c_lo = s.c_lo < 0 ? 0 : s.c_lo; s.c_hi = s.c_hi > a.out_w - 1 ? a.out_w - 1 : s.c_hi;
  s.n_r = s.r_hi - s.r_lo + 1; s.n_c = s.c_hi - s.c_lo + 1;
  const int64_t kernel = a.n_kernels == 1 ? (int64_t)0 : plane;
  if (kernel != staged) {
    const double* src = K + kernel * a.kh * a.kw;
    for (int i = t; i < a.kh * a.kw; i += CB_THREADS) L.taps[tap_word(i / a.kw, i % a.kw, bin, L.kwb)] = src[i];
    staged = kernel;
  }
  if (s.n_r > 0 && s.n_c > 0) {
    const float* src = g_out + plane * ((int64_t)a.out_h * a.out_w);
    for (int i = t; i < s.n_r * s.n_c; i += CB_THREADS) {
      const int r = i / s.n_c;
      L.slice[i] = src[(int64_t)(s.r_lo + r) * a.out_w + s.c_lo + (i - r * s.n_c)];
    }
  }
  return s;
}

// Every term of one pixel that taps were clamped onto (BOUNDARY_NEAREST, a pixel on the edge).  Row i of the kernel meets the pixel
// through the detector rows ceil((y + ay - i) / bin) .. floor(same): one row, or none, inside the plane; 0 .. floor on row 0 and
// ceil .. H / bin - 1 on the last row, where the clamped taps gather.  Quotient and remainder of (y + ay - i) / bin are carried
// from tap to tap (no division in the loops), and so is the LDS word of the tap.
__device__ __forceinline__ double adjoint_pixel_clamped(const AdjointLds& L, const AdjointSlice& s, const CorrBinArgs& a, int y, int x) {
  const int bin = a.bin, kwb = L.kwb;
  const bool top = y == 0, bottom = y == a.height - 1, left = x == 0, right = x == a.width - 1;
  const int ty = y + a.ay, tx = x + a.ax;
  double acc = 0.0;
  int qy = ty / bin, ry = ty - qy * bin;          // ty - i = qy bin + ry, 0 <= ry < bin
  for (int i = 0; i < a.kh; ++i) {
    int ra = top ? 0 : qy + (ry > 0), rb = bottom ? a.out_h - 1 : qy;
    ra = ra < s.r_lo ? s.r_lo : ra; rb = rb > s.r_hi ? s.r_hi : rb;
    if (ra <= rb) {
      int qx = tx / bin, rx = tx - qx * bin;
      int word = i * bin * kwb, jm = 0;           // tap_word(i, j): j = jd bin + jm, word = (i bin + jm) kwb + jd
      for (int j = 0; j < a.kw; ++j) {
        int ca = left ? 0 : qx + (rx > 0), cb = right ? a.out_w - 1 : qx;
        ca = ca < s.c_lo ? s.c_lo : ca; cb = cb > s.c_hi ? s.c_hi : cb;
        if (ca <= cb) {
          const double w = L.taps[word];
          for (int R = ra; R <= rb; ++R) {
            const LdsF32* grow = L.slice + (R - s.r_lo) * s.n_c - s.c_lo;
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

// the fp64 sums of the thread's four pixels, column x < width, over the staged kernel and slice; 0.0 for a row outside the plane
template <bool NEAREST>
__device__ __forceinline__ void adjoint_sum_tile(const AdjointLds& L, const AdjointSlice& s, const CorrBinArgs& a, int y0, int x,
                                                 double (&acc)[CB_NM]) {
  const int bin = a.bin;
#pragma unroll
  for (int m = 0; m < CB_NM; ++m) acc[m] = 0.0;
  if (s.n_r <= 0 || s.n_c <= 0) return;
  bool clamped[CB_NM];                                                // a pixel that taps were clamped onto: on the edge under NEAREST
#pragma unroll
  for (int m = 0; m < CB_NM; ++m) {
    const int y = adjoint_row(y0, m);
    clamped[m] = NEAREST && y < a.height && (x == 0 || x == a.width - 1 || y == 0 || y == a.height - 1);
  }
  {
    // The pixels that no tap was clamped onto.  The thread's pixels share their column, so the taps j = j0 + b bin they meet and
    // the detector columns C0 - b are theirs in common: b runs over one range.  A step of the rows takes tap row i0 + step bin and
    // detector row R0 - step of each pixel; a pixel for which that step does not exist reads rows of zeros instead -- its sum
    // takes + 0.0 * 0.0, which changes no sum that began at +0.0 (such a sum is never -0.0) -- so the four chains run side by
    // side, unpredicated.
    const int tx = x + a.ax, j0 = tx % bin, C0 = tx / bin;
    const int b_min = C0 - s.c_hi > 0 ? C0 - s.c_hi : 0;
    int b_max = j0 < a.kw ? (a.kw - 1 - j0) / bin : -1;
    b_max = b_max < C0 - s.c_lo ? b_max : C0 - s.c_lo;
    int i0[CB_NM], R0[CB_NM], s_min[CB_NM], s_max[CB_NM];
    int s_begin = 0x7fffffff, s_end = -1;
#pragma unroll
    for (int m = 0; m < CB_NM; ++m) {
      const int y = adjoint_row(y0, m);
      const int ty = y + a.ay;
      i0[m] = ty % bin; R0[m] = ty / bin;
      s_min[m] = R0[m] - s.r_hi > 0 ? R0[m] - s.r_hi : 0;
      s_max[m] = i0[m] < a.kh ? (a.kh - 1 - i0[m]) / bin : -1;
      s_max[m] = s_max[m] < R0[m] - s.r_lo ? s_max[m] : R0[m] - s.r_lo;
      if (y >= a.height || clamped[m]) { s_min[m] = 1; s_max[m] = 0; }
      if (s_min[m] <= s_max[m]) {
        s_begin = s_begin < s_min[m] ? s_begin : s_min[m];
        s_end = s_end > s_max[m] ? s_end : s_max[m];
      }
    }
    for (int step = s_begin; step <= s_end; ++step) {
      const LdsF64* kq[CB_NM];
      const LdsF32* gq[CB_NM];
#pragma unroll
      for (int m = 0; m < CB_NM; ++m) {
        const bool live = step >= s_min[m] && step <= s_max[m];
        kq[m] = live ? L.taps + ((i0[m] + step * bin) * bin + j0) * L.kwb : L.zero_taps;
        gq[m] = live ? L.slice + (R0[m] - step - s.r_lo) * s.n_c + (C0 - s.c_lo) : L.zero_row + (L.sw - 1);
      }
#pragma unroll 4
      for (int b = b_min; b <= b_max; ++b) {
#pragma unroll
        for (int m = 0; m < CB_NM; ++m) acc[m] = acc[m] + kq[m][b] * (double)gq[m][-b];
      }
    }
  }
  if (NEAREST) {
#pragma unroll 1
    for (int m = 0; m < CB_NM; ++m) {
      if (clamped[m]) acc[m] = adjoint_pixel_clamped(L, s, a, adjoint_row(y0, m), x);
    }
  }
}

// ---- the finish of a sum kept over runs (coalign.hip, psf_grad.hip) -------------------------------------------------------------
// partials [group][run][per_group] -> out [group][per_group] = run 0 + run 1 + ..., one thread per output, the runs in run order;
// SCALED: times scale.  (A template, so that the files that include this header and launch no finish get no kernel from it.)
constexpr int CB_FINAL_THREADS = 256;

template <bool SCALED>
__global__ __launch_bounds__(CB_FINAL_THREADS) void run_sum_final_kernel(const double* __restrict__ partials, double* __restrict__ out,
                                                                         int n_runs, int64_t per_group, int64_t total, double scale) {
  for (int64_t idx = (int64_t)blockIdx.x * CB_FINAL_THREADS + threadIdx.x; idx < total; idx += (int64_t)gridDim.x * CB_FINAL_THREADS) {
    const int64_t group = idx / per_group;
    const double* src = partials + group * n_runs * per_group + (idx - group * per_group);
    double s = src[0];
#pragma unroll 16
    for (int r = 1; r < n_runs; ++r) s = s + src[(int64_t)r * per_group];      // unrolled: sixteen loads in flight, the adds in order
    out[idx] = SCALED ? scale * s : s;
  }
}

template <bool SCALED>
static inline void launch_run_sum_final(const double* partials, double* out, int n_runs, int64_t per_group, int64_t total, double scale,
                                        hipStream_t st) {
  hipLaunchKernelGGL(run_sum_final_kernel<SCALED>, dim3(grid_of((total + CB_FINAL_THREADS - 1) / CB_FINAL_THREADS)), dim3(CB_FINAL_THREADS), 0, st,
                     partials, out, n_runs, per_group, total, scale);
}
