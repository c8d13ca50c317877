// The six sums of a masked zero-mean normalised cross-correlation for every integer shift of a window
// (include/sunerf_hip_coalign.h): the reduction behind sunerf_hip/coalign.py.  Two kernels:
//
// 1. the PARTIAL kernel: psf_grad.hip's mapping with shifts in the place of taps.  A workgroup stages a tile of 32 x 32 template
//    pixels and the image window that the tile's shifts reach, (32 + 2 max_dy) x (32 + 2 max_dx) pixels, in LDS -- each pixel as
//    the pair (value, validity): a pixel outside the frame, a non-finite or a flagged one is (+0.0, 0.0), every other (v, 1.0), so
//    that the six updates need no branch and a pair outside the set adds zeros.  Threads are mapped to SHIFTS: a workgroup owns a
//    chunk of at most 1024 shifts (a larger window is cut into chunks of equal size) and a thread NT <= 4 of them, q, q + G,
//    q + 2 G, ... with G = ceil(chunk / NT) threads per group; the 6 NT fp64 sums live in registers.  For a fixed template pixel
//    neighbouring dx read neighbouring 8-byte LDS words and the template pixel is one LDS address for every lane of the group (a
//    broadcast).  When the chunk needs fewer than 256 threads, the 256 / G groups each take a SLICE of the tile's template pixels,
//    as in psf_grad.hip.  A workgroup keeps its sums over a RUN of tiles of one plane -- the run is fixed by the arguments -- then
//    adds the slices of each sum through LDS, slice 0 first, and writes one fp64 partial per sum, shift and run to the workspace.
// 2. the FINAL kernel (corr_bin.h's run_sum_final_kernel, shared with psf_grad.hip): one thread per sum adds its partials, run 0 first.
//
// The tile geometry (CorrBinArgs with kh = 2 max_dy + 1, kw = 2 max_dx + 1, bin 1, the anchor in the middle), the thread count and
// the LDS opt-in are corr_bin.h's.  No floating-point atomics; -ffp-contract=off and no explicit fma: every operation is rounded on
// its own, as the header says.
#include "corr_bin.h"
#include "../../include/sunerf_hip_coalign.h"

namespace {

constexpr int CA_TILE = SUNERF_COALIGN_TILE;
constexpr int CA_SUMS = SUNERF_COALIGN_SUMS;
constexpr int CA_MAX_NT = SUNERF_COALIGN_CHUNK / CB_THREADS;      // shifts per thread at most
constexpr int CA_MAX_SC = 4;                                       // column segments of a tile at most
static_assert(CA_MAX_NT * CB_THREADS == SUNERF_COALIGN_CHUNK, "whole shifts per thread");
static_assert(CA_TILE == SUNERF_INSTRUMENT_TILE, "corr_tile gives this tile for every window inside the limit");
static_assert(2 * SUNERF_COALIGN_MAX_SHIFT + 1 + CA_TILE - 1 <= 127, "the window fits the correlation's largest tile");

struct CoalignPlan {
  int shifts, chunks, chunk_shifts;
  int nt, group;                                 // shifts per thread (the NT the kernel is compiled for); threads per slice
  int slices, slice_rows, slice_cols, seg;       // slices = slice_rows * slice_cols; seg: columns of a segment
  int n_runs;
  int64_t tiles;                                 // tiles of a plane
};

CoalignPlan coalign_plan(const CorrBinArgs& a) {
  CoalignPlan p;
  p.shifts = a.kh * a.kw;
  p.chunks = (p.shifts + SUNERF_COALIGN_CHUNK - 1) / SUNERF_COALIGN_CHUNK;
  p.chunk_shifts = (p.shifts + p.chunks - 1) / p.chunks;
  p.nt = 0;
  for (int nt = 1; nt <= CA_MAX_NT; ++nt) {      // the smallest nt / slices; of equals the larger nt (more shifts share one template read)
    const int group = (p.chunk_shifts + nt - 1) / nt;
    if (group > CB_THREADS) continue;
    const int avail = CB_THREADS / group;
    const int rows = avail < CA_TILE ? avail : CA_TILE;
    const int cols = avail / rows < CA_MAX_SC ? avail / rows : CA_MAX_SC;
    if (p.nt == 0 || nt * p.slices <= p.nt * rows * cols) {
      p.nt = nt; p.group = group; p.slice_rows = rows; p.slice_cols = cols; p.slices = rows * cols;
    }
  }
  p.seg = (CA_TILE + p.slice_cols - 1) / p.slice_cols;
  p.tiles = (int64_t)a.tiles_y * a.tiles_x;
  const int cap = SUNERF_COALIGN_MAX_RUNS / a.n_planes < 1 ? 1 : SUNERF_COALIGN_MAX_RUNS / a.n_planes;
  p.n_runs = (int)(p.tiles < cap ? p.tiles : cap);
  return p;
}

// dynamic LDS: the template tile and the image window as (value, validity) pairs, or the slices' sums that take their place once
// a run is over; at most 8 KiB + 72 KiB
size_t coalign_lds_bytes(const CorrBinArgs& a, const CoalignPlan& p) {
  const size_t stage = ((size_t)CA_TILE * CA_TILE + (size_t)corr_tile_words(a)) * sizeof(f32x2);
  const size_t sums = (size_t)p.chunk_shifts * p.slices * CA_SUMS * sizeof(double);
  return stage > sums ? stage : sums;
}

// (value, validity) of a pixel that lies inside the frame
__device__ __forceinline__ f32x2 coalign_pixel(const float* __restrict__ values, const uint8_t* __restrict__ bad, int64_t at) {
  const float v = values[at];
  const bool valid = (__float_as_uint(v) & 0x7f800000u) != 0x7f800000u && !(bad && bad[at]);
  f32x2 px;
  px.x = valid ? v : 0.f;
  px.y = valid ? 1.f : 0.f;
  return px;
}

template <int NT>
__global__ __launch_bounds__(CB_THREADS) void coalign_partial_kernel(const float* __restrict__ image, const float* __restrict__ templ,
                                                                     const uint8_t* __restrict__ bad_image,
                                                                     const uint8_t* __restrict__ bad_templ,
                                                                     double* __restrict__ partials, CorrBinArgs a, CoalignPlan p) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  f32x2* t_tile = (f32x2*)lds;                   // [n_r][n_c]: the tile's template pixels inside the frame
  f32x2* window = t_tile + CA_TILE * CA_TILE;    // [n_r + 2 max_dy][lw]: image pixel (r0 - max_dy, c0 - max_dx) is word (0, 0)
  double* sums = (double*)lds;                   // [slices][chunk_shifts][6], after the run
  const int t = threadIdx.x;
  const int lw = CA_TILE - 1 + a.kw;
  const int64_t plane_px = (int64_t)a.height * a.width;
  const int64_t n_work = (int64_t)a.n_planes * p.n_runs * p.chunks;
  const int slice = t / p.group, q = t - slice * p.group;
  const bool busy = slice < p.slices;            // a thread past the last group only stages
  const int sc = slice / p.slice_rows, sr = slice - sc * p.slice_rows;
  for (int64_t work = blockIdx.x; work < n_work; work += gridDim.x) {
    const int chunk = (int)(work % p.chunks);
    const int64_t pr = work / p.chunks;
    const int run = (int)(pr % p.n_runs);
    const int64_t plane = pr / p.n_runs;
    int word[NT];                                // window word of the shift for template pixel (0, 0); a slot without a shift reads
    double acc[NT][CA_SUMS];                     // word 0 and its sums are dropped
#pragma unroll
    for (int m = 0; m < NT; ++m) {
      const int in_chunk = q + m * p.group, s = chunk * p.chunk_shifts + in_chunk;
      const int i = s / a.kw;
      word[m] = (in_chunk < p.chunk_shifts && s < p.shifts) ? i * lw + (s - i * a.kw) : 0;
#pragma unroll
      for (int k = 0; k < CA_SUMS; ++k) acc[m][k] = 0.0;
    }
    const float* img = image + plane * plane_px;
    const float* tpl = templ + plane * plane_px;
    const uint8_t* bad_i = bad_image ? bad_image + plane * plane_px : nullptr;
    const uint8_t* bad_t = bad_templ ? bad_templ + plane * plane_px : nullptr;
    const int64_t first = (int64_t)run * p.tiles / p.n_runs, end = (int64_t)(run + 1) * p.tiles / p.n_runs;
    for (int64_t tile = first; tile < end; ++tile) {
      const int r0 = (int)(tile / a.tiles_x) * CA_TILE, c0 = (int)(tile % a.tiles_x) * CA_TILE;
      const int n_r = a.height - r0 < CA_TILE ? a.height - r0 : CA_TILE, n_c = a.width - c0 < CA_TILE ? a.width - c0 : CA_TILE;
      const int y0 = r0 - a.ay, x0 = c0 - a.ax;
      for (int i = t; i < (n_r + a.kh - 1) * lw; i += CB_THREADS) {
        const int ly = i / lw;
        const int y = y0 + ly, x = x0 + (i - ly * lw);
        f32x2 px;
        px.x = 0.f; px.y = 0.f;
        if (y >= 0 && y < a.height && x >= 0 && x < a.width) px = coalign_pixel(img, bad_i, (int64_t)y * a.width + x);
        window[i] = px;
      }
      for (int o = t; o < n_r * n_c; o += CB_THREADS) {
        const int r = o / n_c;
        t_tile[o] = coalign_pixel(tpl, bad_t, (int64_t)(r0 + r) * a.width + c0 + (o - r * n_c));
      }
      __syncthreads();
      if (busy) {
        const int c_lo = sc * p.seg, c_hi = (sc + 1) * p.seg < n_c ? (sc + 1) * p.seg : n_c;
        for (int r = sr; r < n_r; r += p.slice_rows) {
          const f32x2* t_row = t_tile + r * n_c;
          const f32x2* w_row = window + r * lw;
#pragma unroll 2
          for (int c = c_lo; c < c_hi; ++c) {
            const f32x2 tb = t_row[c];
            const double b = (double)tb.x, vb = (double)tb.y;
            const double bb = b * b;
#pragma unroll
            for (int m = 0; m < NT; ++m) {
              const f32x2 wa = w_row[word[m] + c];
              const double av = (double)wa.x, va = (double)wa.y;
              acc[m][0] = acc[m][0] + va * vb;
              acc[m][1] = acc[m][1] + av * vb;
              acc[m][2] = acc[m][2] + b * va;
              acc[m][3] = acc[m][3] + (av * av) * vb;
              acc[m][4] = acc[m][4] + bb * va;
              acc[m][5] = acc[m][5] + av * b;
            }
          }
        }
      }
      __syncthreads();                           // the tiles are overwritten by the next tile, or by the sums
    }
    if (busy) {
#pragma unroll
      for (int m = 0; m < NT; ++m) {
        const int in_chunk = q + m * p.group;
        if (in_chunk < p.chunk_shifts) {
#pragma unroll
          for (int k = 0; k < CA_SUMS; ++k) sums[((int64_t)slice * p.chunk_shifts + in_chunk) * CA_SUMS + k] = acc[m][k];
        }
      }
    }
    __syncthreads();
    const int per_slice = p.chunk_shifts * CA_SUMS;
    for (int u = t; u < per_slice; u += CB_THREADS) {
      const int s = chunk * p.chunk_shifts + u / CA_SUMS;
      if (s < p.shifts) {
        double v = sums[u];
        for (int sl = 1; sl < p.slices; ++sl) v = v + sums[sl * per_slice + u];
        partials[((plane * p.n_runs + run) * p.shifts + s) * CA_SUMS + (u % CA_SUMS)] = v;
      }
    }
    __syncthreads();                             // the sums are overwritten by the next work item's tiles
  }
}

int launch(const float* image, const float* templ, const uint8_t* bad_image, const uint8_t* bad_templ, double* out, double* partials,
           const CorrBinArgs& a, const CoalignPlan& p, hipStream_t st) {
  const size_t lds = coalign_lds_bytes(a, p);
  const dim3 grid(grid_of((int64_t)a.n_planes * p.n_runs * p.chunks));
  int e = 0;
#define CA_PARTIAL(NT)                                                                                                       \
  do {                                                                                                                       \
    e = adjoint_lds_opt_in((const void*)coalign_partial_kernel<NT>, lds);                                                    \
    if (e != 0) return e;                                                                                                    \
    SUNERF_CLEAR_ERROR();                                                                                                    \
    hipLaunchKernelGGL((coalign_partial_kernel<NT>), grid, dim3(CB_THREADS), lds, st, image, templ, bad_image, bad_templ,    \
                       partials, a, p);                                                                                      \
  } while (0)
  switch (p.nt) {
    case 1: CA_PARTIAL(1); break;
    case 2: CA_PARTIAL(2); break;
    case 3: CA_PARTIAL(3); break;
    default: CA_PARTIAL(4); break;
  }
#undef CA_PARTIAL
  const int64_t per_plane = (int64_t)p.shifts * CA_SUMS, total = a.n_planes * per_plane;
  launch_run_sum_final<false>(partials, out, p.n_runs, per_plane, total, 1.0, st);
  SUNERF_CHECK_LAUNCH();
  return 0;
}

bool within_limits(int max_dy, int max_dx) { return max_dy <= SUNERF_COALIGN_MAX_SHIFT && max_dx <= SUNERF_COALIGN_MAX_SHIFT; }

// the correlation's geometry of the window: one "kernel" tap per shift, the zero shift in the middle, no binning
CorrBinArgs coalign_args(int n_planes, int height, int width, int max_dy, int max_dx) {
  return corr_bin_args(n_planes, height, width, 1, 2 * max_dy + 1, 2 * max_dx + 1, 1, max_dy, max_dx, 1.0);
}

bool overlaps(const void* a, size_t a_bytes, const void* b, size_t b_bytes) {
  return b && (uintptr_t)a < (uintptr_t)b + b_bytes && (uintptr_t)b < (uintptr_t)a + a_bytes;
}

}  // namespace

extern "C" int sunerf_coalign_abi_version(void) { return SUNERF_COALIGN_ABI_VERSION; }

extern "C" size_t sunerf_coalign_workspace_bytes(int n_planes, int height, int width, int max_dy, int max_dx) {
  if (n_planes < 1 || height < 1 || width < 1 || max_dy < 0 || max_dx < 0 || !within_limits(max_dy, max_dx)) return 0;
  const CoalignPlan p = coalign_plan(coalign_args(n_planes, height, width, max_dy, max_dx));
  return (size_t)n_planes * p.n_runs * p.shifts * CA_SUMS * sizeof(double);
}

extern "C" int sunerf_coalign_shift_sums(const float* image, const float* templ, const unsigned char* bad_image,
                                         const unsigned char* bad_template, int n_planes, int height, int width, int max_dy, int max_dx,
                                         double* sums, void* workspace, void* stream) {
  if (!within_limits(max_dy, max_dx)) return SUNERF_E_UNSUPPORTED;
  const bool bad_count = n_planes < 0 || height < 0 || width < 0 || max_dy < 0 || max_dx < 0;
  if (!bad_count && (n_planes == 0 || height == 0 || width == 0)) return 0;
  if (bad_count) return SUNERF_E_BADARG;
  if (!image || !templ || !sums || !workspace) return SUNERF_E_BADARG;          // the workspace's size is non-zero here
  if ((uintptr_t)sums % sizeof(double) || (uintptr_t)workspace % sizeof(double)) return SUNERF_E_BADARG;
  const CorrBinArgs a = coalign_args(n_planes, height, width, max_dy, max_dx);
  const CoalignPlan p = coalign_plan(a);
  const size_t px = (size_t)n_planes * height * width;
  const size_t sums_bytes = (size_t)n_planes * p.shifts * CA_SUMS * sizeof(double);
  if (overlaps(sums, sums_bytes, image, px * sizeof(float)) || overlaps(sums, sums_bytes, templ, px * sizeof(float)) ||
      overlaps(sums, sums_bytes, bad_image, px) || overlaps(sums, sums_bytes, bad_template, px))
    return SUNERF_E_BADARG;
  return launch(image, templ, bad_image, bad_template, sums, (double*)workspace, a, p, (hipStream_t)stream);
}
