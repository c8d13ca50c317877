// The gradient of the PSF-and-bin correlation with respect to its taps (include/sunerf_hip_psf_grad.h): the
// reduction that makes the point-spread function trainable.  Two kernels:
//
// 1. the PARTIAL kernel.  The tiles, the staging of a tile's input window under the boundary rule and the argument check are
//    corr_bin.h's, shared with instrument.hip; the tile of g_out is staged beside the window.  Threads are mapped to TAPS, not to
//    outputs: for a fixed detector pixel neighbouring j read neighbouring LDS words, and g_out[R][C] is one LDS address for every
//    lane that works on the same pixel (a broadcast).  A workgroup owns a chunk of at most 1024 taps (a larger kernel is cut into
//    chunks of equal size) and a thread NT <= 4 of them, q, q + G, q + 2 G, ... with G = ceil(chunk / NT) threads per group.  When
//    the chunk needs fewer than 256 threads, the 256 / G groups each take a SLICE of the tile's detector pixels -- rows
//    sr, sr + S_r, ... and one of S_c column segments -- so that 3 x 3 taps keep 252 threads busy and 18 x 18 taps 243; NT is
//    chosen on the host to make NT / slices, a thread's share of the work, smallest.  The taps of a thread share its slice, so
//    the inner loop reads g_out once per pixel and then does, per tap, one LDS read, one convert, one fp64 multiply and one fp64
//    add: the forward's inner loop with the roles of the operands swapped.  A workgroup keeps its sums in registers over a RUN of
//    (plane, tile) items of one kernel index -- the run is fixed by the arguments -- then adds the slices of each tap through LDS,
//    slice 0 first, and writes one fp64 partial per tap and run to the workspace.
// 2. the FINAL kernel (corr_bin.h's run_sum_final_kernel, shared with coalign.hip): one thread per tap adds the tap's partials, run 0
//    first, and multiplies by scale.
//
// No floating-point atomics; -ffp-contract=off and no explicit fma: every operation is rounded on its own, as the header says.
#include "corr_bin.h"
#include "../../include/sunerf_hip_psf_grad.h"

namespace {

constexpr int PG_MAX_NT = SUNERF_PSF_GRAD_CHUNK / CB_THREADS;      // taps per thread at most
constexpr int PG_MAX_SC = 4;                                       // column segments of a tile at most
static_assert(PG_MAX_NT * CB_THREADS == SUNERF_PSF_GRAD_CHUNK, "whole taps per thread");

struct PsfGradPlan {
  int taps, chunks, chunk_taps;
  int nt, group;                                 // taps per thread (the NT the kernel is compiled for); threads per slice
  int slices, slice_rows, slice_cols, seg;       // slices = slice_rows * slice_cols; seg: columns of a segment
  int n_runs;
  int64_t tiles, items;                          // tiles of a plane; (plane, tile) items of one kernel index
};

PsfGradPlan psf_grad_plan(const CorrBinArgs& a) {
  PsfGradPlan p;
  p.taps = a.kh * a.kw;
  p.chunks = (p.taps + SUNERF_PSF_GRAD_CHUNK - 1) / SUNERF_PSF_GRAD_CHUNK;
  p.chunk_taps = (p.taps + p.chunks - 1) / p.chunks;
  p.nt = 0;
  for (int nt = 1; nt <= PG_MAX_NT; ++nt) {      // the smallest nt / slices; of equals the larger nt (more taps share one read of g_out)
    const int group = (p.chunk_taps + nt - 1) / nt;
    if (group > CB_THREADS) continue;
    const int avail = CB_THREADS / group;
    const int rows = avail < a.tile ? avail : a.tile;
    int cols = avail / rows < PG_MAX_SC ? avail / rows : PG_MAX_SC;
    cols = cols < a.tile ? cols : a.tile;
    if (p.nt == 0 || nt * p.slices <= p.nt * rows * cols) {
      p.nt = nt; p.group = group; p.slice_rows = rows; p.slice_cols = cols; p.slices = rows * cols;
    }
  }
  p.seg = (a.tile + p.slice_cols - 1) / p.slice_cols;
  p.tiles = (int64_t)a.tiles_y * a.tiles_x;
  p.items = (int64_t)(a.n_planes / a.n_kernels) * p.tiles;
  const int cap = SUNERF_PSF_GRAD_MAX_RUNS / a.n_kernels < 1 ? 1 : SUNERF_PSF_GRAD_MAX_RUNS / a.n_kernels;
  p.n_runs = (int)(p.items < cap ? p.items : cap);
  return p;
}

// dynamic LDS: the tile of g_out and the input window, or the slices' sums that take their place once a run is over
size_t psf_grad_lds_bytes(const CorrBinArgs& a, const PsfGradPlan& p) {
  const size_t stage = ((size_t)a.tile * a.tile + (size_t)corr_tile_words(a)) * sizeof(float);
  const size_t sums = (size_t)p.chunk_taps * p.slices * sizeof(double);
  return stage > sums ? stage : sums;
}

template <bool NEAREST, int NT>
__global__ __launch_bounds__(CB_THREADS) void psf_grad_partial_kernel(const float* __restrict__ in, const float* __restrict__ g_out,
                                                                      double* __restrict__ partials, CorrBinArgs a, PsfGradPlan p) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  float* g_tile = lds;                           // [n_r][n_c]: the tile's detector pixels inside the frame
  float* tile = lds + a.tile * a.tile;           // [lh][lw]
  double* sums = (double*)lds;                   // [slices][chunk_taps], after the run
  const int t = threadIdx.x;
  const int lw = (a.tile - 1) * a.bin + a.kw;
  const int64_t out_px = (int64_t)a.out_h * a.out_w;
  const int64_t n_work = (int64_t)a.n_kernels * p.n_runs * p.chunks;
  const int slice = t / p.group, q = t - slice * p.group;
  const bool busy = slice < p.slices;            // a thread past the last group only stages
  const int sc = slice / p.slice_rows, sr = slice - sc * p.slice_rows;
  for (int64_t work = blockIdx.x; work < n_work; work += gridDim.x) {
    const int chunk = (int)(work % p.chunks);
    const int64_t kr = work / p.chunks;
    const int run = (int)(kr % p.n_runs), k = (int)(kr / p.n_runs);
    int word[NT];                                // LDS word of the tap inside the window of pixel (0, 0); a slot without a tap reads
    double acc[NT];                              // word 0 and its sum is dropped
#pragma unroll
    for (int m = 0; m < NT; ++m) {
      const int in_chunk = q + m * p.group, tap = chunk * p.chunk_taps + in_chunk;
      const int i = tap / a.kw;
      word[m] = (in_chunk < p.chunk_taps && tap < p.taps) ? i * lw + (tap - i * a.kw) : 0;
      acc[m] = 0.0;
    }
    const int64_t first = (int64_t)run * p.items / p.n_runs, end = (int64_t)(run + 1) * p.items / p.n_runs;
    for (int64_t item = first; item < end; ++item) {
      const int64_t plane = k + (item / p.tiles) * a.n_kernels;
      const int in_plane = (int)(item % p.tiles);
      const int r0 = (in_plane / a.tiles_x) * a.tile, c0 = (in_plane % a.tiles_x) * a.tile;
      const int n_r = a.out_h - r0 < a.tile ? a.out_h - r0 : a.tile, n_c = a.out_w - c0 < a.tile ? a.out_w - c0 : a.tile;
      const int npx = n_r * n_c;
      corr_stage_tile<NEAREST>(tile, in, a, plane, r0, c0);
      const float* g_src = g_out + plane * out_px + (int64_t)r0 * a.out_w + c0;
      for (int o = t; o < npx; o += CB_THREADS) {
        const int r = o / n_c;
        g_tile[o] = g_src[(int64_t)r * a.out_w + (o - r * n_c)];
      }
      __syncthreads();
      if (busy) {
        const int c_lo = sc * p.seg, c_hi = (sc + 1) * p.seg < n_c ? (sc + 1) * p.seg : n_c;
        for (int r = sr; r < n_r; r += p.slice_rows) {
          const float* g_row = g_tile + r * n_c;
          const float* t_row = tile + r * a.bin * lw;
#pragma unroll 4
          for (int c = c_lo; c < c_hi; ++c) {
            const double g = (double)g_row[c];
#pragma unroll
            for (int m = 0; m < NT; ++m) acc[m] = acc[m] + g * (double)t_row[word[m] + c * a.bin];
          }
        }
      }
      __syncthreads();                           // the tiles are overwritten by the next item, or by the sums
    }
    if (busy) {
#pragma unroll
      for (int m = 0; m < NT; ++m) {
        const int in_chunk = q + m * p.group;
        if (in_chunk < p.chunk_taps) sums[slice * p.chunk_taps + in_chunk] = acc[m];
      }
    }
    __syncthreads();
    for (int u = t; u < p.chunk_taps; u += CB_THREADS) {
      const int tap = chunk * p.chunk_taps + u;
      if (tap < p.taps) {
        double s = sums[u];
        for (int sl = 1; sl < p.slices; ++sl) s = s + sums[sl * p.chunk_taps + u];
        partials[((int64_t)k * p.n_runs + run) * p.taps + tap] = s;
      }
    }
    __syncthreads();                             // the sums are overwritten by the next work item's tiles
  }
}

template <bool NEAREST>
int launch(const float* in, const float* g_out, double* g_K, double* partials, const CorrBinArgs& a, const PsfGradPlan& p, hipStream_t st) {
  const size_t lds = psf_grad_lds_bytes(a, p);
  const dim3 grid(grid_of((int64_t)a.n_kernels * p.n_runs * p.chunks));
  int e = 0;
#define PG_PARTIAL(NT)                                                                                                       \
  do {                                                                                                                       \
    e = adjoint_lds_opt_in((const void*)psf_grad_partial_kernel<NEAREST, NT>, lds);                                          \
    if (e != 0) return e;                                                                                                    \
    SUNERF_CLEAR_ERROR();                                                                                                    \
    hipLaunchKernelGGL((psf_grad_partial_kernel<NEAREST, NT>), grid, dim3(CB_THREADS), lds, st, in, g_out, partials, a, p);  \
  } while (0)
  switch (p.nt) {
    case 1: PG_PARTIAL(1); break;
    case 2: PG_PARTIAL(2); break;
    case 3: PG_PARTIAL(3); break;
    default: PG_PARTIAL(4); break;
  }
#undef PG_PARTIAL
  const int64_t total = (int64_t)a.n_kernels * p.taps;
  launch_run_sum_final<true>(partials, g_K, p.n_runs, p.taps, total, a.scale, st);
  SUNERF_CHECK_LAUNCH();
  return 0;
}

}  // namespace

extern "C" int sunerf_psf_grad_abi_version(void) { return SUNERF_PSF_GRAD_ABI_VERSION; }

extern "C" size_t sunerf_psf_grad_workspace_bytes(int n_planes, int height, int width, int n_kernels, int kh, int kw, int bin) {
  if (n_planes < 1 || height < 1 || width < 1 || n_kernels < 1 || kh < 1 || kw < 1 || bin < 1 || !corr_bin_within_limits(kh, kw, bin)) return 0;
  if (n_planes % n_kernels != 0 || height / bin == 0 || width / bin == 0) return 0;
  const CorrBinArgs a = corr_bin_args(n_planes, height, width, n_kernels, kh, kw, bin, 0, 0, 1.0);
  const PsfGradPlan p = psf_grad_plan(a);
  return (size_t)n_kernels * p.n_runs * p.taps * sizeof(double);
}

extern "C" int sunerf_psf_grad_taps(const float* in, const float* g_out, int n_planes, int height, int width, int n_kernels, int kh, int kw,
                                    int bin, int anchor_y, int anchor_x, double scale, int boundary, double* g_K, void* workspace,
                                    void* stream) {
  bool empty;
  const int status = corr_bin_check(n_planes, height, width, n_kernels, kh, kw, bin, anchor_y, anchor_x, boundary, &empty, true);
  if (status != 0 || empty) return status;
  if (!in || !g_out || !g_K || !workspace) return SUNERF_E_BADARG;          // the workspace's size is non-zero here
  if ((uintptr_t)g_K % sizeof(double) || (uintptr_t)workspace % sizeof(double)) return SUNERF_E_BADARG;
  const CorrBinArgs a = corr_bin_args(n_planes, height, width, n_kernels, kh, kw, bin, anchor_y, anchor_x, scale);
  if (corr_tile_words(a) > CB_MAX_WORDS) return SUNERF_E_UNSUPPORTED;          // cannot happen inside the limits above
  const PsfGradPlan p = psf_grad_plan(a);
  hipStream_t st = (hipStream_t)stream;
  if (boundary == SUNERF_INSTRUMENT_BOUNDARY_NEAREST) return launch<true>(in, g_out, g_K, (double*)workspace, a, p, st);
  return launch<false>(in, g_out, g_K, (double*)workspace, a, p, st);
}
