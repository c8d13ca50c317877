// Cosmic-ray hits and hot pixels found and filled by an iterated, masked sliding-window median (include/sunerf_hip_despike.h,
// DESIGN.md section 8v).  One entry point enqueues
//
// 1. the START kernel: mask 0 = INVALID where the image is not finite or the caller's `bad` is set, counted per plane;
// 2. up to max_iterations DETECTION passes, a Jacobi update each: pass k reads mask k from one buffer and writes mask k + 1 to the
//    other, and counts the flags it adds in the plane's counter k.  The workgroups of pass k + 1 read that counter: a plane whose
//    pass k added nothing is stopped -- both buffers then hold the same mask for it, so a stopped plane's workgroups return at once.
//    A working mask marks the flags its pass added (a bit of its own, cleared by the next pass and by the fill): a workgroup that
//    stages none of them in its tile and halo would repeat the last pass's tests on the same inputs, and copies its mask through;
// 3. the FILL kernel: the median of the clean neighbours (of the original image) into every flagged pixel, everything else copied;
// 4. the STATE kernel: the counters as the plane's fp64 state.
//
// The host never waits.  The buffers are ordered so that the last detection pass writes the workspace's mask and the fill writes the
// caller's: no kernel reads a buffer it writes.
//
// One kernel template serves 2 and 3, instantiated per radius so that the up to 48 neighbour values of a pixel live in registers
// under compile-time indices.  A workgroup of 256 threads owns a tile of 32 x 8 pixels, one per thread, and stages the tile plus its
// halo once: the value of every neighbour that takes part, +inf for one that does not (flagged, or outside the frame), and the mask
// bytes.  Selection is exact: Batcher's odd-even merge sort as a network of min / max pairs over the neighbours, excluded ones
// sinking to the top as +inf beside the count n, then the two middle order statistics by their ranks.  The MAD needs no second sort:
// the absolute deviations of an ascending sequence from its median fall and then rise, which is a bitonic sequence, and one bitonic
// merge (fp64, log2 steps) orders it.  Counts are integers added with integer atomics; there is no floating-point atomic and no
// floating-point sum across threads.  -ffp-contract=off and no explicit fma: every operation is rounded on its own, as the header says.
#include "sort_network.h"
#include "../../include/sunerf_hip_despike.h"

namespace {

constexpr int DS_TW = 32, DS_TH = 8, DS_THREADS = DS_TW * DS_TH;
constexpr int DS_COUNTERS = SUNERF_DESPIKE_MAX_ITERATIONS + 2;          // per plane: new flags of pass k, then n_invalid, n_unfilled
constexpr int DS_N_INVALID = SUNERF_DESPIKE_MAX_ITERATIONS, DS_N_UNFILLED = SUNERF_DESPIKE_MAX_ITERATIONS + 1;
constexpr int DS_START_PX = 4 * DS_THREADS;                             // pixels of one plane per workgroup of the start kernel
enum { DS_DETECT_MODEL = 0, DS_DETECT_MAD = 1, DS_FILL = 2 };
// a bit of the working masks only, never of the caller's: SPIKE was added by the pass that wrote this mask
constexpr uint8_t DS_NEW = 0x80, DS_PUBLIC = SUNERF_DESPIKE_SPIKE | SUNERF_DESPIKE_INVALID | SUNERF_DESPIKE_UNFILLED;

struct DespikeArgs {
  int n_planes, height, width, tiles_y, tiles_x, flags, min_valid;
  double n_sigma, grow_sigma;
};

// ---- start ----------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(DS_THREADS) void despike_start_kernel(const float* __restrict__ image, const uint8_t* __restrict__ bad,
                                                                   uint8_t* __restrict__ mask, unsigned* __restrict__ counters,
                                                                   int64_t plane_px, int64_t chunks_per_plane, int64_t n_chunks) {
  for (int64_t chunk = blockIdx.x; chunk < n_chunks; chunk += gridDim.x) {
    const int64_t plane = chunk / chunks_per_plane;
    const int64_t first = (chunk - plane * chunks_per_plane) * DS_START_PX;
    int count = 0;                               // the workgroup's, the same on every thread: one integer add per 1024 pixels
#pragma unroll
    for (int m = 0; m < DS_START_PX / DS_THREADS; ++m) {
      const int64_t i = first + m * DS_THREADS + threadIdx.x;
      bool invalid = false;
      if (i < plane_px) {
        const int64_t px = plane * plane_px + i;
        invalid = !isfinite(image[px]) || (bad && bad[px]);
        mask[px] = invalid ? SUNERF_DESPIKE_INVALID : 0;
      }
      count += __syncthreads_count(invalid);
    }
    if (threadIdx.x == 0 && count) atomicAdd(&counters[plane * DS_COUNTERS + DS_N_INVALID], (unsigned)count);
  }
}

// ---- detection and fill ---------------------------------------------------------------------------------------------------------
template <int R, int KIND>
__global__ __launch_bounds__(DS_THREADS) void despike_kernel(const float* __restrict__ image, const double* __restrict__ params,
                                                             const uint8_t* __restrict__ mask_in, uint8_t* __restrict__ mask_out,
                                                             float* __restrict__ clean, unsigned* __restrict__ counters, int pass,
                                                             DespikeArgs a) {
  constexpr int LW = DS_TW + 2 * R, LH = DS_TH + 2 * R, N = (2 * R + 1) * (2 * R + 1) - 1;
  __shared__ float val[LH * LW];
  __shared__ uint8_t msk[LH * LW];
  const int t = threadIdx.x, tx = t % DS_TW, ty = t / DS_TW;
  const int64_t plane_px = (int64_t)a.height * a.width;
  const int64_t tiles_per_plane = (int64_t)a.tiles_y * a.tiles_x;
  const int64_t n_tiles = tiles_per_plane * a.n_planes;
  const float inf = __builtin_inff();
  for (int64_t tile_id = blockIdx.x; tile_id < n_tiles; tile_id += gridDim.x) {
    const int64_t plane = tile_id / tiles_per_plane;
    unsigned* ctr = counters + plane * DS_COUNTERS;
    if (KIND != DS_FILL && pass > 0 && ctr[pass - 1] == 0) continue;          // the whole workgroup: the plane has stopped
    const int64_t in_plane = tile_id - plane * tiles_per_plane;
    const int y0 = (int)(in_plane / a.tiles_x) * DS_TH, x0 = (int)(in_plane % a.tiles_x) * DS_TW;
    const float* img = image + plane * plane_px;
    const uint8_t* min_ = mask_in + plane * plane_px;
    int fresh = 0;                               // a flag the last pass added, in the tile or its halo
    for (int i = t; i < LH * LW; i += DS_THREADS) {
      const int ly = i / LW, lx = i - ly * LW;
      const int y = y0 + ly - R, x = x0 + lx - R;
      float v = inf;                             // a neighbour that takes no part
      uint8_t m = 0;
      if (y >= 0 && y < a.height && x >= 0 && x < a.width) {
        const int64_t q = (int64_t)y * a.width + x;
        m = min_[q];
        if (m == 0) v = img[q];
      }
      val[i] = v;
      msk[i] = m;
      fresh |= m & DS_NEW;
    }
    // A pixel's test reads the mask inside its window only, and the windows of the tile lie inside what was staged: where the
    // last pass added no flag there, this pass repeats the last one's tests on the same inputs and adds none either.
    const bool repeat = !__syncthreads_or(fresh) && pass > 0;
    const int y = y0 + ty, x = x0 + tx;
    int counted = 0;
    if (y < a.height && x < a.width) {
      const int c = (ty + R) * LW + tx + R;
      const uint8_t m = msk[c];
      const int64_t px = plane * plane_px + (int64_t)y * a.width + x;
      const bool work = KIND == DS_FILL ? (m != 0 && !(a.flags & SUNERF_DESPIKE_FILL_NAN)) : (m == 0 && !repeat);
      float out = __builtin_nanf("");
      uint8_t mo = m & DS_PUBLIC;
      if (work) {
        float v[N];
        int n = 0;
#pragma unroll
        for (int k = 0; k < N; ++k) {
          const int w = k < N / 2 ? k : k + 1;          // the window's positions row by row, the centre left out
          v[k] = val[c + (w / (2 * R + 1) - R) * LW + w % (2 * R + 1) - R];
          n += v[k] < inf ? 1 : 0;
        }
        sort_network<N>(v);
        const double med = 0.5 * ((double)pick<N>(v, (n - 1) / 2) + (double)pick<N>(v, n / 2));
        if (KIND == DS_FILL) {
          if (n >= a.min_valid) {
            out = (float)med;
          } else {
            mo = mo | SUNERF_DESPIKE_UNFILLED;
            counted = 1;
          }
        } else if (n >= a.min_valid) {
          bool grow = false;
#pragma unroll
          for (int dy = -1; dy <= 1; ++dy) {
#pragma unroll
            for (int dx = -1; dx <= 1; ++dx)
              if (dy != 0 || dx != 0) grow = grow || (msk[c + dy * LW + dx] & SUNERF_DESPIKE_SPIKE);
          }
          const double thr = grow ? a.grow_sigma : a.n_sigma;
          const double d = (double)val[c] - med;
          const bool two_sided = a.flags & SUNERF_DESPIKE_TWO_SIDED;
          bool hit;
          if (KIND == DS_DETECT_MODEL) {
            const double var = params[4 * plane] + params[4 * plane + 1] * (med > 0.0 ? med : 0.0);
            const double lim = (thr * thr) * var;
            hit = (two_sided ? d != 0.0 : d > 0.0) && d * d > lim;
          } else {
            double dev[N];
#pragma unroll
            for (int i = 0; i < N; ++i) dev[i] = fabs((double)v[i] - med);      // falls, rises, then +inf: bitonic
            bitonic_merge<N>(dev);
            const double mad = 0.5 * (pick<N>(dev, (n - 1) / 2) + pick<N>(dev, n / 2));
            double s = 1.4826 * mad;
            const double floor_ = params[4 * plane + 2];
            s = s > floor_ ? s : floor_;
            hit = (two_sided ? fabs(d) : d) > thr * s;
          }
          if (hit) {
            mo = SUNERF_DESPIKE_SPIKE | DS_NEW;
            counted = 1;
          }
        }
      } else if (KIND == DS_FILL && m == 0) {
        out = image[px];                         // bit for bit
      }
      mask_out[px] = mo;
      if (KIND == DS_FILL) clean[px] = out;
    }
    const int total = __syncthreads_count(counted);          // also: the tile is overwritten by the next
    if (t == 0 && total) atomicAdd(&ctr[KIND == DS_FILL ? DS_N_UNFILLED : pass], (unsigned)total);
  }
}

// ---- state ----------------------------------------------------------------------------------------------------------------------
__global__ void despike_state_kernel(const unsigned* __restrict__ counters, double* __restrict__ state, int n_planes, int max_iterations) {
  const int plane = blockIdx.x * blockDim.x + threadIdx.x;
  if (plane >= n_planes) return;
  const unsigned* ctr = counters + (int64_t)plane * DS_COUNTERS;
  double n_spike = 0.0;
  int passes = 0;
  while (passes < max_iterations && ctr[passes] != 0) n_spike = n_spike + (double)ctr[passes++];
  double* st = state + (int64_t)plane * SUNERF_DESPIKE_STATE;
  st[0] = n_spike;
  st[1] = (double)ctr[DS_N_INVALID];
  st[2] = (double)ctr[DS_N_UNFILLED];
  st[3] = (double)passes;
  st[4] = passes < max_iterations ? 1.0 : 0.0;          // pass number `passes` ran and flagged nothing
  st[5] = 0.0;
}

template <int R>
void launch_pass(int kind, dim3 grid, hipStream_t st, const float* image, const double* params, const uint8_t* mask_in, uint8_t* mask_out,
                 float* clean, unsigned* counters, int pass, const DespikeArgs& a) {
#define DS_LAUNCH(KIND) \
  hipLaunchKernelGGL((despike_kernel<R, KIND>), grid, dim3(DS_THREADS), 0, st, image, params, mask_in, mask_out, clean, counters, pass, a)
  switch (kind) {
    case DS_DETECT_MODEL: DS_LAUNCH(DS_DETECT_MODEL); break;
    case DS_DETECT_MAD: DS_LAUNCH(DS_DETECT_MAD); break;
    default: DS_LAUNCH(DS_FILL); break;
  }
#undef DS_LAUNCH
}

void launch_radius(int radius, int kind, dim3 grid, hipStream_t st, const float* image, const double* params, const uint8_t* mask_in,
                   uint8_t* mask_out, float* clean, unsigned* counters, int pass, const DespikeArgs& a) {
  switch (radius) {
    case 1: launch_pass<1>(kind, grid, st, image, params, mask_in, mask_out, clean, counters, pass, a); break;
    case 2: launch_pass<2>(kind, grid, st, image, params, mask_in, mask_out, clean, counters, pass, a); break;
    default: launch_pass<3>(kind, grid, st, image, params, mask_in, mask_out, clean, counters, pass, a); break;
  }
}

size_t mask_bytes(int n_planes, int height, int width) { return (((size_t)n_planes * height * width) + 7) / 8 * 8; }

}  // namespace

extern "C" int sunerf_despike_abi_version(void) { return SUNERF_DESPIKE_ABI_VERSION; }

extern "C" size_t sunerf_despike_workspace_bytes(int n_planes, int height, int width, int radius) {
  if (n_planes < 1 || height < 1 || width < 1 || radius < 1 || radius > SUNERF_DESPIKE_MAX_RADIUS) return 0;
  return mask_bytes(n_planes, height, width) + (size_t)n_planes * DS_COUNTERS * sizeof(unsigned);
}

extern "C" int sunerf_despike(const float* image, const uint8_t* bad, const double* params, int n_planes, int height, int width,
                              int radius, int mode, int flags, double n_sigma, double grow_sigma, int min_valid, int max_iterations,
                              float* clean, uint8_t* mask, double* state, void* workspace, void* stream) {
  if (radius > SUNERF_DESPIKE_MAX_RADIUS || max_iterations > SUNERF_DESPIKE_MAX_ITERATIONS || min_valid > SUNERF_DESPIKE_MAX_MIN_VALID)
    return SUNERF_E_UNSUPPORTED;
  if (mode != SUNERF_DESPIKE_MODE_MODEL && mode != SUNERF_DESPIKE_MODE_MAD) return SUNERF_E_UNSUPPORTED;
  if (flags & ~(SUNERF_DESPIKE_TWO_SIDED | SUNERF_DESPIKE_FILL_NAN)) return SUNERF_E_UNSUPPORTED;
  if (n_planes >= 0 && height >= 0 && width >= 0 && radius >= 1 && (n_planes == 0 || height == 0 || width == 0)) return 0;
  if (n_planes < 0 || height < 0 || width < 0 || radius < 1 || min_valid < 1 || max_iterations < 0) return SUNERF_E_BADARG;
  if (!(n_sigma > 0.0) || !(grow_sigma > 0.0) || !(n_sigma < __builtin_inf()) || !(grow_sigma < __builtin_inf())) return SUNERF_E_BADARG;
  if (!image || !params || !clean || !mask || !state || !workspace) return SUNERF_E_BADARG;          // the size is non-zero here
  if ((uintptr_t)params % sizeof(double) || (uintptr_t)state % sizeof(double) || (uintptr_t)workspace % sizeof(double))
    return SUNERF_E_BADARG;
  const int64_t plane_px = (int64_t)height * width;
  const size_t image_bytes = (size_t)n_planes * plane_px * sizeof(float);
  if ((uintptr_t)clean < (uintptr_t)image + image_bytes && (uintptr_t)image < (uintptr_t)clean + image_bytes) return SUNERF_E_BADARG;

  DespikeArgs a;
  a.n_planes = n_planes; a.height = height; a.width = width;
  a.tiles_y = (height + DS_TH - 1) / DS_TH; a.tiles_x = (width + DS_TW - 1) / DS_TW;
  a.flags = flags; a.min_valid = min_valid; a.n_sigma = n_sigma; a.grow_sigma = grow_sigma;
  uint8_t* ws_mask = (uint8_t*)workspace;
  unsigned* counters = (unsigned*)((char*)workspace + mask_bytes(n_planes, height, width));
  // pass k reads buffer k % 2 and writes the other: the last pass writes the workspace's, the fill reads it and writes the caller's
  uint8_t* buffer[2] = {max_iterations % 2 ? mask : ws_mask, max_iterations % 2 ? ws_mask : mask};
  hipStream_t st = (hipStream_t)stream;
  const int64_t chunks_per_plane = (plane_px + DS_START_PX - 1) / DS_START_PX;
  const dim3 grid(grid_of((int64_t)a.tiles_y * a.tiles_x * n_planes));
  SUNERF_CLEAR_ERROR();
  hipError_t e = hipMemsetAsync(counters, 0, (size_t)n_planes * DS_COUNTERS * sizeof(unsigned), st);
  if (e != hipSuccess) return (int)e;
  hipLaunchKernelGGL(despike_start_kernel, dim3(grid_of(chunks_per_plane * n_planes)), dim3(DS_THREADS), 0, st, image, bad, buffer[0],
                     counters, plane_px, chunks_per_plane, chunks_per_plane * n_planes);
  SUNERF_CHECK_LAUNCH();
  for (int pass = 0; pass < max_iterations; ++pass) {
    launch_radius(radius, mode == SUNERF_DESPIKE_MODE_MODEL ? DS_DETECT_MODEL : DS_DETECT_MAD, grid, st, image, params, buffer[pass % 2],
                  buffer[(pass + 1) % 2], (float*)nullptr, counters, pass, a);
    SUNERF_CHECK_LAUNCH();
  }
  launch_radius(radius, DS_FILL, grid, st, image, params, ws_mask, mask, clean, counters, 0, a);
  hipLaunchKernelGGL(despike_state_kernel, dim3((unsigned)((n_planes + 63) / 64)), dim3(64), 0, st, (const unsigned*)counters, state,
                     n_planes, max_iterations);
  SUNERF_CHECK_LAUNCH();
  return 0;
}
