// A per-pixel statistic over a stack of up to 64 frames, after an optional iterated clipping against the pixel's own median
// (include/sunerf_hip_stack.h).  One kernel, one lane per pixel: consecutive lanes take consecutive pixels of
// a plane, so each of the n_frames loads of a wave is one coalesced row of 256 bytes and the frame stride is n_planes * height * width.
//
// The samples of a pixel live in registers.  The kernel is instantiated on a padded frame count NP = 4, 8, 16, 32, 64: samples that
// are not valid (not finite, flagged, or past n_frames) enter as +inf beside the count of the valid ones, Batcher's odd-even merge
// sort (sort_network.h, the network of despike.hip) orders them, and from there on the survivors are the run [lo, hi) of the sorted
// registers.  The clipping tests are monotone in the value, so a pass only counts how many survivors fail at either end and moves
// lo and hi; nothing is sorted twice.  The MAD of a pass needs no second sort either: the absolute deviations of an ascending run
// from its median fall and then rise, and with +inf on both sides of the run that is a bitonic sequence (up to a rotation), which
// one bitonic merge in fp64 orders.  Every pick at a run-time rank reads all NP registers (sort_network.h: pick), every loop over
// the registers is unrolled with the range test `lo <= i < hi` as a predicate: no instantiation indexes its registers, none uses
// scratch.
//
// The mask of the samples is written from the two boundary values of the run: the samples are read a second time (the workgroup has
// just read them) rather than kept beside their sorted copies, which would double the registers.  Counts are
// integers, summed per workgroup in LDS and added to the plane's state with integer atomics; there is no floating-point atomic and
// no floating-point sum across threads.  -ffp-contract=off and no explicit fma: every operation is rounded on its own.
#include "sort_network.h"
#include "../../include/sunerf_hip_stack.h"

namespace {

constexpr int ST_THREADS = 256;          // pixels of one plane per workgroup

struct StackArgs {
  int n_frames, n_planes, method, rank, flags, iterations, clip_min, min_valid;
  int64_t plane_px, chunks_per_plane, n_chunks;
  double q, n_sigma;
};

// The workgroup's `n` pixels of one frame or output go through BUFFER instructions: the address of the first pixel is the same on
// every lane and sits in a scalar resource descriptor, the lane's own pixel is the one offset register that all frames share.
// (With per-lane 64-bit pointers every frame's address is a register pair of its own: two more registers per sample.)  The
// descriptor ends after the n pixels: a lane past them would read 0 and write nothing.
__device__ __forceinline__ float load_px(const float* first, int n, unsigned lane) {
  return __uint_as_float(__builtin_amdgcn_raw_buffer_load_b32(make_rsrc(first, 4u * n), (int)(4u * lane), 0, 0));
}
__device__ __forceinline__ uint8_t load_px(const uint8_t* first, int n, unsigned lane) {
  return __builtin_amdgcn_raw_buffer_load_b8(make_rsrc(first, (unsigned)n), (int)lane, 0, 0);
}
__device__ __forceinline__ void store_px(float value, float* first, int n, unsigned lane) {
  __builtin_amdgcn_raw_buffer_store_b32(__float_as_uint(value), make_rsrc(first, 4u * n), (int)(4u * lane), 0, 0);
}
__device__ __forceinline__ void store_px(uint8_t value, uint8_t* first, int n, unsigned lane) {
  __builtin_amdgcn_raw_buffer_store_b8(value, make_rsrc(first, (unsigned)n), (int)lane, 0, 0);
}

// Nothing at run time: the optimiser may not carry an expression of v across this point.  Without it the conversions of the samples
// to fp64 and their differences from the median, which several loops need, are kept in registers between them -- two per sample.
template <int N>
__device__ __forceinline__ void forget(float (&v)[N]) {
#pragma unroll
  for (int k = 0; k < N; ++k) asm volatile("" : "+v"(v[k]));
}

template <int NP, int MODE>
__global__ __launch_bounds__(ST_THREADS) void stack_kernel(const float* __restrict__ frames, const uint8_t* __restrict__ bad,
                                                           const double* __restrict__ params, float* __restrict__ image,
                                                           uint8_t* __restrict__ count, uint8_t* __restrict__ mask,
                                                           unsigned long long* __restrict__ state, StackArgs a) {
  __shared__ unsigned tally[SUNERF_STACK_STATE];          // the workgroup's: rejected, invalid, NaN pixels, most passes
  const float inf = __builtin_inff();
  const double dinf = __builtin_inf();
  const int64_t frame_px = a.plane_px * a.n_planes;
  const bool two_sided = a.flags & SUNERF_STACK_TWO_SIDED;
  for (int64_t chunk = blockIdx.x; chunk < a.n_chunks; chunk += gridDim.x) {
    const int64_t plane = chunk / a.chunks_per_plane;
    const int64_t first_px = (chunk - plane * a.chunks_per_plane) * ST_THREADS;
    // the workgroup's pixels of frame 0, image and count: a base that is the same on every lane plus the lane's own index, so that
    // the address of frame t is a scalar sum and the loads of all frames share one offset register
    const int64_t base = plane * a.plane_px + first_px;
    const unsigned lane = threadIdx.x;
    const int n_px = (int)(a.plane_px - first_px < ST_THREADS ? a.plane_px - first_px : ST_THREADS);
    if (threadIdx.x < SUNERF_STACK_STATE) tally[threadIdx.x] = 0;
    __syncthreads();
    if ((int)lane < n_px) {
      // Every load is issued before any value is looked at, without a branch between them: register t past the last frame loads
      // the last frame again (the same line) and is made +inf afterwards.  The flags come first, as one bit per frame.
      const int last_frame = a.n_frames - 1;
      unsigned long long flagged = 0;
      if (bad) {
        uint8_t b[NP];
#pragma unroll
        for (int t = 0; t < NP; ++t) b[t] = load_px(bad + ((t < last_frame ? t : last_frame) * frame_px + base), n_px, lane);
#pragma unroll
        for (int t = 0; t < NP; ++t) flagged |= (unsigned long long)(b[t] != 0) << t;
      }
      float v[NP];
#pragma unroll
      for (int t = 0; t < NP; ++t) v[t] = load_px(frames + ((t < last_frame ? t : last_frame) * frame_px + base), n_px, lane);
      int n_valid = 0;
#pragma unroll
      for (int t = 0; t < NP; ++t) {
        const bool valid = t < a.n_frames && __builtin_fabsf(v[t]) < inf && !(flagged >> t & 1);
        v[t] = valid ? v[t] : inf;
        n_valid += valid ? 1 : 0;
      }
      sort_network<NP>(v);

      int lo = 0, hi = n_valid, passes = 0;
#pragma unroll 1
      for (int pass = 0; pass < a.iterations; ++pass) {
        const int n = hi - lo;
        if (n < a.clip_min) break;
        forget<NP>(v);          // the NP conversions to fp64 are made again in every pass, not kept in 2 NP registers across the loop
        const double m = 0.5 * ((double)pick<NP>(v, lo + (n - 1) / 2) + (double)pick<NP>(v, lo + n / 2));
        double lim;
        if (MODE == SUNERF_STACK_MODE_MODEL) {
          const double var = params[4 * plane] + params[4 * plane + 1] * (m > 0.0 ? m : 0.0);
          lim = (a.n_sigma * a.n_sigma) * var;
        } else {
          double dev[NP];
#pragma unroll
          for (int k = 0; k < NP; ++k) dev[k] = (k >= lo && k < hi) ? fabs((double)v[k] - m) : dinf;      // +inf, falls, rises, +inf
          bitonic_merge<NP>(dev);
          const double mad = 0.5 * (pick<NP>(dev, (n - 1) / 2) + pick<NP>(dev, n / 2));
          double s = 1.4826 * mad;
          const double floor_ = params[4 * plane + 2];
          s = s > floor_ ? s : floor_;
          lim = a.n_sigma * s;
          forget<NP>(v);          // the tests below form v - m again instead of keeping the NP differences across the merge
        }
        int above = 0, below = 0;
#pragma unroll
        for (int k = 0; k < NP; ++k) {
          const bool in = k >= lo && k < hi;
          const double d = (double)v[k] - m;
          bool up, down;
          if (MODE == SUNERF_STACK_MODE_MODEL) {
            const bool far = d * d > lim;
            up = d > 0.0 && far;
            down = d < 0.0 && far;
          } else {
            up = d > lim;
            down = -d > lim;
          }
          above += (in && up) ? 1 : 0;
          below += (in && down && two_sided) ? 1 : 0;
        }
        if (above + below == 0) break;
        hi -= above;
        lo += below;
        ++passes;
      }

      const int n = hi - lo;
      double r;
      if (a.method == SUNERF_STACK_MEAN) {
        double sum = 0.0;          // (+0.0 + r_0 is r_0 by value)
#pragma unroll
        for (int k = 0; k < NP; ++k) sum = (k >= lo && k < hi) ? sum + (double)v[k] : sum;
        r = sum / (double)n;
      } else {
        int i0, i1;
        double f = 0.5;
        if (a.method == SUNERF_STACK_MEDIAN) {
          i0 = (n - 1) / 2;
          i1 = n / 2;
        } else if (a.method == SUNERF_STACK_PERCENTILE) {
          const double p = a.q / 100.0 * (double)(n - 1);
          const double l = floor(p);
          i0 = (int)l;
          i1 = i0 + 1 < n ? i0 + 1 : i0;
          f = p - l;
        } else {
          i0 = i1 = a.rank >= 0 ? (a.rank < n - 1 ? a.rank : n - 1) : (n + a.rank > 0 ? n + a.rank : 0);
        }
        const double r0 = (double)pick<NP>(v, lo + i0), r1 = (double)pick<NP>(v, lo + i1);
        if (a.method == SUNERF_STACK_MEDIAN) r = 0.5 * (r0 + r1);
        else if (a.method == SUNERF_STACK_PERCENTILE) r = i0 >= n - 1 ? r0 : r0 + f * (r1 - r0);
        else r = r0;
      }
      const bool empty = n < a.min_valid;
      store_px(empty ? __builtin_nanf("") : (float)r, image + base, n_px, lane);
      store_px((uint8_t)n, count + base, n_px, lane);
      if (mask) {
        // n == 0: every valid sample was rejected, and every value lies below +inf
        const float first = n > 0 ? pick<NP>(v, lo) : inf, last = n > 0 ? pick<NP>(v, hi - 1) : -inf;
#pragma unroll 4
        for (int t = 0; t < a.n_frames; ++t) {
          const float x = load_px(frames + (t * frame_px + base), n_px, lane);
          const bool valid = __builtin_fabsf(x) < inf && !(flagged >> t & 1);
          const uint8_t bits = !valid ? SUNERF_STACK_INVALID : ((x < first || x > last) ? SUNERF_STACK_REJECTED : 0);
          store_px(bits, mask + (t * frame_px + base), n_px, lane);
        }
      }
      if (n_valid - n) atomicAdd(&tally[0], (unsigned)(n_valid - n));
      if (a.n_frames - n_valid) atomicAdd(&tally[1], (unsigned)(a.n_frames - n_valid));
      if (empty) atomicAdd(&tally[2], 1u);
      if (passes) atomicMax(&tally[3], (unsigned)passes);
    }
    __syncthreads();
    if (threadIdx.x < SUNERF_STACK_STATE && tally[threadIdx.x]) {
      unsigned long long* st = state + plane * SUNERF_STACK_STATE + threadIdx.x;
      if (threadIdx.x < 3) atomicAdd(st, (unsigned long long)tally[threadIdx.x]);
      else atomicMax(st, (unsigned long long)tally[threadIdx.x]);
    }          // the threads that read the tally are the ones that clear it for the next chunk
  }
}

template <int NP>
void launch_padded(int mode, dim3 grid, hipStream_t st, const float* frames, const uint8_t* bad, const double* params, float* image,
                   uint8_t* count, uint8_t* mask, unsigned long long* state, const StackArgs& a) {
  if (mode == SUNERF_STACK_MODE_MODEL)
    hipLaunchKernelGGL((stack_kernel<NP, SUNERF_STACK_MODE_MODEL>), grid, dim3(ST_THREADS), 0, st, frames, bad, params, image, count, mask, state, a);
  else
    hipLaunchKernelGGL((stack_kernel<NP, SUNERF_STACK_MODE_MAD>), grid, dim3(ST_THREADS), 0, st, frames, bad, params, image, count, mask, state, a);
}

}  // namespace

extern "C" int sunerf_stack_abi_version(void) { return SUNERF_STACK_ABI_VERSION; }

extern "C" int sunerf_stack_combine(const float* frames, const uint8_t* bad, const double* params, int n_frames, int n_planes, int height,
                                    int width, int method, double q, int rank, int mode, int flags, double n_sigma, int iterations,
                                    int clip_min, int min_valid, float* image, uint8_t* count, uint8_t* mask, int64_t* state,
                                    void* stream) {
  if (n_frames > SUNERF_STACK_MAX_FRAMES || iterations > SUNERF_STACK_MAX_ITERATIONS) return SUNERF_E_UNSUPPORTED;
  if (method < SUNERF_STACK_MEAN || method > SUNERF_STACK_RANK) return SUNERF_E_UNSUPPORTED;
  if (mode != SUNERF_STACK_MODE_MODEL && mode != SUNERF_STACK_MODE_MAD) return SUNERF_E_UNSUPPORTED;
  if (flags & ~SUNERF_STACK_TWO_SIDED) return SUNERF_E_UNSUPPORTED;
  if (n_planes >= 0 && height >= 0 && width >= 0 && n_frames >= 1 && (n_planes == 0 || height == 0 || width == 0)) return 0;
  if (n_planes < 0 || height < 0 || width < 0 || n_frames < 1 || iterations < 0 || clip_min < 2 || min_valid < 1) return SUNERF_E_BADARG;
  if (!(n_sigma > 0.0) || !(n_sigma < __builtin_inf())) return SUNERF_E_BADARG;
  if (method == SUNERF_STACK_PERCENTILE && !(q >= 0.0 && q <= 100.0)) return SUNERF_E_BADARG;
  if (!frames || !params || !image || !count || !state) return SUNERF_E_BADARG;
  if ((uintptr_t)params % sizeof(double) || (uintptr_t)state % sizeof(int64_t)) return SUNERF_E_BADARG;
  const int64_t plane_px = (int64_t)height * width;
  // the kernel reads frames and bad while it writes image, count and mask (the samples a second time for the mask)
  const size_t px = (size_t)n_planes * plane_px, samples = px * n_frames;
  const struct { const void* p; size_t bytes; } in[2] = {{frames, samples * sizeof(float)}, {bad, samples}},
                                                  out[3] = {{image, px * sizeof(float)}, {count, px}, {mask, samples}};
  for (const auto& r : in)
    for (const auto& w : out)
      if (r.p && w.p && (uintptr_t)w.p < (uintptr_t)r.p + r.bytes && (uintptr_t)r.p < (uintptr_t)w.p + w.bytes) return SUNERF_E_BADARG;

  StackArgs a;
  a.n_frames = n_frames; a.n_planes = n_planes; a.method = method; a.rank = rank; a.flags = flags;
  a.iterations = iterations; a.clip_min = clip_min; a.min_valid = min_valid;
  a.plane_px = plane_px;
  a.chunks_per_plane = (plane_px + ST_THREADS - 1) / ST_THREADS;
  a.n_chunks = a.chunks_per_plane * n_planes;
  a.q = q; a.n_sigma = n_sigma;
  hipStream_t st = (hipStream_t)stream;
  unsigned long long* counts = (unsigned long long*)state;
  const dim3 grid(grid_of(a.n_chunks));
  if (iterations == 0) mode = SUNERF_STACK_MODE_MODEL;          // no pass runs: the instantiation without the deviations
  SUNERF_CLEAR_ERROR();
  hipError_t e = hipMemsetAsync(state, 0, (size_t)n_planes * SUNERF_STACK_STATE * sizeof(int64_t), st);
  if (e != hipSuccess) return (int)e;
  if (n_frames <= 4) launch_padded<4>(mode, grid, st, frames, bad, params, image, count, mask, counts, a);
  else if (n_frames <= 8) launch_padded<8>(mode, grid, st, frames, bad, params, image, count, mask, counts, a);
  else if (n_frames <= 16) launch_padded<16>(mode, grid, st, frames, bad, params, image, count, mask, counts, a);
  else if (n_frames <= 32) launch_padded<32>(mode, grid, st, frames, bad, params, image, count, mask, counts, a);
  else launch_padded<64>(mode, grid, st, frames, bad, params, image, count, mask, counts, a);
  SUNERF_CHECK_LAUNCH();
  return 0;
}
