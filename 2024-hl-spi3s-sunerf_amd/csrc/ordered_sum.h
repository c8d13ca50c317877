// Sums over a workgroup and over a grid whose order of addition is fixed, so that reruns give the same bits and a plane or image
// scored alone gives the bits it has inside a batch.  No floating-point atomics anywhere: a workgroup
// adds in one fixed tree and writes fp64 partials, and a second stage adds the partials in index order -- a second launch, or
// the workgroup that draws the last ticket.  Each order of addition below is part of its callers' bits and of their NumPy
// restatements under tests/: changing one changes results.  The accumulating side (red[t], the running sum) is always the LEFT
// operand, as `+=` has it, so that a NaN result keeps the payload it had.  (The 32- and 64-lane shuffle sums are ray_scan.h's.)
//
//   lds_tree        the halving tree over THREADS work items in LDS               metrics, volume, reprojection, ssim_loss, enhance,
//                                                                                 deconvolve (control)
//   sum64_dpp       a 64-lane tree whose levels 3 and 4 pair MIRRORED lanes       likelihood
//   wave totals     lane 0 of each wave parks, the totals are added in wave order train_step, likelihood, dt, deconvolve (ratio)
//   Ticket          the last-workgroup protocol and its workspace                 train_step (loss, norm), likelihood, ssim_loss
//
// Kept outside: the per-row ballot walk and the two-level group sum of likelihood.hip, ssim_loss.hip's contiguous-run pass and
// every kernel's own choice of what its last workgroup adds in which order; the float atomics and 32-lane sums of dt_sweep.h;
// the wave tree of deconvolve.hip's ratio kernel, sum64's order written as one loop over two values (two sum64 calls put one
// shuffle chain behind the other and measured 1 % on an iteration).
#pragma once
#include "ray_scan.h"

// ---- the LDS halving tree --------------------------------------------------------------------------------------------------------
// K values per work item, value k of item t at red[k * THREADS + t].  Level s = THREADS/2, THREADS/4, ... 1 pairs item t < s with
// item t + s:  red[t] = op(k, red[t], red[t + s]).  The result of value k is red[k * THREADS].
// Barriers: the tree owns the one between its stores and the first level and the one after every level, the last included, so
// every thread may read the results when it returns.  It owns NO leading barrier and none after the results are read: a caller
// whose `red` may still be read (an earlier result, an aliased array) places that one barrier itself and says why.
struct add_values {
  template <class T>
  __device__ __forceinline__ T operator()(int, T acc, T other) const { return acc + other; }
};
template <int THREADS, int K, class T, class Op>
__device__ __forceinline__ void lds_tree(T* red, const T (&v)[K], Op op) {
  const int t = threadIdx.x;
#pragma unroll
  for (int k = 0; k < K; ++k) red[k * THREADS + t] = v[k];
  __syncthreads();
  for (int s = THREADS / 2; s > 0; s >>= 1) {
    if (t < s) {
#pragma unroll
      for (int k = 0; k < K; ++k) red[k * THREADS + t] = op(k, red[k * THREADS + t], red[k * THREADS + t + s]);
    }
    __syncthreads();
  }
}

// ---- a 64-lane tree by data-parallel moves ---------------------------------------------------------------------------------------
// One level as a DPP move (no trip through the LDS crossbar): every lane reads its partner of CTRL.
template <int CTRL>
__device__ __forceinline__ double dpp_partner(double v) {
  const unsigned long long u = __builtin_bit_cast(unsigned long long, v);
  const int lo = __builtin_amdgcn_update_dpp(0, (int)(unsigned)u, CTRL, 0xF, 0xF, false);
  const int hi = __builtin_amdgcn_update_dpp(0, (int)(unsigned)(u >> 32), CTRL, 0xF, 0xF, false);
  return __builtin_bit_cast(double, ((unsigned long long)(unsigned)hi << 32) | (unsigned long long)(unsigned)lo);
}
// The sum over the 64 lanes, in every lane: partners 1 and 2 lanes apart (quad permutes), the other quad of the group of 8
// (row_half_mirror: lane i with 7 - i), the other half of the row of 16 (row_mirror: i with 15 - i), then the rows 16 and 32
// lanes apart.  NOT sum64: that one goes 32, 16, ... 1 and pairs i with i ^ d at every level.  Both partners of a level add the
// same two numbers, so all lanes of a group hold the same bits.  Needs every lane active.
__device__ __forceinline__ double sum64_dpp(double v) {
  v += dpp_partner<0xB1>(v);       // quad_perm [1, 0, 3, 2]
  v += dpp_partner<0x4E>(v);       // quad_perm [2, 3, 0, 1]
  v += dpp_partner<0x141>(v);      // row_half_mirror
  v += dpp_partner<0x140>(v);      // row_mirror
  v += __shfl_xor(v, 16);
  v += __shfl_xor(v, 32);
  return v;
}

// ---- the waves in wave order -----------------------------------------------------------------------------------------------------
// The wave tree is the caller's choice (sum64, sum64_dpp).  Lane 0 of each wave parks the wave's K totals at sh[wave * K + k];
// after a barrier, value k's total is 0 + sh[k] + sh[K + k] + ... in wave order 0 .. WAVES-1.  (The leading 0 changes no word a
// caller can form: it would turn a total of -0.0 into +0.0, and every caller's lane values start from +0.0.)
template <int K, class T>
__device__ __forceinline__ void park_wave_totals(const T (&wave_total)[K], T* sh) {
  if ((threadIdx.x & 63) == 0) {
#pragma unroll
    for (int k = 0; k < K; ++k) sh[(threadIdx.x >> 6) * K + k] = wave_total[k];
  }
}
template <int WAVES, int K, class T>
__device__ __forceinline__ T sum_in_wave_order(const T* sh, int k) {
  T t = 0;
#pragma unroll
  for (int w = 0; w < WAVES; ++w) t += sh[w * K + k];
  return t;
}
// Both around their barrier, for one value, the total in every thread.  Owns the barrier between parking and adding; the caller
// owns the one before, where sh may still be read by an earlier call.
template <int WAVES, class T>
__device__ __forceinline__ T wave_order_sum(T wave_total, T* sh) {
  const T v[1] = {wave_total};
  park_wave_totals(v, sh);
  __syncthreads();
  return sum_in_wave_order<WAVES, 1>(sh, 0);
}

// ---- the last-workgroup ticket ---------------------------------------------------------------------------------------------------
// A reduction over a grid in ONE launch.  Workspace: an unsigned ticket at byte 0 (zero before the first launch), fp64 partials
// from byte 64.  Every workgroup writes its partials with plain stores and calls last_block():
//   __threadfence()        this thread's partials are visible device-wide before anything that follows
//   __syncthreads()        ... and that holds for every thread of the workgroup before thread 0 draws
//   atomicAdd(ticket, 1)   thread 0 draws; the workgroup that draws gridDim.x - 1 is the last: every other one has drawn, so has
//                          fenced all of its partials
//   __syncthreads()        the answer reaches the workgroup through LDS
//   __threadfence()        in the last workgroup only: its reads of the partials are not moved above the draw
// The last workgroup then reads the partials through seen() -- volatile, so that no load is served from a register or a line
// fetched before the draw -- adds them in an order of its own that depends on nothing but (gridDim.x, threadIdx.x), and its
// thread 0 ends with rearm(): the next launch ON THE SAME STREAM finds the ticket at zero without a memset.  One workspace
// serves one stream at a time.
struct Ticket {
  unsigned* ticket;
  double* partial;
  __host__ __device__ explicit Ticket(void* workspace) : ticket((unsigned*)workspace), partial((double*)((char*)workspace + 64)) {}
  static __host__ __device__ constexpr size_t bytes(size_t n_partials) { return 64 + n_partials * sizeof(double); }
  __device__ __forceinline__ const volatile double* seen() const { return partial; }
  __device__ __forceinline__ void rearm() const { *ticket = 0; }
};
// true for exactly one workgroup of the grid: the one that finishes last
__device__ __forceinline__ bool last_block(unsigned* ticket) {
  __shared__ unsigned last;
  __threadfence();
  __syncthreads();
  if (threadIdx.x == 0) last = atomicAdd(ticket, 1u) == gridDim.x - 1 ? 1u : 0u;
  __syncthreads();
  if (last) __threadfence();
  return last != 0;
}
