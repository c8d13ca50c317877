// Exact selection in registers, shared by despike.hip (up to 48 neighbours of a pixel) and stack.hip (up to 64 frames of a
// pixel): sorting networks of min / max pairs whose every register index is a constant expression, and a pick at a run-time rank
// that reads every element.  Nothing here indexes an array with a run-time value, so no user of it moves its values to scratch.
#pragma once
#include <utility>

#include "sunerf_common.h"

namespace {

__device__ __forceinline__ void order(float& lo, float& hi) {
  const float a = lo, b = hi;
  lo = __builtin_fminf(a, b);
  hi = __builtin_fmaxf(a, b);
}
__device__ __forceinline__ void order(double& lo, double& hi) {
  const double a = lo, b = hi;
  lo = __builtin_fmin(a, b);
  hi = __builtin_fmax(a, b);
}

// The networks are tables of index pairs built at compile time and applied through a pack expansion: every register index is a
// constant expression, whatever the optimiser makes of loops.
template <int N>
struct Network {
  int n = 0;
  unsigned char lo[N * N] = {}, hi[N * N] = {};
  constexpr void add(int i, int j) { lo[n] = (unsigned char)i; hi[n] = (unsigned char)j; ++n; }
};

// Batcher's odd-even merge sort for any N (Knuth 5.2.2 M), ascending
template <int N>
constexpr Network<N> batcher_network() {
  Network<N> t;
  for (int p = 1; p < N; p *= 2)
    for (int k = p; k >= 1; k /= 2)
      for (int j = k % p; j <= N - 1 - k; j += 2 * k)
        for (int i = 0; i <= (k - 1 < N - j - k - 1 ? k - 1 : N - j - k - 1); ++i)
          if ((i + j) / (2 * p) == (i + j + k) / (2 * p)) t.add(i + j, i + j + k);
  return t;
}

// a bitonic merge of v[0 .. N) padded with +inf to the next power of two: a pair whose upper element is padding is in order already
template <int N>
constexpr Network<N> bitonic_merge_network() {
  Network<N> t;
  int m = 1;
  while (m < N) m *= 2;
  for (int d = m / 2; d >= 1; d /= 2)
    for (int i = 0; i < N; ++i)
      if ((i & d) == 0 && (i | d) < N) t.add(i, i | d);
  return t;
}

template <int N>
struct Networks {
  static constexpr Network<N> SORT = batcher_network<N>();
  static constexpr Network<N> MERGE = bitonic_merge_network<N>();
  template <size_t... I>
  static __device__ __forceinline__ void sort(float (&v)[N], std::index_sequence<I...>) {
    const int done[] = {(order(v[SORT.lo[I]], v[SORT.hi[I]]), 0)...};
    (void)done;
  }
  template <size_t... I>
  static __device__ __forceinline__ void merge(double (&v)[N], std::index_sequence<I...>) {
    const int done[] = {(order(v[MERGE.lo[I]], v[MERGE.hi[I]]), 0)...};
    (void)done;
  }
};

template <int N>
__device__ __forceinline__ void sort_network(float (&v)[N]) {
  Networks<N>::sort(v, std::make_index_sequence<Networks<N>::SORT.n>{});
}
template <int N>
__device__ __forceinline__ void bitonic_merge(double (&v)[N]) {
  Networks<N>::merge(v, std::make_index_sequence<Networks<N>::MERGE.n>{});
}

// v[rank] for 0 <= rank < N without an index into the registers: every element is read and the one of that rank kept by its bits.
// (Written as a chain of `i == rank ? v[i] : r`, the optimiser turns the chain back into one indexed load and the array moves to
// scratch.)
template <int N>
__device__ __forceinline__ float pick(const float (&v)[N], int rank) {
  unsigned bits = 0;
#pragma unroll
  for (int i = 0; i < N; ++i) bits |= __float_as_uint(v[i]) & (i == rank ? ~0u : 0u);
  return __uint_as_float(bits);
}
template <int N>
__device__ __forceinline__ double pick(const double (&v)[N], int rank) {
  unsigned long long bits = 0;
#pragma unroll
  for (int i = 0; i < N; ++i) bits |= (unsigned long long)__double_as_longlong(v[i]) & (i == rank ? ~0ull : 0ull);
  return __longlong_as_double((long long)bits);
}

}  // namespace
