// Image enhancement: multi-scale Gaussian normalisation (MGN), ring statistics and the normalising radial
// graded filter (NRGF).  Definitions, formulas and argument rules: include/sunerf_hip_enhance.h.
//   mgn_prep_kernel      validity, the cleaned plane (NaN at an invalid pixel), n_invalid, minimum and maximum (integer atomics on
//                        order-preserving keys)
//   mgn_params_kernel    one lane per plane: lo, hi, floor^2
//   mgn_conv_kernel      the separable convolution, one instantiation per pass: <row>, <column, r = x - G>, <column, t_i and the
//                        accumulator, out at the last scale>.  A workgroup stages its tile plus halo in LDS with the edge rule
//                        applied, so that the tap loop has no bounds; each lane forms V adjacent outputs (8 along a row, 16 along a
//                        column) from a window of V staged values at a time, V x V fused multiply-adds per V LDS reads.  The taps
//                        are a kernel argument by value, indexed uniformly: they arrive through the scalar cache.  In a plane
//                        with an invalid pixel (n_invalid of the plane, uniform over the workgroup) the same loop runs a second
//                        time over the mask.
//   ring_statistics_kernel  one workgroup per ring and plane; per row the ring's one or two column intervals from a root estimate
//                        widened by two pixels, membership by the exact rule.  n_segments == 1: a wave per row, per-lane sums, a
//                        fixed tree over the lanes; n_segments > 1: the workgroup per row, 256 staged pixels at a time, the lane
//                        that owns a segment adds its pixels in staged order.  Two passes: count, sum, min, max; then squares.
//   nrgf_apply_kernel    one lane per pixel, its ring by bisection on edges^2
// No floating-point atomics; every sum has an order fixed by the shape.
#include "sunerf_common.h"
#include "ordered_sum.h"
#include "../../include/sunerf_hip.h"
#include "../../include/sunerf_hip_enhance.h"

#include <math.h>

namespace {

constexpr int kMaxR = SUNERF_ENHANCE_MAX_RADIUS;
constexpr int kPad = 16;                               // zero taps before the first weight: the widest V
constexpr int kTable = 2 * kMaxR + 2 * kPad + 16;      // t[q] = w_(q - kPad - R), 0 elsewhere
struct Taps { float t[kTable]; };

struct PlaneParams { unsigned min_inv, max_key; float lo, hi, floor2, unused[3]; };      // 32 bytes per plane at the head of the workspace

__device__ __forceinline__ bool finite_bits(float v) { return (__float_as_uint(v) & 0x7f800000u) != 0x7f800000u; }
__device__ __forceinline__ float nan32() { return __uint_as_float(0x7fc00000u); }
__device__ __forceinline__ double nan64() { return __longlong_as_double(0x7ff8000000000000LL); }
// order-preserving map of a finite fp32 onto unsigned
__device__ __forceinline__ unsigned order_key(float v) {
  const unsigned b = __float_as_uint(v);
  return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}
__device__ __forceinline__ float key_value(unsigned k) { return __uint_as_float((k & 0x80000000u) ? (k & 0x7fffffffu) : ~k); }

__global__ __launch_bounds__(256) void mgn_prep_kernel(const float* __restrict__ image, const uint8_t* __restrict__ bad, int64_t plane,
                                                        float* __restrict__ xc, PlaneParams* pp, unsigned long long* state) {
  __shared__ unsigned s_min, s_max, s_inv;
  const int t = threadIdx.x, p = blockIdx.y;
  if (t == 0) { s_min = 0u; s_max = 0u; s_inv = 0u; }
  __syncthreads();
  unsigned mn = 0u, mx = 0u, inv = 0u;
  const int64_t base = (int64_t)p * plane;
  for (int64_t i = (int64_t)blockIdx.x * 256 + t; i < plane; i += (int64_t)gridDim.x * 256) {
    const float v = image[base + i];
    const bool ok = finite_bits(v) && !(bad && bad[base + i]);
    if (ok) {
      const unsigned key = order_key(v);
      mn = max(mn, ~key); mx = max(mx, key);
    } else {
      ++inv;
    }
    xc[base + i] = ok ? v : nan32();
  }
  if (mn) atomicMax(&s_min, mn);
  if (mx) atomicMax(&s_max, mx);
  if (inv) atomicAdd(&s_inv, inv);
  __syncthreads();
  if (t == 0) {
    if (s_min) atomicMax(&pp[p].min_inv, s_min);
    if (s_max) atomicMax(&pp[p].max_key, s_max);
    if (s_inv) atomicAdd(state + (int64_t)p * SUNERF_ENHANCE_MGN_STATE, (unsigned long long)s_inv);
  }
}

__global__ __launch_bounds__(64) void mgn_params_kernel(PlaneParams* pp, int n_planes, int64_t plane, const float* lo, const float* hi,
                                                         const float* floor, float* lo_out, float* hi_out, const unsigned long long* state) {
  const int p = blockIdx.x * 64 + threadIdx.x;
  if (p >= n_planes) return;
  const bool any = state[(int64_t)p * SUNERF_ENHANCE_MGN_STATE] < (unsigned long long)plane;
  float l = nan32(), h = nan32();
  if (any) {
    l = lo ? lo[p] : key_value(~pp[p].min_inv) + 0.f;
    h = hi ? hi[p] : key_value(pp[p].max_key) + 0.f;
  }
  const float fl = floor ? floor[p] : ldexpf(fmaxf(fabsf(l), fabsf(h)), -16);
  pp[p].lo = l; pp[p].hi = h; pp[p].floor2 = fl * fl;
  lo_out[p] = l; hi_out[p] = h;
}

enum { EP_ROW = 0, EP_R = 1, EP_T = 2 };

struct ConvArgs {
  const float* src;      // row pass: the cleaned plane or r; column pass: the row sums
  const float* srcm;     // column pass: the row sums of the mask
  float* dst;            // row pass: row sums; EP_R: r; EP_T: the accumulator, which is `out`
  float* dstm;           // row pass: row sums of the mask
  const float* xc;       // the cleaned plane (epilogues)
  const float* r;        // EP_T
  const PlaneParams* pp;
  unsigned long long* state;
  int H, W, R, P;        // P: tap positions of a lane, 2 R + V rounded up to a multiple of V
  float inv_norm;        // fp32(1 / (sum w)^2)
  int square;            // row pass: square the value as it is loaded
  float k, weight, h, c, eg;
  int first, last;
};

template <int V, int ST>
__device__ __forceinline__ void tap_sum(const float* lane, const Taps& taps, int P, float (&acc)[V]) {
#pragma unroll
  for (int v = 0; v < V; ++v) acc[v] = 0.f;
  for (int p0 = 0; p0 < P; p0 += V) {
    float val[V];
#pragma unroll
    for (int u = 0; u < V; ++u) val[u] = lane[(p0 + u) * ST];
#pragma unroll
    for (int u = 0; u < V; ++u) {
#pragma unroll
      for (int v = 0; v < V; ++v) acc[v] = __builtin_fmaf(taps.t[p0 + u - v + kPad], val[u], acc[v]);
    }
  }
}

template <bool COL, int EP>
__global__ __launch_bounds__(256) void mgn_conv_kernel(ConvArgs a, Taps taps) {
  constexpr int V = COL ? 16 : 8;
  constexpr int LC = COL ? 8 : 64, LO = COL ? 32 : 4;      // lanes along and across the convolution axis
  constexpr int NC = LC * V;                               // outputs of the workgroup along the axis: 128 rows or 512 columns
  constexpr int LEN = NC + 2 * kMaxR + V;                  // staged positions along the axis
  __shared__ __attribute__((aligned(16))) float tile[LEN * LO];
  __shared__ unsigned tally[2];
  const int t = threadIdx.x, p = blockIdx.z;
  const int64_t plane = (int64_t)a.H * a.W, base = (int64_t)p * plane;
  const bool masked = a.state[(int64_t)p * SUNERF_ENHANCE_MGN_STATE] != 0ull;      // uniform over the workgroup
  const int lc = COL ? t >> 5 : t & 63, lo = COL ? t & 31 : t >> 6;
  const int c0 = (int)(COL ? blockIdx.y : blockIdx.x) * NC, o0 = (int)(COL ? blockIdx.x : blockIdx.y) * LO;
  const int n_c = COL ? a.H : a.W, n_o = COL ? a.W : a.H;
  const int used = NC - V + a.P;                           // <= LEN - 1
  if (EP == EP_T && t < 2) tally[t] = 0u;
  float num[V], den[V];
#pragma unroll
  for (int v = 0; v < V; ++v) den[v] = 1.f;
  const int phases = masked ? 2 : 1;
  for (int phase = 0; phase < phases; ++phase) {
    if (phase) __syncthreads();
    if (COL) {
      const float* src = (phase ? a.srcm : a.src) + base;
      const int x = min(o0 + lo, n_o - 1);
      for (int i = lc; i < used; i += LC) {
        const int y = min(max(c0 - a.R + i, 0), n_c - 1);
        tile[i * LO + lo] = src[(int64_t)y * a.W + x];
      }
    } else {
      const float* src = a.src + base;
      for (int row = 0; row < LO; ++row) {
        const int64_t line = (int64_t)min(o0 + row, n_o - 1) * a.W;
        for (int i = t; i < used; i += 256) {
          const int x = min(max(c0 - a.R + i, 0), n_c - 1);
          float v = src[line + x];
          const bool ok = finite_bits(v);
          if (a.square) v *= v;
          if (masked) v = phase ? (ok ? 1.f : 0.f) : (ok ? v : 0.f);
          tile[row * LEN + i] = v;
        }
      }
    }
    __syncthreads();
    const float* lane = COL ? tile + (lc * V) * LO + lo : tile + lo * LEN + lc * V;
    if (phase == 0) tap_sum<V, COL ? LO : 1>(lane, taps, a.P, num);
    else tap_sum<V, COL ? LO : 1>(lane, taps, a.P, den);
  }
  const PlaneParams pp = a.pp[p];
  unsigned below = 0u, above = 0u;
#pragma unroll
  for (int v = 0; v < V; ++v) {
    const int y = COL ? c0 + lc * V + v : o0 + lo, x = COL ? o0 + lo : c0 + lc * V + v;
    if (y >= a.H || x >= a.W) continue;
    const int64_t at = base + (int64_t)y * a.W + x;
    if (EP == EP_ROW) {
      a.dst[at] = num[v];
      if (masked) a.dstm[at] = den[v];
      continue;
    }
    const float G = masked ? num[v] / den[v] : num[v] * a.inv_norm;
    if (EP == EP_R) {
      a.dst[at] = a.xc[at] - G;
      continue;
    }
    const float s = sqrtf(G + pp.floor2);
    const float ti = s == 0.f ? 0.f : atanf(a.k * a.r[at] / s);
    float sum = a.weight * ti;
    if (!a.first) sum = a.dst[at] + sum;
    if (a.last) {
      const float xv = a.xc[at];
      if (!finite_bits(xv)) {
        sum = nan32();
      } else {
        float g = 0.f;
        if (pp.hi > pp.lo) g = powf(fminf(fmaxf((xv - pp.lo) / (pp.hi - pp.lo), 0.f), 1.f), a.eg);
        sum = a.h * g + a.c * sum;
        below += xv < pp.lo; above += xv > pp.hi;
      }
    }
    a.dst[at] = sum;
  }
  if (EP == EP_T && a.last) {
    __syncthreads();
    if (below) atomicAdd(&tally[0], below);
    if (above) atomicAdd(&tally[1], above);
    __syncthreads();
    if (t < 2 && tally[t]) atomicAdd(a.state + (int64_t)p * SUNERF_ENHANCE_MGN_STATE + 1 + t, (unsigned long long)tally[t]);
  }
}

// ---- ring statistics ------------------------------------------------------------------------------------------------------------
struct RadialArgs {
  const float* image; const uint8_t* bad;
  int H, W;
  double cy, cx;
  const double* edges;
  int n_rings, S;
  long long* count; double* mean; double* std; double* mn; double* mx;
};

// the columns of row y that can lie in [e0sq, e1sq): up to two closed intervals, each two pixels wider than the root estimate
__device__ __forceinline__ int row_intervals(const RadialArgs& a, double e0sq, double e1sq, int y, int (&xs)[2], int (&xe)[2]) {
  const double dy = (double)y - a.cy, dy2 = dy * dy;
  const double hi2 = e1sq - dy2;
  if (!(hi2 > 0.)) return 0;
  const double last = (double)(a.W - 1);
  const double xo = sqrt(hi2);
  const double left = fmax(a.cx - xo - 2., 0.), right = fmin(a.cx + xo + 2., last);
  if (!(left <= right)) return 0;
  xs[0] = (int)floor(left); xe[0] = (int)ceil(right);
  const double lo2 = e0sq - dy2;
  if (!(lo2 > 0.)) return 1;
  const double xi = sqrt(lo2);
  const double gap_l = a.cx - xi + 2., gap_r = a.cx + xi - 2.;
  if (!(gap_r - gap_l > 2.)) return 1;
  int n = 0;
  if (gap_l >= left) { xs[n] = (int)floor(left); xe[n] = (int)ceil(fmin(gap_l, right)); ++n; }
  if (gap_r <= right) { xs[n] = (int)floor(fmax(gap_r, left)); xe[n] = (int)ceil(right); ++n; }
  return n;
}

__device__ __forceinline__ bool in_ring(const RadialArgs& a, double e0sq, double e1sq, int y, int x, double& dy, double& dx) {
  dy = (double)y - a.cy; dx = (double)x - a.cx;
  const double d2 = dy * dy + dx * dx;      // -ffp-contract=off: two rounded products, one rounded sum
  return d2 >= e0sq && d2 < e1sq;
}

__device__ __forceinline__ void ring_rows(const RadialArgs& a, double e1, int& y0, int& y1) {
  y0 = (int)floor(fmax(a.cy - e1 - 2., 0.));
  y1 = (int)ceil(fmin(a.cy + e1 + 2., (double)(a.H - 1)));      // y0 > y1: no row (a NaN compares false and gives row 0 .. 0 at most)
  if (!(a.cy - e1 - 2. <= (double)(a.H - 1)) || !(a.cy + e1 + 2. >= 0.)) { y0 = 1; y1 = 0; }
}

// one value over the workgroup by ordered_sum.h's halving tree, the result in every thread
template <typename T, typename F>
__device__ __forceinline__ T block_reduce(T v, T* red, F f) {
  const T one[1] = {v};
  lds_tree<256>(red, one, f);
  const T r = red[0];
  __syncthreads();          // the next call overwrites red[0]: every thread has read it
  return r;
}

__global__ __launch_bounds__(256) void ring_statistics_kernel(RadialArgs a) {
  __shared__ double red[256];
  const int t = threadIdx.x, ring = blockIdx.x, p = blockIdx.y;
  const double e0 = a.edges[ring], e1 = a.edges[ring + 1];
  const double e0sq = e0 * e0, e1sq = e1 * e1;
  const int64_t base = (int64_t)p * a.H * a.W;
  int y0, y1;
  ring_rows(a, e1, y0, y1);
  const int wave = t >> 6, lane = t & 63;
  unsigned long long cnt = 0ull;
  double sum = 0., mn = INFINITY, mx = -INFINITY, mean = 0., ss = 0.;
  for (int pass = 0; pass < 2; ++pass) {
    for (int y = y0 + wave; y <= y1; y += 4) {
      int xs[2], xe[2];
      const int n = row_intervals(a, e0sq, e1sq, y, xs, xe);
      for (int k = 0; k < n; ++k) {
        for (int x = xs[k] + lane; x <= xe[k]; x += 64) {
          double dy, dx;
          if (!in_ring(a, e0sq, e1sq, y, x, dy, dx)) continue;
          const int64_t at = base + (int64_t)y * a.W + x;
          const float v = a.image[at];
          if (!finite_bits(v) || (a.bad && a.bad[at])) continue;
          if (pass == 0) {
            ++cnt; sum += (double)v; mn = fmin(mn, (double)v); mx = fmax(mx, (double)v);
          } else {
            const double d = (double)v - mean;
            ss += d * d;
          }
        }
      }
    }
    if (pass == 0) {
      cnt = block_reduce(cnt, reinterpret_cast<unsigned long long*>(red), add_values());
      sum = block_reduce(sum, red, add_values());
      mn = block_reduce(mn, red, [](int, double x, double y) { return fmin(x, y); });
      mx = block_reduce(mx, red, [](int, double x, double y) { return fmax(x, y); });
      mean = sum / (double)cnt;
      if (cnt == 0ull) break;
    } else {
      ss = block_reduce(ss, red, add_values());
    }
  }
  if (t == 0) {
    const int64_t b = (int64_t)p * a.n_rings + ring;
    a.count[b] = (long long)cnt;
    a.mean[b] = cnt ? mean : nan64();
    a.std[b] = cnt ? sqrt(ss / (double)cnt) : nan64();
    a.mn[b] = cnt ? mn : nan64();
    a.mx[b] = cnt ? mx : nan64();
  }
}

// n_segments > 1: lane t owns segments t and t + 256
__global__ __launch_bounds__(256) void ring_segment_statistics_kernel(RadialArgs a) {
  __shared__ int sseg[256];
  __shared__ float sval[256];
  const int t = threadIdx.x, ring = blockIdx.x, p = blockIdx.y;
  const double e0 = a.edges[ring], e1 = a.edges[ring + 1];
  const double e0sq = e0 * e0, e1sq = e1 * e1;
  const int64_t base = (int64_t)p * a.H * a.W;
  const double pi = 3.141592653589793, two_pi = 6.283185307179586;
  int y0, y1;
  ring_rows(a, e1, y0, y1);
  unsigned long long cnt[2] = {0ull, 0ull};
  double sum[2] = {0., 0.}, mn[2] = {INFINITY, INFINITY}, mx[2] = {-INFINITY, -INFINITY}, mean[2] = {0., 0.}, ss[2] = {0., 0.};
  for (int pass = 0; pass < 2; ++pass) {
    for (int y = y0; y <= y1; ++y) {
      int xs[2], xe[2];
      const int n = row_intervals(a, e0sq, e1sq, y, xs, xe);
      for (int k = 0; k < n; ++k) {
        for (int xb = xs[k]; xb <= xe[k]; xb += 256) {
          const int x = xb + t;
          int seg = -1;
          float v = 0.f;
          double dy, dx;
          if (x <= xe[k] && in_ring(a, e0sq, e1sq, y, x, dy, dx)) {
            const int64_t at = base + (int64_t)y * a.W + x;
            v = a.image[at];
            if (finite_bits(v) && !(a.bad && a.bad[at])) {
              const double turn = (atan2(dy, dx) + pi) / two_pi * (double)a.S;
              seg = min((int)floor(turn), a.S - 1);
            }
          }
          __syncthreads();
          sseg[t] = seg; sval[t] = v;
          __syncthreads();
          const int staged = min(256, xe[k] - xb + 1);
#pragma unroll
          for (int q = 0; q < 2; ++q) {
            const int mine = t + 256 * q;
            if (mine >= a.S) continue;
            for (int j = 0; j < staged; ++j) {
              if (sseg[j] != mine) continue;
              const double w = (double)sval[j];
              if (pass == 0) {
                ++cnt[q]; sum[q] += w; mn[q] = fmin(mn[q], w); mx[q] = fmax(mx[q], w);
              } else {
                const double d = w - mean[q];
                ss[q] += d * d;
              }
            }
          }
        }
      }
    }
    if (pass == 0) {
      mean[0] = sum[0] / (double)cnt[0]; mean[1] = sum[1] / (double)cnt[1];
    }
  }
#pragma unroll
  for (int q = 0; q < 2; ++q) {
    const int mine = t + 256 * q;
    if (mine >= a.S) continue;
    const int64_t b = ((int64_t)p * a.n_rings + ring) * a.S + mine;
    const bool any = cnt[q] != 0ull;
    a.count[b] = (long long)cnt[q];
    a.mean[b] = any ? mean[q] : nan64();
    a.std[b] = any ? sqrt(ss[q] / (double)cnt[q]) : nan64();
    a.mn[b] = any ? mn[q] : nan64();
    a.mx[b] = any ? mx[q] : nan64();
  }
}

struct NrgfArgs {
  const float* image; const uint8_t* bad;
  int H, W;
  double cy, cx;
  const double* edges;
  int n_rings, keep;
  float missing;
  const long long* count; const double* mean; const double* std;
  float* out; unsigned long long* state;
};

__global__ __launch_bounds__(256) void nrgf_apply_kernel(NrgfArgs a) {
  __shared__ unsigned tally[SUNERF_ENHANCE_NRGF_STATE];
  const int t = threadIdx.x, p = blockIdx.y;
  if (t < SUNERF_ENHANCE_NRGF_STATE) tally[t] = 0u;
  __syncthreads();
  const int64_t plane = (int64_t)a.H * a.W, i = (int64_t)blockIdx.x * 256 + t;
  if (i < plane) {
    const int y = (int)(i / a.W), x = (int)(i - (int64_t)y * a.W);
    const int64_t at = (int64_t)p * plane + i;
    const float v = a.image[at];
    float res;
    if (!finite_bits(v) || (a.bad && a.bad[at])) {
      res = nan32();
      atomicAdd(&tally[0], 1u);
    } else {
      const double dy = (double)y - a.cy, dx = (double)x - a.cx;
      const double d2 = dy * dy + dx * dx;
      const double first = a.edges[0], last = a.edges[a.n_rings];
      if (!(d2 >= first * first && d2 < last * last)) {
        res = a.keep ? v : a.missing;
        atomicAdd(&tally[1], 1u);
      } else {
        int lo = 0, hi = a.n_rings;
        while (hi - lo > 1) {
          const int mid = (lo + hi) >> 1;
          const double e = a.edges[mid];
          if (e * e <= d2) lo = mid; else hi = mid;
        }
        const int64_t b = (int64_t)p * a.n_rings + lo;
        const double sd = a.std[b];
        if (a.count[b] < 2 || !(sd > 0.)) {
          res = 0.f;
          atomicAdd(&tally[2], 1u);
        } else {
          res = (float)(((double)v - a.mean[b]) / sd);
        }
      }
    }
    a.out[at] = res;
  }
  __syncthreads();
  if (t < SUNERF_ENHANCE_NRGF_STATE && tally[t]) atomicAdd(a.state + (int64_t)p * SUNERF_ENHANCE_NRGF_STATE + t, (unsigned long long)tally[t]);
}

inline bool coordinate_ok(double v) { return v >= -1073741824. && v <= 1073741824.; }      // false for NaN
inline size_t align_up(size_t n, size_t a) { return (n + a - 1) / a * a; }
inline size_t params_bytes(int n_planes) { return align_up((size_t)n_planes * sizeof(PlaneParams), 256); }

void launch_statistics(const RadialArgs& a, int n_planes, hipStream_t st) {
  const dim3 grid((unsigned)a.n_rings, (unsigned)n_planes);
  if (a.S == 1) hipLaunchKernelGGL(ring_statistics_kernel, grid, dim3(256), 0, st, a);
  else hipLaunchKernelGGL(ring_segment_statistics_kernel, grid, dim3(256), 0, st, a);
}

}  // namespace

extern "C" int sunerf_enhance_abi_version(void) { return SUNERF_ENHANCE_ABI_VERSION; }

extern "C" size_t sunerf_enhance_mgn_workspace_bytes(int n_planes, int height, int width) {
  if (n_planes < 1 || height < 1 || width < 1) return 0;
  const size_t plane = align_up((size_t)n_planes * height * width * sizeof(float), 256);
  return params_bytes(n_planes) + 4 * plane;
}

extern "C" int sunerf_enhance_mgn(const float* image, const uint8_t* bad, int n_planes, int height, int width, const double* sigma,
                                  const float* weights, int n_scales, double truncate, float k, float gamma, float h, const float* lo,
                                  const float* hi, const float* floor, float* out, float* lo_out, float* hi_out, int64_t* state,
                                  void* workspace, size_t workspace_bytes, void* stream) {
  if (n_scales < 1 || n_scales > SUNERF_ENHANCE_MAX_SCALES) return SUNERF_E_UNSUPPORTED;
  if (!sigma || !is_finite(truncate) || truncate < 0.) return SUNERF_E_BADARG;
  int radius[SUNERF_ENHANCE_MAX_SCALES];
  for (int i = 0; i < n_scales; ++i)
    if (!is_finite(sigma[i]) || sigma[i] < 0.) return SUNERF_E_BADARG;
  for (int i = 0; i < n_scales; ++i) {
    const double r = truncate * sigma[i] + 0.5;
    if (!(r < (double)(kMaxR + 1))) return SUNERF_E_UNSUPPORTED;
    radius[i] = (int)r;
  }
  const bool negative = n_planes < 0 || height < 0 || width < 0;
  if (!negative && (n_planes == 0 || height == 0 || width == 0)) return 0;
  if (negative || n_planes > 65535 || height > SUNERF_ENHANCE_ROW_TILE_Y * 65535) return SUNERF_E_BADARG;
  if (!is_finite(k) || !is_finite(h) || !is_finite(gamma) || !(gamma > 0.f)) return SUNERF_E_BADARG;
  for (int i = 0; weights && i < n_scales; ++i)
    if (!is_finite(weights[i])) return SUNERF_E_BADARG;
  if (!image || !out || !lo_out || !hi_out || !state || !workspace) return SUNERF_E_BADARG;
  if ((uintptr_t)image % 4 || (uintptr_t)out % 4 || (uintptr_t)lo % 4 || (uintptr_t)hi % 4 || (uintptr_t)floor % 4 || (uintptr_t)lo_out % 4 ||
      (uintptr_t)hi_out % 4 || (uintptr_t)state % 8 || (uintptr_t)workspace % 256)
    return SUNERF_E_BADARG;
  if (workspace_bytes < sunerf_enhance_mgn_workspace_bytes(n_planes, height, width)) return SUNERF_E_WORKSPACE;

  hipStream_t st = (hipStream_t)stream;
  const int64_t plane = (int64_t)height * width;
  const size_t plane_bytes = align_up((size_t)n_planes * plane * sizeof(float), 256);
  char* ws = static_cast<char*>(workspace);
  PlaneParams* pp = reinterpret_cast<PlaneParams*>(ws);
  float* xc = reinterpret_cast<float*>(ws + params_bytes(n_planes));
  float* row_sum = reinterpret_cast<float*>(ws + params_bytes(n_planes) + plane_bytes);
  float* row_mask = reinterpret_cast<float*>(ws + params_bytes(n_planes) + 2 * plane_bytes);
  float* r = reinterpret_cast<float*>(ws + params_bytes(n_planes) + 3 * plane_bytes);
  unsigned long long* counters = reinterpret_cast<unsigned long long*>(state);

  SUNERF_CLEAR_ERROR();
  hipError_t e = hipMemsetAsync(pp, 0, params_bytes(n_planes), st);
  if (e != hipSuccess) return (int)e;
  e = hipMemsetAsync(state, 0, (size_t)n_planes * SUNERF_ENHANCE_MGN_STATE * sizeof(int64_t), st);
  if (e != hipSuccess) return (int)e;
  const int64_t chunks = (plane + 2047) / 2048;
  hipLaunchKernelGGL(mgn_prep_kernel, dim3((unsigned)(chunks < 4096 ? chunks : 4096), (unsigned)n_planes), dim3(256), 0, st, image, bad, plane,
                     xc, pp, counters);
  hipLaunchKernelGGL(mgn_params_kernel, dim3((unsigned)((n_planes + 63) / 64)), dim3(64), 0, st, pp, n_planes, plane, lo, hi, floor, lo_out,
                     hi_out, counters);
  SUNERF_CHECK_LAUNCH();

  const dim3 row_grid((unsigned)((width + SUNERF_ENHANCE_ROW_TILE_X - 1) / SUNERF_ENHANCE_ROW_TILE_X),
                      (unsigned)((height + SUNERF_ENHANCE_ROW_TILE_Y - 1) / SUNERF_ENHANCE_ROW_TILE_Y), (unsigned)n_planes);
  const dim3 col_grid((unsigned)((width + SUNERF_ENHANCE_COL_TILE_X - 1) / SUNERF_ENHANCE_COL_TILE_X),
                      (unsigned)((height + SUNERF_ENHANCE_COL_TILE_Y - 1) / SUNERF_ENHANCE_COL_TILE_Y), (unsigned)n_planes);
  ConvArgs a;
  a.srcm = row_mask; a.dstm = row_mask; a.xc = xc; a.r = r; a.pp = pp; a.state = counters; a.H = height; a.W = width;
  a.k = k; a.h = h; a.c = (float)((1.0 - (double)h) / n_scales); a.eg = (float)(1.0 / (double)gamma);
  for (int i = 0; i < n_scales; ++i) {
    const int R = radius[i];
    Taps taps;
    for (int q = 0; q < kTable; ++q) taps.t[q] = 0.f;
    double total = 0.;
    for (int j = -R; j <= R; ++j) {
      const float w = R == 0 ? 1.f : (float)exp(-(double)(j * j) / (2. * sigma[i] * sigma[i]));
      taps.t[kPad + R + j] = w;
      total += (double)w;
    }
    a.R = R; a.inv_norm = (float)(1. / (total * total)); a.weight = weights ? weights[i] : 1.f;
    a.first = i == 0; a.last = i == n_scales - 1;
    const int row_p = (2 * R + 8 + 7) / 8 * 8, col_p = (2 * R + 16 + 15) / 16 * 16;
    // G[x]: rows, then columns with r = x - G
    a.src = xc; a.dst = row_sum; a.square = 0; a.P = row_p;
    hipLaunchKernelGGL((mgn_conv_kernel<false, EP_ROW>), row_grid, dim3(256), 0, st, a, taps);
    a.src = row_sum; a.dst = r; a.P = col_p;
    hipLaunchKernelGGL((mgn_conv_kernel<true, EP_R>), col_grid, dim3(256), 0, st, a, taps);
    // G[r^2]: rows that square r as they load it, then columns with t_i added into `out`
    a.src = r; a.dst = row_sum; a.square = 1; a.P = row_p;
    hipLaunchKernelGGL((mgn_conv_kernel<false, EP_ROW>), row_grid, dim3(256), 0, st, a, taps);
    a.src = row_sum; a.dst = out; a.square = 0; a.P = col_p;
    hipLaunchKernelGGL((mgn_conv_kernel<true, EP_T>), col_grid, dim3(256), 0, st, a, taps);
    SUNERF_CHECK_LAUNCH();
  }
  return 0;
}

extern "C" int sunerf_enhance_radial_statistics(const float* image, const uint8_t* bad, int n_planes, int height, int width, double cy,
                                                double cx, const double* edges, int n_rings, int n_segments, int64_t* count, double* mean,
                                                double* std, double* min, double* max, void* stream) {
  if (n_rings < 1 || n_rings > SUNERF_ENHANCE_MAX_RINGS || n_segments < 1 || n_segments > SUNERF_ENHANCE_MAX_SEGMENTS ||
      n_rings * n_segments > SUNERF_ENHANCE_MAX_BINS)
    return SUNERF_E_UNSUPPORTED;
  const bool negative = n_planes < 0 || height < 0 || width < 0;
  if (!negative && (n_planes == 0 || height == 0 || width == 0)) return 0;
  if (negative || n_planes > 65535 || !coordinate_ok(cy) || !coordinate_ok(cx)) return SUNERF_E_BADARG;
  if (!image || !edges || !count || !mean || !std || !min || !max) return SUNERF_E_BADARG;
  if ((uintptr_t)image % 4 || (uintptr_t)edges % 8 || (uintptr_t)count % 8 || (uintptr_t)mean % 8 || (uintptr_t)std % 8 || (uintptr_t)min % 8 ||
      (uintptr_t)max % 8)
    return SUNERF_E_BADARG;
  RadialArgs a;
  a.image = image; a.bad = bad; a.H = height; a.W = width; a.cy = cy; a.cx = cx; a.edges = edges; a.n_rings = n_rings; a.S = n_segments;
  a.count = reinterpret_cast<long long*>(count); a.mean = mean; a.std = std; a.mn = min; a.mx = max;
  SUNERF_CLEAR_ERROR();
  launch_statistics(a, n_planes, (hipStream_t)stream);
  SUNERF_CHECK_LAUNCH();
  return 0;
}

extern "C" int sunerf_enhance_nrgf(const float* image, const uint8_t* bad, int n_planes, int height, int width, double cy, double cx,
                                   const double* edges, int n_rings, int outside, float missing, int compute, int64_t* count, double* mean,
                                   double* std, double* min, double* max, float* out, int64_t* state, void* stream) {
  if (n_rings < 1 || n_rings > SUNERF_ENHANCE_MAX_RINGS) return SUNERF_E_UNSUPPORTED;
  if (outside != SUNERF_ENHANCE_OUTSIDE_KEEP && outside != SUNERF_ENHANCE_OUTSIDE_MISSING) return SUNERF_E_UNSUPPORTED;
  const bool negative = n_planes < 0 || height < 0 || width < 0;
  if (!negative && (n_planes == 0 || height == 0 || width == 0)) return 0;
  if (negative || n_planes > 65535 || !coordinate_ok(cy) || !coordinate_ok(cx)) return SUNERF_E_BADARG;
  if (!image || !edges || !count || !mean || !std || !out || !state || (compute && (!min || !max))) return SUNERF_E_BADARG;
  if ((uintptr_t)image % 4 || (uintptr_t)out % 4 || (uintptr_t)edges % 8 || (uintptr_t)count % 8 || (uintptr_t)mean % 8 || (uintptr_t)std % 8 ||
      (uintptr_t)min % 8 || (uintptr_t)max % 8 || (uintptr_t)state % 8)
    return SUNERF_E_BADARG;
  hipStream_t st = (hipStream_t)stream;
  SUNERF_CLEAR_ERROR();
  hipError_t e = hipMemsetAsync(state, 0, (size_t)n_planes * SUNERF_ENHANCE_NRGF_STATE * sizeof(int64_t), st);
  if (e != hipSuccess) return (int)e;
  if (compute) {
    RadialArgs s;
    s.image = image; s.bad = bad; s.H = height; s.W = width; s.cy = cy; s.cx = cx; s.edges = edges; s.n_rings = n_rings; s.S = 1;
    s.count = reinterpret_cast<long long*>(count); s.mean = mean; s.std = std; s.mn = min; s.mx = max;
    launch_statistics(s, n_planes, st);
  }
  NrgfArgs a;
  a.image = image; a.bad = bad; a.H = height; a.W = width; a.cy = cy; a.cx = cx; a.edges = edges; a.n_rings = n_rings;
  a.keep = outside == SUNERF_ENHANCE_OUTSIDE_KEEP; a.missing = missing;
  a.count = reinterpret_cast<const long long*>(count); a.mean = mean; a.std = std; a.out = out;
  a.state = reinterpret_cast<unsigned long long*>(state);
  const int64_t plane = (int64_t)height * width;
  hipLaunchKernelGGL(nrgf_apply_kernel, dim3((unsigned)((plane + 255) / 256), (unsigned)n_planes), dim3(256), 0, st, a);
  SUNERF_CHECK_LAUNCH();
  return 0;
}
