// D-SSIM of a batch of detector-pixel patches and its gradient (include/sunerf_hip_ssim_loss.h): the
// structural term beside the pixel loss of a patch batch.  One launch gives the SSIM of every coarse and fine plane, both
// gradients and the reduced sums; the gradients are written in the forward, as train_step.hip and likelihood.hip do.
//
// Shape.  The rows of a patch are one contiguous block of P P C floats, channel last.  A workgroup takes one patch and one group
// of its channels: it reads the three blocks with consecutive lanes on consecutive floats and keeps the group's channels as planes
// in LDS (plane stride odd, so that the lanes of one pixel's channels fall on different banks), walks the group's channels, and
// writes the two gradient blocks back the same way.  No lane strides through memory by C.  Where P is so large that not even one
// channel's three fp32 planes fit beside the fp64 working set (from P = 59 at w = 7), a workgroup takes ONE channel, fills the
// working planes from the same coalesced sweep and stores that channel's gradient directly.
//
// Per plane, all in fp64 (every operation rounded on its own, -ffp-contract=off):
//   fill    X, Y [P P]: the (stretched) prediction and target; the plane is valid when every value is finite
//   sums    a work item owns one window column and a strip of window rows: the row sums of x, y, x^2, y^2, x y over the w columns,
//           added over the w rows of the strip's first window, then carried down the strip (add the entering row's sums, take off
//           the leaving row's); per window S and the three coefficients alpha, beta, gamma of d S / d x_p = alpha + beta x_p +
//           gamma y_p go to the maps M [3][W W], W = P - w + 1
//   gather  a work item owns one pixel column and a strip of pixel rows: the zero-padded box sums of the three maps by the same
//           scheme, g_p = (box(alpha) + x_p box(beta) + y_p box(gamma)) / W^2, times s'(x_p) under the stretch.  A gather: no atomics
// The strips and the order inside them are fixed by (P, w) alone, so a plane's SSIM and gradient do not depend on its batch.
//
// Reductions: the SSIM of a plane is the sum of its work items' partial sums by ordered_sum.h's halving tree; a workgroup adds its
// planes in channel order and writes 4 fp64 partials to the workspace; the workgroup that takes the last ticket (ordered_sum.h)
// adds the partials in index order (256 contiguous runs, then the same tree).
#include "sunerf_common.h"
#include "ordered_sum.h"
#include "../../include/sunerf_hip_ssim_loss.h"

#include <cmath>

namespace {

constexpr int SL_THREADS = 256;
constexpr int SL_PARTIAL = 4;                               // sum of ssim coarse, fine; valid planes coarse, fine
constexpr size_t SL_LDS_BUDGET = 160 * 1024 - 4096;         // dynamic LDS: the CU's 160 KiB less the static arrays below and a margin

struct Args {
  const float* coarse; const float* fine; const float* target;
  int64_t n;
  int P, C, w, W;              // W = P - w + 1 windows per side
  int staged, CC, n_groups;    // staged: CC channels per workgroup as fp32 planes in LDS; else one channel, no fp32 planes
  int plane_stride;            // floats between two fp32 planes in LDS: P P | 1
  int a_strips, a_rows;        // sums: strips of window rows per column, window rows per strip
  int b_strips, b_rows;        // gather: strips of pixel rows per column, pixel rows per strip
  double c1, c2;
  int use_asinh; double vmax, a, norm;      // norm = asinh(1 / a)
  float* g_coarse; float* g_fine;
  double* plane_ssim; double* stats;
  void* workspace;
};

__device__ __forceinline__ double stretch(const Args& a, float v) {
  if (!a.use_asinh) return (double)v;
  return asinh((double)v / a.vmax / a.a) / a.norm;
}

// the sum of one value over the workgroup, in every thread, by ordered_sum.h's halving tree
__device__ __forceinline__ double block_sum(double v, double* red) {
  const double one[1] = {v};
  __syncthreads();          // red[0] may still be read by a previous call
  lds_tree<SL_THREADS>(red, one, add_values());
  return red[0];
}

// X or Y of channel c: from the group's fp32 planes, or (one channel per workgroup) from a coalesced sweep of the patch's block.
// Returns whether every value this thread saw was finite.
__device__ __forceinline__ bool fill_plane(const Args& a, double* dst, const float* lds_plane, const float* block, int c) {
  const int pixels = a.P * a.P;
  bool ok = true;
  if (a.staged) {
    for (int p = threadIdx.x; p < pixels; p += SL_THREADS) {
      const float v = lds_plane[p];
      ok = ok && isfinite(v);
      dst[p] = stretch(a, v);
    }
  } else {
    const int total = pixels * a.C;
    for (int i = threadIdx.x; i < total; i += SL_THREADS) {
      const int p = i / a.C;
      if (i - p * a.C != c) continue;
      const float v = block[i];
      ok = ok && isfinite(v);
      dst[p] = stretch(a, v);
    }
  }
  return ok;
}

// sums of x, y, x^2, y^2, x y over the w pixels of row r from column j on
__device__ __forceinline__ void row_sums(const double* X, const double* Y, int P, int w, int r, int j, double* h) {
  const double* x = X + r * P + j;
  const double* y = Y + r * P + j;
  h[0] = 0.0; h[1] = 0.0; h[2] = 0.0; h[3] = 0.0; h[4] = 0.0;
  for (int k = 0; k < w; ++k) {
    const double u = x[k], v = y[k];
    h[0] += u; h[1] += v; h[2] += u * u; h[3] += v * v; h[4] += u * v;
  }
}

// sums of the three maps over the windows jlo .. jhi of window row i
__device__ __forceinline__ void map_sums(const double* M, int W, int i, int jlo, int jhi, double* h) {
  const int maps = W * W;
  const double* m = M + i * W;
  h[0] = 0.0; h[1] = 0.0; h[2] = 0.0;
  for (int j = jlo; j <= jhi; ++j) {
    h[0] += m[j]; h[1] += m[maps + j]; h[2] += m[2 * maps + j];
  }
}

// One valid plane: its SSIM (in every thread) and its gradient, to the fp32 plane `g_lds` or, strided, to `g_block + c`.
__device__ __forceinline__ double plane_ssim_and_gradient(const Args& a, const double* X, const double* Y, double* M, double* red,
                                                          float* g_lds, float* g_block, int c) {
  const int P = a.P, w = a.w, W = a.W, t = threadIdx.x;
  const double N = (double)(w * w), N1 = N - 1.0;
  double s_sum = 0.0;
  {
    const int j = t % W, strip = t / W;
    const int i0 = strip * a.a_rows, i1 = min(W, i0 + a.a_rows);
    if (strip < a.a_strips && i0 < i1) {
      double s[5] = {0.0, 0.0, 0.0, 0.0, 0.0}, h[5];
      for (int r = i0; r < i0 + w; ++r) {
        row_sums(X, Y, P, w, r, j, h);
        for (int k = 0; k < 5; ++k) s[k] += h[k];
      }
      for (int i = i0;; ++i) {
        const double mu_x = s[0] / N, mu_y = s[1] / N;
        const double var_x = (s[2] - N * mu_x * mu_x) / N1, var_y = (s[3] - N * mu_y * mu_y) / N1;
        const double cov = (s[4] - N * mu_x * mu_y) / N1;
        const double A1 = 2.0 * mu_x * mu_y + a.c1, A2 = 2.0 * cov + a.c2;
        const double B1 = mu_x * mu_x + mu_y * mu_y + a.c1, B2 = var_x + var_y + a.c2;
        const double S = A1 * A2 / (B1 * B2);
        const double gamma = 2.0 * A1 / (N1 * B1 * B2);
        const double beta = -2.0 * S / (N1 * B2);
        const double alpha = (2.0 * mu_y / N) * A2 / (B1 * B2) - gamma * mu_y - S * (2.0 * mu_x / N) / B1 - beta * mu_x;
        M[i * W + j] = alpha;
        M[W * W + i * W + j] = beta;
        M[2 * W * W + i * W + j] = gamma;
        s_sum += S;
        if (i + 1 >= i1) break;
        row_sums(X, Y, P, w, i + w, j, h);
        for (int k = 0; k < 5; ++k) s[k] += h[k];
        row_sums(X, Y, P, w, i, j, h);
        for (int k = 0; k < 5; ++k) s[k] -= h[k];
      }
    }
  }
  const double windows = (double)(W * W);
  const double ssim = block_sum(s_sum, red) / windows;          // (its barriers publish M)
  {
    const int q = t % P, strip = t / P;
    const int r0 = strip * a.b_rows, r1 = min(P, r0 + a.b_rows);
    if (strip < a.b_strips && r0 < r1) {
      const int jlo = max(0, q - w + 1), jhi = min(W - 1, q);
      double s[3] = {0.0, 0.0, 0.0}, h[3];
      for (int i = max(0, r0 - w + 1); i <= min(W - 1, r0); ++i) {
        map_sums(M, W, i, jlo, jhi, h);
        for (int k = 0; k < 3; ++k) s[k] += h[k];
      }
      const double d_scale = a.vmax * a.a * a.norm;
      for (int r = r0;; ++r) {
        const int p = r * P + q;
        const double x = X[p], y = Y[p];
        double g = (s[0] + x * s[1] + y * s[2]) / windows;
        // s'(v) = 1 / (sqrt(1 + u^2) vmax a norm) with u = v / vmax / a = sinh(norm s(v)): sqrt(1 + u^2) = cosh(norm s(v))
        if (a.use_asinh) g = g / (cosh(x * a.norm) * d_scale);
        if (g_lds) g_lds[p] = (float)g;
        else g_block[(size_t)p * a.C + c] = (float)g;
        if (r + 1 >= r1) break;
        if (r + 1 <= W - 1) {
          map_sums(M, W, r + 1, jlo, jhi, h);
          for (int k = 0; k < 3; ++k) s[k] += h[k];
        }
        if (r + 1 - w >= 0) {
          map_sums(M, W, r + 1 - w, jlo, jhi, h);
          for (int k = 0; k < 3; ++k) s[k] -= h[k];
        }
      }
    }
  }
  return ssim;
}

__global__ __launch_bounds__(SL_THREADS) void ssim_loss_kernel(Args a) {
  extern __shared__ __attribute__((aligned(16))) double lds[];      // X | Y | M [3][W W] | fp32 planes [3][CC][plane_stride]
  __shared__ double red[SL_THREADS];
  const int P = a.P, C = a.C, pixels = P * P, t = threadIdx.x;
  double* X = lds;
  double* Y = X + pixels;
  double* M = Y + pixels;
  float* planes = (float*)(M + 3 * a.W * a.W);
  const int64_t patch = blockIdx.x / a.n_groups;
  const int group = (int)(blockIdx.x - patch * a.n_groups);
  const int c0 = group * a.CC, c1 = min(C, c0 + a.CC);
  const size_t block_at = (size_t)patch * pixels * C;
  const int total = pixels * C;
  const size_t tensor_stride = (size_t)a.CC * a.plane_stride;
  const float* src[3] = {a.coarse + block_at, a.fine + block_at, a.target + block_at};
  float* dst[2] = {a.g_coarse + block_at, a.g_fine + block_at};

  if (a.staged) {
    for (int i = t; i < total; i += SL_THREADS) {
      const int p = i / C, c = i - p * C;
      if (c < c0 || c >= c1) continue;
      const size_t at = (size_t)(c - c0) * a.plane_stride + p;
#pragma unroll
      for (int k = 0; k < 3; ++k) planes[k * tensor_stride + at] = src[k][i];
    }
    __syncthreads();
  }

  double sum[2] = {0.0, 0.0}, valid[2] = {0.0, 0.0};
  for (int c = c0; c < c1; ++c) {
    const size_t at = (size_t)(c - c0) * a.plane_stride;
    const int y_ok = __syncthreads_and(fill_plane(a, Y, planes + 2 * tensor_stride + at, src[2], c));
    for (int k = 0; k < 2; ++k) {
      float* g_lds = a.staged ? planes + k * tensor_stride + at : nullptr;
      const int x_ok = __syncthreads_and(fill_plane(a, X, g_lds, src[k], c));
      double ssim;
      if (x_ok && y_ok) {
        ssim = plane_ssim_and_gradient(a, X, Y, M, red, g_lds, dst[k], c);
        sum[k] += ssim;
        valid[k] += 1.0;
      } else {
        ssim = __builtin_nan("");
        for (int p = t; p < pixels; p += SL_THREADS) {
          if (g_lds) g_lds[p] = 0.f;
          else dst[k][(size_t)p * C + c] = 0.f;
        }
      }
      if (t == 0) a.plane_ssim[((size_t)k * a.n + patch) * C + c] = ssim;
      __syncthreads();          // X, M and red are free again
    }
  }

  if (a.staged) {
    for (int i = t; i < total; i += SL_THREADS) {
      const int p = i / C, c = i - p * C;
      if (c < c0 || c >= c1) continue;
      const size_t at = (size_t)(c - c0) * a.plane_stride + p;
      dst[0][i] = planes[at];
      dst[1][i] = planes[tensor_stride + at];
    }
  }

  const Ticket ws(a.workspace);
  if (t == 0) {
    double* mine = ws.partial + (size_t)blockIdx.x * SL_PARTIAL;
    mine[0] = sum[0]; mine[1] = sum[1]; mine[2] = valid[0]; mine[3] = valid[1];
  }
  if (!last_block(ws.ticket)) return;
  // every sum in index order: thread t adds a contiguous run of workgroups, the 256 runs are added by the tree
  const unsigned run = (gridDim.x + SL_THREADS - 1) / SL_THREADS;
  const unsigned b0 = min((unsigned)t * run, gridDim.x), b1 = min(b0 + run, gridDim.x);
  double s[SL_PARTIAL] = {0.0, 0.0, 0.0, 0.0};
  const volatile double* p = ws.seen();
  for (unsigned b = b0; b < b1; ++b)
    for (int k = 0; k < SL_PARTIAL; ++k) s[k] += p[(size_t)b * SL_PARTIAL + k];
  for (int k = 0; k < SL_PARTIAL; ++k) s[k] = block_sum(s[k], red);
  if (t == 0) {
    const double planes_per_image = (double)a.n * (double)C;
    a.stats[0] = s[2] > 0.0 ? 1.0 - s[0] / s[2] : 0.0;
    a.stats[1] = s[3] > 0.0 ? 1.0 - s[1] / s[3] : 0.0;
    a.stats[2] = s[2] + s[3];
    a.stats[3] = 2.0 * planes_per_image - (s[2] + s[3]);
    ws.rearm();
  }
}

size_t working_bytes(int P, int W) { return (2 * (size_t)P * P + 3 * (size_t)W * W) * sizeof(double); }

}  // namespace

extern "C" int sunerf_ssim_loss_abi_version(void) { return SUNERF_SSIM_LOSS_ABI_VERSION; }

extern "C" size_t sunerf_ssim_loss_workspace_bytes(int64_t n, int C) {
  if (n < 1 || C < 1 || C > SUNERF_SSIM_LOSS_MAX_CHANNELS) return 0;
  if (n > (int64_t)0x7fffffff / C) return 0;          // one workgroup per patch and channel at the most: the grid is 32 bits
  return Ticket::bytes((size_t)n * C * SL_PARTIAL);
}

extern "C" int sunerf_ssim_loss(const float* coarse, const float* fine, const float* target, int64_t n, int P, int C, int window,
                                double data_range, double vmax, double a, int use_asinh, float* g_coarse, float* g_fine,
                                double* plane_ssim, double* stats, void* workspace, size_t workspace_bytes, void* stream) {
  if (window < SUNERF_SSIM_LOSS_MIN_WINDOW || window > SUNERF_SSIM_LOSS_MAX_WINDOW || window % 2 == 0) return SUNERF_E_UNSUPPORTED;
  if (P < window || P > SUNERF_SSIM_LOSS_MAX_PATCH || C < 1 || C > SUNERF_SSIM_LOSS_MAX_CHANNELS) return SUNERF_E_UNSUPPORTED;
  if (!finite_positive(data_range)) return SUNERF_E_UNSUPPORTED;
  if (use_asinh && (!finite_positive(vmax) || !finite_positive(a))) return SUNERF_E_UNSUPPORTED;
  if (n == 0) return 0;
  if (n < 0 || n > (int64_t)0x7fffffff / C) return SUNERF_E_BADARG;
  if (!coarse || !fine || !target || !g_coarse || !g_fine || !plane_ssim || !stats || !workspace) return SUNERF_E_BADARG;
  if ((((uintptr_t)plane_ssim) & 7) != 0 || (((uintptr_t)stats) & 7) != 0 || (((uintptr_t)workspace) & 7) != 0) return SUNERF_E_BADARG;
  if (workspace_bytes < sunerf_ssim_loss_workspace_bytes(n, C)) return SUNERF_E_WORKSPACE;
  Args k;
  k.coarse = coarse; k.fine = fine; k.target = target; k.n = n; k.P = P; k.C = C; k.w = window; k.W = P - window + 1;
  k.plane_stride = (P * P) | 1;
  // as many channels per workgroup as LDS holds, spread evenly over the groups; none: one channel per workgroup, no fp32 planes
  const size_t base = working_bytes(P, k.W), per_channel = 3 * (size_t)k.plane_stride * sizeof(float);
  const int fit = base + per_channel <= SL_LDS_BUDGET ? (int)((SL_LDS_BUDGET - base) / per_channel) : 0;
  k.staged = fit > 0;
  if (k.staged) {
    k.n_groups = (C + fit - 1) / fit;
    k.CC = (C + k.n_groups - 1) / k.n_groups;
  } else {
    k.n_groups = C;
    k.CC = 1;
  }
  const size_t lds = base + (k.staged ? (size_t)k.CC * per_channel : 0);
  if (lds > SL_LDS_BUDGET) return SUNERF_E_UNSUPPORTED;          // (no shape within the limits above comes here)
  k.a_strips = SL_THREADS / k.W < k.W ? SL_THREADS / k.W : k.W;
  k.a_rows = (k.W + k.a_strips - 1) / k.a_strips;
  k.b_strips = SL_THREADS / P < P ? SL_THREADS / P : P;
  k.b_rows = (P + k.b_strips - 1) / k.b_strips;
  k.c1 = (0.01 * data_range) * (0.01 * data_range);
  k.c2 = (0.03 * data_range) * (0.03 * data_range);
  k.use_asinh = use_asinh ? 1 : 0;
  k.vmax = use_asinh ? vmax : 1.0;
  k.a = use_asinh ? a : 1.0;
  k.norm = use_asinh ? std::asinh(1.0 / a) : 1.0;
  k.g_coarse = g_coarse; k.g_fine = g_fine; k.plane_ssim = plane_ssim; k.stats = stats; k.workspace = workspace;
  if (lds > 48 * 1024) {
    hipError_t e = hipFuncSetAttribute((const void*)ssim_loss_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    if (e != hipSuccess) return (int)e;
  }
  SUNERF_CLEAR_ERROR();
  hipLaunchKernelGGL(ssim_loss_kernel, dim3((unsigned)(n * k.n_groups)), dim3(SL_THREADS), lds, (hipStream_t)stream, k);
  SUNERF_CHECK_LAUNCH();
  return 0;
}
