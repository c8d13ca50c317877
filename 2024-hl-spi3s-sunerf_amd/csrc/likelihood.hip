// The Gaussian noise likelihood of the detector model as the training loss: where train_step.hip's loss_kernel
// weighs every pixel alike (sunerf/model/sunerf.py:105-125, :187-191), this one divides every squared residual by the variance the
// instrument's error model gives that pixel (sunerf_hip/instrument.py: Instrument.errors), and multiplies the prediction of every
// table row by a trainable calibration gain first.  One HBM-bound kernel, 16 to 20 bytes per slot; the arithmetic is fp64
// throughout (free next to the traffic) and rounded to fp32 once, at the store.
//
// Reductions.  A ray's codes row may differ from its neighbour's (an ObservationSet mixes instruments), so the lanes of a wave hold
// different table rows.  Per sweep a wave walks the distinct rows its lanes hold (ballot on row == row of the first lane not yet
// served), reduces the four sums of the matching lanes with one fixed tree (ordered_sum.h's sum64_dpp; the others add +0.0), and
// lane 0 adds the result to the wave's own fp64 [row][4] array in LDS.  A workgroup adds its waves' arrays in wave order and
// writes [row][5] partials to the workspace; the workgroup that takes the last ticket (ordered_sum.h) adds the partials in block
// order (groups of 8, then the groups).  The order of every addition is fixed by (n, grid) and by the data.
#include "sunerf_common.h"
#include "ordered_sum.h"
#include "../../include/sunerf_hip_likelihood.h"

namespace {

constexpr int LK_THREADS = 256;
constexpr int LK_WAVES = LK_THREADS / 64;
constexpr int LK_BLOCKS = 128;
constexpr int LK_MAX_ROWS = SUNERF_LIKELIHOOD_MAX_ROWS;
constexpr int LK_MAX_EXTRA = SUNERF_LIKELIHOOD_MAX_FINITE_CHECK;
constexpr int LK_ROW_SUMS = 5;      // count, coarse terms, fine terms, (g fine - target)^2, d / d log gain
constexpr int LK_SCALARS = 3;       // non-finite count, unknown-code count, regularization sum
constexpr int LK_GROUP = 8;         // the last workgroup adds the partials of 8 workgroups per work item, then the 16 groups
constexpr int LK_GROUPS = LK_BLOCKS / LK_GROUP;

// workspace (ordered_sum.h's Ticket): LK_BLOCKS x (5 n_rows + 3) doubles of block partials
__host__ __device__ inline size_t partial_stride(int n_rows) { return (size_t)LK_ROW_SUMS * n_rows + LK_SCALARS; }

struct Args {
  const float* coarse; const float* fine; const float* target; const float* codes;
  int64_t n;                   // slots: N rays x W columns
  const float* row_codes; const double* noise; const float* log_gain; int n_rows;
  int mode;
  const float* reg; int64_t n_reg;
  const float* extra[LK_MAX_EXTRA]; int64_t extra_n[LK_MAX_EXTRA]; int n_extra;
  float lambda_image, lambda_reg;
  float* g_coarse; float* g_fine;
  double* g_log_gain; double* channel_stats;
  float* stats;
  void* workspace;
};

__device__ __forceinline__ double block_sum(double v, double* sh) {
  v = sum64_dpp(v);
  __syncthreads();   // sh may still be read by a previous call
  return wave_order_sum<LK_WAVES>(v, sh);
}

// the term of one prediction p against the target t and its derivative with respect to m = g p
struct Term { double value, d_dm, residual; };
__device__ __forceinline__ Term term_of(int mode, double p, double t, double g, double slope, double base) {
  Term r;
  const double m = g * p, d = m - t;
  r.residual = d;
  if (mode == SUNERF_LIKELIHOOD_OBSERVED) {
    const double s2 = fmax(t, 0.0) * slope + base;
    r.value = d * d / s2;
    r.d_dm = 2.0 * d / s2;
  } else {
    const double s2 = fmax(m, 0.0) * slope + base;
    const double q = d * d / s2;
    r.value = q + log(s2);
    r.d_dm = 2.0 * d / s2;
    if (m > 0.0) r.d_dm += slope * ((1.0 - q) / s2);      // d s2 / d m = G / (U E) where the clamp is open, 0 below it
  }
  return r;
}

__global__ __launch_bounds__(LK_THREADS) void likelihood_kernel(Args a) {
  __shared__ double acc[LK_WAVES][LK_MAX_ROWS][4];
  __shared__ unsigned cnt[LK_WAVES][LK_MAX_ROWS];
  __shared__ double slope[LK_MAX_ROWS], base[LK_MAX_ROWS], gain[LK_MAX_ROWS];
  __shared__ float code_of[LK_MAX_ROWS];
  __shared__ double total[LK_ROW_SUMS * LK_MAX_ROWS + LK_SCALARS];
  __shared__ double group[LK_GROUPS][LK_ROW_SUMS * LK_MAX_ROWS + LK_SCALARS];
  __shared__ double sh[LK_WAVES];
  const int M = a.n_rows;
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  for (int j = threadIdx.x; j < LK_WAVES * LK_MAX_ROWS; j += LK_THREADS) {
    double* p = &acc[0][0][0] + (size_t)j * 4;
    p[0] = 0.0; p[1] = 0.0; p[2] = 0.0; p[3] = 0.0;
    (&cnt[0][0])[j] = 0u;
  }
  if (threadIdx.x < M) {
    const int r = threadIdx.x;
    const double* q = a.noise + (size_t)r * 8;
    const double ue = q[0] * q[1];
    // var(x) = (max(x, 0) U E G + R^2 + extra) / (U E)^2 = max(x, 0) slope + the dark variance; base adds floor^2
    slope[r] = q[2] / ue;
    base[r] = (q[3] * q[3] + q[4]) / (ue * ue) + q[5] * q[5];
    gain[r] = exp((double)a.log_gain[r]);
    code_of[r] = a.row_codes[r];
  }
  __syncthreads();

  const int64_t stride = (int64_t)gridDim.x * LK_THREADS;
  const int64_t tid = (int64_t)blockIdx.x * LK_THREADS + threadIdx.x;
  double bad = 0.0, unknown = 0.0, sum_r = 0.0;
  // the trip count is the same for every lane of a wave (the ballots below need all of them): i0 is the block's first slot
  for (int64_t i0 = (int64_t)blockIdx.x * LK_THREADS; i0 < a.n; i0 += stride) {
    const int64_t i = i0 + threadIdx.x;
    int row = -1;
    double tc = 0.0, tf = 0.0, sq = 0.0, gl = 0.0;
    if (i < a.n) {
      const float c = a.coarse[i], f = a.fine[i], t = a.target[i];
      if (a.codes) {
        const float code = a.codes[i];
        if (code > 0.f) {
          for (int r = 0; r < M; ++r)
            if (code_of[r] == code) { row = r; break; }
          if (row < 0) unknown += 1.0;
        }
      } else {
        row = 0;
      }
      if (!isfinite(t)) row = -1;
      float gc = 0.f, gf = 0.f;
      if (row >= 0) {
        bad += (double)(!isfinite(c) + !isfinite(f));
        const double g = gain[row];
        const Term uc = term_of(a.mode, (double)c, (double)t, g, slope[row], base[row]);
        const Term uf = term_of(a.mode, (double)f, (double)t, g, slope[row], base[row]);
        tc = uc.value; tf = uf.value;
        sq = uf.residual * uf.residual;
        gl = uc.d_dm * (g * (double)c) + uf.d_dm * (g * (double)f);
        gc = (float)(uc.d_dm * g);
        gf = (float)(uf.d_dm * g);
      }
      a.g_coarse[i] = gc;
      a.g_fine[i] = gf;
    }
    unsigned long long todo = __ballot(row >= 0);
    while (todo) {
      const int leader = __ffsll((long long)todo) - 1;
      const int r = __shfl(row, leader);
      const bool mine = row == r;
      const unsigned long long match = __ballot(mine);
      const double s0 = sum64_dpp(mine ? tc : 0.0), s1 = sum64_dpp(mine ? tf : 0.0), s2 = sum64_dpp(mine ? sq : 0.0),
                   s3 = sum64_dpp(mine ? gl : 0.0);
      if (lane == 0) {
        double* p = acc[wave][r];
        p[0] += s0; p[1] += s1; p[2] += s2; p[3] += s3;
        cnt[wave][r] += (unsigned)__popcll(match);
      }
      todo &= ~match;
    }
  }
  for (int64_t i = tid; i < a.n_reg; i += stride) {
    const float r = a.reg[i];
    bad += (double)!isfinite(r);
    sum_r += (double)r;
  }
  for (int k = 0; k < a.n_extra; ++k)
    for (int64_t i = tid; i < a.extra_n[k]; i += stride) bad += (double)!isfinite(a.extra[k][i]);

  const Ticket ws(a.workspace);
  const size_t ps = partial_stride(M);
  const double b0 = block_sum(bad, sh), b1 = block_sum(unknown, sh), b2 = block_sum(sum_r, sh);      // (their barriers order acc too)
  double* mine = ws.partial + (size_t)blockIdx.x * ps;
  for (int j = threadIdx.x; j < M * LK_ROW_SUMS; j += LK_THREADS) {
    const int r = j / LK_ROW_SUMS, k = j - r * LK_ROW_SUMS;
    double s = 0.0;
    if (k == 0) {
      unsigned c = 0;
      for (int w = 0; w < LK_WAVES; ++w) c += cnt[w][r];
      s = (double)c;
    } else {
      for (int w = 0; w < LK_WAVES; ++w) s += acc[w][r][k - 1];
    }
    mine[j] = s;
  }
  if (threadIdx.x == 0) {
    mine[M * LK_ROW_SUMS + 0] = b0; mine[M * LK_ROW_SUMS + 1] = b1; mine[M * LK_ROW_SUMS + 2] = b2;
  }

  if (!last_block(ws.ticket)) return;
  // every sum in block order, in two levels so that the loads of a level are in flight together: work item (k, j) adds value j
  // of the workgroups 8 k .. 8 k + 7, then value j's 16 group sums are added in group order
  const int n_total = M * LK_ROW_SUMS + LK_SCALARS;
  for (int item = threadIdx.x; item < n_total * LK_GROUPS; item += LK_THREADS) {
    const int k = item / n_total, j = item - k * n_total;
    const volatile double* p = ws.seen() + j;
    double v[LK_GROUP];
#pragma unroll
    for (int u = 0; u < LK_GROUP; ++u) {
      const unsigned b = (unsigned)(k * LK_GROUP + u);
      v[u] = b < gridDim.x ? p[(size_t)b * ps] : 0.0;
    }
    double s = 0.0;
#pragma unroll
    for (int u = 0; u < LK_GROUP; ++u) s += v[u];
    group[k][j] = s;
  }
  __syncthreads();
  for (int j = threadIdx.x; j < n_total; j += LK_THREADS) {
    double s = 0.0;
#pragma unroll
    for (int k = 0; k < LK_GROUPS; ++k) s += group[k][j];
    total[j] = s;
  }
  __syncthreads();
  if (threadIdx.x < M) {
    const int r = threadIdx.x;
    const double* t = total + r * LK_ROW_SUMS;
    double* cs = a.channel_stats + (size_t)r * 4;
    cs[0] = t[0]; cs[1] = t[1]; cs[2] = t[2]; cs[3] = t[3];
    a.g_log_gain[r] = t[4];
  }
  if (threadIdx.x == 0) {
    double n_valid = 0.0, sc = 0.0, sf = 0.0, sq = 0.0;
    for (int r = 0; r < M; ++r) {
      const double* t = total + r * LK_ROW_SUMS;
      n_valid += t[0]; sc += t[1]; sf += t[2]; sq += t[3];
    }
    const double* s = total + M * LK_ROW_SUMS;
    const bool any = n_valid > 0.0;
    const double mean_c = any ? sc / n_valid : 0.0, mean_f = any ? sf / n_valid : 0.0;
    const double reg = a.n_reg > 0 ? s[2] / (double)a.n_reg : 0.0;
    a.stats[0] = (float)((double)a.lambda_image * (mean_c + mean_f) + (double)a.lambda_reg * reg);
    a.stats[1] = (float)mean_c;
    a.stats[2] = (float)mean_f;
    a.stats[3] = (float)reg;
    a.stats[4] = any ? (float)(-10.0 * log10(sq / n_valid)) : 0.f;
    a.stats[5] = (float)s[0];
    a.stats[6] = (float)n_valid;
    a.stats[7] = (float)s[1];
    ws.rearm();
  }
}

int blocks_for(int64_t n) {
  const int64_t b = (n + LK_THREADS - 1) / LK_THREADS;
  return (int)(b < 1 ? 1 : (b > LK_BLOCKS ? LK_BLOCKS : b));
}

}  // namespace

extern "C" int sunerf_likelihood_abi_version(void) { return SUNERF_LIKELIHOOD_ABI_VERSION; }

extern "C" size_t sunerf_likelihood_workspace_bytes(int n_rows) {
  if (n_rows < 1 || n_rows > LK_MAX_ROWS) return 0;
  return Ticket::bytes((size_t)LK_BLOCKS * partial_stride(n_rows));
}

extern "C" int sunerf_likelihood_loss(const float* coarse_image, const float* fine_image, const float* target_image,
                                      const float* codes, int64_t n_rays, int n_columns, const float* row_codes,
                                      const double* noise, const float* log_gain, int n_rows, int mode,
                                      const float* regularization, int64_t n_reg, const float* const* finite_check_host,
                                      const int64_t* finite_check_sizes_host, int n_finite_check, float lambda_image,
                                      float lambda_regularization, float* g_coarse, float* g_fine, double* g_log_gain,
                                      double* channel_stats, float* stats, void* workspace, size_t workspace_bytes,
                                      void* stream) {
  if (n_rows > LK_MAX_ROWS || n_finite_check > LK_MAX_EXTRA) return SUNERF_E_UNSUPPORTED;
  if (mode != SUNERF_LIKELIHOOD_OBSERVED && mode != SUNERF_LIKELIHOOD_MODEL) return SUNERF_E_UNSUPPORTED;
  if ((n_rays == 0 || n_columns == 0) && n_rays >= 0 && n_columns >= 0 && n_rows >= 1 && n_reg >= 0 && n_finite_check >= 0)
    return 0;
  if (n_rays < 1 || n_columns < 1 || n_rows < 1 || n_reg < 0 || n_finite_check < 0) return SUNERF_E_BADARG;
  if (n_rays > INT64_MAX / n_columns) return SUNERF_E_BADARG;
  if (!coarse_image || !fine_image || !target_image || !row_codes || !noise || !log_gain) return SUNERF_E_BADARG;
  if (!g_coarse || !g_fine || !g_log_gain || !channel_stats || !stats || !workspace) return SUNERF_E_BADARG;
  if (n_reg > 0 && !regularization) return SUNERF_E_BADARG;
  if ((((uintptr_t)noise) & 7) != 0 || (((uintptr_t)g_log_gain) & 7) != 0 || (((uintptr_t)channel_stats) & 7) != 0 ||
      (((uintptr_t)workspace) & 7) != 0)
    return SUNERF_E_BADARG;
  Args k;
  k.n = n_rays * (int64_t)n_columns;
  int64_t most = k.n > n_reg ? k.n : n_reg;
  k.n_extra = n_finite_check;
  for (int i = 0; i < n_finite_check; ++i) {
    if (!finite_check_host || !finite_check_sizes_host || finite_check_sizes_host[i] < 0) return SUNERF_E_BADARG;
    if (finite_check_sizes_host[i] > 0 && !finite_check_host[i]) return SUNERF_E_BADARG;
    k.extra[i] = finite_check_host[i];
    k.extra_n[i] = finite_check_sizes_host[i];
    if (k.extra_n[i] > most) most = k.extra_n[i];
  }
  if (workspace_bytes < sunerf_likelihood_workspace_bytes(n_rows)) return SUNERF_E_WORKSPACE;
  k.coarse = coarse_image; k.fine = fine_image; k.target = target_image; k.codes = codes;
  k.row_codes = row_codes; k.noise = noise; k.log_gain = log_gain; k.n_rows = n_rows; k.mode = mode;
  k.reg = regularization; k.n_reg = n_reg;
  k.lambda_image = lambda_image; k.lambda_reg = lambda_regularization;
  k.g_coarse = g_coarse; k.g_fine = g_fine; k.g_log_gain = g_log_gain; k.channel_stats = channel_stats; k.stats = stats;
  k.workspace = workspace;
  SUNERF_CLEAR_ERROR();
  hipLaunchKernelGGL(likelihood_kernel, dim3(blocks_for(most)), dim3(LK_THREADS), 0, (hipStream_t)stream, k);
  SUNERF_CHECK_LAUNCH();
  return 0;
}
