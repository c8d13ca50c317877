// Per-pixel DEM inversion of multi-channel images: for every pixel the unique minimiser over x >= 0 of
//   1/2 sum_w ((G x - y)_w / sigma_w)^2 + lam/2 sum_k (x_k / p_k)^2
// -- the zeroth-order regularised, non-negative inversion of (at most 8) channel values y onto (at most 128) log T nodes, the
// classical counterpart of dem.hip's line-of-sight DEM of a model.  Nothing in the reference inverts; the quantities it is
// compared with are dem.hip's (density_temperature.py:237-265 with the response folded out).
//
// Algorithm: semismooth Newton on the dual.  With the whitened residual v_w = (y - G x)_w / sigma_w, Gs = G / sigma and
// ys = y / sigma, the KKT conditions are x_k = p_k^2 max(0, (Gs^T v)_k) / lam and
//   F(v) = v + Gs x(v) - ys = 0,
// the gradient of the strongly convex, piecewise quadratic D(v) = |v|^2 / 2 + sum_k p_k^2 max(0, (Gs^T v)_k)^2 / (2 lam) - ys.v.
// The unknown is v: M <= 8 numbers per pixel, whatever K.  J = I + Gs_A P_A^2 Gs_A^T / lam over the nodes A with
// (Gs^T v)_k >= 0 (at the start v = 0 that is every node: the first step is the unconstrained ridge solution) has its
// eigenvalues >= 1 whatever lam; LDL^T in registers.  The step d is followed by a line search for the minimum of the convex
// phi(t) = D(v + t d): a trial t is accepted when |phi'(t)| <= 1e-3 |phi'(0)| (or max |F| meets the stop), else the next
// trial is the 1-D Newton point t - phi'/phi'' if it lies inside the bracket of the trials so far, else the bracket's middle
// (2 t while there is no upper end).  Every kink of D a step crosses stiffens it by 1 / lam, so a search that only asks for
// a decrease of D shortens its steps to one kink at a time where the positivity constraint binds; this one needs at most 27
// steps on the test cases.  Stop at max |F| <= tol max |ys|.
//
// Layout: one lane per pixel, everything in fp64 (the build has -ffp-contract=off: every fma below is written, every sum has
// one order).  G (k-major, padded to 8 channels), p^2 and the nodes sit in LDS; all lanes read the same address (a broadcast).
// One pass over the nodes yields F and J at a trial point: K (3 M + M (M + 1) / 2) FMAs, branch-free.  A lane is a small
// state machine (trial point -> accept: new Newton step | reject: next trial) around ONE copy of that pass; the wave runs until
// its slowest lane stops.  A left-out channel (y or sigma not finite, sigma <= 0) has 1 / sigma := 0: its row of Gs and its ys
// vanish, v_w stays 0 and its row of J is the unit row -- M is the same for every lane.  A pixel's result depends on nothing
// but its own inputs: no atomics, reruns, any batch and any tiling give the same bits.
// Discrepancy mode bisects log10 lam per lane on chi2(lam) = |v - F|^2 (non-decreasing in lam); every lam a solve uses is
// rounded to fp32 first, so the lam that is returned is exactly the lam of the returned solve.
// dem rows are staged through LDS, 32 nodes of the wave's 64 pixels at a time, and stored as 128-byte row segments.
#include "sunerf_common.h"
#include "../../include/sunerf_hip.h"

namespace {

constexpr int INV_THREADS = 256;
constexpr int INV_MAX_NODES = 128;
constexpr int INV_MAX_CHANNELS = 8;
constexpr int INV_TRIALS = 30;        // line-search trials of one Newton step; after that the solve has stalled (status bit 0)
constexpr int INV_STAGE_COLS = 33;    // 32 nodes + 1: lane l writes row l, bank (33 l + j) % 32 -- no conflict either way

struct InvArgs {
  const float* y;          // (N,M)
  const float* sigma;      // (N,M)
  const double* G;         // (M,K)
  const double* prior;     // (K,)
  const float* nodes;      // (K,)
  const float* lam_in;     // (N,) or (1,); unused in discrepancy mode
  int lam_per_pixel, discrepancy;
  double chi2_target, lam_min, lam_max, log_lo, log_hi, tol;
  int n_bisect, max_iter;
  int64_t n;
  int K;
  float* dem;              // (N,K) or null
  float* em;
  float* logt_mean;
  float* chi2;
  float* lam_out;
  int* status;
};

template <int M>
__global__ __launch_bounds__(INV_THREADS) void dem_invert_kernel(InvArgs a) {
  __shared__ double Gk[INV_MAX_NODES * INV_MAX_CHANNELS];     // [k][8], channels >= M zero
  __shared__ double p2[INV_MAX_NODES];
  __shared__ double xn[INV_MAX_NODES];
  __shared__ float stage[INV_THREADS * INV_STAGE_COLS];
  constexpr int NJ = M * (M + 1) / 2;
  const int tid = threadIdx.x, K = a.K;
  for (int i = tid; i < K * INV_MAX_CHANNELS; i += INV_THREADS) {
    const int k = i >> 3, w = i & 7;
    Gk[i] = w < M ? a.G[(size_t)w * K + k] : 0.0;
  }
  if (tid < K) {
    const double p = a.prior[tid];
    p2[tid] = p * p;
    xn[tid] = (double)a.nodes[tid];
  }
  __syncthreads();
  const int64_t pix = (int64_t)blockIdx.x * INV_THREADS + tid;
  const bool valid = pix < a.n;

  // ---- this lane's pixel
  double ys[M], is[M], v[M], d[M], F[M];
  int n_used = 0;
  double ymax = 0.0;
#pragma unroll
  for (int w = 0; w < M; ++w) {
    const float yf = valid ? a.y[pix * M + w] : NAN, sf = valid ? a.sigma[pix * M + w] : NAN;
    const bool use = isfinite(yf) && isfinite(sf) && sf > 0.f;
    is[w] = use ? 1.0 / (double)sf : 0.0;
    ys[w] = use ? (double)yf * is[w] : 0.0;
    ymax = fmax(ymax, fabs(ys[w]));
    n_used += use ? 1 : 0;
    v[w] = 0.0; d[w] = 0.0; F[w] = 0.0;
  }
  const double stop = a.tol * ymax;
  int status = 0, iters = 0;
  bool done = !valid;
  if (valid && n_used == 0) { status = 2; done = true; }
  double lam = NAN;
  if (!a.discrepancy && valid) {
    lam = (double)a.lam_in[a.lam_per_pixel ? pix : 0];
    if (!(lam > 0.0) || !isfinite(lam)) {
      if (!done) status = 16;
      done = true;
    }
  }
  const bool solved = !done;                 // this lane owns a solution at the end
  const double target = a.chi2_target < 0.0 ? (double)n_used : a.chi2_target;
  double lo = a.log_lo, hi = a.log_hi, chi2 = 0.0;
  const int n_stages = a.discrepancy ? a.n_bisect + 3 : 1;

  for (int s = 0; s < n_stages; ++s) {       // (uniform)
    double mid = 0.0;
    if (a.discrepancy && !done) {
      mid = 0.5 * (lo + hi);
      lam = s == 0 ? a.lam_min : s == 1 ? a.lam_max : (double)(float)exp10(mid);
    }
    const double inv_lam = 1.0 / lam;
    // ---- one solve, warm-started at v
    bool run = !done, first = true;
    double ts = 0.0, slope = 0.0, t_lo = 0.0, t_hi = INFINITY;
    int it = 0, trials = 0;
    while (run) {
      double vt[M], vs[M], r[M], J[NJ];
#pragma unroll
      for (int w = 0; w < M; ++w) {
        vt[w] = first ? v[w] : fma(ts, d[w], v[w]);
        vs[w] = vt[w] * is[w];
        r[w] = 0.0;
      }
#pragma unroll
      for (int j = 0; j < NJ; ++j) J[j] = 0.0;
      for (int k = 0; k < K; ++k) {
        double g[M];
#pragma unroll
        for (int w = 0; w < M; ++w) g[w] = Gk[k * INV_MAX_CHANNELS + w];
        double t = g[0] * vs[0];
#pragma unroll
        for (int w = 1; w < M; ++w) t = fma(g[w], vs[w], t);
        const double c = t >= 0.0 ? p2[k] * inv_lam : 0.0;
        const double x = c * t;
        int j = 0;
#pragma unroll
        for (int p = 0; p < M; ++p) {
          r[p] = fma(g[p], x, r[p]);
          const double cg = c * g[p];
#pragma unroll
          for (int o = p; o < M; ++o) { J[j] = fma(cg, g[o], J[j]); ++j; }
        }
      }
      // phi(t) = D(v + t d) is convex: phi'(t) = F(v + t d) . d and phi''(t) = d^T J(v + t d) d come with the pass
      double Ft[M], ds[M], nFt = 0.0, gp = 0.0, hp = 0.0;
#pragma unroll
      for (int w = 0; w < M; ++w) {
        Ft[w] = fma(is[w], r[w], vt[w]) - ys[w];
        nFt = fmax(nFt, fabs(Ft[w]));
        gp = fma(Ft[w], d[w], gp);
        hp = fma(d[w], d[w], hp);
        ds[w] = d[w] * is[w];
      }
      {
        int j = 0;
#pragma unroll
        for (int p = 0; p < M; ++p)
#pragma unroll
          for (int o = p; o < M; ++o) { hp = fma(J[j] * (p == o ? 1.0 : 2.0), ds[p] * ds[o], hp); ++j; }
      }
      const bool accept = first || fabs(gp) <= 1e-3 * fabs(slope) || nFt <= stop;
      if (accept) {
        if (!first) ++it;
        first = false;
#pragma unroll
        for (int w = 0; w < M; ++w) { v[w] = vt[w]; F[w] = Ft[w]; }
        if (nFt <= stop) {
          run = false;
        } else if (it >= a.max_iter) {
          run = false; status |= 1;
        } else {
          // A = I + diag(is) J diag(is), only its upper triangle A[p][o], o >= p; then L D L^T in place
          double A[M][M];
          {
            int j = 0;
#pragma unroll
            for (int p = 0; p < M; ++p)
#pragma unroll
              for (int o = p; o < M; ++o) { A[p][o] = fma(J[j], is[p] * is[o], p == o ? 1.0 : 0.0); ++j; }
          }
          // A[p][o] (o > p) becomes L[o][p]; A[p][p] the pivot D_p
          double inv_piv[M];
#pragma unroll
          for (int p = 0; p < M; ++p) {
            double piv = A[p][p];
#pragma unroll
            for (int e = 0; e < p; ++e) piv = fma(-(A[e][p] * A[e][p]), A[e][e], piv);
            A[p][p] = piv;
            inv_piv[p] = 1.0 / piv;
#pragma unroll
            for (int o = p + 1; o < M; ++o) {
              double sum = A[p][o];
#pragma unroll
              for (int e = 0; e < p; ++e) sum = fma(-(A[e][o] * A[e][p]), A[e][e], sum);
              A[p][o] = sum * inv_piv[p];
            }
          }
          double z[M];
#pragma unroll
          for (int p = 0; p < M; ++p) {                 // L z = -F
            double sum = -F[p];
#pragma unroll
            for (int e = 0; e < p; ++e) sum = fma(-A[e][p], z[e], sum);
            z[p] = sum;
          }
#pragma unroll
          for (int p = M - 1; p >= 0; --p) {            // L^T d = D^-1 z
            double sum = z[p] * inv_piv[p];
#pragma unroll
            for (int o = p + 1; o < M; ++o) sum = fma(-A[p][o], d[o], sum);
            d[p] = sum;
          }
          slope = 0.0;
#pragma unroll
          for (int w = 0; w < M; ++w) slope = fma(F[w], d[w], slope);
          ts = 1.0; trials = 0; t_lo = 0.0; t_hi = INFINITY;
        }
      } else {
        // the 1-D Newton point of phi' if it lies inside the bracket the trials have built, else the bracket's middle
        if (gp < 0.0) t_lo = ts; else t_hi = ts;
        double tn = ts - gp / hp;
        if (!(t_lo < tn && tn < t_hi)) tn = t_hi < INFINITY ? 0.5 * (t_lo + t_hi) : 2.0 * ts;
        ts = tn;
        if (++trials >= INV_TRIALS) { run = false; status |= 1; }
      }
    }
    if (!done) {
      iters += it;
      chi2 = 0.0;
#pragma unroll
      for (int w = 0; w < M; ++w) { const double e = v[w] - F[w]; chi2 = fma(e, e, chi2); }     // v - F = ys - Gs x
      if (a.discrepancy) {
        if (s == 0) {
          if (chi2 > target) { status |= 4; done = true; }          // even lam_min cannot fit: the positivity constraint binds
        } else if (s == 1) {
          if (chi2 < target) { status |= 8; done = true; }          // even lam_max fits better than asked
        } else if (s < n_stages - 1) {
          if (chi2 > target) hi = mid; else lo = mid;
        }
      }
    }
  }

  // ---- the DEM of the returned v, its sums, and the staged store
  double vs[M];
#pragma unroll
  for (int w = 0; w < M; ++w) vs[w] = v[w] * is[w];
  const double scale = solved ? 1.0 / lam : 0.0;
  double em = 0.0, wt = 0.0;
  const int lane = tid & 63;
  float* rows = stage + (tid - lane) * INV_STAGE_COLS;         // this wave's 64 rows
  const int64_t pix0 = pix - lane;
  for (int k0 = 0; k0 < K; k0 += 32) {                          // (uniform)
    for (int j = 0; j < 32; ++j) {
      const int k = k0 + j;
      double x = 0.0;
      if (k < K) {
        double t = Gk[k * INV_MAX_CHANNELS] * vs[0];
#pragma unroll
        for (int w = 1; w < M; ++w) t = fma(Gk[k * INV_MAX_CHANNELS + w], vs[w], t);
        x = t > 0.0 ? (p2[k] * scale) * t : 0.0;
        em += x;
        wt = fma(x, xn[k], wt);
      }
      rows[lane * INV_STAGE_COLS + j] = (float)x;
    }
    __syncthreads();
    if (a.dem) {
      const int col = lane & 31, k = k0 + col;
      for (int rr = 0; rr < 32; ++rr) {
        const int row = 2 * rr + (lane >> 5);
        if (k < K && pix0 + row < a.n) a.dem[(pix0 + row) * K + k] = rows[row * INV_STAGE_COLS + col];
      }
    }
    __syncthreads();
  }
  if (valid) {
    if (a.em) a.em[pix] = (float)em;
    if (a.logt_mean) a.logt_mean[pix] = (float)(wt / em);        // em = 0: NaN
    if (a.chi2) a.chi2[pix] = (float)chi2;
    if (a.lam_out) a.lam_out[pix] = solved ? (float)lam : NAN;
    a.status[pix] = status | (iters << 8);
  }
}

template <int M>
void launch(const InvArgs& a, hipStream_t stream) {
  hipLaunchKernelGGL(dem_invert_kernel<M>, dim3((unsigned)((a.n + INV_THREADS - 1) / INV_THREADS)), dim3(INV_THREADS), 0, stream, a);
}

}  // namespace

extern "C" int sunerf_dem_invert(const float* y, const float* sigma, const double* response, const double* prior,
                                 const float* logt_nodes, const float* lam, int lam_per_pixel, int discrepancy,
                                 double chi2_target, double lam_min, double lam_max, int n_bisect, double tol, int max_iter,
                                 int64_t n_pixels, int n_channels, int n_nodes, float* dem, float* em, float* logt_mean,
                                 float* chi2, float* lam_out, int* status, void* stream) {
  if (n_pixels < 0 || n_nodes < 2 || n_channels < 1 || n_bisect < 0 || max_iter < 1) return SUNERF_E_BADARG;
  if (n_nodes > INV_MAX_NODES || n_channels > INV_MAX_CHANNELS) return SUNERF_E_UNSUPPORTED;
  if (n_bisect > 60 || max_iter > 4096) return SUNERF_E_UNSUPPORTED;       // the iteration count has 23 bits of `status`
  if (n_pixels == 0) return 0;
  if (!(tol >= 0.0)) return SUNERF_E_BADARG;
  if (discrepancy && (!((float)lam_min > 0.f) || !(lam_max >= lam_min) || !(lam_max <= 3.0e38))) return SUNERF_E_BADARG;
  if (!y || !sigma || !response || !prior || !logt_nodes || !status || (!discrepancy && !lam)) return SUNERF_E_BADARG;
  InvArgs a = {};
  a.y = y; a.sigma = sigma; a.G = response; a.prior = prior; a.nodes = logt_nodes; a.lam_in = lam;
  a.lam_per_pixel = lam_per_pixel ? 1 : 0; a.discrepancy = discrepancy ? 1 : 0;
  a.chi2_target = chi2_target; a.tol = tol; a.n_bisect = n_bisect; a.max_iter = max_iter;
  if (discrepancy) {       // every lam of a solve is an fp32 number: the returned lam is the lam of the returned solve
    a.lam_min = (double)(float)lam_min; a.lam_max = (double)(float)lam_max;
    a.log_lo = log10(a.lam_min); a.log_hi = log10(a.lam_max);
  }
  a.n = n_pixels; a.K = n_nodes;
  a.dem = dem; a.em = em; a.logt_mean = logt_mean; a.chi2 = chi2; a.lam_out = lam_out; a.status = status;
  SUNERF_CLEAR_ERROR();
  switch (n_channels) {
    case 1: launch<1>(a, (hipStream_t)stream); break;
    case 2: launch<2>(a, (hipStream_t)stream); break;
    case 3: launch<3>(a, (hipStream_t)stream); break;
    case 4: launch<4>(a, (hipStream_t)stream); break;
    case 5: launch<5>(a, (hipStream_t)stream); break;
    case 6: launch<6>(a, (hipStream_t)stream); break;
    case 7: launch<7>(a, (hipStream_t)stream); break;
    default: launch<8>(a, (hipStream_t)stream); break;
  }
  SUNERF_CHECK_LAUNCH();
  return 0;
}
