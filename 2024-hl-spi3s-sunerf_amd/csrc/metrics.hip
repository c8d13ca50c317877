// Image scores of a render against its target: mean SSIM, MSE, MAE and mean error, per image of a batch.
//
// Replaces the host-side scoring of the reference's TestImageCallback (sunerf/train/callback.py:46-56, 84-86) and of its
// evaluation scripts (sunerf/evaluation/stash/metrics_simulation.py:41-54, baseline_simulation.py:30-42):
// skimage.metrics.structural_similarity(target, pred, data_range=R) with its defaults, and the means of d^2, |d| and d,
// d = pred - target.  Per image of H x W fp32 pixels, all arithmetic in fp64:
//
//   window 7 x 7 uniform (NP = 49, cov_norm = 49 / 48), boundary scipy 'reflect' (i < 0 -> -i-1, i >= n -> 2n-i-1)
//   ux, uy, uxx, uyy, uxy = window means of x, y, x^2, y^2, xy         (x = target, y = pred)
//   vx = cov_norm (uxx - ux^2), vy = cov_norm (uyy - uy^2), vxy = cov_norm (uxy - ux uy), C1 = (0.01 R)^2, C2 = (0.03 R)^2
//   S = (2 ux uy + C1)(2 vxy + C2) / ((ux^2 + uy^2 + C1)(vx + vy + C2))
//   ssim = mean of S over [3, H-3) x [3, W-3);  mse, mae, me = means of d^2, |d|, d over all H x W pixels
//
// Layout: launch 1 gives every MT_TW x MT_TH tile of outputs of every image one 256-thread workgroup.  It stages the tile's
// (MT_TW + 6) x (MT_TH + 6) input pairs in LDS (reflected indices; each input byte comes from HBM once, the halo of the
// neighbouring tiles from L2), sums the five products over 7 columns into LDS (fp64), then over 7 rows per output, and
// writes four fp64 sums per tile (crop S, d^2, |d|, d) after ordered_sum.h's halving tree.  Launch 2 gives each image one
// workgroup that adds its tiles' sums in a fixed order and divides.  No atomics: results are bit-identical from run to run
// and do not depend on the batch an image is scored in, nor on its place there.  A NaN pixel lies in some crop window
// and in the pixel means, so it makes all four outputs of its image NaN.
#include "sunerf_common.h"
#include "ordered_sum.h"
#include "../../include/sunerf_hip.h"

namespace {

constexpr int MT_THREADS = 256;
constexpr int MT_TW = 64;                     // output columns of a tile: one per lane of a wave
constexpr int MT_TH = 16;                     // output rows of a tile: 4 per wave
constexpr int MT_R = 3;                       // window radius
constexpr int MT_SW = MT_TW + 2 * MT_R;       // staged columns
constexpr int MT_SH = MT_TH + 2 * MT_R;       // staged rows
constexpr int MT_ROWS_PER_THREAD = MT_TH / (MT_THREADS / MT_TW);

struct MetricsArgs {
  const float* pred;
  const float* target;
  int64_t n_images;
  int height, width;
  int tiles_x, tiles_y;
  int64_t tiles_per_image;
  double c1, c2;
  double* partial;           // [n_images * tiles_per_image][4]
  double* out;               // [n_images][4]
};

__device__ __forceinline__ int reflect(int i, int n) {
  i = i < 0 ? -i - 1 : (i >= n ? 2 * n - i - 1 : i);
  // positions beyond one reflection only occur outside the image, for outputs that are never counted: keep them in bounds
  return i < 0 ? 0 : (i >= n ? n - 1 : i);
}

__global__ __launch_bounds__(MT_THREADS) void image_metrics_tiles_kernel(MetricsArgs a) {
  __shared__ float sx[MT_SH][MT_SW];             // target
  __shared__ float sy[MT_SH][MT_SW];             // pred
  __shared__ double hs[5][MT_SH][MT_TW];         // 7-column sums of x, y, x^2, y^2, xy
  const int t = threadIdx.x;
  const int64_t n_tiles = a.n_images * a.tiles_per_image;
  for (int64_t tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
    const int64_t img = tile / a.tiles_per_image;
    const int in_img = (int)(tile - img * a.tiles_per_image);
    const int y0 = (in_img / a.tiles_x) * MT_TH, x0 = (in_img % a.tiles_x) * MT_TW;
    const int64_t base = img * (int64_t)a.height * a.width;
    const float* px = a.target + base;
    const float* py = a.pred + base;

    for (int i = t; i < MT_SH * MT_SW; i += MT_THREADS) {
      const int r = i / MT_SW, c = i - r * MT_SW;
      const int64_t g = (int64_t)reflect(y0 - MT_R + r, a.height) * a.width + reflect(x0 - MT_R + c, a.width);
      sx[r][c] = px[g];
      sy[r][c] = py[g];
    }
    __syncthreads();

    for (int i = t; i < MT_SH * MT_TW; i += MT_THREADS) {
      const int r = i / MT_TW, c = i - r * MT_TW;
      double s0 = 0., s1 = 0., s2 = 0., s3 = 0., s4 = 0.;
#pragma unroll
      for (int k = 0; k < 2 * MT_R + 1; ++k) {
        const double x = sx[r][c + k], y = sy[r][c + k];
        s0 += x;
        s1 += y;
        s2 += x * x;
        s3 += y * y;
        s4 += x * y;
      }
      hs[0][r][c] = s0;
      hs[1][r][c] = s1;
      hs[2][r][c] = s2;
      hs[3][r][c] = s3;
      hs[4][r][c] = s4;
    }
    __syncthreads();

    const int c = t % MT_TW;
    const int gx = x0 + c;
    double acc[4] = {0., 0., 0., 0.};
    constexpr double cov_norm = 49.0 / 48.0;
    for (int j = 0; j < MT_ROWS_PER_THREAD; ++j) {
      const int r = (t / MT_TW) * MT_ROWS_PER_THREAD + j;
      const int gy = y0 + r;
      if (gy >= a.height || gx >= a.width) continue;
      double m[5];
#pragma unroll
      for (int q = 0; q < 5; ++q) {
        double s = 0.;
#pragma unroll
        for (int k = 0; k < 2 * MT_R + 1; ++k) s += hs[q][r + k][c];
        m[q] = s / 49.0;                       // window mean
      }
      const double ux = m[0], uy = m[1];
      const double vx = cov_norm * (m[2] - ux * ux);
      const double vy = cov_norm * (m[3] - uy * uy);
      const double vxy = cov_norm * (m[4] - ux * uy);
      const double a1 = 2. * ux * uy + a.c1, a2 = 2. * vxy + a.c2;
      const double b1 = ux * ux + uy * uy + a.c1, b2 = vx + vy + a.c2;
      const double S = (a1 * a2) / (b1 * b2);
      if (gy >= MT_R && gy < a.height - MT_R && gx >= MT_R && gx < a.width - MT_R) acc[0] += S;
      const double d = (double)sy[r + MT_R][c + MT_R] - (double)sx[r + MT_R][c + MT_R];
      acc[1] += d * d;
      acc[2] += fabs(d);
      acc[3] += d;
    }
    __syncthreads();                             // hs is reused for the reduction: every thread has read its window sums
    double* red = &hs[0][0][0];                  // [4][MT_THREADS]
    lds_tree<MT_THREADS>(red, acc, add_values());
    if (t < 4) a.partial[tile * 4 + t] = red[t * MT_THREADS];
    __syncthreads();                             // red / sx / sy are overwritten by the next tile
  }
}

__global__ __launch_bounds__(MT_THREADS) void image_metrics_finish_kernel(MetricsArgs a) {
  __shared__ double red[4 * MT_THREADS];
  const int t = threadIdx.x;
  const double n_crop = (double)(a.height - 2 * MT_R) * (double)(a.width - 2 * MT_R);
  const double n_pix = (double)a.height * (double)a.width;
  for (int64_t img = blockIdx.x; img < a.n_images; img += gridDim.x) {
    const double* p = a.partial + img * a.tiles_per_image * 4;
    double acc[4] = {0., 0., 0., 0.};
    for (int64_t j = t; j < a.tiles_per_image; j += MT_THREADS) {
#pragma unroll
      for (int k = 0; k < 4; ++k) acc[k] += p[j * 4 + k];
    }
    lds_tree<MT_THREADS>(red, acc, add_values());
    if (t < 4) a.out[img * 4 + t] = red[t * MT_THREADS] / (t == 0 ? n_crop : n_pix);
    __syncthreads();                             // the results are read before the next image's tree overwrites them
  }
}

int64_t tiles_per_image(int height, int width) {
  return (int64_t)((height + MT_TH - 1) / MT_TH) * ((width + MT_TW - 1) / MT_TW);
}

bool shape_ok(int64_t n_images, int height, int width) {
  return n_images >= 0 && height >= 2 * MT_R + 1 && width >= 2 * MT_R + 1;
}

}  // namespace

extern "C" size_t sunerf_image_metrics_workspace_bytes(int64_t n_images, int height, int width) {
  if (!shape_ok(n_images, height, width)) return 0;
  return (size_t)n_images * (size_t)tiles_per_image(height, width) * 4 * sizeof(double);
}

extern "C" int sunerf_image_metrics(const float* pred, const float* target, int64_t n_images, int height, int width,
                                    double data_range, double* out, void* workspace, size_t workspace_bytes, void* stream) {
  if (n_images == 0) return 0;
  if (!shape_ok(n_images, height, width)) return SUNERF_E_BADARG;
  if (!pred || !target || !out || !workspace) return SUNERF_E_BADARG;
  if (!finite_positive(data_range)) return SUNERF_E_BADARG;
  if ((uintptr_t)out % sizeof(double) || (uintptr_t)workspace % sizeof(double)) return SUNERF_E_BADARG;
  if (workspace_bytes < sunerf_image_metrics_workspace_bytes(n_images, height, width)) return SUNERF_E_WORKSPACE;
  MetricsArgs a;
  a.pred = pred; a.target = target; a.n_images = n_images; a.height = height; a.width = width;
  a.tiles_x = (width + MT_TW - 1) / MT_TW;
  a.tiles_y = (height + MT_TH - 1) / MT_TH;
  a.tiles_per_image = tiles_per_image(height, width);
  a.c1 = (0.01 * data_range) * (0.01 * data_range);
  a.c2 = (0.03 * data_range) * (0.03 * data_range);
  a.partial = (double*)workspace;
  a.out = out;
  const int64_t n_tiles = n_images * a.tiles_per_image;
  const int64_t max_grid = (int64_t)1 << 30;
  hipStream_t st = (hipStream_t)stream;
  SUNERF_CLEAR_ERROR();
  hipLaunchKernelGGL(image_metrics_tiles_kernel, dim3((unsigned)(n_tiles < max_grid ? n_tiles : max_grid)),
                     dim3(MT_THREADS), 0, st, a);
  SUNERF_CHECK_LAUNCH();
  hipLaunchKernelGGL(image_metrics_finish_kernel, dim3((unsigned)(n_images < max_grid ? n_images : max_grid)),
                     dim3(MT_THREADS), 0, st, a);
  SUNERF_CHECK_LAUNCH();
  return 0;
}
