// fp32 backward of the sine MLP for SMALL batches (gfx950): parameter gradients from the gradient w.r.t. the raw output,
// with every product and sum in fp32 (v_mfma_f32_32x32x2_f32: exact fp32 products, k-ordered fp32 accumulation) and the
// forward activations RECOMPUTED in fp32 from the query points -- nothing is read from the fp16 activation stash.
//
// Replaces what torch.autograd derives from sunerf/model/model.py:44-57 + 123-132 (reference root), like sunerf_mlp_dgrad +
// sunerf_mlp_wgrad / sunerf_mlp_backward_pipe, for the case those kernels are not built for.  They run the chain
// dZ_{l-1} = (W_l^T dZ_l) cos(Z_{l-1}) on single fp16 operands (dZ, cos, H rounded to 11 bits): every term of a gradient sum
// carries ~2^-12 of relative error.  For a training batch (>= 1e5 samples) that averages out -- every tensor within 1e-3 of the
// fp32 reference, tests/test_gpu_backward.py, test_gpu_e2e.py -- but a sum over a few hundred samples that cancels to a few
// per cent of its terms (bias gradients of tiny batches: tests/tools/fuzz_parity.py cases 23 / 37 / 57, 34 ... 1100 samples) keeps
// 2^-12 x its condition number, 2e-3 ... 3e-2.  tests/tools/bias_conditioning.py reproduces those numbers on the CPU and shows
// that fp32 summation of the bias terms alone changes little (the error sits in the chain's operands, not in the last sum).
// So the small batches (<= 4096 samples by default: sunerf_hip/ops.py:EXACT_BACKWARD_SAMPLES) get the arithmetic of the reference
// instead: 4e-7 ... 5e-5 on every tensor.  Chosen by sample count in sunerf_hip/ops.py:mlp_backward.
//
// Layer-major, plain global-memory GEMMs (one 32 x 32 output tile per wave, operands straight from L2, requested a group of
// products ahead): at these sizes the working set (18 x N x 256 floats) is 75 MB at most; 25 GEMM launches (+ 10 small ones) per backward.
#include "sunerf_common.h"
#include "../../include/sunerf_hip.h"

namespace {

constexpr int EPI_SINCOS = 0;   // out0 = sin(acc + bias), out1 = cos(acc + bias)           (forward layer)
constexpr int EPI_MULC = 1;     // out0 = acc * mul                                           (data gradient: dZ = dH * cos)
constexpr int EPI_PART = 2;     // out0[slice][m][n] = acc over this block's slice of K       (weight gradient partial sums)
constexpr int EPI_STORE = 3;    // out0 = acc                                                 (encoder-feature gradient, tiled GEMM only)

struct GemmArgs {
  const float* A; long a_sm, a_sk;     // A(m, k) = A[m * a_sm + k * a_sk]
  const float* B; long b_sk, b_sn;     // B(k, n) = B[k * b_sk + n * b_sn]
  int M, N, K;
  const float* bias;                   // EPI_SINCOS: [N]
  float* out0; float* out1; long ldo;  // row-major [M][ldo] (EPI_PART: [slice][M][ldo])
  const float* mul; long ldm;          // EPI_MULC: [M][ldm]
};

template <int EPI>
__global__ __launch_bounds__(256) void gemm_f32_kernel(GemmArgs a) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int r = lane & 31, h = lane >> 5;
  const int tiles_n = (a.N + 31) / 32, tiles_m = (a.M + 31) / 32;
  const long tile = (long)blockIdx.x * 4 + wave;
  if (tile >= (long)tiles_m * tiles_n) return;
  const int tm = (int)(tile / tiles_n), tn = (int)(tile % tiles_n);
  const int m = tm * 32 + r, n = tn * 32 + r;
  const bool mok = m < a.M, nok = n < a.N;
  const float* pa = a.A + (long)(mok ? m : 0) * a.a_sm;
  const float* pb = a.B + (long)(nok ? n : 0) * a.b_sn;
  int k0 = 0, k1 = a.K;
  if (EPI == EPI_PART) {
    const int per = ((a.K + (int)gridDim.y - 1) / (int)gridDim.y + 1) & ~1;     // even: a k pair never straddles two slices
    k0 = (int)blockIdx.y * per;
    k1 = k0 + per < a.K ? k0 + per : a.K;
  }
  // lane half h supplies k + h of a 2-deep product (A[i = lane & 31][k = lane >> 5], B[k = lane >> 5][j = lane & 31]).  The
  // operands of GROUP products are requested together, one group ahead of the matrix instructions that consume them: with one
  // load pair and one instruction per trip the loop ran at the latency of an L2 read per 64 matrix cycles (90 us per GEMM at
  // 4096 samples, 25 GEMM launches (+ 10 small ones) per backward).
  constexpr int GROUP = 8;
  f32x16 acc = {0};
  float av[GROUP], bv[GROUP];
  auto fetch = [&](int k, float* fa, float* fb) __attribute__((always_inline)) {
#pragma unroll
    for (int u = 0; u < GROUP; ++u) {
      const int kk = k + 2 * u + h;
      const bool kok = kk < k1;
      const int kc = kok ? kk : k0;
      const float x = pa[(long)kc * a.a_sk], y = pb[(long)kc * a.b_sk];
      fa[u] = (mok && kok) ? x : 0.f;
      fb[u] = (nok && kok) ? y : 0.f;
    }
  };
  if (k0 < k1) fetch(k0, av, bv);
  for (int k = k0; k < k1; k += 2 * GROUP) {
    float an[GROUP], bn[GROUP];
    const bool more = k + 2 * GROUP < k1;
    if (more) fetch(k + 2 * GROUP, an, bn);
#pragma unroll
    for (int u = 0; u < GROUP; ++u) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(av[u], bv[u], acc, 0, 0, 0);
    if (more) {
#pragma unroll
      for (int u = 0; u < GROUP; ++u) { av[u] = an[u]; bv[u] = bn[u]; }
    }
  }
  if (!nok) return;
#pragma unroll
  for (int g = 0; g < 16; ++g) {
    const int row = tm * 32 + acc_row(g, h);
    if (row >= a.M) continue;
    const float v = acc[g];
    if (EPI == EPI_SINCOS) {
      const float z = v + a.bias[n];
      a.out0[(long)row * a.ldo + n] = sinf(z);
      a.out1[(long)row * a.ldo + n] = cosf(z);
    } else if (EPI == EPI_MULC) {
      a.out0[(long)row * a.ldo + n] = v * a.mul[(long)row * a.ldm + n];
    } else {
      a.out0[((long)blockIdx.y * a.M + row) * a.ldo + n] = v;
    }
  }
}

// query points -> the 84 encoder features of PositionalEncoding.forward (model.py:123-132): [x, sin(x 2^k / 2) k-major, cos(...)]
// for samples [first, first + count) of the batch (row i of `enc` is sample first + i)
__global__ void encode_kernel(const float* rays_o, const float* rays_d, const float* times, const float* z_vals,
                              const float* points, long first, long count, int S, float* enc /* [count][84] */) {
  const long local = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (local >= count) return;
  const long i = first + local;
  float v[4];
  if (points) {
    for (int c = 0; c < 4; ++c) v[c] = points[i * 4 + c];
  } else {
    const long ray = i / S;
    const float z = z_vals[i];
    // sampling.py:100: product and sum rounded separately (-ffp-contract=off for the whole library)
    for (int c = 0; c < 3; ++c) v[c] = rays_o[ray * 3 + c] + rays_d[ray * 3 + c] * z;
    v[3] = times[ray];
  }
  float* e = enc + local * SUNERF_ENC_DIM;
  for (int c = 0; c < 4; ++c) e[c] = v[c];
  for (int k = 0; k < 10; ++k) {
    const float f = k == 0 ? 0.5f : (float)(1 << (k - 1));      // 2^k / scale_factor, exact
    for (int c = 0; c < 4; ++c) {
      const float arg = v[c] * f;
      e[4 + 4 * k + c] = sinf(arg);
      e[44 + 4 * k + c] = cosf(arg);
    }
  }
}

// One launch per layer behind the weight-gradient GEMM (they were two: 44 -> 35 launches per backward):
//   blocks [0, ceil(cols / 64)):  db[o] (+)= sum over samples of dZ[s][o], accumulated in fp64 (the sum may cancel to a small fraction
//                                 of its terms); 64 columns per block, 16 row groups, four independent loads in flight per thread
//   the other blocks:             dW[o][j] (+)= sum over slices of partial[slice][o][j]
constexpr int COLSUM_GROUPS = 16;
constexpr int FINISH_THREADS = 64 * COLSUM_GROUPS;
__global__ __launch_bounds__(FINISH_THREADS) void finish_layer_kernel(const float* partial, int slices, long count, float* dw, const float* dz,
                                                                      long n, int ld, int cols, float* db, int accumulate) {
  const int col_blocks = (cols + 63) / 64;
  if ((int)blockIdx.x >= col_blocks) {
    const long i = (long)(blockIdx.x - col_blocks) * FINISH_THREADS + threadIdx.x;
    if (i >= count) return;
    float s = 0.f;
    for (int k = 0; k < slices; ++k) s += partial[(long)k * count + i];
    dw[i] = accumulate ? dw[i] + s : s;
    return;
  }
  __shared__ double part[COLSUM_GROUPS][64];
  const int c = blockIdx.x * 64 + (threadIdx.x & 63), q = threadIdx.x >> 6;
  double s0 = 0.0, s1 = 0.0, s2 = 0.0, s3 = 0.0;
  if (c < cols) {
    long i = q;
    for (; i + 3 * COLSUM_GROUPS < n; i += 4 * COLSUM_GROUPS) {
      const float v0 = dz[i * ld + c], v1 = dz[(i + COLSUM_GROUPS) * ld + c], v2 = dz[(i + 2 * COLSUM_GROUPS) * ld + c],
                  v3 = dz[(i + 3 * COLSUM_GROUPS) * ld + c];
      s0 += (double)v0; s1 += (double)v1; s2 += (double)v2; s3 += (double)v3;
    }
    for (; i < n; i += COLSUM_GROUPS) s0 += (double)dz[i * ld + c];
  }
  part[q][threadIdx.x & 63] = (s0 + s1) + (s2 + s3);
  __syncthreads();
  if (q == 0 && c < cols) {
    double t = 0.0;
#pragma unroll
    for (int k = 0; k < COLSUM_GROUPS; ++k) t += part[k][threadIdx.x];
    const float v = (float)t;
    db[c] = accumulate ? db[c] + v : v;
  }
}

constexpr int K_SLICES = 16;

struct ExactLayout {
  size_t enc, act, dz, partial, total;      // act: [layer][H | cos][N][D]; dz: [2][N][D]
  size_t per;                               // floats per [N][D] tensor
  ExactLayout(int64_t n, int D, int n_linear) {
    auto up = [](size_t v) { return (v + 63) / 64 * 64; };
    per = up((size_t)n * D);
    size_t off = 0;
    enc = off; off += up((size_t)n * SUNERF_ENC_DIM);
    act = off; off += (size_t)(n_linear - 1) * 2 * per;
    dz = off; off += 2 * per;
    partial = off; off += (size_t)K_SLICES * D * (D > SUNERF_ENC_DIM ? D : SUNERF_ENC_DIM);
    total = off * sizeof(float);
  }
};

template <int EPI>
int launch_gemm(const GemmArgs& a, int slices, hipStream_t st) {
  const long tiles = (long)((a.M + 31) / 32) * ((a.N + 31) / 32);
  SUNERF_CLEAR_ERROR();
  hipLaunchKernelGGL(gemm_f32_kernel<EPI>, dim3((unsigned)((tiles + 3) / 4), (unsigned)slices), dim3(256), 0, st, a);
  SUNERF_CHECK_LAUNCH();
  return 0;
}

}  // namespace

extern "C" size_t sunerf_mlp_backward_exact_workspace_bytes(int64_t n_points, int d_filter, int n_linear) {
  if (n_points < 1 || d_filter < 1 || n_linear < 2 || n_linear > SUNERF_MAX_LAYERS) return 0;
  return ExactLayout(n_points, d_filter, n_linear).total;
}

extern "C" int sunerf_mlp_backward_exact(const float* const* weights_host, const float* const* biases_host, int n_linear,
                                         int d_filter, int d_out, const float* rays_o, const float* rays_d, const float* times,
                                         const float* z_vals, const float* points, int64_t n_rays, int n_samples,
                                         const float* g_raw, void* workspace, size_t workspace_bytes,
                                         float* const* grad_weights_host, float* const* grad_biases_host, int accumulate,
                                         void* stream) {
  if (!weights_host || !biases_host || !grad_weights_host || !grad_biases_host || !g_raw || !workspace) return SUNERF_E_BADARG;
  if (n_rays <= 0 || n_samples < 1 || d_filter < 1 || d_out < 1) return SUNERF_E_BADARG;
  if (n_linear < 2 || n_linear > SUNERF_MAX_LAYERS) return SUNERF_E_UNSUPPORTED;
  if (!points && (!rays_o || !rays_d || !times || !z_vals)) return SUNERF_E_BADARG;
  for (int i = 0; i < n_linear; ++i)
    if (!weights_host[i] || !biases_host[i] || !grad_weights_host[i] || !grad_biases_host[i]) return SUNERF_E_BADARG;
  const int64_t N = n_rays * n_samples;
  if (N > (int64_t)1 << 24) return SUNERF_E_UNSUPPORTED;
  const int D = d_filter, n_act = n_linear - 1;
  const ExactLayout L(N, D, n_linear);
  if (workspace_bytes < L.total) return SUNERF_E_WORKSPACE;
  hipStream_t st = (hipStream_t)stream;
  float* ws = (float*)workspace;
  float* enc = ws + L.enc;
  auto H = [&](int l) { return ws + L.act + (size_t)(2 * l) * L.per; };
  auto C = [&](int l) { return ws + L.act + (size_t)(2 * l + 1) * L.per; };
  float* dzb[2] = {ws + L.dz, ws + L.dz + L.per};
  int rc;

  SUNERF_CLEAR_ERROR();
  hipLaunchKernelGGL(encode_kernel, dim3((unsigned)((N + 255) / 256)), dim3(256), 0, st, rays_o, rays_d, times, z_vals, points,
                     0L, (long)N, n_samples, enc);
  SUNERF_CHECK_LAUNCH();
  // forward, fp32: H_l = sin(X W_l^T + b_l), cos kept for the backward
  for (int l = 0; l < n_act; ++l) {
    const int K = l == 0 ? SUNERF_ENC_DIM : D;
    GemmArgs a = {};
    a.A = l == 0 ? enc : H(l - 1); a.a_sm = K; a.a_sk = 1;
    a.B = weights_host[l]; a.b_sk = 1; a.b_sn = K;
    a.M = (int)N; a.N = D; a.K = K; a.bias = biases_host[l];
    a.out0 = H(l); a.out1 = C(l); a.ldo = D;
    if ((rc = launch_gemm<EPI_SINCOS>(a, 1, st))) return rc;
  }
  // backward: dZ of the out layer is g_raw itself
  const float* dz = g_raw;
  int dz_cols = d_out, flip = 0;
  for (int i = n_linear - 1; i >= 0; --i) {
    const int cols = i == 0 ? SUNERF_ENC_DIM : D;           // fan-in of layer i
    const float* X = i == 0 ? enc : H(i - 1);
    // dW_i[o][j] = sum_s dZ_i[s][o] X[s][j]
    GemmArgs w = {};
    w.A = dz; w.a_sm = 1; w.a_sk = dz_cols;
    w.B = X; w.b_sk = cols; w.b_sn = 1;
    w.M = dz_cols; w.N = cols; w.K = (int)N;
    w.out0 = ws + L.partial; w.ldo = cols;
    if ((rc = launch_gemm<EPI_PART>(w, K_SLICES, st))) return rc;
    const long count = (long)dz_cols * cols;
    hipLaunchKernelGGL(finish_layer_kernel, dim3((unsigned)((dz_cols + 63) / 64 + (count + FINISH_THREADS - 1) / FINISH_THREADS)),
                       dim3(FINISH_THREADS), 0, st, ws + L.partial, K_SLICES, count, grad_weights_host[i], dz, (long)N, dz_cols, dz_cols,
                       grad_biases_host[i], accumulate);
    SUNERF_CHECK_LAUNCH();
    if (i == 0) break;
    // dZ_{i-1}[s][j] = (sum_o dZ_i[s][o] W_i[o][j]) cos(Z_{i-1})[s][j]
    GemmArgs d = {};
    d.A = dz; d.a_sm = dz_cols; d.a_sk = 1;
    d.B = weights_host[i]; d.b_sk = D; d.b_sn = 1;
    d.M = (int)N; d.N = D; d.K = dz_cols;
    d.out0 = dzb[flip]; d.ldo = D; d.mul = C(i - 1); d.ldm = D;
    if ((rc = launch_gemm<EPI_MULC>(d, 1, st))) return rc;
    dz = dzb[flip]; dz_cols = D; flip ^= 1;
  }
  return 0;
}

// ---- the same backward at ANY batch size: samples in chunks, LDS-tiled fp32 GEMMs, fp64 cross-chunk sums ---------------------------
// The layer-major kernel above keeps every layer's H and cos for the whole batch (~19 KB per sample at 8 x 256) and gives each wave
// one 32 x 32 tile read straight from L2.  Here the samples run in chunks of chunk_samples(D): per chunk the encoder features, the
// fp32 forward (H and cos of that chunk only), and the backward of the chunk -- data gradients chained layer by layer, every weight
// gradient as split-K partial slabs -- whose partials are added into fp64 accumulators [layer][out][in] / [layer][out] in a fixed
// order (slices, then row blocks, then chunks: no atomics, two runs are bit-identical).  One last launch casts them to fp32 and
// writes or adds them to the gradient buffers.  The workspace depends on (d_filter, n_linear) only.
//
// GEMM: 128 x 128 output block of 256 threads, 2 x 2 waves of 64 x 64 (4 accumulators of v_mfma_f32_32x32x2_f32 each), K in
// steps of 16 staged through LDS; the next step's operands are loaded into registers while the current one is multiplied.  The
// k order of every fp32 chain is the plain 0, 1, 2, ... of the kernel above (zero-filled tails add exact zeros): the forward and
// data-gradient GEMMs are bit-identical to it; weight gradients differ by the slicing of their long K only.
namespace {

constexpr int TB_M = 128, TB_N = 128, TB_K = 16;
constexpr int KC_LD = TB_K + 1;                 // LDS [row][k] of an operand contiguous in k (odd stride: row-parallel reads)
constexpr int RC_LD = TB_M + 32;                // LDS [k][row] of an operand contiguous in its row index (k + 1 lands 32 banks on)
constexpr int TILE_FLOATS = TB_K * RC_LD;       // >= TB_M * KC_LD
constexpr int WGRAD_BLOCKS = 512;               // split-K target of the weight-gradient GEMMs: blocks per launch (2 per CU)
constexpr int COLSUM_ROWS = 256;                // rows per block of the bias column sums

__host__ __device__ constexpr int chunk_samples(int D) { return D > 256 ? 16384 : 32768; }

struct TiledArgs {
  const float* A; long lda;     // A_KC: A(m, k) = A[m * lda + k], else A[k * lda + m]
  const float* B; long ldb;     // B_KC: B(k, n) = B[n * ldb + k], else B[k * ldb + n]
  int M, N, K;
  int k_per;                    // EPI_PART: the K range of one slice (blockIdx.z), a multiple of TB_K
  const float* bias;            // EPI_SINCOS: [N]
  float* out0; float* out1; long ldo;
  const float* mul;             // EPI_MULC: [M][ldo]
};

// one operand's 128 x 16 step: 8 elements per thread, consecutive lanes on the contiguous index
template <bool KC>
__device__ __forceinline__ void tile_load(const float* X, long ld, int rows, int row0, int k0, int kend, float* v) {
  const int t = threadIdx.x;
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    const int row = KC ? (t >> 4) + 16 * j : (t & 127);
    const int k = KC ? (t & 15) : (t >> 7) + 2 * j;
    const int gr = row0 + row, gk = k0 + k;
    v[j] = (gr < rows && gk < kend) ? (KC ? X[(long)gr * ld + gk] : X[(long)gk * ld + gr]) : 0.f;
  }
}

template <bool KC>
__device__ __forceinline__ void tile_store(float* s, const float* v) {
  const int t = threadIdx.x;
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    const int row = KC ? (t >> 4) + 16 * j : (t & 127);
    const int k = KC ? (t & 15) : (t >> 7) + 2 * j;
    s[KC ? row * KC_LD + k : k * RC_LD + row] = v[j];
  }
}

template <bool KC>
__device__ __forceinline__ float tile_at(const float* s, int row, int k) { return s[KC ? row * KC_LD + k : k * RC_LD + row]; }

// out-of-line: 64 inlined copies of the accurate sinf / cosf keep the epilogue loop from unrolling (accumulators in scratch)
__device__ __noinline__ float2 sin_cos(float z) { return make_float2(sinf(z), cosf(z)); }

template <bool A_KC, bool B_KC, int EPI>
__global__ __launch_bounds__(256) void gemm_tiled_kernel(TiledArgs a) {
  __shared__ float sa[TILE_FLOATS], sb[TILE_FLOATS];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int r = lane & 31, h = lane >> 5;
  const int wm = (wave >> 1) * 64, wn = (wave & 1) * 64;
  const int m0 = (int)blockIdx.y * TB_M, n0 = (int)blockIdx.x * TB_N;
  int k0 = 0, k1 = a.K;
  if (EPI == EPI_PART) {
    k0 = (int)blockIdx.z * a.k_per;
    k1 = k0 + a.k_per < a.K ? k0 + a.k_per : a.K;
  }
  f32x16 acc[2][2];
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j) acc[i][j] = f32x16{0};
  float va[8], vb[8];
  if (k0 < k1) {
    tile_load<A_KC>(a.A, a.lda, a.M, m0, k0, k1, va);
    tile_load<B_KC>(a.B, a.ldb, a.N, n0, k0, k1, vb);
    tile_store<A_KC>(sa, va);
    tile_store<B_KC>(sb, vb);
  }
  __syncthreads();
  for (int k = k0; k < k1; k += TB_K) {
    const bool more = k + TB_K < k1;
    if (more) {
      tile_load<A_KC>(a.A, a.lda, a.M, m0, k + TB_K, k1, va);
      tile_load<B_KC>(a.B, a.ldb, a.N, n0, k + TB_K, k1, vb);
    }
#pragma unroll
    for (int kk = 0; kk < TB_K; kk += 2) {
      float fa[2], fb[2];
#pragma unroll
      for (int i = 0; i < 2; ++i) {
        fa[i] = tile_at<A_KC>(sa, wm + 32 * i + r, kk + h);
        fb[i] = tile_at<B_KC>(sb, wn + 32 * i + r, kk + h);
      }
#pragma unroll
      for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j) acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(fa[i], fb[j], acc[i][j], 0, 0, 0);
    }
    __syncthreads();
    if (more) {
      tile_store<A_KC>(sa, va);
      tile_store<B_KC>(sb, vb);
      __syncthreads();
    }
  }
#pragma unroll
  for (int j = 0; j < 2; ++j) {
    const int n = n0 + wn + 32 * j + r;
    if (n >= a.N) continue;
    const float bn = EPI == EPI_SINCOS ? a.bias[n] : 0.f;
#pragma unroll
    for (int i = 0; i < 2; ++i) {
#pragma unroll
      for (int g = 0; g < 16; ++g) {
        const int row = m0 + wm + 32 * i + acc_row(g, h);
        if (row >= a.M) continue;
        const float v = acc[i][j][g];
        const long o = (long)row * a.ldo + n;
        if (EPI == EPI_SINCOS) {
          const float2 sc = sin_cos(v + bn);
          a.out0[o] = sc.x;
          a.out1[o] = sc.y;
        } else if (EPI == EPI_MULC) {
          a.out0[o] = v * a.mul[o];
        } else if (EPI == EPI_STORE) {
          a.out0[o] = v;
        } else {
          a.out0[(long)blockIdx.z * a.M * a.ldo + o] = v;
        }
      }
    }
  }
}

// bias gradient, first half: fp64 sums of COLSUM_ROWS rows of dz per block -> part[row block][col]
__global__ __launch_bounds__(256) void colsum_part_kernel(const float* dz, int rows, int cols, double* part) {
  __shared__ double s[4][64];
  const int c = (int)blockIdx.x * 64 + (threadIdx.x & 63), q = threadIdx.x >> 6;
  const int r0 = (int)blockIdx.y * COLSUM_ROWS;
  const int r1 = r0 + COLSUM_ROWS < rows ? r0 + COLSUM_ROWS : rows;
  double t = 0.0;
  if (c < cols)
    for (int i = r0 + q; i < r1; i += 4) t += (double)dz[(long)i * cols + c];
  s[q][threadIdx.x & 63] = t;
  __syncthreads();
  if (q == 0 && c < cols) part[(long)blockIdx.y * cols + c] = (s[0][threadIdx.x] + s[1][threadIdx.x]) + (s[2][threadIdx.x] + s[3][threadIdx.x]);
}

// one layer of one chunk into the fp64 accumulators: acc_w[i] += sum over slices of wpart[slice][i] (i < count),
// acc_b[c] += sum over row blocks of bpart[block][c]; both in slice / block order
__global__ __launch_bounds__(256) void accumulate_layer_kernel(const float* wpart, int slices, long count, double* acc_w,
                                                               const double* bpart, int blocks, int cols, double* acc_b) {
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < count) {
    double s = 0.0;
    for (int k = 0; k < slices; ++k) s += (double)wpart[(long)k * count + i];
    acc_w[i] += s;
  } else if (i < count + cols) {
    const int c = (int)(i - count);
    double s = 0.0;
    for (int k = 0; k < blocks; ++k) s += bpart[(long)k * cols + c];
    acc_b[c] += s;
  }
}

struct CastArgs {
  float* gw[SUNERF_MAX_LAYERS]; float* gb[SUNERF_MAX_LAYERS];
  long w_off[SUNERF_MAX_LAYERS], b_off[SUNERF_MAX_LAYERS];     // offsets into the fp64 accumulators
  long w_count[SUNERF_MAX_LAYERS]; int b_count[SUNERF_MAX_LAYERS];
  const double* acc; int accumulate;
};

// the fp64 sums -> the fp32 gradient buffers (layer = blockIdx.y)
__global__ __launch_bounds__(256) void cast_grads_kernel(CastArgs a) {
  const int l = blockIdx.y;
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < a.w_count[l]) {
    const float v = (float)a.acc[a.w_off[l] + i];
    a.gw[l][i] = a.accumulate ? a.gw[l][i] + v : v;
  } else if (i < a.w_count[l] + a.b_count[l]) {
    const long c = i - a.w_count[l];
    const float v = (float)a.acc[a.b_off[l] + c];
    a.gb[l][c] = a.accumulate ? a.gb[l][c] + v : v;
  }
}

constexpr int CHUNKED_MAX_OUT = 2;      // d_out of the workspace query (NeRF: 1 or 2)

// weight-gradient split of one layer: slices of a multiple of TB_K rows, about WGRAD_BLOCKS blocks in all
int wgrad_slices(int M, int N, int rows) {
  const int tiles = ((M + TB_M - 1) / TB_M) * ((N + TB_N - 1) / TB_N);
  int s = WGRAD_BLOCKS / tiles;
  const int steps = (rows + TB_K - 1) / TB_K;
  s = s < 1 ? 1 : (s > steps ? steps : s);
  return s;
}
int wgrad_k_per(int rows, int slices) { return ((rows + slices - 1) / slices + TB_K - 1) / TB_K * TB_K; }

struct ChunkedLayout {
  size_t enc, act, dz, wpart, bpart, acc, total;     // byte offsets; act: [layer][H | cos][C][D], dz: [2][C][D]
  size_t per;                                        // floats per [C][D] tensor
  int C;
  ChunkedLayout(int D, int n_linear) {
    auto up = [](size_t v) { return (v + 255) / 256 * 256; };
    C = chunk_samples(D);
    per = (size_t)C * D;
    size_t wp = 0;                                   // largest partial slab of any layer (d_out <= CHUNKED_MAX_OUT)
    for (int i = 0; i < n_linear; ++i) {
      const int M = i == n_linear - 1 ? CHUNKED_MAX_OUT : D, N = i == 0 ? SUNERF_ENC_DIM : D;
      const size_t v = (size_t)wgrad_slices(M, N, C) * M * N;
      wp = v > wp ? v : wp;
    }
    size_t accs = 0;
    for (int i = 0; i < n_linear; ++i) {
      const int M = i == n_linear - 1 ? CHUNKED_MAX_OUT : D, N = i == 0 ? SUNERF_ENC_DIM : D;
      accs += (size_t)M * N + M;
    }
    size_t off = 0;
    enc = off; off += up((size_t)C * SUNERF_ENC_DIM * sizeof(float));
    act = off; off += up((size_t)(n_linear - 1) * 2 * per * sizeof(float));
    dz = off; off += up(2 * per * sizeof(float));
    wpart = off; off += up(wp * sizeof(float));
    bpart = off; off += up((size_t)((C + COLSUM_ROWS - 1) / COLSUM_ROWS) * D * sizeof(double));
    acc = off; off += up(accs * sizeof(double));
    total = off;
  }
};

template <bool A_KC, bool B_KC, int EPI>
int launch_tiled(const TiledArgs& a, int slices, hipStream_t st) {
  SUNERF_CLEAR_ERROR();
  hipLaunchKernelGGL((gemm_tiled_kernel<A_KC, B_KC, EPI>), dim3((unsigned)((a.N + TB_N - 1) / TB_N), (unsigned)((a.M + TB_M - 1) / TB_M),
                     (unsigned)slices), dim3(256), 0, st, a);
  SUNERF_CHECK_LAUNCH();
  return 0;
}

}  // namespace

// ---- input gradients: the last link from dZ_0 to the query points, rays and times ------------------------------------------------
// After the chunk loop's data-gradient chain has reached dZ_0 (the fp32 gradient of the first layer's pre-activation):
//   g_enc[s][j] = sum_o dZ_0[s][o] W_0[o][j]                 (84 encoder columns; the tiled GEMM, fp32-input MFMA)
//   g_x[s][c]   = g_enc[s][c] + sum_k f_k (g_enc[s][4+4k+c] cos(x_c f_k) - g_enc[s][44+4k+c] sin(x_c f_k)),  f_k = 2^k / 2
// (the derivative of PositionalEncoding, model.py:123-132, from the sin / cos already in `enc`; a model without encoding or of a
// padded width has zeros in the padded columns of W_0, so the same formula is exact for it), then in ray mode (x = o + d z, t)
//   g_o[r] = sum_s g_xyz,  g_d[r] = sum_s z_s g_xyz,  g_z[r][s] = d_r . g_xyz,  g_t[r] = sum_s g_t
// in fp64, each ray's samples in sample order; a ray that straddles a chunk seam carries its partial sums into the next chunk
// (two carry slots, alternating by chunk parity: the first ray of a chunk reads one while its last ray writes the other).
namespace {

struct InputGrads {
  float* points;                           // points mode: (N*S, 4)
  float* rays_o; float* rays_d;            // ray mode: (N, 3) each, or NULL
  float* times; float* z;                  // ray mode: (N) and (N, S), or NULL
};

constexpr int RAY_CARRY = 8;               // doubles per carry slot: o 3, d 3, t 1 (+1 pad)

struct InputGradLayout {
  ChunkedLayout base;
  size_t genc, gx, carry, total;           // byte offsets: genc [C][84] floats, gx [C][4] doubles, carry [2][RAY_CARRY] doubles
  InputGradLayout(int D, int n_linear) : base(D, n_linear) {
    auto up = [](size_t v) { return (v + 255) / 256 * 256; };
    size_t off = base.total;
    genc = off; off += up((size_t)base.C * SUNERF_ENC_DIM * sizeof(float));
    gx = off; off += up((size_t)base.C * 4 * sizeof(double));
    carry = off; off += up(2 * RAY_CARRY * sizeof(double));
    total = off;
  }
};

// g_enc + enc -> g_x of samples [first, first + count): written to grad_points (points mode) or, in ray mode, kept in fp64 in `gx`
// for the per-ray sums, with g_z = d . g_xyz written at once
__global__ void encoding_grad_kernel(const float* genc, const float* enc, long first, long count, int S, const float* rays_d,
                                     float* grad_points, double* gx, float* grad_z) {
  const long local = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (local >= count) return;
  const long i = first + local;
  const float* g = genc + local * SUNERF_ENC_DIM;
  const float* e = enc + local * SUNERF_ENC_DIM;
  double v[4];
  for (int c = 0; c < 4; ++c) {
    double s = (double)g[c];
    for (int k = 0; k < 10; ++k) {
      const double f = k == 0 ? 0.5 : (double)(1 << (k - 1));
      s += f * ((double)g[4 + 4 * k + c] * (double)e[44 + 4 * k + c] - (double)g[44 + 4 * k + c] * (double)e[4 + 4 * k + c]);
    }
    v[c] = s;
  }
  if (grad_points) {
    for (int c = 0; c < 4; ++c) grad_points[i * 4 + c] = (float)v[c];
    return;
  }
  for (int c = 0; c < 4; ++c) gx[local * 4 + c] = v[c];
  if (grad_z) {
    const float* d = rays_d + (i / S) * 3;
    grad_z[i] = (float)((double)d[0] * v[0] + (double)d[1] * v[1] + (double)d[2] * v[2]);
  }
}

// one thread per ray touching samples [first, first + count): its sums over the chunk's share of its samples, in sample order,
// started from the carry of the previous chunk if the ray began there, handed to the next chunk if it goes on past this one
__global__ void ray_sums_kernel(const double* gx, long first, long count, int S, const float* z_vals, float* grad_o, float* grad_d,
                                float* grad_t, const double* carry_in, double* carry_out) {
  const long r = first / S + (long)blockIdx.x * blockDim.x + threadIdx.x;
  const long last = first + count;
  if (r > (last - 1) / S) return;
  const long s0 = r * S > first ? r * S : first, s1 = (r + 1) * S < last ? (r + 1) * S : last;
  double o[3] = {0.0, 0.0, 0.0}, d[3] = {0.0, 0.0, 0.0}, t = 0.0;
  if (r * S < first) {
    for (int c = 0; c < 3; ++c) { o[c] = carry_in[c]; d[c] = carry_in[3 + c]; }
    t = carry_in[6];
  }
  for (long i = s0; i < s1; ++i) {
    const double* g = gx + (i - first) * 4;
    const double z = (double)z_vals[i];
    for (int c = 0; c < 3; ++c) { o[c] += g[c]; d[c] += z * g[c]; }
    t += g[3];
  }
  if ((r + 1) * S > last) {
    for (int c = 0; c < 3; ++c) { carry_out[c] = o[c]; carry_out[3 + c] = d[c]; }
    carry_out[6] = t;
    return;
  }
  for (int c = 0; c < 3; ++c) {
    if (grad_o) grad_o[r * 3 + c] = (float)o[c];
    if (grad_d) grad_d[r * 3 + c] = (float)d[c];
  }
  if (grad_t) grad_t[r] = (float)t;
}

// The chunk loop of both entry points below.  Parameter gradients when grad_weights_host != NULL (the fp64 accumulators and the
// final cast), input gradients when `in` != NULL; the launches of the parameter-gradient part are the same either way, so its
// results are bit-identical with and without input gradients.
int chunked_backward(const float* const* weights_host, const float* const* biases_host, int n_linear, int D, int d_out,
                     const float* rays_o, const float* rays_d, const float* times, const float* z_vals, const float* points,
                     int64_t N, int n_samples, const float* g_raw, char* ws, const ChunkedLayout& L,
                     float* const* grad_weights_host, float* const* grad_biases_host, int accumulate, const InputGrads* in,
                     const InputGradLayout* IL, hipStream_t st) {
  const int n_act = n_linear - 1;
  const bool params = grad_weights_host != nullptr;
  float* enc = (float*)(ws + L.enc);
  auto H = [&](int l) { return (float*)(ws + L.act) + (size_t)(2 * l) * L.per; };
  auto Cs = [&](int l) { return (float*)(ws + L.act) + (size_t)(2 * l + 1) * L.per; };
  float* dzb[2] = {(float*)(ws + L.dz), (float*)(ws + L.dz) + L.per};
  float* wpart = (float*)(ws + L.wpart);
  double* bpart = (double*)(ws + L.bpart);
  double* acc = (double*)(ws + L.acc);
  CastArgs ca = {};
  long off = 0, max_count = 0;
  for (int i = 0; i < n_linear; ++i) {
    const int M = i == n_linear - 1 ? d_out : D, K = i == 0 ? SUNERF_ENC_DIM : D;
    ca.gw[i] = params ? grad_weights_host[i] : nullptr; ca.gb[i] = params ? grad_biases_host[i] : nullptr;
    ca.w_off[i] = off; ca.w_count[i] = (long)M * K; off += (long)M * K;
    ca.b_off[i] = off; ca.b_count[i] = M; off += M;
    max_count = (long)M * K + M > max_count ? (long)M * K + M : max_count;
  }
  ca.acc = acc; ca.accumulate = accumulate;
  int rc;
  SUNERF_CLEAR_ERROR();
  if (params && hipMemsetAsync(acc, 0, (size_t)off * sizeof(double), st) != hipSuccess) return (int)hipGetLastError();

  int64_t chunk = 0;
  for (int64_t c0 = 0; c0 < N; c0 += L.C, ++chunk) {
    const int Cn = (int)(N - c0 < L.C ? N - c0 : L.C);
    hipLaunchKernelGGL(encode_kernel, dim3((unsigned)((Cn + 255) / 256)), dim3(256), 0, st, rays_o, rays_d, times, z_vals, points,
                       (long)c0, (long)Cn, n_samples, enc);
    SUNERF_CHECK_LAUNCH();
    // forward, fp32: H_l = sin(X W_l^T + b_l), cos kept for the data gradients
    for (int l = 0; l < n_act; ++l) {
      const int K = l == 0 ? SUNERF_ENC_DIM : D;
      TiledArgs a = {};
      a.A = l == 0 ? enc : H(l - 1); a.lda = K;
      a.B = weights_host[l]; a.ldb = K;
      a.M = Cn; a.N = D; a.K = K; a.bias = biases_host[l];
      a.out0 = H(l); a.out1 = Cs(l); a.ldo = D;
      if ((rc = launch_tiled<true, true, EPI_SINCOS>(a, 1, st))) return rc;
    }
    const float* dz = g_raw + c0 * d_out;
    int dz_cols = d_out, flip = 0;
    for (int i = n_linear - 1; i >= 0; --i) {
      if (params) {
        const int cols = i == 0 ? SUNERF_ENC_DIM : D;         // fan-in of layer i
        const float* X = i == 0 ? enc : H(i - 1);
        // dW_i[o][j] partials = sum over a slice of the chunk's samples of dZ_i[s][o] X[s][j]
        const int slices = wgrad_slices(dz_cols, cols, Cn);
        TiledArgs w = {};
        w.A = dz; w.lda = dz_cols;
        w.B = X; w.ldb = cols;
        w.M = dz_cols; w.N = cols; w.K = Cn; w.k_per = wgrad_k_per(Cn, slices);
        w.out0 = wpart; w.ldo = cols;
        if ((rc = launch_tiled<false, false, EPI_PART>(w, slices, st))) return rc;
        const int blocks = (Cn + COLSUM_ROWS - 1) / COLSUM_ROWS;
        hipLaunchKernelGGL(colsum_part_kernel, dim3((unsigned)((dz_cols + 63) / 64), (unsigned)blocks), dim3(256), 0, st, dz, Cn,
                           dz_cols, bpart);
        SUNERF_CHECK_LAUNCH();
        const long count = (long)dz_cols * cols;
        hipLaunchKernelGGL(accumulate_layer_kernel, dim3((unsigned)((count + dz_cols + 255) / 256)), dim3(256), 0, st, wpart, slices,
                           count, acc + ca.w_off[i], bpart, blocks, dz_cols, acc + ca.b_off[i]);
        SUNERF_CHECK_LAUNCH();
      }
      if (i == 0) break;
      // dZ_{i-1}[s][j] = (sum_o dZ_i[s][o] W_i[o][j]) cos(Z_{i-1})[s][j]
      TiledArgs d = {};
      d.A = dz; d.lda = dz_cols;
      d.B = weights_host[i]; d.ldb = D;
      d.M = Cn; d.N = D; d.K = dz_cols;
      d.out0 = dzb[flip]; d.ldo = D; d.mul = Cs(i - 1);
      if ((rc = launch_tiled<true, false, EPI_MULC>(d, 1, st))) return rc;
      dz = dzb[flip]; dz_cols = D; flip ^= 1;
    }
    if (!in) continue;
    // dz is dZ_0 now: g_enc = dZ_0 W_0 (Cn x 84), then the encoder's derivative and, in ray mode, the per-ray sums
    float* genc = (float*)(ws + IL->genc);
    double* gx = (double*)(ws + IL->gx);
    double* carry = (double*)(ws + IL->carry);
    TiledArgs e = {};
    e.A = dz; e.lda = dz_cols;
    e.B = weights_host[0]; e.ldb = SUNERF_ENC_DIM;
    e.M = Cn; e.N = SUNERF_ENC_DIM; e.K = D;
    e.out0 = genc; e.ldo = SUNERF_ENC_DIM;
    if ((rc = launch_tiled<true, false, EPI_STORE>(e, 1, st))) return rc;
    hipLaunchKernelGGL(encoding_grad_kernel, dim3((unsigned)((Cn + 255) / 256)), dim3(256), 0, st, genc, enc, (long)c0, (long)Cn,
                       n_samples, rays_d, points ? in->points : nullptr, gx, points ? nullptr : in->z);
    SUNERF_CHECK_LAUNCH();
    if (points || (!in->rays_o && !in->rays_d && !in->times)) continue;
    const long rays = (c0 + Cn - 1) / n_samples - c0 / n_samples + 1;
    hipLaunchKernelGGL(ray_sums_kernel, dim3((unsigned)((rays + 255) / 256)), dim3(256), 0, st, gx, (long)c0, (long)Cn, n_samples,
                       z_vals, in->rays_o, in->rays_d, in->times, carry + (chunk & 1) * RAY_CARRY, carry + ((chunk + 1) & 1) * RAY_CARRY);
    SUNERF_CHECK_LAUNCH();
  }
  if (!params) return 0;
  hipLaunchKernelGGL(cast_grads_kernel, dim3((unsigned)((max_count + 255) / 256), (unsigned)n_linear), dim3(256), 0, st, ca);
  SUNERF_CHECK_LAUNCH();
  return 0;
}

// the argument checks both entry points share (parameter gradients optional: both arrays NULL, or both given)
int check_chunked_args(const float* const* weights_host, const float* const* biases_host, int n_linear, int d_filter, int d_out,
                       const float* rays_o, const float* rays_d, const float* times, const float* z_vals, const float* points,
                       int64_t n_rays, int n_samples, const float* g_raw, const void* workspace, float* const* grad_weights_host,
                       float* const* grad_biases_host) {
  if (!weights_host || !biases_host || !g_raw || !workspace) return SUNERF_E_BADARG;
  if (!grad_weights_host != !grad_biases_host) return SUNERF_E_BADARG;
  if (n_rays <= 0 || n_samples < 1 || d_filter < 1 || d_out < 1) return SUNERF_E_BADARG;
  if (n_linear < 2 || n_linear > SUNERF_MAX_LAYERS || d_filter > 512 || d_out > CHUNKED_MAX_OUT) return SUNERF_E_UNSUPPORTED;
  if (!points && (!rays_o || !rays_d || !times || !z_vals)) return SUNERF_E_BADARG;
  for (int i = 0; i < n_linear; ++i) {
    if (!weights_host[i] || !biases_host[i]) return SUNERF_E_BADARG;
    if (grad_weights_host && (!grad_weights_host[i] || !grad_biases_host[i])) return SUNERF_E_BADARG;
  }
  if (n_rays > ((int64_t)1 << 40) / n_samples) return SUNERF_E_UNSUPPORTED;      // 64-bit sample indices throughout
  return 0;
}

}  // namespace

extern "C" size_t sunerf_mlp_backward_exact_chunked_workspace_bytes(int d_filter, int n_linear) {
  if (d_filter < 1 || d_filter > 512 || n_linear < 2 || n_linear > SUNERF_MAX_LAYERS) return 0;
  return ChunkedLayout(d_filter, n_linear).total;
}

extern "C" int sunerf_mlp_backward_exact_chunked(const float* const* weights_host, const float* const* biases_host, int n_linear,
                                                 int d_filter, int d_out, const float* rays_o, const float* rays_d,
                                                 const float* times, const float* z_vals, const float* points, int64_t n_rays,
                                                 int n_samples, const float* g_raw, void* workspace, size_t workspace_bytes,
                                                 float* const* grad_weights_host, float* const* grad_biases_host, int accumulate,
                                                 void* stream) {
  if (!grad_weights_host || !grad_biases_host) return SUNERF_E_BADARG;
  int rc = check_chunked_args(weights_host, biases_host, n_linear, d_filter, d_out, rays_o, rays_d, times, z_vals, points, n_rays,
                              n_samples, g_raw, workspace, grad_weights_host, grad_biases_host);
  if (rc) return rc;
  const ChunkedLayout L(d_filter, n_linear);
  if (workspace_bytes < L.total) return SUNERF_E_WORKSPACE;
  return chunked_backward(weights_host, biases_host, n_linear, d_filter, d_out, rays_o, rays_d, times, z_vals, points,
                          n_rays * n_samples, n_samples, g_raw, (char*)workspace, L, grad_weights_host, grad_biases_host, accumulate,
                          nullptr, nullptr, (hipStream_t)stream);
}

extern "C" size_t sunerf_mlp_input_grad_exact_workspace_bytes(int d_filter, int n_linear) {
  if (d_filter < 1 || d_filter > 512 || n_linear < 2 || n_linear > SUNERF_MAX_LAYERS) return 0;
  return InputGradLayout(d_filter, n_linear).total;
}

extern "C" int sunerf_mlp_input_grad_exact(const float* const* weights_host, const float* const* biases_host, int n_linear,
                                           int d_filter, int d_out, const float* rays_o, const float* rays_d, const float* times,
                                           const float* z_vals, const float* points, int64_t n_rays, int n_samples,
                                           const float* g_raw, void* workspace, size_t workspace_bytes,
                                           float* const* grad_weights_host, float* const* grad_biases_host, int accumulate,
                                           float* grad_points, float* grad_rays_o, float* grad_rays_d, float* grad_times,
                                           float* grad_z, void* stream) {
  int rc = check_chunked_args(weights_host, biases_host, n_linear, d_filter, d_out, rays_o, rays_d, times, z_vals, points, n_rays,
                              n_samples, g_raw, workspace, grad_weights_host, grad_biases_host);
  if (rc) return rc;
  // points mode writes grad_points and no ray gradient; ray mode writes at least one ray gradient and no point gradient
  const bool ray_out = grad_rays_o || grad_rays_d || grad_times || grad_z;
  if (points ? (!grad_points || ray_out) : (grad_points || !ray_out)) return SUNERF_E_BADARG;
  const InputGradLayout IL(d_filter, n_linear);
  if (workspace_bytes < IL.total) return SUNERF_E_WORKSPACE;
  const InputGrads in = {grad_points, grad_rays_o, grad_rays_d, grad_times, grad_z};
  return chunked_backward(weights_host, biases_host, n_linear, d_filter, d_out, rays_o, rays_d, times, z_vals, points,
                          n_rays * n_samples, n_samples, g_raw, (char*)workspace, IL.base, grad_weights_host, grad_biases_host,
                          accumulate, &in, &IL, (hipStream_t)stream);
}
