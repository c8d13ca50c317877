// Density / temperature radiative-transfer integral against a RESPONSE SET: the three kernels of dt.hip (forward, backward,
// backward with the gradients of weights / regularizing quantity) for any instrument's channels instead of the seven AIA rows
// of dt_response.h.  C ABI: include/sunerf_hip_response.h; DESIGN.md section 8m.
//
// A response set is M channels, each a positive integer code (what a ray's `wavelengths` row carries), its own strictly
// increasing log T grid of n_m >= 2 nodes and its response on it: offsets[M + 1] into the concatenated logt[] / resp[].  Per
// ray the W <= 8 columns are resolved against codes[M]; a column <= 0 or with a code the set does not hold is absent (image 0,
// no gradient), the documented semantics of dt.hip's channel_of().
//
// The integral itself is dt_sweep.h, the text dt.hip's kernels run, so that on the AIA set the outputs are those of
// sunerf_dt_integral_* bit for bit (tests/test_gpu_response_set.py).  What this file's set policy differs in: the interval of a
// sample is found by binary search on the channel's own grid (dt_response.h indexes the 0.05-dex grid directly), the tables
// are staged in LDS at the set's size, and the backward's slab is strided by the call's W, not by the maximum.
#include "dt_sweep.h"
#include "../../include/sunerf_hip_response.h"

namespace {

constexpr int RS_MAXW = 8;                    // columns of a wavelengths row
constexpr int RS_MAXM = 64;                   // channels of a set
constexpr int RS_MAX_NODES = 4096;            // nodes of a set, all channels together
// LDS floats before the node tables: offsets[65] | codes[64] | g_kappa[64] g_vol | wave maxima[4], rounded up to 16 bytes
constexpr int RS_OFF = 0, RS_CODES = RS_OFF + RS_MAXM + 1, RS_ACC = RS_CODES + RS_MAXM, RS_WMAX = RS_ACC + RS_MAXM + 1;
constexpr int RS_HEAD = (RS_WMAX + DT_THREADS / 64 + 3) & ~3;

struct RsArgs : DtSweepArgs {
  int M, n_nodes;
  const int* offsets;        // (M+1,)
  const float* codes;        // (M,)
  const float* table_logt;   // (n_nodes,)
  const float* table_resp;   // (n_nodes,), response x exposure time; log_abs is (M,) in set order
};

// linear interpolation on a grid of n nodes; returns value and slope (both 0 outside [x_0, x_{n-1}]).  The interval is the
// largest i <= n - 2 with x_i <= x (searchsorted(right=True) - 1, clamped to the last interval): what dt_response.h's
// response() finds on its uniform grid; the expression below is its expression.
__device__ __forceinline__ void response(const float* lt, const float* rs, int n, float x, float& val, float& slope) {
  val = 0.f; slope = 0.f;
  if (!(x >= lt[0] && x <= lt[n - 1])) return;
  int i = 0, hi = n - 2;
  while (i < hi) {
    const int mid = (i + hi + 1) >> 1;
    if (lt[mid] <= x) i = mid; else hi = mid - 1;
  }
  const float x0 = lt[i], x1 = lt[i + 1], y0 = rs[i], y1 = rs[i + 1];
  slope = (y1 - y0) / (x1 - x0);
  val = y0 + (x - x0) * (y1 - y0) / (x1 - x0);
}

size_t rs_bwd_lds_bytes(int S, int W, int n_nodes) {
  return ((size_t)RS_HEAD + 2 * (size_t)n_nodes + (size_t)DT_RAYS * S * W) * sizeof(float);
}

struct ResponseSet {
  using Args = RsArgs;
  static constexpr int MAXW = RS_MAXW;
  // channel set-up of one ray (lane-uniform): row of the set, first node and node count, absorption coefficient.  Lane n looks
  // at codes n and n + 32; the codes of a set are unique, so the maximum over the 32 lanes is the one match or -1.
  struct Channels {
    int ch[RS_MAXW], first[RS_MAXW], count[RS_MAXW];
    float kappa[RS_MAXW];
    __device__ __forceinline__ void init(const RsArgs& a, const float* lds, int64_t ray, int n) {
      const int* offs = (const int*)(lds + RS_OFF);
      const float c0 = n < a.M ? lds[RS_CODES + n] : 0.f, c1 = n + 32 < a.M ? lds[RS_CODES + n + 32] : 0.f;
#pragma unroll
      for (int w = 0; w < RS_MAXW; ++w) {
        int m = -1;
        if (w < a.W) {
          const float wl = a.wavelengths[ray * a.W + w];
          if (wl > 0.f) m = wl == c0 ? n : (wl == c1 ? n + 32 : -1);
#pragma unroll
          for (int d = 16; d >= 1; d >>= 1) m = max(m, __shfl_xor(m, d, 32));
        }
        ch[w] = m;
        first[w] = m >= 0 ? offs[m] : 0;
        count[w] = m >= 0 ? offs[m + 1] - offs[m] : 0;
        kappa[w] = m >= 0 ? fmaxf(a.log_abs[m], 0.f) : 0.f;
      }
    }
  };
  static __device__ __forceinline__ void lookup(const RsArgs& a, const Channels& C, int w, const float* tab, float logt, float& R,
                                                float& dR) {
    response(tab + C.first[w], tab + a.n_nodes + C.first[w], C.count[w], logt, R, dR);
  }
  static __device__ __forceinline__ int stride(const RsArgs& a) { return a.W; }
  // LDS floats: head (offsets as int bits, codes, g_kappa[64] g_vol, wave maxima) | logt[n_nodes] | resp[n_nodes] |
  // [DT_RAYS][S][W] exp(-A); the forward stops after the tables
  static constexpr int VOL = RS_MAXM;
  static __host__ __device__ __forceinline__ int n_abs(const RsArgs& a) { return a.M; }
  static __device__ __forceinline__ void stage(const RsArgs& a, float* lds, int tid) {
    int* offs = (int*)(lds + RS_OFF);
    for (int i = tid; i <= a.M; i += DT_THREADS) offs[i] = a.offsets[i];
    for (int i = tid; i < a.M; i += DT_THREADS) lds[RS_CODES + i] = a.codes[i];
    float* tab = lds + RS_HEAD;
    for (int i = tid; i < a.n_nodes; i += DT_THREADS) { tab[i] = a.table_logt[i]; tab[a.n_nodes + i] = a.table_resp[i]; }
  }
  static __device__ __forceinline__ const float* tab(const float* lds) { return lds + RS_HEAD; }
  static __device__ __forceinline__ float* acc(float* lds) { return lds + RS_ACC; }
  static __device__ __forceinline__ float* wave_max(float* lds) { return lds + RS_WMAX; }
  static __device__ __forceinline__ float* slab(const RsArgs& a, float* lds) { return lds + RS_HEAD + 2 * a.n_nodes; }
  static size_t bwd_lds_bytes(const RsArgs& a) { return rs_bwd_lds_bytes(a.S, a.W, a.n_nodes); }
};

__global__ __launch_bounds__(DT_THREADS) void dt_response_fwd_kernel(RsArgs a) {
  extern __shared__ __attribute__((aligned(16))) float lds[];      // head | logt | resp
  dt_forward<ResponseSet>(a, lds);
}

// sizes and limits, then the empty batch (returns 1: "nothing to launch"), then the pointers every entry point reads
int check_common(const RsArgs& a) {
  if (a.n_rays < 0 || a.S < 3 || a.M < 1 || a.n_nodes < 2 * a.M) return SUNERF_E_BADARG;
  if (a.M > RS_MAXM || a.n_nodes > RS_MAX_NODES || a.W < 1 || a.W > RS_MAXW) return SUNERF_E_UNSUPPORTED;
  if (a.n_rays == 0) return 1;
  if (!a.raw || !a.z_vals || !a.rays_o || !a.rays_d || !a.wavelengths || !a.offsets || !a.codes || !a.table_logt ||
      !a.table_resp || !a.log_abs || !a.vol_c)
    return SUNERF_E_BADARG;
  return 0;
}

template <bool EXTRA>
int run_bwd(const RsArgs& a, void* stream) {
  const int rc = check_common(a);
  if (rc < 0) return rc;
  // an empty batch has null (N,...) tensors; its call only clears the scalar outputs
  if (!a.g_log_abs || !a.g_vol_c || !a.g_absmax_bits || (a.n_rays > 0 && (!a.g_image || !a.g_raw))) return SUNERF_E_BADARG;
  return dt_launch_bwd<ResponseSet, EXTRA>(a, (hipStream_t)stream);
}

RsArgs common_args(const float* raw, const float* z_vals, const float* rays_o, const float* rays_d, const float* wavelengths,
                   int n_wavelengths, int n_channels, int n_nodes_total, const int* offsets, const float* codes,
                   const float* logt, const float* resp, const float* log_abs, const float* vol_c, float base_log_density,
                   float base_log_temperature, float pixel_intensity_factor, float reg_radius, int64_t n_rays, int n_samples) {
  RsArgs a = {};
  a.raw = raw; a.z_vals = z_vals; a.rays_o = rays_o; a.rays_d = rays_d; a.wavelengths = wavelengths; a.W = n_wavelengths;
  a.M = n_channels; a.n_nodes = n_nodes_total; a.offsets = offsets; a.codes = codes; a.table_logt = logt; a.table_resp = resp;
  a.log_abs = log_abs; a.vol_c = vol_c; a.base_rho = base_log_density; a.base_t = base_log_temperature;
  a.pixel_factor = pixel_intensity_factor; a.reg_radius = reg_radius; a.n_rays = n_rays; a.S = n_samples;
  return a;
}

}  // namespace

extern "C" int sunerf_response_abi_version(void) { return SUNERF_RESPONSE_ABI_VERSION; }

extern "C" size_t sunerf_dt_response_bwd_lds_bytes(int n_samples, int n_wavelengths, int n_nodes_total) {
  if (n_samples < 0 || n_wavelengths < 0 || n_nodes_total < 0) return 0;
  return rs_bwd_lds_bytes(n_samples, n_wavelengths, n_nodes_total);
}

extern "C" int sunerf_dt_response_fwd(const float* raw, const float* z_vals, const float* rays_o, const float* rays_d,
                                      const float* wavelengths, int n_wavelengths, int n_channels, int n_nodes_total,
                                      const int* offsets, const float* codes, const float* logt, const float* resp,
                                      const float* log_abs, const float* vol_c, float base_log_density,
                                      float base_log_temperature, float pixel_intensity_factor, float reg_radius,
                                      int64_t n_rays, int n_samples, float* image, float* weights, float* reg_q,
                                      float* height_map, float* absorption_map, float* regularization, void* stream) {
  RsArgs a = common_args(raw, z_vals, rays_o, rays_d, wavelengths, n_wavelengths, n_channels, n_nodes_total, offsets, codes, logt,
                         resp, log_abs, vol_c, base_log_density, base_log_temperature, pixel_intensity_factor, reg_radius, n_rays,
                         n_samples);
  a.image = image; a.weights = weights; a.reg_q = reg_q; a.height_map = height_map; a.absorption_map = absorption_map;
  a.regularization = regularization;
  const int rc = check_common(a);
  if (rc) return rc < 0 ? rc : 0;
  if (!image || !weights || !reg_q) return SUNERF_E_BADARG;
  const size_t lds = ((size_t)RS_HEAD + 2 * (size_t)n_nodes_total) * sizeof(float);      // <= 33 KiB
  SUNERF_CLEAR_ERROR();
  hipLaunchKernelGGL(dt_response_fwd_kernel, dim3((unsigned)((n_rays + DT_RAYS - 1) / DT_RAYS)), dim3(DT_THREADS), lds,
                     (hipStream_t)stream, a);
  SUNERF_CHECK_LAUNCH();
  return 0;
}

extern "C" int sunerf_dt_response_bwd(const float* raw, const float* z_vals, const float* rays_o, const float* rays_d,
                                      const float* wavelengths, int n_wavelengths, int n_channels, int n_nodes_total,
                                      const int* offsets, const float* codes, const float* logt, const float* resp,
                                      const float* log_abs, const float* vol_c, float base_log_density,
                                      float base_log_temperature, float pixel_intensity_factor, float reg_radius,
                                      int64_t n_rays, int n_samples, const float* g_image, const float* g_reg, float* g_raw,
                                      float* g_log_abs, float* g_vol_c, void* g_absmax, void* stream) {
  RsArgs a = common_args(raw, z_vals, rays_o, rays_d, wavelengths, n_wavelengths, n_channels, n_nodes_total, offsets, codes, logt,
                         resp, log_abs, vol_c, base_log_density, base_log_temperature, pixel_intensity_factor, reg_radius, n_rays,
                         n_samples);
  a.g_image = g_image; a.g_reg = g_reg; a.g_raw = g_raw; a.g_log_abs = g_log_abs; a.g_vol_c = g_vol_c;
  a.g_absmax_bits = (unsigned*)g_absmax;
  return run_bwd<false>(a, stream);
}

extern "C" int sunerf_dt_response_bwd_full(const float* raw, const float* z_vals, const float* rays_o, const float* rays_d,
                                           const float* wavelengths, int n_wavelengths, int n_channels, int n_nodes_total,
                                           const int* offsets, const float* codes, const float* logt, const float* resp,
                                           const float* log_abs, const float* vol_c, float base_log_density,
                                           float base_log_temperature, float pixel_intensity_factor, float reg_radius,
                                           int64_t n_rays, int n_samples, const float* g_image, const float* g_reg,
                                           const float* g_weights, const float* g_reg_q, float* g_raw, float* g_log_abs,
                                           float* g_vol_c, void* g_absmax, void* stream) {
  RsArgs a = common_args(raw, z_vals, rays_o, rays_d, wavelengths, n_wavelengths, n_channels, n_nodes_total, offsets, codes, logt,
                         resp, log_abs, vol_c, base_log_density, base_log_temperature, pixel_intensity_factor, reg_radius, n_rays,
                         n_samples);
  a.g_image = g_image; a.g_reg = g_reg; a.g_raw = g_raw; a.g_log_abs = g_log_abs; a.g_vol_c = g_vol_c;
  a.g_absmax_bits = (unsigned*)g_absmax; a.g_weights = g_weights; a.g_reg_q = g_reg_q;
  return run_bwd<true>(a, stream);
}
