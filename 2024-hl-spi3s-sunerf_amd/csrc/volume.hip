// 3-D volumes of the field: the query points of a grid, the physical quantities of the model's answer
// and a weighted, masked 3-D score.
//
// Replaces the host-side cube of the reference's sunerf/evaluation/stash/voxel_volume.py:30-56 (np.meshgrid of three
// linspaces, a time column, exp(raw0), the shell mask 1 < r < 1.3) and the point arrays its callers push through
// load_coords (evaluation/loader.py:119-134): 16 B per point over PCIe in, 8 B out, and the caller left to know that emission
// is exp(raw0) and a DT density exp(relu(inf0)).  Here the points are made on the device, the MLP (or a field kernel) answers
// them unchanged, and one element-wise launch turns the answer into the physical fields.
//
// grid_points_kernel      : one thread per voxel; the fp64 expressions of include/sunerf_hip.h, one 16-byte store of the point
//                           and one 4-byte store of the radius per voxel.  The spherical grid multiplies host-made trig values
//                           (n_lat + n_lon of them): per-voxel sin / cos in fp64 would make a 20 B / voxel kernel VALU-bound.
// field_quantities_kernel : a workgroup walks 512-voxel chunks, two voxels per thread: one 16-byte load of the two answers, 8-byte
//                           load of the radii, 8-byte stores of the scalar fields.  The per-channel fields (M, W) are staged in
//                           LDS and leave as 16-byte stores of the chunk's contiguous 512 W floats.  A thread's two voxels are
//                           neighbours, so lane to lane the staging writes are 2 W floats apart: an even stride, two-way bank
//                           conflicts at the least, paid for the 16-byte load; the kernel waits on HBM, not on LDS.  The LDS is
//                           dynamic and sized by what was asked for: none for the scalar modes (the 256^3 emission cube), the
//                           table and one 512 W stage per per-channel output otherwise.  Pointers that are not aligned for the
//                           wide accesses (a tile that starts at an odd voxel) take scalar ones; the arithmetic per voxel is
//                           the same function either way.
// volume_metrics_*        : metrics.hip's structure.  Launch 1: grid-stride over the voxels, eleven fp64 accumulators per thread,
//                           a fixed LDS tree per workgroup, partial[workgroup][11].  Launch 2: one workgroup adds the partials in
//                           a fixed order.  No atomics; the grid is a function of the voxel count only.
#include "sunerf_common.h"
#include "ordered_sum.h"
#include "dt_response.h"
#include "../../include/sunerf_hip.h"

namespace {

// ---- grid points -----------------------------------------------------------------------------------------------------------
struct GridArgs {
  const double* a0; const double* a1; const double* a2;
  int n0, n1, n2;
  SunerfGridFrame f;
  double scale;              // Rs_per_ds
  float time_value;
  int64_t first, count;
  float* points; float* radius;
};

// voxel p -> (i, j, k), C order; 32-bit division where the grid allows it (64-bit division is a long software sequence)
__device__ __forceinline__ void voxel_index(int64_t p, int n1, int n2, bool small, int& i, int& j, int& k) {
  if (small) {
    const unsigned q = (unsigned)p / (unsigned)n2;
    k = (int)((unsigned)p - q * (unsigned)n2);
    i = (int)(q / (unsigned)n1);
    j = (int)(q - (unsigned)i * (unsigned)n1);
  } else {
    const int64_t q = p / n2;
    k = (int)(p - q * n2);
    i = (int)(q / n1);
    j = (int)(q - (int64_t)i * n1);
  }
}

template <int KIND>
__global__ __launch_bounds__(256) void grid_points_kernel(GridArgs a, bool small) {
  const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= a.count) return;
  int i, j, k;
  voxel_index(a.first + t, a.n1, a.n2, small, i, j, k);
  double x, y, z, r;
  if (KIND == SUNERF_GRID_AFFINE) {
    const double u = a.a0[i], v = a.a1[j], w = a.a2[k];
    x = a.f.origin[0] + u * a.f.basis[0][0] + v * a.f.basis[1][0] + w * a.f.basis[2][0];
    y = a.f.origin[1] + u * a.f.basis[0][1] + v * a.f.basis[1][1] + w * a.f.basis[2][1];
    z = a.f.origin[2] + u * a.f.basis[0][2] + v * a.f.basis[1][2] + w * a.f.basis[2][2];
    r = sqrt((x * x + y * y) + z * z);
  } else {
    const double cb = a.a0[i], sb = a.a0[a.n0 + i], cl = a.a1[j], sl = a.a1[a.n1 + j];
    r = a.a2[k];
    x = (-cb * sl) * r;
    y = (cb * cl) * r;
    z = (-sb) * r;
  }
  const f32x4 p = {(float)(x / a.scale), (float)(y / a.scale), (float)(z / a.scale), a.time_value};
  *(f32x4*)(a.points + t * 4) = p;
  a.radius[t] = (float)r;
}

// ---- field quantities ------------------------------------------------------------------------------------------------------
constexpr int FQ_THREADS = 256;
constexpr int FQ_CHUNK = 2 * FQ_THREADS;       // voxels per workgroup step
constexpr int FQ_MAX_GRID = 4096;
constexpr int FQ_TAB = (NTAB + 3) & ~3;        // floats per table half in LDS, so that the stages behind them are 16-byte aligned

// dynamic LDS of field_quantities_kernel [bytes]: the two table halves (emissivity only) and one stage per per-channel output
size_t fq_lds_bytes(bool emissivity, bool absorption_w, int W) {
  return sizeof(float) * ((emissivity ? 2 * FQ_TAB : 0) + (size_t)((emissivity ? 1 : 0) + (absorption_w ? 1 : 0)) * FQ_CHUNK * W);
}

struct FieldArgs {
  int mode, C, W;
  const float* inf; const float* radius;
  int64_t m;
  float r_in, r_out, fill, kappa;
  const float* wavelengths; const float* table_logt; const float* table_resp; const float* log_abs;
  float* out0; float* out1; float* emissivity; float* absorption_w;
  bool vec_io, vec_w;
};

// One voxel.  em / ab: the voxel's W-float rows of the LDS stages (or null).
__device__ __forceinline__ void field_voxel(const FieldArgs& a, const float* tab, const int* ch, const float* kap, float i0,
                                            float i1, float rad, float& o0, float& o1, float* em, float* ab) {
  if (!(rad >= a.r_in && rad <= a.r_out)) {                    // outside the shell, or a NaN radius
    o0 = o1 = a.fill;
    for (int w = 0; w < a.W; ++w) {
      if (em) em[w] = a.fill;
      if (ab) ab[w] = a.fill;
    }
    return;
  }
  if (a.mode == SUNERF_FIELD_EMISSION) {
    o0 = expf(i0);
    o1 = fmaxf(i1, 0.f);
  } else if (a.mode == SUNERF_FIELD_WHITE_LIGHT) {
    o0 = expf(a.kappa * i0);
    o1 = 0.f;
  } else {
    const float rho = expf(fmaxf(i0, 0.f));
    const float logt = fmaxf(i1, 0.f);
    o0 = rho;
    o1 = logt;
    if (em || ab) {
      for (int w = 0; w < a.W; ++w) {
        const int c = ch[w];                                   // an absent channel is 0, whatever the density (inf * 0 is NaN)
        if (em) {
          float R = 0.f, dR;
          if (c >= 0) response(tab + c * 101, tab + FQ_TAB + c * 101, logt, R, dR);
          em[w] = c >= 0 ? rho * rho * R : 0.f;
        }
        if (ab) ab[w] = c >= 0 ? rho * kap[w] : 0.f;
      }
    }
  }
}

// the chunk's n_fl staged floats -> global, 16 bytes per lane where the destination allows it
__device__ __forceinline__ void flush_stage(const float* stage, float* dst, int n_fl, bool vec) {
  const int t = threadIdx.x;
  if (vec) {
    const int n4 = n_fl >> 2;
    for (int q = t; q < n4; q += FQ_THREADS) *(f32x4*)(dst + 4 * q) = *(const f32x4*)(stage + 4 * q);
    for (int q = 4 * n4 + t; q < n_fl; q += FQ_THREADS) dst[q] = stage[q];
  } else {
    for (int q = t; q < n_fl; q += FQ_THREADS) dst[q] = stage[q];
  }
}

__global__ __launch_bounds__(FQ_THREADS) void field_quantities_kernel(FieldArgs a) {
  extern __shared__ __attribute__((aligned(16))) float fq_lds[];          // fq_lds_bytes(): tab | stage_em | stage_ab
  float* tab = fq_lds;
  float* stage_em = fq_lds + (a.emissivity ? 2 * FQ_TAB : 0);
  float* stage_ab = stage_em + (a.emissivity ? FQ_CHUNK * a.W : 0);
  __shared__ int ch[NCH];
  __shared__ float kap[NCH];
  const int t = threadIdx.x;
  const bool per_channel = a.emissivity || a.absorption_w;
  if (per_channel) {
    if (a.emissivity)
      for (int i = t; i < NTAB; i += FQ_THREADS) { tab[i] = a.table_logt[i]; tab[FQ_TAB + i] = a.table_resp[i]; }
    if (t < NCH) {
      const int c = t < a.W ? channel_of(a.wavelengths[t]) : -1;
      ch[t] = c;
      kap[t] = c >= 0 ? fmaxf(a.log_abs[c], 0.f) : 0.f;
    }
    __syncthreads();
  }
  const int64_t n_chunks = (a.m + FQ_CHUNK - 1) / FQ_CHUNK;
  for (int64_t chunk = blockIdx.x; chunk < n_chunks; chunk += gridDim.x) {
    const int64_t base = chunk * FQ_CHUNK;
    const int n_here = (int)((a.m - base) < FQ_CHUNK ? (a.m - base) : FQ_CHUNK);
    const int l0 = 2 * t, l1 = 2 * t + 1;                      // this thread's two voxels of the chunk
    const int64_t v0 = base + l0;
    float* em0 = a.emissivity ? stage_em + l0 * a.W : nullptr;
    float* ab0 = a.absorption_w ? stage_ab + l0 * a.W : nullptr;
    float* em1 = em0 ? em0 + a.W : nullptr;
    float* ab1 = ab0 ? ab0 + a.W : nullptr;
    if (l1 < n_here && a.vec_io) {
      const f32x4 in = *(const f32x4*)(a.inf + v0 * 2);
      const f32x2 rad = *(const f32x2*)(a.radius + v0);
      f32x2 o0, o1;
      float x, y;
      field_voxel(a, tab, ch, kap, in[0], in[1], rad[0], x, y, em0, ab0);
      o0[0] = x; o1[0] = y;
      field_voxel(a, tab, ch, kap, in[2], in[3], rad[1], x, y, em1, ab1);
      o0[1] = x; o1[1] = y;
      if (a.out0) *(f32x2*)(a.out0 + v0) = o0;
      if (a.out1) *(f32x2*)(a.out1 + v0) = o1;
    } else {
#pragma unroll
      for (int s = 0; s < 2; ++s) {
        if (l0 + s >= n_here) break;
        const int64_t v = v0 + s;
        const float i0 = a.inf[v * a.C];
        const float i1 = a.C > 1 ? a.inf[v * a.C + 1] : 0.f;
        float x, y;
        field_voxel(a, tab, ch, kap, i0, i1, a.radius[v], x, y, s ? em1 : em0, s ? ab1 : ab0);
        if (a.out0) a.out0[v] = x;
        if (a.out1) a.out1[v] = y;
      }
    }
    if (per_channel) {
      __syncthreads();
      if (a.emissivity) flush_stage(stage_em, a.emissivity + base * a.W, n_here * a.W, a.vec_w);
      if (a.absorption_w) flush_stage(stage_ab, a.absorption_w + base * a.W, n_here * a.W, a.vec_w);
      __syncthreads();                                         // the stages are rewritten by the next chunk
    }
  }
}

// ---- volume metrics --------------------------------------------------------------------------------------------------------
constexpr int VM_THREADS = 256;
constexpr int VM_MAX_GRID = 1024;
constexpr int VM_N = SUNERF_VOLUME_METRICS_N;
constexpr int VM_MAX = 9;                      // the one output that is a maximum, not a sum

struct VolMetricArgs {
  const float* a; const float* b;
  const double* w0; const double* w1; const double* w2;
  int n0, n1, n2;
  int64_t total;
  double* partial;           // [n_blocks][VM_N]
  double* out;               // [VM_N]
  int n_blocks;
};

// ordered_sum.h's halving tree over the VM_N values, value VM_MAX by fmax; result k in red[k * VM_THREADS].  Each kernel runs it
// once on an array of its own: no barrier of the caller's.
__device__ __forceinline__ void vm_tree(double* red, const double (&v)[VM_N]) {
  lds_tree<VM_THREADS>(red, v, [](int k, double acc, double other) { return k == VM_MAX ? fmax(acc, other) : acc + other; });
}

__global__ __launch_bounds__(VM_THREADS) void volume_metrics_partial_kernel(VolMetricArgs a, bool small) {
  __shared__ double red[VM_N * VM_THREADS];
  double acc[VM_N];
#pragma unroll
  for (int k = 0; k < VM_N; ++k) acc[k] = 0.;
  for (int64_t p = (int64_t)blockIdx.x * VM_THREADS + threadIdx.x; p < a.total; p += (int64_t)gridDim.x * VM_THREADS) {
    const float fa = a.a[p], fb = a.b[p];
    if (!(fabsf(fa) < INFINITY && fabsf(fb) < INFINITY)) continue;       // NaN or inf in either: left out
    int i, j, k;
    voxel_index(p, a.n1, a.n2, small, i, j, k);
    const double w = (a.w0[i] * a.w1[j]) * a.w2[k];
    const double x = fa, y = fb, d = x - y, ad = fabs(d);
    acc[0] += w;
    acc[1] += w * x;
    acc[2] += w * y;
    acc[3] += w * d;
    acc[4] += w * ad;
    acc[5] += w * (d * d);
    acc[6] += w * (x * x);
    acc[7] += w * (y * y);
    acc[8] += w * (x * y);
    acc[9] = fmax(acc[9], ad);
    acc[10] += 1.;
  }
  vm_tree(red, acc);
  if (threadIdx.x < VM_N) a.partial[(size_t)blockIdx.x * VM_N + threadIdx.x] = red[threadIdx.x * VM_THREADS];
}

__global__ __launch_bounds__(VM_THREADS) void volume_metrics_finish_kernel(VolMetricArgs a) {
  __shared__ double red[VM_N * VM_THREADS];
  double acc[VM_N];
#pragma unroll
  for (int k = 0; k < VM_N; ++k) acc[k] = 0.;
  for (int b = threadIdx.x; b < a.n_blocks; b += VM_THREADS) {
#pragma unroll
    for (int k = 0; k < VM_N; ++k) {
      const double v = a.partial[(size_t)b * VM_N + k];
      acc[k] = k == VM_MAX ? fmax(acc[k], v) : acc[k] + v;
    }
  }
  vm_tree(red, acc);
  if (threadIdx.x < VM_N) a.out[threadIdx.x] = red[threadIdx.x * VM_THREADS];
}

int vm_blocks(int64_t total) {
  const int64_t g = (total + VM_THREADS - 1) / VM_THREADS;
  return (int)(g < VM_MAX_GRID ? g : VM_MAX_GRID);
}

bool fits_32bit(int n0, int n1, int n2) { return (int64_t)n0 * n1 * n2 < ((int64_t)1 << 31); }

}  // namespace

extern "C" int sunerf_grid_points(int kind, const double* a0, const double* a1, const double* a2, int n0, int n1, int n2,
                                  SunerfGridFrame frame, double Rs_per_ds, float time_value, int64_t first, int64_t count,
                                  float* points, float* radius, void* stream) {
  if (kind != SUNERF_GRID_AFFINE && kind != SUNERF_GRID_SPHERICAL) return SUNERF_E_BADARG;
  if (n0 < 1 || n1 < 1 || n2 < 1 || first < 0 || count < 0) return SUNERF_E_BADARG;
  if (count > (int64_t)n0 * n1 * n2 - first) return SUNERF_E_BADARG;            // a range outside the grid reads past the axes
  if (!(Rs_per_ds > 0.0)) return SUNERF_E_BADARG;
  if (count == 0) return 0;
  if (!a0 || !a1 || !a2 || !points || !radius) return SUNERF_E_BADARG;
  if ((uintptr_t)points % 16 || (uintptr_t)a0 % 8 || (uintptr_t)a1 % 8 || (uintptr_t)a2 % 8) return SUNERF_E_BADARG;
  GridArgs a;
  a.a0 = a0; a.a1 = a1; a.a2 = a2; a.n0 = n0; a.n1 = n1; a.n2 = n2; a.f = frame; a.scale = Rs_per_ds;
  a.time_value = time_value; a.first = first; a.count = count; a.points = points; a.radius = radius;
  const bool small = fits_32bit(n0, n1, n2);
  if ((count + 255) / 256 > 0x7fffffff) return SUNERF_E_UNSUPPORTED;
  const dim3 grid((unsigned)((count + 255) / 256));
  SUNERF_CLEAR_ERROR();
  if (kind == SUNERF_GRID_AFFINE)
    hipLaunchKernelGGL(grid_points_kernel<SUNERF_GRID_AFFINE>, grid, dim3(256), 0, (hipStream_t)stream, a, small);
  else
    hipLaunchKernelGGL(grid_points_kernel<SUNERF_GRID_SPHERICAL>, grid, dim3(256), 0, (hipStream_t)stream, a, small);
  SUNERF_CHECK_LAUNCH();
  return 0;
}

extern "C" int sunerf_field_quantities(int mode, const float* inferences, int n_channels, const float* radius,
                                       int64_t n_points, float r_in, float r_out, float fill, float kappa,
                                       const float* wavelengths, int n_wavelengths, const float* table_logt,
                                       const float* table_resp, const float* log_abs, float* out0, float* out1,
                                       float* emissivity, float* absorption_w, void* stream) {
  if (mode != SUNERF_FIELD_EMISSION && mode != SUNERF_FIELD_DT && mode != SUNERF_FIELD_WHITE_LIGHT) return SUNERF_E_BADARG;
  if (n_points < 0 || n_channels < 1) return SUNERF_E_BADARG;
  if (mode != SUNERF_FIELD_WHITE_LIGHT && n_channels != 2) return SUNERF_E_BADARG;
  if (mode != SUNERF_FIELD_DT && (emissivity || absorption_w)) return SUNERF_E_BADARG;
  if (mode == SUNERF_FIELD_WHITE_LIGHT && out1) return SUNERF_E_BADARG;
  if (r_in != r_in || r_out != r_out) return SUNERF_E_BADARG;
  const bool per_channel = emissivity || absorption_w;
  if (per_channel) {
    if (n_wavelengths < 1) return SUNERF_E_BADARG;
    if (n_wavelengths > NCH) return SUNERF_E_UNSUPPORTED;
    if (!wavelengths || !log_abs || (emissivity && (!table_logt || !table_resp))) return SUNERF_E_BADARG;
  }
  if (n_points == 0) return 0;
  if (!inferences || !radius) return SUNERF_E_BADARG;
  FieldArgs a;
  a.mode = mode; a.C = n_channels; a.W = per_channel ? n_wavelengths : 0; a.inf = inferences; a.radius = radius; a.m = n_points;
  a.r_in = r_in; a.r_out = r_out; a.fill = fill; a.kappa = kappa; a.wavelengths = wavelengths; a.table_logt = table_logt;
  a.table_resp = table_resp; a.log_abs = log_abs; a.out0 = out0; a.out1 = out1; a.emissivity = emissivity;
  a.absorption_w = absorption_w;
  a.vec_io = n_channels == 2 && (uintptr_t)inferences % 16 == 0 && (uintptr_t)radius % 8 == 0 && (uintptr_t)out0 % 8 == 0 &&
             (uintptr_t)out1 % 8 == 0;
  a.vec_w = (uintptr_t)emissivity % 16 == 0 && (uintptr_t)absorption_w % 16 == 0;
  const int64_t n_chunks = (n_points + FQ_CHUNK - 1) / FQ_CHUNK;
  SUNERF_CLEAR_ERROR();
  hipLaunchKernelGGL(field_quantities_kernel, dim3((unsigned)(n_chunks < FQ_MAX_GRID ? n_chunks : FQ_MAX_GRID)),
                     dim3(FQ_THREADS), fq_lds_bytes(emissivity, absorption_w, a.W), (hipStream_t)stream, a);
  SUNERF_CHECK_LAUNCH();
  return 0;
}

extern "C" size_t sunerf_volume_metrics_workspace_bytes(int64_t n_voxels) {
  if (n_voxels < 1) return 0;
  return (size_t)vm_blocks(n_voxels) * VM_N * sizeof(double);
}

extern "C" int sunerf_volume_metrics(const float* va, const float* vb, int n0, int n1, int n2, const double* w0,
                                     const double* w1, const double* w2, double* out, void* workspace, size_t workspace_bytes,
                                     void* stream) {
  if (n0 < 1 || n1 < 1 || n2 < 1) return SUNERF_E_BADARG;
  if (!va || !vb || !w0 || !w1 || !w2 || !out || !workspace) return SUNERF_E_BADARG;
  if ((uintptr_t)out % sizeof(double) || (uintptr_t)workspace % sizeof(double) || (uintptr_t)w0 % 8 || (uintptr_t)w1 % 8 ||
      (uintptr_t)w2 % 8)
    return SUNERF_E_BADARG;
  VolMetricArgs a;
  a.a = va; a.b = vb; a.w0 = w0; a.w1 = w1; a.w2 = w2; a.n0 = n0; a.n1 = n1; a.n2 = n2;
  a.total = (int64_t)n0 * n1 * n2;
  if (workspace_bytes < sunerf_volume_metrics_workspace_bytes(a.total)) return SUNERF_E_WORKSPACE;
  a.partial = (double*)workspace; a.out = out; a.n_blocks = vm_blocks(a.total);
  hipStream_t st = (hipStream_t)stream;
  SUNERF_CLEAR_ERROR();
  hipLaunchKernelGGL(volume_metrics_partial_kernel, dim3((unsigned)a.n_blocks), dim3(VM_THREADS), 0, st, a,
                     fits_32bit(n0, n1, n2));
  SUNERF_CHECK_LAUNCH();
  hipLaunchKernelGGL(volume_metrics_finish_kernel, dim3(1), dim3(VM_THREADS), 0, st, a);
  SUNERF_CHECK_LAUNCH();
  return 0;
}
