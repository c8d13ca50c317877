// Training-set side of the path: observation images -> shuffled, rank-sharded ray pool, one launch.
//
// Replaces the host assembly of the reference's data modules (sunerf/data/loader/single_channel.py:44-52,
// multi_thermal_loader.py:54-61, 209-258: per-pixel rays, the time broadcast, three full copies and one
// np.random.permutation over all rays).  The kernel runs in SLOT order: thread i of the launch owns output record
// slot_begin + i, so every store is contiguous and a rank builds nothing but its own shard; the image reads are the random
// side.  For slot j
//   q = pi(j)                        keyed bijection of [0, V): cycle-walking 4-round Feistel network, integer arithmetic only
//   p = valid_index ? valid_index[q] : q     global pixel number (views concatenated, row-major inside a view)
//   (view k, row, col)  from p       binary search over the views' pixel offsets
//   ray                              sunerf_pixel_ray (ray_math.h): the bits sunerf_observer_rays gives for that pixel
//   target[c]                        mean of the f x f source block of the channel's plane: fp64 sum in row-major order, / (f f),
//                                    rounded to fp32 once; f = 1: the pixel itself.  Absent channels: target 0, wavelength 0.
// A block of 256 records is staged in LDS and leaves as 16-byte-per-lane stores (1 KiB per wave instruction): the 24-byte
// ray records and the 4 C-byte rows are never stored field by field.  No atomics: the same key gives the same bytes.
#include "sunerf_common.h"
#include "ray_math.h"
#include "../../include/sunerf_hip.h"

namespace {

constexpr int kBlock = 256;

__host__ __device__ inline uint32_t fmix32(uint32_t h) {      // murmur3 finaliser
  h ^= h >> 16; h *= 0x85ebca6bu; h ^= h >> 13; h *= 0xc2b2ae35u; h ^= h >> 16;
  return h;
}

struct PoolArgs {
  const SunerfViewDesc* views; int n_views;
  int64_t n_pixels;
  const int64_t* valid_index; uint64_t V;
  int C, permute, half_bits;
  uint32_t key[4];
  int64_t slot_begin, n_slots;
  float* rays; float* time; float* target; float* wavelength;
};

// pi(x): the walk follows the cycle of a bijection of [0, 2^(2 half_bits)) that started below V, so it returns below V
__device__ __forceinline__ uint64_t permuted(uint64_t x, const PoolArgs& a) {
  const int b = a.half_bits;
  const uint32_t mask = (1u << b) - 1u;
  do {
    uint32_t L = (uint32_t)(x >> b), R = (uint32_t)x & mask;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const uint32_t t = L ^ (fmix32(R + a.key[r]) & mask);
      L = R; R = t;
    }
    x = ((uint64_t)L << b) | R;
  } while (x >= a.V);
  return x;
}

// rows of `n_valid` floats from LDS to global memory: 16 bytes per lane while whole quads remain, single floats at the ragged end
__device__ __forceinline__ void flush(float* dst, const float* src, int n_valid) {
  for (int v = threadIdx.x * 4; v < n_valid; v += kBlock * 4) {
    if (v + 4 <= n_valid) {
      *reinterpret_cast<f32x4*>(dst + v) = *reinterpret_cast<const f32x4*>(src + v);
    } else {
      for (int e = v; e < n_valid; ++e) dst[e] = src[e];
    }
  }
}

__global__ __launch_bounds__(kBlock) void build_ray_pool_kernel(PoolArgs a) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  const int C = a.C, t = threadIdx.x;
  float* s_rays = lds;                       // [256][6]
  float* s_time = s_rays + kBlock * 6;       // [256]
  float* s_target = s_time + kBlock;         // [256][C]
  float* s_wl = s_target + kBlock * C;       // [256][C]
  const int64_t first = (int64_t)blockIdx.x * kBlock;
  const int64_t i = first + t;
  if (i < a.n_slots) {
    const uint64_t j = (uint64_t)(a.slot_begin + i);
    const uint64_t q = a.permute ? permuted(j, a) : j;
    const int64_t p = a.valid_index ? a.valid_index[q] : (int64_t)q;
    // last view whose first pixel is <= p
    int lo = 0, hi = a.n_views - 1;
    while (lo < hi) {
      const int mid = (lo + hi + 1) >> 1;
      if (a.views[mid].pix_offset <= p) lo = mid; else hi = mid - 1;
    }
    const SunerfViewDesc& v = a.views[lo];
    const int64_t local = p - v.pix_offset;
    float o[3] = {0.f, 0.f, 0.f}, d[3] = {0.f, 0.f, 0.f}, time = 0.f;
    const bool inside = p >= 0 && p < a.n_pixels && local >= 0 && local < (int64_t)v.height * v.width;
    int row = 0, col = 0;
    if (inside) {      // (a pixel number outside the table can only come from a corrupt valid_index: such a record is all zero)
      row = (int)(local / v.width); col = (int)(local - (int64_t)row * v.width);
      const double Tx = v.per_pixel ? v.tx[local] : v.tx[col];
      const double Ty = v.per_pixel ? v.ty[local] : v.ty[row];
      sunerf_pixel_ray(Tx, Ty, v.c2w, o, d);
      time = v.time;
    }
#pragma unroll
    for (int r = 0; r < 3; ++r) { s_rays[t * 6 + r] = o[r]; s_rays[t * 6 + 3 + r] = d[r]; }
    s_time[t] = time;
    if (a.target || a.wavelength) {
      const int f = v.downscale;
      const int64_t src_w = (int64_t)v.width * f, plane_size = (int64_t)v.height * f * src_w;
      for (int c = 0; c < C; ++c) {
        const int pl = inside ? v.plane[c] : -1;
        float value = 0.f, wl = 0.f;
        if (pl >= 0 && pl < v.n_planes) {
          const float* src = v.image + pl * plane_size + (int64_t)row * f * src_w + (int64_t)col * f;
          if (f == 1) {
            value = src[0];
          } else {
            double sum = 0.;
            for (int y = 0; y < f; ++y)
              for (int x = 0; x < f; ++x) sum += (double)src[y * src_w + x];
            value = (float)(sum / (double)(f * f));
          }
          wl = v.wavelength[c];
        }
        s_target[t * C + c] = value;
        s_wl[t * C + c] = wl;
      }
    }
  }
  __syncthreads();
  const int64_t left = a.n_slots - first;
  const int n = left < kBlock ? (int)left : kBlock;      // records of this block
  flush(a.rays + first * 6, s_rays, n * 6);
  flush(a.time + first, s_time, n);
  if (a.target) flush(a.target + first * C, s_target, n * C);
  if (a.wavelength) flush(a.wavelength + first * C, s_wl, n * C);
}

inline bool misaligned(const void* p) { return ((uintptr_t)p & 15u) != 0; }

}  // namespace

extern "C" size_t sunerf_view_desc_bytes(void) { return sizeof(SunerfViewDesc); }

extern "C" int sunerf_build_ray_pool(const SunerfViewDesc* views, int n_views, int64_t n_pixels, const int64_t* valid_index,
                                     int64_t n_valid, int n_channels, int permute, uint64_t seed, uint64_t epoch,
                                     int64_t slot_begin, int64_t n_slots, float* rays, float* time, float* target_image,
                                     float* wavelength, void* stream) {
  if (!views || n_views < 1 || n_pixels < 1 || n_valid < 1 || n_valid > n_pixels || n_valid >= ((int64_t)1 << 40))
    return SUNERF_E_BADARG;
  if (!valid_index && n_valid != n_pixels) return SUNERF_E_BADARG;
  if (n_channels < 1 || n_channels > SUNERF_OBS_MAX_CHANNELS) return SUNERF_E_BADARG;
  if (slot_begin < 0 || n_slots < 0 || slot_begin > n_valid || n_slots > n_valid - slot_begin) return SUNERF_E_BADARG;
  if (n_slots == 0) return 0;
  if ((n_slots + kBlock - 1) / kBlock > 0x7fffffff) return SUNERF_E_BADARG;      // one launch: callers tile beyond 2^39 records
  if (!rays || !time) return SUNERF_E_BADARG;
  if (misaligned(rays) || misaligned(time) || misaligned(target_image) || misaligned(wavelength)) return SUNERF_E_BADARG;
  PoolArgs a;
  a.views = views; a.n_views = n_views; a.n_pixels = n_pixels; a.valid_index = valid_index; a.V = (uint64_t)n_valid;
  a.C = n_channels; a.permute = permute != 0;
  int bits = 0;                                   // bit_length(V - 1)
  for (uint64_t m = a.V - 1; m; m >>= 1) ++bits;
  a.half_bits = (bits + 1) / 2;
  const uint32_t s32 = (uint32_t)seed ^ fmix32((uint32_t)(seed >> 32) + 0x9e3779b9u);
  const uint32_t e32 = (uint32_t)epoch ^ fmix32((uint32_t)(epoch >> 32) + 0x9e3779b9u);
  for (uint32_t r = 0; r < 4; ++r)
    a.key[r] = fmix32((s32 + 0x9e3779b9u * (r + 1)) ^ fmix32(e32 + 0x85ebca6bu * (r + 1)));
  a.slot_begin = slot_begin; a.n_slots = n_slots;
  a.rays = rays; a.time = time; a.target = target_image; a.wavelength = wavelength;
  const size_t lds_bytes = (size_t)kBlock * (7 + 2 * n_channels) * sizeof(float);
  SUNERF_CLEAR_ERROR();
  hipLaunchKernelGGL(build_ray_pool_kernel, dim3((unsigned)((n_slots + kBlock - 1) / kBlock)), dim3(kBlock), lds_bytes,
                     (hipStream_t)stream, a);
  SUNERF_CHECK_LAUNCH();
  return 0;
}
