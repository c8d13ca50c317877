// Noise gating of an image sequence in overlapping apodised blocks of BT x 16 x 16 samples (include/sunerf_hip_noise_gate.h,
// DESIGN.md section 8z).  A workgroup of 256 lanes owns 16 slabs of 16 x 16 samples: the 16 / BT blocks of one pass that are
// neighbours along x, slab q = block * BT + t.  The blocks of one pass do not overlap, so a pass adds its blocks to `out` with plain
// loads and stores; the 4 x 4 x 4 passes follow each other on the stream and the first one stores.
//
// The transform of a block is separable and every pass over an axis gives one line to one lane, which transforms it in registers
// with a radix-2 network whose twiddles are literals (the loops unroll, the indices are constants):
//   x   256 lines (q, y) of 16 real samples: one 8-point complex transform of the pairs (even, odd) and the split into the bins
//       k_x = 0 .. 8 -- the other seven are the conjugates of a real line and are never formed;
//   y   144 lines (q, k_x) of 16 complex samples;
//   t   144 * 16 / BT lines (block, k_y, k_x) of BT complex samples, in which the lane also forms the factors and transforms back.
// The half spectrum lives in LDS as float2 at q * 146 + y * 9 + k_x.  Read as 8-byte elements, 32 lanes at a time, over 32 banks:
// the y pass takes lanes (k_x, q) with q fastest, 146 q = 18 q mod 32 are the 16 even banks and the next k_x the odd ones; the t
// pass takes lanes (k_y, k_x) at 9 k_y + k_x, consecutive; the x pass takes lanes y x {q, q + 8}, 9 y mod 32 are 16 banks and
// 8 * 146 = 16 mod 32 moves the second slab onto the other 16.  A row of 16 complex bins at a stride of 128 bytes would put all 32
// lanes of the x pass on one bank.  The real samples are staged at q * 274 + y * 17 + x (4-byte elements over 32 banks: 17 y covers
// 16 banks, 8 * 274 = 16 mod 32 the others) so that global memory is read and written in rows of 64 bytes.
//
// Sums that decide something are fp64 and taken in a fixed order: a lane sums its line, 16 lanes sum the lines of a slab, every
// lane sums the slabs of its block.  Counts are integers, summed per workgroup in LDS and added to the plane's state with integer
// atomics.  -ffp-contract=off and no explicit fma: every operation is rounded on its own.
#include "sunerf_common.h"
#include "../../include/sunerf_hip_noise_gate.h"

namespace {

constexpr int NG_THREADS = 256;
constexpr int NG_BINS = 9;                  // k_x = 0 .. 8
constexpr int NG_LINES = 16 * NG_BINS;      // lines (k_y, k_x) of a block, and lines (q, k_x) of a workgroup
constexpr int NG_SLAB = NG_LINES + 2;       // float2 between two slabs of the half spectrum
constexpr int NG_ROW = 17;                  // floats between two rows of the staged samples
constexpr int NG_STAGE_SLAB = 16 * NG_ROW + 2;

// sin^2(pi (k + 1/2) / N) for N = 1, 4, 8, 16: rows 0 .. 3
__device__ const double NG_WINDOW[4][16] = {
    {1.0},
    {0.14644660940672624, 0.8535533905932737, 0.8535533905932737, 0.14644660940672624},
    {0.03806023374435662, 0.3086582838174551, 0.6913417161825449, 0.9619397662556434, 0.9619397662556434, 0.6913417161825449,
     0.3086582838174551, 0.03806023374435662},
    {0.009607359798384776, 0.08426519384872735, 0.22221488349019888, 0.40245483899193585, 0.5975451610080642, 0.777785116509801,
     0.9157348061512728, 0.9903926402016151, 0.9903926402016151, 0.9157348061512728, 0.777785116509801, 0.5975451610080642,
     0.40245483899193585, 0.22221488349019888, 0.08426519384872735, 0.009607359798384776}};
// cos and sin of 2 pi k / 16, k = 1, 2, 3 (k = 0 and 4 multiply by 1 and -+i; 5 .. 7 mirror 3 .. 1)
constexpr float NG_C1 = 0.9238795325112867f, NG_C2 = 0.7071067811865476f, NG_C3 = 0.3826834323650898f;

struct NgArgs {
  const float* frames;
  const uint8_t* bad;
  const double* params;
  const float* spectrum;
  float* out;
  unsigned long long* state;
  int n_frames, n_planes, height, width, mode, fill, first, last;
  int ot0, oy0, ox0;          // where the first block of this pass begins
  int nbt, nby, ngx;          // blocks of this pass along t and y, workgroups along x
  long long n_groups;
  double g2;                  // gamma^2
  float scale;                // 1 / (BT * 16 * 8 * 1.5^axes): the x pass transforms 8 points
};

__device__ __forceinline__ int fold(int i, int n) {
  const int p = 2 * n;
  int m = i % p;
  m = m < 0 ? m + p : m;
  return m < n ? m : p - 1 - m;
}

// v * exp(-+ 2 pi i k / 16), 0 <= k < 8, k a constant wherever this is called
template <bool INV>
__device__ __forceinline__ float2 twiddle(float2 v, int k) {
  if (k == 0) return v;
  if (k == 4) return INV ? make_float2(-v.y, v.x) : make_float2(v.y, -v.x);
  const float c = k == 1 ? NG_C1 : k == 2 ? NG_C2 : k == 3 ? NG_C3 : k == 5 ? -NG_C3 : k == 6 ? -NG_C2 : -NG_C1;
  const float s = k == 1 ? NG_C3 : k == 2 ? NG_C2 : k == 3 ? NG_C1 : k == 5 ? NG_C1 : k == 6 ? NG_C2 : NG_C3;
  return INV ? make_float2(v.x * c - v.y * s, v.y * c + v.x * s) : make_float2(v.x * c + v.y * s, v.y * c - v.x * s);
}

template <int N>
__device__ __forceinline__ constexpr int bitrev(int i) {
  int r = 0;
  for (int b = 1; b < N; b <<= 1) {
    r = (r << 1) | (i & 1);
    i >>= 1;
  }
  return r;
}

template <int N, int LEN, bool INV>
__device__ __forceinline__ void fft_stages(float2 (&v)[N]) {
  if constexpr (LEN >= 2) {
    constexpr int half = LEN / 2, step = 16 / LEN;
#pragma unroll
    for (int base = 0; base < N; base += LEN) {
#pragma unroll
      for (int j = 0; j < half; ++j) {
        const float2 a = v[base + j], b = v[base + j + half];
        v[base + j] = make_float2(a.x + b.x, a.y + b.y);
        v[base + j + half] = twiddle<INV>(make_float2(a.x - b.x, a.y - b.y), j * step);
      }
    }
    fft_stages<N, LEN / 2, INV>(v);
  }
}

// The unnormalised N-point transform in place, decimation in frequency: bin k is left in v[bitrev<N>(k)].
template <int N, bool INV>
__device__ __forceinline__ void fft(float2 (&v)[N]) {
  fft_stages<N, N, INV>(v);
}

template <int BT>
__global__ __launch_bounds__(NG_THREADS) void noise_gate_kernel(NgArgs a) {
  constexpr int NB = 16 / BT;                                            // blocks of a workgroup
  constexpr int T_LINES = NB * NG_LINES;                                 // lines of the t pass
  constexpr int ITER = (T_LINES + NG_THREADS - 1) / NG_THREADS;
  constexpr int WROW = BT == 1 ? 0 : BT == 4 ? 1 : BT == 8 ? 2 : 3;
  __shared__ float2 spec[16 * NG_SLAB];
  __shared__ float stage[16 * NG_STAGE_SLAB];
  __shared__ double line_sum[256], line_pow[256], slab_sum[16], slab_pow[16], blk_pow[16];
  __shared__ int line_cnt[256], slab_cnt[16], blk_cnt[16];
  __shared__ unsigned tally[SUNERF_NOISE_GATE_STATE];
  const float inf = __builtin_inff(), nan = __builtin_nanf("");
  const int lane = threadIdx.x;
  const int cy = lane >> 4, cx = lane & 15;                              // global memory: row cy, sample cx of every slab
  const int ly = lane & 15, lq = ((lane >> 4) & 1) * 8 + (lane >> 5);    // x passes: line ly of slab lq
  const int lt = lq % BT, lb = lq / BT;
  const int T = a.n_frames, C = a.n_planes, H = a.height, W = a.width;

  for (long long g = blockIdx.x; g < a.n_groups; g += gridDim.x) {
    long long rest = g;
    const int gx = (int)(rest % a.ngx);
    rest /= a.ngx;
    const int by = (int)(rest % a.nby);
    rest /= a.nby;
    const int bt = (int)(rest % a.nbt);
    const int c = (int)(rest / a.nbt);
    const int ot = a.ot0 + bt * BT, oy = a.oy0 + by * 16, ox = a.ox0 + gx * (NB * 16);
    if (lane < SUNERF_NOISE_GATE_STATE) tally[lane] = 0;

    // ---- the samples, folded at the edges, row by row into LDS; what is not valid as NaN
    const int py = oy + cy, iy = fold(py, H);
    const bool in_y = py >= 0 && py < H;
    unsigned ok_bits = 0, n_invalid = 0;
    {
      // every load is issued before any value is looked at: 16 (32 with flags) loads in flight per lane, not one after the other
      int64_t off[16];
      float v[16];
      uint8_t flag[16];
#pragma unroll
      for (int q = 0; q < 16; ++q) {
        const int pt = ot + q % BT, px = ox + (q / BT) * 16 + cx;
        off[q] = (((int64_t)fold(pt, T) * C + c) * H + iy) * W + fold(px, W);
        v[q] = a.frames[off[q]];
      }
      if (a.bad) {
#pragma unroll
        for (int q = 0; q < 16; ++q) flag[q] = a.bad[off[q]];
      } else {
#pragma unroll
        for (int q = 0; q < 16; ++q) flag[q] = 0;
      }
#pragma unroll
      for (int q = 0; q < 16; ++q) {
        const int pt = ot + q % BT, px = ox + (q / BT) * 16 + cx;
        const bool ok = __builtin_fabsf(v[q]) < inf && !flag[q];
        stage[q * NG_STAGE_SLAB + cy * NG_ROW + cx] = ok ? v[q] : nan;
        ok_bits |= (ok ? 1u : 0u) << q;
        n_invalid += (a.first && !ok && in_y && pt >= 0 && pt < T && px >= 0 && px < W) ? 1u : 0u;
      }
    }
    __syncthreads();

    // ---- a lane's line of 16 samples: the sums of the block's mean and noise power
    float r[16];
    const double wty = NG_WINDOW[WROW][lt] * NG_WINDOW[3][ly];
    {
      const double pa = a.params[4 * c], pb = a.params[4 * c + 1];
      double s = 0.0, p = 0.0;
      int n = 0;
#pragma unroll
      for (int x = 0; x < 16; ++x) {
        r[x] = stage[lq * NG_STAGE_SLAB + ly * NG_ROW + x];
        if (r[x] == r[x]) {
          const double w = wty * NG_WINDOW[3][x], v = (double)r[x];
          s += v;
          p += (w * w) * (pa + pb * (v > 0.0 ? v : 0.0));
          ++n;
        }
      }
      line_sum[lq * 16 + ly] = s;
      line_pow[lq * 16 + ly] = p;
      line_cnt[lq * 16 + ly] = n;
    }
    __syncthreads();
    if (lane < 16) {
      double s = 0.0, p = 0.0;
      int n = 0;
      for (int y = 0; y < 16; ++y) {
        s += line_sum[lane * 16 + y];
        p += line_pow[lane * 16 + y];
        n += line_cnt[lane * 16 + y];
      }
      slab_sum[lane] = s;
      slab_pow[lane] = p;
      slab_cnt[lane] = n;
    }
    __syncthreads();
    float mean;
    {
      double s = 0.0, p = 0.0;
      int n = 0;
#pragma unroll
      for (int t = 0; t < BT; ++t) {
        s += slab_sum[lb * BT + t];
        p += slab_pow[lb * BT + t];
        n += slab_cnt[lb * BT + t];
      }
      mean = n > 0 ? (float)(s / (double)n) : 0.0f;
      if (ly == 0 && lt == 0) {
        const bool counted = n > 0 && ox + lb * 16 < W;          // a block past the last one of the row has no sample inside
        blk_pow[lb] = p;
        blk_cnt[lb] = counted ? n : 0;
        if (counted) atomicAdd(&tally[1], 1u);
      }
    }

    // ---- x: window, 8-point transform of (even, odd), bins 0 .. 8 of the real line
    {
      float2 z[8];
#pragma unroll
      for (int n = 0; n < 8; ++n) {
        const float v0 = r[2 * n] == r[2 * n] ? r[2 * n] : mean, v1 = r[2 * n + 1] == r[2 * n + 1] ? r[2 * n + 1] : mean;
        z[n] = make_float2((float)(wty * NG_WINDOW[3][2 * n]) * v0, (float)(wty * NG_WINDOW[3][2 * n + 1]) * v1);
      }
      fft<8, false>(z);
#pragma unroll
      for (int k = 0; k <= 8; ++k) {
        const float2 zk = z[bitrev<8>(k & 7)], zm = z[bitrev<8>((8 - k) & 7)];
        const float2 e = make_float2(0.5f * (zk.x + zm.x), 0.5f * (zk.y - zm.y));
        const float2 d = make_float2(0.5f * (zk.x - zm.x), 0.5f * (zk.y + zm.y));
        float2 o = make_float2(d.y, -d.x);
        if (k == 8) o = make_float2(-o.x, -o.y);
        else o = twiddle<false>(o, k);
        spec[lq * NG_SLAB + ly * NG_BINS + k] = make_float2(e.x + o.x, e.y + o.y);
      }
    }
    __syncthreads();

    // ---- y
    if (lane < NG_LINES) {
      float2* line = spec + (lane & 15) * NG_SLAB + (lane >> 4);
      float2 v[16];
#pragma unroll
      for (int y = 0; y < 16; ++y) v[y] = line[y * NG_BINS];
      fft<16, false>(v);
#pragma unroll
      for (int i = 0; i < 16; ++i) line[bitrev<16>(i) * NG_BINS] = v[i];
    }
    __syncthreads();

    // ---- t
    if (BT > 1) {
#pragma unroll
      for (int it = 0; it < ITER; ++it) {
        const int l = it * NG_THREADS + lane;
        if (l < T_LINES) {
          float2* line = spec + (l / NG_LINES) * (BT * NG_SLAB) + l % NG_LINES;
          float2 v[BT];
#pragma unroll
          for (int t = 0; t < BT; ++t) v[t] = line[t * NG_SLAB];
          fft<BT, false>(v);
#pragma unroll
          for (int i = 0; i < BT; ++i) line[bitrev<BT>(i) * NG_SLAB] = v[i];
        }
      }
      __syncthreads();
    }

    // ---- the factors.  k and -k share the one of whichever comes first; at 0 < k_x < 8 that is k itself
    float fac[ITER][BT];
    unsigned kept = 0, total = 0;
#pragma unroll
    for (int it = 0; it < ITER; ++it) {
      const int l = it * NG_THREADS + lane;
      if (l < T_LINES) {
        const int blk = l / NG_LINES, ky = (l % NG_LINES) / NG_BINS, kx = l % NG_BINS;
        const bool paired = kx == 0 || kx == 8, counted = blk_cnt[blk] > 0;
        const double thr0 = a.g2 * blk_pow[blk];
        const unsigned weight = paired ? 1u : 2u;
        float2 f[BT];
        float shape[BT];          // all loads of the line before the first use
        int from[BT];             // (k_t, k_y) of the coefficient that decides, as k_t * 16 + k_y
#pragma unroll
        for (int kt = 0; kt < BT; ++kt) {
          const int own = kt * 16 + ky, other = ((BT - kt) % BT) * 16 + ((16 - ky) & 15);
          from[kt] = paired && other < own ? other : own;
          f[kt] = spec[(blk * BT + (from[kt] >> 4)) * NG_SLAB + (from[kt] & 15) * NG_BINS + kx];
        }
        if (a.spectrum) {
#pragma unroll
          for (int kt = 0; kt < BT; ++kt) shape[kt] = a.spectrum[((int64_t)c * BT * 16 + from[kt]) * 16 + kx];
        } else {
#pragma unroll
          for (int kt = 0; kt < BT; ++kt) shape[kt] = 1.0f;
        }
#pragma unroll
        for (int kt = 0; kt < BT; ++kt) {
          const double mag = (double)f[kt].x * (double)f[kt].x + (double)f[kt].y * (double)f[kt].y;
          const double thr = thr0 * (double)shape[kt];
          float factor = 1.0f;
          if (kt | ky | kx) {
            if (a.mode == SUNERF_NOISE_GATE_MODE_GATE) {
              factor = mag >= thr ? 1.0f : 0.0f;
            } else {
              const double w = mag > 0.0 ? 1.0 - thr / mag : 0.0;
              factor = w > 0.0 ? (float)w : 0.0f;
            }
            total += counted ? weight : 0u;
            kept += counted && factor > 0.0f ? weight : 0u;
          }
          fac[it][kt] = factor;
        }
      }
    }
    __syncthreads();

    // ---- t back
#pragma unroll
    for (int it = 0; it < ITER; ++it) {
      const int l = it * NG_THREADS + lane;
      if (l < T_LINES) {
        float2* line = spec + (l / NG_LINES) * (BT * NG_SLAB) + l % NG_LINES;
        float2 v[BT];
#pragma unroll
        for (int t = 0; t < BT; ++t) {
          const float2 f = line[t * NG_SLAB];
          v[t] = make_float2(f.x * fac[it][t], f.y * fac[it][t]);
        }
        if (BT > 1) fft<BT, true>(v);
#pragma unroll
        for (int i = 0; i < BT; ++i) line[bitrev<BT>(i) * NG_SLAB] = v[i];
      }
    }
    __syncthreads();

    // ---- y back
    if (lane < NG_LINES) {
      float2* line = spec + (lane & 15) * NG_SLAB + (lane >> 4);
      float2 v[16];
#pragma unroll
      for (int y = 0; y < 16; ++y) v[y] = line[y * NG_BINS];
      fft<16, true>(v);
#pragma unroll
      for (int i = 0; i < 16; ++i) line[bitrev<16>(i) * NG_BINS] = v[i];
    }
    __syncthreads();

    // ---- x back: the bins 0 .. 8 of a real line (the real parts of bins 0 and 8) to its even and odd samples, window, scale
    {
      float2 z[8];
#pragma unroll
      for (int k = 0; k < 8; ++k) {
        float2 xk = spec[lq * NG_SLAB + ly * NG_BINS + k], xm = spec[lq * NG_SLAB + ly * NG_BINS + 8 - k];
        if (k == 0) xk.y = 0.0f, xm.y = 0.0f;
        const float2 e = make_float2(0.5f * (xk.x + xm.x), 0.5f * (xk.y - xm.y));
        const float2 o = twiddle<true>(make_float2(0.5f * (xk.x - xm.x), 0.5f * (xk.y + xm.y)), k);
        z[k] = make_float2(e.x - o.y, e.y + o.x);
      }
      fft<8, true>(z);
#pragma unroll
      for (int n = 0; n < 8; ++n) {
        const float2 v = z[bitrev<8>(n)];
        stage[lq * NG_STAGE_SLAB + ly * NG_ROW + 2 * n] = ((float)(wty * NG_WINDOW[3][2 * n]) * v.x) * a.scale;
        stage[lq * NG_STAGE_SLAB + ly * NG_ROW + 2 * n + 1] = ((float)(wty * NG_WINDOW[3][2 * n + 1]) * v.y) * a.scale;
      }
    }
    __syncthreads();

    // ---- the samples inside the image: the first pass stores, the others add, the last one marks the invalid samples
    if (in_y) {
      // what out holds is loaded for all 16 samples before the first store, so that the loads are in flight together
      float held[16];
      unsigned inside = 0;
#pragma unroll
      for (int q = 0; q < 16; ++q) {
        const int pt = ot + q % BT, px = ox + (q / BT) * 16 + cx;
        const bool in = pt >= 0 && pt < T && px >= 0 && px < W;
        inside |= (in ? 1u : 0u) << q;
        held[q] = (in && !a.first) ? a.out[(((int64_t)pt * C + c) * H + py) * W + px] : 0.0f;
      }
#pragma unroll
      for (int q = 0; q < 16; ++q) {
        if (inside >> q & 1) {
          const int pt = ot + q % BT, px = ox + (q / BT) * 16 + cx;
          float v = stage[q * NG_STAGE_SLAB + cy * NG_ROW + cx];
          if (!a.first) v = held[q] + v;
          if (a.last && !a.fill && !(ok_bits >> q & 1)) v = nan;
          a.out[(((int64_t)pt * C + c) * H + py) * W + px] = v;
        }
      }
    }
    if (n_invalid) atomicAdd(&tally[0], n_invalid);
    if (kept) atomicAdd(&tally[2], kept);
    if (total) atomicAdd(&tally[3], total);
    __syncthreads();
    if (lane < SUNERF_NOISE_GATE_STATE && tally[lane])
      atomicAdd(a.state + (int64_t)c * SUNERF_NOISE_GATE_STATE + lane, (unsigned long long)tally[lane]);
  }          // the lanes that read the tally are the ones that clear it for the next group
}

template <int BT>
void launch_pass(const NgArgs& a, hipStream_t st) {
  hipLaunchKernelGGL((noise_gate_kernel<BT>), dim3(grid_of(a.n_groups)), dim3(NG_THREADS), 0, st, a);
}

}  // namespace

extern "C" int sunerf_noise_gate_abi_version(void) { return SUNERF_NOISE_GATE_ABI_VERSION; }

extern "C" int sunerf_noise_gate(const float* frames, const uint8_t* bad, const double* params, const float* spectrum, int n_frames,
                                 int n_planes, int height, int width, int bt, int mode, int flags, double gamma, float* out,
                                 int64_t* state, void* stream) {
  if (bt != 1 && bt != 4 && bt != 8 && bt != 16) return SUNERF_E_UNSUPPORTED;
  if (mode != SUNERF_NOISE_GATE_MODE_GATE && mode != SUNERF_NOISE_GATE_MODE_WIENER) return SUNERF_E_UNSUPPORTED;
  if (flags & ~SUNERF_NOISE_GATE_FILL_INVALID) return SUNERF_E_UNSUPPORTED;
  if (n_frames >= 0 && n_planes >= 0 && height >= 0 && width >= 0 && (n_frames == 0 || n_planes == 0 || height == 0 || width == 0)) return 0;
  if (n_frames < 0 || n_planes < 0 || height < 0 || width < 0) return SUNERF_E_BADARG;
  if (!(gamma > 0.0) || !(gamma < __builtin_inf())) return SUNERF_E_BADARG;
  if (!frames || !params || !out || !state) return SUNERF_E_BADARG;
  if ((uintptr_t)params % sizeof(double) || (uintptr_t)state % sizeof(int64_t)) return SUNERF_E_BADARG;
  if ((uintptr_t)frames % sizeof(float) || (uintptr_t)spectrum % sizeof(float) || (uintptr_t)out % sizeof(float)) return SUNERF_E_BADARG;
  const size_t samples = (size_t)n_frames * n_planes * height * width;
  const struct { const void* p; size_t bytes; } in[4] = {{frames, samples * sizeof(float)}, {bad, samples},
                                                         {params, (size_t)n_planes * 4 * sizeof(double)},
                                                         {spectrum, (size_t)n_planes * bt * 256 * sizeof(float)}};
  for (const auto& r : in)
    if (r.p && (uintptr_t)out < (uintptr_t)r.p + r.bytes && (uintptr_t)r.p < (uintptr_t)out + samples * sizeof(float)) return SUNERF_E_BADARG;

  NgArgs a;
  a.frames = frames; a.bad = bad; a.params = params; a.spectrum = spectrum; a.out = out; a.state = (unsigned long long*)state;
  a.n_frames = n_frames; a.n_planes = n_planes; a.height = height; a.width = width; a.mode = mode;
  a.fill = flags & SUNERF_NOISE_GATE_FILL_INVALID;
  a.g2 = gamma * gamma;
  a.scale = (float)(1.0 / (128.0 * bt * (bt > 1 ? 3.375 : 2.25)));
  const int passes_t = bt > 1 ? 4 : 1, stride_t = bt > 1 ? bt / 4 : 1, per_group = 16 / bt;
  hipStream_t st = (hipStream_t)stream;
  SUNERF_CLEAR_ERROR();
  hipError_t e = hipMemsetAsync(state, 0, (size_t)n_planes * SUNERF_NOISE_GATE_STATE * sizeof(int64_t), st);
  if (e != hipSuccess) return (int)e;
  int pass = 0;
  for (int pt = 0; pt < passes_t; ++pt)
    for (int py = 0; py < 4; ++py)
      for (int px = 0; px < 4; ++px, ++pass) {
        a.first = pass == 0;
        a.last = pass == passes_t * 16 - 1;
        a.ot0 = bt > 1 ? pt * stride_t - (bt - stride_t) : 0;
        a.oy0 = 4 * py - 12;
        a.ox0 = 4 * px - 12;
        a.nbt = (int)(((int64_t)n_frames - a.ot0 + bt - 1) / bt);
        a.nby = (int)(((int64_t)height - a.oy0 + 15) / 16);
        const int64_t nbx = ((int64_t)width - a.ox0 + 15) / 16;
        a.ngx = (int)((nbx + per_group - 1) / per_group);
        a.n_groups = (long long)n_planes * a.nbt * a.nby * a.ngx;
        if (bt == 1) launch_pass<1>(a, st);
        else if (bt == 4) launch_pass<4>(a, st);
        else if (bt == 8) launch_pass<8>(a, st);
        else launch_pass<16>(a, st);
      }
  SUNERF_CHECK_LAUNCH();
  return 0;
}
