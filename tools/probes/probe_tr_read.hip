// Hardware probe: ds_read_b64_tr_b16 under the three LDS images measured for bwd_pipe.hip (unskewed, pair skew -- the shipped one --, pair skew + row swizzle).
//   1. semantics: does each lane's address feed only its own 8 bytes?  A fragment pair is filled with 16-bit values that name
//      their own byte address; from the shipped (affine) pattern the map (lane, element) -> (lane whose address was used, element
//      of its 8 bytes) is derived, and every other pattern -- the pair skew, skew + row swizzle, and a scrambled one with no
//      structure at all -- must return addr[that lane] + 2 * element under the SAME map.
//   2. cost: 64 back-to-back reads between two s_memtime stamps (offsets as in the kernel: k-step * 256, second read + 64), one
//      wave and then eight waves on one CU; clocks per instruction.
// Build: hipcc --offload-arch=gfx950 -O2 -o probe_tr_read probe_tr_read.hip
#include <hip/hip_runtime.h>
#include <cstdio>
#include <cstdlib>
#include <vector>
#include <algorithm>

constexpr int LDS_BYTES = 8192;
constexpr int N_PAT = 4, REPS = 64;
const char* const PAT_NAME[N_PAT] = {"shipped", "pair skew", "pair skew + row swizzle", "scrambled (no structure)"};

// lane part of the address, patterns 0..2 as in bwd_pipe.hip; 3: the 64 lanes' 8-byte slots in a pseudo-random order
__host__ __device__ inline unsigned lane_offset(int pat, int lane) {
  const int g = lane >> 4, i = lane & 15, q = i >> 2, p = i & 3;
  int row = (p >> 1) * 32 + 8 * (g >> 1) + q;
  if (pat == 3) return (unsigned)((lane * 37 + 11) & 63) * 24 + 8 * ((lane * 5) & 1);      // distinct 8-byte slots, 24 B apart
  if (pat == 2) row ^= 8 * (row >> 5);
  return (g & 1) * (pat ? 1088 : 1024) + row * 16 + (p & 1) * 8;
}

__global__ void semantics_kernel(int pat, int imm64, unsigned short* out) {
  extern __shared__ __attribute__((aligned(16))) unsigned short lds[];
  for (int i = threadIdx.x; i < LDS_BYTES / 2; i += 64) lds[i] = (unsigned short)(2 * i);      // value = own byte address
  __syncthreads();
  const unsigned addr = (unsigned)(uintptr_t)lds + lane_offset(pat, threadIdx.x);
  unsigned r0, r1;
  if (imm64) asm volatile("ds_read_b64_tr_b16 v[2:3], %2 offset:64\n\ts_waitcnt lgkmcnt(0)\n\tv_mov_b32 %0, v2\n\tv_mov_b32 %1, v3" : "=v"(r0), "=v"(r1) : "v"(addr) : "v2", "v3", "memory");
  else asm volatile("ds_read_b64_tr_b16 v[2:3], %2\n\ts_waitcnt lgkmcnt(0)\n\tv_mov_b32 %0, v2\n\tv_mov_b32 %1, v3" : "=v"(r0), "=v"(r1) : "v"(addr) : "v2", "v3", "memory");
  unsigned short* o = out + threadIdx.x * 4;
  o[0] = r0 & 0xffffu; o[1] = r0 >> 16; o[2] = r1 & 0xffffu; o[3] = r1 >> 16;
}

#define RD(d, off) "ds_read_b64_tr_b16 " d ", %2 offset:" #off "\n\t"
#define RD8(k) RD("v[2:3]", k * 256) RD("v[4:5]", k * 256 + 64) RD("v[6:7]", k * 256 + 1024) RD("v[8:9]", k * 256 + 1088) \
               RD("v[10:11]", k * 256 + 2048) RD("v[12:13]", k * 256 + 2112) RD("v[14:15]", k * 256 + 3072) RD("v[16:17]", k * 256 + 3136)

// every wave: REPS stamp pairs around 64 reads each; out[wave][rep] = {begin, end}
__global__ void timing_kernel(int pat, unsigned long long* out) {
  extern __shared__ __attribute__((aligned(16))) unsigned short lds[];
  for (int i = threadIdx.x; i < LDS_BYTES / 2; i += blockDim.x) lds[i] = (unsigned short)(2 * i);
  __syncthreads();
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const unsigned addr = (unsigned)(uintptr_t)lds + lane_offset(pat, lane);
  for (int rep = 0; rep < REPS; ++rep) {
    unsigned long long t0, t1;
    __syncthreads();
    asm volatile("s_memtime %0\n\ts_waitcnt lgkmcnt(0)\n\t"
                 RD8(0) RD8(1) RD8(2) RD8(3) RD8(0) RD8(1) RD8(2) RD8(3)
                 "s_waitcnt lgkmcnt(0)\n\ts_memtime %1\n\ts_waitcnt lgkmcnt(0)"
                 : "=&s"(t0), "=&s"(t1) : "v"(addr)
                 : "v2", "v3", "v4", "v5", "v6", "v7", "v8", "v9", "v10", "v11", "v12", "v13", "v14", "v15", "v16", "v17", "memory");
    if (lane == 0) { out[(wave * REPS + rep) * 2] = t0; out[(wave * REPS + rep) * 2 + 1] = t1; }
  }
}

#define CHECK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { printf("%s: %s\n", #x, hipGetErrorString(e_)); return 1; } } while (0)

int main() {
  unsigned short* d_out;
  unsigned long long* d_t;
  CHECK(hipMalloc(&d_out, 64 * 4 * 2));
  CHECK(hipMalloc(&d_t, 8 * REPS * 2 * 8));

  // bank arithmetic of the patterns (64 banks of 4 bytes; one read is 128 dwords: floor 2 per bank)
  printf("== bank arithmetic (host): banks touched / max dwords per bank ==\n");
  for (int pat = 0; pat < N_PAT; ++pat) {
    printf("%-26s", PAT_NAME[pat]);
    for (int part = 0; part < 3; ++part) {
      int cnt[64] = {0}, touched = 0, mx = 0;
      const int lo = part == 2 ? 32 : 0, hi = part == 1 ? 32 : 64;
      for (int l = lo; l < hi; ++l) { const unsigned o = lane_offset(pat, l); cnt[(o / 4) & 63]++; cnt[(o / 4 + 1) & 63]++; }
      for (int b = 0; b < 64; ++b) { touched += cnt[b] > 0; mx = std::max(mx, cnt[b]); }
      printf("  %s %2d / %d", part == 0 ? "64 lanes" : part == 1 ? "lanes 0-31" : "lanes 32-63", touched, mx);
    }
    printf("\n");
  }

  // ---- 1. semantics ----
  printf("\n== semantics: which source bytes each lane receives ==\n");
  int src_lane[64][4], src_el[64][4];
  bool all_ok = true;
  for (int pat = 0; pat < N_PAT; ++pat)
    for (int imm = 0; imm < 2; ++imm) {
      CHECK(hipMemset(d_out, 0xff, 64 * 4 * 2));
      hipLaunchKernelGGL(semantics_kernel, dim3(1), dim3(64), LDS_BYTES, 0, pat, imm, d_out);
      CHECK(hipDeviceSynchronize());
      std::vector<unsigned short> r(256);
      CHECK(hipMemcpy(r.data(), d_out, 512, hipMemcpyDeviceToHost));
      if (pat == 0 && imm == 0) {
        // the map, from the shipped pattern: the lanes' 8-byte ranges are disjoint there, so the owner of a byte is unique
        for (int l = 0; l < 64; ++l)
          for (int e = 0; e < 4; ++e) {
            src_lane[l][e] = -1;
            for (int m = 0; m < 64; ++m) {
              const unsigned a = lane_offset(0, m);
              if (r[l * 4 + e] >= a && r[l * 4 + e] < a + 8) { src_lane[l][e] = m; src_el[l][e] = (r[l * 4 + e] - a) / 2; }
            }
          }
        printf("map derived from the shipped pattern, lane: element e <- (address of lane M, its 16-bit element k) as M.k\n");
        for (int l = 0; l < 64; ++l) {
          printf("  lane %2d:", l);
          for (int e = 0; e < 4; ++e) printf(" %2d.%d", src_lane[l][e], src_el[l][e]);
          printf((l & 3) == 3 ? "\n" : "   ");
        }
        bool own_block = true;
        for (int l = 0; l < 64; ++l) for (int e = 0; e < 4; ++e) own_block = own_block && src_lane[l][e] >= 0 && (src_lane[l][e] >> 4) == (l >> 4);
        printf("every element comes from an address of the lane's own 16-lane block: %s\n", own_block ? "yes" : "NO");
      }
      int bad = 0, first_bad = -1;
      for (int l = 0; l < 64; ++l)
        for (int e = 0; e < 4; ++e) {
          const int m = src_lane[l][e];
          const unsigned want = m < 0 ? 0xffffu : lane_offset(pat, m) + 64 * imm + 2 * src_el[l][e];
          if (r[l * 4 + e] != want) { if (first_bad < 0) first_bad = l; ++bad; }
        }
      printf("%-26s offset:%-2d  %3d of 256 elements differ from addr[M] + 2 k under that map%s\n", PAT_NAME[pat], 64 * imm, bad,
             bad ? "  <-- the lanes' addresses are NOT independent" : "");
      if (bad) {
        all_ok = false;
        printf("  first differing lane %d: received bytes", first_bad);
        for (int e = 0; e < 4; ++e) printf(" %u", r[first_bad * 4 + e]);
        printf("; all lanes' received byte addresses:\n");
        for (int l = 0; l < 64; ++l) printf("  lane %2d (addr %4u): %4u %4u %4u %4u\n", l, lane_offset(pat, l) + 64 * imm, r[l * 4], r[l * 4 + 1], r[l * 4 + 2], r[l * 4 + 3]);
      }
    }
  printf("verdict: %s\n", all_ok ? "each lane's address feeds only its own 8 bytes: any per-lane pattern (the row swizzle included) reads correctly"
                                 : "see the differing patterns above");

  // ---- 2. cost ----
  printf("\n== cost: 64 back-to-back reads per stamp pair, %d stamp pairs, s_memtime ticks per instruction ==\n", REPS);
  for (int waves = 1; waves <= 8; waves *= 8)
    for (int pat = 0; pat < 3; ++pat) {
      hipLaunchKernelGGL(timing_kernel, dim3(1), dim3(64 * waves), LDS_BYTES, 0, pat, d_t);
      CHECK(hipDeviceSynchronize());
      std::vector<unsigned long long> t(8 * REPS * 2);
      CHECK(hipMemcpy(t.data(), d_t, t.size() * 8, hipMemcpyDeviceToHost));
      // per wave: median over the stamp pairs; all waves: (latest end - earliest begin) of a repetition over waves * 64 reads
      std::vector<double> per, agg;
      for (int rep = REPS / 2; rep < REPS; ++rep) {
        unsigned long long b = ~0ull, e = 0;
        for (int w = 0; w < waves; ++w) {
          const unsigned long long t0 = t[(w * REPS + rep) * 2], t1 = t[(w * REPS + rep) * 2 + 1];
          per.push_back((double)(t1 - t0) / 64.0);
          b = std::min(b, t0); e = std::max(e, t1);
        }
        agg.push_back((double)(e - b) / (64.0 * waves));
      }
      std::sort(per.begin(), per.end()); std::sort(agg.begin(), agg.end());
      printf("%d wave%s  %-26s per wave: median %.2f (min %.2f)   CU-wide: median %.2f ticks per instruction\n", waves, waves > 1 ? "s" : " ",
             PAT_NAME[pat], per[per.size() / 2], per[0], agg[agg.size() / 2]);
    }
  return 0;
}
