/* Instrument entry points of libsunerf_hip.so: a rendered frame becomes what a detector would have recorded -- correlation with
 * the point-spread function and summation of sub-pixels into detector pixels (one strided correlation), photon and read noise,
 * digitisation, saturation.  A fifth table beside sunerf_hip.h, sunerf_hip_ext.h, sunerf_hip_response.h and sunerf_hip_prep.h,
 * which stay as they are and keep their versions; the same library holds all five.  Same conventions: row-major device tensors
 * [n_planes, height, width], `stream` a hipStream_t (NULL: the default stream), status 0 on success, SUNERF_E_BADARG (-1),
 * SUNERF_E_UNSUPPORTED (-2), SUNERF_E_WORKSPACE (-3, not returned by this table: nothing here takes a workspace) or a positive
 * hipError_t; argument errors are found before anything touches a device.  The Python binding is sunerf_hip/lib.py:
 * _INSTRUMENT_SIGNATURES; the host side is sunerf_hip/instrument.py.  DESIGN.md section 8o.
 *
 * No floating-point atomics anywhere: reruns are bit-identical, and a plane alone gives the bits it gives inside a batch of
 * planes.  All arithmetic below is IEEE fp64 with every operation rounded on its own (no fused multiply-add), in the order
 * written, and one rounding to fp32 at the end. */
#ifndef SUNERF_HIP_INSTRUMENT_H
#define SUNERF_HIP_INSTRUMENT_H

#include "sunerf_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Version of THIS table; sunerf_hip/lib.py refuses a library that answers anything else. */
#define SUNERF_INSTRUMENT_ABI_VERSION 1
int sunerf_instrument_abi_version(void);

#define SUNERF_INSTRUMENT_MAX_KERNEL 96 /* rows and columns of a correlation kernel at most                                  */
#define SUNERF_INSTRUMENT_MAX_BIN 8     /* bin factor at most                                                                */
/* The correlation works on square tiles of T x T output pixels, T = min(32, (127 - max(kh, kw)) / bin + 1): the input tile with
 * its halo, ((T - 1) bin + kh) x ((T - 1) bin + kw) fp32 words, lives in LDS and is at most 127 x 127 words = 63 KiB. */
#define SUNERF_INSTRUMENT_TILE 32
/* boundary of sunerf_instrument_correlate_bin: what a tap past the edge of the plane reads */
#define SUNERF_INSTRUMENT_BOUNDARY_ZERO 0    /* 0.0                                      */
#define SUNERF_INSTRUMENT_BOUNDARY_NEAREST 1 /* the pixel at the index clamped to the plane */
/* flags of sunerf_instrument_noise */
#define SUNERF_INSTRUMENT_POISSON 1  /* n ~ Poisson(lam); else n = lam                   */
#define SUNERF_INSTRUMENT_READ 2     /* + read_noise * z, z ~ N(0, 1)                    */
#define SUNERF_INSTRUMENT_QUANTISE 4 /* dn = rint(dn), ties to even                      */
#define SUNERF_INSTRUMENT_SATURATE 8 /* saturated = dn >= saturation; dn = min(dn, saturation) */
#define SUNERF_INSTRUMENT_PARAMS 8   /* doubles per plane: unit, exposure, dn_per_photon, read_noise, pedestal, saturation, 2 reserved */
#define SUNERF_INSTRUMENT_MAX_ROUNDS 256 /* rejection rounds of the PTRS sampler at most */

/* Strided correlation: out [n_planes, height / bin, width / bin] fp32 (integer division: trailing rows and columns of `in` that
 * do not fill a detector pixel are dropped) from in [n_planes, height, width] fp32,
 *   out[p, R, C] = scale * sum_{i < kh} sum_{j < kw}  K[p or 0, i, j] * in[p, R bin + i - anchor_y, C bin + j - anchor_x]
 * with K [n_kernels, kh, kw] fp64 (device), n_kernels 1 (one kernel for all planes) or n_planes.  The sum is taken in fp64 in ONE
 * order: i ascending, inside it j ascending; each product K * (double) in is rounded, then added, and the first product starts
 * the sum (a 1 x 1 kernel of 1.0 returns the input by bits, -0.0 included); the sum is multiplied by `scale`, then rounded to
 * fp32.  A tap past the edge reads 0.0 (BOUNDARY_ZERO) or the pixel at the clamped index
 * (BOUNDARY_NEAREST).  Non-finite input propagates by IEEE rules through every tap that reads it, a tap whose K is 0 included:
 * a NaN under a zero tap is still NaN (0 * NaN), and so is an infinity under one.
 * Checked in this order: kh or kw above 96, bin above 8, a boundary other than the two: UNSUPPORTED; n_planes, height / bin or
 * width / bin 0 while no count is negative and kh, kw, bin >= 1: 0, nothing read or written; a negative count, kh, kw or bin
 * below 1, n_kernels neither 1 nor n_planes, an anchor outside [0, kh) x [0, kw), a NULL in, K or out, a K not aligned to 8
 * bytes: BADARG. */
int sunerf_instrument_correlate_bin(const float* in, int n_planes, int height, int width, const double* K, int n_kernels, int kh,
                                    int kw, int bin, int anchor_y, int anchor_x, double scale, int boundary, float* out,
                                    void* stream);

/* out [n, 4] = Philox4x32-10(ctr [n, 4], key = (key0, key1)), all uint32 (device): ten rounds of
 *   c = (hi(M1 c2) ^ c1 ^ k0, lo(M1 c2), hi(M0 c0) ^ c3 ^ k1, lo(M0 c0)),  M0 = 0xD2511F53, M1 = 0xCD9E8D57,
 * the key advanced by the Weyl constants (k0 += 0x9E3779B9, k1 += 0xBB67AE85) between two rounds (Salmon et al. 2011, the
 * Random123 known answers).  The generator of sunerf_instrument_noise, pinned apart from its use.
 * Checked in this order: n == 0: 0, nothing read or written; n < 0, a NULL ctr or out: BADARG. */
int sunerf_instrument_philox(const uint32_t* ctr, int64_t n, uint32_t key0, uint32_t key1, uint32_t* out, void* stream);

/* Detector noise, per element of expected [n_planes, height, width] fp32, with params [n_planes, 8] fp64 (device) = unit,
 * exposure, dn_per_photon (g), read_noise, pedestal, saturation, reserved, reserved of the element's plane:
 *   v   = (double) expected * unit;  v = v < 0 ? 0 : v;  lam = (v * exposure) / g
 *         lam not finite or lam > 2^52: image = sigma = NaN, saturated = 0, nothing drawn
 *   n   = Poisson(lam) (POISSON) or lam
 *   dn  = (n * g + pedestal) [+ read_noise * z (READ)]
 *   dn  = rint(dn) (QUANTISE);  saturated = dn >= saturation, dn = saturated ? saturation : dn (SATURATE; else saturated = 0)
 *   image = (float) (((dn - pedestal) / exposure) / unit)
 *   sigma = (float) ((sqrt((lam * (g * g) + read_noise * read_noise) + (QUANTISE ? 1.0 / 12.0 : 0.0)) / exposure) / unit)
 * image [n_planes, height, width] fp32; sigma (fp32) and saturated (uint8), same shape, may each be NULL.
 *
 * Randomness is counter-based, so that tiles, ranks and reruns agree: block(e, j, s) = Philox4x32-10 with
 *   key = (seed & 0xffffffff, seed >> 32),  counter = (e & 0xffffffff, e >> 32, j, s)
 * e = index_offset + the element's flat index in this call, j = 0, 1, ... the draw number, s = 0 for the photon count and 1 for
 * the read noise.  A block (w0, w1, w2, w3) gives two uniforms in (0, 1], exact in fp64:
 *   u_a = ((w0 >> 5) * 2^26 + (w1 >> 6) + 1) * 2^-53,   u_b = ((w2 >> 5) * 2^26 + (w3 >> 6) + 1) * 2^-53
 * Poisson, lam < 10: inversion with u = u_a of block(e, 0, 0):  k = 0; p = exp(-lam); s = p;
 *   while (u > s && k < 200) { k += 1; p = p * (lam / k); s = s + p; }   n = k
 * Poisson, lam >= 10: Hoermann's transformed rejection PTRS (1993) with the constants of NumPy's random_poisson_ptrs:
 *   slam = sqrt(lam); loglam = log(lam); b = 0.931 + 2.53 * slam; a = -0.059 + 0.02483 * b;
 *   invalpha = 1.1239 + 1.1328 / (b - 3.4); vr = 0.9277 - 3.6224 / (b - 2.0);
 *   round j = 0, 1, ...: U = u_a - 0.5, V = u_b of block(e, j, 0); us = 0.5 - fabs(U);
 *     k = floor(((2.0 * a) / us + b) * U + lam + 0.43);
 *     if (us >= 0.07 && V <= vr) accept k;
 *     if (k < 0 || (us < 0.013 && V > us)) next round;
 *     if ((log(V) + log(invalpha)) - log(a / (us * us) + b) <= (-lam + k * loglam) - lgamma(k + 1.0)) accept k;
 *   after SUNERF_INSTRUMENT_MAX_ROUNDS rounds without acceptance (probability below 1e-200) n = rint(lam).
 * Read noise: z = sqrt(-2.0 * log(u_a)) * cos(6.283185307179586 * u_b) of block(e, 0, 1).
 * exp, log, lgamma, cos are the device's fp64 functions: a decision above that falls within their last bits of a tie may differ
 * from another implementation of this text.
 * Checked in this order: flag bits above 15: UNSUPPORTED; n_planes, height or width 0 and none negative: 0, nothing read or
 * written; a negative count or index_offset, a NULL expected, params or image, params not aligned to 8 bytes: BADARG. */
int sunerf_instrument_noise(const float* expected, int n_planes, int height, int width, const double* params, uint64_t seed,
                            int64_t index_offset, int flags, float* image, float* sigma, uint8_t* saturated, void* stream);

#ifdef __cplusplus
}
#endif
#endif
