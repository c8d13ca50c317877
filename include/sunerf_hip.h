/*
 * sunerf_hip.h -- C ABI of the MI355X (gfx950) SuNeRF ray-march renderer.
 *
 * The reference (FrontierDevelopmentLab/2024-HL-SPI3S-SuNeRF) has no FFI / plugin registry: its hot path is
 * the Python class API of sunerf.rendering + sunerf.model + sunerf.train.sampling.  This
 * header is the drop-in boundary *under* that API: every entry point replaces a span of aten ops of one
 * reference function (cited per function, paths relative to the reference root) and is called by the Python
 * mirror classes in 2024-hl-spi3s-sunerf_amd/sunerf/ through ctypes.
 *
 * Conventions
 *   - all pointers are DEVICE pointers (HIP, same device as `stream`) unless the name ends in `_host`;
 *   - fp32 row-major contiguous tensors, shapes given per argument;
 *   - no allocation, no host synchronisation, no ownership transfer: callers own inputs, outputs and
 *     workspaces; every call is asynchronous on `stream` (a hipStream_t passed as void*);
 *   - returns 0 on success, a negative SUNERF_E_* code on argument errors, a positive hipError_t if a launch
 *     failed.  The Python side turns non-zero into RuntimeError / ValueError.
 *   - thread-safe / re-entrant: no global mutable state (evaluation/loader.py:226-229 calls the renderer from
 *     a ThreadPoolExecutor).
 *   - a kernel reads and writes exactly the extents given per argument, whatever the launch is rounded up to, and no
 *     result depends on what an output or a workspace held before the call (unless the argument is documented as
 *     accumulated into, updated in place or zeroed by the caller); a workspace of the size its *_bytes() query returns
 *     is enough, a smaller one is refused with SUNERF_E_WORKSPACE before anything is queued
 *     (tests/test_gpu_abi_extents.py holds every entry point to this between guard words).
 *   - an empty batch (a count of zero rays, points, pixels, columns, voxels, slots, rows or images) is handled per entry
 *     point, in one of three ways (each checked by tests/test_gpu_abi_extents.py):
 *       returns 0 and touches no buffer: sunerf_sample_z, _hier_resample, _sample_pdf, _emission_render_fwd, _mlp_points_fwd,
 *         _emission_integral_fwd, _mlp_dgrad, _dt_integral_fwd, _thomson_integral_fwd, _dem_integral, _column_stats,
 *         _simple_star_field(_dev), _mhd_field(_points), _grid_field_fwd, _observer_rays, _column_rays, _build_ray_pool,
 *         _synchronic_map (n_rows == 0), _grid_points, _field_quantities, _image_metrics, _dem_invert, _clip_adam_step;
 *       returns 0 and writes the gradient of nothing: sunerf_emission_integral_bwd / _thomson_integral_bwd clear g_absmax,
 *         sunerf_dt_integral_bwd(_full) clear g_log_abs, g_vol_c and g_absmax, and with accumulate == 0 sunerf_mlp_wgrad
 *         zeroes every grad_weights / grad_biases tensor, sunerf_grid_field_bwd g_values and sunerf_simple_star_bwd g_params
 *         (accumulate != 0: left as they are);
 *       is SUNERF_E_BADARG, nothing written: sunerf_mlp_backward_pipe, _mlp_backward_exact, _mlp_backward_exact_chunked and
 *         _mlp_input_grad_exact (n_rays >= 1), sunerf_training_loss (n >= 1), sunerf_map_fill and sunerf_reproject_views
 *         (n_pixels >= 1), sunerf_volume_metrics (every n >= 1).
 */
#ifndef SUNERF_HIP_H
#define SUNERF_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SUNERF_ABI_VERSION 9

#define SUNERF_E_BADARG   (-1)   /* null pointer / non-positive size                               */
#define SUNERF_E_UNSUPPORTED (-2) /* d_filter / n_layers / sample count outside the compiled set     */
#define SUNERF_E_WORKSPACE (-3)  /* workspace too small                                             */

#define SUNERF_MAX_LAYERS 16     /* Linear layers per MLP including in_layer and out_layer          */
#define SUNERF_ENC_DIM    84     /* PositionalEncoding(d_input=4, n_freqs=10).d_output, model.py:109 */

/* forward arithmetic of the MLP products x*w (x, w split into fp16 head + exact fp32 remainder); the packed image and the
 * render call must name the same mode.
 *   FAST  : head*head on the fp16 matrix cores + the two cross terms as block-scaled fp8 products
 *           (v_mfma_scale_f32_32x32x64_f8f6f4); raw MLP output within ~1e-5 |raw| rms (4e-5 |raw| worst sample) of fp32,
 *           i.e. images ~1e-5 rel for |raw| ~ 1: inside the 1e-4 parity gate; 18 % (d_filter 256) / 23 % (512) faster
 *   EXACT : all three terms as fp16 products (fp32-class results, raw within ~1e-7)
 *   HALF  : (opt-in) single fp16 operands, fp32 accumulate: the head product only.  This is the
 *           "bf16 MLP weights on MFMA" class of BASELINE.json config 3 (with fp16's 11-bit instead of bf16's 8-bit
 *           mantissa): results follow an fp16-emulating evaluation to 1e-4 and deviate from fp32 by ~1e-3; it does NOT meet
 *           the 1e-4-vs-fp32 parity gate and is never the default */
#define SUNERF_PRECISION_FAST  0
#define SUNERF_PRECISION_EXACT 1
#define SUNERF_PRECISION_HALF  2

/* sampler kinds -- sunerf/train/sampling.py */
#define SUNERF_SAMPLER_STRATIFIED 0   /* StratifiedSampler.forward  sampling.py:68-102 */
#define SUNERF_SAMPLER_SPHERICAL  1   /* SphericalSampler.forward   sampling.py:16-54  */

int sunerf_abi_version(void);

/* ------------------------------------------------------------------------------------------------------------
 * Weight packing.  The fused renderer consumes the MLP weights as fp16 hi/lo pairs (w = hi + lo, |err| <= 2^-22
 * relative) stored in MFMA A-fragment order, plus fp32 biases.  Must be re-run after every optimiser step.
 *
 * Replaces: nothing numerically -- it is a re-layout of the nn.Linear parameters of NeRF (model.py:28-42).
 *
 *   weights_host[i] -> device fp32 W_i [out_i, in_i] row-major (nn.Linear layout), i = 0..n_linear-1
 *   biases_host[i]  -> device fp32 b_i [out_i]
 *   n_linear = n_layers + 1 : in_layer (84 -> d_filter), n_layers-1 hidden (d_filter -> d_filter), out_layer
 *   packed: device buffer of sunerf_packed_mlp_bytes() bytes, 16-byte aligned; every byte of it is written in every mode (the
 *           scale block that only FAST uses is zero otherwise), so two packs of one model are the same bytes
 *   precision: SUNERF_PRECISION_FAST / _EXACT (above); selects the stream format of the hidden and out layers
 * ---------------------------------------------------------------------------------------------------------- */
size_t sunerf_packed_mlp_bytes(int d_filter, int n_linear);

int sunerf_pack_mlp(const float* const* weights_host, const float* const* biases_host, int n_linear,
                    int d_filter, int d_out, int precision, void* packed, void* stream);

/* ------------------------------------------------------------------------------------------------------------
 * Sample placement along rays.
 * Replaces StratifiedSampler.forward sampling.py:68-98 / SphericalSampler.forward sampling.py:16-49 (z_vals only;
 * the points o + d*z of :100 / :52 are formed inside the render kernel and never materialised).
 *
 *   rays_o, rays_d [N,3]; t_vals [S] (the module buffer, sampling.py:65-66); t_rand [N,S] or NULL
 *   (perturb=False); distance = sampler.distance buffer, solar_R = sampler.solar_R buffer; z_vals out [N,S]
 * ---------------------------------------------------------------------------------------------------------- */
int sunerf_sample_z(int sampler_kind, const float* rays_o, const float* rays_d, const float* t_vals,
                    const float* t_rand, int64_t n_rays, int n_samples, float distance, float solar_R,
                    float* z_vals, void* stream);

/* ------------------------------------------------------------------------------------------------------------
 * Fused render pass: points -> time concat -> positional encoding -> MLP -> emission/absorption integral.
 * Replaces, for one coarse or fine pass:
 *   sampling.py:100 (points), base_tracing.py:64-65 / :83-84 (time concat), base_tracing.py:118-129 (_render),
 *   model.py:123-132 (PositionalEncoding.forward), model.py:44-57 (NeRF.forward), emission.py:14-54
 *   (raw2outputs), base_tracing.py:135-156 (cumprod_exclusive), and the epilogues base_tracing.py:99-110
 *   (absorption_map, distance, height_map, regularization with defect D2 resolved to (N,S)).
 *
 *   packed     : sunerf_pack_mlp output for this pass's model
 *   rays_o/d   : [N,3]; times [N] (the (N,1) column); z_vals [N,S]
 *   image      : [N]    sum_S I*T                                  (emission.py:46)
 *   weights    : [N,S]  I*T / (sum + 1e-10)                        (emission.py:49-50)
 *   absorption : [N,S]  exp(-relu(r1)*dists)  'regularizing_quantity' (emission.py:35)
 *   raw        : [N,S,2] MLP output ('inferences'), may be NULL
 *   height_map, absorption_map : [N] or NULL;  regularization : [N,S] or NULL  (base_tracing.py:99-106)
 *   reg_radius : 1.2 / Rs_per_ds (base_tracing.py:44)
 *   act_stash  : NULL for inference; for training a device buffer of sunerf_act_stash_bytes() bytes that
 *                receives the hidden activations for the backward kernels
 *   stash_format: SUNERF_STASH_FP16 -- fp16 sin and fp16 cos of every activation (8.2 KB per sample of an 8 x 256 network): what
 *                sunerf_mlp_dgrad / sunerf_mlp_wgrad read -- or SUNERF_STASH_PHASE -- the 16-bit phase of every pre-activation
 *                (4.1 KB per sample; sin and cos to 4.8e-5 from it): what sunerf_mlp_backward_pipe reads; d_filter = 256 only
 *   workspace  : sunerf_render_workspace_bytes(d_filter) bytes of device scratch (may be NULL when that is 0)
 *   n_samples >= 2 (the first interval of emission.py:19-26 is the second one, duplicated): a single sample is
 *   SUNERF_E_BADARG, here and in sunerf_emission_integral_fwd / _bwd, sunerf_mlp_dgrad, sunerf_mlp_wgrad and
 *   sunerf_mlp_backward_pipe
 * ---------------------------------------------------------------------------------------------------------- */
#define SUNERF_STASH_FP16  0
#define SUNERF_STASH_PHASE 1
size_t sunerf_act_stash_bytes(int64_t n_rays, int n_samples, int d_filter, int n_linear, int stash_format);
/* d_filter = 512 (the reference's default width, model.py:16): scratch for layer outputs; 0 for narrower nets */
size_t sunerf_render_workspace_bytes(int d_filter);

int sunerf_emission_render_fwd(const void* packed, int d_filter, int n_linear, int precision,
                               const float* rays_o, const float* rays_d, const float* times,
                               const float* z_vals, int64_t n_rays, int n_samples,
                               float* image, float* weights, float* absorption, float* raw,
                               float* height_map, float* absorption_map, float* regularization,
                               float reg_radius, void* act_stash, int stash_format, void* workspace,
                               size_t workspace_bytes, void* stream);

/* NeRF.forward on free-standing query points, model.py:44-57 (positional encoding + sine MLP, no ray, no integral): the fused
 * render kernel fed with explicit points.  points [M,4] = (x, y, z, t), M a multiple of 32 (callers pad); raw [M,2].
 * act_stash (optional): as in sunerf_emission_render_fwd with n_rays = M / 32, n_samples = 32 -- sunerf_mlp_dgrad /
 * sunerf_mlp_wgrad then take g_raw [M/32, 32, 2] (a loss on arbitrary points trains, as the reference's module call does).
 * Serves evaluation/loader.py:load_coords (volume queries) at the kernel's full rate. */
int sunerf_mlp_points_fwd(const void* packed, int d_filter, int n_linear, int precision, const float* points,
                          int64_t n_points, float* raw, void* act_stash, int stash_format, void* workspace, size_t workspace_bytes,
                          void* stream);

/* ------------------------------------------------------------------------------------------------------------
 * Backward of the fused render pass (training).  The reference has no backward code of its own: these entry points
 * replace what torch.autograd derives from base_tracing.py:118-129 + emission.py:14-54 + model.py:44-57 for the
 * loss of sunerf/model/sunerf.py:110-120 (gradients w.r.t. the MLP parameters only: sampling.py:120 detaches the
 * resampled z, so nothing flows to the ray geometry).  Call order for one pass:
 *
 *   sunerf_emission_render_fwd(..., act_stash != NULL)       forward, stashes fp16 sin / cos fragments
 *   sunerf_emission_integral_bwd                             g_image (N), g_reg (N,S) -> g_raw (N,S,2), max |g_raw|
 *   sunerf_mlp_dgrad                                         dZ of every layer -> dz_stash (fp16, scaled)
 *   sunerf_mlp_wgrad                                         dW, db of every Linear layer (nn.Linear layouts)
 *
 *   packedT  : sunerf_pack_mlp_t output (transposed fp16 weight image, each layer times a power of two chosen from the layer's
 *              own weights so that the data gradient keeps the scale of g_raw from layer to layer; the same buffer goes to
 *              sunerf_mlp_dgrad and sunerf_mlp_wgrad), re-pack after every optimiser step; sunerf_packed_mlp_t_bytes() bytes,
 *              every one of them written (the tail holds SUNERF_MAX_LAYERS floats: the sum of squares of every layer's weights
 *              behind the first, 0 in the slots no layer owns)
 *   g_reg    : (N,S) gradient w.r.t. the 'regularization' output, or NULL with g_reg_const (the usual
 *              lambda / (N*S) of regularization.mean(), sunerf.py:118-119)
 *   g_absmax : 4-byte device scratch (bit pattern of max |g_raw|; selects the fp16 gradient scale on the device)
 *   workspace: sunerf_wgrad_workspace_bytes(d_filter, n_linear, split) bytes; split = number of partial sums per layer
 *   accumulate != 0 adds to grad_* instead of overwriting (autograd .grad accumulation)
 * ---------------------------------------------------------------------------------------------------------- */
size_t sunerf_packed_mlp_t_bytes(int d_filter, int n_linear);
int sunerf_pack_mlp_t(const float* const* weights_host, int n_linear, int d_filter, int d_out, void* packedT,
                      void* stream);
size_t sunerf_dz_stash_bytes(int64_t n_rays, int n_samples, int d_filter, int n_linear);
size_t sunerf_wgrad_workspace_bytes(int d_filter, int n_linear, int split);

/* EmissionRadiativeTransfer.raw2outputs (sunerf/rendering/emission.py:14-54, cumprod_exclusive base_tracing.py:135-156) on a
 * GIVEN raw tensor -- the subclass hook SuNeRFRendering._render calls (base_tracing.py:128): raw (N,S,2), z_vals (N,S),
 * rays_d (N,3) -> image (N), weights (N,S), absorption (N,S) = the 'regularizing_quantity'.  (Inside
 * sunerf_emission_render_fwd the same arithmetic is fused behind the MLP.)  n_samples >= 2. */
int sunerf_emission_integral_fwd(const float* raw, const float* z_vals, const float* rays_d, int64_t n_rays, int n_samples,
                                 float* image, float* weights, float* absorption, void* stream);

/* g_weights / g_absorption: optional (N,S) gradients w.r.t. the 'weights' and 'regularizing_quantity' outputs of
 * raw2outputs (NULL on the training path, whose loss only reads image and regularization).  g_raw (N,S,2) is overwritten;
 * g_absmax (4 bytes, required) is cleared by every call, an empty batch (n_rays == 0) included, and then raised to max |g_raw| */
int sunerf_emission_integral_bwd(const float* raw, const float* z_vals, const float* rays_o, const float* rays_d,
                                 const float* g_image, const float* g_reg, const float* g_weights, const float* g_absorption,
                                 float g_reg_const, float reg_radius, int64_t n_rays, int n_samples, float* g_raw,
                                 void* g_absmax, void* stream);

int sunerf_mlp_dgrad(const void* packedT, int d_filter, int n_linear, const float* g_raw, const void* g_absmax,
                     const void* act_stash, void* dz_stash, int64_t n_rays, int n_samples, void* stream);

/* packedT: the SAME transposed image sunerf_mlp_dgrad ran with -- sunerf_pack_mlp_t folds a power of two per layer into it
 * that keeps the data gradient at the scale of g_raw from layer to layer (fp16 operands), and the sums are divided by
 * those powers here */
int sunerf_mlp_wgrad(int d_filter, int n_linear, int d_out, const void* packedT, const void* act_stash,
                     const void* dz_stash, const float* g_raw, const void* g_absmax, int64_t n_rays, int n_samples,
                     void* workspace, int split, float* const* grad_weights_host, float* const* grad_biases_host,
                     int accumulate, void* stream);

/* Layer-pipelined backward (d_filter = 256, n_linear >= 3, a 256-CU device): sunerf_mlp_dgrad + sunerf_mlp_wgrad in one
 * pass that never writes the hidden layers' dZ to HBM (csrc/bwd_pipe.hip).  Replaces the same autograd span of
 * sunerf/model/model.py:44-57.  A streaming prologue forms dZ of the last activation layer and the out layer's dW / db; then
 * one persistent launch in which pairs of workgroups own one Linear layer each (its dW accumulators and W^T rows stay in
 * registers) and hand dZ from layer to layer through the L2 of the XCD they share.
 *   act_stash: written by the forward with stash_format = SUNERF_STASH_PHASE [ABI 9] (the 16-bit phase of every pre-activation:
 *              half the bytes of the fp16 sin + cos stash the two-kernel backward reads; decoded inside the kernel)
 *   workspace: sunerf_bwd_pipe_workspace_bytes(...) bytes (0 = configuration not supported: use dgrad + wgrad).  Its first 256
 *              bytes (SUNERF_PIPE_WS_STICKY) are a STICKY STATUS block that belongs to the caller: zero it once after the
 *              allocation; word 0 is only ever raised by the library, to the largest launch status seen: 0 = every launch since
 *              the caller last cleared it ran to the end; non-zero = a launch gave up (1: its workgroups were not co-resident,
 *              2: a class of workgroups was not placed on one XCD, 3: a hand-off timed out) -- the gradients of THAT call are
 *              NaN (the optimiser's non-finite guard skips the step) and the caller should fall back to sunerf_mlp_dgrad +
 *              sunerf_mlp_wgrad.  One workspace may serve any number of launches between two looks at the word (the
 *              per-launch control block behind it is cleared in front of every launch; a give-up of an earlier launch
 *              survives later ones here).  Debug counters (flags bit 1): 64 KiB at SUNERF_PIPE_WS_DEBUG.
 *   flags    : bit 0 = single fp16 W^T in the data gradient (default: fp16 head + fp16 remainder, as sunerf_mlp_dgrad);
 *              bit 1 = per-workgroup debug counters; bit 7 = bracket the pipelined kernel of this call with library-owned
 *              HIP events on `stream` (read and released by sunerf_bwd_pipe_kernel_time: bench.py's roofline line times the
 *              dominant kernel without changing the call sequence users run);
 *              bit 8 = TEST HOOK: the placement check of workgroup class 0 fails, so the launch gives up the way a really
 *              misplaced one would (status 2, NaN gradients) -- tests/test_gpu_pipe.py exercises the fallback with it
 * Requires that no other kernel holds CUs of the device while it runs long enough to starve it (all 256 workgroups must
 * become resident; every wait is bounded, so a starved launch gives up instead of hanging).
 * sunerf_bwd_pipe_kernel_time: waits for the timed launches (flags bit 7) issued so far by this process, returns the sum of
 * their kernel durations (ms) and their number, and forgets them. */
#define SUNERF_PIPE_WS_STICKY 0
#define SUNERF_PIPE_WS_DEBUG  256
size_t sunerf_bwd_pipe_workspace_bytes(int64_t n_rays, int n_samples, int d_filter, int n_linear);
int sunerf_mlp_backward_pipe(int d_filter, int n_linear, int d_out, const void* packedT, const void* act_stash,
                             const float* g_raw, const void* g_absmax, int64_t n_rays, int n_samples, void* workspace,
                             size_t workspace_bytes, float* const* grad_weights_host, float* const* grad_biases_host,
                             int accumulate, int flags, void* stream);
int sunerf_bwd_pipe_kernel_time(double* total_ms, int* launches);

/* The same gradients in the REFERENCE's arithmetic, for small batches: every product and sum in fp32 (fp32-input MFMA), the
 * forward activations recomputed in fp32 from the query points (the fp16 activation stash is not read).  Replaces
 * torch.autograd over sunerf/model/model.py:44-57 + 123-132 where the fp16 kernels above are not the right tool: their
 * operands (dZ, cos, H) carry 2^-12 of relative rounding error per term, which a training batch averages away but a sum over a
 * few hundred samples that cancels to a few per cent of its terms does not (bias gradients of tiny batches: 2e-3 ... 3e-2).
 *   weights / biases          : host arrays of n_linear DEVICE pointers, nn.Linear layouts of the kernel shapes
 *                               ([d_filter][84], [d_filter][d_filter] ..., [d_out][d_filter]; fp32)
 *   query points              : either rays (rays_o, rays_d (N,3), times (N), z_vals (N,S); points = o + d z as sampling.py:100
 *                               forms them) or `points` (N*S, 4) given explicitly (then the ray arguments may be NULL)
 *   g_raw (N,S,d_out)         : gradient w.r.t. the raw MLP output (no scaling convention: plain fp32)
 *   workspace                 : sunerf_mlp_backward_exact_workspace_bytes(N*S, d_filter, n_linear) bytes
 *   grad_weights / grad_biases: as sunerf_mlp_wgrad (overwritten, or added to when accumulate != 0)
 * Cost ~ 0.25 us per sample of an 8 x 256 network: meant for <= a few thousand samples (sunerf_hip/ops.py picks it by count). */
size_t sunerf_mlp_backward_exact_workspace_bytes(int64_t n_points, int d_filter, int n_linear);
int sunerf_mlp_backward_exact(const float* const* weights_host, const float* const* biases_host, int n_linear, int d_filter,
                              int d_out, const float* rays_o, const float* rays_d, const float* times, const float* z_vals,
                              const float* points, int64_t n_rays, int n_samples, const float* g_raw, void* workspace,
                              size_t workspace_bytes, float* const* grad_weights_host, float* const* grad_biases_host,
                              int accumulate, void* stream);

/* The same gradients, same arithmetic, at ANY batch size (opt-in: SUNERF_BACKWARD_PRECISION=exact, sunerf_hip/ops.py).  Replaces
 * torch.autograd over sunerf/model/model.py:44-57 + 123-132 for a whole training batch.  The samples run in chunks of 32768
 * (16384 at d_filter > 256): per chunk the encoder features and the fp32 forward are recomputed and the chunk's weight and bias
 * gradients are added into fp64 accumulators in a fixed order (no atomics: two runs give bit-identical gradients); the GEMMs are
 * LDS-tiled fp32-input MFMA.  The workspace depends on (d_filter, n_linear) only.
 *   arguments                 : as sunerf_mlp_backward_exact; d_out 1 or 2; N*S up to 2^40 samples
 *   workspace                 : sunerf_mlp_backward_exact_chunked_workspace_bytes(d_filter, n_linear) bytes */
size_t sunerf_mlp_backward_exact_chunked_workspace_bytes(int d_filter, int n_linear);
int sunerf_mlp_backward_exact_chunked(const float* const* weights_host, const float* const* biases_host, int n_linear,
                                      int d_filter, int d_out, const float* rays_o, const float* rays_d, const float* times,
                                      const float* z_vals, const float* points, int64_t n_rays, int n_samples,
                                      const float* g_raw, void* workspace, size_t workspace_bytes,
                                      float* const* grad_weights_host, float* const* grad_biases_host, int accumulate,
                                      void* stream);

/* Gradients w.r.t. the QUERY of the MLP -- points, or rays / times / sample positions -- in the arithmetic of the chunked kernel
 * above, with that kernel's parameter gradients alongside on request.  Replaces torch.autograd of sunerf/model/model.py:44-57 +
 * 123-132 (and sampling.py:100's o + d z) w.r.t. its inputs: NeRF(points) differentiated w.r.t. `points`, a raw2outputs loss
 * differentiated w.r.t. the rays.  Per chunk of samples the same fp32 forward and data-gradient chain run down to dZ_0, then
 * g_enc = dZ_0 W_0 (84 columns, fp32-input MFMA), the derivative of the positional encoding from the chunk's own sin / cos
 * features, and in ray mode the per-ray sums in fp64 (fixed sample order, a ray straddling a chunk seam carried into the next
 * chunk; no atomics: two runs are bit-identical).
 *   arguments                 : as sunerf_mlp_backward_exact_chunked, except that grad_weights / grad_biases may both be NULL
 *                               (input gradients only: no weight-gradient GEMMs, column sums or fp64 accumulation); given, they
 *                               are bit-identical to sunerf_mlp_backward_exact_chunked's for the same inputs
 *   grad_points (N*S, 4)      : points mode (points != NULL): required; every ray gradient NULL
 *   grad_rays_o, grad_rays_d  : ray mode: (N, 3) each; grad_times (N); grad_z (N, S); any of them NULL (not written), at least
 *                               one given, grad_points NULL.  Always overwritten (no accumulate)
 *   workspace                 : sunerf_mlp_input_grad_exact_workspace_bytes(d_filter, n_linear) bytes
 * Cost: the chunked kernel's forward and data-gradient GEMMs (its weight-gradient work only when asked for) + one 84-column GEMM
 * per chunk. */
size_t sunerf_mlp_input_grad_exact_workspace_bytes(int d_filter, int n_linear);
int sunerf_mlp_input_grad_exact(const float* const* weights_host, const float* const* biases_host, int n_linear, int d_filter,
                                int d_out, const float* rays_o, const float* rays_d, const float* times, const float* z_vals,
                                const float* points, int64_t n_rays, int n_samples, const float* g_raw, void* workspace,
                                size_t workspace_bytes, float* const* grad_weights_host, float* const* grad_biases_host,
                                int accumulate, float* grad_points, float* grad_rays_o, float* grad_rays_d, float* grad_times,
                                float* grad_z, void* stream);

/* ------------------------------------------------------------------------------------------------------------
 * Density / temperature head (run_density_temperature.py path).
 * Replaces DensityTemperatureRadiativeTransfer.raw2outputs / regularization, density_temperature.py:192-274, the base
 * offsets of NeRF_DT.forward, model.py:181-185, and the DT epilogues of base_tracing.py:99-110; the per-wavelength Python
 * loop with host syncs (density_temperature.py:245-256) is one launch.  The MLP runs in sunerf_emission_render_fwd
 * (its `raw` output is the input here; its emission outputs are ignored).
 *
 *   raw (N,S,2); wavelengths (N,W<=7) in Angstrom, <= 0 = channel absent; table_logt / table_resp (7,101) fp32 =
 *   LOGTE / TRESP x exposure time of aia_temp_resp.genx in channel order 94,131,171,193,211,304,335
 *   (density_temperature.py:131-146); log_abs (7) = log_absortpion parameters in that order; vol_c (1)
 *   image (N,W); weights (N,S) = relu(inf0)/(sum+1e-10); reg_q (N,S) = relu(inf0);
 *   height_map / absorption_map (N) and regularization (N,S) optional; reg_radius = 1.25 / Rs_per_ds
 *   backward: g_image (N,W), g_reg (N,S) or NULL -> g_raw (N,S,2) (feed sunerf_mlp_dgrad / sunerf_mlp_wgrad),
 *   g_log_abs (7), g_vol_c (1) (overwritten: cleared by the call, then summed with float atomics -- every ray adds its term
 *   to its workgroup's sum and every workgroup its sum to the output, so from three rays on the order of the adds is free and
 *   reruns agree to rounding, not by bits; g_raw and g_absmax do not depend on it), g_absmax as in
 *   sunerf_emission_integral_bwd; all three required; an empty batch (n_rays == 0) clears them and touches nothing else
 *   n_samples >= 3 (forward and backward; fewer: SUNERF_E_BADARG), at most 705 in the backward (its LDS: SUNERF_E_UNSUPPORTED)
 * ---------------------------------------------------------------------------------------------------------- */
int sunerf_dt_integral_fwd(const float* raw, const float* z_vals, const float* rays_o, const float* rays_d,
                           const float* wavelengths, int n_wavelengths, const float* table_logt, const float* table_resp,
                           const float* log_abs, const float* vol_c, float base_log_density, float base_log_temperature,
                           float pixel_intensity_factor, float reg_radius, int64_t n_rays, int n_samples, float* image,
                           float* weights, float* reg_q, float* height_map, float* absorption_map, float* regularization,
                           void* stream);

int sunerf_dt_integral_bwd(const float* raw, const float* z_vals, const float* rays_o, const float* rays_d,
                           const float* wavelengths, int n_wavelengths, const float* table_logt, const float* table_resp,
                           const float* log_abs, const float* vol_c, float base_log_density, float base_log_temperature,
                           float pixel_intensity_factor, float reg_radius, int64_t n_rays, int n_samples,
                           const float* g_image, const float* g_reg, float* g_raw, float* g_log_abs, float* g_vol_c,
                           void* g_absmax, void* stream);

/* sunerf_dt_integral_bwd for gradients w.r.t. all three outputs of raw2outputs (density_temperature.py:267-271), what
 * the reference's autograd gives a subclass that overrides a hook (its loss reaches `weights` through height_map and
 * `regularizing_quantity` through its own regularization, base_tracing.py:99-110):
 *   g_weights (N,S) or NULL : d loss / d weights,  weights = relu(inf0) / (sum_s relu(inf0) + 1e-10)
 *   g_reg_q (N,S) or NULL   : d loss / d reg_q,    reg_q = relu(inf0)
 * both added to g_raw[..., 0] where inf0 = raw0 + base_log_density > 0.  Everything else as sunerf_dt_integral_bwd
 * (which stays the entry point of the fused path: it has no such outputs). */
int sunerf_dt_integral_bwd_full(const float* raw, const float* z_vals, const float* rays_o, const float* rays_d,
                                const float* wavelengths, int n_wavelengths, const float* table_logt, const float* table_resp,
                                const float* log_abs, const float* vol_c, float base_log_density, float base_log_temperature,
                                float pixel_intensity_factor, float reg_radius, int64_t n_rays, int n_samples,
                                const float* g_image, const float* g_reg, const float* g_weights, const float* g_reg_q,
                                float* g_raw, float* g_log_abs, float* g_vol_c, void* g_absmax, void* stream);

/* ------------------------------------------------------------------------------------------------------------
 * Line-of-sight differential emission measure of the density / temperature model: the thermal structure
 * behind a pixel of sunerf_dt_integral_fwd.  Restates that kernel's forward, density_temperature.py:237-265, with the
 * temperature response folded out; the reference has no such product (a user bins per-sample profiles on the host).
 *
 *   raw (N,S,2), z_vals (N,S), base offsets: as sunerf_dt_integral_fwd.  rho = exp(relu(raw0 + base_log_density)),
 *   logT = relu(raw1 + base_log_temperature), both sums in fp32 (density_temperature.py:237-241)
 *   logt_nodes (K) fp32 device, strictly increasing (not checked), need not be uniform, 2 <= K <= 128
 *   log_abs (1) device or NULL: kappa = relu(log_abs[0]), the absorption scalar of ONE channel; NULL or <= 0: optically thin
 *   quadrature points j = 0..S-2 (the last sample is not one, exactly as in the render, :263-265):
 *     q_j = trapezoid weight of z_j on the grid z_0..z_{S-2}  (S = 2: a single point of weight 0, everything 0)
 *     t_j = exp(-A_{j+1}),  A = cumulative_trapezoid(rho kappa, z)                        :261-263 (the render's index shift)
 *     m_j = 1 if r_in <= |rays_o + rays_d z_j| <= r_out else 0 (a NaN radius: 0).  r_in <= 0 with r_out = +inf: no mask, and
 *           rays_o / rays_d may then be NULL
 *     v_j = q_j t_j m_j rho_j^2
 *   dem (N,K) or NULL: i = clamp(searchsorted(nodes, logT_j, right) - 1, 0, K-2), f = (logT_j - x_i) / (x_{i+1} - x_i),
 *     dem[i] += v_j (1 - f), dem[i+1] += v_j f for the samples with x_0 <= logT_j <= x_{K-1}; the others deposit nothing
 *     (Interp1D's extrap = 0, :245-256).  On the response table's grid:  image_w = vol_c pixel_intensity_factor sum_k dem_k R_w[k]
 *   em (N) = sum_j v_j over all samples, inside the node grid or not
 *   logt_mean (N) or NULL = sum_j v_j logT_j / em  (em = 0: NaN);  column (N) or NULL = sum_j q_j m_j rho_j, not attenuated
 *   fp32 sums in a fixed order without atomics: reruns, and a ray alone or inside a batch, give the same bits.  n_samples has
 *   no upper limit (nothing per sample lives in LDS).
 * Checked in this order, before anything is queued: n_rays < 0, n_samples < 2 or n_nodes < 2: SUNERF_E_BADARG;
 * n_nodes > 128: SUNERF_E_UNSUPPORTED; n_rays == 0: 0; a NULL raw / z_vals / logt_nodes / em, or NULL rays with a mask:
 * SUNERF_E_BADARG.
 * ---------------------------------------------------------------------------------------------------------- */
int sunerf_dem_integral(const float* raw, const float* z_vals, const float* rays_o, const float* rays_d,
                        const float* logt_nodes, int n_nodes, float base_log_density, float base_log_temperature,
                        const float* log_abs, float r_in, float r_out, int64_t n_rays, int n_samples, float* dem, float* em,
                        float* logt_mean, float* column, void* stream);

/* ------------------------------------------------------------------------------------------------------------
 * White-light Thomson scattering (total / polarised brightness, Howard & Tappin 2009).
 * Replaces ThompsonScattering.raw2outputs, sunerf/rendering/thompson.py:17-109, with the reference's defects resolved
 * (DESIGN.md 8b): the radius runs over (x, y, z) only (:43, :53 take the time coordinate in), the geometry is fp64 (the
 * fp32 expressions of :59-66 lose 8 % at 215 solar radii), and the outputs are those of the table below.
 *
 *   raw (N,S,C), C in {1, 2}: channel 0 is the log density, rho = exp(kappa raw0) (kappa = ln 10 for a NeRF, :39,
 *   1 for a field answering ln rho); z_vals (N,S); rays_o / rays_d (N,3);
 *   solar_radius, limb_darkening_coeff, c0: (1) device scalars, the module's buffers (:11-15), read in the kernel
 *   pixel_b (N,2) = C_0 (sum rho |I_tot| ds, sum rho |I_P| ds)      (:82-90, eqs. 23, 24, 29)
 *   pixel_density (N) = sum rho ds;  distance_from_sun / _obs (N) = sum rho r / (M + 1e-10), sum rho z |d| / (M + 1e-10);
 *   weights (N,S) = rho / (M + 1e-10), M = sum rho                   (:94-101)
 *   ds_j = (z_j - z_{j-1}) |d|, ds_0 = ds_1 (:25-31); for S = 1 there is no ds and pixel_b = pixel_density = 0.
 *   On the limb and on degenerate rays (both entry points; tests/test_gpu_thomson_seams.py):
 *     |x_j| == solar_radius by bits, or less: the sample is inside the Sun, I_tot = I_P = 0 for it (and no gradient through
 *     pixel_b); it still counts in pixel_density, the two distances and weights.  |x_j| > solar_radius by any amount: the
 *     limb values (I_P -> u / 4 sin^2 chi, I_tot -> 2 ((1 - u) 4/3 + u 3/4) - I_P).  A sample at the origin is inside.
 *     rays_d = (0, 0, 0): sin^2 chi = 0 / 0, every intensity and every ds is 0: pixel_b = pixel_density = distance_from_obs
 *     = 0, distance_from_sun = |rays_o| (M > 0), weights as ever.  rays_o x rays_d = 0 (a ray through the centre): pB = 0.
 *     z_j == z_{j-1}: ds_j = 0, the sample adds nothing to pixel_b / pixel_density.
 *   backward: any subset of g_pixel_b (N,2), g_pixel_density, g_distance_from_sun, g_distance_from_obs (N),
 *   g_weights (N,S) (NULL = absent) -> g_raw (N,S,C) (channel 1 written 0); g_absmax (4 bytes, may be NULL) receives
 *   the bit pattern of max |g_raw|, as in sunerf_emission_integral_bwd (the scale sunerf_mlp_dgrad takes); given, it is
 *   cleared by every call, an empty batch (n_rays == 0) included.
 *   n_samples >= 1; no float atomics: reruns are bit-identical.
 * ---------------------------------------------------------------------------------------------------------- */
int sunerf_thomson_integral_fwd(const float* raw, int n_channels, float kappa, const float* z_vals, const float* rays_o,
                                const float* rays_d, const float* solar_radius, const float* limb_darkening_coeff,
                                const float* c0, int64_t n_rays, int n_samples, float* pixel_b, float* pixel_density,
                                float* distance_from_sun, float* distance_from_obs, float* weights, void* stream);

int sunerf_thomson_integral_bwd(const float* raw, int n_channels, float kappa, const float* z_vals, const float* rays_o,
                                const float* rays_d, const float* solar_radius, const float* limb_darkening_coeff,
                                const float* c0, int64_t n_rays, int n_samples, const float* g_pixel_b,
                                const float* g_pixel_density, const float* g_distance_from_sun,
                                const float* g_distance_from_obs, const float* g_weights, float* g_raw, void* g_absmax,
                                void* stream);

/* ------------------------------------------------------------------------------------------------------------
 * Input side of the path: observer rays on the device.
 * Replaces get_rays, sunerf/data/ray_sampling.py:7-36, and the host-side tiling / H2D copy of the rays and of the
 * time column in SuNeRFLoader.render_observer_image, sunerf/evaluation/loader.py:73-92 and :186-214.
 *   tx, ty   : helioprojective angles [rad], fp64, device.  per_pixel = 0: tx[width] (columns) and ty[rows] (axes of a
 *              regular grid; pixel p = row * width + column);  per_pixel != 0: tx[p], ty[p] for every pixel of the frame
 *              (e.g. sunpy's all_coordinates_from_map for a real WCS)
 *   pixels [pix_begin, pix_begin + n_pix) of the frame are produced (one tile)
 *   c2w_host : HOST pointer, 12 floats = rows of pose_spherical(...)[:3, :4] (train/coordinate_transformation.py:36-54)
 *   rays_o, rays_d : [n_pix, 3] out;  times : [n_pix] out, filled with time_value (may be NULL)
 * ---------------------------------------------------------------------------------------------------------- */
int sunerf_observer_rays(const double* tx, const double* ty, int per_pixel, int width, int64_t pix_begin, int64_t n_pix,
                         const float* c2w_host, float time_value, float* rays_o, float* rays_d, float* times,
                         void* stream);

/* ------------------------------------------------------------------------------------------------------------
 * Training sets from observation images: replaces the host assembly of the reference's data modules
 * (sunerf/data/loader/single_channel.py:44-52, multi_thermal_loader.py:54-61, 209-258) -- per-pixel rays, time broadcast,
 * flatten, one permutation over all rays -- by one launch that writes a rank's shard of the shuffled pool.
 *
 * A training set is a list of views.  View k holds height x width pixels (AFTER its downscale), numbered row-major from
 * pix_offset (views concatenated in table order: pix_offset[0] = 0, pix_offset[k+1] = pix_offset[k] + height * width),
 * n_pixels in all.  Record `slot` of the pool is pixel  p = valid_index ? valid_index[pi(slot)] : pi(slot), where pi is a
 * bijection of [0, n_valid) keyed by (seed, epoch) (permute == 0: the identity): cycle-walking over a 4-round balanced Feistel
 * network on 2 b bits, b = ceil(bit_length(n_valid - 1) / 2), round function fmix32(R + k_r) & (2^b - 1) (murmur3 finaliser),
 *   k_r = fmix32((s + 0x9e3779b9 (r + 1)) ^ fmix32(e + 0x85ebca6b (r + 1))),  s / e = lo ^ fmix32(hi + 0x9e3779b9) of the 64-bit seed / epoch,
 * all in uint32 arithmetic (restated in numpy by tests/observations_reference.py).  No table of size n_valid, no atomics:
 * two builds with one key are bit-identical, and the shards of one key are disjoint and complete by construction.
 * ---------------------------------------------------------------------------------------------------------- */
#define SUNERF_OBS_MAX_CHANNELS 16

typedef struct SunerfViewDesc {
  int64_t pix_offset;        /* number of the view's first pixel                                                       */
  const double* tx;          /* DEVICE: column angles [width] (per_pixel == 0) or per-pixel angles [height * width]    */
  const double* ty;          /* DEVICE: row angles [height] or per-pixel angles, of the grid AFTER the downscale       */
  const float* image;        /* DEVICE: [n_planes, height * downscale, width * downscale], the present channels only   */
  int32_t height, width;     /* pixels of the view after the downscale                                                 */
  int32_t downscale;         /* f >= 1: a pixel is the mean of an f x f source block (fp64 sum, row-major, fp32 once)  */
  int32_t per_pixel;
  float c2w[12];             /* rows of pose_spherical(...)[:3, :4]                                                    */
  float time;                /* normalised observation time                                                            */
  int32_t n_planes;
  int32_t plane[SUNERF_OBS_MAX_CHANNELS];      /* per output channel: its plane of `image`, or -1 (absent: target 0, wavelength 0) */
  float wavelength[SUNERF_OBS_MAX_CHANNELS];   /* per output channel: the value written for a present channel                */
} SunerfViewDesc;

/*   views : DEVICE table of n_views descriptors (size of one: the function below; the caller keeps every pointer in it valid)
 *   valid_index : DEVICE [n_valid] ascending pixel numbers, or NULL when no pixel was dropped (then n_valid == n_pixels)
 *   records [slot_begin, slot_begin + n_slots) of the permuted set are written to the FIRST n_slots rows of
 *   rays [n_slots, 2, 3] (origin, direction: the bits of sunerf_observer_rays for that pixel), time [n_slots, 1],
 *   target_image [n_slots, n_channels], wavelength [n_slots, n_channels] (the last two may be NULL); outputs 16-byte aligned.
 *   n_valid < 1 or >= 2^40, n_channels outside [1, SUNERF_OBS_MAX_CHANNELS], negative counts, slots outside [0, n_valid), null
 *   or misaligned pointers give SUNERF_E_BADARG; n_slots == 0 does nothing. */
size_t sunerf_view_desc_bytes(void);
int sunerf_build_ray_pool(const SunerfViewDesc* views, int n_views, int64_t n_pixels, const int64_t* valid_index,
                          int64_t n_valid, int n_channels, int permute, uint64_t seed, uint64_t epoch, int64_t slot_begin,
                          int64_t n_slots, float* rays, float* time, float* target_image, float* wavelength, void* stream);

/* ------------------------------------------------------------------------------------------------------------
 * Reprojection baseline: all emission is taken to come from the sphere r = radius (1 R_sun in scene units).
 * Replaces sunerf/baseline/reprojection.py: create_heliographic_map :52-95 (reproject_and_coadd of the views with
 * reproject_interp, default mean, match_background=False, then nan_to_num(array, nan=nanmean(array))), transform :98-125 and
 * load_views :128-168 (h_map.reproject_to(observer) for one observer / a grid of them through a multiprocessing.Pool).
 * Geometry is this project's pinhole convention (the pixel direction of ray_math.h), all of it in fp64; c2w is promoted.
 *
 * Conventions.  Map pixel (i, j) lies at p = radius * u(lat[i], lon[j]), u = (-cos b sin l, cos b cos l, -sin b); lat / lon are
 * ascending fp64 axes of pixel centres [rad].  A pixel with angles (Tx, Ty) of a view looks along
 * c2w[:3,:3] (sin Tx, -sin Ty cos Tx, -cos Tx cos Ty); a camera-frame vector (x, y, z) = c2w[:3,:3]^-1 (p - o), o = c2w[:, 3],
 * has Tx = atan2(x, hypot(y, z)), Ty = atan2(-y, -z) (the inverse by cofactors in fp64, not the transpose: the fp32 pose is
 * orthonormal to 1e-7 only, and a pixel's own surface point must come back to the pixel).  The fractional pixel coordinate of an angle on an axis: binary search
 * for the interval, linear interpolation inside it (linear extrapolation of the end intervals outside the axis); ascending or
 * descending, uniform or not; an axis of one pixel covers its own angle only (any other angle: NaN).
 * Bilinear sample of an n_y x n_x plane at (y, x): NaN outside [0, n_y - 1] x [0, n_x - 1]; inside i0 = floor, i1 = min(i0 + 1,
 * n - 1) and the four-term weighted sum in fp64 of the fp32 taps -- scipy.ndimage.map_coordinates(order=1, mode='constant',
 * cval=nan).  With downscale f > 1 a tap is the block mean the pool kernel forms (fp64 sum, row-major, / f^2, fp32 once).
 *
 * sunerf_synchronic_map: rows [row_begin, row_begin + n_rows) of the n_lat x n_lon map from n_views views.  A per_pixel view
 *   has no closed inverse: the table is on the device, so the entry point cannot see it -- the binding refuses such views with
 *   an error and the kernel lets one cover nothing.  View v covers channel c of a pixel iff p . o - radius^2 > 0 (p is the near
 *   intersection of its own line of sight), the view has the channel, and the sample is not NaN.
 *     map [n_channels][n_rows][n_lon] fp32 = fp64 sum of the covering samples in view order / their number, NaN where none
 *     footprint [n_channels][n_rows][n_lon] int32 = number of covering views
 *     coords (NULL, or n_views == 1) [3][n_rows][n_lon] fp64 = x, y on the view's axes and p . o - radius^2
 * sunerf_map_fill: nan_to_num(map, nan=nanmean(map)) per channel of map [n_channels][n_pixels].  mode 0: only the statistics;
 *   1: NaNs become the channel's mean; 2: NaNs become `value`.  stats [n_channels][2] fp64 (device) = mean of the non-NaN
 *   pixels (NaN if there are none), their number.  Two launches, per-workgroup fp64 partial sums in `workspace`
 *   (the size the workspace function returns, 8-byte aligned) added in a fixed order: no atomics, bit-identical reruns.
 * sunerf_reproject_views: the map seen by n_observers observers, pixel p of observer k = row * width + col numbered from
 *   pix_offset (observers concatenated as views are).  Per pixel: unit direction d as above, c = o x d, on the disk iff
 *   m = radius^2 - |c|^2 > 0 and o . d < 0, near point p = o + d (-(o . d) - sqrt(m)), lat = atan2(-p_z, hypot(p_x, p_y)),
 *   lon = atan2(-p_x, p_y) brought into [lon[0], lon[0] + 2 pi), bilinear sample of every channel of map [n_channels][n_lat][n_lon].
 *     out [n_pixels][n_channels] fp32 (16-byte aligned): NaN outside the map's axes; off the disk `off_disk` (pass NaN for
 *     the reference's behaviour);  coords (may be NULL) [3][n_pixels] fp64 = x (longitude axis), y (latitude axis), m / radius^2
 * Null pointers, non-positive shapes, n_channels outside [1, SUNERF_OBS_MAX_CHANNELS], rows outside the map, radius that is
 * not > 0 and finite, coords with n_views != 1, a mode outside 0..2 give SUNERF_E_BADARG; a small workspace SUNERF_E_WORKSPACE.
 * Monotone axes are the caller's responsibility.
 * ---------------------------------------------------------------------------------------------------------- */
typedef struct SunerfObserverDesc {
  int64_t pix_offset;        /* number of the observer's first pixel                                                   */
  const double* tx;          /* DEVICE: column angles [width]                                                          */
  const double* ty;          /* DEVICE: row angles [height]                                                            */
  int32_t height, width;
  float c2w[12];             /* rows of pose_spherical(...)[:3, :4]                                                    */
} SunerfObserverDesc;

size_t sunerf_observer_desc_bytes(void);
int sunerf_synchronic_map(const SunerfViewDesc* views, int n_views, int n_channels, const double* lat, int n_lat,
                          const double* lon, int n_lon, int row_begin, int n_rows, double radius, float* map, int32_t* footprint,
                          double* coords, void* stream);
size_t sunerf_map_fill_workspace_bytes(int n_channels);
int sunerf_map_fill(float* map, int n_channels, int64_t n_pixels, int mode, double value, double* stats, void* workspace,
                    size_t workspace_bytes, void* stream);
int sunerf_reproject_views(const float* map, int n_channels, const double* lat, int n_lat, const double* lon, int n_lon,
                           double radius, const SunerfObserverDesc* observers, int n_observers, int64_t n_pixels,
                           float off_disk, float* out, double* coords, void* stream);

/* ------------------------------------------------------------------------------------------------------------
 * Heliographic analyses: radial columns from the solar centre, one per (latitude, longitude).
 * Replaces the host-side point generation of the reference's stash scripts, sunerf/evaluation/stash/
 * topographical_map.py:36-49, topographical_profile.py:33-45, topographical_slice.py:119-130, eruption_profile.py:76-88.
 *   lat, lon : [rad], fp64, device, in the convention of render_observer_image (loader.py:63-108).  per_column = 0:
 *              lat[n_lat] (rows, south first) and lon[n_lon] (columns) are the axes of a regular grid, column
 *              p = row * n_lon + col;  per_column != 0: lat[p], lon[p] for every column (arcs, point lists)
 *   columns [col_begin, col_begin + n_cols) are produced (one tile)
 *   rays_o [n_cols, 3] out (zeros);  rays_d [n_cols, 3] out = fp32(u), u = (-cos lat sin lon, cos lat cos lon, -sin lat)
 *              evaluated in fp64 (the normalised position of pose_spherical(-lon, lat, d));  times [n_cols] out, filled
 *              with time_value (may be NULL)
 * ---------------------------------------------------------------------------------------------------------- */
int sunerf_column_rays(const double* lat, const double* lon, int per_column, int n_lon, int64_t col_begin, int64_t n_cols,
                       float time_value, float* rays_o, float* rays_d, float* times, void* stream);

/* Column statistics of a fused emission pass over columns of sunerf_column_rays (one wave64 per column, fp32 sums):
 *   raw [N,S,2] (sunerf_emission_render_fwd's raw), z_row [S] (the z shared by every column), rays_d [N,3]
 *   e_j  = exp(raw_j0),  dr_j = (z_j - z_{j-1}) |rays_d| with the first interval duplicated (the integral's own dists,
 *          emission.py:19-26),  r_j = z_j |rays_d| (the sample's distance from the centre)
 *   emission_height [N] = height_scale * sum r_j e_j / sum e_j            topographical_profile.py:57
 *   emission_column [N] = sum e_j dr_j  (optically thin column)          topographical_slice.py:131-140 (there without dr)
 *   emission [N,S] = e_j, absorption [N,S] = 1 - exp(-relu(raw_j1) dr_j) eruption_profile.py:89-94 (both NULL or both set)
 *   n_samples >= 2 (SUNERF_E_BADARG otherwise: dr needs an interval)
 * ---------------------------------------------------------------------------------------------------------- */
int sunerf_column_stats(const float* raw, const float* z_row, const float* rays_d, int64_t n_cols, int n_samples,
                        float height_scale, float* emission_height, float* emission_column, float* emission,
                        float* absorption, void* stream);

/* ------------------------------------------------------------------------------------------------------------
 * 3-D volumes of the field: query points of a grid, physical quantities of the model's answer and a
 * weighted 3-D score.  The MLP between the first two is sunerf_mlp_points_fwd (or a field kernel), unchanged.
 *
 * sunerf_grid_points replaces the host-side cube of the reference's sunerf/evaluation/stash/voxel_volume.py:30-44
 * (np.meshgrid of three linspaces + a time column, pushed to the device batch by batch) and the point arrays its
 * callers hand to load_coords (evaluation/loader.py:119-134).  Voxels [first, first + count) of a grid of n0 x n1 x n2
 * nodes, voxel index C-order (last axis fastest):
 *   points [count, 4] out, fp32, 16-byte aligned = (x, y, z, time_value) in model units;  radius [count] out, fp32 [solar radii]
 *   SUNERF_GRID_AFFINE:    a0[n0], a1[n1], a2[n2] fp64 device axes [solar radii];
 *       X = origin + a0[i] e0 + a1[j] e1 + a2[k] e2, per component, left to right, in fp64 (e_m = frame.basis[m]);
 *       point = fp32(X / Rs_per_ds), radius = fp32(sqrt((X_x^2 + X_y^2) + X_z^2)).  A plane is n2 = 1.
 *   SUNERF_GRID_SPHERICAL: a0 = [cos lat | sin lat] (2 n0 values), a1 = [cos lon | sin lon] (2 n1), a2 = r[n2] [solar radii],
 *       fp64, the trig values taken on the host;  X = r_k u, u = (-cos b sin l, cos b cos l, -sin b) (sunerf_column_rays' u);
 *       point = fp32(X / Rs_per_ds), radius = fp32(r_k).  `frame` is not read.
 * The library is compiled without floating-point contraction, so a host evaluation of the same fp64 expressions gives
 * the same bits.
 * ---------------------------------------------------------------------------------------------------------- */
#define SUNERF_GRID_AFFINE    0
#define SUNERF_GRID_SPHERICAL 1
typedef struct SunerfGridFrame {
  double origin[3];
  double basis[3][3];      /* basis[m] = e_m */
} SunerfGridFrame;
int sunerf_grid_points(int kind, const double* a0, const double* a1, const double* a2, int n0, int n1, int n2,
                       SunerfGridFrame frame, double Rs_per_ds, float time_value, int64_t first, int64_t count,
                       float* points, float* radius, void* stream);

/* sunerf_field_quantities: the physical fields of a model's answer, one element-wise launch.
 *   inferences [M, C] fp32 (C = 2 except white light: C >= 1), radius [M] fp32 (sunerf_grid_points'), outputs fp32:
 *   SUNERF_FIELD_EMISSION   : out0 = emission = exp(raw0)                                voxel_volume.py:47
 *                             out1 = absorption = relu(raw1), the coefficient kappa     rendering/emission.py:31-37
 *   SUNERF_FIELD_DT         : out0 = density = exp(relu(inf0)), out1 = log_temperature = relu(inf1), inf with the base
 *                             offsets as NeRF_DT.forward returns it                     density_temperature.py:237-241
 *                             emissivity [M, W] = density^2 R_w(log_temperature)         :245-256, :263
 *                             absorption_w [M, W] = density relu(log_abs[channel w])     :260-261
 *                             R_w: the response interpolation of sunerf_dt_integral_fwd (the same device function);
 *                             wavelengths [W] device, W <= 7; a channel that is not one of the seven gives 0.
 *                             emissivity / absorption_w may be NULL (then wavelengths and tables are not read).
 *   SUNERF_FIELD_WHITE_LIGHT: out0 = electron_density = exp(kappa raw0), kappa as sunerf_thomson_integral_fwd   thompson.py:39
 *   out0 / out1 may be NULL.  A voxel whose radius is not inside [r_in, r_out] (a NaN radius included) gets `fill` in
 *   every output; r_out = +inf: no outer mask.  exp overflows to +inf as the reference's fp32 does.
 * ---------------------------------------------------------------------------------------------------------- */
#define SUNERF_FIELD_EMISSION    0
#define SUNERF_FIELD_DT          1
#define SUNERF_FIELD_WHITE_LIGHT 2
int sunerf_field_quantities(int mode, const float* inferences, int n_channels, const float* radius, int64_t n_points,
                            float r_in, float r_out, float fill, float kappa, const float* wavelengths, int n_wavelengths,
                            const float* table_logt, const float* table_resp, const float* log_abs, float* out0, float* out1,
                            float* emissivity, float* absorption_w, void* stream);

/* sunerf_volume_metrics: weighted, masked comparison of two scalar volumes a, b [n0][n1][n2] (fp32), in fp64.  Nothing
 * in the reference scores a volume; its 2-D scores are sunerf_image_metrics'.
 *   weight of voxel (i, j, k) = (w0[i] w1[j]) w2[k], fp64 device vectors;  a voxel where a or b is not finite is left out
 *   out [11] fp64 device = sum w, sum w a, sum w b, sum w d, sum w |d|, sum w d^2, sum w a^2, sum w b^2, sum w a b,
 *                          max |d|, number of voxels counted (exact below 2^53);  d = a - b
 *   Per-workgroup partial sums go to `workspace` (sunerf_volume_metrics_workspace_bytes, 8-byte aligned) and a second
 *   launch adds them in a fixed order: no atomics, reruns are bit-identical; the grid depends on the voxel count only.
 * ---------------------------------------------------------------------------------------------------------- */
#define SUNERF_VOLUME_METRICS_N 11
size_t sunerf_volume_metrics_workspace_bytes(int64_t n_voxels);
int sunerf_volume_metrics(const float* a, const float* b, int n0, int n1, int n2, const double* w0, const double* w1,
                          const double* w2, double* out, void* workspace, size_t workspace_bytes, void* stream);

/* ------------------------------------------------------------------------------------------------------------
 * Per-pixel DEM inversion: channel images -> DEM(log T) per pixel.  Nothing in the reference inverts; the
 * result is comparable, key for key, with sunerf_dem_integral's -- the line-of-sight DEM of the model behind
 * density_temperature.py:237-265 -- and, folded with the response, with that render's image.
 *
 * For every pixel i, with y [N][M] the channel values, sigma [N][M] > 0 their errors (fp32), response [M][K] >= 0 the
 * channels' response on the K log T nodes times the render's constant, prior [K] > 0 a scale per node (fp64) and lam > 0:
 *   x* = argmin over x >= 0 of  1/2 sum_w ((response x - y)_w / sigma_w)^2 + lam/2 sum_k (x_k / prior_k)^2
 * (strictly convex: unique; what scipy.optimize.nnls returns for the stacked system), by semismooth Newton on the dual in
 * fp64, one lane per pixel: stops at max |F| <= tol max |y / sigma| or after max_iter Newton steps.
 *   A channel whose y is not finite, or whose sigma is not finite or <= 0, is left out for that pixel.
 *   discrepancy == 0: lam [N] (lam_per_pixel != 0) or [1] fp32 device, each > 0 and finite.
 *   discrepancy != 0: lam is not read; per pixel log10 lam is bisected n_bisect times on [lam_min, lam_max] for
 *     chi2(lam) = sum_w ((response x* - y)_w / sigma_w)^2 = chi2_target (< 0: the number of channels the pixel uses); each
 *     solve starts from the previous one; the solve at the middle of the last bracket is returned.  chi2(lam_min) > target
 *     returns the solve at lam_min and sets status bit 4, chi2(lam_max) < target the solve at lam_max and bit 8.  Every lam
 *     of a solve is an fp32 number (lam_min and lam_max are rounded first): lam_out is the lam of the returned x*.
 *   dem [N][K] = x*, em [N] = sum_k x*_k, logt_mean [N] = sum_k x*_k logt_nodes[k] / em (NaN where em = 0), chi2 [N],
 *   lam_out [N] (fp32; the sums in fp64); each may be NULL.  status [N] int32, required: bit 0 a solve stopped before it
 *   met tol (max_iter, or 30 line-search trials of one step), 2 no channel left (dem = em = 0, logt_mean = lam_out = NaN), 4 / 8 the
 *   bracket ends, 16 a lam that is not > 0 and finite (outputs as for 2); bits 8.. the Newton steps of all solves.
 * No atomics; a pixel's outputs depend on its own inputs only: reruns, batches and tilings give the same bits.
 * Sizes are checked first (n_nodes < 2, n_channels < 1, n_bisect < 0, max_iter < 1, n_pixels < 0: -1; n_nodes > 128,
 * n_channels > 8, n_bisect > 60 or max_iter > 4096: -2), then the empty batch (0), then values and null pointers (tol < 0,
 * in discrepancy mode a [lam_min, lam_max] that is not 0 < lam_min <= lam_max < inf, a NULL input or status: -1).
 * ---------------------------------------------------------------------------------------------------------- */
int sunerf_dem_invert(const float* y, const float* sigma, const double* response, const double* prior,
                      const float* logt_nodes, const float* lam, int lam_per_pixel, int discrepancy, double chi2_target,
                      double lam_min, double lam_max, int n_bisect, double tol, int max_iter, int64_t n_pixels,
                      int n_channels, int n_nodes, float* dem, float* em, float* logt_mean, float* chi2, float* lam_out,
                      int* status, void* stream);

/* ------------------------------------------------------------------------------------------------------------
 * Voxel-grid field: values [n0][n1][n2][C] fp32 on the nodes of a grid (C order over the grid's axes,
 * the layout of sample_volume's `inferences`), 1 <= C <= 4, gathered trilinearly and fitted through the adjoint.
 * Generalises the interpolators of MHDModel, sunerf/model/mhd_model.py:45-75 (RegularGridInterpolator(method='linear',
 * bounds_error=False, fill_value=...)), to the grids of the volumes -- the cube of
 * sunerf/evaluation/stash/voxel_volume.py:30-44 included -- and adds the gradient w.r.t. the values.
 *
 * One sample at the point p [model units, fp32]; X = p * Rs_per_ds [solar radii] and everything up to the weights in fp64:
 *   SUNERF_GRID_AFFINE   : u = inverse (X - origin), u_m = (inverse[m][0] dx + inverse[m][1] dy) + inverse[m][2] dz;
 *                          `inverse` is the inverse of the node map X = origin + u_0 e_0 + u_1 e_1 + u_2 e_2
 *   SUNERF_GRID_SPHERICAL: the inverse of sunerf_grid_points' X = r (-cos b sin l, cos b cos l, -sin b):
 *                          r = sqrt((X^2 + Y^2) + Z^2), u = (lat, lon, r) = (asin(clamp(-Z / r)), atan2(-X, Y), r), the
 *                          longitude then reduced into [lon[0], lon[0] + 2 pi)
 *   cell per axis : i = searchsorted(axis, u, 'left') - 1 clipped to [0, n - 2] (axes strictly increasing, n >= 2),
 *                   t = (u - axis[i]) / (axis[i + 1] - axis[i]); the weights (float)(1 - t), (float)t; interpolation in fp32
 *   inside        : lo[k] <= u_k <= hi[k] (the axis ends) on every axis that is not a periodic longitude.  Outside, or with
 *                   a NaN coordinate (missed rays of SphericalSampler): raw = fill[c], no gradient
 *   lon_mode      : SUNERF_GRID_LON_PATCH  a limited span: outside it the fill
 *                   SUNERF_GRID_LON_CLOSED periodic, the axis spans 2 pi and its last node repeats the first
 *                   SUNERF_GRID_LON_OPEN   periodic, endpoint left out: one more cell joins the last node to the first + 2 pi
 *
 * sunerf_grid_field_fwd: ray mode (points == NULL): the samples o + d z (multiply, then add, in fp32) of rays_o / rays_d
 *   [N,3], z_vals [N,S] -> raw [N,S,C]; points mode: points [M, point_stride] (stride 3 or 4; a time column is ignored: the
 *   field is static), n_rays = M, n_samples = 1 -> raw [M,C].  cells [N S] int32 and weights [N S][3][2] fp32 (both or
 *   neither): the flattened cell id of every sample (outside: the number of cells) and its weights, for the backward.
 * sunerf_grid_field_bwd: g_values[node][c] (+)= sum over samples of w(sample, node) g_raw[sample][c], the adjoint.
 *   perm [n_total] int64: a stable ascending sort of `cells`; seg_start [number of cells + 1] int64: the first sorted
 *   position of every cell id (searchsorted of the sorted ids).  No floating-point atomics: per node the segments of its
 *   adjacent cells are added in a fixed order, segments longer than 64 samples through per-wave partial sums in `workspace`
 *   (sunerf_grid_field_bwd_workspace_bytes): reruns are bit-identical.  accumulate != 0 adds onto g_values.  g_values
 *   [n0][n1][n2][C] fp32; g_raw [n_total][C].  n_total == 0: g_values is zeroed (accumulate == 0) or left alone, and no other
 *   pointer is read.
 * Sizes and the descriptor are checked first (n[k] < 2, C < 1, a bad kind / lon_mode, Rs_per_ds <= 0: -1; C > 4 or 2^31
 * cells: -2), then the empty batch (0), then null pointers (-1) and the workspace (-3).  `grid` is a HOST pointer; its
 * axis pointers are device arrays (fp64).
 * ---------------------------------------------------------------------------------------------------------- */
#define SUNERF_GRID_FIELD_MAX_CHANNELS 4
#define SUNERF_GRID_LON_PATCH  0
#define SUNERF_GRID_LON_CLOSED 1
#define SUNERF_GRID_LON_OPEN   2
typedef struct SunerfGridFieldDesc {
  const double* axis[3];    /* device, strictly increasing, n[k] nodes */
  int n[3];
  int n_channels;
  int kind;                 /* SUNERF_GRID_AFFINE / SUNERF_GRID_SPHERICAL */
  int lon_mode;             /* SUNERF_GRID_LON_*; PATCH for an affine grid */
  double lo[3];             /* axis[k][0] */
  double hi[3];             /* axis[k][n[k] - 1] */
  double inverse[3][3];     /* affine grids */
  double origin[3];
  double Rs_per_ds;
  float fill[4];
} SunerfGridFieldDesc;
size_t sunerf_grid_field_desc_bytes(void);
int sunerf_grid_field_fwd(const SunerfGridFieldDesc* grid, const float* values, const float* rays_o, const float* rays_d,
                          const float* z_vals, int64_t n_rays, int n_samples, const float* points, int point_stride,
                          float* raw, int* cells, float* weights, void* stream);
size_t sunerf_grid_field_bwd_workspace_bytes(int64_t n_total, int n_channels);
int sunerf_grid_field_bwd(const SunerfGridFieldDesc* grid, const float* g_raw, const int* cells, const float* weights,
                          const int64_t* perm, const int64_t* seg_start, int64_t n_total, void* workspace,
                          size_t workspace_bytes, float* g_values, int accumulate, void* stream);

/* ------------------------------------------------------------------------------------------------------------
 * Output side of the path: training loss and optimiser step without host synchronisation.
 *
 * sunerf_training_loss replaces EmissionSuNeRFModule.training_step's loss section, sunerf/model/sunerf.py:105-125
 * (finite asserts :105-107, ImageAsinhScaling sunerf/train/scaling.py:17-28, 2 x nn.MSELoss, regularization.mean(),
 * psnr) and, with scaling = 0, DensityTemperatureSuNeRFModule.training_step sunerf.py:185-200 (plain MSE).
 *   coarse_image / fine_image / target_image : n = N * W floats each;  regularization : n_reg floats (may be 0)
 *   finite_check_host[n_finite_check <= 8]   : HOST arrays of further device tensors (+ sizes) that only take part in
 *                                              the NaN / Inf count (z_vals, height_map, ...: sunerf.py:105-107)
 *   scaling 1 = asinh(x / vmax / a) / asinh(1 / a) applied to all three images; 0 = none
 *   g_coarse / g_fine : d loss / d coarse_image, d loss / d fine_image (n floats each); d loss / d regularization is
 *                       the constant lambda_regularization / n_reg
 *   stats (8 floats, device): loss, coarse MSE, fine MSE, regularization mean, psnr, number of non-finite values, 0, 0
 *   workspace: sunerf_train_workspace_bytes() bytes, ZERO-INITIALISED once by the caller (the kernels leave it zeroed);
 *              one workspace serves one stream
 *
 * sunerf_clip_adam_step replaces torch.nn.utils.clip_grad_norm_(params, max_norm) (Lightning gradient_clip_val,
 * run_emission.py:72) followed by torch.optim.Adam.step() (sunerf.py:31) on ONE flat fp32 buffer:
 *   g = grads * grad_scale (1 / world size after a sum all-reduce); total = ||g||_2; g *= min(1, max_norm / (total + 1e-6));
 *   m += (1 - beta1)(g - m); v = beta2 v + (1 - beta2) g g; p -= lr / (1 - beta1^step) * m / (sqrt(v) / sqrt(1 - beta2^step) + eps)
 *   max_norm <= 0 disables clipping; step counts from 1.
 *   skip_if_positive: optional device float -- the number of non-finite outputs of this step summed over ALL ranks (the
 *     caller carries it as one extra element at the tail of the all-reduced gradient bucket); a value > 0
 *     leaves params and moments untouched, and so does a non-finite gradient norm: every rank takes the same decision
 *     because both inputs are results of the all-reduce (the reference asserts instead, sunerf.py:105-107).
 *   norm_out (4 floats, device): total norm, clip coefficient, skipped (0 / 1), 0.  grads holds the scaled, clipped
 *     gradient afterwards.  norm_out / workspace may be NULL only with max_norm <= 0 and step_counter == NULL (then there
 *     is no norm pass and only skip_if_positive can skip).
 *   step_counter: optional device int64 -- number of APPLIED updates.  When given it is authoritative (`step` is ignored):
 *     the update uses *step_counter + 1 for the bias corrections and advances the counter only if it is not skipped.
 * ---------------------------------------------------------------------------------------------------------- */
size_t sunerf_train_workspace_bytes(void);
int sunerf_training_loss(const float* coarse_image, const float* fine_image, const float* target_image, int64_t n,
                         const float* regularization, int64_t n_reg, const float* const* finite_check_host,
                         const int64_t* finite_check_sizes_host, int n_finite_check, int scaling, float vmax, float a,
                         float lambda_image, float lambda_regularization, float* g_coarse, float* g_fine, float* stats,
                         void* workspace, size_t workspace_bytes, void* stream);
int sunerf_clip_adam_step(float* params, float* grads, float* exp_avg, float* exp_avg_sq, int64_t n, double lr,
                          double beta1, double beta2, double eps, float max_norm, float grad_scale, int64_t step,
                          const float* skip_if_positive, float* norm_out, void* workspace, size_t workspace_bytes,
                          void* step_counter, void* stream);

/* ------------------------------------------------------------------------------------------------------------
 * Image scores: replaces the host-side scoring of the reference's TestImageCallback,
 * sunerf/train/callback.py:46-56 and :84-86 (skimage SSIM, MSE, PSNR), and of its evaluation scripts,
 * sunerf/evaluation/stash/metrics_simulation.py:41-54 and baseline_simulation.py:30-42 (SSIM, MAE, ME).
 *   pred, target : [n_images][height][width] fp32, each image contiguous;  all arithmetic fp64
 *   out [n_images][4] (fp64, device) = ssim, mse, mae, me per image:
 *     ssim = skimage.metrics.structural_similarity(target, pred, data_range) with its defaults (7 x 7 uniform window,
 *            sample covariance 49 / 48, scipy 'reflect' boundary, C1 = (0.01 R)^2, C2 = (0.03 R)^2, mean of the SSIM map
 *            over [3, height - 3) x [3, width - 3));
 *     mse, mae, me = means of d^2, |d| and d over all pixels, d = pred - target.
 *   A NaN pixel makes all four outputs of its image NaN and no other.  Two launches, no atomics: bit-identical reruns, and
 *   an image's scores do not depend on the batch it is scored in.
 *   workspace : the size the workspace function returns (fp64 partial sums of every tile), 8-byte aligned.
 *   n_images == 0 does nothing; height or width < 7 (skimage: win_size exceeds image extent), a data_range that is not
 *   finite or not > 0 and null pointers give SUNERF_E_BADARG; a smaller workspace gives SUNERF_E_WORKSPACE.
 * ---------------------------------------------------------------------------------------------------------- */
size_t sunerf_image_metrics_workspace_bytes(int64_t n_images, int height, int width);
int sunerf_image_metrics(const float* pred, const float* target, int64_t n_images, int height, int width,
                         double data_range, double* out, void* workspace, size_t workspace_bytes, void* stream);

/* ------------------------------------------------------------------------------------------------------------
 * Analytic field of SimpleStar: replaces SimpleStar.forward, sunerf/model/stellar_model.py:53-102,
 * evaluated at the sample points o + d z (sampling.py:100) of every ray; the result feeds sunerf_dt_integral_fwd with
 * base_log_density = base_log_temperature = 0 exactly as the MLP output of NeRF_DT does
 * (DensityTemperatureRadiativeTransfer(model=SimpleStar), evaluation/image_render.py:266-268).
 *   raw [N, S, 2] out: (ln rho, log10 T);  rho_0 [cm^-3], h0 and Rs [solar radii], T0 and t_photosphere [K]
 * ---------------------------------------------------------------------------------------------------------- */
int sunerf_simple_star_field(const float* rays_o, const float* rays_d, const float* z_vals, int64_t n_rays, int n_samples,
                             float rho_0, float h0, float T0, float Rs, float t_photosphere, float* raw, void* stream);

/* Trainable SimpleStar: the stellar parameters as the reference's nn.ParameterDict `stellar_parameters` holds them
 * (stellar_model.py:5-52), in its order, so that the four scalars of an optimiser's flat buffer ARE the array:
 *   params [4] DEVICE fp32 = (Rs [solar radii], h0 [solar radii], T0 [K], rho_0 [cm^-3])
 *
 * sunerf_simple_star_field_dev: sunerf_simple_star_field with the parameters read on the device (no host copy after an
 *   optimiser step); the same fp32 arithmetic, bit for bit.
 * sunerf_simple_star_bwd: the gradient of a loss w.r.t. the four parameters, given
 *   g_raw [N, S, 2] = d loss / d (ln rho, log10 T) at o + d z  ->  g_params [4] in the order of `params`, overwritten
 *   (accumulate = 0) or added to (accumulate != 0, e.g. the parameters' slots of a flat gradient buffer).
 *   The reference's masks (radius <= 1, > 1, <= Rs, > Rs) carry no gradient; a NaN radius (missed-sphere rays of
 *   SphericalSampler) contributes exactly 0.  Deterministic: per-workgroup fp64 partials in `workspace`
 *   (sunerf_simple_star_bwd_workspace_bytes()), summed in a fixed order by a second launch; no atomics.
 *   No gradient w.r.t. rays, z or t_photosphere (a plain float in the reference). */
int sunerf_simple_star_field_dev(const float* rays_o, const float* rays_d, const float* z_vals, int64_t n_rays, int n_samples,
                                 const float* params, float t_photosphere, float* raw, void* stream);
size_t sunerf_simple_star_bwd_workspace_bytes(void);
int sunerf_simple_star_bwd(const float* rays_o, const float* rays_d, const float* z_vals, int64_t n_rays, int n_samples,
                           const float* params, float t_photosphere, const float* g_raw, void* workspace,
                           size_t workspace_bytes, float* g_params, int accumulate, void* stream);

/* ------------------------------------------------------------------------------------------------------------
 * MHD simulation cube (PSI rho / t frames): replaces MHDModel.forward, sunerf/model/mhd_model.py:76-142, as a field
 * behind sunerf_dt_integral_fwd (DensityTemperatureRadiativeTransfer(model=MHDModel), evaluation/image_render.py:244-269).
 *
 * Per point (x, y, z, t), fp32 (:100-103, :121-124):
 *   r = sqrt(x^2 + y^2 + z^2), theta = acos(z / r), phi = atan2(y, x) (+ 2 pi where < 0)
 *   f = t (flast - ffirst) + ffirst, w = f - trunc(f), f1 = floor(f), f2 = ceil(f)
 *   v_k = trilinear interpolation of frame f_k on ITS (phi, theta, r) grid, (1e-10, 1e-10) outside it (bounds inclusive),
 *         NaN for a NaN coordinate (RegularGridInterpolator(method='linear', bounds_error=False, fill_value=1e-10), :45-75)
 *   raw = (ln((1 - w) rho_1 + w rho_2), log10(1e6 ((1 - w) T_1 + w T_2)))                                  (:137-138)
 *
 * Residency: frames[] holds one SunerfMhdFrame per resident slot, slot[f - ffirst] (f = ffirst..flast) the slot of
 * frame f or -1.  A point whose frame is not resident gets NaN and sets *status = 1 (status is only ever written 1;
 * the caller zeroes it).  No host synchronisation.
 *   sunerf_mhd_field:        rays_o [N,3], rays_d [N,3], z_vals [N,S], times [N] -> raw [N,S,2]  (points o + d z in the kernel)
 *   sunerf_mhd_field_points: points [M,4] = (x, y, z, t) -> raw [M,2]
 *   sunerf_mhd_frame_bytes:  sizeof(SunerfMhdFrame), for bindings that lay the table out themselves.
 * ---------------------------------------------------------------------------------------------------------- */
typedef struct SunerfMhdFrame {
  const float* data;        /* [n_phi][n_theta][n_r] nodes, each (rho, T) interleaved: 8 bytes per node */
  const float* axis[3];     /* phi, theta, r nodes, strictly increasing */
  const int* bucket[3];     /* per axis nb[k] entries: the cell (lower node) holding the lower edge of each uniform bucket */
  int n[3];                 /* nodes per axis, >= 2 */
  int nb[3];                /* buckets per axis, >= 1 */
  float lo[3];              /* axis[k][0] */
  float hi[3];              /* axis[k][n[k] - 1] */
  float inv_width[3];       /* nb[k] / (hi[k] - lo[k]) */
  int reserved;
} SunerfMhdFrame;

size_t sunerf_mhd_frame_bytes(void);
int sunerf_mhd_field(const float* rays_o, const float* rays_d, const float* z_vals, const float* times, int64_t n_rays,
                     int n_samples, const SunerfMhdFrame* frames, const int* slot, int ffirst, int flast, float* raw,
                     int* status, void* stream);
int sunerf_mhd_field_points(const float* points, int64_t n_points, const SunerfMhdFrame* frames, const int* slot, int ffirst,
                            int flast, float* raw, int* status, void* stream);

/* ------------------------------------------------------------------------------------------------------------
 * Hierarchical (inverse-CDF) resampling + merge.
 * Replaces HierarchicalSampler.forward / sample_pdf, sampling.py:111-169 (perturb=False: u = linspace(0,1,S_f),
 * passed in as the tensor `u` [S_f] so that torch.linspace's own fp32 values are used; or a per-ray u [N,S_f]
 * with u_per_ray != 0 for perturb=True).
 *
 *   z_vals [N,S_c], weights [N,S_c] -> new_z [N,S_f], z_comb [N,S_c+S_f] (sorted);  S_c >= 3 (the pdf is weights[1:-1]), S_f >= 1
 * ---------------------------------------------------------------------------------------------------------- */
int sunerf_hier_resample(const float* z_vals, const float* weights, const float* u, int u_per_ray,
                         int64_t n_rays, int n_coarse, int n_fine, float* new_z, float* z_comb, void* stream);

/* ------------------------------------------------------------------------------------------------------------
 * Inverse-CDF sampling on given bins.
 * Replaces HierarchicalSampler.sample_pdf called by itself, sampling.py:128-169: pdf = (w + 1e-5) / sum(w + 1e-5),
 * cdf = [0, cumsum(pdf)], searchsorted(cdf, u, right=True), linear interpolation between the neighbouring bins with the
 * reference's `denom < 1e-5 -> 1` rule.  `u` as in sunerf_hier_resample.
 *
 *   bins [N,B], weights [N,B-1] -> samples [N,S_f];  B >= 2, S_f >= 1
 * ---------------------------------------------------------------------------------------------------------- */
int sunerf_sample_pdf(const float* bins, const float* weights, const float* u, int u_per_ray, int64_t n_rays,
                      int n_bins, int n_fine, float* samples, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* SUNERF_HIP_H */
