"""Float64 restatement of the training update (csrc/train_step.hip): the loss of ``loss_kernel``, the gradient norm and clip
coefficient of ``grad_norm_kernel`` and the Adam step of ``adam_kernel``, evaluated on the same fp32 inputs the kernels get,
with error bounds derived from the kernels' arithmetic (tests/test_gpu_update_f64.py; checked against torch in float64 by
tests/test_update_reference_host.py).

Inputs are taken as the fp32 values the kernels see -- images, gradients, moments, and also the scalars, which the C ABI passes
as ``float`` (lambdas, ``vmax``, ``a``, ``grad_scale``, ``max_norm``) or which torch rounds to fp32 where a python float meets an
fp32 tensor (Adam's ``1 - beta1``, ``beta2``, ``1 - beta2``, ``eps``, ``step_size``, ``sqrt(bias_correction2)``).  Everything
after that is float64.

Bounds are first-order in ``U`` = 2^-24, the unit roundoff of fp32: a correctly rounded fp32 operation is off by at most
``U |result|``; ``asinhf`` is taken as at most 2 ulp = 4 U.  A reduction launch has ``min(128, ceil(n_max / 256))`` workgroups
of 256 threads; each thread sums its terms in fp32 (``terms_per_thread``), the partials are summed in fp64 (error ~2^-53, not
counted), and the sum of k fp32 terms is off by at most (k - 1) U sum|term|.
"""
import math

import numpy as np
import torch

U = 2.0 ** -24              # fp32 unit roundoff
TINY = 2.0 ** -126          # smallest normal fp32: absolute floor for a value that underflows into the subnormal range
THREADS, MAX_BLOCKS = 256, 128
SCALE_ROUNDINGS = 7         # s(x) = asinhf((x / vmax) / a) / norm: two divisions, asinhf (4 U), the normalisation
SCALE_GRAD_ROUNDINGS = 8    # s'(x) = 1 / (sqrtf(u * u + 1) * norm * a * vmax), u from two divisions: 8 roundings deep


def f32(x: float) -> float:
    return float(np.float32(x))


def ulp32(x: torch.Tensor) -> torch.Tensor:
    """Spacing of the fp32 grid at |x| (float64 tensor)."""
    a = np.abs(x.cpu().numpy().astype(np.float32))
    return torch.from_numpy(np.spacing(a).astype(np.float64))


def reduction_threads(n_max: int) -> int:
    """Threads of a reduction launch over arrays of at most ``n_max`` elements (train_step.hip: ``blocks_for``)."""
    return THREADS * max(1, min(MAX_BLOCKS, -(-n_max // THREADS)))


def terms_per_thread(n: int, threads: int) -> int:
    """Most fp32 terms a thread sums of an n-element array.  A scalar grid-stride loop gives ceil(n / threads); ``sweep()``'s
    16-byte path takes 4 elements from each of its ceil(floor(n / 4) / threads) vectors, plus at most one tail element."""
    return max(-(-n // threads), 4 * -(-(n // 4) // threads) + 1)


def asinh_constants(scaling):
    """(vmax, a, normalisation) as the kernel holds them: fp32 vmax and a, asinh(1 / a) in fp64 rounded to fp32."""
    vmax, a = f32(scaling[0]), f32(scaling[1])
    return vmax, a, f32(math.asinh(1.0 / a))


def _d(x):
    return x.detach().cpu().double().reshape(-1)


def loss64(coarse, fine, target, reg, lambda_image, lambda_regularization, scaling=None, finite_check=()):
    """sunerf.py:105-125 in float64: ``lambda_image (MSE(s(coarse), s(target)) + MSE(s(fine), s(target))) + lambda_reg mean(reg)``,
    PSNR = -10 log10(MSE(fine)), d loss / d image, and the count of non-finite values among the images, ``reg`` and
    ``finite_check``.  Also returns what the bounds need (scaled values, differences, d s / d image)."""
    c, f, t = _d(coarse), _d(fine), _d(target)
    r = _d(reg) if reg is not None else torch.zeros(0, dtype=torch.float64)
    li, lr = f32(lambda_image), f32(lambda_regularization)
    if scaling is None:
        def s(x):
            return x

        def ds(x):
            return torch.ones_like(x)
    else:
        vmax, a, norm = asinh_constants(scaling)

        def s(x):
            return torch.asinh(x / vmax / a) / norm

        def ds(x):
            u = x / vmax / a
            return 1.0 / (torch.sqrt(u * u + 1.0) * norm * a * vmax)
    sc, sf, st = s(c), s(f), s(t)
    dc, df = sc - st, sf - st
    n = c.numel()
    mse_c, mse_f = (dc * dc).sum().item() / n, (df * df).sum().item() / n
    reg_mean = r.sum().item() / r.numel() if r.numel() else 0.0
    gscale = 2.0 * li / n
    count = sum(int((~torch.isfinite(_d(x))).sum()) for x in (coarse, fine, *([reg] if reg is not None else []), *finite_check))
    return {'loss': li * (mse_c + mse_f) + lr * reg_mean, 'coarse': mse_c, 'fine': mse_f, 'regularization': reg_mean,
            'psnr': math.inf if mse_f == 0 else -10.0 * math.log10(mse_f), 'non_finite': count,
            'g_coarse': gscale * dc * ds(c), 'g_fine': gscale * df * ds(f),
            # for the bounds
            'n': n, 'r': r, 'lambda_image': li, 'lambda_regularization': lr, 'gscale': gscale, 'scaled': scaling is not None,
            'sc': sc, 'sf': sf, 'st': st, 'dc': dc, 'df': df, 'ds_c': ds(c), 'ds_f': ds(f)}


def loss_bounds(ref, threads):
    """Bounds on |kernel - ref| for every loss output, given the launch's thread count.

    Per element, s(x) carries SCALE_ROUNDINGS U relative error and the difference d = s(x) - s(t) one more rounding:
    delta = SCALE_ROUNDINGS U (|s(x)| + |s(t)|) + U |d|.  The MSE sums the fp32 squares (one rounding each) in k-term thread
    sums, then divides once: (sum 2 |d| delta + (k + 1) U sum d^2) / n + U mse.  The regularisation mean: k U sum|r| / n_reg +
    U |mean|.  The loss adds four roundings on top, PSNR = -10 log10f(mse) 10 / ln 10 times the MSE's relative error plus 5 U
    (log10f of 2 ulp, the product).  The image gradient gscale d s'(x): gscale (1 rounding), s'(x), two products, plus the
    error of d times gscale s'(x)."""
    n, r = ref['n'], ref['r']
    k_img = -(-n // threads)                        # the image loop is a scalar grid-stride loop
    k_reg = terms_per_thread(r.numel(), threads)
    sr = SCALE_ROUNDINGS if ref['scaled'] else 0
    out = {}
    for key, sx, d in (('coarse', ref['sc'], ref['dc']), ('fine', ref['sf'], ref['df'])):
        delta = sr * U * (sx.abs() + ref['st'].abs()) + U * d.abs() + TINY
        out[key] = ((2 * d.abs() * delta + delta * delta).sum().item() + (k_img + 1) * U * (d * d).sum().item()) / n \
            + U * ref[key]
        out['delta_' + key] = delta
    out['regularization'] = (k_reg * U * r.abs().sum().item() / r.numel() + U * abs(ref['regularization'])) if r.numel() else 0.0
    li, lr = ref['lambda_image'], ref['lambda_regularization']
    out['loss'] = li * (out['coarse'] + out['fine']) + abs(lr) * out['regularization'] \
        + 4 * U * (li * (ref['coarse'] + ref['fine']) + abs(lr * ref['regularization']))
    out['psnr'] = (10.0 / math.log(10.0)) * out['fine'] / ref['fine'] + 5 * U * abs(ref['psnr']) if ref['fine'] > 0 else 0.0
    sg = SCALE_GRAD_ROUNDINGS if ref['scaled'] else 0
    for key, g, dsx in (('g_coarse', ref['g_coarse'], ref['ds_c']), ('g_fine', ref['g_fine'], ref['ds_f'])):
        out[key] = (sg + 3) * U * g.abs() + ref['gscale'] * dsx.abs() * out['delta_' + key[2:]] + TINY
    return out


def clip64(grads, grad_scale, max_norm):
    """clip_grad_norm_ of ``grads * grad_scale`` in float64: (total norm, coefficient max_norm / (total + 1e-6) capped at 1;
    1 when ``max_norm`` <= 0)."""
    g = _d(grads) * f32(grad_scale)
    total = math.sqrt((g * g).sum().item())
    coef = min(f32(max_norm) / (total + f32(1e-6)), 1.0) if f32(max_norm) > 0 else 1.0
    return total, coef


def clip_bounds(n, total, coef, max_norm):
    """|total_kernel - total| and |coef_kernel - coef|.  Each thread sums k fp32 squares of fl(g * grad_scale) (three roundings
    per term), so the sum of squares is off by (k + 2) U of itself (+ an underflow floor per term); the square root halves the
    relative error and the conversion to fp32 adds U.  The coefficient adds the sum with 1e-6 and the division (2 U)."""
    k = terms_per_thread(n, reduction_threads(n))
    e_total = ((k + 2) / 2 + 1) * U * total + (n * 2.0 ** -149 / (2 * total) if total > 0 else math.sqrt(n * 2.0 ** -149))
    if f32(max_norm) <= 0:
        return e_total, 0.0                       # clipping off: the coefficient is 1 exactly
    capped = f32(max_norm) / (total + e_total + f32(1e-6)) * (1 - 2 * U) >= 1.0       # fminf(q, 1) = 1 exactly
    return e_total, 0.0 if capped else coef * (e_total / (total + f32(1e-6)) + 2 * U)


def adam64(params, grads, exp_avg, exp_avg_sq, step, lr, betas, eps, grad_scale, coef):
    """One torch.optim.Adam step (torch/optim/adam.py, single tensor, no weight decay / amsgrad) on the clipped, scaled
    gradient ``grads * grad_scale * coef``, in float64 from the fp32 state.  ``step`` is the number of the applied update."""
    b1, b2 = betas
    omb1, b2f, omb2, epsf = f32(1.0 - b1), f32(b2), f32(1.0 - b2), f32(eps)
    step_size = f32(lr / (1.0 - b1 ** step))
    bc2_sqrt = f32(math.sqrt(1.0 - b2 ** step))
    g = _d(grads) * f32(grad_scale) * coef
    m0, v0, p0 = _d(exp_avg), _d(exp_avg_sq), _d(params)
    m = m0 + omb1 * (g - m0)                                   # exp_avg.lerp_(grad, 1 - beta1)
    v = v0 * b2f + omb2 * g * g                                # exp_avg_sq.mul_(beta2).addcmul_(grad, grad, value=1 - beta2)
    denom = torch.sqrt(v) / bc2_sqrt + epsf                    # (exp_avg_sq.sqrt() / bias_correction2_sqrt).add_(eps)
    dp = -step_size * m / denom                                # param.addcdiv_(exp_avg, denom, value=-step_size)
    return {'g': g, 'm': m, 'v': v, 'denom': denom, 'dp': dp, 'p': p0 + dp, 'm0': m0, 'v0': v0,
            'step_size': step_size, 'bc2_sqrt': bc2_sqrt, 'omb1': omb1, 'b2f': b2f, 'omb2': omb2}


def adam_bounds(ref, coef, e_coef, p_new):
    """Per-element bounds on the written-back gradient, m, v and the update Delta p = p_new - p_old.

    g = fl(fl(x gs) coef): 2 U + the coefficient's relative error.  m = m0 + fl(omb1 fl(g - m0)): three roundings.
    v = fl(v0 b2) + fl(fl(omb2 g) g): four roundings, and g's error twice.  denom = fl(fl(sqrtf(v) / bc2) + eps), with
    |sqrt(v') - sqrt(v)| <= min(e_v / sqrt(v), sqrt(e_v)).  Delta p = fl(fl(-ss m) / denom), then the write-back to p (half an
    ulp of p_new, taken as a whole ulp: the form |Delta p - Delta p64| <= c U |Delta p64| + ulp(p_new), with m's own error
    added where m cancels); 2 U more on ss and bc2 for the device's double pow() rounding on the other side of an fp32 tie."""
    g, m, v, m0, v0 = ref['g'], ref['m'], ref['v'], ref['m0'], ref['v0']
    omb1, omb2, b2f = ref['omb1'], ref['omb2'], ref['b2f']
    e_g = g.abs() * ((e_coef / coef if coef > 0 else 0.0) + 2 * U) + TINY
    e_m = omb1 * (e_g + 2 * U * (g - m0).abs()) + U * m.abs() + TINY
    e_v = 2 * omb2 * g.abs() * e_g + U * (b2f * v0 + 2 * omb2 * g * g + v) + TINY
    sv = torch.sqrt(v)
    e_s = torch.minimum(e_v / sv.clamp_min(1e-300), torch.sqrt(e_v)) + U * sv
    q = sv / ref['bc2_sqrt']
    e_den = e_s / ref['bc2_sqrt'] + U * (2 * q + ref['denom'])
    dp = ref['dp']
    e_dp = ref['step_size'] * e_m / ref['denom'] + dp.abs() * (e_den / ref['denom'] + 4 * U) + ulp32(p_new)
    return {'g': e_g, 'm': e_m, 'v': e_v, 'dp': e_dp}
