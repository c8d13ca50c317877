"""fp64 numpy restatement of the structural loss of csrc/ssim_loss.hip (include/sunerf_hip_ssim_loss.h), written
from the definitions: every window's five sums are direct sums over its w x w pixels (w columns, then w rows; nothing is carried
from one window to the next and nothing is ever taken off a sum), the gradient is the
closed form d S / d x_p = alpha + beta x_p + gamma y_p gathered by direct zero-padded box sums.  The GPU tests compare the kernel
with it; tests/test_ssim_loss_host.py checks its value against tests/metrics_reference.py (and through it scikit-image) and its
gradient against central differences.  Images are the kernel's rows: ``[n P P, C]``, channel last."""
import numpy as np


def stretch(v, asinh_scaling):
    """``s(v) = asinh(v / vmax / a) / asinh(1 / a)`` in fp64, or ``v``."""
    v = np.asarray(v, dtype=np.float64)
    if asinh_scaling is None:
        return v
    vmax, a = asinh_scaling
    return np.arcsinh(v / vmax / a) / np.arcsinh(1.0 / a)


def stretch_derivative(v, asinh_scaling):
    v = np.asarray(v, dtype=np.float64)
    if asinh_scaling is None:
        return np.ones_like(v)
    vmax, a = asinh_scaling
    u = v / vmax / a
    return 1.0 / (np.sqrt(1.0 + u * u) * vmax * a * np.arcsinh(1.0 / a))


def _window_sums(v, w):
    """[W, W]: the sum of ``v`` over every fully inside w x w window: w shifted columns added, then w shifted rows of those."""
    n = v.shape[0] - w + 1
    rows = np.zeros((v.shape[0], n))
    for dx in range(w):
        rows += v[:, dx:dx + n]
    out = np.zeros((n, n))
    for dy in range(w):
        out += rows[dy:dy + n, :]
    return out


def _box_back(m, w, p):
    """[P, P]: the zero-padded w x w box sum of a window map back onto the pixels: pixel (r, q) gets every window that holds it."""
    n = m.shape[0]
    rows = np.zeros((n, p))
    for dx in range(w):
        rows[:, dx:dx + n] += m
    out = np.zeros((p, p))
    for dy in range(w):
        out[dy:dy + n, :] += rows
    return out


def ssim_map(x, y, window, data_range):
    """``(S, alpha, beta, gamma)`` [W, W] of stretched planes ``x`` (prediction) and ``y`` (target)."""
    n = float(window * window)
    sx, sy = _window_sums(x, window), _window_sums(y, window)
    sxx, syy, sxy = _window_sums(x * x, window), _window_sums(y * y, window), _window_sums(x * y, window)
    mu_x, mu_y = sx / n, sy / n
    var_x, var_y, cov = (sxx - n * mu_x * mu_x) / (n - 1), (syy - n * mu_y * mu_y) / (n - 1), (sxy - n * mu_x * mu_y) / (n - 1)
    c1, c2 = (0.01 * data_range) ** 2, (0.03 * data_range) ** 2
    a1, a2 = 2 * mu_x * mu_y + c1, 2 * cov + c2
    b1, b2 = mu_x * mu_x + mu_y * mu_y + c1, var_x + var_y + c2
    s = a1 * a2 / (b1 * b2)
    gamma = 2 * a1 / ((n - 1) * b1 * b2)
    beta = -2 * s / ((n - 1) * b2)
    alpha = (2 * mu_y / n) * a2 / (b1 * b2) - gamma * mu_y - s * (2 * mu_x / n) / b1 - beta * mu_x
    return s, alpha, beta, gamma


def ssim(pred, target, window=7, data_range=1.0, asinh_scaling=None):
    """The SSIM of one ``P x P`` plane: the mean over the fully inside windows."""
    return ssim_map(stretch(pred, asinh_scaling), stretch(target, asinh_scaling), window, data_range)[0].mean()


def ssim_and_gradient(pred, target, window=7, data_range=1.0, asinh_scaling=None):
    """``(ssim, d ssim / d pred [P, P])`` of one plane."""
    x, y = stretch(pred, asinh_scaling), stretch(target, asinh_scaling)
    p = x.shape[0]
    s, alpha, beta, gamma = ssim_map(x, y, window, data_range)
    g = (_box_back(alpha, window, p) + x * _box_back(beta, window, p) + y * _box_back(gamma, window, p)) / s.size
    return s.mean(), g * stretch_derivative(pred, asinh_scaling)


def evaluate(coarse, fine, target, n, P, window=7, data_range=1.0, asinh_scaling=None):
    """Every output of the kernel and of the autograd node for images ``[n P P, C]``: ``plane_ssim`` [2, n, C] (NaN where the
    plane is invalid), ``g_coarse`` / ``g_fine`` as the kernel stores them (d ssim(plane) / d x, 0 on an invalid plane),
    ``stats`` [4], ``loss`` = stats[0] + stats[1] and ``d_coarse`` / ``d_fine`` = d loss / d x."""
    images = [np.asarray(v, dtype=np.float64).reshape(n, P, P, -1) for v in (coarse, fine, target)]
    channels = images[0].shape[-1]
    plane_ssim = np.full((2, n, channels), np.nan)
    grads = [np.zeros_like(images[0]), np.zeros_like(images[0])]
    for k in range(n):
        for c in range(channels):
            y = images[2][k, :, :, c]
            for i in range(2):
                x = images[i][k, :, :, c]
                if np.isfinite(x).all() and np.isfinite(y).all():          # every plane is looked at: none is left out
                    plane_ssim[i, k, c], grads[i][k, :, :, c] = ssim_and_gradient(x, y, window, data_range, asinh_scaling)
    valid = np.isfinite(plane_ssim)
    counts = valid.sum(axis=(1, 2))
    dssim = [1.0 - plane_ssim[i][valid[i]].sum() / counts[i] if counts[i] else 0.0 for i in range(2)]
    stats = np.array([dssim[0], dssim[1], float(counts.sum()), float(2 * n * channels - counts.sum())])
    shape = (n * P * P, channels)
    return {'plane_ssim': plane_ssim, 'g_coarse': grads[0].reshape(shape), 'g_fine': grads[1].reshape(shape), 'stats': stats,
            'loss': dssim[0] + dssim[1], 'counts': counts,
            'd_coarse': -grads[0].reshape(shape) / max(counts[0], 1), 'd_fine': -grads[1].reshape(shape) / max(counts[1], 1)}


KINDS = ('noise', 'smooth', 'flat')


def make_plane(P, kind, rng):
    """One ``P x P`` fp32 plane in (0, 1): uniform noise, a smooth field, or a nearly flat plane (1e-3 of ripple on 0.1).

    The level of the flat plane follows from the definition itself: var = (sum x^2 - N mu^2) / (N - 1) carries a rounding error of
    a few ulp(mu^2), which SSIM divides by B2 >= C2 = 9e-4 R^2.  At a level of 0.1 that is a few 1.7e-18 / 9e-4 = 1e-14 per window
    for ANY two fp64 evaluations that order their sums differently (this file, tests/metrics_reference.py, the kernel); at a level of
    0.5 it is 30 times as much, which no fp64 evaluation of these formulas can hold to 1e-13."""
    if kind == 'noise':
        v = rng.uniform(0.02, 1.0, (P, P))
    else:
        r, q = np.meshgrid(np.arange(P) / max(P - 1, 1), np.arange(P) / max(P - 1, 1), indexing='ij')
        field = 0.5 + 0.4 * np.sin(2.0 * r + rng.uniform(0, 3)) * np.cos(3.0 * q + rng.uniform(0, 3))
        v = field if kind == 'smooth' else 0.1 + 1e-3 * (field - 0.5) + 1e-4 * rng.uniform(-1, 1, (P, P))
    return v.astype(np.float32)


def make_case(n, P, C, seed):
    """``coarse, fine, target`` [n P P, C] fp32: per plane one of the three kinds in turn; the predictions are the target times a
    smooth gain plus noise, so that SSIM is neither 0 nor 1."""
    rng = np.random.default_rng([seed, n, P, C])
    target = np.empty((n, P, P, C), dtype=np.float32)
    for k in range(n):
        for c in range(C):
            target[k, :, :, c] = make_plane(P, KINDS[(k * C + c) % 3], rng)
    out = []
    for spread in (0.2, 0.05):
        pred = target * rng.uniform(1 - spread, 1 + spread, (n, 1, 1, C)) + spread * 0.5 * rng.uniform(-1, 1, target.shape) * target
        out.append(pred.astype(np.float32).reshape(n * P * P, C))
    return out[0], out[1], target.reshape(n * P * P, C)
