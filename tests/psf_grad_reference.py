"""NumPy fp64 restatement of include/sunerf_hip_psf_grad.h and of the host chain of sunerf_hip/psf_fit.py, on whole
arrays: the gradient of the PSF-and-bin correlation with respect to its taps (``in_b`` built with ``np.pad``, then an einsum over
strided windows), the correlation itself, the TrainablePSF formulas with their derivatives, flip-and-box with its transpose, and
a calibration fit by Adam.  Nothing here knows how the kernels sum."""
import math

import numpy as np

FWHM_PER_SIGMA = 2.0 * math.sqrt(2.0 * math.log(2.0))
ZERO, NEAREST = 0, 1


# ---- the correlation and its tap gradient ---------------------------------------------------------------------------------------
def windows_of(planes, kh, kw, bin, ay, ax, boundary):
    """``[n, H // bin, W // bin, kh, kw]`` fp64: element (p, R, C, i, j) is ``in_b[p, R bin + i - ay, C bin + j - ax]``."""
    x = np.asarray(planes, dtype=np.float64)
    n, h, w = x.shape
    oh, ow = h // bin, w // bin
    need_h, need_w = (oh - 1) * bin + kh, (ow - 1) * bin + kw          # rows and columns from index -ay, -ax on
    pad = ((0, 0), (ay, max(0, need_h - ay - h)), (ax, max(0, need_w - ax - w)))
    padded = np.pad(x, pad, mode='edge' if boundary == NEAREST else 'constant')
    view = np.lib.stride_tricks.sliding_window_view(padded, (kh, kw), axis=(1, 2))
    return view[:, ::bin, ::bin][:, :oh, :ow]


def correlate_bin(planes, K, bin, ay, ax, scale, boundary):
    """fp64 ``[n, H // bin, W // bin]``: the correlation before its rounding to fp32; plane p takes kernel ``p % len(K)``."""
    K = np.asarray(K, dtype=np.float64)
    n = np.asarray(planes).shape[0]
    win = windows_of(planes, K.shape[1], K.shape[2], bin, ay, ax, boundary)
    return scale * np.einsum('prcij,pij->prc', win, K[np.arange(n) % K.shape[0]])


def tap_gradient(planes, g_out, n_kernels, kh, kw, bin, ay, ax, scale, boundary):
    """fp64 ``[n_kernels, kh, kw]``: the header's definition."""
    g = np.asarray(g_out, dtype=np.float64)
    win = windows_of(planes, kh, kw, bin, ay, ax, boundary)
    per_plane = np.einsum('prc,prcij->pij', g, win)
    return scale * per_plane.reshape(-1, n_kernels, kh, kw).sum(axis=0)


def tap_gradient_bound(planes, g_out, n_kernels, kh, kw, bin, ay, ax, scale, boundary):
    """``2 (N + 2) 2^-53 scale sum |g_out| |in_b|`` per tap, N the number of terms of a tap: every addition of the kernel and the
    final ``* scale`` round once, the products are exact, and the factor 2 covers this restatement's own rounding."""
    n, h, w = np.asarray(planes).shape
    terms = (n // n_kernels) * (h // bin) * (w // bin)
    mass = tap_gradient(np.abs(np.asarray(planes, dtype=np.float64)), np.abs(np.asarray(g_out, dtype=np.float64)), n_kernels, kh, kw,
                        bin, ay, ax, abs(scale), boundary)
    return 2.0 * (terms + 2) * 2.0 ** -53 * mass


# ---- stamps -----------------------------------------------------------------------------------------------------------------------
def _r2(radius):
    ax = np.arange(-radius, radius + 1, dtype=np.float64)
    return ax[:, None] ** 2 + ax[None, :] ** 2


def _normalise(k, *dks):
    """``p = k / sum k`` and, for each derivative ``dk`` of k, that of p."""
    s = k.sum()
    return (k / s,) + tuple(dk / s - k * (dk.sum() / (s * s)) for dk in dks)


def gaussian_stamp(fwhm, radius):
    """``(p, dp / dlog fwhm)`` of gaussian_psf's formula."""
    sigma = fwhm / FWHM_PER_SIGMA
    r2 = _r2(radius)
    k = np.exp(-r2 / (2.0 * sigma * sigma))
    return _normalise(k, k * (r2 / (sigma * sigma)))


def moffat_stamp(fwhm, beta, radius):
    """``(p, dp / dlog fwhm, dp / dlog beta)`` of moffat_psf's formula."""
    r2 = _r2(radius)
    root = 2.0 ** (1.0 / beta)
    u = 4.0 * r2 * (root - 1.0) / (fwhm * fwhm)          # r^2 / alpha^2
    k = (1.0 + u) ** -beta
    dk_dlogf = k * (2.0 * beta * u / (1.0 + u))
    du_dbeta = 4.0 * r2 / (fwhm * fwhm) * root * math.log(2.0) * (-1.0 / (beta * beta))
    dk_dbeta = k * (-np.log1p(u) - beta * du_dbeta / (1.0 + u))
    return _normalise(k, dk_dlogf, beta * dk_dbeta)


def free_stamp(logits):
    z = np.asarray(logits, dtype=np.float64)
    e = np.exp(z - z.max())
    return e / e.sum()


def free_stamp_vjp(p, g):
    """The gradient with respect to the logits of a loss whose gradient with respect to the softmax ``p`` is ``g``."""
    return p * (g - (g * p).sum())


# ---- flip and box -----------------------------------------------------------------------------------------------------------------
def flip_box(stamp, bin):
    """``A psf``: Instrument.effective_kernel of one stamp ``(kh, kw)``."""
    kh, kw = stamp.shape
    K = np.zeros((kh + bin - 1, kw + bin - 1))
    for dy in range(bin):
        for dx in range(bin):
            K[dy:dy + kh, dx:dx + kw] += stamp[::-1, ::-1]
    return K


def flip_box_transpose(Y, bin):
    """``A^T Y`` for ``Y`` of the effective kernel's shape."""
    kh, kw = Y.shape[0] - bin + 1, Y.shape[1] - bin + 1
    out = np.zeros((kh, kw))
    for dy in range(bin):
        for dx in range(bin):
            out += Y[dy:dy + kh, dx:dx + kw]
    return out[::-1, ::-1].copy()


# ---- the calibration problem of the tests ------------------------------------------------------------------------------------------
FIT = dict(bin=2, radius=6, boundary=NEAREST, hidden=3.0, start=2.0, steps=200, lr=0.05)


def fit_scene():
    """2 x 48 x 48, rounded to fp32: a blob plus a sinusoid plus twelve point sources per plane."""
    rng = np.random.default_rng(11)
    y, x = np.mgrid[0:48, 0:48].astype(np.float64)
    planes = []
    for c in range(2):
        img = np.exp(-((y - 22.0 - 3 * c) ** 2 + (x - 25.0 + 2 * c) ** 2) / (2.0 * 9.0 ** 2)) + 0.2 * np.sin(0.4 * x + 0.23 * y + c) + 0.3
        for _ in range(12):
            img[rng.integers(4, 44), rng.integers(4, 44)] += rng.uniform(2.0, 6.0)
        planes.append(img)
    return np.stack(planes).astype(np.float32)


def observe(scene, fwhm, bin=FIT['bin'], radius=FIT['radius'], boundary=FIT['boundary']):
    """fp64: the scene through a Gaussian of ``fwhm`` and the mean of ``bin x bin`` sub-pixels."""
    K = flip_box(gaussian_stamp(fwhm, radius)[0], bin)[None]
    return correlate_bin(scene, K, bin, radius, radius, 1.0 / (bin * bin), boundary)


def fit_gaussian(scene, observed, start, steps, lr, bin=FIT['bin'], radius=FIT['radius'], boundary=FIT['boundary']):
    """Adam (torch.optim.Adam's update, betas 0.9 / 0.999, eps 1e-8) on ``log fwhm`` against the mean square: ``(fwhm, losses)``."""
    log_f, m, v = math.log(start), 0.0, 0.0
    scale = 1.0 / (bin * bin)
    k = 2 * radius + bin
    losses = []
    for step in range(1, steps + 1):
        p, dp = gaussian_stamp(math.exp(log_f), radius)
        K = flip_box(p, bin)[None]
        residual = correlate_bin(scene, K, bin, radius, radius, scale, boundary) - observed
        losses.append(float((residual * residual).mean()))
        g_K = tap_gradient(scene, 2.0 * residual / residual.size, 1, k, k, bin, radius, radius, scale, boundary)
        g = float((flip_box_transpose(g_K[0], bin) * dp).sum())
        m = 0.9 * m + 0.1 * g
        v = 0.999 * v + 0.001 * g * g
        log_f -= lr * (m / (1.0 - 0.9 ** step)) / (math.sqrt(v / (1.0 - 0.999 ** step)) + 1e-8)
    return math.exp(log_f), losses
