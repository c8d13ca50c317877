"""fp64 numpy restatement of the image scores of csrc/metrics.hip and of the reference callbacks' scoring
(sunerf/train/callback.py:46-56, 84-86), written from the definitions with direct 7-tap window sums.  The GPU tests compare
the kernel with it; tests/test_metrics_host.py checks it against scikit-image's own output (tests/golden/skimage/g14_ssim_skimage.npz)."""
import numpy as np

WIN = 7
COV_NORM = 49.0 / 48.0
ASINH_A = 0.005


def _window_mean(v):
    """Mean over the 7 x 7 window around every pixel, scipy's 'reflect' boundary (numpy's 'symmetric'), direct sums."""
    h, w = v.shape
    p = np.pad(v, 3, mode='symmetric')
    rows = sum(p[:, k:k + w] for k in range(WIN))
    return sum(rows[k:k + h, :] for k in range(WIN)) / 49.0


def ssim_map(target, pred, data_range):
    x = np.asarray(target, dtype=np.float64)
    y = np.asarray(pred, dtype=np.float64)
    ux, uy = _window_mean(x), _window_mean(y)
    uxx, uyy, uxy = _window_mean(x * x), _window_mean(y * y), _window_mean(x * y)
    vx, vy, vxy = COV_NORM * (uxx - ux * ux), COV_NORM * (uyy - uy * uy), COV_NORM * (uxy - ux * uy)
    c1, c2 = (0.01 * data_range) ** 2, (0.03 * data_range) ** 2
    return (2 * ux * uy + c1) * (2 * vxy + c2) / ((ux * ux + uy * uy + c1) * (vx + vy + c2))


def ssim(target, pred, data_range):
    """skimage.metrics.structural_similarity(target, pred, data_range=data_range) of one 2-d image."""
    s = ssim_map(target, pred, data_range)
    if s.shape[0] < WIN or s.shape[1] < WIN:
        raise ValueError('win_size exceeds image extent')
    return s[3:-3, 3:-3].mean()


def image_metrics(pred, target, data_range):
    """Dict of fp64 arrays of shape (...) for inputs (..., H, W): ssim, mse, mae, me, psnr (the kernel's outputs)."""
    pred = np.asarray(pred)
    target = np.asarray(target)
    h, w = pred.shape[-2:]
    p = pred.reshape(-1, h, w).astype(np.float64)
    t = target.reshape(-1, h, w).astype(np.float64)
    d = p - t
    out = {'ssim': np.array([ssim(t[i], p[i], data_range) for i in range(p.shape[0])]),
           'mse': (d * d).mean(axis=(1, 2)), 'mae': np.abs(d).mean(axis=(1, 2)), 'me': d.mean(axis=(1, 2))}
    with np.errstate(divide='ignore'):          # identical images: psnr = inf
        out['psnr'] = 10. * np.log10(data_range ** 2 / out['mse'])
    return {k: v.reshape(pred.shape[:-2]) for k, v in out.items()}


def asinh_normalize(x):
    """ImageNormalize(vmin=0, vmax=1, stretch=AsinhStretch(0.005), clip=True) of the emission callback, in fp64:
    clip(x, 0, 1), then asinh(x / a) / asinh(1 / a) (astropy mpl_normalize.py:157-173, stretch.py:31-44, 499-504)."""
    x = np.clip(np.asarray(x, dtype=np.float64), 0., 1.)
    return np.arcsinh(x / ASINH_A) / np.arcsinh(1. / ASINH_A)


def callback_scores(fine, target, image_shape, normalize):
    """The callbacks' {'validation.loss', 'validation.ssim', 'validation.psnr'} of stored outputs (N, C): reshaped to
    (H, W, C), asinh-normalised for the emission module (then taken as fp32, the kernel's input), MSE over all channels,
    SSIM on channel 0 with data_range 1."""
    h, w = image_shape
    fine = np.asarray(fine, dtype=np.float64).reshape(h, w, -1)
    target = np.asarray(target, dtype=np.float64).reshape(h, w, -1)
    if normalize:
        fine = asinh_normalize(fine).astype(np.float32).astype(np.float64)
        target = asinh_normalize(target).astype(np.float32).astype(np.float64)
    loss = ((fine - target) ** 2).mean()
    return {'validation.loss': loss, 'validation.ssim': ssim(target[..., 0], fine[..., 0], 1.0),
            'validation.psnr': -10. * np.log10(loss)}
