"""D-SSIM of a batch of detector-pixel patches as a training term (include/sunerf_hip_ssim_loss.h, csrc/ssim_loss.hip, DESIGN.md
section 8r).

``patch_ssim``  the SSIM of every plane (one channel of one patch) of a prediction against the target, fp64 ``[n, C]``.
``ssim_loss``   ``dssim(coarse) + dssim(fine)`` behind ONE autograd node, one kernel, no host read anywhere.

The images are the rows a patch batch's pixel loss receives: fp32 ``[n P P, C]``, channel last.  Per plane the SSIM is
scikit-image's ``structural_similarity(target, pred, win_size=window, data_range=data_range)`` of the ``P x P`` patch (uniform
window, sample covariances, the mean over the fully inside windows), after ``s(v) = asinh(v / vmax / a) / asinh(1 / a)`` of both
images when ``asinh_scaling=(vmax, a)`` is given.  A plane with a non-finite value is invalid: it adds nothing, its gradient is 0
and its SSIM reads NaN.  ``dssim(image) = 1 - mean over the image's valid planes``; 0 when it has none.  There is no CPU path.
"""
import math

import torch

from . import lib as _l
from ._ffi import _dev, _ptr, _stream

STAT_KEYS = ('dssim_coarse', 'dssim_fine', 'n_valid', 'n_invalid')
MIN_WINDOW, MAX_WINDOW, MAX_PATCH, MAX_CHANNELS = 3, 11, 64, 64
_ws = {}      # (device, stream, n, C) -> zero-initialised reduction workspace


def check_shape(P: int, window: int, C: int = 1):
    """Raises ``ValueError`` for a patch side, window or channel count the kernel does not take."""
    if window != int(window) or window % 2 == 0 or not MIN_WINDOW <= window <= MAX_WINDOW:
        raise ValueError(f'the SSIM window must be odd and in {MIN_WINDOW} .. {MAX_WINDOW}, got {window}')
    if not window <= P <= MAX_PATCH:
        raise ValueError(f'a patch of {P} x {P} pixels cannot take a {window} x {window} SSIM window (window <= P <= {MAX_PATCH})')
    if not 1 <= C <= MAX_CHANNELS:
        raise ValueError(f'the structural loss takes 1 .. {MAX_CHANNELS} channels, got {C}')


def _workspace(dev, n, channels) -> torch.Tensor:
    key = (dev, torch.cuda.current_stream(dev).cuda_stream, n, channels)
    ws = _ws.get(key)
    if ws is None:
        ws = _ws[key] = torch.zeros(_l.load().sunerf_ssim_loss_workspace_bytes(n, channels), dtype=torch.uint8, device=dev)
    return ws


def _check(coarse, fine, target, n, P, data_range, window, asinh_scaling):
    coarse_c = _dev(coarse, 'coarse')
    n, P, window = int(n), int(P), int(window)
    if coarse_c.dim() != 2 or n < 1 or coarse_c.shape[0] != n * P * P:
        raise ValueError(f'the images must be [n P P, C] = [{n} x {P} x {P}, C], got {tuple(coarse.shape)}')
    check_shape(P, window, coarse_c.shape[1])
    fine_c, target_c = _dev(fine, 'fine', coarse_c.shape), _dev(target, 'target', coarse_c.shape)
    if not (float(data_range) > 0.0 and math.isfinite(float(data_range))):
        raise ValueError(f'data_range must be > 0 and finite, got {data_range}')
    if asinh_scaling is not None:
        vmax, a = (float(v) for v in asinh_scaling)
        if not (vmax > 0.0 and a > 0.0 and math.isfinite(vmax) and math.isfinite(a)):
            raise ValueError(f'asinh_scaling = (vmax, a) must be > 0 and finite, got {asinh_scaling}')
        asinh_scaling = (vmax, a)
    return coarse_c, fine_c, target_c, n, P, window, float(data_range), asinh_scaling


def launch(coarse, fine, target, n, P, data_range, window=7, asinh_scaling=None, workspace=None):
    """One call of ``sunerf_ssim_loss`` on contiguous device tensors: ``(g_coarse, g_fine, plane_ssim, stats)`` with the
    gradients as the kernel leaves them: d ssim(plane) / d x, neither negated nor divided by the number of valid planes."""
    dev = coarse.device
    channels = coarse.shape[1]
    vmax, a = asinh_scaling if asinh_scaling is not None else (1.0, 1.0)
    g_coarse, g_fine = torch.empty_like(coarse), torch.empty_like(fine)
    plane_ssim = torch.empty((2, n, channels), dtype=torch.float64, device=dev)
    stats = torch.empty(4, dtype=torch.float64, device=dev)
    ws = _workspace(dev, n, channels) if workspace is None else workspace
    _l.call(dev, 'sunerf_ssim_loss', _ptr(coarse), _ptr(fine), _ptr(target), n, P, channels, window, data_range, vmax, a,
            int(asinh_scaling is not None), _ptr(g_coarse), _ptr(g_fine), _ptr(plane_ssim), _ptr(stats), _ptr(ws), ws.numel(),
            _stream(dev))
    return g_coarse, g_fine, plane_ssim, stats


class _SsimLoss(torch.autograd.Function):
    @staticmethod
    def forward(ctx, coarse, fine, target, cfg):
        g_coarse, g_fine, plane_ssim, stats = launch(*cfg['tensors'], cfg['n'], cfg['P'], cfg['data_range'], cfg['window'],
                                                     cfg['asinh_scaling'])
        # the number of valid planes of each image, from the NaN the kernel stores for an invalid plane (device arithmetic)
        counts = torch.isfinite(plane_ssim).sum(dim=(1, 2)).double().clamp_min(1.0)
        ctx.set_materialize_grads(False)
        ctx.save_for_backward(g_coarse, g_fine, counts)
        ctx.mark_non_differentiable(stats, plane_ssim)
        return stats[0] + stats[1], stats, plane_ssim

    @staticmethod
    def backward(ctx, g_loss, _g_stats, _g_plane_ssim):
        if g_loss is None:
            return None, None, None, None
        g_coarse, g_fine, counts = ctx.saved_tensors
        # d dssim / d x = -(d ssim / d x) / n_valid: -g_loss / n_valid as a device scalar, in fp64, so that a gradient is rounded to
        # fp32 twice (the kernel's store and the one below), never three times.  No valid plane: every stored gradient is 0 already.
        scale = -g_loss.double() / counts
        grads = [None] * 4
        if ctx.needs_input_grad[0]:
            grads[0] = (g_coarse.double() * scale[0]).float()
        if ctx.needs_input_grad[1]:
            grads[1] = (g_fine.double() * scale[1]).float()
        return tuple(grads)


def ssim_loss(coarse: torch.Tensor, fine: torch.Tensor, target: torch.Tensor, n: int, P: int, data_range: float, window: int = 7,
              asinh_scaling=None):
    """``dssim(coarse) + dssim(fine)`` of ``n`` patches of ``P x P`` detector pixels, images ``[n P P, C]`` (module docstring).

    Returns ``(loss, stats, plane_ssim)``: ``loss`` a 0-dim fp64 tensor differentiable with respect to ``coarse`` and ``fine``;
    ``stats`` 4 device doubles (``STAT_KEYS``: the two D-SSIM values, the valid and the invalid planes counted over both images);
    ``plane_ssim`` fp64 ``[2, n, C]`` (coarse, fine; NaN for an invalid plane).  Nothing is read back to the host."""
    coarse_c, fine_c, target_c, n, P, window, data_range, asinh_scaling = _check(coarse, fine, target, n, P, data_range, window,
                                                                                 asinh_scaling)
    cfg = {'tensors': (coarse_c, fine_c, target_c), 'n': n, 'P': P, 'data_range': data_range, 'window': window,
           'asinh_scaling': asinh_scaling}
    return _SsimLoss.apply(coarse, fine, target, cfg)


def patch_ssim(pred: torch.Tensor, target: torch.Tensor, n: int, P: int, data_range: float, window: int = 7, asinh_scaling=None):
    """The SSIM of every plane of ``pred`` ``[n P P, C]`` against ``target``: fp64 ``[n, C]``, NaN for an invalid plane.  No
    gradient."""
    pred_c, _, target_c, n, P, window, data_range, asinh_scaling = _check(pred.detach(), pred.detach(), target.detach(), n, P,
                                                                          data_range, window, asinh_scaling)
    return launch(pred_c, pred_c, target_c, n, P, data_range, window, asinh_scaling)[2][0]


def stats_dict(stats: torch.Tensor):
    return {k: stats[i] for i, k in enumerate(STAT_KEYS)}
