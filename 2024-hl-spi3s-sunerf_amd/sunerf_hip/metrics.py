"""Scores of a render against its target on the device: what the reference's TestImageCallback
(``sunerf/train/callback.py:46-56, 84-86``) and its evaluation scripts (``sunerf/evaluation/stash/metrics_simulation.py:41-54``,
``baseline_simulation.py:30-42``, ``uncertainty_correlation.py:56-77``) compute on the host with scikit-image and numpy.

``image_metrics`` is one call of the HIP entry point ``sunerf_image_metrics`` (two kernel launches, no host synchronisation);
``error_uncertainty_correlation`` is plain torch (a sort and reductions, once per evaluation).
"""
import math
from typing import Dict

import torch

from . import lib as _l
from ._ffi import _ptr, _stream


def image_metrics(pred: torch.Tensor, target: torch.Tensor, data_range: float) -> Dict[str, torch.Tensor]:
    """Per-image scores of ``pred`` against ``target``, device tensors of equal shape ``(..., H, W)`` (taken as contiguous
    fp32).  Returns fp64 tensors of shape ``(...)``:

    - ``ssim``: ``skimage.metrics.structural_similarity(target, pred, data_range=data_range)`` with its defaults;
    - ``mse``, ``mae``, ``me``: means of ``d**2``, ``|d|`` and ``d`` over all pixels, ``d = pred - target``;
    - ``psnr = 10 log10(data_range**2 / mse)`` (``-10 log10(mse)`` at ``data_range = 1``, as the reference computes it).

    A NaN in an image makes that image's scores NaN.  H and W must be at least 7 (skimage's window)."""
    if pred.shape != target.shape:
        raise ValueError(f'image_metrics: pred {tuple(pred.shape)} and target {tuple(target.shape)} differ in shape')
    if pred.dim() < 2:
        raise ValueError('image_metrics: inputs must be (..., H, W)')
    if not pred.is_cuda or target.device != pred.device:
        raise _l.SunerfHipError('image_metrics: pred / target must be on one ROCm device (there is no CPU path)')
    data_range = float(data_range)
    if not (math.isfinite(data_range) and data_range > 0):
        raise ValueError(f'image_metrics: data_range must be finite and > 0, got {data_range}')
    batch = pred.shape[:-2]
    height, width = pred.shape[-2:]
    if height < 7 or width < 7:
        raise ValueError(f'image_metrics: {height} x {width} images are smaller than the 7 x 7 window')
    dev = pred.device
    p = pred.detach().to(torch.float32).contiguous()
    t = target.detach().to(torch.float32).contiguous()
    n = p.numel() // (height * width)
    out = torch.empty(max(n, 1), 4, dtype=torch.float64, device=dev)
    if n:
        lib = _l.load()
        nbytes = lib.sunerf_image_metrics_workspace_bytes(n, height, width)
        ws = torch.empty(max(nbytes, 8), dtype=torch.uint8, device=dev)
        _l.call(dev, 'sunerf_image_metrics', _ptr(p), _ptr(t), n, height, width, data_range, _ptr(out), _ptr(ws), ws.numel(),
                _stream(dev))
    out = out[:n].reshape(*batch, 4)
    ssim, mse, mae, me = out.unbind(-1)
    return {'ssim': ssim, 'mse': mse, 'mae': mae, 'me': me, 'psnr': 10. * torch.log10(data_range ** 2 / mse)}


def _pearson(x: torch.Tensor, y: torch.Tensor) -> torch.Tensor:
    xm, ym = x - x.mean(), y - y.mean()
    return (xm * ym).sum() / torch.sqrt((xm * xm).sum() * (ym * ym).sum())


def _average_ranks(v: torch.Tensor) -> torch.Tensor:
    """1-based ranks of ``v`` (1-d fp64), ties sharing the mean of their ranks (``scipy.stats.rankdata(method='average')``)."""
    sorted_v, order = torch.sort(v, stable=True)
    first = torch.ones_like(sorted_v, dtype=torch.bool)
    first[1:] = sorted_v[1:] != sorted_v[:-1]
    group = torch.cumsum(first.to(torch.int64), 0) - 1              # tie group of every sorted position
    counts = torch.bincount(group).to(torch.float64)
    starts = torch.cumsum(counts, 0) - counts                          # 0-based position of each group's first element
    ranks = torch.empty_like(v)
    ranks[order] = (starts + (counts + 1.) / 2.)[group]
    return ranks


def error_uncertainty_correlation(errors: torch.Tensor, uncertainties: torch.Tensor) -> Dict[str, torch.Tensor]:
    """Pearson and Spearman correlation (0-d fp64 device tensors) of ``errors`` with ``uncertainties`` over all elements
    (``uncertainty_correlation.py:56-77``: ``|pred - gt|`` against the ensemble's ``np.std``).  Spearman uses average ranks
    for ties, as ``scipy.stats.spearmanr`` does (an ensemble of identical members has uncertainty 0 everywhere)."""
    if errors.shape != uncertainties.shape:
        raise ValueError(f'errors {tuple(errors.shape)} and uncertainties {tuple(uncertainties.shape)} differ in shape')
    x = errors.detach().reshape(-1).to(torch.float64)
    y = uncertainties.detach().reshape(-1).to(device=x.device, dtype=torch.float64)
    return {'pearson': _pearson(x, y), 'spearman': _pearson(_average_ranks(x), _average_ranks(y))}
