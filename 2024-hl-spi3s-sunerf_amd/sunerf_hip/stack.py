"""Stacks of frames of one detector combined per pixel (include/sunerf_hip_stack.h, csrc/stack.hip): the median, a
percentile, an order statistic or the mean of every pixel over up to 64 frames, after an optional clipping of the samples that
stand out of the pixel's own median -- the step in front of everything that works on one image.

* **Multi-frame rejection.**  A hit that ``despike`` cannot tell from a compact bright point in one frame is an outlier against the
  same pixel of the neighbouring exposures: ``combine(burst, method='mean', iterations=2, a=..., b=...)`` (or
  ``Instrument.combine``) is the clipped mean of a burst, and its ``mask`` says which sample of which frame was dropped.
* **Background models.**  :func:`background`: a low percentile of a long sequence is the static part of a coronagraph frame.
* **Robust stacks.**  The median or clipped mean of ``n`` frames has a noise near ``1 / sqrt(n)`` of one frame's, which is what
  ``Instrument.errors`` and the likelihood then have to be told.

A sample is valid when it is finite and not flagged in ``bad``; the clipping rule is a function of the value alone, so the
survivors of a pixel are the valid samples inside one closed interval of values and equal values share one fate.  One call enqueues
one kernel; no result is read back.  There is no CPU path: tests/stack_reference.py is the NumPy restatement."""
from typing import Optional

import numpy as np
import torch

from . import lib as _l
from ._ffi import _ptr, _stream
from .despike import MODES, _per_plane

REJECTED, INVALID = 1, 2                        # include/sunerf_hip_stack.h
METHODS = {'mean': 0, 'median': 1, 'percentile': 2, 'rank': 3, 'min': 3, 'max': 3}
TWO_SIDED = 1
MAX_FRAMES = 64
MAX_ITERATIONS = 16
MIN_MAD_FRAMES = 8
N_STATE = 4


def launch(frames, bad, params, method, q, rank, mode, flags, n_sigma, iterations, clip_min, min_valid, with_mask=True):
    """``sunerf_stack_combine`` on device tensors: ``frames`` [T, C, H, W] float32, ``bad`` uint8 of that shape or None,
    ``params`` [C, 4] float64.  Returns ``(image, count, mask, state)``: [C, H, W] float32 and uint8, [T, C, H, W] uint8 (None
    without ``with_mask``) and [C, 4] int64."""
    t, c, h, w = frames.shape
    dev = frames.device
    image = torch.empty((c, h, w), dtype=torch.float32, device=dev)
    count = torch.empty((c, h, w), dtype=torch.uint8, device=dev)
    mask = torch.empty((t, c, h, w), dtype=torch.uint8, device=dev) if with_mask else None
    state = torch.empty((c, N_STATE), dtype=torch.int64, device=dev)
    if image.numel() == 0:          # the empty call writes nothing
        return image, count, mask, state.zero_()
    _l.call(dev, 'sunerf_stack_combine', _ptr(frames), _ptr(bad), _ptr(params), t, c, h, w, int(method), float(q), int(rank), int(mode),
            int(flags), float(n_sigma), int(iterations), int(clip_min), int(min_valid), _ptr(image), _ptr(count), _ptr(mask),
            _ptr(state), _stream(dev))
    return image, count, mask, state


def combine(frames: torch.Tensor, method: str = 'median', q: Optional[float] = None, rank: Optional[int] = None, a=None, b=None,
            floor=0., mode: str = 'model', n_sigma: float = 5., iterations: int = 0, clip_min: int = 3, min_valid: int = 1,
            two_sided: bool = False, bad: Optional[torch.Tensor] = None, return_mask: bool = False) -> dict:
    """``frames`` [T, C, H, W] or [T, H, W] float32 on the device, ``1 <= T <= 64``, in image units; NaN and infinite samples are
    INVALID, as are those of ``bad`` (same shape, bool or uint8).  A longer sequence is combined in chunks.

    ``method``: 'median', 'mean', 'percentile' (of ``q`` in [0, 100], linear between the two neighbouring order statistics, NumPy's
    default), 'rank' (the order statistic ``rank``: 0 the smallest, -1 the largest, clamped to the survivors), 'min', 'max'.

    ``iterations`` > 0 clips first, at most that many passes (16 at most): while a pixel has ``clip_min`` survivors or more, every
    survivor ``v`` above the survivors' median ``m`` by more than ``n_sigma`` standard deviations is rejected (``two_sided``:
    below it too), until a pass rejects nothing.  ``mode='model'``: the variance is ``a + b * max(m, 0)`` (numbers or one per
    plane; ``despike_params`` gives an instrument's, ``Instrument.combine`` passes them); with Poisson and read noise and hits of
    10 to 30 sigma in 1 % of the samples, 8 frames miss no hit and flag 1e-5 of the clean samples, 4 frames miss only pixels hit
    twice.  ``mode='mad'``: the scale is ``max(1.4826 MAD, floor)`` of the survivors themselves; the MAD of a handful of samples
    is not a scale (3 to 5 frames miss 3 to 14 % of such hits and flag 1 to 3 % of the clean samples), so it is refused below 8
    frames; 16 frames miss about 6 hits in 1e4 and flag 1e-3 of the clean samples.

    A pixel with fewer than ``min_valid`` survivors is NaN.  Returns ``image`` [C, H, W] float32, ``count`` [C, H, W] uint8 (the
    survivors), ``mask`` [T, C, H, W] uint8 (REJECTED 1, INVALID 2; only with ``return_mask``) and per plane ``n_rejected``,
    ``n_invalid`` (samples), ``n_empty`` (NaN pixels) and ``passes`` (the most passes that rejected something at one pixel), int64
    -- all on the device; no result is read back.  (The ``[C, 4]`` parameters go to the device as a pageable copy, which torch
    synchronises the stream for, as in ``despike``; :func:`launch` on device tensors enqueues and returns.)"""
    if method not in METHODS:
        raise ValueError(f'method must be one of {sorted(METHODS)}, got {method!r}')
    if mode not in MODES:
        raise ValueError(f"mode must be 'model' or 'mad', got {mode!r}")
    if method == 'percentile':
        if q is None or not (np.isscalar(q) and 0 <= q <= 100):
            raise ValueError(f"method='percentile' needs q in [0, 100], got {q!r}")
    elif q is not None:
        raise ValueError(f'q belongs to method=\'percentile\', not to {method!r}')
    if method == 'rank':
        if rank is None or isinstance(rank, bool) or int(rank) != rank or abs(int(rank)) > 2 ** 31 - 1:
            raise ValueError(f"method='rank' needs an integer rank, got {rank!r}")
    elif rank is not None:
        raise ValueError(f'rank belongs to method=\'rank\', not to {method!r}')
    rank = {'min': 0, 'max': -1}.get(method, 0 if rank is None else int(rank))
    if not (np.isscalar(n_sigma) and np.isfinite(n_sigma) and n_sigma > 0):
        raise ValueError(f'n_sigma must be a finite number above 0, got {n_sigma!r}')
    if int(iterations) != iterations or not 0 <= int(iterations) <= MAX_ITERATIONS:
        raise ValueError(f'iterations must be an integer in 0 .. {MAX_ITERATIONS}, got {iterations!r}')
    if int(clip_min) != clip_min or not 2 <= int(clip_min) <= MAX_FRAMES:
        raise ValueError(f'clip_min must be an integer in 2 .. {MAX_FRAMES}, got {clip_min!r}')
    if int(min_valid) != min_valid or not 1 <= int(min_valid) <= MAX_FRAMES:
        raise ValueError(f'min_valid must be an integer in 1 .. {MAX_FRAMES}, got {min_valid!r}')
    if not isinstance(frames, torch.Tensor):
        raise TypeError('combine: frames must be a torch.Tensor')
    stack = frames[:, None] if frames.dim() == 3 else frames
    if stack.dim() != 4 or stack.dtype != torch.float32:
        raise ValueError(f'combine: frames must be float32 [T, C, H, W] or [T, H, W], got {frames.dtype} {tuple(frames.shape)}')
    t, c = stack.shape[:2]
    if not 1 <= t <= MAX_FRAMES:
        raise ValueError(f'combine: 1 to {MAX_FRAMES} frames, got {t} (combine a longer sequence in chunks)')
    if mode == 'mad' and iterations > 0 and t < MIN_MAD_FRAMES:
        raise ValueError(f"mode='mad' needs {MIN_MAD_FRAMES} frames or more, got {t}: the MAD of a handful of samples is not a scale")
    if mode == 'model' and iterations > 0 and (a is None or b is None):
        raise ValueError("mode='model' needs the variance parameters a and b (despike_params(instrument, C), or Instrument.combine)")
    params = np.zeros((c, 4))
    params[:, 0] = _per_plane(0.0 if a is None else a, 'a', c)
    params[:, 1] = _per_plane(0.0 if b is None else b, 'b', c)
    params[:, 2] = _per_plane(floor, 'floor', c)
    flagged = None
    if bad is not None:
        flagged = torch.as_tensor(bad)
        flagged = flagged[:, None] if flagged.dim() == 3 else flagged
        if tuple(flagged.shape) != tuple(stack.shape):
            raise ValueError(f'bad must have the shape of the frames {tuple(stack.shape)}, got {tuple(flagged.shape)}')
    if not stack.is_cuda:
        raise _l.SunerfHipError('combine runs on a ROCm device (there is no CPU path)')
    stack = stack.contiguous()
    dev = stack.device
    if flagged is not None:
        flagged = (flagged.to(dev) != 0).to(torch.uint8).contiguous()
    image, count, mask, state = launch(stack, flagged, torch.as_tensor(params, dtype=torch.float64).to(dev), METHODS[method],
                                       0.0 if q is None else q, rank, MODES[mode], TWO_SIDED if two_sided else 0, n_sigma, iterations,
                                       clip_min, min_valid, with_mask=return_mask)
    out = {'image': image, 'count': count, 'n_rejected': state[:, 0], 'n_invalid': state[:, 1], 'n_empty': state[:, 2],
           'passes': state[:, 3]}
    if return_mask:
        out['mask'] = mask
    return out


def background(frames: torch.Tensor, q: float = 5., bad: Optional[torch.Tensor] = None, **kw) -> dict:
    """The static part of a sequence: ``combine(frames, method='percentile', q=q)``.

    A white-light coronagraph frame is dominated by the F-corona (sunlight scattered by dust) and by stray light, which do not
    change over days, while the K-corona -- the electrons ``ThompsonScattering`` renders -- rotates and evolves under them.  Along
    a sequence that spans enough rotation every pixel sees the streamers pass and leave: a low order statistic of its samples is
    the static part plus the least K-corona the pixel saw (the "monthly minimum" of the LASCO and SECCHI pipelines; a low
    percentile such as the default 5 instead of the minimum itself keeps noise and dropouts out of it), and
    ``frames - background(frames)['image']`` is the K-corona to train on -- plain torch.  ``q=0`` is the minimum."""
    return combine(frames, method='percentile', q=q, bad=bad, **kw)
