"""Cosmic-ray hits and hot pixels removed from observed images (include/sunerf_hip_despike.h, csrc/despike.hip): the
step in front of ``prepare_image`` -- whose spline prefilter spreads one hit over its neighbourhood -- and of
``Instrument.deconvolve``, which sharpens one into a point source.

A pixel is a hit when it stands out of the median of its clean neighbours by more than ``n_sigma`` standard deviations
(``grow_sigma`` beside a pixel already flagged, which is how tracks and the wings of a hit are caught); the standard deviation is
the instrument's noise model at that median (``mode='model'``) or the neighbours' own scatter (``mode='mad'``).  Flagged pixels
take no part in their neighbours' medians, and the test is repeated until a pass flags nothing.  Every pass and the fill are
enqueued by one call and the stopping rule is decided on the device per plane: the host never waits.  The result is the cleaned
image AND the mask, so that what follows can choose between inpainted pixels and dropped ones:

    clean = inst.despike(img, fill='nan')['image']
    obs.add_prepared_view(clean, wcs, ..., nan_policy='propagate')

There is no CPU path.  :func:`add_cosmic_rays` (plain torch on a host generator) is the generator of the tests and tools."""
from typing import Optional, Sequence, Tuple, Union

import numpy as np
import torch

from . import lib as _l
from ._ffi import _ptr, _stream, _workspace

SPIKE, INVALID, UNFILLED = 1, 2, 4              # include/sunerf_hip_despike.h
MODES = {'model': 0, 'mad': 1}
TWO_SIDED, FILL_NAN = 1, 2
MAX_ITERATIONS = 64
N_STATE = 6
_WORKSPACES = {}


def despike_params(instrument, n_channels: int) -> np.ndarray:
    """``[C, 4]`` fp64 = ``a, b, floor, 0`` per channel: the variance of an observed pixel in image units is
    ``a + b * max(x, 0)`` -- ``Instrument.errors(x) ** 2`` -- with ``b = dn_per_photon / (unit * exposure)`` and
    ``a = (read_noise^2 + (1/12 if quantise)) / (unit * exposure)^2``; ``floor = sqrt(a)``, the least scale ``mode='mad'`` admits."""
    p = instrument.params(n_channels)
    ue, g, read_noise = p[:, 0] * p[:, 1], p[:, 2], p[:, 3]
    a = (read_noise * read_noise + (1.0 / 12.0 if instrument.quantise else 0.0)) / (ue * ue)
    return np.stack([a, g / ue, np.sqrt(a), np.zeros_like(a)], axis=1)


def launch(image, bad, params, radius, mode, flags, n_sigma, grow_sigma, min_valid, max_iterations):
    """``sunerf_despike`` on device tensors: ``image`` [C, H, W] float32, ``bad`` uint8 of that shape or None, ``params`` [C, 4]
    float64.  Returns ``(clean, mask, state)``: float32 and uint8 of the image's shape and [C, 6] float64."""
    c, h, w = image.shape
    dev = image.device
    clean = torch.empty_like(image)
    mask = torch.empty(image.shape, dtype=torch.uint8, device=dev)
    state = torch.empty((c, N_STATE), dtype=torch.float64, device=dev)
    if image.numel() == 0:          # the empty call writes nothing
        return clean, mask, state.zero_()
    with torch.cuda.device(dev):
        nbytes = int(_l.load().sunerf_despike_workspace_bytes(c, h, w, radius))
    ws = _workspace(_WORKSPACES, dev, max(nbytes, 8))
    _l.call(dev, 'sunerf_despike', _ptr(image), _ptr(bad), _ptr(params), c, h, w, int(radius), int(mode), int(flags), float(n_sigma),
            float(grow_sigma), int(min_valid), int(max_iterations), _ptr(clean), _ptr(mask), _ptr(state), _ptr(ws), _stream(dev))
    return clean, mask, state


def _per_plane(value, name, c):
    v = np.atleast_1d(np.asarray(value, dtype=np.float64))
    if v.ndim != 1 or v.shape[0] not in (1, c):
        raise ValueError(f'{name} must be a number or one per plane ({c}), got shape {v.shape}')
    if not np.all(np.isfinite(v)) or np.any(v < 0):
        raise ValueError(f'{name} must be finite and >= 0, got {value!r}')
    return np.broadcast_to(v, (c,))


def despike(image: torch.Tensor, *, a=None, b=None, mode: str = 'model', floor=0., window: int = 5, n_sigma: float = 5.,
            grow_sigma: float = 3., min_valid: int = 3, iterations: int = 4, two_sided: bool = False, fill: str = 'median',
            bad: Optional[torch.Tensor] = None) -> dict:
    """``image`` [C, H, W] or [H, W] float32 on the device, in image units; NaN and infinite pixels are INVALID from the start, as
    are those of ``bad`` (same shape, bool or uint8).

    ``mode='model'``: the variance at a pixel is ``a + b * max(median, 0)`` (numbers or one per plane; :func:`despike_params`
    gives an instrument's).  ``mode='mad'``: the scale is ``max(1.4826 MAD, floor)`` of the neighbours; it needs ``window`` 5 or 7
    (the 8 neighbours of a 3 x 3 window give no usable MAD: one clean pixel in a hundred is flagged).  ``window``: 3, 5 or 7.
    ``n_sigma`` / ``grow_sigma``: the threshold, and the lower one beside a flagged pixel.  ``min_valid``: the clean neighbours a
    pixel needs to be tested or filled.  ``iterations``: detection passes at most (0: only INVALID pixels are filled).
    ``two_sided``: negative outliers too.  ``fill``: 'median' (of the clean neighbours of the ORIGINAL image; NaN and the
    UNFILLED bit where fewer than ``min_valid`` exist) or 'nan'.

    Returns ``image`` [C, H, W] float32 (untouched pixels bit for bit), ``mask`` [C, H, W] uint8 (SPIKE 1, INVALID 2, UNFILLED 4),
    and per plane ``n_spike``, ``n_invalid``, ``n_unfilled``, ``passes`` (int64: passes that flagged something) and ``converged``
    (bool: a pass flagged nothing) -- all on the device, nothing waits for the host."""
    if mode not in MODES:
        raise ValueError(f"mode must be 'model' or 'mad', got {mode!r}")
    if window not in (3, 5, 7):
        raise ValueError(f'window must be 3, 5 or 7, got {window!r}')
    if mode == 'mad' and window == 3:
        raise ValueError("mode='mad' needs window 5 or 7: the 8 neighbours of a 3 x 3 window give no usable MAD")
    if fill not in ('median', 'nan'):
        raise ValueError(f"fill must be 'median' or 'nan', got {fill!r}")
    for name, v in (('n_sigma', n_sigma), ('grow_sigma', grow_sigma)):
        if not (np.isscalar(v) and np.isfinite(v) and v > 0):
            raise ValueError(f'{name} must be a finite number above 0, got {v!r}')
    n_neighbours = window * window - 1
    if int(min_valid) != min_valid or not 1 <= int(min_valid) <= n_neighbours:
        raise ValueError(f'min_valid must be an integer in 1 .. {n_neighbours} (the neighbours of the window), got {min_valid!r}')
    if int(iterations) != iterations or not 0 <= int(iterations) <= MAX_ITERATIONS:
        raise ValueError(f'iterations must be an integer in 0 .. {MAX_ITERATIONS}, got {iterations!r}')
    if not isinstance(image, torch.Tensor):
        raise TypeError('despike: image must be a torch.Tensor')
    planes = image[None] if image.dim() == 2 else image
    if planes.dim() != 3 or planes.dtype != torch.float32:
        raise ValueError(f'despike: image must be float32 [C, H, W] or [H, W], got {image.dtype} {tuple(image.shape)}')
    c = planes.shape[0]
    if mode == 'model' and (a is None or b is None):
        raise ValueError("mode='model' needs the variance parameters a and b (despike_params(instrument, C), or Instrument.despike)")
    params = np.zeros((c, 4))
    params[:, 0] = _per_plane(0.0 if a is None else a, 'a', c)
    params[:, 1] = _per_plane(0.0 if b is None else b, 'b', c)
    params[:, 2] = _per_plane(floor, 'floor', c)
    mask_in = None
    if bad is not None:
        mask_in = torch.as_tensor(bad)
        mask_in = mask_in[None] if mask_in.dim() == 2 else mask_in
        if tuple(mask_in.shape) != tuple(planes.shape):
            raise ValueError(f'bad must have the shape of the image {tuple(planes.shape)}, got {tuple(mask_in.shape)}')
    if not planes.is_cuda:
        raise _l.SunerfHipError('despike runs on a ROCm device (there is no CPU path)')
    planes = planes.contiguous()
    dev = planes.device
    if mask_in is not None:
        mask_in = (mask_in.to(dev) != 0).to(torch.uint8).contiguous()
    flags = (TWO_SIDED if two_sided else 0) | (FILL_NAN if fill == 'nan' else 0)
    clean, mask, state = launch(planes, mask_in, torch.as_tensor(params, dtype=torch.float64).to(dev), window // 2, MODES[mode], flags,
                                n_sigma, grow_sigma, min_valid, iterations)
    return {'image': clean, 'mask': mask, 'n_spike': state[:, 0].to(torch.int64), 'n_invalid': state[:, 1].to(torch.int64),
            'n_unfilled': state[:, 2].to(torch.int64), 'passes': state[:, 3].to(torch.int64), 'converged': state[:, 4] != 0}


def add_cosmic_rays(image: torch.Tensor, rate: float, amplitude: Union[float, Tuple[float, float]], length: Sequence[int] = (1, 4),
                    sigma: Optional[torch.Tensor] = None, seed: int = 0):
    """Synthetic particle hits on ``image`` [C, H, W] or [H, W] (plain torch, a host generator: the same ``seed`` gives the same
    hits on any device): ``(image, truth)``, a copy with the hits added and the bool mask of the pixels hit.

    ``rate``: the fraction of pixels hit, per plane.  A hit is a straight track of ``length[0] .. length[1]`` pixels (uniform) from
    a uniform start in one of the eight directions, cut at the frame's edge; every pixel of it gains an amplitude drawn per track,
    uniform in ``amplitude`` (a number: that value) -- in image units, or in units of ``sigma`` (the image's shape) where given."""
    if not isinstance(image, torch.Tensor) or image.dim() not in (2, 3):
        raise ValueError('add_cosmic_rays: image must be a tensor [C, H, W] or [H, W]')
    lo_len, hi_len = int(length[0]), int(length[1])
    if not 0 <= rate <= 1 or not 1 <= lo_len <= hi_len:
        raise ValueError(f'add_cosmic_rays: rate must lie in [0, 1] and length be 1 <= lo <= hi, got {rate!r}, {length!r}')
    lo_amp, hi_amp = (float(amplitude), float(amplitude)) if np.isscalar(amplitude) else (float(amplitude[0]), float(amplitude[1]))
    if sigma is not None and tuple(sigma.shape) != tuple(image.shape):
        raise ValueError(f'sigma must have the shape of the image {tuple(image.shape)}, got {tuple(sigma.shape)}')
    planes = image[None] if image.dim() == 2 else image
    c, h, w = planes.shape
    gen = torch.Generator().manual_seed(int(seed))
    n_tracks = int(round(rate * h * w / (0.5 * (lo_len + hi_len))))
    added = torch.zeros((c, h, w), dtype=torch.float32)
    truth = torch.zeros((c, h, w), dtype=torch.bool)
    steps = torch.tensor([(-1, -1), (-1, 0), (-1, 1), (0, -1), (0, 1), (1, -1), (1, 0), (1, 1)])
    for p in range(c if n_tracks else 0):
        y = torch.randint(0, h, (n_tracks,), generator=gen)
        x = torch.randint(0, w, (n_tracks,), generator=gen)
        n = torch.randint(lo_len, hi_len + 1, (n_tracks,), generator=gen)
        step = steps[torch.randint(0, 8, (n_tracks,), generator=gen)]
        amp = lo_amp + (hi_amp - lo_amp) * torch.rand(n_tracks, generator=gen)
        for j in range(hi_len):
            yy, xx = y + j * step[:, 0], x + j * step[:, 1]
            keep = (n > j) & (yy >= 0) & (yy < h) & (xx >= 0) & (xx < w)
            added[p].index_put_((yy[keep], xx[keep]), amp[keep], accumulate=True)
            truth[p, yy[keep], xx[keep]] = True
    added, truth = added.to(image.device), truth.to(image.device)
    if sigma is not None:
        added = added * (sigma[None] if image.dim() == 2 else sigma).to(torch.float32)
    out = planes + added.to(planes.dtype)
    return (out[0], truth[0]) if image.dim() == 2 else (out, truth)
