"""Richardson-Lucy deconvolution of observed images against their instrument (include/sunerf_hip_deconvolve.h,
csrc/deconvolve.hip): the classical baseline of the instrument chain -- deconvolve every observed view first, then
train on rays as before -- beside training THROUGH the instrument.

The iteration is the shifted-Poisson form (Snyder et al. 1993), the EM iteration for Poisson counts plus Gaussian read noise:
with ``A = Instrument.expected``, ``c`` photons per image unit and ``off`` the read variance in image units of the same scale,

    u <- u * A^T((d + off) / (A u + off)) / A^T(valid)

Every iterate's goodness of fit, the Poisson deviance per valid pixel, is reduced on the device, and the discrepancy rule --
stop at the first iterate whose deviance per valid pixel is at most the threshold, 1 for a model that fits to the noise -- is
decided there too: one call enqueues all iterations and the host never waits between them.  There is no CPU path; ``init`` is
built in plain torch (it is not the hot path)."""
from typing import Optional, Union

import numpy as np
import torch

from . import lib as _l
from ._ffi import _ptr, _stream, _workspace
from .instrument import BOUNDARY, Instrument, correlate_bin_adjoint

MAX_ITERATIONS = 10000                           # include/sunerf_hip_deconvolve.h
N_STATE = 4
_WORKSPACES = {}


def photon_params(instrument: Instrument, n_channels: int) -> np.ndarray:
    """``[C, 2]`` fp64 = ``c, v`` per channel: ``c = unit * exposure / dn_per_photon`` photons per image unit and
    ``v = (read_noise^2 + (1/12 if quantise)) / dn_per_photon^2`` the read variance in photons^2."""
    p = instrument.params(n_channels)
    unit, exposure, g, read_noise = p[:, 0], p[:, 1], p[:, 2], p[:, 3]
    c = unit * exposure / g
    v = (read_noise * read_noise + (1.0 / 12.0 if instrument.quantise else 0.0)) / (g * g)
    return np.stack([c, v], axis=1)


def launch(u, d, bad, norm, params, taps, n_kernels, kh, kw, bin_factor, ay, ax, scale, boundary, n_iterations, stop):
    """``sunerf_deconvolve_richardson_lucy`` on device tensors: ``u`` [C, H, W] float32 is updated in place; returns ``(state, ratio)``:
    ``state`` [C, 4] float64 (deviance, n_valid, iterations_applied, stopped) and ``ratio`` [C, h, w] float32, the call's scratch
    (the ratio of the last pass that ran on each plane).  ``params`` [C, 2] and ``taps`` are float64 on the device, ``bad`` uint8
    or None."""
    c, h, w = u.shape
    dev = u.device
    state = torch.empty((c, N_STATE), dtype=torch.float64, device=dev)
    ratio = torch.empty((c, h // bin_factor, w // bin_factor), dtype=torch.float32, device=dev)
    if ratio.numel() == 0:          # the empty call writes nothing
        return state.zero_(), ratio
    with torch.cuda.device(dev):
        nbytes = int(_l.load().sunerf_deconvolve_workspace_bytes(c, h, w, kh, kw, bin_factor))
    ws = _workspace(_WORKSPACES, dev, max(nbytes, 8))
    _l.call(dev, 'sunerf_deconvolve_richardson_lucy', _ptr(u), _ptr(d), _ptr(bad), _ptr(norm), _ptr(params), c, h, w, _ptr(taps),
            n_kernels, kh, kw, bin_factor, ay, ax, float(scale), boundary, int(n_iterations), float(stop), _ptr(ratio), _ptr(state),
            _ptr(ws), _stream(dev))
    return state, ratio


def initial_image(image: torch.Tensor, valid: torch.Tensor, instrument: Instrument, init='image') -> torch.Tensor:
    """The start of the iteration, [C, h bin, w bin] float32 (plain torch).  'image': every detector pixel replicated
    ``bin x bin`` (divided by ``bin^2`` under ``bin_mode='sum'``), invalid or non-positive pixels replaced by the plane's mean
    over its valid positive pixels (1 for a plane that has none); 'flat': that mean everywhere."""
    b = instrument.bin
    x = image / float(b * b) if instrument.bin_mode == 'sum' else image
    good = valid & (x > 0)
    count = good.sum(dim=(1, 2), keepdim=True)
    total = torch.where(good, x, torch.zeros_like(x)).double().sum(dim=(1, 2), keepdim=True)
    mean = torch.where(count > 0, total / count.clamp_min(1), torch.ones_like(total)).to(torch.float32)
    if init == 'flat':
        start = mean.expand_as(x)
    else:
        start = torch.where(good, x, mean.expand_as(x))
    return start.repeat_interleave(b, dim=1).repeat_interleave(b, dim=2).contiguous()


def richardson_lucy(image: torch.Tensor, instrument: Instrument, iterations: int = 25,
                    stop: Optional[Union[str, float]] = None, bad: Optional[torch.Tensor] = None, init='image') -> dict:
    """``image`` [C, h, w] or [h, w] float32 on the device, an observed frame in image units, deconvolved against
    ``instrument``'s PSF, binning and noise model.  ``iterations``: the number of updates at most.  ``stop``: None runs exactly
    that many; 'discrepancy' stops a plane at the first iterate whose Poisson deviance per valid pixel is <= 1, a float sets
    that threshold.  ``bad`` (same shape, bool or uint8): pixels that take no part, beside the non-finite ones.  ``init``:
    'image', 'flat' (:func:`initial_image`) or a float32 tensor [C, h bin, w bin] (copied).

    Returns ``image`` [C, h bin, w bin] (the iterate of the frame ``Instrument.latent_grid`` describes), ``deviance`` [C]
    (float64, per valid pixel, of that iterate), ``iterations`` [C] (int64, updates applied), ``stopped`` [C] (bool: the
    iterate meets the threshold) and ``norm`` [C, h bin, w bin] (A^T of the valid mask: 0 where no valid pixel sees the frame)."""
    d = instrument._planes(image, 'richardson_lucy')
    c, h, w = d.shape
    dev = d.device
    if int(iterations) != iterations or not 0 <= int(iterations) <= MAX_ITERATIONS:
        raise ValueError(f'iterations must be an integer in 0 .. {MAX_ITERATIONS}, got {iterations}')
    if stop is None:
        threshold = 0.0
    elif isinstance(stop, str):
        if stop != 'discrepancy':
            raise ValueError(f"stop must be None, 'discrepancy' or a positive number, got {stop!r}")
        threshold = 1.0
    else:
        threshold = float(stop)
        if not threshold > 0.0:
            raise ValueError(f"stop must be None, 'discrepancy' or a positive number, got {stop!r}")
    K, (ay, ax) = instrument.effective_kernel()
    if (K < 0).any():
        raise ValueError('richardson_lucy needs a PSF without negative taps (the iterates would not stay non-negative)')
    if K.shape[0] not in (1, c):
        raise ValueError(f'the psf has {K.shape[0]} channels, the image {c}')
    params = torch.as_tensor(photon_params(instrument, c), dtype=torch.float64).to(dev)
    mask = None
    if bad is not None:
        mask = torch.as_tensor(bad, device=dev)
        mask = mask[None] if mask.dim() == 2 else mask
        if tuple(mask.shape) != (c, h, w):
            raise ValueError(f'bad must have the shape of the image {(c, h, w)}, got {tuple(mask.shape)}')
        mask = (mask != 0).to(torch.uint8).contiguous()
    valid = torch.isfinite(d) if mask is None else torch.isfinite(d) & (mask == 0)
    b = instrument.bin
    height, width = h * b, w * b
    if isinstance(init, torch.Tensor):
        if tuple(init.shape) != (c, height, width) or init.dtype != torch.float32 or init.device != dev:
            raise ValueError(f'init must be float32 [{c}, {height}, {width}] on {dev}, got {init.dtype} {tuple(init.shape)} on {init.device}')
        u = init.detach().clone().contiguous()
    elif init in ('image', 'flat'):
        u = initial_image(d, valid, instrument, init)
    else:
        raise ValueError(f"init must be 'image', 'flat' or a tensor, got {init!r}")
    taps = instrument._taps(K, dev)
    call = (taps, K.shape[0], K.shape[1], K.shape[2], b, ay, ax, instrument.scale, BOUNDARY[instrument.boundary])
    norm = correlate_bin_adjoint(valid.to(torch.float32), height, width, *call)
    state, _ = launch(u, d, mask, norm, params, *call, int(iterations), threshold)
    return {'image': u, 'deviance': state[:, 0] / state[:, 1].clamp_min(1.0), 'iterations': state[:, 2].to(torch.int64),
            'stopped': state[:, 3] != 0, 'norm': norm}
