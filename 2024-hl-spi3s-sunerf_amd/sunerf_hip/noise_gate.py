"""Noise gating of image sequences (include/sunerf_hip_noise_gate.h, csrc/noise_gate.hip; DeForest 2017): the
sequence is cut into overlapping apodised blocks of ``block_t x 16 x 16`` samples, every block is Fourier-transformed, every
coefficient that does not stand out of the block's own expected noise power -- the detector's noise model ``a + b max(x, 0)``
summed under the window -- is dropped (``mode='gate'``) or attenuated (``mode='wiener'``), and the blocks are transformed back and
overlap-added.  Unlike a temporal median it keeps structure that moves; it is the step that removes photon noise in front of
``prepare_image``, ``deconvolve`` and the likelihood, which then have to be told that the noise is lower and correlated.

A sample is valid when it is finite and not flagged in ``bad``; invalid samples take the mean of their block and carry no noise.
One call enqueues 64 kernels (16 for ``block_t=1``) on the current stream and reads nothing back.  There is no CPU path:
tests/noise_gate_reference.py is the NumPy restatement.

Out of scope: measuring the noise spectrum from the data (``spectrum`` is the caller's), blocks other than 16 pixels, gradients,
and registration or derotation of the frames (structure has to stay inside a block while it is in view: run
``sunerf_hip.register.register_frames`` first)."""
from typing import Optional

import numpy as np
import torch

from . import lib as _l
from ._ffi import _ptr, _stream
from .despike import _per_plane

MODES = {'gate': 0, 'wiener': 1}                # include/sunerf_hip_noise_gate.h
DEFAULT_N_SIGMA = {'gate': 3.0, 'wiener': 1.0}
FILL_INVALID = 1
BLOCK = 16
BLOCK_T = (1, 4, 8, 16)
N_STATE = 4


def launch(frames, bad, params, spectrum, block_t, mode, flags, n_sigma):
    """``sunerf_noise_gate`` on device tensors: ``frames`` [T, C, H, W] float32, ``bad`` uint8 of that shape or None, ``params``
    [C, 4] float64, ``spectrum`` [C, block_t, 16, 16] float32 or None.  Returns ``(out, state)``: float32 of the frames' shape and
    [C, 4] int64."""
    t, c, h, w = frames.shape
    dev = frames.device
    out = torch.empty((t, c, h, w), dtype=torch.float32, device=dev)
    state = torch.empty((c, N_STATE), dtype=torch.int64, device=dev)
    if out.numel() == 0:          # the empty call writes nothing
        return out, state.zero_()
    _l.call(dev, 'sunerf_noise_gate', _ptr(frames), _ptr(bad), _ptr(params), _ptr(spectrum), t, c, h, w, int(block_t), int(mode),
            int(flags), float(n_sigma), _ptr(out), _ptr(state), _stream(dev))
    return out, state


def noise_gate(frames: torch.Tensor, *, a, b, block_t: int = 8, mode: str = 'gate', n_sigma: Optional[float] = None,
               spectrum: Optional[torch.Tensor] = None, bad: Optional[torch.Tensor] = None, fill_invalid: bool = False) -> dict:
    """``frames`` [T, C, H, W] or [T, H, W] float32 on the device, in image units; the variance of a sample is
    ``a + b * max(x, 0)`` (numbers or one per plane; ``despike_params`` gives an instrument's, ``Instrument.noise_gate`` passes
    them).  NaN and infinite samples are invalid, as are those of ``bad`` (same shape, bool or uint8).

    ``block_t``: 1 (a purely spatial gate), 4, 8 or 16 frames per block, not more than ``T``.  ``mode='gate'`` keeps a coefficient
    whose power is at least ``n_sigma^2`` times the expected noise power (default 3: pure noise passes with probability
    ``exp(-9)``) and drops the others; ``mode='wiener'`` multiplies by ``max(0, 1 - n_sigma^2 P / |F|^2)`` (default 1: the classical
    estimate).  ``spectrum`` [C, block_t, 16, 16] or [block_t, 16, 16] float32, non-negative, in DFT layout, shapes the noise power
    over the coefficients (coloured noise after resampling); it has to be symmetric under ``k -> -k``.

    Returns ``image`` (the frames' shape; NaN where the input is invalid, or the gated estimate with ``fill_invalid``) and per plane
    ``n_invalid`` (samples), ``n_blocks`` (with a valid sample), ``n_kept`` and ``n_coefficients`` (non-DC coefficients of those
    blocks with a factor above 0, and all of them), int64 -- all on the device; no result is read back."""
    if mode not in MODES:
        raise ValueError(f"mode must be 'gate' or 'wiener', got {mode!r}")
    if isinstance(block_t, bool) or block_t not in BLOCK_T:
        raise ValueError(f'block_t must be one of {BLOCK_T}, got {block_t!r}')
    n_sigma = DEFAULT_N_SIGMA[mode] if n_sigma is None else n_sigma
    if not (np.isscalar(n_sigma) and np.isfinite(n_sigma) and n_sigma > 0):
        raise ValueError(f'n_sigma must be a finite number above 0, got {n_sigma!r}')
    if not isinstance(frames, torch.Tensor):
        raise TypeError('noise_gate: frames must be a torch.Tensor')
    seq = frames[:, None] if frames.dim() == 3 else frames
    if seq.dim() != 4 or seq.dtype != torch.float32:
        raise ValueError(f'noise_gate: frames must be float32 [T, C, H, W] or [T, H, W], got {frames.dtype} {tuple(frames.shape)}')
    t, c = seq.shape[:2]
    if t < block_t:
        raise ValueError(f'noise_gate: {t} frames are fewer than block_t = {block_t}: use a smaller block '
                         f'({max(n for n in BLOCK_T if n <= max(t, 1))} fits)')
    params = np.zeros((c, 4))
    params[:, 0] = _per_plane(a, 'a', c)
    params[:, 1] = _per_plane(b, 'b', c)
    shape = None
    if spectrum is not None:
        if not isinstance(spectrum, torch.Tensor) or spectrum.dtype != torch.float32:
            raise ValueError('spectrum must be a float32 torch.Tensor')
        shape = spectrum[None].expand(c, -1, -1, -1) if spectrum.dim() == 3 else spectrum
        if tuple(shape.shape) != (c, block_t, BLOCK, BLOCK):
            raise ValueError(f'spectrum must be [{c}, {block_t}, 16, 16] or [{block_t}, 16, 16], got {tuple(spectrum.shape)}')
    flagged = None
    if bad is not None:
        flagged = torch.as_tensor(bad)
        flagged = flagged[:, None] if flagged.dim() == 3 else flagged
        if tuple(flagged.shape) != tuple(seq.shape):
            raise ValueError(f'bad must have the shape of the frames {tuple(seq.shape)}, got {tuple(flagged.shape)}')
    if not seq.is_cuda:
        raise _l.SunerfHipError('noise_gate runs on a ROCm device (there is no CPU path)')
    seq = seq.contiguous()
    dev = seq.device
    if flagged is not None:
        flagged = (flagged.to(dev) != 0).to(torch.uint8).contiguous()
    if shape is not None:
        shape = shape.to(dev).contiguous()
    out, state = launch(seq, flagged, torch.as_tensor(params, dtype=torch.float64).to(dev), shape, block_t, MODES[mode],
                        FILL_INVALID if fill_invalid else 0, n_sigma)
    return {'image': out[:, 0] if frames.dim() == 3 else out, 'n_invalid': state[:, 0], 'n_blocks': state[:, 1], 'n_kept': state[:, 2],
            'n_coefficients': state[:, 3]}
