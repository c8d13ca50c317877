"""The Gaussian noise likelihood of the detector model as the training loss, with trainable cross-calibration gains
(include/sunerf_hip_likelihood.h, csrc/likelihood.hip).

``NoiseLikelihood``  the table the kernel reads: per row (a channel code of a ``ResponseSet``, or the emission module's single
                     channel) the noise scalars of its ``Instrument`` and a trainable ``log_gain``.
``likelihood_loss``  ``training_loss``'s counterpart: ONE kernel behind an autograd node, no host read anywhere.

Per slot, in fp64: ``m = exp(log_gain[row]) p`` and ``var(x) = (max(x, 0) U E G + R^2 + extra_var) / (U E)^2``, whose square root
is ``Instrument.errors(x)``.  ``mode='observed'``: ``(m - t)^2 / (var(t) + floor^2)``, the classical chi-square with fixed weights;
``mode='model'``: ``(m - t)^2 / s2 + ln s2`` with ``s2 = var(m) + floor^2``, the negative log-likelihood whose variance follows
the model.  There is no CPU path.
"""
import ctypes
from collections.abc import Mapping
from typing import Iterable, Optional

import numpy as np
import torch
from torch import nn

from . import lib as _l
from ._ffi import _dev, _ptr, _stream
from .instrument import Instrument
from .response import MAX_CHANNELS, ResponseSet, as_response_set

MODES = {'observed': 0, 'model': 1}
STAT_KEYS = ('loss', 'coarse', 'fine', 'regularization', 'psnr', 'non_finite', 'n_valid', 'unknown_codes')
CHANNEL_STAT_KEYS = ('n_valid', 'coarse', 'fine', 'squared_error')
N_NOISE = 8
_ws = {}      # (device, stream, rows) -> zero-initialised reduction workspace


def noise_table(instruments, codes, floor: float = 0.0) -> np.ndarray:
    """``[M, 8]`` fp64: unit, exposure, dn_per_photon, read_noise, extra_var, floor, 0, 0 per row of ``codes``.  ``instruments``
    is one ``Instrument`` for all rows or a mapping from code to ``Instrument``; the rows that share an instrument, in row
    order, are its channels: a per-channel scalar needs one value per such row.  ``extra_var`` is 1 / 12 where the instrument
    quantises."""
    codes = tuple(codes)
    m = len(codes)
    if isinstance(instruments, Instrument):
        per_row = [instruments] * m
    elif isinstance(instruments, Mapping):
        table = {}
        for key, inst in instruments.items():
            if not isinstance(inst, Instrument):
                raise TypeError(f'instruments[{key!r}] is no Instrument')
            table[int(key)] = inst
        missing = [c for c in codes if c not in table]
        if missing:
            raise ValueError(f'codes {missing} have no instrument')
        per_row = [table[c] for c in codes]
    else:
        raise TypeError('instruments must be an Instrument or a mapping from code to Instrument')
    if not floor >= 0.0:
        raise ValueError(f'floor must be >= 0, got {floor}')
    out = np.zeros((m, N_NOISE))
    seen = []
    for inst in per_row:
        if any(inst is s for s in seen):
            continue
        seen.append(inst)
        rows = [i for i, other in enumerate(per_row) if other is inst]
        params = inst.params(len(rows))          # raises when a per-channel scalar cannot be laid onto the rows
        out[rows, :4] = params[:, :4]
        out[rows, 4] = 1.0 / 12.0 if inst.quantise else 0.0
    out[:, 5] = float(floor)
    if not (np.isfinite(out).all() and (out[:, 0] > 0).all() and (out[:, 1] > 0).all() and (out[:, 2] >= 0).all()):
        raise ValueError('unit and exposure must be > 0, dn_per_photon >= 0 and every noise scalar finite')
    dark = out[:, 3] ** 2 + out[:, 4] + out[:, 5] ** 2
    if (dark == 0).any():
        bad = [codes[i] for i in np.nonzero(dark == 0)[0]]
        raise ValueError(f'rows {bad}: read_noise^2 + extra_var + floor^2 is 0, so sigma is 0 on a dark pixel; give the instrument '
                         'a read noise or the likelihood a floor')
    return out


class NoiseLikelihood(nn.Module):
    """``NoiseLikelihood(instruments, codes=None, mode='observed', free=(), gain_rate=1.0, floor=0.0)``.

    ``codes``: a ``ResponseSet``, a sequence of codes, or None for one row (the emission module's channel).  ``free``: the codes
    whose gains train ('all': every row); the gradient of any other row is exactly 0, and with nothing free the module has no
    trainable parameter.  ``log_gain`` [M] is the stored parameter, initialised to 0; the kernel is given ``gain_rate * log_gain``,
    so that the gains can move faster than a network that shares their learning rate.  ``floor``: a standard deviation in image
    units added in quadrature."""

    def __init__(self, instruments, codes=None, mode: str = 'observed', free=(), gain_rate: float = 1.0, floor: float = 0.0):
        super().__init__()
        if mode not in MODES:
            raise ValueError(f"mode must be 'observed' or 'model', got {mode!r}")
        if codes is None:
            row_codes, self.single_row = (1,), True
        else:
            self.single_row = False
            if isinstance(codes, ResponseSet):
                row_codes = codes.codes
            else:
                codes = list(codes)
                if len(codes) > MAX_CHANNELS:
                    raise ValueError(f'a likelihood has 1 .. {MAX_CHANNELS} rows, got {len(codes)}')
                row_codes, _ = as_response_set(codes)
        if not float(gain_rate) > 0.0:
            raise ValueError(f'gain_rate must be > 0, got {gain_rate}')
        self.mode, self.codes, self.gain_rate, self.floor = mode, tuple(row_codes), float(gain_rate), float(floor)
        m = len(self.codes)
        if isinstance(free, str) or free is True:
            if free not in ('all', True):
                raise ValueError(f"free must be a sequence of codes or 'all', got {free!r}")
            mask = np.ones(m, dtype=bool)
        else:
            mask = np.zeros(m, dtype=bool)
            for c in free:
                try:
                    known = float(c) == int(c) and int(c) in self.codes
                except (TypeError, ValueError, OverflowError):
                    known = False
                if self.single_row:
                    raise ValueError("a single-row likelihood frees its gain with free='all'")
                if not known:
                    raise ValueError(f'free code {c!r} is no row of the likelihood ({", ".join(str(k) for k in self.codes)})')
                mask[self.codes.index(int(c))] = True
        table = noise_table(instruments, self.codes, self.floor)
        self.register_buffer('free', torch.from_numpy(mask))
        self.register_buffer('row_codes', torch.tensor(self.codes, dtype=torch.float32))
        self.register_buffer('noise', torch.from_numpy(table))
        self.log_gain = nn.Parameter(torch.zeros(m, dtype=torch.float32), requires_grad=bool(mask.any()))

    @property
    def n_rows(self) -> int:
        return len(self.codes)

    def effective_log_gain(self) -> torch.Tensor:
        """``gain_rate * log_gain``: what the kernel exponentiates (fp32, detached)."""
        return (self.log_gain.detach() * self.gain_rate).contiguous()

    def gains(self) -> torch.Tensor:
        """``exp(gain_rate * log_gain)`` per row (fp64, detached)."""
        return torch.exp(self.effective_log_gain().double())

    def sigma(self, image: torch.Tensor, row: int = 0) -> torch.Tensor:
        """``sqrt(var(image) + floor^2)`` of one row in fp64: the error bar the 'observed' mode gives a target (plain torch)."""
        unit, exposure, g, rn, extra, floor = (float(v) for v in self.noise[row, :6])
        x = torch.as_tensor(image).double()
        return ((x.clamp_min(0.0) * unit * exposure * g + rn * rn + extra) / (unit * exposure) ** 2 + floor * floor).sqrt()

    def reduced_chi2(self, channel_stats: torch.Tensor) -> torch.Tensor:
        """Per row, the sum of the fine terms over the number of valid slots (NaN for a row without any): a reduced chi-square
        in 'observed' mode, the mean negative log-likelihood in 'model' mode."""
        return channel_stats[:, 2] / channel_stats[:, 0]

    def extra_repr(self) -> str:
        return f'rows={self.n_rows}, mode={self.mode!r}, free={int(self.free.sum())}, gain_rate={self.gain_rate}, floor={self.floor}'


def _workspace(dev, n_rows) -> torch.Tensor:
    key = (dev, torch.cuda.current_stream(dev).cuda_stream, n_rows)
    ws = _ws.get(key)
    if ws is None:
        ws = _ws[key] = torch.zeros(_l.load().sunerf_likelihood_workspace_bytes(n_rows), dtype=torch.uint8, device=dev)
    return ws


def launch(coarse, fine, target, codes, row_codes, noise, log_gain, mode, reg, extras, lambda_image, lambda_regularization,
           workspace=None):
    """One call of ``sunerf_likelihood_loss`` on contiguous device tensors: ``(g_coarse, g_fine, g_log_gain, channel_stats,
    stats)``, the gradients as the kernel leaves them (not divided by the number of valid slots)."""
    dev = coarse.device
    n_rays, n_columns = coarse.shape
    m = row_codes.numel()
    n_reg = reg.numel() if reg is not None else 0
    ptrs = (ctypes.c_void_p * max(1, len(extras)))(*[t.data_ptr() for t in extras])
    sizes = (ctypes.c_int64 * max(1, len(extras)))(*[t.numel() for t in extras])
    g_coarse, g_fine = torch.empty_like(coarse), torch.empty_like(fine)
    g_log_gain = torch.empty(m, dtype=torch.float64, device=dev)
    channel_stats = torch.empty((m, 4), dtype=torch.float64, device=dev)
    stats = torch.empty(8, dtype=torch.float32, device=dev)
    ws = _workspace(dev, m) if workspace is None else workspace
    _l.call(dev, 'sunerf_likelihood_loss', _ptr(coarse), _ptr(fine), _ptr(target), _ptr(codes), n_rays, n_columns, _ptr(row_codes),
            _ptr(noise), _ptr(log_gain), m, mode, _ptr(reg), n_reg, ptrs, sizes, len(extras), lambda_image,
            lambda_regularization, _ptr(g_coarse), _ptr(g_fine), _ptr(g_log_gain), _ptr(channel_stats), _ptr(stats), _ptr(ws),
            ws.numel(), _stream(dev))
    return g_coarse, g_fine, g_log_gain, channel_stats, stats


class _LikelihoodLoss(torch.autograd.Function):
    @staticmethod
    def forward(ctx, coarse, fine, target, reg, log_gain, cfg):
        like = cfg['likelihood']
        coarse_c, fine_c = _dev(coarse, 'coarse_image'), _dev(fine, 'fine_image')
        if coarse_c.dim() != 2 or coarse_c.numel() == 0:
            raise ValueError(f'coarse_image must be a non-empty [N, W] tensor, got {tuple(coarse.shape)}')
        if fine.shape != coarse.shape:
            raise ValueError('coarse_image and fine_image differ in shape')
        target_c = _dev(target, 'target_image', coarse.shape)
        codes = cfg['codes']
        codes_c = None if codes is None else _dev(codes.detach(), 'codes', coarse.shape)
        if codes_c is None and not like.single_row:
            raise ValueError('a likelihood with channel codes needs the codes of every slot')
        dev = coarse_c.device
        if like.noise.device != dev:
            raise _l.SunerfHipError(f'the likelihood is on {like.noise.device}, the images on {dev}')
        reg_c = _dev(reg, 'regularization') if reg is not None else None
        n_reg = reg_c.numel() if reg_c is not None else 0
        extras = [_dev(t.detach(), 'finite-check tensor') for t in cfg['finite_check']]
        effective = (log_gain.detach() * like.gain_rate).contiguous()
        g_coarse, g_fine, g_log_gain, channel_stats, stats = launch(
            coarse_c, fine_c, target_c, codes_c, like.row_codes, like.noise, effective, MODES[like.mode], reg_c, extras,
            cfg['lambda_image'], cfg['lambda_regularization'])
        ctx.set_materialize_grads(False)
        ctx.save_for_backward(g_coarse, g_fine, g_log_gain, stats, like.free)
        ctx.lambda_image, ctx.gain_rate = cfg['lambda_image'], like.gain_rate
        ctx.reg_shape = None if reg is None else tuple(reg.shape)
        ctx.reg_grad = cfg['lambda_regularization'] / n_reg if n_reg else 0.0
        ctx.mark_non_differentiable(stats, channel_stats)
        return stats[0], stats, channel_stats

    @staticmethod
    def backward(ctx, g_loss, _g_stats, _g_channel_stats):
        if g_loss is None:
            return None, None, None, None, None, None
        g_coarse, g_fine, g_log_gain, stats, free = ctx.saved_tensors
        # lambda_image / n_valid * g_loss as a device scalar, in fp64: a gradient is rounded to fp32 twice (the kernel's store
        # and the one below), never three times.  No valid slot: every stored gradient is 0 already.
        scale = g_loss.double() * ctx.lambda_image / stats[6].double().clamp_min(1.0)
        grads = [None] * 6
        if ctx.needs_input_grad[0]:
            grads[0] = (g_coarse.double() * scale).float()
        if ctx.needs_input_grad[1]:
            grads[1] = (g_fine.double() * scale).float()
        if ctx.reg_shape is not None and ctx.needs_input_grad[3]:
            grads[3] = (g_loss * ctx.reg_grad).expand(ctx.reg_shape)
        if ctx.needs_input_grad[4]:
            g = g_log_gain * (scale * ctx.gain_rate)
            grads[4] = torch.where(free, g, torch.zeros_like(g)).float()
        return tuple(grads)


def likelihood_loss(coarse_image: torch.Tensor, fine_image: torch.Tensor, target_image: torch.Tensor,
                    regularization: Optional[torch.Tensor], likelihood: NoiseLikelihood, codes: Optional[torch.Tensor] = None,
                    lambda_image: float = 1.0, lambda_regularization: float = 1.0, finite_check: Iterable[torch.Tensor] = ()):
    """``lambda_image * (mean_valid(term(coarse)) + mean_valid(term(fine))) + lambda_regularization * mean(reg)`` with the terms
    of ``likelihood`` (module docstring).  ``codes`` [N, W]: the channel code of every slot (a DT batch's ``wavelength``), None
    for a single-row likelihood.  A slot whose code is <= 0, whose target is not finite or whose code is no row is masked.

    Returns ``(loss, stats, channel_stats)``: ``loss`` a 0-dim tensor differentiable with respect to ``coarse_image``,
    ``fine_image``, ``regularization`` and ``likelihood.log_gain``; ``stats`` 8 device floats (``STAT_KEYS``); ``channel_stats``
    fp64 ``[M, 4]`` (``CHANNEL_STAT_KEYS``).  Nothing is read back to the host."""
    if not isinstance(likelihood, NoiseLikelihood):
        raise TypeError('likelihood must be a NoiseLikelihood')
    cfg = {'likelihood': likelihood, 'codes': codes, 'lambda_image': float(lambda_image),
           'lambda_regularization': float(lambda_regularization), 'finite_check': list(finite_check)}
    if len(cfg['finite_check']) > 8:
        raise ValueError('at most 8 extra tensors can take part in the finite check')
    return _LikelihoodLoss.apply(coarse_image, fine_image, target_image, regularization, likelihood.log_gain, cfg)


def stats_dict(stats: torch.Tensor):
    return {k: stats[i] for i, k in enumerate(STAT_KEYS)}
