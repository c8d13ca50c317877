"""The point-spread function as a trainable part of the instrument (include/sunerf_hip_psf_grad.h, csrc/psf_grad.hip, DESIGN.md
8t): the gradient of the PSF-and-bin correlation with respect to its taps, the parameterisations that sit on top of it and a
calibration against a known scene.

``Instrument`` treats its PSF as a constant.  :class:`FittedInstrument` takes a :class:`TrainablePSF` instead: ``expected`` and
``expected_windows`` are then differentiable with respect to the planes (the adjoint of the correlation, as before) AND to the
parameters of the PSF -- ``sunerf_psf_grad_taps`` gives the gradient of the effective kernel's taps in fp64, and plain torch
carries it through the box of the binning, the flip, the normalisation and the profile (the stamp is tiny: no kernel).  There is
no CPU path for the correlation or its gradients."""
from typing import Optional, Union

import numpy as np
import torch

from . import lib as _l
from ._ffi import _ptr, _stream, _workspace
from .instrument import BOUNDARY, FWHM_PER_SIGMA, MAX_KERNEL, Instrument, _correlate_bin, correlate_bin_adjoint

_WORKSPACES = {}


def tap_gradient(planes: torch.Tensor, g_out: torch.Tensor, n_kernels: int, kh: int, kw: int, bin: int, ay: int, ax: int,
                 scale: float, boundary: int) -> torch.Tensor:
    """``sunerf_psf_grad_taps``: fp64 ``[n_kernels, kh, kw]``, the gradient with respect to the taps of the strided correlation
    that read ``planes`` [n, H, W] (float32, on the device) and whose output has the cotangent ``g_out`` [n, H // bin, W // bin]
    (float32).  Plane ``p`` belongs to kernel ``p % n_kernels``; ``n_kernels`` divides ``n``.  The empty call gives zeros."""
    if not isinstance(planes, torch.Tensor) or not isinstance(g_out, torch.Tensor):
        raise TypeError('tap_gradient: planes and g_out must be torch.Tensors')
    if not planes.is_cuda or g_out.device != planes.device:
        raise _l.SunerfHipError('tap_gradient runs on a ROCm device (there is no CPU path); planes and g_out share it')
    if planes.dim() != 3 or planes.dtype != torch.float32:
        raise ValueError(f'tap_gradient: planes must be float32 [n, H, W], got {planes.dtype} {tuple(planes.shape)}')
    n, h, w = planes.shape
    n_kernels, kh, kw, bin = int(n_kernels), int(kh), int(kw), int(bin)
    if kh < 1 or kw < 1 or bin < 1 or n_kernels < 1 or n % n_kernels:
        raise ValueError(f'tap_gradient: kh, kw, bin must be >= 1 and n_kernels divide the {n} planes, got {kh}, {kw}, {bin}, {n_kernels}')
    if tuple(g_out.shape) != (n, h // bin, w // bin) or g_out.dtype != torch.float32:
        raise ValueError(f'tap_gradient: g_out must be float32 [{n}, {h // bin}, {w // bin}], got {g_out.dtype} {tuple(g_out.shape)}')
    dev = planes.device
    if g_out.numel() == 0:          # the empty call writes nothing: no detector pixel, no gradient
        return torch.zeros((n_kernels, kh, kw), dtype=torch.float64, device=dev)
    planes, g_out = planes.contiguous(), g_out.contiguous()
    g_taps = torch.empty((n_kernels, kh, kw), dtype=torch.float64, device=dev)
    with torch.cuda.device(dev):
        nbytes = int(_l.load().sunerf_psf_grad_workspace_bytes(n, h, w, n_kernels, kh, kw, bin))
    ws = _workspace(_WORKSPACES, dev, max(nbytes, 8))
    _l.call(dev, 'sunerf_psf_grad_taps', _ptr(planes), _ptr(g_out), n, h, w, n_kernels, kh, kw, bin, int(ay), int(ax), float(scale),
            int(boundary), _ptr(g_taps), _ptr(ws), _stream(dev))
    return g_taps


def _per_channel(value, channels, name):
    v = np.atleast_1d(np.asarray(value, dtype=np.float64))
    if v.ndim != 1 or v.size == 0 or not (v > 0).all():
        raise ValueError(f'{name} must be a positive scalar or one positive value per channel, got {value!r}')
    if channels is not None:
        if v.size not in (1, int(channels)):
            raise ValueError(f'{name} has {v.size} values, channels = {channels}')
        v = np.broadcast_to(v, (int(channels),)).copy()
    return v


class TrainablePSF(torch.nn.Module):
    """A point-spread function with trainable parameters: :meth:`gaussian`, :meth:`moffat` or :meth:`free`.  The parameters are
    float32 (what ``ClipAdam`` takes); ``rate`` multiplies the stored parameter as ``gain_rate`` does in ``NoiseLikelihood``, so
    that the one learning rate of the optimiser serves the network and the PSF.  The stamp is formed in fp64."""

    def __init__(self, kind: str, shape, rate: float = 1.0):
        super().__init__()
        if not float(rate) > 0.0:
            raise ValueError(f'rate must be > 0, got {rate}')
        self.kind, self.rate = kind, float(rate)
        self.kh, self.kw = int(shape[0]), int(shape[1])
        if max(self.kh, self.kw) > MAX_KERNEL:
            raise ValueError(f'a stamp of {self.kh} x {self.kw} exceeds {MAX_KERNEL} taps per axis')

    @classmethod
    def gaussian(cls, fwhm, radius: int, channels: Optional[int] = None, rate: float = 1.0) -> 'TrainablePSF':
        """The formula of ``gaussian_psf``; ``log_fwhm`` [n] is the parameter, n = 1 (a scalar ``fwhm`` and no ``channels``: a
        shared PSF) or one per channel."""
        radius = int(radius)
        if radius < 0:
            raise ValueError(f'radius must be >= 0, got {radius}')
        self = cls('gaussian', (2 * radius + 1, 2 * radius + 1), rate)
        self.radius = radius
        f = _per_channel(fwhm, channels, 'fwhm')
        self.log_fwhm = torch.nn.Parameter(torch.as_tensor(np.log(f) / self.rate, dtype=torch.float32))
        return self

    @classmethod
    def moffat(cls, fwhm, beta, radius: int, channels: Optional[int] = None, rate: float = 1.0, train_beta: bool = False) -> 'TrainablePSF':
        """The formula of ``moffat_psf``; ``log_fwhm`` [n] is the parameter and, with ``train_beta``, ``log_beta`` [n] as well
        (it is kept as a frozen parameter otherwise)."""
        radius = int(radius)
        if radius < 0:
            raise ValueError(f'radius must be >= 0, got {radius}')
        self = cls('moffat', (2 * radius + 1, 2 * radius + 1), rate)
        self.radius = radius
        f = _per_channel(fwhm, channels, 'fwhm')
        b = _per_channel(beta, len(f) if len(f) > 1 else channels, 'beta')
        if len(b) != len(f):
            f = np.broadcast_to(f, b.shape).copy()
        self.log_fwhm = torch.nn.Parameter(torch.as_tensor(np.log(f) / self.rate, dtype=torch.float32))
        self.log_beta = torch.nn.Parameter(torch.as_tensor(np.log(b) / self.rate, dtype=torch.float32), requires_grad=bool(train_beta))
        return self

    @classmethod
    def free(cls, stamp, rate: float = 1.0) -> 'TrainablePSF':
        """One logit per tap; the stamp is the softmax of ``rate * logits``: non-negative taps that sum to 1.  ``stamp``
        ``(kh, kw)`` or ``(C, kh, kw)`` is the start (normalised; a tap of 0 starts at 1e-30 of the sum)."""
        s = np.asarray(stamp.detach().cpu().numpy() if isinstance(stamp, torch.Tensor) else stamp, dtype=np.float64)
        if s.ndim == 2:
            s = s[None]
        if s.ndim != 3 or 0 in s.shape or not (s >= 0).all() or not (s.sum(axis=(1, 2)) > 0).all():
            raise ValueError('free: stamp must be (kh, kw) or (C, kh, kw), non-negative, with a positive sum')
        self = cls('free', s.shape[1:], rate)
        s = np.maximum(s / s.sum(axis=(1, 2), keepdims=True), 1e-30)
        self.logits = torch.nn.Parameter(torch.as_tensor(np.log(s) / self.rate, dtype=torch.float32))
        return self

    @property
    def n(self) -> int:
        return int((self.logits if self.kind == 'free' else self.log_fwhm).shape[0])

    @property
    def fwhm(self):
        """``exp(rate * log_fwhm)`` [n] (fp64, detached); None for a free-form PSF."""
        if self.kind == 'free':
            return None
        return torch.exp(self.log_fwhm.detach().double() * self.rate)

    @property
    def beta(self):
        return torch.exp(self.log_beta.detach().double() * self.rate) if self.kind == 'moffat' else None

    def stamp(self) -> torch.Tensor:
        """fp64 ``[n, kh, kw]`` on the parameters' device, differentiable by plain torch."""
        if self.kind == 'free':
            z = self.logits.double() * self.rate
            return torch.softmax(z.reshape(z.shape[0], -1), dim=1).reshape(z.shape)
        dev = self.log_fwhm.device
        ax = torch.arange(-self.radius, self.radius + 1, dtype=torch.float64, device=dev)
        r2 = (ax[:, None] ** 2 + ax[None, :] ** 2)[None]
        fwhm = torch.exp(self.log_fwhm.double() * self.rate)[:, None, None]
        if self.kind == 'gaussian':
            sigma = fwhm / FWHM_PER_SIGMA
            k = torch.exp(-r2 / (2.0 * sigma * sigma))
        else:
            beta = torch.exp(self.log_beta.double() * self.rate)[:, None, None]
            alpha = fwhm / (2.0 * torch.sqrt(2.0 ** (1.0 / beta) - 1.0))
            k = (1.0 + r2 / (alpha * alpha)) ** -beta
        return k / k.sum(dim=(1, 2), keepdim=True)

    def numpy(self) -> np.ndarray:
        """The current stamp as ``Instrument(psf=...)`` takes it: ``(kh, kw)`` for a shared PSF, ``(C, kh, kw)`` per channel."""
        s = self.stamp().detach().cpu().numpy()
        return s[0] if s.shape[0] == 1 else s

    def extra_repr(self):
        return f'{self.kind}, n={self.n}, stamp={self.kh}x{self.kw}, rate={self.rate}'


def effective_kernel_of(stamp: torch.Tensor, bin: int) -> torch.Tensor:
    """``Instrument.effective_kernel`` in torch, on the stamp's device: the flipped stamp [n, kh, kw] summed over the
    ``bin x bin`` box, [n, kh + bin - 1, kw + bin - 1], the additions in that method's order (``dy`` then ``dx``) so that the
    bits agree.  Differentiable."""
    b = int(bin)
    flipped = torch.flip(stamp, dims=(1, 2))
    K = torch.zeros((stamp.shape[0], stamp.shape[1] + b - 1, stamp.shape[2] + b - 1), dtype=stamp.dtype, device=stamp.device)
    for dy in range(b):
        for dx in range(b):
            K = K + torch.nn.functional.pad(flipped, (dx, b - 1 - dx, dy, b - 1 - dy))
    return K


class _CorrelateBinTaps(torch.autograd.Function):
    """The strided correlation with both of its gradients: the adjoint for the planes, ``sunerf_psf_grad_taps`` for the taps,
    each produced only when it is needed.  ``taps`` [n_taps, kh, kw] fp64 is what is differentiated; ``grad_kernels`` says how
    the planes share it (plane p takes kernel p % grad_kernels), while the forward call takes the taps as ``forward_taps``,
    expanded to one kernel per plane where the forward needs that."""

    @staticmethod
    def forward(ctx, planes, taps, forward_taps, n_kernels, kh, kw, bin_factor, ay, ax, scale, boundary):
        ctx.call = (forward_taps, n_kernels, kh, kw, bin_factor, ay, ax, scale, boundary)
        ctx.frame, ctx.grad_kernels = tuple(planes.shape[1:]), taps.shape[0]
        ctx.save_for_backward(planes)
        return _correlate_bin(planes, *ctx.call)

    @staticmethod
    def backward(ctx, g):
        planes, = ctx.saved_tensors
        g = g.to(torch.float32).contiguous()
        g_planes = g_taps = None
        if ctx.needs_input_grad[0]:
            g_planes = correlate_bin_adjoint(g, *ctx.frame, *ctx.call)
        if ctx.needs_input_grad[1]:
            _, _, kh, kw, bin_factor, ay, ax, scale, boundary = ctx.call
            g_taps = tap_gradient(planes, g, ctx.grad_kernels, kh, kw, bin_factor, ay, ax, scale, boundary)
        return (g_planes, g_taps) + (None,) * 9


class FittedInstrument(Instrument):
    """An :class:`Instrument` whose PSF is a :class:`TrainablePSF`: ``FittedInstrument(psf_model, bin=..., unit=..., ...)``.
    ``psf`` is the current stamp; its size is fixed, so ``effective_kernel``, ``window_shape``, ``noise``, ``errors`` and
    ``deconvolve`` work unchanged and see the current PSF.  ``expected`` and ``expected_windows`` are differentiable with respect
    to the planes and to the parameters of ``psf_model``; they build the effective kernel on the device from ``stamp()`` at every
    call and never read the per-stream tap cache, which would serve stale taps."""

    def __init__(self, psf_model: TrainablePSF, **kw):
        if not isinstance(psf_model, TrainablePSF):
            raise TypeError('FittedInstrument: psf_model must be a TrainablePSF')
        if 'psf' in kw:
            raise TypeError('FittedInstrument takes its psf from psf_model')
        self.psf_model = psf_model
        super().__init__(psf=None, **kw)
        if max(psf_model.kh, psf_model.kw) + self.bin - 1 > MAX_KERNEL:
            raise ValueError(f'psf {(psf_model.kh, psf_model.kw)} with bin {self.bin}: the effective kernel exceeds {MAX_KERNEL} taps per axis')

    @property
    def psf(self) -> np.ndarray:
        return self.psf_model.numpy()

    @psf.setter
    def psf(self, value):
        if value is not None:
            raise AttributeError('the psf of a FittedInstrument is its psf_model')

    def freeze(self) -> Instrument:
        """A plain ``Instrument`` with the current stamp and this instrument's settings."""
        scalars = {name: getattr(self, name) for name in ('unit', 'exposure', 'dn_per_photon', 'read_noise', 'pedestal', 'saturation')}
        return Instrument(psf=self.psf, bin=self.bin, bin_mode=self.bin_mode, boundary=self.boundary, quantise=self.quantise, **scalars)

    def _taps(self, K: np.ndarray, dev, repeat: int = 1) -> torch.Tensor:
        """``K`` on the device, never cached: the PSF may have moved since the last call."""
        taps = torch.as_tensor(K, dtype=torch.float64).contiguous().to(dev)
        return taps if repeat == 1 else taps.repeat(repeat, 1, 1).contiguous()

    def _device_taps(self, dev) -> torch.Tensor:
        stamp = self.psf_model.stamp()
        if stamp.device != dev:
            raise ValueError(f'the psf_model is on {stamp.device}, the planes on {dev}')
        return effective_kernel_of(stamp, self.bin).contiguous()

    def _correlate(self, planes, taps, repeat, ay, ax, boundary):
        n_taps, kh, kw = taps.shape
        forward_taps = taps.detach()
        if repeat > 1:
            forward_taps = forward_taps.repeat(repeat, 1, 1).contiguous()
        call = (forward_taps, forward_taps.shape[0], kh, kw, self.bin, ay, ax, self.scale, boundary)
        if torch.is_grad_enabled() and (planes.requires_grad or taps.requires_grad):
            return _CorrelateBinTaps.apply(planes, taps, *call)
        return _correlate_bin(planes, *call)

    def expected(self, planes: torch.Tensor) -> torch.Tensor:
        """``Instrument.expected`` with the current PSF, differentiable with respect to ``planes`` and to the PSF's parameters."""
        planes = self._planes(planes, 'FittedInstrument.expected')
        c = planes.shape[0]
        taps = self._device_taps(planes.device)
        if taps.shape[0] not in (1, c):
            raise ValueError(f'the psf has {taps.shape[0]} channels, the frame {c}')
        return self._correlate(planes, taps, 1, self.psf_model.kh // 2, self.psf_model.kw // 2, BOUNDARY[self.boundary])

    def expected_windows(self, windows: torch.Tensor) -> torch.Tensor:
        """``Instrument.expected_windows`` with the current PSF, differentiable with respect to ``windows`` and to the PSF's
        parameters.  A per-channel PSF is expanded to one kernel per plane for the forward and the adjoint; the tap gradient
        takes the ``[n, C]`` layout as it is (``n_kernels = C``)."""
        if not isinstance(windows, torch.Tensor):
            raise TypeError('FittedInstrument.expected_windows: windows must be a torch.Tensor')
        if not windows.is_cuda:
            raise _l.SunerfHipError('FittedInstrument.expected_windows runs on a ROCm device (there is no CPU path)')
        if windows.dim() != 4 or windows.dtype != torch.float32:
            raise ValueError(f'FittedInstrument.expected_windows: windows must be float32 [n, C, hw, ww], got {windows.dtype} '
                             f'{tuple(windows.shape)}')
        n, c, hw, ww = windows.shape
        b = self.bin
        kh, kw = self.psf_model.kh + b - 1, self.psf_model.kw + b - 1
        if self.psf_model.n not in (1, c):
            raise ValueError(f'the psf has {self.psf_model.n} channels, the windows {c}')
        if hw < kh or ww < kw or (hw - kh) % b or (ww - kw) % b or (hw - kh) // b != (ww - kw) // b:
            raise ValueError(f'windows of {hw} x {ww} sub-pixels are no ((P - 1) {b} + {kh}) x ((P - 1) {b} + {kw}) window of a '
                             'P x P patch')
        p = (hw - kh) // b + 1
        if n == 0:
            return windows.new_zeros((0, c, p, p))
        taps = self._device_taps(windows.device)
        planes = windows.contiguous().view(n * c, hw, ww)
        out = self._correlate(planes, taps, n if taps.shape[0] > 1 else 1, 0, 0, BOUNDARY['zero'])
        return out[:, :p, :p].reshape(n, c, p, p)


def fit_psf(instrument: FittedInstrument, sharp: torch.Tensor, observed: torch.Tensor, steps: int = 200, lr: float = 0.05,
            sigma: Union[None, float, torch.Tensor] = None) -> dict:
    """Calibration without a network: Adam on the parameters of ``instrument.psf_model`` through ``instrument.expected(sharp)``
    against ``observed`` -- a lunar transit, or a sharper instrument's image of the same scene.  The loss is the mean square of
    the residual, or of ``residual / sigma`` (a chi-square per pixel) where ``sigma`` is given.  Returns ``loss`` (the history,
    fp64 [steps]), ``fwhm`` (fp64 [n]; None for a free-form PSF) and ``stamp`` (the fitted stamp, NumPy)."""
    if not isinstance(instrument, FittedInstrument):
        raise TypeError('fit_psf: instrument must be a FittedInstrument')
    params = [p for p in instrument.psf_model.parameters() if p.requires_grad]
    if not params:
        raise ValueError('fit_psf: the psf_model has no parameter that requires a gradient')
    sharp = instrument._planes(sharp, 'fit_psf').detach()
    observed = instrument._planes(observed, 'fit_psf').detach().double()
    weight = None if sigma is None else 1.0 / torch.as_tensor(sigma, device=observed.device).double()
    optimiser = torch.optim.Adam(params, lr=lr)
    history = []
    for _ in range(int(steps)):
        optimiser.zero_grad(set_to_none=True)
        residual = instrument.expected(sharp).double() - observed
        if weight is not None:
            residual = residual * weight
        loss = (residual * residual).mean()
        loss.backward()
        optimiser.step()
        history.append(loss.detach())
    loss = torch.stack(history).cpu() if history else torch.zeros(0, dtype=torch.float64)
    fwhm = instrument.psf_model.fwhm
    return {'loss': loss, 'fwhm': None if fwhm is None else fwhm.cpu(), 'stamp': instrument.psf_model.numpy()}
