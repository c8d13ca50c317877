"""A render observed through an instrument (include/sunerf_hip_instrument.h): correlation with the point-spread
function, summation of ``bin x bin`` sub-pixels into detector pixels, photon and read noise, digitisation, saturation -- the way
from a noise-free pinhole render back to what a detector would have recorded, and the error model (``sigma``) that goes with it.

The PSF and the box of the binning are folded into ONE kernel on the host (:meth:`Instrument.effective_kernel`), so a detector
pixel costs ``(k + bin - 1)^2`` multiply-adds and not ``bin^2 k^2``; the device runs one strided correlation
(``sunerf_instrument_correlate_bin``) and one per-element noise kernel (``sunerf_instrument_noise``) whose randomness is the
counter-based Philox4x32-10 of the header: an element's draw depends on the seed and on its index alone, so tiles, ranks and
reruns agree by bits.  There is no CPU path for either; :meth:`Instrument.errors` and the kernel builders are plain host code.

Units: ``unit`` photons-per-second-per-pixel per image unit (what one unit of the render is worth at the detector), ``exposure``
seconds, ``dn_per_photon`` the gain, ``read_noise``, ``pedestal`` and ``saturation`` in DN.  Images go in and come out in image units."""
import ctypes
import math
from typing import Sequence, Tuple, Union

import numpy as np
import torch

from . import lib as _l
from ._ffi import _ptr, _stream

MAX_KERNEL, MAX_BIN = 96, 8                      # include/sunerf_hip_instrument.h
BOUNDARY = {'zero': 0, 'nearest': 1}
POISSON, READ, QUANTISE, SATURATE = 1, 2, 4, 8
N_PARAMS = 8
FWHM_PER_SIGMA = 2.0 * math.sqrt(2.0 * math.log(2.0))
_SCALARS = ('unit', 'exposure', 'dn_per_photon', 'read_noise', 'pedestal', 'saturation')


def _radial_grid(radius: int):
    radius = int(radius)
    if radius < 0:
        raise ValueError(f'radius must be >= 0, got {radius}')
    ax = np.arange(-radius, radius + 1, dtype=np.float64)
    return ax[:, None] ** 2 + ax[None, :] ** 2


def gaussian_psf(fwhm: float, radius: int) -> np.ndarray:
    """A Gaussian of full width at half maximum ``fwhm`` (pixels of the rendered grid) sampled at the pixel centres of a
    ``(2 radius + 1)^2`` stamp, fp64, normalised to sum to 1."""
    if not fwhm > 0:
        raise ValueError(f'fwhm must be > 0, got {fwhm}')
    sigma = float(fwhm) / FWHM_PER_SIGMA
    k = np.exp(-_radial_grid(radius) / (2.0 * sigma * sigma))
    return k / k.sum()


def moffat_psf(fwhm: float, beta: float, radius: int) -> np.ndarray:
    """A Moffat profile ``(1 + r^2 / alpha^2)^-beta`` of full width at half maximum ``fwhm`` (pixels of the rendered grid), fp64,
    on a ``(2 radius + 1)^2`` stamp, normalised to sum to 1."""
    if not fwhm > 0 or not beta > 0:
        raise ValueError(f'fwhm and beta must be > 0, got {fwhm}, {beta}')
    alpha = float(fwhm) / (2.0 * math.sqrt(2.0 ** (1.0 / float(beta)) - 1.0))
    k = (1.0 + _radial_grid(radius) / (alpha * alpha)) ** -float(beta)
    return k / k.sum()


Scalar = Union[float, Sequence[float]]


class Instrument:
    """The forward model of a detector.  ``psf``: ``(kh, kw)`` or per channel ``(C, kh, kw)``, its centre at index
    ``((kh - 1) // 2, (kw - 1) // 2)`` (``scipy.signal.convolve2d(mode='same')``'s); None: no blur.  ``bin``: sub-pixels per
    detector pixel and axis, ``bin_mode`` their 'mean' (an intensity) or 'sum' (a flux).  ``boundary``: what the PSF reads past
    the frame's edge, the 'nearest' pixel or 'zero'.  Every scalar may be one value or one per channel."""

    def __init__(self, psf=None, bin: int = 1, bin_mode: str = 'mean', boundary: str = 'nearest', unit: Scalar = 1.,
                 exposure: Scalar = 1., dn_per_photon: Scalar = 1., read_noise: Scalar = 0., pedestal: Scalar = 0.,
                 saturation: Scalar = math.inf, quantise: bool = False):
        if bin_mode not in ('mean', 'sum'):
            raise ValueError(f"bin_mode must be 'mean' or 'sum', got {bin_mode!r}")
        if boundary not in BOUNDARY:
            raise ValueError(f"boundary must be 'nearest' or 'zero', got {boundary!r}")
        if int(bin) != bin or not 1 <= int(bin) <= MAX_BIN:
            raise ValueError(f'bin must be an integer in 1 .. {MAX_BIN}, got {bin}')
        self.bin, self.bin_mode, self.boundary, self.quantise = int(bin), bin_mode, boundary, bool(quantise)
        self.psf = None
        if psf is not None:
            psf = np.asarray(psf.detach().cpu().numpy() if isinstance(psf, torch.Tensor) else psf, dtype=np.float64)
            if psf.ndim not in (2, 3) or 0 in psf.shape:
                raise ValueError(f'psf must be (kh, kw) or (C, kh, kw), got {psf.shape}')
            if max(psf.shape[-2:]) + self.bin - 1 > MAX_KERNEL:
                raise ValueError(f'psf {psf.shape[-2:]} with bin {self.bin}: the effective kernel exceeds {MAX_KERNEL} taps per axis')
            self.psf = psf
        for name, value in zip(_SCALARS, (unit, exposure, dn_per_photon, read_noise, pedestal, saturation)):
            v = np.asarray(value, dtype=np.float64)
            if v.ndim > 1:
                raise ValueError(f'{name} must be a scalar or one value per channel')
            setattr(self, name, v)
        self._device_kernels = {}

    # ---- host side ----------------------------------------------------------------------------------------------------------
    @classmethod
    def from_spec(cls, spec: str) -> 'Instrument':
        """``'fwhm=2.5,bin=2,exposure=2.9,dn_per_photon=1.2,read_noise=1.2,unit=40'``: a Gaussian PSF of that FWHM (``beta=``
        makes it a Moffat; ``radius=`` its half-size, default ceil(3 fwhm) for a Gaussian, ceil(4 fwhm) for a Moffat) and the
        constructor's scalars; ``quantise=1``, ``bin_mode=sum``, ``boundary=zero`` as named."""
        fields = {}
        for item in filter(None, (s.strip() for s in spec.split(','))):
            key, sep, value = item.partition('=')
            if not sep:
                raise ValueError(f'instrument spec: {item!r} is not key=value')
            fields[key.strip()] = value.strip()
        kw = {}
        fwhm, beta, radius = fields.pop('fwhm', None), fields.pop('beta', None), fields.pop('radius', None)
        if fwhm is not None:
            fwhm = float(fwhm)
            if beta is None:
                kw['psf'] = gaussian_psf(fwhm, int(radius) if radius is not None else math.ceil(3 * fwhm))
            else:
                kw['psf'] = moffat_psf(fwhm, float(beta), int(radius) if radius is not None else math.ceil(4 * fwhm))
        elif beta is not None or radius is not None:
            raise ValueError('instrument spec: beta / radius need fwhm')
        for key, value in fields.items():
            if key in _SCALARS:
                kw[key] = float(value)
            elif key == 'bin':
                kw[key] = int(value)
            elif key in ('bin_mode', 'boundary'):
                kw[key] = value
            elif key == 'quantise':
                kw[key] = value.lower() in ('1', 'true', 'yes')
            else:
                raise ValueError(f'instrument spec: unknown key {key!r}')
        return cls(**kw)

    def effective_kernel(self) -> Tuple[np.ndarray, Tuple[int, int]]:
        """``(K, (anchor_y, anchor_x))``, ``K`` fp64 ``(n, kh + bin - 1, kw + bin - 1)`` with n = 1 or C: the flipped PSF
        convolved with the ``bin x bin`` box of ones, so that the blurred and summed detector pixel (R, C) is
        ``sum_ij K[i, j] in[R bin + i - anchor_y, C bin + j - anchor_x]``; the 'mean' of ``bin_mode`` is the ``scale`` of the
        device call, not part of ``K``."""
        psf = np.ones((1, 1, 1)) if self.psf is None else (self.psf[None] if self.psf.ndim == 2 else self.psf)
        n, kh, kw = psf.shape
        b = self.bin
        flipped = psf[:, ::-1, ::-1]
        K = np.zeros((n, kh + b - 1, kw + b - 1))
        for dy in range(b):
            for dx in range(b):
                K[:, dy:dy + kh, dx:dx + kw] += flipped
        return K, (kh // 2, kw // 2)          # kh - 1 - (kh - 1) // 2

    @property
    def scale(self) -> float:
        return 1.0 / (self.bin * self.bin) if self.bin_mode == 'mean' else 1.0

    def params(self, n_channels: int) -> np.ndarray:
        """``[C, 8]`` fp64: unit, exposure, dn_per_photon, read_noise, pedestal, saturation, 0, 0 per channel."""
        out = np.zeros((n_channels, N_PARAMS))
        for k, name in enumerate(_SCALARS):
            v = getattr(self, name)
            if v.ndim == 1 and v.shape[0] != n_channels:
                raise ValueError(f'{name} has {v.shape[0]} values, the frame {n_channels} channels')
            out[:, k] = v
        return out

    def detector_grid(self, grid: dict) -> dict:
        """The plate-scale dict of the binned frame of a rendered frame ``grid`` (``shape``, ``cdelt``, optional ``crpix`` /
        ``crval``): ``bin`` times the pixel size, the reference pixel moved with the field of view (the rule of
        ``sunerf.evaluation.loader.linear_plate_scale_axes``), trailing rows and columns that fill no detector pixel dropped."""
        h, w = grid['shape']
        b = self.bin
        cdx, cdy = grid['cdelt']
        cpx, cpy = grid.get('crpix', ((w + 1) / 2., (h + 1) / 2.))
        out = {k: v for k, v in grid.items() if k not in ('shape', 'cdelt', 'crpix')}
        out.update(shape=(h // b, w // b), cdelt=(cdx * b, cdy * b), crpix=((cpx - 0.5) / b + 0.5, (cpy - 0.5) / b + 0.5))
        return out

    def latent_grid(self, grid: dict) -> dict:
        """The inverse of :meth:`detector_grid`: the plate-scale dict of the ``bin``-times-finer frame whose binning is the
        detector frame ``grid`` -- the frame of a deconvolved view (:meth:`deconvolve`), which is added with
        ``ObservationSet.add_view(..., grid=latent_grid(grid))``."""
        h, w = grid['shape']
        b = self.bin
        cdx, cdy = grid['cdelt']
        cpx, cpy = grid.get('crpix', ((w + 1) / 2., (h + 1) / 2.))
        out = {k: v for k, v in grid.items() if k not in ('shape', 'cdelt', 'crpix')}
        out.update(shape=(h * b, w * b), cdelt=(cdx / b, cdy / b), crpix=((cpx - 0.5) * b + 0.5, (cpy - 0.5) * b + 0.5))
        return out

    def errors(self, image, channel_axis: int = -1):
        """The ``sigma`` of an OBSERVED image (image units, any device, plain torch): the sigma formula of :meth:`observe` with
        the photon count estimated from the image itself, ``lam = max(dn - pedestal, 0) / dn_per_photon``.  Same shape as
        ``image`` -- ``(..., M)`` with the channels last is what ``invert_dem(errors=...)`` takes; per-channel scalars are laid
        along ``channel_axis`` (0 for planes)."""
        image = torch.as_tensor(image)
        x = image.double()

        def s(name):
            v = getattr(self, name)
            if v.ndim == 0:
                return float(v)
            if x.dim() == 0 or x.shape[channel_axis] != v.shape[0]:
                raise ValueError(f'{name} has {v.shape[0]} values, the image {tuple(x.shape)} along axis {channel_axis}')
            shape = [1] * x.dim()
            shape[channel_axis] = v.shape[0]
            return torch.as_tensor(v, device=x.device).view(shape)
        unit, exposure, g, rn = s('unit'), s('exposure'), s('dn_per_photon'), s('read_noise')
        signal = (x * unit * exposure).clamp_min(0.0)          # dn - pedestal
        lam = signal / g
        var = lam * (g * g) + rn * rn + (1.0 / 12.0 if self.quantise else 0.0)
        return (var.sqrt() / exposure / unit).to(torch.float32)

    # ---- device side --------------------------------------------------------------------------------------------------------
    def _planes(self, planes, what):
        if not isinstance(planes, torch.Tensor):
            raise TypeError(f'{what}: planes must be a torch.Tensor')
        if not planes.is_cuda:
            raise _l.SunerfHipError(f'{what} runs on a ROCm device (there is no CPU path)')
        if planes.dim() == 2:
            planes = planes[None]
        if planes.dim() != 3 or planes.dtype != torch.float32:
            raise ValueError(f'{what}: planes must be float32 [C, H, W], got {planes.dtype} {tuple(planes.shape)}')
        return planes.contiguous()

    def _taps(self, K: np.ndarray, dev, repeat: int = 1) -> torch.Tensor:
        """``K`` on the device (fp64), ``repeat`` copies of its kernels in a row; kept per device and stream."""
        key = (dev, torch.cuda.current_stream(dev).cuda_stream) if repeat == 1 else \
            (dev, torch.cuda.current_stream(dev).cuda_stream, repeat)
        if key not in self._device_kernels:
            taps = torch.as_tensor(K, dtype=torch.float64).contiguous().to(dev)
            self._device_kernels[key] = taps if repeat == 1 else taps.repeat(repeat, 1, 1).contiguous()
        return self._device_kernels[key]

    def expected(self, planes: torch.Tensor) -> torch.Tensor:
        """``[C, H // bin, W // bin]`` float32: ``planes`` [C, H, W] blurred by the PSF and binned, noise-free.  Differentiable
        with respect to ``planes``: the backward is ``sunerf_patch_correlate_bin_adjoint`` with the same kernel, anchor, scale
        and boundary (the PSF itself takes no gradient)."""
        planes = self._planes(planes, 'Instrument.expected')
        c = planes.shape[0]
        K, (ay, ax) = self.effective_kernel()
        if K.shape[0] not in (1, c):
            raise ValueError(f'the psf has {K.shape[0]} channels, the frame {c}')
        call = (self._taps(K, planes.device), K.shape[0], K.shape[1], K.shape[2], self.bin, ay, ax, self.scale,
                BOUNDARY[self.boundary])
        if torch.is_grad_enabled() and planes.requires_grad:
            return _CorrelateBin.apply(planes, *call)
        return _correlate_bin(planes, *call)

    def window_shape(self, patch: int) -> Tuple[int, int]:
        """``(hw, ww)``: the sub-pixels a patch of ``patch x patch`` detector pixels reads, halo included."""
        K, _ = self.effective_kernel()
        return (int(patch) - 1) * self.bin + K.shape[1], (int(patch) - 1) * self.bin + K.shape[2]

    def expected_windows(self, windows: torch.Tensor) -> torch.Tensor:
        """``[n, C, P, P]`` float32: the VALID correlation of ``windows`` [n, C, hw, ww] that carry their full halo,
        ``(hw, ww) = window_shape(P)`` -- detector pixel (r, c) of a window reads its sub-pixels
        ``[r bin, r bin + kh) x [c bin, c bin + kw)`` and nothing past its edge, so no boundary rule takes part.
        Differentiable with respect to ``windows``.  The forward correlation with anchor (0, 0) over the ``n C`` planes; its
        surplus output rows and columns (those whose taps leave the window) are cropped and take no gradient.  A per-channel
        PSF is expanded to one kernel per plane."""
        if not isinstance(windows, torch.Tensor):
            raise TypeError('Instrument.expected_windows: windows must be a torch.Tensor')
        if not windows.is_cuda:
            raise _l.SunerfHipError('Instrument.expected_windows runs on a ROCm device (there is no CPU path)')
        if windows.dim() != 4 or windows.dtype != torch.float32:
            raise ValueError(f'Instrument.expected_windows: windows must be float32 [n, C, hw, ww], got {windows.dtype} '
                             f'{tuple(windows.shape)}')
        n, c, hw, ww = windows.shape
        K, _ = self.effective_kernel()
        if K.shape[0] not in (1, c):
            raise ValueError(f'the psf has {K.shape[0]} channels, the windows {c}')
        kh, kw = K.shape[1:]
        b = self.bin
        if hw < kh or ww < kw or (hw - kh) % b or (ww - kw) % b or (hw - kh) // b != (ww - kw) // b:
            raise ValueError(f'windows of {hw} x {ww} sub-pixels are no ((P - 1) {b} + {kh}) x ((P - 1) {b} + {kw}) window of a '
                             'P x P patch')
        p = (hw - kh) // b + 1
        if n == 0:
            return windows.new_zeros((0, c, p, p))
        per_plane = K.shape[0] > 1
        call = (self._taps(K, windows.device, n if per_plane else 1), n * c if per_plane else 1, kh, kw, b, 0, 0, self.scale,
                BOUNDARY['zero'])
        planes = windows.contiguous().view(n * c, hw, ww)
        if torch.is_grad_enabled() and planes.requires_grad:
            out = _CorrelateBin.apply(planes, *call)
        else:
            out = _correlate_bin(planes, *call)
        return out[:, :p, :p].reshape(n, c, p, p)

    def flags(self, poisson: bool = True, read: bool = True) -> int:
        saturate = bool(np.isfinite(self.saturation).any())
        return (POISSON if poisson else 0) | (READ if read else 0) | (QUANTISE if self.quantise else 0) | (SATURATE if saturate else 0)

    def noise(self, expected: torch.Tensor, seed: int, index_offset: int = 0, poisson: bool = True, read: bool = True,
              want_sigma: bool = True, want_saturated: bool = True):
        """The noise stage alone on ``expected`` [C, H, W] (image units): ``(image, sigma, saturated)``; element (c, r, k) draws
        with the counter ``index_offset + (c H + r) W + k``."""
        expected = self._planes(expected, 'Instrument.noise')
        c, h, w = expected.shape
        dev = expected.device
        if not 0 <= int(seed) < 1 << 64 or int(index_offset) < 0:
            raise ValueError('seed must fit 64 bits and index_offset be >= 0')
        params = torch.as_tensor(self.params(c), dtype=torch.float64).to(dev)
        image = torch.empty_like(expected)
        sigma = torch.empty_like(expected) if want_sigma else None
        saturated = torch.empty(expected.shape, dtype=torch.uint8, device=dev) if want_saturated else None
        _l.call(dev, 'sunerf_instrument_noise', _ptr(expected), c, h, w, _ptr(params), ctypes.c_uint64(int(seed)), int(index_offset),
                self.flags(poisson, read), _ptr(image), _ptr(sigma), _ptr(saturated), _stream(dev))
        return image, sigma, saturated

    def observe(self, planes: torch.Tensor, seed: int, index_offset: int = 0, poisson: bool = True, read: bool = True) -> dict:
        """``planes`` [C, H, W] seen through the instrument: ``expected`` (blurred, binned, noise-free), ``image`` (one noisy
        realisation of it, image units), ``sigma`` (its standard deviation from the expected count) and ``saturated`` (uint8),
        each [C, H // bin, W // bin].  The same ``seed`` gives the same bits; ``index_offset`` places a tile in a larger frame."""
        expected = self.expected(planes)
        image, sigma, saturated = self.noise(expected, seed, index_offset, poisson, read)
        return {'image': image, 'expected': expected, 'sigma': sigma, 'saturated': saturated}

    def deconvolve(self, image: torch.Tensor, **kw) -> dict:
        """Richardson-Lucy deconvolution of an observed ``image`` [C, h, w] against this instrument:
        :func:`sunerf_hip.deconvolve.richardson_lucy` (``iterations``, ``stop``, ``bad``, ``init``)."""
        from .deconvolve import richardson_lucy
        return richardson_lucy(image, self, **kw)

    def despike(self, image: torch.Tensor, **kw) -> dict:
        """Cosmic-ray hits and hot pixels of an observed ``image`` [C, h, w] found against this instrument's noise model and
        filled: :func:`sunerf_hip.despike.despike` with ``a``, ``b`` and ``floor`` of :func:`sunerf_hip.despike.despike_params`
        (``mode``, ``window``, ``n_sigma``, ``grow_sigma``, ``min_valid``, ``iterations``, ``two_sided``, ``fill``, ``bad``)."""
        from .despike import despike, despike_params
        if not isinstance(image, torch.Tensor) or image.dim() not in (2, 3):
            raise ValueError('Instrument.despike: image must be a tensor [C, h, w] or [h, w]')
        p = despike_params(self, 1 if image.dim() == 2 else image.shape[0])
        for k, name in enumerate(('a', 'b', 'floor')):
            kw.setdefault(name, p[:, k])
        return despike(image, **kw)

    def combine(self, frames: torch.Tensor, **kw) -> dict:
        """A stack of observed ``frames`` [T, C, h, w] combined per pixel with this instrument's noise model behind the clipping:
        :func:`sunerf_hip.stack.combine` with ``a``, ``b`` and ``floor`` of :func:`sunerf_hip.despike.despike_params` (``method``,
        ``q``, ``rank``, ``mode``, ``n_sigma``, ``iterations``, ``clip_min``, ``min_valid``, ``two_sided``, ``bad``,
        ``return_mask``)."""
        from .despike import despike_params
        from .stack import combine
        if not isinstance(frames, torch.Tensor) or frames.dim() not in (3, 4):
            raise ValueError('Instrument.combine: frames must be a tensor [T, C, h, w] or [T, h, w]')
        p = despike_params(self, 1 if frames.dim() == 3 else frames.shape[1])
        for k, name in enumerate(('a', 'b', 'floor')):
            kw.setdefault(name, p[:, k])
        return combine(frames, **kw)

    def stokes(self, frames: torch.Tensor, angles, **kw) -> dict:
        """Polariser exposures ``frames`` [N, C, h, w] observed at ``angles`` turned into Stokes planes, tB and pB with this
        instrument's noise model as the weights: :func:`sunerf_hip.polarimetry.stokes` with ``a`` and ``b`` of
        :func:`sunerf_hip.despike.despike_params` (``center``, ``throughput``, ``efficiency``, ``bad``)."""
        from .despike import despike_params
        from .polarimetry import stokes
        if not isinstance(frames, torch.Tensor) or frames.dim() not in (3, 4):
            raise ValueError('Instrument.stokes: frames must be a tensor [N, C, h, w] or [N, h, w]')
        p = despike_params(self, 1 if frames.dim() == 3 else frames.shape[1])
        for k, name in enumerate(('a', 'b')):
            kw.setdefault(name, p[:, k])
        return stokes(frames, angles, **kw)

    def noise_gate(self, frames: torch.Tensor, **kw) -> dict:
        """A sequence of observed ``frames`` [T, C, h, w] noise-gated with this instrument's noise model as the expected noise
        power: :func:`sunerf_hip.noise_gate.noise_gate` with ``a`` and ``b`` of :func:`sunerf_hip.despike.despike_params`
        (``block_t``, ``mode``, ``n_sigma``, ``spectrum``, ``bad``, ``fill_invalid``)."""
        from .despike import despike_params
        from .noise_gate import noise_gate
        if not isinstance(frames, torch.Tensor) or frames.dim() not in (3, 4):
            raise ValueError('Instrument.noise_gate: frames must be a tensor [T, C, h, w] or [T, h, w]')
        p = despike_params(self, 1 if frames.dim() == 3 else frames.shape[1])
        for k, name in enumerate(('a', 'b')):
            kw.setdefault(name, p[:, k])
        return noise_gate(frames, **kw)


def _correlate_bin(planes, taps, n_kernels, kh, kw, bin_factor, ay, ax, scale, boundary):
    c, h, w = planes.shape
    dev = planes.device
    out = torch.empty((c, h // bin_factor, w // bin_factor), dtype=torch.float32, device=dev)
    _l.call(dev, 'sunerf_instrument_correlate_bin', _ptr(planes), c, h, w, _ptr(taps), n_kernels, kh, kw, bin_factor, ay, ax,
            scale, boundary, _ptr(out), _stream(dev))
    return out


def correlate_bin_adjoint(g_out, height, width, taps, n_kernels, kh, kw, bin_factor, ay, ax, scale, boundary):
    """``g_in`` [C, height, width] float32: the transpose of the strided correlation applied to ``g_out``
    [C, height // bin, width // bin] (``sunerf_patch_correlate_bin_adjoint``)."""
    c = g_out.shape[0]
    dev = g_out.device
    if tuple(g_out.shape) != (c, height // bin_factor, width // bin_factor) or g_out.dtype != torch.float32:
        raise ValueError(f'g_out must be float32 [{c}, {height // bin_factor}, {width // bin_factor}], got {g_out.dtype} '
                         f'{tuple(g_out.shape)}')
    if g_out.numel() == 0:          # the empty call writes nothing: no detector pixel, no gradient
        return torch.zeros((c, height, width), dtype=torch.float32, device=dev)
    g_out = g_out.contiguous()
    g_in = torch.empty((c, height, width), dtype=torch.float32, device=dev)
    _l.call(dev, 'sunerf_patch_correlate_bin_adjoint', _ptr(g_out), c, height, width, _ptr(taps), n_kernels, kh, kw, bin_factor,
            ay, ax, scale, boundary, _ptr(g_in), _stream(dev))
    return g_in


class _CorrelateBin(torch.autograd.Function):
    """The strided correlation with its adjoint as the backward; the kernel is a constant."""

    @staticmethod
    def forward(ctx, planes, *call):
        ctx.call, ctx.frame = call, tuple(planes.shape[1:])
        return _correlate_bin(planes, *call)

    @staticmethod
    def backward(ctx, g):
        return (correlate_bin_adjoint(g.to(torch.float32), *ctx.frame, *ctx.call),) + (None,) * len(ctx.call)


def philox(counters: torch.Tensor, key0: int, key1: int) -> torch.Tensor:
    """Philox4x32-10 of ``counters`` [n, 4] (int32 / uint32 bit patterns, on the device) under the key: [n, 4], same dtype."""
    if not counters.is_cuda:
        raise _l.SunerfHipError('philox runs on a ROCm device (there is no CPU path)')
    if counters.dim() != 2 or counters.shape[1] != 4 or counters.element_size() != 4:
        raise ValueError(f'counters must be [n, 4] of 32-bit words, got {counters.dtype} {tuple(counters.shape)}')
    counters = counters.contiguous()
    out = torch.empty_like(counters)
    _l.call(counters.device, 'sunerf_instrument_philox', _ptr(counters), counters.shape[0], int(key0) & 0xFFFFFFFF,
            int(key1) & 0xFFFFFFFF, _ptr(out), _stream(counters.device))
    return out
