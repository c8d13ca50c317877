"""Enhancement of coronal images (include/sunerf_hip_enhance.h, csrc/enhance.hip): what makes a registered,
combined and gated image readable.

* :func:`mgn` -- multi-scale Gaussian normalisation (Morgan & Druckmuller 2014) for EUV frames: at each scale the image is
  normalised by its local mean and standard deviation (Gaussian windows), squashed through an arctangent, and a gamma-stretched copy
  of the image is added.
* :func:`radial_statistics` and :func:`nrgf` -- the normalising radial graded filter (Morgan, Habbal & Woo 2006) for anything off
  the limb: the mean of a pixel's annulus around the Sun is removed and the rest divided by the annulus's standard deviation, which
  takes out the steep radial fall-off.  The ring x segment table of :func:`radial_statistics` is what a Fourier variant would
  stand on.
* :func:`sun_geometry`, :func:`radial_edges` -- the centre and the rings in pixels from an observer.

Inputs are float32 device tensors ``[C, H, W]`` or ``[H, W]``; planes are independent.  A pixel that is not finite or flagged in
``bad`` is invalid: it enters no sum and is NaN in every output.  Everything is enqueued on the current stream and nothing is read
back; results are dicts of device tensors.  There is no CPU path: tests/enhance_reference.py is the NumPy restatement.

Out of scope: the Fourier NRGF, gradients, parity with sunkit-image (not pinned), spatially varying scales."""
import ctypes
import math
from typing import Optional, Sequence

import numpy as np
import torch

from . import lib as _l
from ._ffi import _ptr, _stream, _workspace

MAX_SCALES, MAX_RADIUS = 8, 128
MAX_RINGS, MAX_SEGMENTS, MAX_BINS = 4096, 360, 65536
MAX_CENTER = 2.0 ** 30
ROW_TILE, COL_TILE = (4, 512), (128, 32)          # (rows, columns) a workgroup of the row pass / the column pass forms
DEFAULT_SIGMA = (1.25, 2.5, 5.0, 10.0, 20.0, 40.0)
OUTSIDE_MODES = {'keep': 0, 'missing': 1}
_WORKSPACES = {}


def radius_of(sigma: float, truncate: float) -> int:
    """scipy's rule: ``int(truncate * sigma + 0.5)``."""
    return int(truncate * sigma + 0.5)


def _planes(name, image):
    if not isinstance(image, torch.Tensor):
        raise TypeError(f'{name}: image must be a torch.Tensor, got {type(image).__name__}')
    if image.dtype != torch.float32 or image.dim() not in (2, 3):
        raise ValueError(f'{name}: image must be float32 [C, H, W] or [H, W], got {image.dtype} {tuple(image.shape)}')
    squeeze = image.dim() == 2
    planes = image[None] if squeeze else image
    if min(planes.shape) < 1:
        raise ValueError(f'{name}: image must have at least one plane of 1 x 1 pixels, got {tuple(image.shape)}')
    if planes.shape[0] > 65535:
        raise ValueError(f'{name}: image has at most 65535 planes, got {planes.shape[0]}')
    return planes, squeeze


def _bad(name, bad, planes):
    if bad is None:
        return None
    if not isinstance(bad, torch.Tensor):
        raise TypeError(f'{name}: bad must be a torch.Tensor, got {type(bad).__name__}')
    if bad.dtype not in (torch.bool, torch.uint8):
        raise ValueError(f'{name}: bad must be bool or uint8, got {bad.dtype}')
    if bad.dim() == planes.dim() - 1:
        bad = bad[None]
    if tuple(bad.shape) != tuple(planes.shape):
        raise ValueError(f'{name}: bad must have the shape of image, got {tuple(bad.shape)}')
    return bad


def _device(name, planes, *others):
    dev = planes.device
    if dev.type != 'cuda' or any(o is not None and o.device != dev for o in others):
        raise _l.SunerfHipError(f'{name} runs on one ROCm device (there is no CPU path)')
    return dev


def _per_plane(name, arg, value, c, minimum=None):
    """None, a scalar or one value per plane -> None or a float32 host array [c] of finite numbers."""
    if value is None:
        return None
    v = np.asarray(value.tolist() if isinstance(value, torch.Tensor) else value, dtype=np.float64).reshape(-1)
    if v.shape[0] == 1:
        v = np.repeat(v, c)
    if v.shape != (c,) or not np.isfinite(v).all():
        raise ValueError(f'{name}: {arg} must be a finite scalar or one finite value per plane ({c}), got {value!r}')
    if minimum is not None and (v < minimum).any():
        raise ValueError(f'{name}: {arg} must be >= {minimum}, got {value!r}')
    return v.astype(np.float32)


def _number(name, arg, value, positive=False):
    if isinstance(value, bool) or not isinstance(value, (int, float, np.integer, np.floating)):
        raise TypeError(f'{name}: {arg} must be a number, got {type(value).__name__}')
    value = float(value)
    if not math.isfinite(value) or (positive and not value > 0):
        raise ValueError(f'{name}: {arg} must be finite{" and > 0" if positive else ""}, got {value}')
    return value


def mgn_launch(planes, bad, sigma, weights, truncate, k, gamma, h, lo, hi, floor):
    """``sunerf_enhance_mgn`` on checked arguments: ``planes`` float32 [C, H, W] and ``bad`` uint8 or None on the device, ``sigma``
    float64 and ``weights`` float32 host arrays, ``lo`` / ``hi`` / ``floor`` float32 device tensors [C] or None.  Returns ``(out,
    lo, hi, state [C, 3])``."""
    dev = planes.device
    c, hgt, wid = (int(v) for v in planes.shape)
    lib = _l.load()
    out = torch.empty_like(planes)
    lo_out, hi_out = torch.empty(c, dtype=torch.float32, device=dev), torch.empty(c, dtype=torch.float32, device=dev)
    state = torch.empty((c, 3), dtype=torch.int64, device=dev)
    nbytes = int(lib.sunerf_enhance_mgn_workspace_bytes(c, hgt, wid))
    ws = _workspace(_WORKSPACES, dev, nbytes + 256)
    offset = (-ws.data_ptr()) % 256
    sigma = np.ascontiguousarray(sigma, dtype=np.float64)
    weights = None if weights is None else np.ascontiguousarray(weights, dtype=np.float32)
    _l.call(dev, 'sunerf_enhance_mgn', _ptr(planes), _ptr(bad), c, hgt, wid, sigma.ctypes.data_as(ctypes.c_void_p),
            None if weights is None else weights.ctypes.data_as(ctypes.c_void_p), int(sigma.shape[0]), float(truncate), float(k),
            float(gamma), float(h), _ptr(lo), _ptr(hi), _ptr(floor), _ptr(out), _ptr(lo_out), _ptr(hi_out), _ptr(state),
            ctypes.c_void_p(ws.data_ptr() + offset), nbytes, _stream(dev))
    return out, lo_out, hi_out, state


def mgn(image, sigma: Sequence[float] = DEFAULT_SIGMA, weights: Optional[Sequence[float]] = None, k: float = 0.7, gamma: float = 3.2,
        h: float = 0.7, truncate: float = 3.0, lo=None, hi=None, floor=None, bad=None) -> dict:
    """Multi-scale Gaussian normalisation of ``image`` (float32 ``[C, H, W]`` or ``[H, W]`` on the device).

    Per scale ``sigma_i`` (at most 8; the radius ``int(truncate * sigma_i + 0.5)`` at most 128) with the Gaussian window ``G_i``
    (edge-replicating, normalised over valid taps): ``r = x - G_i[x]``, ``s = sqrt(G_i[r^2] + floor^2)``, ``t_i = atan(k r / s)``.
    The result is ``h g + (1 - h) / n sum_i weights_i t_i`` with ``g = clamp((x - lo) / (hi - lo), 0, 1) ** (1 / gamma)``.
    ``lo`` / ``hi``: scalars or one value per plane, default the minimum / maximum of the plane's valid pixels (found on the device).
    ``floor`` (data units, >= 0): default ``2^-16 max(|lo|, |hi|)``, just above the rounding noise of the window sums on a pedestal.
    ``bad``: bool or uint8 of the image's shape; flagged and non-finite pixels enter no sum and are NaN in the result.

    The defaults are sunkit-image's.  Its clipping of non-positive data to ``1e-15`` before the filter is the caller's business:
    nothing is clipped here.

    Returns ``image``, ``lo``, ``hi`` (``[C]`` float32, what was used; NaN for a plane without a valid pixel) and ``counts``
    (``[C, 3]`` int64: invalid pixels, valid pixels below ``lo``, valid pixels above ``hi``) -- all on the device."""
    planes, squeeze = _planes('mgn', image)
    bad = _bad('mgn', bad, planes)
    try:
        sig = np.asarray(sigma, dtype=np.float64).reshape(-1)
    except (TypeError, ValueError):
        raise TypeError(f'mgn: sigma must be a sequence of numbers, got {sigma!r}') from None
    if not 1 <= sig.shape[0] <= MAX_SCALES or not np.isfinite(sig).all() or (sig < 0).any():
        raise ValueError(f'mgn: sigma must be 1 .. {MAX_SCALES} finite values >= 0, got {sigma!r}')
    truncate = _number('mgn', 'truncate', truncate)
    if truncate < 0:
        raise ValueError(f'mgn: truncate must be >= 0, got {truncate}')
    radii = [radius_of(s, truncate) for s in sig]
    if max(radii) > MAX_RADIUS:
        raise ValueError(f'mgn: the radius int(truncate * sigma + 0.5) is at most {MAX_RADIUS}, got {max(radii)}')
    if weights is not None:
        weights = np.asarray(weights, dtype=np.float64).reshape(-1)
        if weights.shape != sig.shape or not np.isfinite(weights).all():
            raise ValueError(f'mgn: weights must be one finite value per scale ({sig.shape[0]}), got {weights!r}')
    k, h = _number('mgn', 'k', k), _number('mgn', 'h', h)
    gamma = _number('mgn', 'gamma', gamma, positive=True)
    c = int(planes.shape[0])
    lo, hi = _per_plane('mgn', 'lo', lo, c), _per_plane('mgn', 'hi', hi, c)
    floor = _per_plane('mgn', 'floor', floor, c, minimum=0.0)
    dev = _device('mgn', planes, bad)
    planes = planes.contiguous()
    if bad is not None:
        bad = bad.to(torch.uint8).contiguous()
    lo, hi, floor = (None if v is None else torch.from_numpy(v).to(dev) for v in (lo, hi, floor))
    out, lo_out, hi_out, state = mgn_launch(planes, bad, sig, weights, truncate, k, gamma, h, lo, hi, floor)
    return {'image': out[0] if squeeze else out, 'lo': lo_out, 'hi': hi_out, 'counts': state}


def _geometry(name, center, edges, n_segments=1):
    try:
        cy, cx = (float(v) for v in center)
    except (TypeError, ValueError):
        raise TypeError(f'{name}: center must be a pair (cy, cx) of numbers, got {center!r}') from None
    if not (abs(cy) <= MAX_CENTER and abs(cx) <= MAX_CENTER):
        raise ValueError(f'{name}: center must be finite and within 2^30 pixels, got {center!r}')
    e = np.asarray(edges.tolist() if isinstance(edges, torch.Tensor) else edges, dtype=np.float64)
    if e.ndim != 1 or not 2 <= e.shape[0] <= MAX_RINGS + 1:
        raise ValueError(f'{name}: edges must be 2 .. {MAX_RINGS + 1} values (1 .. {MAX_RINGS} rings), got shape {e.shape}')
    if not np.isfinite(e).all() or e[0] < 0 or not (np.diff(e) > 0).all():
        raise ValueError(f'{name}: edges must be finite, >= 0 and strictly ascending')
    if isinstance(n_segments, bool) or not isinstance(n_segments, (int, np.integer)):
        raise TypeError(f'{name}: n_segments must be an int, got {type(n_segments).__name__}')
    if not 1 <= n_segments <= MAX_SEGMENTS or (e.shape[0] - 1) * n_segments > MAX_BINS:
        raise ValueError(f'{name}: n_segments must be 1 .. {MAX_SEGMENTS} with at most {MAX_BINS} bins, got {n_segments} x {e.shape[0] - 1} rings')
    return cy, cx, e


def statistics_launch(planes, bad, cy, cx, edges, n_segments):
    """``sunerf_enhance_radial_statistics``: ``edges`` a float64 device tensor.  Returns count, mean, std, min, max ``[C, R, S]``."""
    dev = planes.device
    c, hgt, wid = (int(v) for v in planes.shape)
    shape = (c, int(edges.shape[0]) - 1, int(n_segments))
    count = torch.empty(shape, dtype=torch.int64, device=dev)
    mean, std, mn, mx = (torch.empty(shape, dtype=torch.float64, device=dev) for _ in range(4))
    _l.call(dev, 'sunerf_enhance_radial_statistics', _ptr(planes), _ptr(bad), c, hgt, wid, float(cy), float(cx), _ptr(edges), shape[1],
            shape[2], _ptr(count), _ptr(mean), _ptr(std), _ptr(mn), _ptr(mx), _stream(dev))
    return count, mean, std, mn, mx


def radial_statistics(image, center, edges, n_segments: int = 1, bad=None) -> dict:
    """Statistics of the valid pixels of every ring (and angular segment) around ``center = (cy, cx)`` [pixels].  ``edges``: the
    ring radii in pixels, ``>= 0`` and strictly ascending; pixel ``(y, x)`` is in ring ``i`` iff ``edges[i]^2 <= (y - cy)^2 + (x -
    cx)^2 < edges[i + 1]^2``, and with ``n_segments > 1`` in the segment its angle ``atan2(y - cy, x - cx) + pi`` falls in.

    Returns ``count`` (int64), ``mean``, ``std`` (population), ``min``, ``max`` (float64; NaN in an empty bin), each ``[C, rings,
    n_segments]`` (``[rings, n_segments]`` for an image without a plane axis), on the device."""
    planes, squeeze = _planes('radial_statistics', image)
    bad = _bad('radial_statistics', bad, planes)
    cy, cx, e = _geometry('radial_statistics', center, edges, n_segments)
    dev = _device('radial_statistics', planes, bad)
    if bad is not None:
        bad = bad.to(torch.uint8).contiguous()
    stats = statistics_launch(planes.contiguous(), bad, cy, cx, torch.from_numpy(e).to(dev), int(n_segments))
    return {key: (v[0] if squeeze else v) for key, v in zip(('count', 'mean', 'std', 'min', 'max'), stats)}


def nrgf_launch(planes, bad, cy, cx, edges, outside, missing, statistics):
    """``sunerf_enhance_nrgf``: ``statistics`` None (computed in the call) or ``(count, mean, std)`` device tensors ``[C, R]``.
    Returns ``(out, state [C, 3], (count, mean, std, min, max))`` -- min and max None with the caller's statistics."""
    dev = planes.device
    c, hgt, wid = (int(v) for v in planes.shape)
    rings = int(edges.shape[0]) - 1
    if statistics is None:
        count = torch.empty((c, rings), dtype=torch.int64, device=dev)
        mean, std, mn, mx = (torch.empty((c, rings), dtype=torch.float64, device=dev) for _ in range(4))
    else:
        (count, mean, std), mn, mx = statistics, None, None
    out = torch.empty_like(planes)
    state = torch.empty((c, 3), dtype=torch.int64, device=dev)
    _l.call(dev, 'sunerf_enhance_nrgf', _ptr(planes), _ptr(bad), c, hgt, wid, float(cy), float(cx), _ptr(edges), rings, int(outside),
            float(missing), int(statistics is None), _ptr(count), _ptr(mean), _ptr(std), _ptr(mn), _ptr(mx), _ptr(out), _ptr(state),
            _stream(dev))
    return out, state, (count, mean, std, mn, mx)


def nrgf(image, center, edges, outside: str = 'keep', missing: float = float('nan'), bad=None, statistics: Optional[dict] = None) -> dict:
    """The normalising radial graded filter: ``(x - mean_b) / std_b`` with the statistics of the pixel's ring ``b`` (see
    :func:`radial_statistics`), 0 where the ring holds fewer than two valid pixels or has no spread.  A pixel outside ``[edges[0],
    edges[-1])`` keeps its value (``outside='keep'``) or becomes ``missing`` (``outside='missing'``).  ``statistics``: a dict with
    ``count``, ``mean`` and ``std`` ``[C, rings]`` (or ``[C, rings, 1]``) on the device -- another frame's, a smoothed table -- used
    instead of the image's own.

    Returns ``image``, ``counts`` (``[C, 3]`` int64: invalid pixels, pixels outside the rings, pixels of degenerate rings) and
    ``statistics`` (``count``, ``mean``, ``std`` and, when computed here, ``min`` and ``max``, each ``[C, rings]``)."""
    planes, squeeze = _planes('nrgf', image)
    bad = _bad('nrgf', bad, planes)
    cy, cx, e = _geometry('nrgf', center, edges)
    if outside not in OUTSIDE_MODES:
        raise ValueError(f"nrgf: outside must be 'keep' or 'missing', got {outside!r}")
    if isinstance(missing, bool) or not isinstance(missing, (int, float, np.integer, np.floating)):
        raise TypeError(f'nrgf: missing must be a number, got {type(missing).__name__}')
    c, rings = int(planes.shape[0]), e.shape[0] - 1
    given = None
    if statistics is not None:
        if not isinstance(statistics, dict) or any(key not in statistics for key in ('count', 'mean', 'std')):
            raise TypeError("nrgf: statistics must be a dict with 'count', 'mean' and 'std'")
        given = []
        for key, dtype in (('count', torch.int64), ('mean', torch.float64), ('std', torch.float64)):
            v = statistics[key]
            if not isinstance(v, torch.Tensor) or v.dtype != dtype:
                raise TypeError(f'nrgf: statistics[{key!r}] must be a {dtype} tensor')
            if v.numel() != c * rings or tuple(v.shape) not in ((c, rings), (c, rings, 1), (rings,), (rings, 1)):
                raise ValueError(f'nrgf: statistics[{key!r}] must be [{c}, {rings}], got {tuple(v.shape)}')
            given.append(v)
    dev = _device('nrgf', planes, bad, *(given or ()))
    if bad is not None:
        bad = bad.to(torch.uint8).contiguous()
    if given is not None:
        given = tuple(v.reshape(c, rings).contiguous() for v in given)
    out, state, stats = nrgf_launch(planes.contiguous(), bad, cy, cx, torch.from_numpy(e).to(dev), OUTSIDE_MODES[outside], missing, given)
    table = {key: (v[0] if squeeze else v) for key, v in zip(('count', 'mean', 'std', 'min', 'max'), stats) if v is not None}
    return {'image': out[0] if squeeze else out, 'counts': state, 'statistics': table}


def sun_geometry(observer, Rs_per_ds: float = 1.0):
    """``(center, pixels_per_radius)`` of a ``reprojection.Observer`` or ``View``: ``center = (cy, cx)`` is where both pixel axes cross
    zero angle, ``pixels_per_radius`` the limb angle ``asin(R / distance)`` over the pixel pitch.  Raises for axes that are not
    uniform (per pixel within 1e-6 of the pitch) and for pitches that differ between x and y by more than 1e-9 relative."""
    from .reprojection import _as_observer, _radius
    radius = _radius(Rs_per_ds)
    obs = _as_observer(observer)
    tx, ty = (np.asarray(a.tolist(), dtype=np.float64) for a in obs.axes('cpu'))
    pitch = []
    for name, axis in (('tx', tx), ('ty', ty)):
        if axis.shape[0] < 2:
            raise ValueError(f'sun_geometry: {name} needs at least two pixels to have a pitch')
        step = (axis[-1] - axis[0]) / (axis.shape[0] - 1)
        if not (np.isfinite(step) and step != 0) or (np.abs(np.diff(axis) - step) > 1e-6 * abs(step)).any():
            raise ValueError(f'sun_geometry: {name} is not a uniform axis')
        pitch.append(step)
    if abs(abs(pitch[0]) - abs(pitch[1])) > 1e-9 * abs(pitch[0]):
        raise ValueError(f'sun_geometry: the pitches of tx and ty differ: {abs(pitch[0])} and {abs(pitch[1])} rad per pixel')
    distance = float(obs.distance)
    if not distance > radius:
        raise ValueError(f'sun_geometry: the observer at {distance} is inside the sphere of radius {radius}')
    center = (float(-ty[0] / pitch[1]), float(-tx[0] / pitch[0]))
    return center, float(math.asin(radius / distance) / abs(pitch[0]))


def radial_edges(r_min: float, r_max: float, n: int, pixels_per_radius: float) -> np.ndarray:
    """``n + 1`` linear ring edges in pixels from ``r_min`` to ``r_max`` in apparent solar radii."""
    r_min, r_max = _number('radial_edges', 'r_min', r_min), _number('radial_edges', 'r_max', r_max)
    pixels_per_radius = _number('radial_edges', 'pixels_per_radius', pixels_per_radius, positive=True)
    if isinstance(n, bool) or not isinstance(n, (int, np.integer)):
        raise TypeError(f'radial_edges: n must be an int, got {type(n).__name__}')
    if not 1 <= n <= MAX_RINGS:
        raise ValueError(f'radial_edges: n must be 1 .. {MAX_RINGS}, got {n}')
    if not 0 <= r_min < r_max:
        raise ValueError(f'radial_edges: 0 <= r_min < r_max, got {r_min} and {r_max}')
    return np.linspace(r_min, r_max, n + 1) * pixels_per_radius
