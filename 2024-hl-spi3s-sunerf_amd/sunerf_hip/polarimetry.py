"""White-light polarimetry (include/sunerf_hip_polarimetry.h, csrc/polarimetry.hip): the way from what a coronagraph
records to the two planes ``ThompsonScattering`` renders and trains on, and the classical 3-D estimate that stands beside the model.

* **Polariser frames in.**  A coronagraph records three or more exposures through a linear polariser at different angles, not tB
  and pB.  :func:`stokes` (or ``Instrument.stokes``, ``ObservationSet.add_polarised_view``) fits (I, Q, U) to them per pixel by
  weighted least squares and rotates into the Sun's tangential / radial frame: ``tb``, ``pb``, the cross term, chi^2 and, with a
  noise model, the standard deviations of tB and pB.
* **The forward of the same model.**  :func:`polarise`: what a polariser wheel records of a (tB, pB) render; plain torch.
* **The polarisation-ratio method** (Moran & Davis 2004).  :func:`ratio_depth` / :func:`view_ratio_depth`: pB / tB of a pixel fixes
  how far from the plane of the sky ONE scattering electron would sit; per ray 64 bisection steps through the Thomson-scattering
  formulas the render kernel evaluates.  The method cannot tell front from back: both points are returned.

The model of frame ``k`` is ``y_k = (t_k / 2) (I + e_k (Q cos 2 theta_k + U sin 2 theta_k))`` with ``Q = -pB C2``, ``U = -pB S2``
for light polarised tangentially (``C2``, ``S2``: cosine and sine of twice the position angle of the pixel about the Sun's centre).
One call enqueues one kernel; no result is read back.  There is no CPU path: tests/polarimetry_reference.py is the NumPy
restatement.  Out of scope: circular polarisation, Mueller matrices beyond throughput and efficiency, impact parameters below 1.25
solar radii (two roots per side), the F-corona's polarisation, gradients, and the choice between front and back."""
import ctypes
import math
from typing import Optional

import numpy as np
import torch

from . import lib as _l
from ._ffi import _dev, _ptr, _stream

DETERMINED, UNDETERMINED, CENTRE = 0, 1, 2                        # include/sunerf_hip_polarimetry.h: status of a pixel
OK, ABOVE, BELOW, CLOSE, DEGENERATE, INVALID = 0, 1, 2, 3, 4, 5    # ... of a ray
MIN_FRAMES, MAX_FRAMES = 3, 8
N_COUNTS = 4
MIN_IMPACT = 1.25
STOKES_OUTPUTS = ('stokes', 'tb', 'pb', 'pb_cross', 'chi2', 'sigma_tb', 'sigma_pb', 'status', 'counts')
DEPTH_OUTPUTS = ('depth', 'z_front', 'z_back', 'radius', 'slope', 'status')


def _host(values):
    return (ctypes.c_double * len(values))(*[float(v) for v in values])


def design(angles, throughput=None, efficiency=None):
    """``(cos2, sin2, throughput, efficiency)`` as fp64 arrays of one length: cosine and sine of twice the polariser ``angles``
    [rad], the throughputs ``t_k`` and efficiencies ``e_k`` (None or a number: the same for every frame; default 1)."""
    angles = np.atleast_1d(np.asarray(angles, dtype=np.float64))
    if angles.ndim != 1 or not np.all(np.isfinite(angles)):
        raise ValueError(f'angles must be a list of finite polariser angles [rad], got {angles!r}')
    n = angles.shape[0]
    out = [np.cos(2.0 * angles), np.sin(2.0 * angles)]
    for name, value in (('throughput', throughput), ('efficiency', efficiency)):
        v = np.atleast_1d(np.asarray(1.0 if value is None else value, dtype=np.float64))
        if v.ndim != 1 or v.shape[0] not in (1, n):
            raise ValueError(f'{name} must be a number or one per frame ({n}), got shape {v.shape}')
        if not np.all(np.isfinite(v)) or np.any(v <= 0):
            raise ValueError(f'{name} must be finite and above 0, got {value!r}')
        out.append(np.ascontiguousarray(np.broadcast_to(v, (n,))))
    return tuple(out)


def _centre(center):
    cy, cx = (float(v) for v in center)
    if not (math.isfinite(cy) and math.isfinite(cx)):
        raise ValueError(f'center must be two finite pixel coordinates (row, column), got {center!r}')
    return cy, cx


def stokes_launch(frames, bad, cos2, sin2, throughput, efficiency, a, b, cy, cx, outputs=STOKES_OUTPUTS):
    """``sunerf_polarimetry_stokes`` on device tensors: ``frames`` [N, C, H, W] float32, ``bad`` uint8 of that shape or None, the four
    host sequences of length N, ``a`` / ``b`` [C] float64 on the device or both None.  ``outputs``: which of ``STOKES_OUTPUTS`` to
    allocate (``tb`` and ``pb`` always are); the others are passed as NULL.  Returns the dict of those tensors."""
    n, c, h, w = frames.shape
    dev = frames.device
    f32 = dict(dtype=torch.float32, device=dev)
    want = set(outputs) | {'tb', 'pb'}
    out = {}
    for name in STOKES_OUTPUTS:
        if name not in want:
            continue
        if name == 'stokes':
            out[name] = torch.empty((3, c, h, w), **f32)
        elif name == 'status':
            out[name] = torch.empty((c, h, w), dtype=torch.uint8, device=dev)
        elif name == 'counts':
            out[name] = torch.zeros((c, N_COUNTS), dtype=torch.int64, device=dev)
        else:
            out[name] = torch.empty((c, h, w), **f32)
    if c * h * w == 0:          # the empty call writes nothing
        return out
    _l.call(dev, 'sunerf_polarimetry_stokes', _ptr(frames), _ptr(bad), _host(cos2), _host(sin2), _host(throughput), _host(efficiency),
            _ptr(a), _ptr(b), n, c, h, w, float(cy), float(cx), *[_ptr(out.get(k)) for k in STOKES_OUTPUTS], _stream(dev))
    return out


def stokes(frames: torch.Tensor, angles, *, center, throughput=None, efficiency=None, a=None, b=None,
           bad: Optional[torch.Tensor] = None) -> dict:
    """``frames`` [N, C, H, W] or [N, H, W] float32 on the device, ``3 <= N <= 8`` exposures through a linear polariser at
    ``angles`` [rad, from the image's column axis towards its row axis]; NaN and infinite samples are not valid, nor are those of
    ``bad`` (same shape, bool or uint8).  ``center = (cy, cx)``: the Sun's centre in pixels (``enhance.sun_geometry`` gives a
    view's).  ``throughput`` / ``efficiency``: ``t_k`` and ``e_k`` of the model above, numbers or one per frame.  ``a`` / ``b``:
    the variance of a sample is ``a + b max(y, 0)`` (numbers or one per plane; ``despike_params`` gives an instrument's,
    ``Instrument.stokes`` passes them); without them every sample weighs 1 and no standard deviation is formed.

    Returns device tensors: ``stokes`` [3, C, H, W] (I, Q, U in the image frame), ``tb``, ``pb``, ``pb_cross``, ``chi2``,
    ``sigma_tb``, ``sigma_pb`` [C, H, W] float32, ``status`` uint8 (DETERMINED 0; UNDETERMINED 1: fewer than three valid samples or
    angles that do not span the three unknowns, every output NaN; CENTRE 2: the pixel on the Sun's centre, where pB has no
    direction), ``counts`` [C, 4] int64 (pixels determined, undetermined, centre, and pixels that lost at least one sample), and in
    plain torch ``polarised_fraction = sqrt(Q^2 + U^2) / I`` and ``angle = atan2(U, Q) / 2``.  A three-dimensional input gives
    the planes without the channel axis."""
    if not isinstance(frames, torch.Tensor):
        raise TypeError('stokes: frames must be a torch.Tensor')
    stack = frames[:, None] if frames.dim() == 3 else frames
    if stack.dim() != 4 or stack.dtype != torch.float32:
        raise ValueError(f'stokes: frames must be float32 [N, C, H, W] or [N, H, W], got {frames.dtype} {tuple(frames.shape)}')
    n, c = stack.shape[:2]
    if not MIN_FRAMES <= n <= MAX_FRAMES:
        raise ValueError(f'stokes: {MIN_FRAMES} to {MAX_FRAMES} frames, got {n}')
    cos2, sin2, thr, eff = design(angles, throughput, efficiency)
    if cos2.shape[0] != n:
        raise ValueError(f'stokes: {n} frames and {cos2.shape[0]} angles')
    cy, cx = _centre(center)
    if (a is None) != (b is None):
        raise ValueError('stokes: the noise model needs both a and b (despike_params(instrument, C), or Instrument.stokes)')
    from .despike import _per_plane
    pa = None if a is None else np.array(_per_plane(a, 'a', c))          # (a copy: the broadcast view is read-only)
    pb = None if b is None else np.array(_per_plane(b, 'b', c))
    flagged = None
    if bad is not None:
        flagged = torch.as_tensor(bad)
        flagged = flagged[:, None] if flagged.dim() == 3 else flagged
        if tuple(flagged.shape) != tuple(stack.shape):
            raise ValueError(f'bad must have the shape of the frames {tuple(stack.shape)}, got {tuple(flagged.shape)}')
    if not stack.is_cuda:
        raise _l.SunerfHipError('stokes runs on a ROCm device (there is no CPU path)')
    stack = stack.contiguous()
    dev = stack.device
    if flagged is not None:
        flagged = (flagged.to(dev) != 0).to(torch.uint8).contiguous()
    pa = None if pa is None else torch.as_tensor(pa, dtype=torch.float64).to(dev)
    pb = None if pb is None else torch.as_tensor(pb, dtype=torch.float64).to(dev)
    out = stokes_launch(stack, flagged, cos2, sin2, thr, eff, pa, pb, cy, cx)
    i, q, u = out['stokes']
    out['polarised_fraction'] = torch.sqrt(q * q + u * u) / i
    out['angle'] = 0.5 * torch.atan2(u, q)
    if frames.dim() == 3:
        out = {k: (v if k == 'counts' else (v[:, 0] if k == 'stokes' else v[0])) for k, v in out.items()}
    return out


def rotation(height: int, width: int, center, device=None, dtype=torch.float64):
    """``(C2, S2)`` [H, W]: cosine and sine of twice the position angle of every pixel about ``center = (cy, cx)``, without
    trigonometry: ``((dx^2 - dy^2) / (dx^2 + dy^2), 2 dx dy / (dx^2 + dy^2))``; NaN on the centre itself."""
    cy, cx = _centre(center)
    dy = (torch.arange(height, dtype=torch.float64, device=device) - cy)[:, None]
    dx = (torch.arange(width, dtype=torch.float64, device=device) - cx)[None, :]
    n = dx * dx + dy * dy
    return ((dx * dx - dy * dy) / n).to(dtype), ((2.0 * (dx * dy)) / n).to(dtype)


def polarise(tb: torch.Tensor, pb: torch.Tensor, angles, *, center, throughput=None, efficiency=None) -> torch.Tensor:
    """What a polariser wheel records of a render: ``tb``, ``pb`` [..., H, W] -> frames [N, ..., H, W] of the model above with
    ``I = tb``, ``Q = -pb C2``, ``U = -pb S2`` (tangential polarisation, no cross term).  Plain torch on the tensors' device, in
    their dtype (float64 in, float64 out); the pixel on the Sun's centre, where pB has no direction, is unpolarised."""
    if tb.shape != pb.shape or tb.dim() < 2:
        raise ValueError(f'polarise: tb and pb must have one shape [..., H, W], got {tuple(tb.shape)} and {tuple(pb.shape)}')
    cos2, sin2, thr, eff = design(angles, throughput, efficiency)
    c2, s2 = (torch.nan_to_num(v, nan=0.0) for v in rotation(tb.shape[-2], tb.shape[-1], center, tb.device))   # (0 / 0 on the centre)
    work = torch.float64
    i, q, u = tb.to(work), -(pb.to(work) * c2), -(pb.to(work) * s2)
    frames = [(0.5 * t) * (i + e * (q * c + u * s)) for c, s, t, e in zip(cos2.tolist(), sin2.tolist(), thr.tolist(), eff.tolist())]
    return torch.stack(frames).to(tb.dtype)


def ratio_depth_launch(tb, pb, rays_o, rays_d, solar_radius, limb_darkening_coeff, x_max_factor=64., outputs=DEPTH_OUTPUTS):
    """``sunerf_polarimetry_ratio_depth`` on device tensors: ``tb``, ``pb`` [n], ``rays_o``, ``rays_d`` [n, 3] float32 and the two
    one-element float32 buffers.  ``outputs``: which of ``DEPTH_OUTPUTS`` to allocate (``depth`` and ``status`` always are)."""
    n = tb.shape[0]
    dev = tb.device
    want = set(outputs) | {'depth', 'status'}
    out = {k: torch.empty(n, dtype=torch.uint8 if k == 'status' else torch.float32, device=dev) for k in DEPTH_OUTPUTS if k in want}
    if n == 0:
        return out
    _l.call(dev, 'sunerf_polarimetry_ratio_depth', _ptr(tb), _ptr(pb), _ptr(rays_o), _ptr(rays_d), _ptr(solar_radius),
            _ptr(limb_darkening_coeff), n, float(x_max_factor), *[_ptr(out.get(k)) for k in DEPTH_OUTPUTS], _stream(dev))
    return out


def ratio_depth(tb: torch.Tensor, pb: torch.Tensor, rays_o: torch.Tensor, rays_d: torch.Tensor, constants, x_max_factor: float = 64.,
                ratio_sigma: Optional[torch.Tensor] = None) -> dict:
    """The polarisation-ratio depth of ``n`` lines of sight: ``tb``, ``pb`` [n] and ``rays_o``, ``rays_d`` [n, 3] float32 on the
    device; ``constants = (solar_radius, limb_darkening_coeff)``, the one-element buffers of a ``ThompsonScattering`` module (or
    numbers), in the rays' length unit.  Returns ``depth`` (the distance ``x >= 0`` from the ray's point closest to the Sun, model
    length units, searched in ``[0, x_max_factor b]`` with ``b`` the impact parameter), ``z_front`` / ``z_back`` (the two ray
    parameters ``z0 -+ x / |d|``), ``radius = sqrt(b^2 + x^2)``, ``slope = d(pB / tB) / dx`` there, and ``status`` uint8: OK 0;
    ABOVE 1 (ratio above the plane-of-sky value: ``x = 0``; noise does this); BELOW 2 (ratio below that of the far end, negative
    pB included: ``x`` is the far end); CLOSE 3 (impact parameter below 1.25 solar radii, where the ratio has two roots per side),
    DEGENERATE 4 (``d = 0``) and INVALID 5 (``tb``, ``pb`` not finite or ``tb <= 0``), all NaN.  With ``ratio_sigma`` [n], the
    standard deviation of pB / tB, also ``depth_sigma = ratio_sigma / |slope|``."""
    if not isinstance(tb, torch.Tensor) or tb.dim() != 1:
        raise ValueError('ratio_depth: tb must be a tensor [n]')
    if not (np.isscalar(x_max_factor) and math.isfinite(x_max_factor) and x_max_factor > 0):
        raise ValueError(f'ratio_depth: x_max_factor must be a finite number above 0, got {x_max_factor!r}')
    if len(constants) < 2:
        raise ValueError('ratio_depth: constants are (solar_radius, limb_darkening_coeff)')
    n = tb.shape[0]
    tb = _dev(tb, 'tb', (n,)); pb = _dev(pb, 'pb', (n,))
    rays_o = _dev(rays_o, 'rays_o', (n, 3)); rays_d = _dev(rays_d, 'rays_d', (n, 3))
    dev = tb.device
    rs, ld = (_dev(torch.as_tensor(c, dtype=torch.float32).detach().reshape(1).to(dev), name, (1,))
              for c, name in zip(constants[:2], ('solar_radius', 'limb_darkening_coeff')))
    out = ratio_depth_launch(tb, pb, rays_o, rays_d, rs, ld, x_max_factor)
    if ratio_sigma is not None:
        out['depth_sigma'] = _dev(ratio_sigma, 'ratio_sigma', (n,)) / out['slope'].abs()
    return out


def view_ratio_depth(tb: torch.Tensor, pb: torch.Tensor, observer_or_view, rendering, x_max_factor: float = 64.,
                     ratio_sigma: Optional[torch.Tensor] = None) -> dict:
    """:func:`ratio_depth` of a whole frame: ``tb``, ``pb`` [H, W] of ``observer_or_view`` (a ``reprojection.Observer``, a ``View`` or
    a dict of Observer arguments), whose rays come from ``sunerf_hip.rays.grid_rays``; ``solar_radius`` and
    ``limb_darkening_coeff`` are those of ``rendering``, a ``ThompsonScattering`` module.  Returns the maps of :func:`ratio_depth`
    as [H, W] and ``points_front`` / ``points_back`` [H, W, 3]: ``o + d z`` at the two ray parameters, in solar radii."""
    from .rays import grid_rays
    from .reprojection import _as_observer
    obs = _as_observer(observer_or_view)
    if not isinstance(tb, torch.Tensor) or tb.dim() != 2 or tb.shape != pb.shape:
        raise ValueError('view_ratio_depth: tb and pb must be tensors [H, W] of one shape')
    if not tb.is_cuda:
        raise _l.SunerfHipError('view_ratio_depth runs on a ROCm device (there is no CPU path)')
    tx, ty = obs.axes(tb.device)
    h, w = tb.shape
    if (ty.shape[0], tx.shape[0]) != (h, w):
        raise ValueError(f'view_ratio_depth: the observer\'s grid is {ty.shape[0]} x {tx.shape[0]}, the planes are {h} x {w}')
    rays_o, rays_d = grid_rays(tx, ty, obs.c2w)
    flat = None if ratio_sigma is None else ratio_sigma.reshape(-1)
    out = ratio_depth(tb.reshape(-1), pb.reshape(-1), rays_o, rays_d, (rendering.solar_radius, rendering.limb_darkening_coeff),
                      x_max_factor, flat)
    per_radius = 1.0 / rendering.solar_radius.to(rays_o.device)
    points = {f'points_{side}': ((rays_o + rays_d * out[f'z_{side}'][:, None]) * per_radius).view(h, w, 3) for side in ('front', 'back')}
    out = {k: v.view(h, w) for k, v in out.items()}
    out.update(points)
    return out
