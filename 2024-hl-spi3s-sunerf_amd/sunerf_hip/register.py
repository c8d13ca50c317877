"""Registration of image sequences (include/sunerf_hip_register.h, csrc/register.hip): every frame of a
sequence, taken by its own observer on its own pixel grid at its own time, is resampled onto ONE reference observer, grid and
time, so that pixel ``(y, x)`` of every frame shows the same piece of the Sun.  That is what ``combine``, ``background`` and
``noise_gate`` assume and what nothing else in the project makes true: ``coalign`` measures a pointing offset and never applies
it to pixels, ``prep`` resamples by one affine map.

The map of an output pixel: its line of sight from the reference observer meets the sphere ``r = 1 / Rs_per_ds`` (off the disk:
the point of closest approach, or ``missing``); that point is turned by the differential rotation law
``A + B sin^2 lat + C sin^4 lat`` over ``t_k - t_ref``; the turned point is projected into frame ``k`` (``missing`` behind its limb
or outside its grid), moved by the frame's pointing offset and sampled with the B-spline of ``prep``.  All geometry is fp64.
One call prefilters (``sunerf_prep_spline_prefilter``, once when the frames share a shape) and enqueues one kernel for all
frames on the current stream; nothing is read back.  There is no CPU path: tests/register_reference.py is the NumPy restatement.

Out of scope: gradients, foreshortening or limb-darkening corrections of the value, height-dependent rotation off the limb,
flux-conserving (area-weighted) resampling, per-pixel angle tables, a rotation law other than the three-term one."""
from datetime import datetime
from typing import Optional, Sequence

import numpy as np
import torch

from . import lib as _l
from ._ffi import _ptr, _stream

# struct SunerfRegisterFrameDesc (include/sunerf_hip_register.h)
FRAME_DESC = np.dtype({'names': ['coefficients', 'mask', 'tx', 'ty', 'height', 'width', 'c2w', 'dt', 'shift_y', 'shift_x'],
                       'formats': ['<u8', '<u8', '<u8', '<u8', '<i4', '<i4', ('<f4', 12), '<f8', '<f8', '<f8'],
                       'offsets': [0, 8, 16, 24, 32, 36, 40, 88, 96, 104], 'itemsize': 112})
ON_DISK, OFF_DISK, BEHIND, OUTSIDE = 1, 2, 4, 8
OFF_DISK_MODES = {'missing': 0, 'closest': 1}
PROPAGATE = 1
TILE = 16
N_STATE = 4
EDGE_EPS = 2.0 ** -20
MAX_FRAMES = 65535

CARRINGTON_RATE = 2.86533e-6          # rad/s sidereal: the frame of the observers' longitudes
# sidereal (A, B, C) in rad/s
ROTATION_PRESETS = {'snodgrass': (2.851e-6, -0.343e-6, -0.474e-6), 'howard': (2.894e-6, -0.428e-6, -0.370e-6),
                    'rigid': (2.86533e-6, 0.0, 0.0)}


def rotation_rates(rotation, frame: str = 'carrington', seconds_per_dt: float = 86400.0):
    """``(A, B, C)`` in radians per unit of ``dt`` relative to the scene frame.  ``rotation``: None (nothing turns in the scene
    frame), a preset name of ``ROTATION_PRESETS`` or a sidereal triple in rad/s; ``frame='carrington'`` (the frame of the observers'
    longitudes in the project's use) subtracts ``CARRINGTON_RATE`` from ``A``, ``frame='sidereal'`` leaves the triple as it is."""
    if frame not in ('carrington', 'sidereal'):
        raise ValueError(f"frame must be 'carrington' or 'sidereal', got {frame!r}")
    seconds_per_dt = float(seconds_per_dt)
    if not (np.isfinite(seconds_per_dt) and seconds_per_dt > 0):
        raise ValueError(f'seconds_per_dt must be finite and > 0, got {seconds_per_dt}')
    if rotation is None:
        return 0.0, 0.0, 0.0
    if isinstance(rotation, str):
        if rotation not in ROTATION_PRESETS:
            raise ValueError(f'rotation must be None, a triple (A, B, C) or one of {sorted(ROTATION_PRESETS)}, got {rotation!r}')
        rotation = ROTATION_PRESETS[rotation]
    triple = np.asarray(rotation, dtype=np.float64).reshape(-1)
    if triple.shape != (3,) or not np.isfinite(triple).all():
        raise ValueError(f'rotation must be three finite numbers (A, B, C) in rad/s, got {rotation!r}')
    a = triple[0] - (CARRINGTON_RATE if frame == 'carrington' else 0.0)
    return float(a * seconds_per_dt), float(triple[1] * seconds_per_dt), float(triple[2] * seconds_per_dt)


def launch(table, n_frames, n_planes, order, c2w_ref, tx_ref, ty_ref, radius, A, B, C, off_disk, missing, flags, want_coords=True):
    """``sunerf_register_frames`` on device tensors: ``table`` uint8 [n_frames * 112] (``FRAME_DESC`` rows), ``c2w_ref`` float32 [12],
    ``tx_ref`` [W] and ``ty_ref`` [H] float64.  Returns ``(out [T, C, H, W] float32, status [T, H, W] uint8, coords [T, 2, H, W]
    float64 or None, state [T, 4] int64)``."""
    dev = table.device
    h, w = int(ty_ref.shape[0]), int(tx_ref.shape[0])
    out = torch.empty((n_frames, n_planes, h, w), dtype=torch.float32, device=dev)
    status = torch.empty((n_frames, h, w), dtype=torch.uint8, device=dev)
    coords = torch.empty((n_frames, 2, h, w), dtype=torch.float64, device=dev) if want_coords else None
    state = torch.empty((n_frames, N_STATE), dtype=torch.int64, device=dev)
    if n_frames * h * w == 0:          # the empty call writes nothing
        return out, status, coords, state.zero_()
    if int(_l.load().sunerf_register_frame_desc_bytes()) != FRAME_DESC.itemsize:
        raise _l.SunerfHipError('SunerfRegisterFrameDesc: the library and sunerf_hip.register disagree about its layout')
    _l.call(dev, 'sunerf_register_frames', _ptr(table), int(n_frames), int(n_planes), int(order), _ptr(c2w_ref), _ptr(tx_ref),
            _ptr(ty_ref), h, w, float(radius), float(A), float(B), float(C), int(off_disk), float(missing), int(flags), _ptr(out),
            _ptr(status), _ptr(coords), _ptr(state), _stream(dev))
    return out, status, coords, state


def _pose(c2w) -> np.ndarray:
    return np.asarray(torch.as_tensor(c2w)[:3, :4].reshape(-1).tolist(), dtype=np.float32)


def _time_differences(times, reference_time, seconds_per_dt):
    """``t_k - t_ref`` in units of ``dt``: numbers are taken as they are, datetimes are divided by ``seconds_per_dt``."""
    stamps = [isinstance(t, datetime) for t in list(times) + [reference_time]]
    if all(stamps):
        return [(t - reference_time).total_seconds() / float(seconds_per_dt) for t in times]
    if any(stamps):
        raise ValueError('times and reference_time must be all datetimes or all numbers')
    dts = [float(t) - float(reference_time) for t in times]
    if not np.isfinite(dts).all():
        raise ValueError('times must be finite')
    return dts


def register_frames(frames, observers: Sequence, times: Sequence, *, reference=0, reference_time=None, grid=None, rotation=None,
                    frame: str = 'carrington', seconds_per_dt: float = 86400., Rs_per_ds: float = 1., order: int = 3,
                    off_disk: str = 'closest', missing: float = float('nan'), shifts=None, bad=None, propagate: bool = False,
                    return_coords: bool = False) -> dict:
    """``frames``: ``[T, C, H, W]`` or ``[T, H, W]`` float32 on the device, or a list of ``[C, h_k, w_k]`` / ``[h_k, w_k]`` frames
    that may differ in shape.  ``observers``: one ``reprojection.Observer`` or ``View`` per frame (its pose and its pixel axes, which
    have to fit the frame).  ``times``: one per frame, numbers in units of ``dt`` (the sets' normalised time) or datetimes.

    ``reference``: the index of the frame whose observer and time the result is put on, or an ``Observer`` (then ``reference_time``
    has to be given).  ``grid``: the output grid when it is not the reference observer's own -- a plate-scale dict or a pair of axes
    ``(tx, ty)``.  ``rotation``: see :func:`rotation_rates` (None, a preset name, a sidereal triple in rad/s; ``frame``).
    ``order``: the B-spline order 0 .. 5.  ``off_disk``: ``'closest'`` samples an off-disk pixel at its line of sight's point of
    closest approach (no rotation law holds there: the surface's is used), ``'missing'`` gives it ``missing``.  ``shifts``
    ``[T, 2]``: pointing offsets ``(dy, dx)`` in pixels of each frame, what ``coalign`` reports.  ``bad`` (the frames' shape, bool or
    uint8) with ``propagate=True``: the value is NaN where a tap read a flagged or non-finite pixel; without ``propagate`` non-finite
    pixels enter as 0.

    Returns ``image`` (``[T, C, H', W']``, or ``[T, H', W']`` for frames without a plane axis), ``status`` (``[T, H', W']`` uint8:
    ``ON_DISK``, ``OFF_DISK``, ``BEHIND`` or ``OUTSIDE``), ``counts`` (``[T, 4]`` int64, pixels of each status) and with
    ``return_coords`` ``coords`` (``[T, 2, H', W']`` float64: the row and column sampled) -- all on the device."""
    from .prep import _check_order, spline_prefilter
    from .reprojection import Observer, _as_observer, _monotone, _radius
    order = _check_order(order)
    if off_disk not in OFF_DISK_MODES:
        raise ValueError(f"off_disk must be 'closest' or 'missing', got {off_disk!r}")
    A, B, C = rotation_rates(rotation, frame, seconds_per_dt)
    radius = _radius(Rs_per_ds)
    # ---- the frames
    squeeze = False
    if isinstance(frames, torch.Tensor):
        if frames.dim() not in (3, 4) or frames.dtype != torch.float32:
            raise ValueError(f'register_frames: frames must be float32 [T, C, H, W] or [T, H, W], got {frames.dtype} {tuple(frames.shape)}')
        squeeze = frames.dim() == 3
        planes = [f for f in (frames[:, None] if squeeze else frames)]
        stacked = frames[:, None] if squeeze else frames
    elif isinstance(frames, (list, tuple)):
        if not all(isinstance(f, torch.Tensor) and f.dim() in (2, 3) and f.dtype == torch.float32 for f in frames):
            raise ValueError('register_frames: a list of frames holds float32 tensors [C, h, w] or [h, w]')
        if len({f.dim() for f in frames}) > 1:
            raise ValueError('register_frames: the frames of a list all have a plane axis or none has')
        squeeze = bool(frames) and frames[0].dim() == 2
        planes = [f[None] if squeeze else f for f in frames]
        stacked = None
    else:
        raise TypeError('register_frames: frames must be a torch.Tensor or a list of them')
    n = len(planes)
    if n < 1 or n > MAX_FRAMES:
        raise ValueError(f'register_frames: 1 .. {MAX_FRAMES} frames, got {n}')
    c = int(planes[0].shape[0])
    if c < 1 or any(int(p.shape[0]) != c for p in planes):
        raise ValueError('register_frames: every frame has the same number of planes, at least one')
    if any(p.shape[1] < 1 or p.shape[2] < 1 for p in planes):
        raise ValueError('register_frames: a frame has at least 1 x 1 pixels')
    if len(observers) != n or len(times) != n:
        raise ValueError(f'register_frames: {n} frames need {n} observers and {n} times, got {len(observers)} and {len(times)}')
    observers = [_as_observer(o) for o in observers]
    # ---- the reference
    if isinstance(reference, (int, np.integer)) and not isinstance(reference, bool):
        if not 0 <= int(reference) < n:
            raise IndexError(f'reference frame {reference} of {n}')
        ref = observers[int(reference)]
        reference_time = times[int(reference)] if reference_time is None else reference_time
    else:
        ref = _as_observer(reference)
        if reference_time is None:
            raise ValueError('register_frames: a reference observer needs reference_time=')
    dts = _time_differences(times, reference_time, seconds_per_dt)
    if grid is not None:
        target = Observer.__new__(Observer)
        target.lat, target.lon, target.distance, target.center, target.c2w = ref.lat, ref.lon, ref.distance, None, ref.c2w
        if isinstance(grid, dict):
            target.grid, target.tx, target.ty = grid, None, None
        else:
            try:
                tx, ty = grid
            except (TypeError, ValueError):
                raise ValueError('grid must be a plate-scale dict or a pair of axes (tx, ty)') from None
            target.grid, target.tx, target.ty = None, tx, ty
        ref = target
    if shifts is None:
        shifts = np.zeros((n, 2))
    shifts = np.asarray(shifts.tolist() if isinstance(shifts, torch.Tensor) else shifts, dtype=np.float64)          # (never through fp32)
    if shifts.shape != (n, 2) or not np.isfinite(shifts).all():
        raise ValueError(f'shifts must be [{n}, 2] finite (dy, dx), got {shifts.shape}')
    if bad is not None:
        if not propagate:
            raise ValueError('bad flags pixels for propagate=True; without it a flagged pixel is sampled like any other')
        bad = [torch.as_tensor(b) for b in bad] if isinstance(bad, (list, tuple)) else [b for b in torch.as_tensor(bad)]
        bad = [b[None] if b.dim() == 2 else b for b in bad]
        if len(bad) != n or any(tuple(b.shape) != tuple(p.shape) for b, p in zip(bad, planes)):
            raise ValueError('bad must have the shape of the frames')
    dev = planes[0].device
    if dev.type != 'cuda' or any(p.device != dev for p in planes):
        raise _l.SunerfHipError('register_frames runs on one ROCm device (there is no CPU path)')
    # ---- axes
    tx_ref, ty_ref = ref.axes(dev)
    if not (_monotone(tx_ref) and _monotone(ty_ref)):
        raise ValueError('the reference grid\'s tx / ty must be strictly monotone axes')
    axes = []
    for k, (o, p) in enumerate(zip(observers, planes)):
        tx, ty = o.axes(dev)
        if (int(ty.shape[0]), int(tx.shape[0])) != (int(p.shape[1]), int(p.shape[2])):
            raise ValueError(f'frame {k} is {p.shape[1]} x {p.shape[2]} and its observer\'s grid {ty.shape[0]} x {tx.shape[0]}')
        if getattr(o, '_axes_monotone', None) is None:
            o._axes_monotone = _monotone(tx) and _monotone(ty)
        if not o._axes_monotone:
            raise ValueError(f'frame {k}: tx / ty must be strictly monotone axes')
        axes.append((tx, ty))
    # ---- spline coefficients: one call when the frames share a shape
    if stacked is None and len({tuple(p.shape) for p in planes}) == 1:
        stacked = torch.stack(planes)
    if stacked is not None:
        h, w = int(stacked.shape[2]), int(stacked.shape[3])
        coef, mask = spline_prefilter(stacked.reshape(n * c, h, w), order, want_mask=propagate)
        coefs = [coef[k * c:(k + 1) * c] for k in range(n)]
        masks = [mask[k * c:(k + 1) * c] for k in range(n)] if propagate else [None] * n
    else:
        pairs = [spline_prefilter(p, order, want_mask=propagate) for p in planes]
        coefs, masks = [q[0] for q in pairs], [q[1] for q in pairs]
    if bad is not None:
        masks = [(m | (b.to(dev) != 0).to(torch.uint8)).contiguous() for m, b in zip(masks, bad)]
    rows = np.zeros(n, dtype=FRAME_DESC)
    for k, row in enumerate(rows):
        row['coefficients'], row['mask'] = coefs[k].data_ptr(), masks[k].data_ptr() if masks[k] is not None else 0
        row['tx'], row['ty'] = axes[k][0].data_ptr(), axes[k][1].data_ptr()
        row['height'], row['width'] = coefs[k].shape[1], coefs[k].shape[2]
        row['c2w'] = _pose(observers[k].c2w)
        row['dt'], row['shift_y'], row['shift_x'] = dts[k], shifts[k, 0], shifts[k, 1]
    table = torch.from_numpy(rows.view(np.uint8).reshape(-1).copy()).to(dev)
    c2w_ref = torch.from_numpy(_pose(ref.c2w)).to(dev)
    out, status, coords, state = launch(table, n, c, order, c2w_ref, tx_ref, ty_ref, radius, A, B, C, OFF_DISK_MODES[off_disk],
                                        missing, PROPAGATE if propagate else 0, want_coords=return_coords)
    result = {'image': out[:, 0] if squeeze else out, 'status': status, 'counts': state}
    if return_coords:
        result['coords'] = coords
    return result


def derotate(frames, observer, times: Sequence, **kw) -> dict:
    """The single-observer convenience: a sequence that one observer took, put onto the time of frame ``reference`` (default 0)
    under ``rotation`` (default ``'snodgrass'``); ``kw`` as :func:`register_frames` takes them."""
    kw.setdefault('rotation', 'snodgrass')
    return register_frames(frames, [observer] * len(times), times, **kw)
