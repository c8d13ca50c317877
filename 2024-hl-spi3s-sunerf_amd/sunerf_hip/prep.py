"""Observation images prepared on the device: a detector image with its header numbers becomes a north-up
view on one plate scale, scaled, normalised and clipped -- the arithmetic half of the reference's loaders
(``sunerf/data/prep/{sdo,stereo,so,psi}.py`` and ``sunerf/data/utils.py:74-125``, ``loadMapStack``), which run it on the host in a
``multiprocessing.Pool``, one image per process.  Reading FITS files and headers is not part of it.

Three HIP entry points (``include/sunerf_hip_prep.h``, ``csrc/prep.hip``) do the work: the spline prefilter, the affine resample
with its fused epilogue, and exact order statistics for the percentile clip.  The semantics are those of
``scipy.ndimage.affine_transform(order, mode='constant', cval=missing, prefilter=True)`` (scipy 1.15) in fp64, rounded to fp32
once; parity with ``sunpy.map.Map.rotate`` is not pinned.  There is no CPU path.

Geometry: the plate-scale dict of ``sunerf.evaluation.loader`` (``shape`` (H, W), ``cdelt``, ``crpix``, ``crval``; x before y, pixels
1-based) plus one optional key, ``'crota'`` (CROTA2 in radians) or ``'pc'`` (2 x 2), the FITS linear WCS

    [Tx - crval_x, Ty - crval_y] = diag(cdelt) . PC . [x - crpix_x, y - crpix_y]

with ``PC = [[cos, -sin cdelt_y / cdelt_x], [sin cdelt_x / cdelt_y, cos]]`` from ``crota``.
"""
import math
from typing import Optional, Sequence, Tuple

import numpy as np
import torch

from . import lib as _l
from ._ffi import _ptr, _stream

SEGMENT = 128                                   # SUNERF_PREP_SEGMENT: samples of a line that one thread filters
HORIZON = {0: 0, 1: 0, 2: 23, 3: 30, 4: 39, 5: 47}      # samples a segment's recursions start early / late (largest pole)
SECOND_HORIZON = {4: 10, 5: 13}                 # the same for the second, smaller pole of orders 4 and 5
MAX_ORDER = 5
MAX_RANKS = 8
STAGE_PREFILTER, STAGE_ORDER_STATISTICS = 0, 1
CLIP_RANGE, NORM, NORM_CLIP, CLIP_NEGATIVE, PROPAGATE = 1, 2, 4, 8, 16
N_PARAMS = 6
_QUARTER_TURN_EPS = 1e-15


# ---- geometry (host, fp64) ------------------------------------------------------------------------------------------------------
def _geometry(wcs: dict):
    h, w = (int(v) for v in wcs['shape'])
    cdx, cdy = (float(v) for v in wcs['cdelt'])
    cpx, cpy = (float(v) for v in wcs.get('crpix', ((w + 1) / 2., (h + 1) / 2.)))
    cvx, cvy = (float(v) for v in wcs.get('crval', (0., 0.)))
    if not (math.isfinite(cdx) and math.isfinite(cdy) and cdx != 0. and cdy != 0.):
        raise ValueError(f'cdelt must be finite and non-zero, got {(cdx, cdy)}')
    if 'pc' in wcs and 'crota' in wcs:
        raise ValueError("a geometry carries 'crota' or 'pc', not both")
    if 'pc' in wcs:
        pc = np.asarray(wcs['pc'], dtype=np.float64)
        if pc.shape != (2, 2):
            raise ValueError("'pc' must be 2 x 2")
    else:
        rota = float(wcs.get('crota', 0.))
        c, s = math.cos(rota), math.sin(rota)
        # a quarter turn is exact: cos(pi / 2) = 6e-17 would push border pixels of a pure permutation out of the frame
        if abs(c) < _QUARTER_TURN_EPS:
            c, s = 0., math.copysign(1., s)
        if abs(s) < _QUARTER_TURN_EPS:
            c, s = math.copysign(1., c), 0.
        pc = np.array([[c, -s * cdy / cdx if s else 0.], [s * cdx / cdy if s else 0., c]], dtype=np.float64)
    det = pc[0, 0] * pc[1, 1] - pc[0, 1] * pc[1, 0]
    if not (math.isfinite(det) and det != 0.):
        raise ValueError("'pc' is singular")
    return (h, w), (cdx, cdy), (cpx, cpy), (cvx, cvy), pc, det


def _pixel_matrix(wcs: dict, scale: float) -> np.ndarray:
    """``A`` (x before y) with ``p - crpix = A (p' - crpix')``: ``PC^-1 diag(scale / cdelt)``."""
    _, (cdx, cdy), _, _, pc, det = _geometry(wcs)
    inv = np.array([[pc[1, 1] / det, -pc[0, 1] / det], [-pc[1, 0] / det, pc[0, 0] / det]])
    return inv * np.array([[scale / cdx, scale / cdy]])


def _inverse_pixel_matrix(wcs: dict, scale: float) -> np.ndarray:
    """``A^-1 = diag(cdelt) PC / scale``."""
    _, (cdx, cdy), _, _, pc, _ = _geometry(wcs)
    return np.array([[cdx], [cdy]]) * pc / scale


def output_grid(wcs: dict, target_scale: Optional[float] = None, out_shape: Optional[Tuple[int, int]] = None, recenter: bool = True,
                field_of_view: Optional[Tuple[float, float]] = None) -> dict:
    """The north-up plate-scale dict (no roll key) a prepared image lives on: ``cdelt = (s, s)`` with ``s = target_scale``
    (default: the input's ``cdelt_x``), ``crval`` kept; ``recenter=True`` puts ``crval`` on the centre of the output, ``False``
    puts the input's centre pixel there.  ``out_shape`` (H', W'), or ``field_of_view = (half_x, half_y)`` in the units of
    ``cdelt`` -> ``(round(2 half_y / s), round(2 half_x / s))`` (the reference's ``center_crop``), or -- neither given -- the
    smallest frame that contains the four corners of the input."""
    (h, w), (cdx, _), (cpx, cpy), crval, _, _ = _geometry(wcs)
    s = float(cdx if target_scale is None else target_scale)
    if not (math.isfinite(s) and s > 0.):
        raise ValueError(f'target_scale must be finite and > 0, got {s}')
    inv = _inverse_pixel_matrix(wcs, s)
    centre = np.array([(w + 1) / 2., (h + 1) / 2.])
    anchor = np.array([cpx, cpy]) if recenter else centre          # the input pixel that lands on the output's centre
    if out_shape is not None and field_of_view is not None:
        raise ValueError('give out_shape or field_of_view, not both')
    if field_of_view is not None:
        half_x, half_y = (float(v) for v in field_of_view)
        out_shape = (int(round(2. * half_y / s)), int(round(2. * half_x / s)))
    elif out_shape is None:
        corners = np.array([[0.5, 0.5], [w + 0.5, 0.5], [0.5, h + 0.5], [w + 0.5, h + 0.5]])
        reach = np.abs((corners - anchor) @ inv.T).max(0)          # |p' - centre'| of the corners, x and y
        # (an extent that is a whole number of pixels up to rounding -- an identity, a quarter turn -- is not rounded up)
        out_shape = (max(1, math.ceil(2. * reach[1] - 1e-9)), max(1, math.ceil(2. * reach[0] - 1e-9)))
    nh, nw = int(out_shape[0]), int(out_shape[1])
    if nh < 1 or nw < 1:
        raise ValueError(f'empty output shape {(nh, nw)}')
    centre_out = np.array([(nw + 1) / 2., (nh + 1) / 2.])
    crpix = centre_out if recenter else centre_out - inv @ (centre - np.array([cpx, cpy]))
    return {'shape': (nh, nw), 'cdelt': (s, s), 'crpix': (float(crpix[0]), float(crpix[1])), 'crval': crval}


def affine_matrix(wcs: dict, out_grid: dict):
    """``(matrix (2, 2), offset (2,))`` fp64 in the (row, column) order of ``scipy.ndimage.affine_transform``: the 0-based source
    coordinate of the 0-based output pixel ``o`` is ``matrix @ o + offset`` -- ``p = crpix + PC^-1 diag(1 / cdelt) s (p' - crpix')``
    on 1-based pixels."""
    _, _, (cpx, cpy), _, _, _ = _geometry(wcs)
    sx, sy = (float(v) for v in out_grid['cdelt'])
    if sx != sy or 'crota' in out_grid or 'pc' in out_grid:
        raise ValueError('the output grid is north-up with one plate scale')
    nh, nw = out_grid['shape']
    opx, opy = (float(v) for v in out_grid.get('crpix', ((nw + 1) / 2., (nh + 1) / 2.)))
    a = _pixel_matrix(wcs, sx)
    off_x = (cpx - 1.) - (a[0, 0] * (opx - 1.) + a[0, 1] * (opy - 1.))
    off_y = (cpy - 1.) - (a[1, 0] * (opx - 1.) + a[1, 1] * (opy - 1.))
    return np.array([[a[1, 1], a[1, 0]], [a[0, 1], a[0, 0]]]), np.array([off_y, off_x])


# ---- the three kernels ----------------------------------------------------------------------------------------------------------
def _device_planes(image, device=None) -> torch.Tensor:
    image = torch.as_tensor(image)
    if image.dim() == 2:
        image = image[None]
    if image.dim() != 3:
        raise ValueError(f'image must be (H, W) or (C, H, W), got {tuple(image.shape)}')
    if device is not None:
        image = image.to(device)
    if not image.is_cuda:
        raise _l.SunerfHipError('image preparation runs on a ROCm device (there is no CPU path)')
    return image.detach().to(torch.float32).contiguous()


def _check_order(order) -> int:
    order = int(order)
    if not 0 <= order <= MAX_ORDER:
        raise ValueError(f'spline order must be 0 .. {MAX_ORDER}, got {order}')
    return order


def spline_prefilter(image: torch.Tensor, order: int = 3, want_mask: bool = False):
    """``(coefficients (C, H, W) fp64, mask (C, H, W) uint8 or None)`` of device planes ``(C, H, W)`` fp32:
    ``scipy.ndimage.spline_filter(order, mode='mirror')`` with non-finite pixels taken as 0 and flagged in the mask."""
    order = _check_order(order)
    image = _device_planes(image)
    dev = image.device
    c, h, w = image.shape
    coef = torch.empty(c, h, w, dtype=torch.float64, device=dev)
    mask = torch.empty(c, h, w, dtype=torch.uint8, device=dev) if want_mask else None
    if image.numel():
        nbytes = int(_l.load().sunerf_prep_workspace_bytes(STAGE_PREFILTER, c, h, w, order))
        ws = torch.empty(max(nbytes, 8) // 8, dtype=torch.float64, device=dev)
        _l.call(dev, 'sunerf_prep_spline_prefilter', _ptr(image), c, h, w, order, _ptr(coef), _ptr(mask), _ptr(ws), nbytes,
                _stream(dev))
    return coef, mask


def affine_resample(coefficients: torch.Tensor, matrix, offset, out_shape, order: int = 3, missing: float = 0.,
                    params: Optional[torch.Tensor] = None, flags: int = 0, mask: Optional[torch.Tensor] = None) -> torch.Tensor:
    """``(C, H', W')`` fp32 from prefiltered planes: ``scipy.ndimage.affine_transform(matrix, offset, mode='constant',
    cval=missing)`` followed per plane by the epilogue that ``flags`` and ``params (C, 6)`` fp64 = lo, hi, factor, vmin, vmax, 0
    describe (``include/sunerf_hip_prep.h``).  ``params=None``: factor 1."""
    order = _check_order(order)
    if coefficients.dim() != 3 or coefficients.dtype != torch.float64 or not coefficients.is_cuda:
        raise ValueError('coefficients must be (C, H, W) fp64 on a ROCm device')
    coefficients = coefficients.contiguous()
    dev = coefficients.device
    c, h, w = coefficients.shape
    m = np.asarray(matrix, dtype=np.float64).reshape(2, 2)
    o = np.asarray(offset, dtype=np.float64).reshape(2)
    nh, nw = int(out_shape[0]), int(out_shape[1])
    if params is None:
        params = torch.zeros(c, N_PARAMS, dtype=torch.float64, device=dev)
        params[:, 2] = 1.
    if tuple(params.shape) != (c, N_PARAMS) or params.dtype != torch.float64 or params.device != dev:
        raise ValueError(f'params must be ({c}, {N_PARAMS}) fp64 on the device of the coefficients')
    if flags & PROPAGATE:
        if mask is None or tuple(mask.shape) != (c, h, w) or mask.dtype != torch.uint8 or mask.device != dev:
            raise ValueError('PROPAGATE needs the non-finite mask of the prefilter')
        mask = mask.contiguous()
    out = torch.empty(c, nh, nw, dtype=torch.float32, device=dev)
    _l.call(dev, 'sunerf_prep_affine_resample', _ptr(coefficients), _ptr(mask), c, h, w, order, float(m[0, 0]), float(m[0, 1]),
            float(m[1, 0]), float(m[1, 1]), float(o[0]), float(o[1]), float(missing), _ptr(params.contiguous()), int(flags), nh, nw,
            _ptr(out), _stream(dev))
    return out


def order_statistics(x: torch.Tensor, ranks: torch.Tensor):
    """``(values (C, R) fp32, nan_count (C,) int64)``: the elements of 0-based rank ``ranks (C, R)`` (int64, on the device) of
    every plane of ``x (C, ...)`` in ascending order with NaNs left out; NaN for a rank outside the valid ones."""
    if not x.is_cuda:
        raise _l.SunerfHipError('order statistics run on a ROCm device (there is no CPU path)')
    x = x.detach().to(torch.float32).contiguous()
    c = x.shape[0]
    x = x.reshape(c, -1)
    n = x.shape[1]
    dev = x.device
    ranks = torch.as_tensor(ranks, dtype=torch.int64).to(dev).reshape(c, -1).contiguous()
    r = ranks.shape[1]
    if not 1 <= r <= MAX_RANKS:
        raise ValueError(f'1 .. {MAX_RANKS} ranks per plane, got {r}')
    if n >= 2 ** 31:
        raise ValueError('a plane holds fewer than 2^31 values')
    values = torch.full((c, r), float('nan'), dtype=torch.float32, device=dev)
    nan_count = torch.zeros(c, dtype=torch.int64, device=dev)
    if c and n:
        nbytes = int(_l.load().sunerf_prep_workspace_bytes(STAGE_ORDER_STATISTICS, c, n, 1, r))
        ws = torch.empty((nbytes + 7) // 8, dtype=torch.int64, device=dev)
        _l.call(dev, 'sunerf_prep_order_statistics', _ptr(x), c, n, _ptr(ranks), r, _ptr(values), _ptr(nan_count), _ptr(ws), nbytes,
                _stream(dev))
    return values, nan_count


def plane_quantiles(x: torch.Tensor, q) -> torch.Tensor:
    """``np.percentile(plane, q)`` (numpy's default, linear definition) of every plane of ``x (C, ...)`` over its values that are
    not NaN: ``(C, len(q))`` fp32 on the device, ``q`` in percent.  The two order statistics around each percentile are exact
    (``order_statistics``); their lerp is fp64 and rounded to fp32 once.  A plane without a valid value gives NaN.  Nothing is
    copied to the host."""
    if not x.is_cuda:
        raise _l.SunerfHipError('plane_quantiles runs on a ROCm device (there is no CPU path)')
    qs = [float(v) for v in np.atleast_1d(np.asarray(q, dtype=np.float64))]
    if not qs or any(not 0. <= v <= 100. for v in qs):
        raise ValueError(f'percentiles lie in [0, 100], got {qs}')
    if 2 * len(qs) > MAX_RANKS:
        raise ValueError(f'at most {MAX_RANKS // 2} percentiles per call')
    c = x.shape[0]
    flat = x.detach().reshape(c, -1)
    dev = flat.device
    n_valid = (flat.shape[1] - torch.isnan(flat).sum(1)).to(torch.float64)                      # (C,)
    pos = (n_valid[:, None] - 1.) * (torch.tensor(qs, dtype=torch.float64, device=dev) / 100.)[None]     # numpy: (n - 1) * (q / 100)
    lo = torch.floor(pos)
    hi = torch.minimum(lo + 1., (n_valid[:, None] - 1.).expand_as(lo))
    ranks = torch.stack([lo, hi], -1).reshape(c, -1).to(torch.int64)
    values, _ = order_statistics(flat, ranks)
    a, b = values.reshape(c, len(qs), 2).double().unbind(-1)
    t = pos - lo
    # numpy's _lerp: a + (b - a) t, taken from the other end for t >= 0.5 (an infinite neighbour gives NaN, as it does there)
    return torch.where(t >= 0.5, b - (b - a) * (1. - t), a + (b - a) * t).to(torch.float32)


# ---- the whole preparation ------------------------------------------------------------------------------------------------------
def _per_plane(value, c: int, what: str, dev) -> torch.Tensor:
    if torch.is_tensor(value):
        t = value.detach().to(device=dev, dtype=torch.float64).reshape(-1)
    else:
        t = torch.tensor(np.atleast_1d(np.asarray(value, dtype=np.float64)).reshape(-1), dtype=torch.float64, device=dev)
    if t.numel() == 1:
        t = t.expand(c)
    if t.numel() != c:
        raise ValueError(f'{what}: a scalar or one value per plane ({c}), got {t.numel()}')
    return t


def prepare_image(image, wcs: dict, *, target_scale: Optional[float] = None, out_shape: Optional[Tuple[int, int]] = None,
                  field_of_view: Optional[Tuple[float, float]] = None, recenter: bool = True, order: int = 3, missing: float = 0.,
                  factor=1., norm: Optional[Sequence] = None, clip_negative: bool = True, clip_to_input_range: bool = True,
                  nan_policy: str = 'zero', percentile_clip: Optional[float] = None, device=None):
    """``(image (C, H', W') fp32 on the device, grid dict)``: ``image`` ((H, W) or (C, H, W), device or host) with the geometry
    ``wcs`` rolled to north, recentred and resampled to ``target_scale`` on ``output_grid(wcs, target_scale, out_shape, recenter,
    field_of_view)`` with a spline of ``order``; outside the detector ``missing``.  Then per plane, fused into the resample:

    1. ``clip_to_input_range``: clamp to the finite input's [min, max] joined with ``missing`` (sunpy's ``clip=True``);
    2. ``* factor`` (a scalar or one per plane; the caller passes correction / exposure);
    3. ``norm = (vmin, vmax)`` or ``(vmin, vmax, clip)``, scalars or one per plane: ``(v - vmin) / (vmax - vmin)``, ``clip``
       clamps that to [0, 1];
    4. ``clip_negative``: ``v < 0 -> 0``;
    5. ``nan_policy``: ``'zero'`` -- non-finite input pixels enter the filter as 0 and a non-finite result becomes 0, the output
       is finite; ``'propagate'`` -- the same, and an output pixel whose ``(order + 1)^2`` taps read a non-finite input pixel is
       NaN (``ObservationSet`` then drops the ray).

    ``percentile_clip = p`` finally clips every plane at its ``(100 - p)``-th percentile (``plane_quantiles``)."""
    order = _check_order(order)
    if nan_policy not in ('zero', 'propagate'):
        raise ValueError(f"nan_policy must be 'zero' or 'propagate', got {nan_policy!r}")
    planes = _device_planes(image, device)
    dev = planes.device
    c, h, w = planes.shape
    if (h, w) != tuple(int(v) for v in wcs['shape']):
        raise ValueError(f"geometry shape {tuple(wcs['shape'])} is not the image's {(h, w)}")
    if h < 1 or w < 1 or c < 1:
        raise ValueError(f'empty image {tuple(planes.shape)}')
    grid = output_grid(wcs, target_scale, out_shape, recenter, field_of_view)
    matrix, offset = affine_matrix(wcs, grid)
    propagate = nan_policy == 'propagate'
    coef, mask = spline_prefilter(planes, order, want_mask=propagate)

    flags = (CLIP_NEGATIVE if clip_negative else 0) | (PROPAGATE if propagate else 0)
    params = torch.zeros(c, N_PARAMS, dtype=torch.float64, device=dev)
    params[:, 2] = _per_plane(factor, c, 'factor', dev)
    if clip_to_input_range:
        flags |= CLIP_RANGE
        finite = torch.isfinite(planes)
        inf = torch.tensor(float('inf'), dtype=torch.float32, device=dev)
        lo = torch.where(finite, planes, inf).amin((1, 2)).double()
        hi = torch.where(finite, planes, -inf).amax((1, 2)).double()
        params[:, 0] = torch.clamp(lo, max=float(missing))
        params[:, 1] = torch.clamp(hi, min=float(missing))
    if norm is not None:
        if len(norm) not in (2, 3):
            raise ValueError('norm is (vmin, vmax) or (vmin, vmax, clip)')
        flags |= NORM | (NORM_CLIP if len(norm) == 3 and norm[2] else 0)
        params[:, 3] = _per_plane(norm[0], c, 'norm vmin', dev)
        params[:, 4] = _per_plane(norm[1], c, 'norm vmax', dev)
    out = affine_resample(coef, matrix, offset, grid['shape'], order, missing, params, flags, mask)
    if percentile_clip is not None:
        threshold = plane_quantiles(out, 100. - float(percentile_clip))              # (C, 1)
        out = torch.where(out > threshold[:, :, None], threshold[:, :, None].expand_as(out), out)      # NaN pixels stay NaN
    return out, grid
