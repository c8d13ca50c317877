"""3-D volumes of the corona: the reconstructed field sampled on a grid, as physical quantities, on the
device -- what the reference draws in ``sunerf/evaluation/stash/voxel_volume.py:30-56`` from a host-side cube pushed through
``load_coords`` (``evaluation/loader.py:119-134``) -- and a weighted, masked 3-D score of two such volumes.

A grid (:class:`CartesianGrid`, :class:`Plane`, :class:`SphericalGrid`) is a host object: three fp64 axes [solar radii] and,
for the affine kinds, a frame.  ``sunerf_grid_points`` turns a range of its voxels into query points on the device, the model's
own ``forward`` answers them (the MLP kernels are not touched), ``sunerf_field_quantities`` turns the answer into emission /
density / temperature / emissivity with the Sun's interior masked, and :func:`sample_volume` drives the three tile by tile and
shards the slowest axis over the ranks of a process group like ``maps.render_columns``.  Volumes are plain C order over the
grid's axes -- ``(x, y, z)`` for a Cartesian box; the reference's ``np.meshgrid`` default (``indexing='xy'``) swaps the first
two axes of its cube.
"""
import math
from collections.abc import Sequence as _SequenceABC
from typing import Dict, Optional, Sequence, Tuple

import numpy as np
import torch

from . import lib as _l
from ._ffi import _dev, _ptr, _stream
from .maps import _gather_rows, _process_group, column_directions
from .ops import AIA_WAVELENGTHS

TILE_POINTS = 1 << 22               # default tile: 64 MiB of query points, 32 MiB of answers
LN10 = 2.302585092994046
_MODES = {'emission': 0, 'dt': 1, 'white_light': 2}
QUANTITIES = {'emission': ('emission', 'absorption'),
              'dt': ('density', 'log_temperature', 'emissivity', 'absorption'),
              'white_light': ('electron_density',)}
SUM_NAMES = ('w', 'wa', 'wb', 'wd', 'wabs', 'wd2', 'wa2', 'wb2', 'wab', 'max_abs', 'count')


# ---- grids ------------------------------------------------------------------------------------------------------------------
def _axis(values, name: str) -> torch.Tensor:
    t = torch.as_tensor(np.asarray(values.detach().cpu() if isinstance(values, torch.Tensor) else values, dtype=np.float64))
    if t.dim() != 1 or t.shape[0] < 1:
        raise ValueError(f'{name} must be a non-empty 1-d axis, got shape {tuple(t.shape)}')
    if not bool(torch.isfinite(t).all()):
        raise ValueError(f'{name} holds a value that is not finite')
    return t.contiguous()


def _vector(values, name: str) -> torch.Tensor:
    t = torch.as_tensor(np.asarray(values, dtype=np.float64)).reshape(-1)
    if t.shape[0] != 3 or not bool(torch.isfinite(t).all()):
        raise ValueError(f'{name} must be three finite numbers, got {values!r}')
    return t


def trapezoid_widths(axis: torch.Tensor) -> torch.Tensor:
    """Per-node widths of the trapezoid rule on a 1-d axis: half the distance between a node's neighbours, half an interval at
    the two ends; their sum is ``axis[-1] - axis[0]``.  An axis of one node has width 1."""
    axis = torch.as_tensor(axis, dtype=torch.float64)
    if axis.shape[0] == 1:
        return torch.ones(1, dtype=torch.float64)
    step = axis[1:] - axis[:-1]
    w = torch.zeros_like(axis)
    w[:-1] += step / 2
    w[1:] += step / 2
    return w


class _Grid:
    kind = None                     # 'affine' / 'spherical'

    def __init__(self):
        self._device_axes = {}

    @property
    def n_voxels(self) -> int:
        return self._shape3[0] * self._shape3[1] * self._shape3[2]

    def _on_device(self, dev):
        """The three axis arrays as ``sunerf_grid_points`` takes them, uploaded once per device."""
        key = str(dev)
        if key not in self._device_axes:
            self._device_axes[key] = tuple(a.to(dev) for a in self._kernel_axes())
        return self._device_axes[key]

    def __getstate__(self):
        state = self.__dict__.copy()
        state['_device_axes'] = {}
        return state


class CartesianGrid(_Grid):
    """Nodes ``X = origin + x[i] e0 + y[j] e1 + z[k] e2`` [solar radii], shape ``(len(x), len(y), len(z))``, C order.
    ``basis``: the rows ``e0, e1, e2`` (default: the identity; any three vectors give an oblique box)."""
    kind = 'affine'

    def __init__(self, x, y, z, origin=(0., 0., 0.), basis=None):
        super().__init__()
        self.axes = (_axis(x, 'x'), _axis(y, 'y'), _axis(z, 'z'))
        self.origin = _vector(origin, 'origin')
        basis = torch.eye(3, dtype=torch.float64) if basis is None else torch.as_tensor(np.asarray(basis, dtype=np.float64))
        if tuple(basis.shape) != (3, 3) or not bool(torch.isfinite(basis).all()):
            raise ValueError(f'basis must be three finite vectors (3, 3), got shape {tuple(basis.shape)}')
        self.basis = basis.contiguous()
        self._shape3 = tuple(a.shape[0] for a in self.axes)

    @classmethod
    def cube(cls, half_width: float = 1.3, n: int = 256) -> 'CartesianGrid':
        """The reference's cube (voxel_volume.py:30-33): ``n`` nodes ``linspace(-half_width, half_width)`` per axis."""
        if int(n) != n or n < 1 or not (math.isfinite(half_width) and half_width > 0):
            raise ValueError(f'cube needs n >= 1 nodes and a positive half width, got n={n!r}, half_width={half_width!r}')
        ax = torch.linspace(-float(half_width), float(half_width), int(n), dtype=torch.float64)
        return cls(ax, ax, ax)

    @property
    def shape(self) -> Tuple[int, ...]:
        return self._shape3

    def _kernel_axes(self):
        return self.axes

    def _measure(self) -> float:
        return abs(torch.linalg.det(self.basis).item())

    def cell_weights(self) -> Tuple[torch.Tensor, ...]:
        """Per-axis trapezoid widths (fp64); the voxel weight is their product.  The volume element of an oblique basis,
        ``|det basis|``, is folded into the first axis, so that the weights sum to the box's volume."""
        w = [trapezoid_widths(a) for a in self.axes]
        w[0] = w[0] * self._measure()
        return tuple(w)

    def _points3(self) -> torch.Tensor:
        a0, a1, a2 = (a.view(s) for a, s in zip(self.axes, ((-1, 1, 1, 1), (1, -1, 1, 1), (1, 1, -1, 1))))
        return self.origin + a0 * self.basis[0] + a1 * self.basis[1] + a2 * self.basis[2]      # left to right, as the kernel

    def points_f64(self, Rs_per_ds: float = 1.0) -> torch.Tensor:
        """Host fp64 restatement of the kernel: ``(*shape, 3)`` points in model units."""
        return (self._points3() / float(Rs_per_ds)).reshape(*self.shape, 3)

    def radius_f64(self) -> torch.Tensor:
        """``(*shape)`` distance from the solar centre [solar radii], the kernel's expression in fp64."""
        p = self._points3()
        return torch.sqrt((p[..., 0] * p[..., 0] + p[..., 1] * p[..., 1]) + p[..., 2] * p[..., 2]).reshape(self.shape)

    def describe(self) -> Dict[str, np.ndarray]:
        return {'grid_kind': np.array(type(self).__name__), 'axis0': self.axes[0].numpy(), 'axis1': self.axes[1].numpy(),
                'axis2': self.axes[2].numpy(), 'origin': self.origin.numpy(), 'basis': self.basis.numpy()}


class Plane(CartesianGrid):
    """A slice ``X = origin + u[i] e_u + v[j] e_v``, shape ``(len(u), len(v))``: an affine grid with ``n2 = 1``."""

    def __init__(self, origin, e_u, e_v, u, v):
        e_u, e_v = _vector(e_u, 'e_u'), _vector(e_v, 'e_v')
        super().__init__(u, v, [0.], origin, torch.stack([e_u, e_v, torch.zeros(3, dtype=torch.float64)]))

    @property
    def shape(self) -> Tuple[int, ...]:
        return self._shape3[:2]

    def _measure(self) -> float:
        return torch.linalg.cross(self.basis[0], self.basis[1]).norm().item()      # area element


class SphericalGrid(_Grid):
    """Nodes ``X = r[k] u(lat[i], lon[j])``, shape ``(n_lat, n_lon, n_r)`` -- the layout of
    ``render_heliographic_map(profiles=True)`` -- with ``u`` of ``maps.column_directions``; angles in radians, ``r`` in solar
    radii."""
    kind = 'spherical'

    def __init__(self, lat, lon, r):
        super().__init__()
        self.axes = (_axis(lat, 'lat'), _axis(lon, 'lon'), _axis(r, 'r'))
        if bool((self.axes[2] < 0).any()):
            raise ValueError('r must not be negative')
        self._shape3 = tuple(a.shape[0] for a in self.axes)

    @property
    def shape(self) -> Tuple[int, ...]:
        return self._shape3

    def _kernel_axes(self):
        lat, lon, r = self.axes
        return torch.cat([torch.cos(lat), torch.sin(lat)]), torch.cat([torch.cos(lon), torch.sin(lon)]), r

    def cell_weights(self) -> Tuple[torch.Tensor, ...]:
        """``cos(lat) dlat``, ``dlon``, ``r^2 dr`` with trapezoid widths: their product is the voxel's volume."""
        lat, lon, r = self.axes
        return torch.cos(lat) * trapezoid_widths(lat), trapezoid_widths(lon), r * r * trapezoid_widths(r)

    def points_f64(self, Rs_per_ds: float = 1.0) -> torch.Tensor:
        lat, lon, r = self.axes
        n0, n1, n2 = self._shape3
        u = column_directions(lat[:, None].expand(n0, n1), lon[None, :].expand(n0, n1))          # (n0, n1, 3)
        return (u[:, :, None, :] * r[None, None, :, None]) / float(Rs_per_ds)

    def radius_f64(self) -> torch.Tensor:
        return self.axes[2][None, None, :].expand(self._shape3).clone()

    def describe(self) -> Dict[str, np.ndarray]:
        return {'grid_kind': np.array('SphericalGrid'), 'axis0': self.axes[0].numpy(), 'axis1': self.axes[1].numpy(),
                'axis2': self.axes[2].numpy()}


def grid_from_description(d) -> _Grid:
    """The grid a :meth:`describe` dictionary (or a loaded ``.npz``) holds."""
    kind = str(d['grid_kind'])
    if kind == 'SphericalGrid':
        return SphericalGrid(d['axis0'], d['axis1'], d['axis2'])
    if kind == 'Plane':
        return Plane(d['origin'], d['basis'][0], d['basis'][1], d['axis0'], d['axis1'])
    if kind == 'CartesianGrid':
        return CartesianGrid(d['axis0'], d['axis1'], d['axis2'], d['origin'], d['basis'])
    raise ValueError(f'unknown grid kind {kind!r}')


# ---- wrappers ---------------------------------------------------------------------------------------------------------------
def _frame(grid: _Grid) -> '_l.GridFrame':
    f = _l.GridFrame()
    if grid.kind == 'affine':
        for c in range(3):
            f.origin[c] = grid.origin[c].item()
            for m in range(3):
                f.basis[m][c] = grid.basis[m, c].item()
    return f


def _check_scale(Rs_per_ds) -> float:
    Rs_per_ds = float(Rs_per_ds)
    if not (math.isfinite(Rs_per_ds) and Rs_per_ds > 0):
        raise ValueError(f'Rs_per_ds must be finite and > 0, got {Rs_per_ds}')
    return Rs_per_ds


def grid_points(grid: _Grid, Rs_per_ds: float = 1.0, time: float = 0.0, first: int = 0, count: Optional[int] = None,
                device='cuda') -> Tuple[torch.Tensor, torch.Tensor]:
    """Query points of voxels ``[first, first + count)`` of ``grid`` (C order over its axes; ``sunerf_grid_points``):
    ``points (count, 4)`` fp32 = ``(x, y, z, time)`` in model units, bit-identical to ``grid.points_f64(Rs_per_ds).float()``,
    and ``radius (count,)`` fp32 [solar radii], bit-identical to ``grid.radius_f64().float()``."""
    if not isinstance(grid, _Grid):
        raise TypeError(f'grid must be a CartesianGrid, Plane or SphericalGrid, not {type(grid).__name__}')
    Rs_per_ds = _check_scale(Rs_per_ds)
    total = grid.n_voxels
    count = total - first if count is None else count
    if first < 0 or count < 0 or first + count > total:
        raise ValueError(f'voxels [{first}, {first + count}) are outside the {total} of the grid')
    dev = torch.device(device)
    if dev.type != 'cuda':
        raise _l.SunerfHipError('grid_points: the points are made on a ROCm device (the host restatement is grid.points_f64)')
    a0, a1, a2 = grid._on_device(dev)
    points = torch.empty(count, 4, dtype=torch.float32, device=dev)
    radius = torch.empty(count, dtype=torch.float32, device=dev)
    n0, n1, n2 = grid._shape3
    _l.call(dev, 'sunerf_grid_points', 0 if grid.kind == 'affine' else 1, _ptr(a0), _ptr(a1), _ptr(a2), n0, n1, n2, _frame(grid),
            Rs_per_ds, float(time), first, count, _ptr(points), _ptr(radius), _stream(dev))
    return points, radius


def _check_r_range(r_range) -> Tuple[float, float]:
    if len(r_range) != 2:
        raise ValueError(f'r_range must be (r_in, r_out), not {tuple(r_range)!r}')
    r_in = 1.0 if r_range[0] is None else float(r_range[0])
    r_out = math.inf if r_range[1] is None else float(r_range[1])
    if math.isnan(r_in) or math.isnan(r_out) or not r_out >= r_in:
        raise ValueError(f'r_range must be (r_in, r_out) with r_out >= r_in (None: no outer mask), not {tuple(r_range)!r}')
    return r_in, r_out


def _check_quantities(kind: str, quantities, have_wavelengths: bool) -> Tuple[str, ...]:
    if kind not in QUANTITIES:
        raise ValueError(f"kind must be one of {tuple(QUANTITIES)}, not {kind!r}")
    if quantities is None:
        if kind == 'dt':
            return ('density', 'log_temperature') + (('emissivity',) if have_wavelengths else ())
        return QUANTITIES[kind]
    quantities = tuple(quantities)
    for q in quantities:
        if q not in QUANTITIES[kind]:
            raise ValueError(f'{q!r} is not a quantity of a {kind} field (those are {QUANTITIES[kind]})')
    return quantities


def _per_channel(kind: str, quantities: Sequence[str]) -> bool:
    return kind == 'dt' and ('emissivity' in quantities or 'absorption' in quantities)


def field_quantities(inferences: torch.Tensor, radius: torch.Tensor, kind: str, quantities: Optional[Sequence[str]] = None,
                     r_range=(1.0, None), fill: float = math.nan, kappa: float = 1.0,
                     wavelengths: Optional[torch.Tensor] = None, response_table=None, log_abs: Optional[torch.Tensor] = None,
                     out: Optional[Dict[str, torch.Tensor]] = None) -> Dict[str, torch.Tensor]:
    """Physical fields of a model's answer ``inferences (M, C)`` at points of ``radius (M,)`` (``sunerf_field_quantities``,
    one launch):

    - ``kind='emission'``: ``emission = exp(raw0)`` (voxel_volume.py:47), ``absorption = relu(raw1)``;
    - ``kind='dt'``: ``density = exp(relu(inf0))``, ``log_temperature = relu(inf1)`` (``inf`` with the base offsets, as the
      models return it) and, with ``wavelengths (W,)``, ``response_table = (logte (7, 101), response (7, 101))`` and ``log_abs
      (7,)``: ``emissivity (M, W) = density^2 R_w(log_temperature)`` and, on request, ``absorption (M, W) = density
      relu(log_abs_w)`` (density_temperature.py:237-263).  A wavelength that is not an AIA channel gives 0;
    - ``kind='white_light'``: ``electron_density = exp(kappa raw0)``.

    Points whose ``radius`` is outside ``r_range = (r_in, r_out)`` (``None``: 1 / no outer mask) get ``fill`` in every
    output.  ``out``: preallocated contiguous fp32 outputs to write into."""
    r_in, r_out = _check_r_range(r_range)
    quantities = _check_quantities(kind, quantities, wavelengths is not None)
    per_channel = _per_channel(kind, quantities)
    if per_channel and wavelengths is None:
        raise ValueError('field_quantities: emissivity / absorption per channel need the wavelengths (W,)')
    if not per_channel and wavelengths is not None:
        raise ValueError(f'field_quantities: the quantities {quantities} of a {kind} field take no wavelengths')
    if not isinstance(inferences, torch.Tensor) or inferences.dim() != 2:
        raise ValueError('inferences must be (M, C)')
    m, c = inferences.shape
    inferences = _dev(inferences, 'inferences')
    radius = _dev(radius, 'radius', (m,))
    dev = inferences.device
    if kind != 'white_light' and c != 2:
        raise ValueError(f'a {kind} field answers 2 values per point, got {c}')
    wl = logt = resp = la = None
    w = 0
    if per_channel:
        wl = torch.as_tensor(wavelengths).to(device=dev, dtype=torch.float32).reshape(-1).contiguous()
        w = wl.shape[0]
        if not 1 <= w <= len(AIA_WAVELENGTHS):
            raise ValueError(f'1 to {len(AIA_WAVELENGTHS)} wavelengths per call, got {w}')
        if log_abs is None:
            raise ValueError('field_quantities: the per-channel quantities need log_abs (7,)')
        la = _dev(log_abs.detach().to(dev), 'log_abs', (7,))
        if 'emissivity' in quantities:
            if response_table is None:
                raise ValueError('field_quantities: emissivity needs response_table = (logte (7, 101), response (7, 101))')
            logt = _dev(torch.as_tensor(response_table[0]).to(dev), 'response_table[0]', (7, 101))
            resp = _dev(torch.as_tensor(response_table[1]).to(dev), 'response_table[1]', (7, 101))
    res: Dict[str, torch.Tensor] = {}
    for q in quantities:
        shape = (m, w) if (kind == 'dt' and q in ('emissivity', 'absorption')) else (m,)
        if out is not None and q in out:
            res[q] = _dev(out[q], f'out[{q!r}]', shape)
            if res[q].data_ptr() != out[q].data_ptr():
                raise ValueError(f'out[{q!r}] must be contiguous')
        else:
            res[q] = torch.empty(shape, dtype=torch.float32, device=dev)
    if kind == 'dt':
        slots = (res.get('density'), res.get('log_temperature'), res.get('emissivity'), res.get('absorption'))
    elif kind == 'emission':
        slots = (res.get('emission'), res.get('absorption'), None, None)
    else:
        slots = (res.get('electron_density'), None, None, None)
    _l.call(dev, 'sunerf_field_quantities', _MODES[kind], _ptr(inferences), c, _ptr(radius), m, r_in, r_out, float(fill),
            float(kappa), _ptr(wl), w, _ptr(logt), _ptr(resp), _ptr(la), *(_ptr(s) for s in slots), _stream(dev))
    return res


def metrics_from_sums(sums: Sequence[float]) -> Dict[str, float]:
    """The statistics of :func:`volume_metrics` from its eleven sums (:data:`SUM_NAMES`), on the host in fp64.  With nothing
    counted every statistic is ``nan`` (``max_abs`` 0, ``count`` 0)."""
    s = dict(zip(SUM_NAMES, (float(v) for v in sums)))
    out = {f'sum_{k}': s[k] for k in SUM_NAMES[:9]}
    w = s['w']
    with np.errstate(all='ignore'):
        div = lambda x: float(np.float64(x) / np.float64(w))      # noqa: E731  (0 / 0 -> nan, no exception)
        cov = np.float64(s['wab']) - np.float64(s['wa']) * np.float64(s['wb']) / np.float64(w)
        var_a = np.float64(s['wa2']) - np.float64(s['wa']) ** 2 / np.float64(w)
        var_b = np.float64(s['wb2']) - np.float64(s['wb']) ** 2 / np.float64(w)
        out.update(me=div(s['wd']), mae=div(s['wabs']), rmse=float(np.sqrt(np.float64(div(s['wd2'])))),
                   pearson=float(cov / np.sqrt(var_a * var_b)), mean_a=div(s['wa']), mean_b=div(s['wb']),
                   max_abs=s['max_abs'], count=int(s['count']))
    return out


def volume_metrics(a: torch.Tensor, b: torch.Tensor, weights=None) -> Dict[str, float]:
    """Weighted, masked comparison of two scalar volumes ``a``, ``b`` (equal shape, 3-d or a 2-d plane; fp32 on the device) in
    fp64 (``sunerf_volume_metrics``: two launches, no atomics, bit-identical reruns).  ``weights``: a grid (its
    ``cell_weights()``), three per-axis vectors, or ``None`` for unit weights; a voxel's weight is their product.  A voxel
    where either volume is not finite (masked, overflowed) is left out.

    Returns the sums ``sum_w, sum_wa, sum_wb, sum_wd, sum_wabs, sum_wd2, sum_wa2, sum_wb2, sum_wab`` (``d = a - b``) and,
    derived on the host: ``me``, ``mae``, ``rmse``, ``pearson``, ``mean_a``, ``mean_b``, ``max_abs``, ``count``."""
    if not isinstance(a, torch.Tensor) or not isinstance(b, torch.Tensor) or a.shape != b.shape:
        raise ValueError('volume_metrics: a and b must be tensors of equal shape')
    if a.dim() not in (2, 3) or a.numel() == 0:
        raise ValueError(f'volume_metrics: volumes must be 3-d (or a 2-d plane) and not empty, got shape {tuple(a.shape)}')
    shape3 = tuple(a.shape) + (1,) * (3 - a.dim())
    if weights is None:
        weights = tuple(torch.ones(n, dtype=torch.float64) for n in shape3)
    elif isinstance(weights, _Grid):
        weights = weights.cell_weights()
    weights = tuple(torch.as_tensor(w, dtype=torch.float64).reshape(-1) for w in weights)
    if len(weights) != 3 or tuple(w.shape[0] for w in weights) != shape3:
        raise ValueError(f'volume_metrics: the weights {tuple(w.shape[0] for w in weights)} do not fit volumes of shape {shape3}')
    if not a.is_cuda or b.device != a.device:
        raise _l.SunerfHipError('volume_metrics: a / b must be on one ROCm device (there is no CPU path)')
    dev = a.device
    a32, b32 = a.detach().to(torch.float32).contiguous(), b.detach().to(torch.float32).contiguous()
    w0, w1, w2 = (w.to(dev).contiguous() for w in weights)
    out = torch.empty(len(SUM_NAMES), dtype=torch.float64, device=dev)
    nbytes = _l.load().sunerf_volume_metrics_workspace_bytes(a32.numel())
    ws = torch.empty(max(nbytes, 8), dtype=torch.uint8, device=dev)
    _l.call(dev, 'sunerf_volume_metrics', _ptr(a32), _ptr(b32), *shape3, _ptr(w0), _ptr(w1), _ptr(w2), _ptr(out), _ptr(ws),
            ws.numel(), _stream(dev))
    return metrics_from_sums(out.cpu().tolist())


# ---- driver -----------------------------------------------------------------------------------------------------------------
def _volume_kind(field, kind: Optional[str], model: str):
    """``(field module, kind, rendering or None)`` of what :func:`sample_volume` was handed."""
    if model not in ('fine', 'coarse'):
        raise ValueError(f"model must be 'fine' or 'coarse', not {model!r}")
    if not hasattr(field, f'{model}_model'):                      # a bare field module
        if kind not in QUANTITIES:
            raise ValueError(f'sample_volume: a bare field module needs kind= one of {tuple(QUANTITIES)}, got {kind!r}')
        return field, kind, None
    from sunerf.rendering.density_temperature import DensityTemperatureRadiativeTransfer
    from sunerf.rendering.emission import EmissionRadiativeTransfer
    from sunerf.rendering.thompson import ThompsonScattering
    found = None
    for cls, name in ((EmissionRadiativeTransfer, 'emission'), (DensityTemperatureRadiativeTransfer, 'dt'),
                      (ThompsonScattering, 'white_light')):
        if isinstance(field, cls):
            # a subclass with its own hooks (or a foreign field module) reads the model's answer its own way, as for
            # maps._kind: the caller says which
            found = None if field._hooks_replaced(cls) else name
    if kind is not None and kind not in QUANTITIES:
        raise ValueError(f'kind must be one of {tuple(QUANTITIES)}, not {kind!r}')
    if found is None and kind is None:
        raise ValueError(f'sample_volume: {type(field).__name__} does not say how its model\'s answer is read; pass kind=')
    if found is not None and kind is not None and kind != found:
        raise ValueError(f'sample_volume: {type(field).__name__} is a {found} rendering, not {kind!r}')
    return getattr(field, f'{model}_model'), found or kind, field


def _log_abs_vector(model) -> Optional[torch.Tensor]:
    if hasattr(model, 'log_abs_vector'):
        return model.log_abs_vector().detach()
    table = getattr(model, 'log_absortpion', None)
    if table is None:
        return None
    return torch.stack([table[str(w)].detach() for w in AIA_WAVELENGTHS])


@torch.no_grad()
def sample_volume(field, grid: _Grid, time, wavelengths=None, quantities: Optional[Sequence[str]] = None,
                  r_range=(1.0, None), fill: float = math.nan, model: str = 'fine', tile_points: Optional[int] = None,
                  rank: Optional[int] = None, world: Optional[int] = None, kind: Optional[str] = None,
                  response_table=None, Rs_per_ds: Optional[float] = None) -> Dict[str, object]:
    """The field of ``field`` on ``grid`` at the normalised ``time``, as physical quantities, assembled on the device.

    ``field``: a rendering module (``EmissionRadiativeTransfer``: emission, ``DensityTemperatureRadiativeTransfer`` with
    ``NeRF_DT`` / ``SimpleStar`` / ``MHDModel``: dt, ``ThompsonScattering``: white light; its ``model`` = ``'fine'`` or
    ``'coarse'`` network is sampled), or a bare field module with ``kind=`` (and ``Rs_per_ds``, default 1; ``response_table``
    for a dt field's emissivity).  Per tile of ``tile_points`` voxels: ``sunerf_grid_points``, the model's own
    ``forward(points)``, ``sunerf_field_quantities``, written into preallocated outputs.

    Returns ``inferences (*grid.shape, C)`` (the model's answer, bit-identical to ``model(points)['inferences']``), ``radius
    (*grid.shape)`` [solar radii], ``grid``, ``times``, ``Rs_per_ds``, ``kind`` and the quantities of
    :func:`field_quantities` (``(*grid.shape)`` or ``(*grid.shape, W)``), masked outside ``r_range`` with ``fill``.  A sequence
    of times gives every output but ``radius`` a leading axis.  A dt rendering needs ``wavelengths (W,)`` unless the
    ``quantities`` asked for are ``density`` / ``log_temperature`` only; the others take none.

    ``rank`` / ``world`` (default: the initialised process group, else a single process): each rank samples its
    ``shard_range`` of the slowest axis and, with ``world > 1``, every rank ends with the whole volume."""
    from .dist import shard_range
    if not isinstance(grid, _Grid):
        raise TypeError(f'grid must be a CartesianGrid, Plane or SphericalGrid, not {type(grid).__name__}')
    net, kind, rendering = _volume_kind(field, kind, model)
    r_range = _check_r_range(r_range)
    if kind == 'dt' and quantities is None and wavelengths is None and rendering is not None:
        raise ValueError('sample_volume: a density-temperature rendering needs the wavelengths (W,)')
    if kind != 'dt' and wavelengths is not None:
        raise ValueError(f'sample_volume: a {kind.replace("_", " ")} field takes no wavelengths')
    quantities = _check_quantities(kind, quantities, wavelengths is not None)
    per_channel = _per_channel(kind, quantities)
    if per_channel and wavelengths is None:
        raise ValueError('sample_volume: emissivity / absorption per channel need the wavelengths (W,)')
    if not per_channel and wavelengths is not None:
        raise ValueError(f'sample_volume: the quantities {quantities} take no wavelengths')
    if per_channel:
        heads = getattr(net, 'log_absortpion', None)
        if getattr(rendering, 'response_set', None) is not None or \
                (heads is not None and tuple(heads.keys()) != tuple(str(w) for w in AIA_WAVELENGTHS)):
            raise ValueError('sample_volume: per-channel emissivity / absorption exist for the seven AIA channels only; this model '
                             'has the channels of a response set (' + ', '.join(heads.keys() if heads is not None else ()) +
                             '): ask for density / log_temperature')
        wl_host = torch.as_tensor(np.asarray(wavelengths.detach().cpu() if isinstance(wavelengths, torch.Tensor) else wavelengths,
                                             dtype=np.float32)).reshape(-1)
        if not 1 <= wl_host.shape[0] <= len(AIA_WAVELENGTHS):
            raise ValueError(f'1 to {len(AIA_WAVELENGTHS)} wavelengths per volume, got {wl_host.shape[0]}')
        if rendering is not None and response_table is None:
            response_table = (rendering.response_logte, rendering.response_table)
        if 'emissivity' in quantities and response_table is None:
            raise ValueError('sample_volume: the emissivity of a bare dt field needs response_table=(logte, response)')
    if tile_points is not None and (int(tile_points) != tile_points or tile_points < 1):
        raise ValueError(f'tile_points must be a positive integer, not {tile_points!r}')
    scalar_time = not isinstance(time, (_SequenceABC, np.ndarray, torch.Tensor)) or (isinstance(time, torch.Tensor) and time.dim() == 0)
    times = [float(time)] if scalar_time else [float(t) for t in time]
    if not times or not all(math.isfinite(t) for t in times):
        raise ValueError(f'time must be a finite number or a non-empty sequence of them, got {time!r}')
    if Rs_per_ds is None:
        Rs_per_ds = float(rendering.Rs_per_ds) if rendering is not None else 1.0
    Rs_per_ds = _check_scale(Rs_per_ds)
    rank, world = _process_group(rank, world)
    n0, n1, n2 = grid._shape3
    if n0 < world:
        raise ValueError(f'sample_volume: the {n0} nodes of the slowest axis cannot be shared by {world} ranks')
    param = next(net.parameters(), None)
    dev = param.device if param is not None else torch.device('cuda')
    if dev.type != 'cuda':
        raise _l.SunerfHipError('sample_volume: the field module is on the CPU; volumes are sampled on a ROCm device only')

    kappa = 1.0
    if kind == 'white_light':
        kappa = float(rendering._kappa()) if rendering is not None and hasattr(rendering, '_kappa') else \
            (1.0 if hasattr(net, 'field_on_rays') else LN10)
    log_abs = _log_abs_vector(net) if per_channel else None
    if per_channel and log_abs is None:
        raise ValueError(f'sample_volume: {type(net).__name__} has no log_absortpion table for the per-channel quantities')
    wl = wl_host.to(dev) if per_channel else None
    if per_channel and 'emissivity' in quantities:
        response_table = tuple(torch.as_tensor(t).to(device=dev, dtype=torch.float32).contiguous() for t in response_table)

    per_row = n1 * n2
    row_begin, row_end = shard_range(n0, rank, world)
    v_begin, v_end = row_begin * per_row, row_end * per_row
    n_local = v_end - v_begin
    tile = int(tile_points) if tile_points is not None else TILE_POINTS
    f32 = dict(dtype=torch.float32, device=dev)
    n_wl = wl.shape[0] if per_channel else 0
    part: Dict[str, torch.Tensor] = {'radius': torch.empty(n_local, **f32)}
    for q in quantities:
        wide = kind == 'dt' and q in ('emissivity', 'absorption')
        part[q] = torch.empty((len(times), n_local) + ((n_wl,) if wide else ()), **f32)
    for ti, t in enumerate(times):
        for begin in range(v_begin, v_end, tile):
            n = min(tile, v_end - begin)
            lo = begin - v_begin
            points, radius = grid_points(grid, Rs_per_ds, t, begin, n, dev)
            answer = net(points)
            inf = (answer['inferences'] if isinstance(answer, dict) else answer).detach()
            if 'inferences' not in part:
                part['inferences'] = torch.empty((len(times), n_local, inf.shape[-1]), **f32)
            part['inferences'][ti, lo:lo + n] = inf
            if ti == 0:
                part['radius'][lo:lo + n] = radius
            field_quantities(inf.contiguous(), radius, kind, quantities, r_range, fill, kappa, wl, response_table, log_abs,
                             out={q: part[q][ti, lo:lo + n] for q in quantities})
    if world > 1:
        counts = [(e - b) * per_row for b, e in (shard_range(n0, r, world) for r in range(world))]
        gathered = {}
        for k, v in sorted(part.items()):
            if k == 'radius':
                gathered[k] = _gather_rows(v, counts)
            else:                                                  # the voxel axis first for the collective, then back
                gathered[k] = _gather_rows(v.transpose(0, 1).contiguous(), counts).transpose(0, 1).contiguous()
        part = gathered
    out: Dict[str, object] = {}
    for k, v in part.items():
        if k == 'radius':
            out[k] = v.view(grid.shape)
        else:
            v = v.view(len(times), *grid.shape, *v.shape[2:])
            out[k] = v[0] if scalar_time else v
    out.update(grid=grid, times=times[0] if scalar_time else list(times), Rs_per_ds=Rs_per_ds, kind=kind)
    if per_channel:
        out['wavelengths'] = wl
    return out


# ---- files ------------------------------------------------------------------------------------------------------------------
_META = ('grid', 'times', 'Rs_per_ds', 'kind')


def save_volume(path, volume: Dict[str, object]) -> None:
    """Writes what :func:`sample_volume` returned (tensors or numpy arrays) into one ``.npz``: every array, the grid's axes
    and frame, ``Rs_per_ds``, the times and the kind."""
    if 'grid' not in volume or not isinstance(volume['grid'], _Grid):
        raise ValueError("save_volume: the volume has no 'grid'")
    arrays = dict(volume['grid'].describe())
    for k, v in volume.items():
        if k in ('grid',):
            continue
        if k in arrays or k.startswith('axis') or k in ('grid_kind', 'origin', 'basis'):
            raise ValueError(f'save_volume: the key {k!r} is taken by the grid description')
        arrays[k] = v.detach().cpu().numpy() if isinstance(v, torch.Tensor) else np.asarray(v)
    with open(path, 'wb') as fh:                                  # (np.savez would append '.npz' to a bare path)
        np.savez(fh, **arrays)


def load_volume(path) -> Dict[str, object]:
    """The dictionary :func:`save_volume` wrote: numpy arrays, ``grid`` rebuilt, ``times`` / ``Rs_per_ds`` / ``kind`` as plain
    Python values."""
    with np.load(path, allow_pickle=False) as z:
        data = {k: z[k] for k in z.files}
    out: Dict[str, object] = {'grid': grid_from_description(data)}
    for k, v in data.items():
        if k.startswith('axis') or k in ('grid_kind', 'origin', 'basis'):
            continue
        if k == 'times':
            out[k] = v.tolist()
        elif k == 'Rs_per_ds':
            out[k] = float(v)
        elif k == 'kind':
            out[k] = str(v)
        else:
            out[k] = v
    return out
