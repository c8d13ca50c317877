"""Voxel-grid field: values on the nodes of a grid of :mod:`sunerf_hip.volume`, gathered at the samples
of a ray batch or at free-standing points (``sunerf_grid_field_fwd``) and differentiable w.r.t. the values through the adjoint
scatter (``sunerf_grid_field_bwd``).  It generalises the trilinear gather of ``MHDModel`` (mhd_model.py:45-75; csrc/mhd.hip)
to any grid and channel count and gives it the gradient a fit needs.

The backward uses no floating-point atomics: the forward leaves every sample's flattened cell id, a stable ``torch.sort`` of
the ids gives the inverted index (permutation + segment starts), and one thread per node adds the segments of its adjacent
cells in a fixed order -- bit-identical from run to run.

The call of the forward, the backward with its sort and the autograd node are written once, for a :class:`Kind`; the field
with a time axis (:mod:`sunerf_hip.dynamic_grid`, section 8l) is the second kind.
"""
import ctypes
import math
from typing import Callable, NamedTuple, Optional, Sequence

import torch

from . import lib as _l
from ._ffi import _dev, _ptr, _stream, _workspace
from .volume import CartesianGrid, Plane, _Grid

MAX_CHANNELS = 4
LON_PATCH, LON_CLOSED, LON_OPEN = 0, 1, 2
LON_NAMES = {LON_PATCH: 'patch', LON_CLOSED: 'closed', LON_OPEN: 'open'}
TWO_PI = 2.0 * math.pi
_SEAM_TOLERANCE = 1e-9          # a longitude axis closes when its span is 2 pi to this relative accuracy


class GridFieldDesc(ctypes.Structure):
    """``SunerfGridFieldDesc`` (include/sunerf_hip.h)."""
    _fields_ = [('axis', ctypes.c_void_p * 3), ('n', ctypes.c_int * 3), ('n_channels', ctypes.c_int), ('kind', ctypes.c_int),
                ('lon_mode', ctypes.c_int), ('lo', ctypes.c_double * 3), ('hi', ctypes.c_double * 3),
                ('inverse', (ctypes.c_double * 3) * 3), ('origin', ctypes.c_double * 3), ('Rs_per_ds', ctypes.c_double),
                ('fill', ctypes.c_float * 4)]


# ---- host-side checks --------------------------------------------------------------------------------------------------------
def check_grid(grid) -> None:
    """A grid a field can live on: three axes of at least two strictly increasing nodes each (a ``Plane`` has no cell)."""
    if not isinstance(grid, _Grid):
        raise TypeError(f'grid must be a CartesianGrid or SphericalGrid, not {type(grid).__name__}')
    if isinstance(grid, Plane):
        raise ValueError('a Plane has no cells: a grid field needs three axes of at least two nodes')
    for k, axis in enumerate(grid.axes):
        if axis.shape[0] < 2:
            raise ValueError(f'axis {k} of the grid has {axis.shape[0]} node: a grid field needs at least two per axis')
        if not bool((axis[1:] > axis[:-1]).all()):
            raise ValueError(f'axis {k} of the grid is not strictly increasing')
    if grid.kind == 'affine' and abs(torch.linalg.det(grid.basis).item()) == 0.0:
        raise ValueError('the basis of the grid is singular')


def longitude_mode(grid, periodic_lon: Optional[bool] = None) -> int:
    """How the longitude axis of ``grid`` is read (``LON_*``; an affine grid has none: ``LON_PATCH``).

    - ``LON_CLOSED``: the axis spans 2 pi, its last node repeats the first (``linspace(-pi, pi, n)``);
    - ``LON_OPEN``: the span is shorter and the field is periodic (``endpoint=False``): a wrap cell joins the last node to the
      first + 2 pi;
    - ``LON_PATCH``: a limited span, outside it the fill.

    ``periodic_lon=None`` decides by the axis: closed when it spans 2 pi, open when it is uniform and one more step would close
    it, a patch otherwise.  ``True`` asks for a periodic reading of any axis shorter than 2 pi, ``False`` for a patch."""
    if grid.kind != 'spherical':
        if periodic_lon:
            raise ValueError('periodic_lon: only a SphericalGrid has a longitude axis')
        return LON_PATCH
    lon = grid.axes[1]
    span = (lon[-1] - lon[0]).item()
    if span > TWO_PI * (1 + _SEAM_TOLERANCE):
        raise ValueError(f'the longitude axis spans {span} > 2 pi')
    closed = abs(span - TWO_PI) <= TWO_PI * _SEAM_TOLERANCE
    if periodic_lon is None:
        step = span / (lon.shape[0] - 1)
        uniform = bool(((lon[1:] - lon[:-1]) - step).abs().max().item() <= 1e-9 * step)
        periodic_lon = closed or (uniform and abs(span + step - TWO_PI) <= TWO_PI * _SEAM_TOLERANCE)
    if not periodic_lon:
        return LON_PATCH
    return LON_CLOSED if closed else LON_OPEN


def n_cells(grid, lon_mode: int) -> int:
    n0, n1, n2 = grid._shape3
    return (n0 - 1) * (n1 if lon_mode == LON_OPEN else n1 - 1) * (n2 - 1)


class GridDescriptor:
    """The host descriptor of a grid field on one device: the ctypes record and the device axes it points to."""

    def __init__(self, grid, n_channels: int, Rs_per_ds: float, fill: Sequence[float], lon_mode: int, device):
        check_grid(grid)
        if not 1 <= int(n_channels) <= MAX_CHANNELS:
            raise ValueError(f'a grid field holds 1 to {MAX_CHANNELS} channels per node, got {n_channels}')
        Rs_per_ds = float(Rs_per_ds)
        if not (math.isfinite(Rs_per_ds) and Rs_per_ds > 0):
            raise ValueError(f'Rs_per_ds must be finite and > 0, got {Rs_per_ds}')
        fill = [float(v) for v in fill]
        if len(fill) != n_channels:
            raise ValueError(f'fill has {len(fill)} values for {n_channels} channels')
        self.device = torch.device(device)
        self.grid, self.n_channels, self.lon_mode = grid, int(n_channels), int(lon_mode)
        self.n_ids = self.n_cells = n_cells(grid, lon_mode)                           # n_ids: the sentinel of the forward
        self.shape = (*grid._shape3, self.n_channels)                                 # of `values`
        self.axes = tuple(a.to(self.device).contiguous() for a in grid.axes)          # fp64, kept alive here
        d = GridFieldDesc()
        for k in range(3):
            d.axis[k] = self.axes[k].data_ptr() if self.device.type == 'cuda' else None
            d.n[k] = grid.axes[k].shape[0]
            d.lo[k], d.hi[k] = grid.axes[k][0].item(), grid.axes[k][-1].item()
        d.n_channels = int(n_channels)
        d.kind = 0 if grid.kind == 'affine' else 1
        d.lon_mode = int(lon_mode)
        if grid.kind == 'affine':
            inverse = affine_inverse(grid)
            for m in range(3):
                d.origin[m] = grid.origin[m].item()
                for c in range(3):
                    d.inverse[m][c] = inverse[m, c].item()
        d.Rs_per_ds = Rs_per_ds
        for c, v in enumerate(fill):
            d.fill[c] = v
        self.record = d

    def ref(self):
        return ctypes.byref(self.record)


def affine_inverse(grid: CartesianGrid) -> torch.Tensor:
    """(3, 3) fp64 ``M`` with ``u = M (X - origin)``: the inverse of the node map ``X = origin + u_0 e_0 + u_1 e_1 + u_2 e_2``.
    The identity basis gives the identity exactly."""
    if bool((grid.basis == torch.eye(3, dtype=torch.float64)).all()):
        return torch.eye(3, dtype=torch.float64)
    return torch.linalg.inv(grid.basis.T.contiguous())


# ---- wrappers ----------------------------------------------------------------------------------------------------------------
class Kind(NamedTuple):
    """What tells the static field from the one with a time axis (:mod:`sunerf_hip.dynamic_grid`) in the shared code below.  The
    descriptors carry the rest: ``shape``, of the values, and ``n_ids``, the sentinel of the forward."""
    label: str                  # the entry points are sunerf_<label>_fwd, _bwd and _bwd_workspace_bytes
    width: int                  # weights per sample: 4 + 2 x the frames a sample touches
    fwd_lead: Callable          # desc -> the arguments of _fwd between the descriptor and `values`
    bwd_lead: Callable          # desc -> the arguments of _bwd between the descriptor and `g_raw`


STATIC = Kind('grid_field', 6, lambda desc: (), lambda desc: ())


def _values(desc, values: torch.Tensor) -> torch.Tensor:
    values = _dev(values, 'values', desc.shape)
    if values.device.type != desc.device.type or (desc.device.index is not None and values.device.index != desc.device.index):
        raise ValueError(f'values are on {values.device}, the descriptor on {desc.device}')
    return values


def _index(total: int, width: int, dev):
    return torch.empty(total, dtype=torch.int32, device=dev), torch.empty(total, width, dtype=torch.float32, device=dev)


def _gather(kind: Kind, desc, values, rays, points, dims, want_index: bool):
    """One forward of checked device tensors.  ``rays``: what the entry point takes between ``values`` and the sizes, all None
    in points mode; ``dims``: ``(N, S)``, or ``(M,)`` with ``points (M, stride)``.  Returns ``raw (*dims, C)``, with
    ``want_index`` also ``(cells, weights)``."""
    dev = values.device
    n, s = dims if points is None else (dims[0], 1)
    raw = torch.empty(*dims, desc.n_channels, dtype=torch.float32, device=dev)
    cells, weights = _index(n * s, kind.width, dev) if want_index else (None, None)
    _l.call(dev, f'sunerf_{kind.label}_fwd', desc.ref(), *kind.fwd_lead(desc), _ptr(values), *(_ptr(r) for r in rays), n, s,
            _ptr(points), 0 if points is None else points.shape[1], _ptr(raw), _ptr(cells), _ptr(weights), _stream(dev))
    return (raw, (cells, weights)) if want_index else raw


_bwd_workspaces = {}            # per entry point, then per device and stream: the two kinds share no buffer


def _scatter(kind: Kind, desc, g_raw, index, out, accumulate):
    """The adjoint of :func:`_gather`: ``g_values`` of ``desc.shape``.  A stable sort of the ids is the permutation,
    ``searchsorted`` of the sorted ids the start of every id's segment in it."""
    cells, weights = index
    total = cells.shape[0]
    dev = cells.device
    shape = desc.shape
    g_raw = _dev(g_raw.reshape(-1, g_raw.shape[-1]), 'g_raw', (total, desc.n_channels))
    if out is None:
        if accumulate:
            raise ValueError(f'{kind.label}_bwd: accumulate needs out=')
        out = torch.empty(shape, dtype=torch.float32, device=dev)
    elif tuple(out.shape) != shape or out.dtype != torch.float32 or not out.is_contiguous() or out.device != dev:
        raise ValueError(f'out must be a contiguous float32 tensor of shape {shape} on {dev}')
    if total == 0:
        perm = seg = ws = None
        nbytes = 0
    else:
        ids, perm = torch.sort(cells, stable=True)
        seg = torch.searchsorted(ids, torch.arange(desc.n_ids + 1, dtype=torch.int32, device=dev))
        nbytes = getattr(_l.load(), f'sunerf_{kind.label}_bwd_workspace_bytes')(total, desc.n_channels)
        ws = _workspace(_bwd_workspaces.setdefault(kind.label, {}), dev, nbytes)
    _l.call(dev, f'sunerf_{kind.label}_bwd', desc.ref(), *kind.bwd_lead(desc), _ptr(g_raw), _ptr(cells), _ptr(weights),
            _ptr(perm), _ptr(seg), total, _ptr(ws), nbytes, _ptr(out), 1 if accumulate else 0, _stream(dev))
    return out


def grid_field_rays(desc: GridDescriptor, values, rays_o, rays_d, z_vals, want_index: bool = False):
    """``raw (N, S, C)`` of the field at the samples ``o + d z``; with ``want_index`` also ``(cells (N S,) int32, weights
    (N S, 6))`` for :func:`grid_field_bwd`."""
    n, s = z_vals.shape
    values = _values(desc, values)
    rays_o = _dev(rays_o, 'rays_o', (n, 3)); rays_d = _dev(rays_d, 'rays_d', (n, 3)); z_vals = _dev(z_vals, 'z_vals', (n, s))
    return _gather(STATIC, desc, values, (rays_o, rays_d, z_vals), None, (n, s), want_index)


def grid_field_points(desc: GridDescriptor, values, points, want_index: bool = False):
    """``raw (M, C)`` of the field at ``points (M, 3 | 4)`` (a time column is ignored: the field is static)."""
    if not isinstance(points, torch.Tensor) or points.dim() != 2 or points.shape[1] not in (3, 4):
        raise ValueError('points must be (M, 3) or (M, 4)')
    values = _values(desc, values)
    points = _dev(points, 'points')
    return _gather(STATIC, desc, values, (None,) * 3, points, points.shape[:1], want_index)


def grid_field_bwd(desc: GridDescriptor, g_raw, index, out: Optional[torch.Tensor] = None, accumulate: bool = False):
    """The adjoint of the gather: ``g_values (n0, n1, n2, C)`` from ``g_raw (..., C)`` and the ``index = (cells, weights)`` the
    forward left.  ``out``: a contiguous fp32 tensor of that shape to write into, or with ``accumulate`` to add onto."""
    return _scatter(STATIC, desc, g_raw, index, out, accumulate)


# ---- autograd ----------------------------------------------------------------------------------------------------------------
class _FieldGather(torch.autograd.Function):
    """A grid field of either kind, on rays or at points, as an autograd node: ``gather(desc, values, *where)``, differentiable
    w.r.t. ``values`` only through ``scatter`` (not the rays or z: the resampled z is detached in the reference,
    sampling.py:120).  No index and no extra work when nothing needs a gradient."""

    @staticmethod
    def forward(ctx, gather, scatter, desc, values, *where):
        ctx.set_materialize_grads(False)
        ctx.n_inputs = 4 + len(where)
        if not ctx.needs_input_grad[3]:
            return gather(desc, values.detach(), *where)
        raw, ctx.index = gather(desc, values.detach(), *where, want_index=True)
        ctx.scatter, ctx.desc, ctx.values = scatter, desc, values
        return raw

    @staticmethod
    def backward(ctx, g_raw):
        grads = [None] * ctx.n_inputs
        if g_raw is not None and ctx.needs_input_grad[3]:
            grads[3] = _values_grad(ctx, g_raw.contiguous().float())
        return tuple(grads)


def _values_grad(ctx, g_raw):
    """The gradient of the node's ``values`` input: added straight into a contiguous fp32 ``.grad`` the parameter already owns
    (``ClipAdam`` keeps them as views of one flat buffer; autograd then gets None), else a fresh tensor."""
    values = ctx.values
    grad = values.grad
    if values.is_leaf and grad is not None and grad.dtype == torch.float32 and grad.is_contiguous() and \
            grad.shape == values.shape and grad.device == values.device:
        ctx.scatter(ctx.desc, g_raw, ctx.index, out=grad, accumulate=True)
        return None
    return ctx.scatter(ctx.desc, g_raw, ctx.index)


def _field(gather, scatter, desc, values, *where) -> torch.Tensor:
    """``gather(desc, values, *where)``; through autograd when gradients are enabled and ``values`` requires one."""
    if torch.is_grad_enabled() and values.requires_grad:
        return _FieldGather.apply(gather, scatter, desc, values, *(w.detach() for w in where))
    return gather(desc, values.detach(), *where)


def field_on_rays(desc: GridDescriptor, values, rays_o, rays_d, z_vals) -> torch.Tensor:
    """``raw (N, S, C)``; through autograd when gradients are enabled and ``values`` requires one."""
    return _field(grid_field_rays, grid_field_bwd, desc, values, rays_o, rays_d, z_vals)


def field_on_points(desc: GridDescriptor, values, points) -> torch.Tensor:
    """``raw (M, C)``; through autograd when gradients are enabled and ``values`` requires one."""
    return _field(grid_field_points, grid_field_bwd, desc, values, points)
