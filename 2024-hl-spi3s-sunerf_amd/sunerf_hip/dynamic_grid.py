"""Voxel-grid field with a time axis: ``values (T, n0, n1, n2, C)`` on ``frame_times (T,)``, gathered at
the samples of a ray batch at the time of their ray, or at points ``(x, y, z, t)`` (``sunerf_dynamic_grid_fwd``), and
differentiable w.r.t. the values through the adjoint scatter (``sunerf_dynamic_grid_bwd``; include/sunerf_hip_ext.h).

The static field of :mod:`sunerf_hip.grid_field` blended linearly between its two neighbouring frames, as ``MHDModel`` blends
two simulation frames (mhd_model.py:112-124).  The backward is that module's sorted inverted index over the ids
``interval * n_cells + cell``: no floating-point atomics, bit-identical from run to run.
"""
from typing import Optional, Sequence

import numpy as np
import torch

from . import lib as _l
from .grid_field import GridDescriptor
from .ops import _dev, _ptr, _stream, _workspace

TIME_CLAMP, TIME_FILL = 0, 1
TIME_MODES = {'clamp': TIME_CLAMP, 'fill': TIME_FILL}


# ---- host-side checks --------------------------------------------------------------------------------------------------------
def check_frame_times(frame_times) -> torch.Tensor:
    """``frame_times`` as a ``(T,)`` fp64 CPU tensor: at least two, finite, strictly increasing."""
    if frame_times is None:
        raise ValueError('frame_times: a grid with a time axis needs the normalised times of its frames')
    if isinstance(frame_times, torch.Tensor):
        frame_times = frame_times.detach().cpu().numpy()
    tau = torch.as_tensor(np.asarray(frame_times, dtype=np.float64)).reshape(-1).clone()
    if tau.shape[0] < 2:
        raise ValueError(f'frame_times has {tau.shape[0]} time: a grid with a time axis needs at least two frames '
                         '(one frame is a GridField)')
    if not bool(torch.isfinite(tau).all()):
        raise ValueError('frame_times must be finite')
    if not bool((tau[1:] > tau[:-1]).all()):
        raise ValueError('frame_times must be strictly increasing')
    return tau


def time_mode(name) -> int:
    if name not in TIME_MODES:
        raise ValueError(f"time_mode must be 'clamp' or 'fill', got {name!r}")
    return TIME_MODES[name]


class DynamicGridDescriptor:
    """The kernels' view of a field with a time axis on one device: the :class:`GridDescriptor` of the shared grid and, beside
    it, the frame times as a device fp64 tensor."""

    def __init__(self, grid, n_channels: int, Rs_per_ds: float, fill: Sequence[float], lon_mode: int, frame_times, mode, device):
        self.space = GridDescriptor(grid, n_channels, Rs_per_ds, fill, lon_mode, device)
        tau = check_frame_times(frame_times)
        self.time_mode = time_mode(mode) if isinstance(mode, str) else int(mode)
        self.n_frames = int(tau.shape[0])
        self.n_ids = (self.n_frames - 1) * self.space.n_cells            # the sentinel of the forward
        if self.n_ids >= 2 ** 31 - 1:
            raise ValueError(f'{self.n_frames - 1} intervals of {self.space.n_cells} cells: the ids do not fit int32')
        self.frame_times = tau.to(self.space.device).contiguous()         # fp64, kept alive here
        self.device, self.grid, self.n_channels = self.space.device, grid, self.space.n_channels
        self.shape = (self.n_frames, *grid._shape3, self.n_channels)

    def ref(self):
        return self.space.ref()


# ---- wrappers ----------------------------------------------------------------------------------------------------------------
def _values(desc: DynamicGridDescriptor, values: torch.Tensor) -> torch.Tensor:
    values = _dev(values, 'values', desc.shape)
    if values.device.type != desc.device.type or (desc.device.index is not None and values.device.index != desc.device.index):
        raise ValueError(f'values are on {values.device}, the descriptor on {desc.device}')
    return values


def _index(total: int, want_index: bool, dev):
    if not want_index:
        return None, None
    return torch.empty(total, dtype=torch.int32, device=dev), torch.empty(total, 8, dtype=torch.float32, device=dev)


def dynamic_grid_rays(desc: DynamicGridDescriptor, values, rays_o, rays_d, z_vals, times, want_index: bool = False):
    """``raw (N, S, C)`` of the field at the samples ``o + d z`` at the rays' ``times (N, 1) | (N,)``; with ``want_index`` also
    ``(cells (N S,) int32, weights (N S, 8))`` for :func:`dynamic_grid_bwd`."""
    n, s = z_vals.shape
    values = _values(desc, values)
    rays_o = _dev(rays_o, 'rays_o', (n, 3)); rays_d = _dev(rays_d, 'rays_d', (n, 3)); z_vals = _dev(z_vals, 'z_vals', (n, s))
    if not isinstance(times, torch.Tensor) or times.numel() != n:
        raise ValueError(f'times must hold one time per ray: ({n}, 1) or ({n},)')
    times = _dev(times.reshape(n), 'times', (n,))
    dev = values.device
    raw = torch.empty(n, s, desc.n_channels, dtype=torch.float32, device=dev)
    cells, weights = _index(n * s, want_index, dev)
    _l.call(dev, 'sunerf_dynamic_grid_fwd', desc.ref(), _ptr(desc.frame_times), desc.n_frames, desc.time_mode, _ptr(values),
            _ptr(rays_o), _ptr(rays_d), _ptr(z_vals), _ptr(times), n, s, None, 0, _ptr(raw), _ptr(cells), _ptr(weights),
            _stream(dev))
    return (raw, (cells, weights)) if want_index else raw


def dynamic_grid_points(desc: DynamicGridDescriptor, values, points, want_index: bool = False):
    """``raw (M, C)`` of the field at ``points (M, 4) = (x, y, z, t)``."""
    if not isinstance(points, torch.Tensor) or points.dim() != 2 or points.shape[1] != 4:
        raise ValueError('points must be (M, 4): a grid with a time axis needs the time of every point')
    values = _values(desc, values)
    points = _dev(points, 'points')
    m = points.shape[0]
    dev = values.device
    raw = torch.empty(m, desc.n_channels, dtype=torch.float32, device=dev)
    cells, weights = _index(m, want_index, dev)
    _l.call(dev, 'sunerf_dynamic_grid_fwd', desc.ref(), _ptr(desc.frame_times), desc.n_frames, desc.time_mode, _ptr(values),
            None, None, None, None, m, 1, _ptr(points), 4, _ptr(raw), _ptr(cells), _ptr(weights), _stream(dev))
    return (raw, (cells, weights)) if want_index else raw


_bwd_workspaces = {}


def dynamic_grid_bwd(desc: DynamicGridDescriptor, g_raw, index, out: Optional[torch.Tensor] = None, accumulate: bool = False):
    """The adjoint of the gather: ``g_values (T, n0, n1, n2, C)`` from ``g_raw (..., C)`` and the ``index = (cells, weights)``
    the forward left.  ``out``: a contiguous fp32 tensor of that shape to write into, or with ``accumulate`` to add onto."""
    cells, weights = index
    total = cells.shape[0]
    dev = cells.device
    shape = desc.shape
    g_raw = _dev(g_raw.reshape(-1, g_raw.shape[-1]), 'g_raw', (total, desc.n_channels))
    if out is None:
        if accumulate:
            raise ValueError('dynamic_grid_bwd: accumulate needs out=')
        out = torch.empty(shape, dtype=torch.float32, device=dev)
    elif tuple(out.shape) != shape or out.dtype != torch.float32 or not out.is_contiguous() or out.device != dev:
        raise ValueError(f'out must be a contiguous float32 tensor of shape {shape} on {dev}')
    if total == 0:
        perm = seg = ws = None
        nbytes = 0
    else:
        ids, perm = torch.sort(cells, stable=True)
        seg = torch.searchsorted(ids, torch.arange(desc.n_ids + 1, dtype=torch.int32, device=dev))
        nbytes = _l.load().sunerf_dynamic_grid_bwd_workspace_bytes(total, desc.n_channels)
        ws = _workspace(_bwd_workspaces, dev, nbytes)
    _l.call(dev, 'sunerf_dynamic_grid_bwd', desc.ref(), desc.n_frames, _ptr(g_raw), _ptr(cells), _ptr(weights), _ptr(perm),
            _ptr(seg), total, _ptr(ws), nbytes, _ptr(out), 1 if accumulate else 0, _stream(dev))
    return out


# ---- autograd ----------------------------------------------------------------------------------------------------------------
def _values_grad(ctx, values, g_raw):
    """The gradient of a node's ``values`` input: added straight into a contiguous fp32 ``.grad`` the parameter already owns
    (``ClipAdam`` keeps them as views of one flat buffer; autograd then gets None), else a fresh tensor."""
    grad = values.grad
    if values.is_leaf and grad is not None and grad.dtype == torch.float32 and grad.is_contiguous() and \
            grad.shape == values.shape and grad.device == values.device:
        dynamic_grid_bwd(ctx.desc, g_raw, ctx.index, out=grad, accumulate=True)
        return None
    return dynamic_grid_bwd(ctx.desc, g_raw, ctx.index)


class _DynamicGridOnRays(torch.autograd.Function):
    """The field at the samples ``o + d z`` of a ray batch at the rays' times as an autograd node: ``raw (N, S, C)``,
    differentiable w.r.t. ``values`` only."""

    @staticmethod
    def forward(ctx, desc, values, rays_o, rays_d, z_vals, times):
        ctx.set_materialize_grads(False)
        if not ctx.needs_input_grad[1]:
            return dynamic_grid_rays(desc, values.detach(), rays_o, rays_d, z_vals, times)
        raw, ctx.index = dynamic_grid_rays(desc, values.detach(), rays_o, rays_d, z_vals, times, want_index=True)
        ctx.desc, ctx.values = desc, values
        return raw

    @staticmethod
    def backward(ctx, g_raw):
        if g_raw is None or not ctx.needs_input_grad[1]:
            return (None,) * 6
        return (None, _values_grad(ctx, ctx.values, g_raw.contiguous().float()), None, None, None, None)


class _DynamicGridOnPoints(torch.autograd.Function):
    """The points twin of :class:`_DynamicGridOnRays`: ``raw (M, C)`` at ``points (M, 4)``."""

    @staticmethod
    def forward(ctx, desc, values, points):
        ctx.set_materialize_grads(False)
        if not ctx.needs_input_grad[1]:
            return dynamic_grid_points(desc, values.detach(), points)
        raw, ctx.index = dynamic_grid_points(desc, values.detach(), points, want_index=True)
        ctx.desc, ctx.values = desc, values
        return raw

    @staticmethod
    def backward(ctx, g_raw):
        if g_raw is None or not ctx.needs_input_grad[1]:
            return (None,) * 3
        return (None, _values_grad(ctx, ctx.values, g_raw.contiguous().float()), None)


def field_on_rays(desc: DynamicGridDescriptor, values, rays_o, rays_d, z_vals, times) -> torch.Tensor:
    """``raw (N, S, C)``; through autograd when gradients are enabled and ``values`` requires one."""
    if torch.is_grad_enabled() and values.requires_grad:
        return _DynamicGridOnRays.apply(desc, values, rays_o.detach(), rays_d.detach(), z_vals.detach(), times.detach())
    return dynamic_grid_rays(desc, values.detach(), rays_o, rays_d, z_vals, times)


def field_on_points(desc: DynamicGridDescriptor, values, points) -> torch.Tensor:
    """``raw (M, C)``; through autograd when gradients are enabled and ``values`` requires one."""
    if torch.is_grad_enabled() and values.requires_grad:
        return _DynamicGridOnPoints.apply(desc, values, points.detach())
    return dynamic_grid_points(desc, values.detach(), points)
