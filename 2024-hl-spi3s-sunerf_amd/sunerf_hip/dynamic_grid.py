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

from . import grid_field as _gf
from ._ffi import _dev, _ptr

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
        self.space = _gf.GridDescriptor(grid, n_channels, Rs_per_ds, fill, lon_mode, device)
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


# ---- wrappers: the shared code of grid_field.py with the frame times in front ---------------------------------------------------
DYNAMIC = _gf.Kind('dynamic_grid', 8, lambda desc: (_ptr(desc.frame_times), desc.n_frames, desc.time_mode),
                   lambda desc: (desc.n_frames,))


def dynamic_grid_rays(desc: DynamicGridDescriptor, values, rays_o, rays_d, z_vals, times, want_index: bool = False):
    """``raw (N, S, C)`` of the field at the samples ``o + d z`` at the rays' ``times (N, 1) | (N,)``; with ``want_index`` also
    ``(cells (N S,) int32, weights (N S, 8))`` for :func:`dynamic_grid_bwd`."""
    n, s = z_vals.shape
    values = _gf._values(desc, values)
    rays_o = _dev(rays_o, 'rays_o', (n, 3)); rays_d = _dev(rays_d, 'rays_d', (n, 3)); z_vals = _dev(z_vals, 'z_vals', (n, s))
    if not isinstance(times, torch.Tensor) or times.numel() != n:
        raise ValueError(f'times must hold one time per ray: ({n}, 1) or ({n},)')
    times = _dev(times.reshape(n), 'times', (n,))
    return _gf._gather(DYNAMIC, desc, values, (rays_o, rays_d, z_vals, times), None, (n, s), want_index)


def dynamic_grid_points(desc: DynamicGridDescriptor, values, points, want_index: bool = False):
    """``raw (M, C)`` of the field at ``points (M, 4) = (x, y, z, t)``."""
    if not isinstance(points, torch.Tensor) or points.dim() != 2 or points.shape[1] != 4:
        raise ValueError('points must be (M, 4): a grid with a time axis needs the time of every point')
    values = _gf._values(desc, values)
    points = _dev(points, 'points')
    return _gf._gather(DYNAMIC, desc, values, (None,) * 4, points, points.shape[:1], want_index)


def dynamic_grid_bwd(desc: DynamicGridDescriptor, g_raw, index, out: Optional[torch.Tensor] = None, accumulate: bool = False):
    """The adjoint of the gather: ``g_values (T, n0, n1, n2, C)`` from ``g_raw (..., C)`` and the ``index = (cells, weights)``
    the forward left.  ``out``: a contiguous fp32 tensor of that shape to write into, or with ``accumulate`` to add onto."""
    return _gf._scatter(DYNAMIC, desc, g_raw, index, out, accumulate)


def field_on_rays(desc: DynamicGridDescriptor, values, rays_o, rays_d, z_vals, times) -> torch.Tensor:
    """``raw (N, S, C)``; through autograd when gradients are enabled and ``values`` requires one."""
    return _gf._field(dynamic_grid_rays, dynamic_grid_bwd, desc, values, rays_o, rays_d, z_vals, times)


def field_on_points(desc: DynamicGridDescriptor, values, points) -> torch.Tensor:
    """``raw (M, C)``; through autograd when gradients are enabled and ``values`` requires one."""
    return _gf._field(dynamic_grid_points, dynamic_grid_bwd, desc, values, points)
