"""A field that is a plain array of values on a grid: rendered through the same line-of-sight
integrals as the MLP and **fitted** through them -- classical rotational tomography as the non-ML baseline -- or baked from a
trained model (``sample_volume`` -> :meth:`GridField.from_volume`) so that a frame skips the network.

The reference has two grid interpolators, both forward-only and on the CPU: ``MHDModel``'s scipy
``RegularGridInterpolator`` (sunerf/model/mhd_model.py:45-75) and the cube of ``evaluation/stash/voxel_volume.py:30-56``,
which it only draws.  ``GridField`` is their device form for any grid of :mod:`sunerf_hip.volume` with the adjoint
(``csrc/grid_field.hip``), ``GridFieldDT`` carries the density-temperature head exactly as ``MHDModel`` does.

``DynamicGridField`` gives the grid a time axis: ``T`` frames on one grid, blended linearly in time as
``MHDModel`` blends its simulation frames (mhd_model.py:112-124) -- time-dependent tomography with a temporal regulariser, and
baked sequences (``csrc/dynamic_grid.hip``).
"""
import math

import numpy as np
import torch
from torch import nn

from sunerf.model.model import absorption_scalars
from sunerf_hip import dynamic_grid as _dg
from sunerf_hip import grid_field as _gf
from sunerf_hip import ops

EMPTY = -50.0                   # exp(-50) ~ 2e-22: "nothing here" for a channel that is exponentiated


def default_fill(d_output: int):
    """What a sample outside the grid answers when no ``fill`` is given: ``(-50, 0, 0, 0)[:d_output]``.

    - emission (``d_output=2``: ln emission, absorption logit): ``exp(raw0) ~ 0``, ``relu(raw1) = 0`` -- empty space;
    - white light (``d_output=1``: ln rho): ``exp(-50) ~ 0`` electrons;
    - density / temperature: :class:`GridFieldDT` has its own default, ``MHDModel``'s."""
    return (EMPTY, 0.0, 0.0, 0.0)[:d_output]


def _initial_values(init, shape, d_output):
    """``values`` of ``shape`` from ``init``: ``None`` (zeros), a number, ``d_output`` numbers, an array of the last four axes of
    ``shape`` (one frame, repeated over a leading time axis) or the full array."""
    if init is None:
        return torch.zeros(shape, dtype=torch.float32)
    init = torch.as_tensor(np.asarray(init.detach().cpu() if isinstance(init, torch.Tensor) else init), dtype=torch.float32)
    if init.dim() <= 1 and init.numel() in (1, d_output):
        return init.reshape(-1).expand(shape).clone()
    if tuple(init.shape) in (tuple(shape), tuple(shape[-4:])):
        return init.expand(shape).clone()
    raise ValueError(f'init has shape {tuple(init.shape)}; expected a number, {d_output} numbers or {tuple(shape)}')


class GridField(nn.Module):
    """``values (n0, n1, n2, C)`` on the nodes of ``grid`` (a ``CartesianGrid`` or ``SphericalGrid`` of
    :mod:`sunerf_hip.volume`; C order over its axes, the layout of ``sample_volume``'s ``inferences``), interpolated
    trilinearly at points given in model units (``X = p * Rs_per_ds`` solar radii).  The field is static: times are ignored
    (:class:`DynamicGridField` has a time axis).

    ``d_output``: channels per node, 1 to 4; ``d_input`` is accepted (the renderings force both into ``model_config``) and
    must be 3 or 4.  ``init``: ``None`` (zeros), a number, ``d_output`` numbers, or a full array.  ``fill (C,)``: the answer
    outside the grid (:func:`default_fill`).  ``periodic_lon``: how a ``SphericalGrid``'s longitude axis is read
    (:func:`sunerf_hip.grid_field.longitude_mode`).  ``trainable=False`` freezes ``values``.

    A model of a rendering: ``EmissionRadiativeTransfer(model=GridField, model_config={'grid': grid, ...})``; the rendering's
    ``Rs_per_ds`` goes into ``model_config`` too."""

    def __init__(self, grid, d_output=2, d_input=4, Rs_per_ds=1.0, init=None, fill=None, periodic_lon=None, trainable=True):
        super().__init__()
        _gf.check_grid(grid)
        if int(d_output) != d_output or not 1 <= d_output <= _gf.MAX_CHANNELS:
            raise ValueError(f'a grid field holds 1 to {_gf.MAX_CHANNELS} channels per node, got d_output={d_output!r}')
        if d_input not in (3, 4):
            raise ValueError(f'a grid field takes points (x, y, z[, t]): d_input must be 3 or 4, got {d_input!r}')
        Rs_per_ds = float(Rs_per_ds)
        if not (math.isfinite(Rs_per_ds) and Rs_per_ds > 0):
            raise ValueError(f'Rs_per_ds must be finite and > 0, got {Rs_per_ds}')
        self.grid, self.d_output, self.d_input, self.Rs_per_ds = grid, int(d_output), int(d_input), Rs_per_ds
        self.lon_mode = _gf.longitude_mode(grid, periodic_lon)
        values = _initial_values(init, (*grid._shape3, self.d_output), self.d_output)
        self.values = nn.Parameter(values.contiguous(), requires_grad=bool(trainable))
        fill = self._default_fill() if fill is None else fill
        fill = torch.as_tensor(np.asarray(fill, dtype=np.float32)).reshape(-1)
        if fill.shape[0] != self.d_output:
            raise ValueError(f'fill has {fill.shape[0]} values for {self.d_output} channels')
        self.register_buffer('fill', fill)
        self._descs = {}

    def _default_fill(self):
        return default_fill(self.d_output)

    # ---- construction from a volume -----------------------------------------------------------------------------------------
    @classmethod
    def from_volume(cls, volume, trainable=False, **kwargs):
        """The field whose values are ``volume['inferences']``, bit for bit, on ``volume['grid']`` with ``volume['Rs_per_ds']``:
        the dict ``sample_volume`` / ``load_volume`` return (tensors or numpy arrays; one time)."""
        grid, inf = volume['grid'], volume['inferences']
        _gf.check_grid(grid)
        device = inf.device if isinstance(inf, torch.Tensor) else torch.device('cpu')
        inf = torch.as_tensor(np.asarray(inf.detach().cpu() if isinstance(inf, torch.Tensor) else inf))
        if inf.dim() != 4 or tuple(inf.shape[:3]) != tuple(grid._shape3):
            raise ValueError(f'from_volume: inferences of shape {tuple(inf.shape)} do not fit the grid {tuple(grid._shape3)} '
                             '(one time, channels last)')
        if inf.dtype != torch.float32:
            raise ValueError(f'from_volume: inferences must be float32, got {inf.dtype}')
        kwargs.setdefault('Rs_per_ds', volume.get('Rs_per_ds', 1.0))
        field = cls(grid, d_output=inf.shape[-1], init=inf, trainable=trainable, **kwargs)
        return field.to(device)

    @classmethod
    def bake(cls, field_or_rendering, grid, time, trainable=False, fill=None, periodic_lon=None, **sample_volume_kwargs):
        """``sample_volume(field_or_rendering, grid, time, ...)`` turned into a field: a trained model's answer on ``grid`` at
        the normalised ``time``, from which frames render without the network."""
        from sunerf_hip.volume import sample_volume
        if isinstance(time, (list, tuple, np.ndarray)) or (isinstance(time, torch.Tensor) and time.dim() > 0):
            raise ValueError('bake: one time per field (the grid has no time axis)')
        volume = sample_volume(field_or_rendering, grid, time, **sample_volume_kwargs)
        return cls.from_volume(volume, trainable=trainable, fill=fill, periodic_lon=periodic_lon)

    # ---- evaluation ---------------------------------------------------------------------------------------------------------
    def descriptor(self, device=None) -> '_gf.GridDescriptor':
        """The kernels' descriptor of this field on ``device`` (default: where ``values`` are), rebuilt when ``fill`` changed."""
        device = self.values.device if device is None else torch.device(device)
        key = (self.fill.data_ptr(), self.fill._version)
        cached = self._descs.get(str(device))
        if cached is None or cached[0] != key:
            desc = _gf.GridDescriptor(self.grid, self.d_output, self.Rs_per_ds, self.fill.detach().cpu().tolist(), self.lon_mode,
                                      device)
            cached = self._descs[str(device)] = (key, desc)
        return cached[1]

    def field_parameters(self):
        """The parameters :meth:`field_on_rays` carries gradients for."""
        return [self.values]

    def field_on_rays(self, rays_o, rays_d, z_vals):
        """``raw (N, S, C)`` at the samples ``o + d z`` (``sunerf_grid_field_fwd``); differentiable w.r.t. ``values``."""
        return _gf.field_on_rays(self.descriptor(), self.values, rays_o, rays_d, z_vals)

    def inferences(self, query_points):
        points = query_points.reshape(-1, query_points.shape[-1])
        return _gf.field_on_points(self.descriptor(), self.values, points)

    def forward(self, query_points):
        """``(M, 3 | 4)`` query points -> ``{'inferences': (M, C)}``; a time column is ignored."""
        return {'inferences': self.inferences(query_points)}

    # ---- prior --------------------------------------------------------------------------------------------------------------
    def smoothness(self):
        """A discrete ``|grad v|^2``: per axis the mean over nodes and channels of ``((v[i + 1] - v[i]) / (a[i + 1] - a[i]))^2``
        in the axis' own coordinate (solar radii, radians), then the mean over the three axes.  On a periodic longitude the
        differences across the seam count too: last node -> first node + 2 pi on an open axis; on a closed axis the two seam
        nodes are one place, and their difference is taken at the axis' mean step.  Plain torch ops, differentiable."""
        return self._spatial_smoothness(self.values)

    def _spatial_smoothness(self, v):
        """:meth:`smoothness` of ``v (..., n0, n1, n2, C)``; leading axes (frames) are averaged over."""
        total = 0.0
        lead = v.dim() - 4
        for k, axis in enumerate(self.grid.axes):
            dim = lead + k
            step = (axis[1:] - axis[:-1]).to(device=v.device, dtype=v.dtype)
            shape = [1] * v.dim()
            shape[dim] = -1
            d = (v.narrow(dim, 1, v.shape[dim] - 1) - v.narrow(dim, 0, v.shape[dim] - 1)) / step.view(shape)
            if k == 1 and self.lon_mode != _gf.LON_PATCH:
                if self.lon_mode == _gf.LON_OPEN:
                    seam = (axis[0] + _gf.TWO_PI - axis[-1]).item()
                else:
                    seam = ((axis[-1] - axis[0]) / (axis.shape[0] - 1)).item()
                d = torch.cat([d, (v.narrow(dim, 0, 1) - v.narrow(dim, v.shape[dim] - 1, 1)) / seam], dim)
            total = total + d.pow(2).mean()
        return total / 3.0

    def __getstate__(self):
        state = self.__dict__.copy()
        state['_descs'] = {}
        return state


class _DTHead:
    """The density-temperature head of ``MHDModel`` (mhd_model.py:11-24) in front of a grid field of ``(ln rho, log10 T)``:
    the ``log_absortpion`` scalars (``channels``: see ``sunerf.model.model.absorption_scalars``), ``volumetric_constant`` and
    zero base offsets.  Default ``fill``: ``(ln 1e-10, log10 1e-10)``, ``MHDModel``'s ``FILL_VALUE`` outside its cube."""

    def __init__(self, grid, d_output=2, channels=None, **kwargs):
        if d_output != 2:
            raise ValueError(f'a density-temperature grid holds (ln rho, log10 T): d_output must be 2, got {d_output!r}')
        super().__init__(grid, d_output=2, **kwargs)
        self.log_absortpion = absorption_scalars(channels)
        self.volumetric_constant = nn.Parameter(torch.tensor(1.0, dtype=torch.float32, requires_grad=True))
        self.base_log_density = 0.0
        self.base_log_temperature = 0.0

    def _default_fill(self):
        return (math.log(1e-10), -10.0)

    def forward(self, query_points):
        """``{'inferences': (M, 2), 'log_abs', 'vol_c'}``, as ``NeRF_DT`` / ``MHDModel`` answer."""
        return {'inferences': self.inferences(query_points), 'log_abs': self.log_absortpion, 'vol_c': self.volumetric_constant}


class GridFieldDT(_DTHead, GridField):
    """A grid of ``(ln rho, log10 T)`` with the density-temperature head exactly as ``MHDModel`` carries it (mhd_model.py:11-24):
    the ``log_absortpion`` scalars over the AIA channels, ``volumetric_constant`` and zero base offsets, so that
    ``DensityTemperatureRadiativeTransfer(model=GridFieldDT)`` renders and fits it.  Default ``fill``: ``(ln 1e-10, log10
    1e-10)``, ``MHDModel``'s ``FILL_VALUE`` outside its cube."""


class DynamicGridField(GridField):
    """``values (T, n0, n1, n2, C)`` on ``frame_times (T,)``: :class:`GridField` with a time axis.  All
    frames share ``grid``; a sample at the point ``p`` and the normalised time ``t`` of its ray is the trilinear value of the
    two neighbouring frames blended linearly in time.

    ``frame_times``: at least two finite, strictly increasing normalised times (kept as an fp64 buffer, so they travel in
    ``state_dict`` and ``.snf``).  ``time_mode='clamp'``: before the first frame the first, after the last the last;
    ``'fill'``: outside the frames the ``fill``.  A NaN time answers the fill.  ``init``: as :class:`GridField`, or one frame
    ``(n0, n1, n2, C)`` repeated over time, or the full array.  ``d_input`` must be 4: a point is ``(x, y, z, t)``.

    A model of a rendering: ``EmissionRadiativeTransfer(model=DynamicGridField, model_config={'grid': grid, 'frame_times':
    times})``; ``time_dependent`` makes the renderings hand it the rays' times."""

    time_dependent = True       # functional._field_raw hands the rays' times to field_on_rays

    def __init__(self, grid, d_output=2, d_input=4, Rs_per_ds=1.0, init=None, fill=None, periodic_lon=None, trainable=True,
                 frame_times=None, time_mode='clamp'):
        if d_input != 4:
            raise ValueError(f'a grid with a time axis takes points (x, y, z, t): d_input must be 4, got {d_input!r}')
        tau = _dg.check_frame_times(frame_times)
        _dg.time_mode(time_mode)
        super().__init__(grid, d_output=d_output, d_input=4, Rs_per_ds=Rs_per_ds, init=None, fill=fill,
                         periodic_lon=periodic_lon, trainable=trainable)
        values = _initial_values(init, (tau.shape[0], *grid._shape3, self.d_output), self.d_output)
        self.values = nn.Parameter(values.contiguous(), requires_grad=bool(trainable))
        self.time_mode = time_mode
        self.register_buffer('frame_times', tau)

    @property
    def n_frames(self):
        return self.values.shape[0]

    # ---- construction from a volume -----------------------------------------------------------------------------------------
    @classmethod
    def from_volume(cls, volume, trainable=False, **kwargs):
        """The field whose values are ``volume['inferences'] (T, n0, n1, n2, C)``, bit for bit, on ``volume['grid']`` at
        ``volume['times']`` (a list): what ``sample_volume`` returns for a sequence of times."""
        grid, inf, times = volume['grid'], volume['inferences'], volume['times']
        _gf.check_grid(grid)
        if not isinstance(times, (list, tuple, np.ndarray)) or np.ndim(times) != 1:
            raise ValueError('DynamicGridField.from_volume: the volume holds one time; use GridField.from_volume')
        device = inf.device if isinstance(inf, torch.Tensor) else torch.device('cpu')
        inf = torch.as_tensor(np.asarray(inf.detach().cpu() if isinstance(inf, torch.Tensor) else inf))
        if len(times) < 2:
            raise ValueError(f'DynamicGridField.from_volume: the volume holds {len(times)} time; use GridField.from_volume')
        if inf.dim() != 5 or tuple(inf.shape[:4]) != (len(times), *grid._shape3):
            raise ValueError(f'from_volume: inferences of shape {tuple(inf.shape)} do not fit {len(times)} times on the grid '
                             f'{tuple(grid._shape3)} (times first, channels last)')
        if inf.dtype != torch.float32:
            raise ValueError(f'from_volume: inferences must be float32, got {inf.dtype}')
        kwargs.setdefault('Rs_per_ds', volume.get('Rs_per_ds', 1.0))
        field = cls(grid, d_output=inf.shape[-1], init=inf, trainable=trainable, frame_times=list(times), **kwargs)
        return field.to(device)

    @classmethod
    def bake(cls, field_or_rendering, grid, times, trainable=False, fill=None, periodic_lon=None, time_mode='clamp',
             **sample_volume_kwargs):
        """``sample_volume(field_or_rendering, grid, times, ...)`` for the sequence ``times`` turned into a field: a trained
        model's answer on ``grid`` at those frames, from which a film renders without the network."""
        from sunerf_hip.volume import sample_volume
        times = [float(t) for t in _dg.check_frame_times(times)]
        volume = sample_volume(field_or_rendering, grid, times, **sample_volume_kwargs)
        return cls.from_volume(volume, trainable=trainable, fill=fill, periodic_lon=periodic_lon, time_mode=time_mode)

    # ---- evaluation ---------------------------------------------------------------------------------------------------------
    def descriptor(self, device=None) -> '_dg.DynamicGridDescriptor':
        """The kernels' descriptor of this field on ``device`` (default: where ``values`` are), rebuilt when ``fill`` or
        ``frame_times`` changed."""
        device = self.values.device if device is None else torch.device(device)
        key = (self.fill.data_ptr(), self.fill._version, self.frame_times.data_ptr(), self.frame_times._version, self.time_mode)
        cached = self._descs.get(str(device))
        if cached is None or cached[0] != key:
            desc = _dg.DynamicGridDescriptor(self.grid, self.d_output, self.Rs_per_ds, self.fill.detach().cpu().tolist(),
                                             self.lon_mode, self.frame_times.detach().double(), self.time_mode, device)
            cached = self._descs[str(device)] = (key, desc)
        return cached[1]

    def field_on_rays(self, rays_o, rays_d, z_vals, times):
        """``raw (N, S, C)`` at the samples ``o + d z`` at the rays' ``times (N, 1) | (N,)`` (``sunerf_dynamic_grid_fwd``);
        differentiable w.r.t. ``values``."""
        return _dg.field_on_rays(self.descriptor(), self.values, rays_o, rays_d, z_vals, times)

    def inferences(self, query_points):
        points = query_points.reshape(-1, query_points.shape[-1])
        return _dg.field_on_points(self.descriptor(), self.values, points)

    def forward(self, query_points):
        """``(M, 4)`` query points ``(x, y, z, t)`` -> ``{'inferences': (M, C)}``."""
        return {'inferences': self.inferences(query_points)}

    # ---- priors -------------------------------------------------------------------------------------------------------------
    def temporal_smoothness(self):
        """A discrete ``|dv / dt|^2``: the mean over intervals, nodes and channels of ``((v[j + 1] - v[j]) / (tau[j + 1] -
        tau[j]))^2`` in normalised time.  Plain torch ops, differentiable.  (:meth:`smoothness` is the spatial prior, its mean
        over the frames.)"""
        v = self.values
        step = (self.frame_times[1:] - self.frame_times[:-1]).to(device=v.device, dtype=v.dtype)
        return ((v[1:] - v[:-1]) / step.view(-1, 1, 1, 1, 1)).pow(2).mean()


class DynamicGridFieldDT(_DTHead, DynamicGridField):
    """:class:`DynamicGridField` of ``(ln rho, log10 T)`` with the density-temperature head exactly as :class:`GridFieldDT`
    carries it, so that ``DensityTemperatureRadiativeTransfer(model=DynamicGridFieldDT)`` renders and fits it."""
