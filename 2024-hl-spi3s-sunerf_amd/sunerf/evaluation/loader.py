"""Mirror of the reference's ``sunerf/evaluation/loader.py``: the inference-side caller of the render path
 on the device-side frame driver ``sunerf_hip.rays.render_frame``.

Kept: class names, constructor and method signatures, the dict-of-numpy-images result (``(H, W, ...)`` per output key).
Changed: no ``nn.DataParallel`` and no ``ThreadPoolExecutor`` (loader.py:37-39, :226-229) -- one process drives one GPU,
rays are generated on the device, tiles are rendered back to back on the current stream and assembled there;
``batch_size`` is the tile size in rays and defaults to what keeps the kernels busy instead of 128 / 4096.

``astropy`` / ``sunpy`` are optional.  With them, angles may be ``astropy`` quantities and the pixel grid comes from
the reference map's WCS exactly as in the reference (``all_coordinates_from_map``).  Without them, angles are plain
radians, distances plain solar radii, and the pixel grid is a linear plate scale described by a dict
``{'shape': (H, W), 'cdelt': (arcsec/pixel x, y), 'crpix': (x, y) 1-based, 'crval': (arcsec x, y)}``.
"""
from datetime import datetime, timedelta
from typing import Optional, Tuple

import numpy as np
import torch

from sunerf_hip.dem import _dt_rendering, render_dem_columns, render_dem_frame
from sunerf_hip.maps import render_columns
from sunerf_hip.rays import pose_spherical, render_frame
from sunerf_hip.volume import QUANTITIES, CartesianGrid, Plane, sample_volume

AU_IN_SOLAR_RADII = 215.03215567054764      # (1 * u.AU).to(u.solRad), IAU 2012 / 2015 nominal values
ARCSEC = np.pi / 180. / 3600.


def _radians(x) -> float:
    if hasattr(x, 'to_value'):
        from astropy import units as u
        return float(x.to_value(u.rad))
    return float(x)


def _radians_array(x) -> np.ndarray:
    """:func:`_radians` of an array of angles (plain numbers: radians) -> float64 array."""
    if hasattr(x, 'to_value'):
        from astropy import units as u
        return np.asarray(x.to_value(u.rad), dtype=np.float64)
    return np.asarray(x, dtype=np.float64)


def _solar_radii(x) -> float:
    if hasattr(x, 'to_value'):
        from astropy import units as u
        return float(x.to_value(u.solRad))
    return float(x)


def normalize_datetime(date, seconds_per_dt, ref_time):
    """sunerf/data/date_util.py:4-17."""
    return (date - ref_time).total_seconds() / seconds_per_dt


def unnormalize_datetime(norm_date: float, seconds_per_dt, ref_time) -> datetime:
    """sunerf/data/date_util.py:20-31."""
    return ref_time + timedelta(seconds=norm_date * seconds_per_dt)


def linear_plate_scale_axes(grid: dict, resolution=None, device='cuda') -> Tuple[torch.Tensor, torch.Tensor]:
    """Column (Tx) and row (Ty) angles [rad, fp64] of a frame described by a linear plate scale; ``resolution`` (H, W)
    resamples it over the same field of view like ``Map.resample`` (loader.py:73-75)."""
    h, w = grid['shape']
    cdx, cdy = grid['cdelt']
    cpx, cpy = grid.get('crpix', ((w + 1) / 2., (h + 1) / 2.))
    cvx, cvy = grid.get('crval', (0., 0.))
    if resolution is not None:
        nh, nw = (resolution, resolution) if np.isscalar(resolution) else resolution
        sx, sy = w / nw, h / nh                      # pixel-size ratio; pixel centres move with the field of view
        cdx, cdy = cdx * sx, cdy * sy
        cpx, cpy = (cpx - 0.5) / sx + 0.5, (cpy - 0.5) / sy + 0.5
        h, w = nh, nw
    col = torch.arange(1, w + 1, dtype=torch.float64, device=device)
    row = torch.arange(1, h + 1, dtype=torch.float64, device=device)
    return ((col - cpx) * cdx + cvx) * ARCSEC, ((row - cpy) * cdy + cvy) * ARCSEC


def load_state_file(state_path):
    """``torch.load`` of a ``.snf`` state (sunerf.py:62-74).  A density-temperature state written by the reference holds
    ``xitorch.interpolate.Interp1D`` objects (density_temperature.py:143-146); where xitorch is not installed a state-only
    stand-in of that name is registered for the load, and ``DensityTemperatureRadiativeTransfer.__setstate__`` takes the
    response table out of whatever the objects carry."""
    try:
        return torch.load(state_path, map_location='cpu', weights_only=False)
    except ModuleNotFoundError as err:
        if not (err.name or '').split('.')[0] == 'xitorch':
            raise
    import importlib.abc
    import importlib.machinery
    import sys
    import types

    class _Anything:                      # every class the pickle names under xitorch.* becomes a plain state holder
        def __init__(self, *a, **k):
            pass

    class _StandIn(types.ModuleType):
        __path__ = []                     # a package: sub-modules of any depth resolve through the finder below

        def __getattr__(self, name):
            if name.startswith('__'):
                raise AttributeError(name)
            cls = type(name, (_Anything,), {'__module__': self.__name__})
            setattr(self, name, cls)
            return cls

    class _Finder(importlib.abc.MetaPathFinder, importlib.abc.Loader):
        def find_spec(self, fullname, path=None, target=None):
            if fullname == 'xitorch' or fullname.startswith('xitorch.'):
                return importlib.machinery.ModuleSpec(fullname, self, is_package=True)
            return None

        def create_module(self, spec):
            return _StandIn(spec.name)

        def exec_module(self, module):
            pass
    finder = _Finder()
    sys.meta_path.insert(0, finder)
    try:
        return torch.load(state_path, map_location='cpu', weights_only=False)
    finally:
        sys.meta_path.remove(finder)
        for name in [m for m in sys.modules if m == 'xitorch' or m.startswith('xitorch.')]:
            del sys.modules[name]


class SuNeRFLoader:
    """loader.py:16-134."""

    def __init__(self, state_path, device=None):
        device = torch.device('cuda') if device is None else torch.device(device)
        self.device = device
        state = load_state_file(state_path)
        data_config = state['data_config']
        self.config = data_config
        self.wavelength = data_config.get('wavelength')
        self.times = data_config.get('times')
        self.wcs = data_config.get('wcs')
        self.resolution = data_config.get('resolution')
        self.rendering = state['rendering'].to(device)
        self.model = self.rendering.fine_model
        self.seconds_per_dt = state['seconds_per_dt']
        self.Rs_per_ds = state['Rs_per_ds']
        self.Mm_per_ds = self.Rs_per_ds * 695.7            # (1 * u.R_sun).to_value(u.Mm)
        self.ref_time = state['ref_time']
        self.ref_map = self._reference_map()

    def _reference_map(self):
        if isinstance(self.wcs, dict):                      # linear plate scale (no sunpy needed)
            return self.wcs
        from sunpy.map import Map                           # raises if sunpy is missing: a real WCS needs it
        return Map(np.zeros(self.resolution), self.wcs)

    @property
    def start_time(self):
        return np.min(self.times)

    @property
    def end_time(self):
        return np.max(self.times)

    def _pixel_angles(self, resolution):
        """Helioprojective angles of every pixel: two axes for a plate-scale dict, per-pixel arrays for a sunpy map."""
        if isinstance(self.ref_map, dict):
            return linear_plate_scale_axes(self.ref_map, resolution, self.device)
        from astropy import units as u
        from sunpy.coordinates import frames
        from sunpy.map import all_coordinates_from_map
        ref_map = self.ref_map.resample(resolution) if resolution is not None else self.ref_map
        coords = all_coordinates_from_map(ref_map).transform_to(frames.Helioprojective)
        tx = torch.from_numpy(np.ascontiguousarray(coords.Tx.to_value(u.rad), dtype=np.float64)).to(self.device)
        ty = torch.from_numpy(np.ascontiguousarray(coords.Ty.to_value(u.rad), dtype=np.float64)).to(self.device)
        return tx, ty

    def _frame_grid(self, lat, lon, distance, center, resolution, strides):
        """Pixel angles (``tx``, ``ty``) and camera pose of the observer's frame, every ``strides``-th pixel of it."""
        target_pose = pose_spherical(-_radians(lon), _radians(lat), _solar_radii(distance), center)
        tx, ty = self._pixel_angles(resolution)
        strides = int(strides)
        if strides < 1:
            raise ValueError(f'strides must be >= 1, got {strides}')
        if strides > 1:         # pixels [::strides, ::strides] of the full frame (the reference scripts' gt[::s, ::s])
            if tx.dim() == 2:
                tx, ty = tx[::strides, ::strides].contiguous(), ty[::strides, ::strides].contiguous()
            else:
                tx, ty = tx[::strides].contiguous(), ty[::strides].contiguous()
        return tx, ty, target_pose

    def _render(self, lat, lon, time: float, distance, center, resolution, batch_size, wl=None, as_numpy=True, strides=1):
        tx, ty, target_pose = self._frame_grid(lat, lon, distance, center, resolution, strides)
        wavelengths = None if wl is None else torch.as_tensor(np.asarray(wl), dtype=torch.float32, device=self.device)
        frame = render_frame(self.rendering, tx, ty, target_pose, float(time), wavelengths, tile_rays=int(batch_size))
        if not as_numpy:
            return frame
        return {k: v.cpu().numpy() for k, v in frame.items()}

    @torch.no_grad()
    def render_observer_image(self, lat, lon, time: datetime, distance=AU_IN_SOLAR_RADII,
                              center: Tuple[float, float, float] = None, resolution=None, batch_size: int = 1 << 18,
                              as_numpy: bool = True, strides: int = 1):
        """loader.py:63-108: image of the observer at (lat, lon, distance) at ``time`` (a datetime).  ``strides`` renders the
        pixels ``[::strides, ::strides]`` of that frame only (the evaluation scripts compare with ``gt[::strides, ::strides]``)."""
        time = normalize_datetime(time, self.seconds_per_dt, self.ref_time)
        return self._render(lat, lon, time, distance, center, resolution, batch_size, None, as_numpy, strides)

    def _observe(self, lat, lon, time: float, instrument, seed, distance, center, resolution, batch_size, wl, as_numpy, poisson,
                 read):
        """The frame rendered at ``instrument.bin`` times the detector resolution over the same field of view -- the bin x bin
        sub-pixels tile each detector pixel -- moved to planes and seen through ``instrument``; back in (H, W[, C]) layout."""
        from sunerf_hip.observations import resampled_grid
        if not isinstance(self.ref_map, dict) or 'shape' not in self.ref_map:
            raise TypeError('observe_image needs a plate-scale dict with a shape as the reference map')
        if resolution is None:
            resolution = self.ref_map['shape']
        nh, nw = (resolution, resolution) if np.isscalar(resolution) else resolution
        b = instrument.bin
        fine = (int(nh) * b, int(nw) * b)
        frame = self._render(lat, lon, time, distance, center, fine, batch_size, wl, as_numpy=False)['image']
        planes = (frame[None] if frame.dim() == 2 else frame.permute(2, 0, 1)).contiguous()
        out = instrument.observe(planes, seed, poisson=poisson, read=read)
        out = {k: (v[0] if frame.dim() == 2 else v.permute(1, 2, 0).contiguous()) for k, v in out.items()}
        if as_numpy:
            out = {k: v.cpu().numpy() for k, v in out.items()}
        out['grid'] = instrument.detector_grid(resampled_grid(self.ref_map, fine))
        return out

    @torch.no_grad()
    def observe_image(self, lat, lon, time: datetime, instrument, seed: int = 0, resolution=None,
                      distance=AU_IN_SOLAR_RADII, center: Tuple[float, float, float] = None, batch_size: int = 1 << 18,
                      as_numpy: bool = True, poisson: bool = True, read: bool = True):
        """What ``instrument`` (``sunerf_hip.instrument.Instrument``) records of the observer's view at ``time``: ``image`` (one
        noisy realisation), ``expected`` (blurred and binned, noise-free), ``sigma``, ``saturated`` at the detector's
        ``resolution`` (default: the reference map's) and ``grid``, the plate-scale dict of that frame.  ``seed`` fixes the noise."""
        time = normalize_datetime(time, self.seconds_per_dt, self.ref_time)
        return self._observe(lat, lon, time, instrument, seed, distance, center, resolution, batch_size, None, as_numpy, poisson, read)

    def _columns(self, lat, lon, time: float, grid, r_range, n_samples, batch_size, profiles, wl, as_numpy):
        wavelengths = None if wl is None else torch.as_tensor(np.asarray(wl), dtype=torch.float32, device=self.device)
        lat = torch.from_numpy(_radians_array(lat).reshape(-1)).to(self.device)
        lon = torch.from_numpy(_radians_array(lon).reshape(-1)).to(self.device)
        r_range = (_solar_radii(r_range[0]), _solar_radii(r_range[1]))
        out = render_columns(self.rendering, lat, lon, float(time), r_range, n_samples, wavelengths,
                             None if batch_size is None else int(batch_size), profiles=profiles, grid=grid)
        if not as_numpy:
            return out
        return {k: v.cpu().numpy() for k, v in out.items()}

    def _map(self, time: float, lat_range, lon_range, shape, r_range, n_samples, batch_size, profiles, wl, as_numpy):
        n_lat, n_lon = (int(shape), int(shape)) if np.isscalar(shape) else (int(shape[0]), int(shape[1]))
        lat = np.linspace(_radians(lat_range[0]), _radians(lat_range[1]), n_lat)      # pixel centres include both ends
        lon = np.linspace(_radians(lon_range[0]), _radians(lon_range[1]), n_lon)
        return self._columns(lat, lon, time, True, r_range, n_samples, batch_size, profiles, wl, as_numpy)

    @torch.no_grad()
    def render_heliographic_map(self, time: datetime, lat_range=(-np.pi / 2, np.pi / 2), lon_range=(-np.pi, np.pi),
                                shape=(721, 1441), r_range=(1.0, 1.3), n_samples: int = 512, batch_size: Optional[int] = None,
                                profiles: bool = False, as_numpy: bool = True):
        """Heliographic map of the corona at ``time`` (a datetime): one radial column per (latitude, longitude) pixel through
        the fine model, ``n_samples`` radii ``linspace(*r_range)`` [solar radii] per column (sunerf/evaluation/stash/
        topographical_map.py:36-66, topographical_profile.py:33-58).  Angles as in :meth:`render_observer_image` (plain
        numbers: radians); pixel centres ``linspace(*lat_range, shape[0])`` x ``linspace(*lon_range, shape[1])``, row 0 the
        southernmost latitude, column 0 the smallest longitude.  Returns the outputs of ``sunerf_hip.maps.render_columns``,
        each ``(n_lat, n_lon, ...)``; heights in solar radii.  ``batch_size``: columns per tile (default: about 1 GiB of
        scratch per tile)."""
        time = normalize_datetime(time, self.seconds_per_dt, self.ref_time)
        return self._map(time, lat_range, lon_range, shape, r_range, n_samples, batch_size, profiles, None, as_numpy)

    @torch.no_grad()
    def render_radial_profile(self, lats, lons, time: datetime, r_range=(1.0, 1.3), n_samples: int = 512,
                              batch_size: Optional[int] = None, profiles: bool = True, as_numpy: bool = True):
        """Radial columns along an arc or at arbitrary points: per-column ``lats`` / ``lons`` of equal length (radians or
        astropy quantities) at ``time`` (a datetime) (topographical_profile.py:33-58, topographical_slice.py:119-140,
        eruption_profile.py:76-101).  Returns the outputs of ``sunerf_hip.maps.render_columns``, each ``(n, ...)``, with the
        per-sample profiles ``(n, n_samples)`` by default."""
        time = normalize_datetime(time, self.seconds_per_dt, self.ref_time)
        return self._columns(lats, lons, time, False, r_range, n_samples, batch_size, profiles, None, as_numpy)

    def _dem_image(self, lat, lon, time: float, distance, center, resolution, batch_size, as_numpy, strides, logt_nodes,
                   attenuation_wavelength, r_range, length_scale):
        rendering = _dt_rendering(self.rendering, 'render_dem_image')           # before any device work
        tx, ty, target_pose = self._frame_grid(lat, lon, distance, center, resolution, strides)
        r_in = _solar_radii(r_range[0]) / rendering.Rs_per_ds
        r_out = np.inf if r_range[1] is None else _solar_radii(r_range[1]) / rendering.Rs_per_ds
        out = render_dem_frame(rendering, tx, ty, target_pose, float(time), logt_nodes, attenuation_wavelength, (r_in, r_out),
                               tile_rays=int(batch_size), length_scale=length_scale)
        if not as_numpy:
            return out
        return {k: v.cpu().numpy() for k, v in out.items()}

    def _dem_map(self, time: float, lat_range, lon_range, shape, r_range, n_samples, batch_size, as_numpy, logt_nodes,
                 attenuation_wavelength, length_scale):
        rendering = _dt_rendering(self.rendering, 'render_dem_map')
        n_lat, n_lon = (int(shape), int(shape)) if np.isscalar(shape) else (int(shape[0]), int(shape[1]))
        lat = torch.from_numpy(np.linspace(_radians(lat_range[0]), _radians(lat_range[1]), n_lat)).to(self.device)
        lon = torch.from_numpy(np.linspace(_radians(lon_range[0]), _radians(lon_range[1]), n_lon)).to(self.device)
        r_range = (_solar_radii(r_range[0]), _solar_radii(r_range[1]))
        out = render_dem_columns(rendering, lat, lon, float(time), r_range, n_samples, logt_nodes, attenuation_wavelength,
                                 None if batch_size is None else int(batch_size), length_scale=length_scale)
        if not as_numpy:
            return out
        return {k: v.cpu().numpy() for k, v in out.items()}

    @torch.no_grad()
    def render_dem_image(self, lat, lon, time: datetime, distance=AU_IN_SOLAR_RADII,
                         center: Tuple[float, float, float] = None, resolution=None, batch_size: int = 1 << 18,
                         as_numpy: bool = True, strides: int = 1, logt_nodes=None, attenuation_wavelength=None,
                         r_range=(0., None), length_scale: float = 1.0):
        """The line-of-sight DEM behind every pixel of :meth:`render_observer_image`'s frame (same observer arguments), for a
        density-temperature rendering: ``dem`` (H, W, K) on ``logt_nodes`` (default: the response table's log T grid), ``em``,
        ``logt_mean``, ``column`` (H, W) and ``logt_nodes`` (K,) (``sunerf_hip.dem``).  ``attenuation_wavelength``: attenuate
        with that channel's absorption; ``r_range`` [solar radii]: only samples at these radii count (default: all);
        ``length_scale`` multiplies ``dem``, ``em`` and ``column`` (default: the model's length unit, like the render).
        Raises ``TypeError`` for a rendering without a temperature."""
        _dt_rendering(self.rendering, 'render_dem_image')
        time = normalize_datetime(time, self.seconds_per_dt, self.ref_time)
        return self._dem_image(lat, lon, time, distance, center, resolution, batch_size, as_numpy, strides, logt_nodes,
                               attenuation_wavelength, r_range, length_scale)

    @torch.no_grad()
    def render_dem_map(self, time: datetime, lat_range=(-np.pi / 2, np.pi / 2), lon_range=(-np.pi, np.pi), shape=(721, 1441),
                       r_range=(1.0, 1.3), n_samples: int = 512, batch_size: Optional[int] = None, as_numpy: bool = True,
                       logt_nodes=None, attenuation_wavelength=None, length_scale: float = 1.0):
        """The DEM of the radial columns of :meth:`render_heliographic_map` (same grid arguments): ``dem`` (n_lat, n_lon, K),
        ``em``, ``logt_mean``, ``column`` (n_lat, n_lon) and ``logt_nodes`` (K,); the other arguments as
        :meth:`render_dem_image`."""
        _dt_rendering(self.rendering, 'render_dem_map')
        time = normalize_datetime(time, self.seconds_per_dt, self.ref_time)
        return self._dem_map(time, lat_range, lon_range, shape, r_range, n_samples, batch_size, as_numpy, logt_nodes,
                             attenuation_wavelength, length_scale)

    @torch.no_grad()
    def invert_dem_image(self, images, wl=None, logt_nodes=None, errors=None, as_numpy: bool = True, **solver):
        """The classical per-pixel DEM inversion (optically thin) of ``images`` (..., M) -- a frame of
        :meth:`render_observer_image` of a density-temperature rendering, or observations in its units -- for the channels ``wl``
        (default: all seven): ``DensityTemperatureRadiativeTransfer.invert_dem`` (``sunerf_hip.dem_inversion``), to set next to
        :meth:`render_dem_image`'s ``dem`` / ``em`` / ``logt_mean`` of the same frame.  ``errors``, ``lam``, ``prior``,
        ``chi2_target``, ... go through.  Raises ``TypeError`` for a rendering without a temperature."""
        rendering = _dt_rendering(self.rendering, 'invert_dem_image')           # before any device work
        if not isinstance(images, torch.Tensor):
            images = torch.as_tensor(np.asarray(images), dtype=torch.float32)
        if errors is not None and not isinstance(errors, torch.Tensor):
            errors = torch.as_tensor(np.asarray(errors), dtype=torch.float32)
        images = images.to(self.device)
        out = rendering.invert_dem(images, None if wl is None else np.asarray(wl).reshape(-1).tolist(), logt_nodes,
                                   None if errors is None else errors.to(self.device), **solver)
        if not as_numpy:
            return out
        return {k: v.cpu().numpy() for k, v in out.items()}

    def _volume(self, time: float, grid, wl, quantities, r_range, fill, batch_size, as_numpy):
        out = sample_volume(self.rendering, grid, float(time), None if wl is None else np.asarray(wl, dtype=np.float32),
                            quantities, r_range, fill, tile_points=None if batch_size is None else int(batch_size))
        if not as_numpy:
            return out
        return {k: v.cpu().numpy() if isinstance(v, torch.Tensor) else v for k, v in out.items()}

    @staticmethod
    def _cube(half_width, shape, grid):
        if grid is not None:
            return grid
        n = (int(shape),) * 3 if np.isscalar(shape) else tuple(int(s) for s in shape)
        hw = (_solar_radii(half_width),) * 3 if np.isscalar(half_width) or hasattr(half_width, 'to_value') else \
            tuple(_solar_radii(h) for h in half_width)
        if len(n) != 3 or len(hw) != 3:
            raise ValueError('a volume has three axes: shape and half_width are a number or three of them')
        return CartesianGrid(*(np.linspace(-h, h, k) for h, k in zip(hw, n)))

    @staticmethod
    def _slice(origin, e_u, e_v, half_width, shape):
        n = (int(shape),) * 2 if np.isscalar(shape) else tuple(int(s) for s in shape)
        hw = (_solar_radii(half_width),) * 2 if np.isscalar(half_width) or hasattr(half_width, 'to_value') else \
            tuple(_solar_radii(h) for h in half_width)
        if len(n) != 2 or len(hw) != 2:
            raise ValueError('a slice has two axes: shape and half_width are a number or two of them')
        return Plane(origin, e_u, e_v, np.linspace(-hw[0], hw[0], n[0]), np.linspace(-hw[1], hw[1], n[1]))

    @torch.no_grad()
    def render_volume(self, time: datetime, half_width=1.3, shape=256, grid=None, quantities=None, r_range=(1.0, None),
                      fill: float = float('nan'), batch_size: Optional[int] = None, as_numpy: bool = True):
        """3-D volume of the fine model at ``time`` (a datetime) (sunerf/evaluation/stash/voxel_volume.py:30-56): the cube
        ``linspace(-half_width, half_width, shape)`` per axis [solar radii], plain C order ``(x, y, z)`` (the reference's
        ``np.meshgrid`` default swaps x and y), or any ``grid`` of ``sunerf_hip.volume`` (``CartesianGrid``, ``Plane``,
        ``SphericalGrid``).  Returns the outputs of ``sunerf_hip.volume.sample_volume``: ``inferences (*grid.shape, 2)``,
        ``radius``, ``grid``, ``times`` and the physical quantities (``emission`` and ``absorption`` for an emission model),
        ``fill`` where the radius is outside ``r_range`` (default: inside the Sun).  ``batch_size``: voxels per tile."""
        time = normalize_datetime(time, self.seconds_per_dt, self.ref_time)
        return self._volume(time, self._cube(half_width, shape, grid), None, quantities, r_range, fill, batch_size, as_numpy)

    @torch.no_grad()
    def render_slice(self, time: datetime, origin=(0., 0., 0.), e_u=(1., 0., 0.), e_v=(0., 1., 0.), half_width=1.3, shape=512,
                     quantities=None, r_range=(1.0, None), fill: float = float('nan'), batch_size: Optional[int] = None,
                     as_numpy: bool = True):
        """A plane through the fine model at ``time`` (a datetime): points ``origin + u e_u + v e_v`` [solar radii] with
        ``u, v = linspace(-half_width, half_width, shape)``; outputs as :meth:`render_volume`, shaped ``(n_u, n_v, ...)``."""
        time = normalize_datetime(time, self.seconds_per_dt, self.ref_time)
        return self._volume(time, self._slice(origin, e_u, e_v, half_width, shape), None, quantities, r_range, fill, batch_size,
                            as_numpy)

    def normalize_datetime(self, time):
        return normalize_datetime(time, self.seconds_per_dt, self.ref_time)

    def unnormalize_datetime(self, time):
        return unnormalize_datetime(time, self.seconds_per_dt, self.ref_time)

    @torch.no_grad()
    def load_coords(self, query_points_npy, batch_size=1 << 20):
        """loader.py:119-134: model output (emission / absorption or density / temperature logits) at query points
        ``(..., 4)`` = (x, y, z, t)."""
        target_shape = query_points_npy.shape[:-1]
        flat = torch.from_numpy(np.ascontiguousarray(query_points_npy)).float().reshape(-1, 4)
        parts = []
        for b in range(0, flat.shape[0], batch_size):
            answer = self.model(flat[b:b + batch_size].to(self.device))      # any field model: NeRF (fused points mode), SimpleStar, ...
            parts.append((answer['inferences'] if isinstance(answer, dict) else answer).cpu())      # D3 resolved: the tensor
        return torch.cat(parts, 0).view(*target_shape, -1).numpy()


class ModelLoader(SuNeRFLoader):
    """loader.py:137-242: loader around an in-memory rendering module (density-temperature path: ``wl`` channels)."""

    def __init__(self, rendering, model, ref_map, device=None):
        device = torch.device('cuda') if device is None else torch.device(device)
        self.device = device
        self.ref_map = ref_map
        self.rendering = rendering.to(device)
        self.model = model.to(device)
        self.seconds_per_dt = 1
        meta = ref_map.get('meta', {}) if isinstance(ref_map, dict) else ref_map.meta
        stamp = meta['t_obs'] if 't_obs' in meta else meta.get('date-obs')
        self.ref_time = datetime.strptime(stamp, '%Y-%m-%dT%H:%M:%S.%f') if stamp is not None else None

    def process_batch(self, b_rays_o, b_rays_d, b_time, b_wl):
        return self.rendering(b_rays_o, b_rays_d, b_time, b_wl)

    def process_batch_with_index(self, index, b_rays_o, b_rays_d, b_time, b_wl):
        return index, self.process_batch(b_rays_o, b_rays_d, b_time, b_wl)

    @torch.no_grad()
    def render_observer_image(self, lat, lon, time: float, distance=AU_IN_SOLAR_RADII, wl: Optional[np.ndarray] = None,
                              center: Tuple[float, float, float] = None, resolution=None, batch_size: int = 1 << 17,
                              as_numpy: bool = True, strides: int = 1):
        """loader.py:159-242: ``time`` is already normalised here (a float); ``strides`` as in
        :meth:`SuNeRFLoader.render_observer_image`."""
        return self._render(lat, lon, time, distance, center, resolution, batch_size, wl, as_numpy, strides)

    @torch.no_grad()
    def observe_image(self, lat, lon, time: float, instrument, seed: int = 0, resolution=None, distance=AU_IN_SOLAR_RADII,
                      wl: Optional[np.ndarray] = None, center: Tuple[float, float, float] = None, batch_size: int = 1 << 17,
                      as_numpy: bool = True, poisson: bool = True, read: bool = True):
        """:meth:`SuNeRFLoader.observe_image` with ``time`` already normalised (a float) and the channels ``wl``."""
        return self._observe(lat, lon, time, instrument, seed, distance, center, resolution, batch_size, wl, as_numpy, poisson, read)

    @torch.no_grad()
    def render_heliographic_map(self, time: float, lat_range=(-np.pi / 2, np.pi / 2), lon_range=(-np.pi, np.pi),
                                shape=(721, 1441), r_range=(1.0, 1.3), n_samples: int = 512, wl: Optional[np.ndarray] = None,
                                batch_size: Optional[int] = None, profiles: bool = False, as_numpy: bool = True):
        """:meth:`SuNeRFLoader.render_heliographic_map` with ``time`` already normalised (a float) and the channels ``wl`` of a
        density-temperature rendering."""
        return self._map(time, lat_range, lon_range, shape, r_range, n_samples, batch_size, profiles, wl, as_numpy)

    @torch.no_grad()
    def render_radial_profile(self, lats, lons, time: float, r_range=(1.0, 1.3), n_samples: int = 512,
                              wl: Optional[np.ndarray] = None, batch_size: Optional[int] = None, profiles: bool = True,
                              as_numpy: bool = True):
        """:meth:`SuNeRFLoader.render_radial_profile` with ``time`` already normalised (a float) and the channels ``wl``."""
        return self._columns(lats, lons, time, False, r_range, n_samples, batch_size, profiles, wl, as_numpy)

    @torch.no_grad()
    def render_dem_image(self, lat, lon, time: float, distance=AU_IN_SOLAR_RADII, center: Tuple[float, float, float] = None,
                         resolution=None, batch_size: int = 1 << 17, as_numpy: bool = True, strides: int = 1, logt_nodes=None,
                         attenuation_wavelength=None, r_range=(0., None), length_scale: float = 1.0):
        """:meth:`SuNeRFLoader.render_dem_image` with ``time`` already normalised (a float)."""
        return self._dem_image(lat, lon, time, distance, center, resolution, batch_size, as_numpy, strides, logt_nodes,
                               attenuation_wavelength, r_range, length_scale)

    @torch.no_grad()
    def render_dem_map(self, time: float, lat_range=(-np.pi / 2, np.pi / 2), lon_range=(-np.pi, np.pi), shape=(721, 1441),
                       r_range=(1.0, 1.3), n_samples: int = 512, batch_size: Optional[int] = None, as_numpy: bool = True,
                       logt_nodes=None, attenuation_wavelength=None, length_scale: float = 1.0):
        """:meth:`SuNeRFLoader.render_dem_map` with ``time`` already normalised (a float)."""
        return self._dem_map(time, lat_range, lon_range, shape, r_range, n_samples, batch_size, as_numpy, logt_nodes,
                             attenuation_wavelength, length_scale)

    @torch.no_grad()
    def render_volume(self, time: float, half_width=1.3, shape=256, grid=None, wl: Optional[np.ndarray] = None, quantities=None,
                      r_range=(1.0, None), fill: float = float('nan'), batch_size: Optional[int] = None, as_numpy: bool = True):
        """:meth:`SuNeRFLoader.render_volume` with ``time`` already normalised (a float) and the channels ``wl`` of a
        density-temperature rendering (``density``, ``log_temperature``, ``emissivity (..., W)``)."""
        return self._volume(time, self._cube(half_width, shape, grid), wl, quantities, r_range, fill, batch_size, as_numpy)

    @torch.no_grad()
    def render_slice(self, time: float, origin=(0., 0., 0.), e_u=(1., 0., 0.), e_v=(0., 1., 0.), half_width=1.3, shape=512,
                     wl: Optional[np.ndarray] = None, quantities=None, r_range=(1.0, None), fill: float = float('nan'),
                     batch_size: Optional[int] = None, as_numpy: bool = True):
        """:meth:`SuNeRFLoader.render_slice` with ``time`` already normalised (a float) and the channels ``wl``."""
        return self._volume(time, self._slice(origin, e_u, e_v, half_width, shape), wl, quantities, r_range, fill, batch_size,
                            as_numpy)


class EnsembleLoader:
    """K trained members of one model (``.snf`` files) rendered from the same observer (uncertainty_correlation.py:56-77,
    overview_simulation.py:47-52): one :class:`SuNeRFLoader` per file, all on one device.  The members must share
    ``ref_time``, ``seconds_per_dt``, ``Rs_per_ds``, ``wcs`` and ``resolution``."""

    _SHARED = ('ref_time', 'seconds_per_dt', 'Rs_per_ds', 'wcs', 'resolution')

    def __init__(self, state_paths, device=None):
        state_paths = list(state_paths)
        if not state_paths:
            raise ValueError('EnsembleLoader needs at least one state file')
        self.loaders = [SuNeRFLoader(path, device=device) for path in state_paths]
        first = self.loaders[0]
        for path, member in zip(state_paths[1:], self.loaders[1:]):
            for field in self._SHARED:
                if not _same(getattr(member, field), getattr(first, field)):
                    raise ValueError(f'EnsembleLoader: {path} has a different {field} than {state_paths[0]}')
        self.device = first.device

    @torch.no_grad()
    def render_observer_image(self, lat, lon, time: datetime, distance=AU_IN_SOLAR_RADII,
                              center: Tuple[float, float, float] = None, resolution=None, batch_size: int = 1 << 18,
                              as_numpy: bool = True, strides: int = 1):
        """Member 0's :meth:`SuNeRFLoader.render_observer_image` outputs, plus ``ensemble_mean`` and ``ensemble_std`` (ddof 0,
        as ``np.std(predictions, 0)``) of ``image`` over the members: two passes in fp64, in member order, then fp32."""
        frames = [m.render_observer_image(lat, lon, time, distance, center, resolution, batch_size, False, strides)
                  for m in self.loaders]
        images = [f['image'].double() for f in frames]
        mean = images[0].clone()
        for img in images[1:]:
            mean += img
        mean /= len(images)
        var = torch.zeros_like(mean)
        for img in images:
            var += (img - mean) ** 2
        var /= len(images)
        out = dict(frames[0])
        out['ensemble_mean'] = mean.float()
        out['ensemble_std'] = torch.sqrt(var).float()
        if not as_numpy:
            return out
        return {k: v.cpu().numpy() for k, v in out.items()}

    @torch.no_grad()
    def render_volume(self, time: datetime, half_width=1.3, shape=256, grid=None, quantities=None, r_range=(1.0, None),
                      fill: float = float('nan'), batch_size: Optional[int] = None, as_numpy: bool = True):
        """Every member's :meth:`SuNeRFLoader.render_volume` on the same grid: ``radius``, ``grid`` and ``times`` of member 0
        and, for each quantity ``q``, ``q_mean`` and ``q_std`` (ddof 0) over the members: two passes in fp64, in member order,
        then fp32, like :meth:`render_observer_image`.  Masked voxels stay ``fill``-like (NaN) in both.  The members are
        ``.snf`` loaders, whose ``render_volume`` takes no channels: a density-temperature ensemble gives ``density`` and
        ``log_temperature`` only."""
        grid = SuNeRFLoader._cube(half_width, shape, grid)
        vols = [m.render_volume(time, grid=grid, quantities=quantities, r_range=r_range, fill=fill, batch_size=batch_size,
                                as_numpy=False) for m in self.loaders]
        first = vols[0]
        out = {k: first[k] for k in ('radius', 'grid', 'times', 'Rs_per_ds', 'kind') if k in first}
        for q in QUANTITIES[first['kind']]:
            if q not in first:
                continue
            fields = [vol[q].double() for vol in vols]
            mean = fields[0].clone()
            for f in fields[1:]:
                mean += f
            mean /= len(fields)
            var = torch.zeros_like(mean)
            for f in fields:
                var += (f - mean) ** 2
            var /= len(fields)
            out[q + '_mean'] = mean.float()
            out[q + '_std'] = torch.sqrt(var).float()
        if not as_numpy:
            return out
        return {k: v.cpu().numpy() if isinstance(v, torch.Tensor) else v for k, v in out.items()}


def _same(a, b) -> bool:
    if isinstance(a, dict) and isinstance(b, dict):
        return a.keys() == b.keys() and all(_same(a[k], b[k]) for k in a)
    if isinstance(a, (np.ndarray, list, tuple)) or isinstance(b, (np.ndarray, list, tuple)):
        try:
            return bool(np.array_equal(np.asarray(a), np.asarray(b)))
        except Exception:
            return False
    try:
        return bool(a == b)
    except Exception:       # objects without a usable equality (e.g. a WCS that refuses the comparison)
        return a is b
