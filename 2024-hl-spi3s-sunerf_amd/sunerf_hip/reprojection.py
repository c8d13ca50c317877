"""The reprojection baseline on the device: ``sunerf/baseline/reprojection.py`` of the reference.

All emission is taken to come from the solar surface ``r = 1 R_sun``: the observed views are projected onto that sphere and
averaged into a heliographic ("synchronic") map (``create_heliographic_map``, reprojection.py:52-95), and the map is looked at
from new observers (``transform`` :98-125, ``load_views`` :128-168).  ``evaluation/stash/baseline_simulation.py:27-44`` scores
that prediction against held-out images; it is what the scores of a trained model are read against.

:func:`synchronic_map` is one launch of ``sunerf_synchronic_map`` plus the two of ``sunerf_map_fill``;
:meth:`SynchronicMap.reproject_many` is one launch of ``sunerf_reproject_views`` for any number of observers
(``csrc/reprojection.hip``; conventions and formulas: ``include/sunerf_hip.h``).  The host code here is plumbing: there is no
CPU path.

Deviations from the reference: the geometry is this project's pinhole convention (``get_rays``), not a FITS WCS, so a map and
a ``render_heliographic_map`` of the same shape and ranges are comparable pixel for pixel and a reprojected view lies on the
pixels ``render_observer_image`` renders -- parity with ``reproject`` + sunpy is not pinned (neither is installed where this
runs), only the interpolation is (scipy's ``map_coordinates``).  Coverage ends at the outermost pixel centres.  The map is in
the frame of the rays; there is no differential rotation and no time handling.
"""
import warnings
from typing import Iterator, List, Optional, Sequence, Tuple

import numpy as np
import torch

from . import lib as _l
from ._ffi import _ptr, _stream
from .observations import AU_IN_SOLAR_RADII, VIEW_DESC, View, view_descriptors

# struct SunerfObserverDesc (include/sunerf_hip.h)
OBSERVER_DESC = np.dtype({'names': ['pix_offset', 'tx', 'ty', 'height', 'width', 'c2w'],
                          'formats': ['<i8', '<u8', '<u8', '<i4', '<i4', ('<f4', 12)],
                          'offsets': [0, 8, 16, 24, 28, 32], 'itemsize': 80})
MAX_SLAB_ROWS = 65535       # rows of one sunerf_synchronic_map launch


def map_axes(shape=(1024, 2048), lat_range=(-np.pi / 2, np.pi / 2), lon_range=(-np.pi, np.pi)) -> Tuple[np.ndarray, np.ndarray]:
    """The two fp64 axes of pixel centres as ``render_heliographic_map`` builds them: ``linspace`` including both ends, row 0
    southernmost."""
    from sunerf.evaluation.loader import _radians
    n_lat, n_lon = (int(shape), int(shape)) if np.isscalar(shape) else (int(shape[0]), int(shape[1]))
    if n_lat < 1 or n_lon < 1:
        raise ValueError(f'a map has at least 1 x 1 pixels, not {n_lat} x {n_lon}')
    lat0, lat1, lon0, lon1 = (_radians(v) for v in (*lat_range, *lon_range))
    if not (lat1 > lat0 and lon1 > lon0) or not all(np.isfinite(v) for v in (lat0, lat1, lon0, lon1)):
        raise ValueError(f'lat_range / lon_range must be ascending and finite, got {lat_range!r} / {lon_range!r}')
    return np.linspace(lat0, lat1, n_lat), np.linspace(lon0, lon1, n_lon)


def view_grid_coordinates(strides_deg=10) -> np.ndarray:
    """(n, 2) float32 (lat, lon) [deg] of ``load_views``' observers: ``mgrid[-90:91:s, 0:361:s]`` (reprojection.py:140-141)."""
    return np.stack(np.mgrid[-90:91:strides_deg, :361:strides_deg], -1).astype(np.float32).reshape((-1, 2))


def _monotone(axis: torch.Tensor) -> bool:
    if axis.numel() < 2:
        return True
    d = axis[1:] - axis[:-1]
    return bool(((d > 0).all() | (d < 0).all()).reshape(1)[0])


def check_views(views: Sequence[View]) -> int:
    """Host-side checks before anything touches the device; returns the channel count."""
    if not views:
        raise ValueError('no views to build a map from')
    for v in views:
        if v.per_pixel:
            raise ValueError(f'view {v.name!r} has per-pixel angles: a grid that is not two axes has no closed inverse '
                             'projection, so the reprojection baseline does not take it')
        if v.plane.size != views[0].plane.size:
            raise ValueError('all views of a map carry the same number of channels')
    for v in views:
        if getattr(v, '_axes_monotone', None) is None:
            v._axes_monotone = _monotone(v.tx) and _monotone(v.ty)
        if not v._axes_monotone:
            raise ValueError(f'view {v.name!r}: tx / ty must be strictly monotone axes')
    return int(views[0].plane.size)


def _device_of(views: Sequence[View]) -> torch.device:
    dev = views[0].image.device
    if dev.type != 'cuda' or any(v.image.device != dev or v.tx.device != dev for v in views):
        raise _l.SunerfHipError('the reprojection baseline runs on one ROCm device: views on the CPU have no path '
                                '(there is no CPU fallback)')
    return dev


def _radius(Rs_per_ds) -> float:
    Rs_per_ds = float(Rs_per_ds)
    if not (np.isfinite(Rs_per_ds) and Rs_per_ds > 0):
        raise ValueError(f'Rs_per_ds must be finite and > 0, got {Rs_per_ds}')
    return 1.0 / Rs_per_ds


def map_rows(views: Sequence[View], lat: torch.Tensor, lon: torch.Tensor, Rs_per_ds: float = 1.0, row_begin: int = 0,
             n_rows: Optional[int] = None, want_coords: bool = False):
    """Rows ``[row_begin, row_begin + n_rows)`` of the coadd, before the fill (``sunerf_synchronic_map``): ``image``
    (C, n_rows, n_lon) fp32 with NaN where no view covers, ``footprint`` int32 and, with ``want_coords`` (one view only),
    ``coords`` (3, n_rows, n_lon) fp64 = the view's pixel coordinates x, y and the visibility margin ``p . o - R^2``."""
    n_channels = check_views(views)
    radius = _radius(Rs_per_ds)
    if want_coords and len(views) != 1:
        raise ValueError('want_coords: the coordinates are those of one view')
    dev = _device_of(views)
    if lat.device != dev or lon.device != dev or lat.dtype != torch.float64 or lon.dtype != torch.float64:
        raise _l.SunerfHipError('map_rows: lat / lon must be float64 axes on the views\' device')
    lib = _l.load()
    if int(lib.sunerf_view_desc_bytes()) != VIEW_DESC.itemsize:
        raise _l.SunerfHipError('SunerfViewDesc: the library and sunerf_hip.observations disagree about its layout')
    n_lat, n_lon = int(lat.shape[0]), int(lon.shape[0])
    n_rows = n_lat - row_begin if n_rows is None else int(n_rows)
    if row_begin < 0 or n_rows < 0 or row_begin + n_rows > n_lat:
        raise ValueError(f'rows [{row_begin}, {row_begin + n_rows}) are outside the {n_lat} of the map')
    rows, _ = view_descriptors(views)
    desc = torch.from_numpy(rows.view(np.uint8).reshape(-1).copy()).to(dev)
    image = torch.empty(n_channels, n_rows, n_lon, dtype=torch.float32, device=dev)
    footprint = torch.empty(n_channels, n_rows, n_lon, dtype=torch.int32, device=dev)
    coords = torch.empty(3, n_rows, n_lon, dtype=torch.float64, device=dev) if want_coords else None
    for begin in range(0, n_rows, MAX_SLAB_ROWS):            # one launch unless the slab is taller than a grid
        n = min(MAX_SLAB_ROWS, n_rows - begin)
        if n == n_rows:
            out, fp, co = image, footprint, coords
        else:
            out, fp = torch.empty_like(image[:, :n]), torch.empty_like(footprint[:, :n])
            co = torch.empty_like(coords[:, :n]) if want_coords else None
        _l.call(dev, 'sunerf_synchronic_map', _ptr(desc), len(views), n_channels, _ptr(lat), n_lat, _ptr(lon), n_lon,
                row_begin + begin, n, radius, _ptr(out), _ptr(fp), _ptr(co), _stream(dev))
        if n != n_rows:
            image[:, begin:begin + n], footprint[:, begin:begin + n] = out, fp
            if want_coords:
                coords[:, begin:begin + n] = co
    return (image, footprint, coords) if want_coords else (image, footprint)


def fill_map(image: torch.Tensor, fill='mean') -> torch.Tensor:
    """``nan_to_num(image, nan=nanmean(image))`` per channel, in place (``sunerf_map_fill``, reprojection.py:90-92).
    ``fill``: ``'mean'``, None (NaNs stay) or a number.  Returns ``stats`` (C, 2) fp64 on the device: the mean of the non-NaN
    pixels of every channel and their number."""
    if not image.is_cuda or image.dtype != torch.float32 or not image.is_contiguous() or image.dim() != 3:
        raise _l.SunerfHipError('fill_map: the map must be a contiguous (C, n_lat, n_lon) float32 tensor on a ROCm device')
    if fill is None:
        mode, value = 0, 0.0
    elif isinstance(fill, str):
        if fill != 'mean':
            raise ValueError(f"fill must be 'mean', None or a number, not {fill!r}")
        mode, value = 1, 0.0
    else:
        mode, value = 2, float(fill)
    dev = image.device
    n_channels = image.shape[0]
    stats = torch.empty(n_channels, 2, dtype=torch.float64, device=dev)
    nbytes = int(_l.load().sunerf_map_fill_workspace_bytes(n_channels))
    ws = torch.empty(max(nbytes, 8), dtype=torch.uint8, device=dev)
    _l.call(dev, 'sunerf_map_fill', _ptr(image), n_channels, image.shape[1] * image.shape[2], mode, value, _ptr(stats), _ptr(ws),
            ws.numel(), _stream(dev))
    return stats


class Observer:
    """A new observer: position as ``ObservationSet.add_view`` takes it (radians and solar radii, or astropy quantities) and a
    pixel grid -- ``grid``, the plate-scale dict of ``sunerf.evaluation.loader``, or ``tx`` (W,) / ``ty`` (H,) axes [rad]."""

    def __init__(self, lat, lon, distance=AU_IN_SOLAR_RADII, grid: Optional[dict] = None, tx=None, ty=None, center=None):
        from sunerf.evaluation.loader import _radians, _solar_radii
        from .rays import pose_spherical
        self.lat, self.lon, self.distance = _radians(lat), _radians(lon), _solar_radii(distance)
        if grid is None and (tx is None or ty is None):
            raise ValueError('an observer needs grid= (plate-scale dict) or tx= / ty= (axes of pixel angles)')
        self.grid, self.tx, self.ty, self.center = grid, tx, ty, center
        self.c2w = pose_spherical(-self.lon, self.lat, self.distance, center)

    @classmethod
    def of_view(cls, view: View) -> 'Observer':
        """The observer of ``view``: its pose and its (downscaled) pixel grid."""
        if view.per_pixel:
            raise ValueError(f'view {view.name!r} has per-pixel angles: the reprojection baseline takes axes only')
        obs = cls.__new__(cls)
        obs.lat, obs.lon, obs.distance, obs.grid, obs.center = view.lat, view.lon, view.distance, view.grid, None
        obs.tx, obs.ty, obs.c2w = view.tx, view.ty, view.c2w
        return obs

    def axes(self, device) -> Tuple[torch.Tensor, torch.Tensor]:
        if self.tx is None:
            from sunerf.evaluation.loader import linear_plate_scale_axes
            self.tx, self.ty = linear_plate_scale_axes(self.grid, None, device)
        tx = torch.as_tensor(self.tx, dtype=torch.float64).to(device).contiguous()
        ty = torch.as_tensor(self.ty, dtype=torch.float64).to(device).contiguous()
        if tx.dim() != 1 or ty.dim() != 1 or tx.shape[0] < 1 or ty.shape[0] < 1:
            raise ValueError('an observer\'s tx / ty must be axes (W,) / (H,): per-pixel angles are not supported')
        self.tx, self.ty = tx, ty
        return tx, ty


def _as_observer(o) -> Observer:
    if isinstance(o, Observer):
        return o
    if isinstance(o, View):
        return Observer.of_view(o)
    if isinstance(o, dict):
        return Observer(**o)
    raise TypeError(f'an observer is an Observer, a View or a dict of Observer arguments, not {type(o).__name__}')


class SynchronicMap:
    """A heliographic map of the solar surface built from views.  ``image`` (C, n_lat, n_lon) fp32, ``footprint`` (the number of
    covering views, int32), ``lat`` / ``lon`` (fp64 axes of pixel centres [rad]) live on the device; ``covered_fraction`` is the
    share of pixels some view covered (before the fill), ``fill_value`` (C,) the per-channel mean of those pixels,
    ``wavelength`` (C,) the channels' values."""

    def __init__(self, image, footprint, lat, lon, Rs_per_ds, wavelength, covered_fraction, fill_value):
        self.image, self.footprint, self.lat, self.lon = image, footprint, lat, lon
        self.Rs_per_ds, self.wavelength = Rs_per_ds, wavelength
        self.covered_fraction, self.fill_value = covered_fraction, fill_value

    @property
    def shape(self) -> Tuple[int, int]:
        return int(self.image.shape[1]), int(self.image.shape[2])

    def _reproject(self, observers: Sequence, off_disk=None, want_coords: bool = False):
        observers = [_as_observer(o) for o in observers]
        if not observers:
            raise ValueError('no observers')
        dev = self.image.device
        if dev.type != 'cuda':
            raise _l.SunerfHipError('SynchronicMap.reproject: the map is on the CPU; reprojection runs on a ROCm device only')
        if int(_l.load().sunerf_observer_desc_bytes()) != OBSERVER_DESC.itemsize:
            raise _l.SunerfHipError('SunerfObserverDesc: the library and sunerf_hip.reprojection disagree about its layout')
        rows = np.zeros(len(observers), dtype=OBSERVER_DESC)
        keep, shapes, offset = [], [], 0
        for row, o in zip(rows, observers):
            tx, ty = o.axes(dev)
            keep.append((tx, ty))
            row['pix_offset'], row['tx'], row['ty'] = offset, tx.data_ptr(), ty.data_ptr()
            row['height'], row['width'] = ty.shape[0], tx.shape[0]
            row['c2w'] = np.asarray(o.c2w[:3, :4].reshape(-1).tolist(), dtype=np.float32)
            shapes.append((int(ty.shape[0]), int(tx.shape[0])))
            offset += shapes[-1][0] * shapes[-1][1]
        desc = torch.from_numpy(rows.view(np.uint8).reshape(-1).copy()).to(dev)
        n_channels = self.image.shape[0]
        out = torch.empty(offset, n_channels, dtype=torch.float32, device=dev)
        coords = torch.empty(3, offset, dtype=torch.float64, device=dev) if want_coords else None
        _l.call(dev, 'sunerf_reproject_views', _ptr(self.image), n_channels, _ptr(self.lat), self.lat.shape[0], _ptr(self.lon),
                self.lon.shape[0], _radius(self.Rs_per_ds), _ptr(desc), len(observers), offset,
                float('nan') if off_disk is None else float(off_disk), _ptr(out), _ptr(coords), _stream(dev))
        images, begin = [], 0
        for h, w in shapes:
            images.append(out[begin:begin + h * w].view(h, w, n_channels))
            begin += h * w
        return (images, coords) if want_coords else images

    def reproject_many(self, observers: Sequence, off_disk=None, want_coords: bool = False):
        """The map seen by every observer of ``observers`` (:class:`Observer`, ``View`` or dicts of :class:`Observer`'s
        arguments), one launch: a list of ``(H, W, C)`` fp32 device tensors (views into one buffer), the layout of
        ``render_observer_image(as_numpy=False)['image']``.  Off-disk pixels are NaN, or ``off_disk`` if given; pixels that
        look at a part of the sphere outside the map's axes are NaN.  ``want_coords``: also ``(3, n_pixels)`` fp64 -- map
        coordinates x (longitude axis), y (latitude axis) and ``1 - b^2 / R^2`` of every pixel, observers concatenated."""
        return self._reproject(observers, off_disk, want_coords)

    def reproject(self, lat, lon, distance=AU_IN_SOLAR_RADII, grid: Optional[dict] = None, tx=None, ty=None, center=None,
                  off_disk=None) -> torch.Tensor:
        """``h_map.reproject_to(observer)`` (reprojection.py:118-120) for one observer: ``(H, W, C)``."""
        return self._reproject([Observer(lat, lon, distance, grid, tx, ty, center)], off_disk)[0]

    def view_grid(self, strides_deg=10, distance=AU_IN_SOLAR_RADII, grid: Optional[dict] = None, tx=None, ty=None,
                  off_disk=None) -> Iterator[Tuple[Tuple[float, float], torch.Tensor]]:
        """``load_views`` (reprojection.py:128-168): yields ``((lat, lon) [deg], image (H, W, C))`` for the observers of
        ``mgrid[-90:91:s, 0:361:s]`` on one pixel grid -- all of them from one launch."""
        coords = view_grid_coordinates(strides_deg)
        template = Observer(0., 0., distance, grid, tx, ty)
        tx, ty = template.axes(self.image.device)
        observers = [Observer(np.deg2rad(float(b)), np.deg2rad(float(l)), distance, tx=tx, ty=ty) for b, l in coords]
        for (b, l), image in zip(coords, self._reproject(observers, off_disk)):
            yield (float(b), float(l)), image


def finish_map(image, footprint, lat, lon, Rs_per_ds, wavelength, fill='mean') -> SynchronicMap:
    """The fill and the statistics of an assembled coadd; the covered count is the one number that crosses to the host."""
    stats = fill_map(image, fill)
    covered = stats[:, 1].sum().item()
    fraction = covered / float(image.numel())
    if fraction < 0.5:
        warnings.warn('More than 50 percent of the heliographic map are NaNs!')       # reprojection.py:90-91
    return SynchronicMap(image, footprint, lat, lon, Rs_per_ds, wavelength, fraction, stats[:, 0])


def synchronic_map(views: Sequence[View], shape=(1024, 2048), lat_range=(-np.pi / 2, np.pi / 2), lon_range=(-np.pi, np.pi),
                   Rs_per_ds: float = 1.0, fill='mean', rank: Optional[int] = None, world: Optional[int] = None) -> SynchronicMap:
    """``create_heliographic_map(*views, shape_out=shape)`` (reprojection.py:52-95): every view projected onto the sphere
    ``r = 1 R_sun`` and sampled bilinearly at the map's pixel centres, the covering views averaged, and the pixels nothing covers
    filled -- ``fill='mean'``: the mean of the covered pixels of the channel (the reference), None: NaN, a number: that number.

    ``rank`` / ``world`` (default: the initialised process group, else a single process): each rank builds its
    ``shard_range`` of the rows, the slabs are gathered, and the fill is taken on the whole map, so every rank holds the same
    map, bit for bit, as a single process."""
    from .dist import shard_range
    from .maps import _gather_rows, _process_group
    n_channels = check_views(views)
    _radius(Rs_per_ds)
    lat_np, lon_np = map_axes(shape, lat_range, lon_range)
    if isinstance(fill, str) and fill != 'mean':
        raise ValueError(f"fill must be 'mean', None or a number, not {fill!r}")
    rank, world = _process_group(rank, world)
    if lat_np.shape[0] < world:
        raise ValueError(f'synchronic_map: {lat_np.shape[0]} rows cannot be shared by {world} ranks')
    dev = _device_of(views)
    lat, lon = torch.from_numpy(lat_np).to(dev), torch.from_numpy(lon_np).to(dev)
    begin, end = shard_range(lat_np.shape[0], rank, world)
    image, footprint = map_rows(views, lat, lon, Rs_per_ds, begin, end - begin)
    if world > 1:
        counts = [e - b for b, e in (shard_range(lat_np.shape[0], r, world) for r in range(world))]
        image = _gather_rows(image.permute(1, 0, 2).contiguous(), counts).permute(1, 0, 2).contiguous()
        footprint = _gather_rows(footprint.permute(1, 0, 2).contiguous(), counts).permute(1, 0, 2).contiguous()
    wavelength = np.max(np.stack([v.wavelength for v in views]), 0)
    return finish_map(image, footprint, lat, lon, Rs_per_ds, wavelength, fill)
