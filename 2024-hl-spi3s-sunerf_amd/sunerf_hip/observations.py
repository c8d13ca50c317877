"""Training sets from observation images, built on the device.

The reference turns images into a training set on the host (``sunerf/data/loader/single_channel.py:22-64``,
``multi_thermal_loader.py:37-75, 209-258``, ``base_loader.py:87-103``): per-pixel rays, the time broadcast, three full copies
and one ``np.random.permutation`` over all rays, written to ``*_batches.npy``.  Here the views stay where the renderer left
them: an :class:`ObservationSet` collects images, poses, times and pixel grids, and :meth:`ObservationSet.pool` has the kernel
``sunerf_build_ray_pool`` (``csrc/observations.hip``) write this rank's shard of the shuffled pool in one launch -- ray, time,
target and wavelength of every record.  The result is a :class:`sunerf_hip.feed.RayPool`, so ``training_batches`` and
``fit_steps`` read it unchanged.

Kept from the reference: the hold-out view ``len(views) // 6``, the record layout and file names, absent channels as
target 0 / wavelength 0, the mean over ``downscale x downscale`` blocks.  Deviations: the shuffle is a keyed bijection
(cycle-walking Feistel network, ``include/sunerf_hip.h``) instead of ``np.random.permutation``, so no table of the set's size
exists and any rank can build any slot; ``downscale`` must divide the image (``skimage.block_reduce`` pads with zeros);
pixels with a non-finite value are dropped (``drop_nonfinite``) instead of reaching the loss.
"""
import os
from datetime import datetime
from typing import Dict, List, Optional, Sequence

import numpy as np
import torch

from . import lib as _l
from ._ffi import _ptr, _stream
from .dist import shard_range
from .feed import RayPool

MAX_CHANNELS = 16           # SUNERF_OBS_MAX_CHANNELS
AU_IN_SOLAR_RADII = 215.03215567054764
POLARISED_PLANES = (1.0, 2.0)          # the wavelength labels of the two planes of a white-light view: total and polarised brightness

# struct SunerfViewDesc (include/sunerf_hip.h); the library's sizeof is compared when a table is first built
VIEW_DESC = np.dtype({
    'names': ['pix_offset', 'tx', 'ty', 'image', 'height', 'width', 'downscale', 'per_pixel', 'c2w', 'time', 'n_planes',
              'plane', 'wavelength'],
    'formats': ['<i8', '<u8', '<u8', '<u8', '<i4', '<i4', '<i4', '<i4', ('<f4', 12), '<f4', '<i4', ('<i4', MAX_CHANNELS),
                ('<f4', MAX_CHANNELS)],
    'offsets': [0, 8, 16, 24, 32, 36, 40, 44, 48, 96, 100, 104, 104 + 4 * MAX_CHANNELS],
    'itemsize': 104 + 8 * MAX_CHANNELS})

FILE_NAMES = {'rays': 'rays_batches.npy', 'time': 'times_batches.npy', 'target_image': 'images_batches.npy',
              'wavelength': 'wavelengths_batches.npy'}


def normalize_time(time, seconds_per_dt, ref_time) -> float:
    """``sunerf/data/date_util.py:4-17`` for a datetime; a number is taken as already normalised."""
    if isinstance(time, datetime):
        return (time - ref_time).total_seconds() / seconds_per_dt
    return float(time)


def resampled_grid(grid: dict, shape) -> dict:
    """The plate-scale dict of the same field of view on ``shape`` = (H, W) pixels, with ``crpix`` / ``crval`` spelled out:
    the arithmetic of ``sunerf.evaluation.loader.linear_plate_scale_axes(grid, resolution)``, so the axes of the result are
    the axes that function gives for the resampled frame, bit for bit."""
    h, w = grid['shape']
    cdx, cdy = grid['cdelt']
    cpx, cpy = grid.get('crpix', ((w + 1) / 2., (h + 1) / 2.))
    cvx, cvy = grid.get('crval', (0., 0.))
    nh, nw = int(shape[0]), int(shape[1])
    if (nh, nw) != (h, w):
        sx, sy = w / nw, h / nh
        cdx, cdy = cdx * sx, cdy * sy
        cpx, cpy = (cpx - 0.5) / sx + 0.5, (cpy - 0.5) / sy + 0.5
    out = {k: v for k, v in grid.items() if k not in ('shape', 'cdelt', 'crpix', 'crval')}
    out.update(shape=(nh, nw), cdelt=(cdx, cdy), crpix=(cpx, cpy), crval=(cvx, cvy))
    return out


def channel_map(wavelengths, n_planes: int):
    """(plane index or -1 per output channel, wavelength per channel) of a view that carries ``n_planes`` planes for the
    non-zero entries of ``wavelengths``, in order (multi_thermal_loader.py:243-254: absent channels are wavelength 0)."""
    wl = np.asarray(wavelengths, dtype=np.float32).reshape(-1)
    if not 1 <= wl.size <= MAX_CHANNELS:
        raise ValueError(f'a view has 1 to {MAX_CHANNELS} channels, got {wl.size}')
    present = wl != 0
    if int(present.sum()) != n_planes:
        raise ValueError(f'{int(present.sum())} non-zero wavelengths but {n_planes} image planes')
    plane = np.full(wl.size, -1, dtype=np.int32)
    plane[present] = np.arange(n_planes, dtype=np.int32)
    return plane, wl


def hold_out_index(n_views: int) -> int:
    """single_channel.py:35-37, multi_thermal_loader.py:47."""
    return n_views // 6


class View:
    """One observation: image planes on the device, pose, normalised time, the angles of its (downscaled) pixel grid."""

    def __init__(self, image, tx, ty, c2w, time, plane, wavelength, downscale, grid, name, lat, lon, distance, raw_time):
        self.image, self.tx, self.ty, self.c2w, self.time = image, tx, ty, c2w, time
        self.plane, self.wavelength, self.downscale, self.grid, self.name = plane, wavelength, downscale, grid, name
        self.lat, self.lon, self.distance, self.raw_time = lat, lon, distance, raw_time
        self.per_pixel = tx.dim() == 2
        self.height = image.shape[1] // downscale
        self.width = image.shape[2] // downscale

    @property
    def n_pixels(self) -> int:
        return self.height * self.width


def view_descriptors(views: Sequence[View]):
    """(``SunerfViewDesc`` rows as a numpy record array, total pixel count) of ``views`` concatenated in order."""
    rows = np.zeros(len(views), dtype=VIEW_DESC)
    offset = 0
    for row, v in zip(rows, views):
        row['pix_offset'] = offset
        row['tx'], row['ty'], row['image'] = v.tx.data_ptr(), v.ty.data_ptr(), v.image.data_ptr()
        row['height'], row['width'], row['downscale'], row['per_pixel'] = v.height, v.width, v.downscale, int(v.per_pixel)
        row['c2w'] = np.asarray(v.c2w[:3, :4].reshape(-1).tolist(), dtype=np.float32)
        row['time'] = np.float32(v.time)
        row['n_planes'] = v.image.shape[0]
        row['plane'][:] = -1
        row['plane'][:v.plane.size] = v.plane
        row['wavelength'][:v.wavelength.size] = v.wavelength
        offset += v.n_pixels
    return rows, offset


class _Table:
    """Device table of view descriptors + the ascending list of valid pixels (None: every pixel)."""

    def __init__(self, views: Sequence[View], device, drop_nonfinite: bool):
        if not views:
            raise ValueError('no views to build a ray set from')
        if int(_l.load().sunerf_view_desc_bytes()) != VIEW_DESC.itemsize:
            raise _l.SunerfHipError('SunerfViewDesc: the library and sunerf_hip.observations disagree about its layout')
        if torch.device(device).type != 'cuda':
            raise _l.SunerfHipError('ray pools are built by sunerf_build_ray_pool on a ROCm device (there is no CPU path)')
        self.views = list(views)              # keeps every tensor the table points to alive
        rows, self.n_pixels = view_descriptors(views)
        self.n_channels = int(views[0].plane.size)
        self.desc = torch.from_numpy(rows.view(np.uint8).reshape(-1).copy()).to(device)
        self.valid_index = None
        if drop_nonfinite:
            # torch ops (plumbing): a block mean is finite exactly when every source pixel of the block is
            masks = []
            for v in views:
                ok = torch.isfinite(v.image).all(0)
                if v.downscale > 1:
                    ok = ok.view(v.height, v.downscale, v.width, v.downscale).all(3).all(1)
                masks.append(ok.reshape(-1))
            mask = torch.cat(masks)
            if not bool(mask.all()):
                self.valid_index = mask.nonzero().reshape(-1).contiguous()
        self.n_valid = self.n_pixels if self.valid_index is None else int(self.valid_index.numel())
        if self.n_valid < 1:
            raise ValueError('no valid pixel in the views')
        self.device = self.desc.device

    def empty(self, n: int, with_wavelength: bool) -> Dict[str, torch.Tensor]:
        out = {'rays': torch.empty(n, 2, 3, dtype=torch.float32, device=self.device),
               'time': torch.empty(n, 1, dtype=torch.float32, device=self.device),
               'target_image': torch.empty(n, self.n_channels, dtype=torch.float32, device=self.device)}
        if with_wavelength:
            out['wavelength'] = torch.empty(n, self.n_channels, dtype=torch.float32, device=self.device)
        return out

    def build(self, out: Dict[str, torch.Tensor], slot_begin: int, n_slots: int, permute: bool, seed: int = 0, epoch: int = 0):
        """Records ``[slot_begin, slot_begin + n_slots)`` into the first ``n_slots`` rows of ``out``'s tensors."""
        if n_slots > out['rays'].shape[0]:
            raise ValueError('output tensors are smaller than the slot range')
        _l.call(self.device, 'sunerf_build_ray_pool', _ptr(self.desc), len(self.views), self.n_pixels, _ptr(self.valid_index),
                self.n_valid, self.n_channels, 1 if permute else 0, int(seed) & (2 ** 64 - 1), int(epoch) & (2 ** 64 - 1),
                int(slot_begin), int(n_slots), _ptr(out['rays']), _ptr(out['time']), _ptr(out.get('target_image')),
                _ptr(out.get('wavelength')), _stream(self.device))


class ObservationPool(RayPool):
    """This rank's shard ``shard_range(V, rank, world)`` of the permuted ray set of an :class:`ObservationSet`, as a
    :class:`RayPool`: ``batch``, ``order``, ``len`` and iteration as there.

    ``reshuffle='batches'``: the shard is built once with key ``(seed, 0)``; an epoch visits its fixed batches in a fresh
    order (the reference's semantics).  ``reshuffle='rays'``: the shard is rebuilt IN PLACE with key ``(seed, epoch)`` at the
    start of every epoch -- a fresh permutation of all rays; batches are then read front to back, and a batch (a view) kept
    from an earlier epoch shows the new records."""

    def __init__(self, table: _Table, with_wavelength: bool, batch_size: int, rank: int, world: int, seed: int,
                 reshuffle: str, drop_last: bool = False):
        if reshuffle not in ('batches', 'rays'):
            raise ValueError(f"reshuffle must be 'batches' or 'rays', got {reshuffle!r}")
        self.table, self.reshuffle = table, reshuffle
        self.total_rays = table.n_valid
        self.begin, self.end = shard_range(self.total_rays, rank, world)
        self.batch_size, self.shuffle, self.seed, self.drop_last = int(batch_size), reshuffle == 'batches', seed, drop_last
        self.rank, self.world = rank, world
        self.data = table.empty(self.n_rays, with_wavelength)
        self.epoch = 0
        self.rebuild(0)

    def rebuild(self, epoch: int):
        """One kernel launch: the shard under key ``(seed, epoch)``."""
        self.table.build(self.data, self.begin, self.n_rays, True, self.seed, epoch)
        self.built_epoch = epoch

    def __iter__(self):
        if self.reshuffle == 'batches':
            yield from super().__iter__()
            return
        if self.built_epoch != self.epoch:
            self.rebuild(self.epoch)
        self.epoch += 1
        for i in range(len(self)):
            yield self.batch(i)


class ObservationSet:
    """Views in, shuffled and rank-sharded ray pool out.  Carries what ``sunerf.model.sunerf.save_state`` reads from a data
    module (``config``, ``Rs_per_ds``, ``seconds_per_dt``, ``ref_time``)."""

    def __init__(self, Rs_per_ds=1.0, seconds_per_dt=86400.0, ref_time: Optional[datetime] = None, device='cuda',
                 wavelength=None):
        self.Rs_per_ds, self.seconds_per_dt, self.ref_time = Rs_per_ds, seconds_per_dt, ref_time
        self.device = torch.device(device)
        self.wavelength = wavelength            # label of a single-channel set (config['wavelength'])
        self.views: List[View] = []
        self._single = True                     # no wavelength array: set by the first view
        self._held = None
        self._tables = {}

    # ---------------------------------------------------------------- views
    def add_view(self, image, lat, lon, distance=AU_IN_SOLAR_RADII, time=0.0, grid: Optional[dict] = None, tx=None, ty=None,
                 wavelengths=None, downscale: int = 1, center=None, name: Optional[str] = None) -> int:
        """Adds one view and returns its index.

        ``image``: ``(H, W)`` or ``(C_present, H, W)``, fp32, on the device (kept, not copied) or on the host (uploaded once).
        ``lat`` / ``lon`` / ``distance`` / ``center``: as ``render_observer_image`` takes them (radians and solar radii, or
        astropy quantities).  ``time``: a datetime (normalised like ``date_util.normalize_datetime``; the first one becomes
        ``ref_time`` if none was given) or an already normalised number.  Pixel grid: ``grid``, the plate-scale dict of
        ``sunerf.evaluation.loader`` for the image as given, or ``tx`` / ``ty`` angles [rad, fp64] of the grid AFTER the
        downscale (two axes ``(W,)``, ``(H,)`` or per-pixel ``(H, W)``).  ``wavelengths``: ``(W,)`` with 0 for the channels
        this view lacks; None: a single channel.  All views of a set have the same number of channels."""
        from sunerf.evaluation.loader import _radians, _solar_radii, linear_plate_scale_axes
        from .rays import pose_spherical
        image = torch.as_tensor(image)
        if image.dim() == 2:
            image = image[None]
        if image.dim() != 3 or image.shape[1] < 1 or image.shape[2] < 1:
            raise ValueError(f'image must be (H, W) or (C, H, W), got {tuple(image.shape)}')
        downscale = int(downscale)
        if downscale < 1 or image.shape[1] % downscale or image.shape[2] % downscale:
            raise ValueError(f'downscale {downscale} does not divide the {image.shape[1]} x {image.shape[2]} image '
                             '(skimage.block_reduce would pad with zeros: not supported)')
        height, width = image.shape[1] // downscale, image.shape[2] // downscale
        if wavelengths is None:
            plane, wl = channel_map([1.0], image.shape[0])
            single = True
        else:
            plane, wl = channel_map(wavelengths, image.shape[0])
            single = False
        if self.views and (plane.size != self.views[0].plane.size or single != self._single):
            raise ValueError('all views of a set carry the same number of channels')
        if grid is not None:
            if tuple(grid['shape']) != (image.shape[1], image.shape[2]):
                raise ValueError(f"grid shape {tuple(grid['shape'])} is not the image's {tuple(image.shape[1:])}")
            grid = resampled_grid(grid, (height, width))
            tx, ty = linear_plate_scale_axes(grid, None, self.device)
        elif tx is None or ty is None:
            raise ValueError('a view needs grid= (plate-scale dict) or tx= / ty= (pixel angles)')
        else:
            tx = torch.as_tensor(tx, dtype=torch.float64).to(self.device).contiguous()
            ty = torch.as_tensor(ty, dtype=torch.float64).to(self.device).contiguous()
            if tx.dim() == 2:
                if tx.shape != ty.shape or tuple(tx.shape) != (height, width):
                    raise ValueError(f'per-pixel tx / ty must be ({height}, {width})')
            elif tx.dim() != 1 or ty.dim() != 1 or tx.shape[0] != width or ty.shape[0] != height:
                raise ValueError(f'tx / ty must be axes of {width} / {height} angles or per-pixel ({height}, {width})')
        if isinstance(time, datetime) and self.ref_time is None:
            self.ref_time = time
        lat_r, lon_r, dist = _radians(lat), _radians(lon), _solar_radii(distance)
        view = View(image.to(device=self.device, dtype=torch.float32).contiguous(), tx, ty,
                    pose_spherical(-lon_r, lat_r, dist, center), normalize_time(time, self.seconds_per_dt, self.ref_time),
                    plane, wl, downscale, grid, name if name is not None else f'view{len(self.views)}', lat_r, lon_r, dist, time)
        self._single = single
        self.views.append(view)
        self._tables = {}
        return len(self.views) - 1

    def add_prepared_view(self, image, wcs: dict, lat, lon, distance=AU_IN_SOLAR_RADII, time=0.0, wavelengths=None,
                          downscale: int = 1, center=None, name: Optional[str] = None, **prep) -> int:
        """Prepares a detector image on the device (``sunerf_hip.prep.prepare_image(image, wcs, **prep)``: roll to north,
        recentre, one plate scale, scaling, norm and clips) and adds the result with the grid it was
        prepared on: ``add_view(prepared, ..., grid=prepared grid)``.  ``wcs``: the plate-scale dict of the image as given, with
        an optional ``'crota'`` or ``'pc'``.  With ``nan_policy='propagate'`` the pixels that saw a non-finite input pixel are NaN
        and ``pool(drop_nonfinite=True)`` leaves their rays out."""
        from .prep import prepare_image
        prepared, grid = prepare_image(image, wcs, device=self.device, **prep)
        return self.add_view(prepared, lat, lon, distance, time, grid=grid, wavelengths=wavelengths, downscale=downscale,
                             center=center, name=name)

    def add_polarised_view(self, frames, angles, lat, lon, distance=AU_IN_SOLAR_RADII, time=0.0, grid: Optional[dict] = None,
                           tx=None, ty=None, center=None, name: Optional[str] = None, **stokes_kw) -> dict:
        """Adds the white-light view that ``N`` exposures through a linear polariser make: ``frames`` [N, H, W] at the polariser
        ``angles`` go through :func:`sunerf_hip.polarimetry.stokes` (``throughput``, ``efficiency``, ``a``, ``b``, ``bad``), and the
        ``(tB, pB)`` pair becomes a two-plane view -- the planes ``ThompsonScattering`` renders -- with the wavelength labels
        ``POLARISED_PLANES``.  ``center = (cy, cx)``: the Sun's centre in pixels; default: where the view's pixel axes cross zero
        angle (``enhance.sun_geometry``).  UNDETERMINED pixels (and pB on the centre pixel) are NaN, so
        ``pool(drop_nonfinite=True)`` leaves their rays out.  Returns the Stokes dict, with the view's ``index``."""
        from .enhance import sun_geometry
        from .polarimetry import stokes
        from .reprojection import Observer
        frames = torch.as_tensor(frames)
        if frames.dim() != 3:
            raise ValueError(f'add_polarised_view: frames must be (N, H, W) exposures of one detector, got {tuple(frames.shape)}')
        if center is None:
            center, _ = sun_geometry(Observer(lat, lon, distance, grid=None if grid is None else dict(grid), tx=tx, ty=ty), self.Rs_per_ds)
        out = stokes(frames.to(device=self.device, dtype=torch.float32), angles, center=center, **stokes_kw)
        out['index'] = self.add_view(torch.stack([out['tb'], out['pb']]), lat, lon, distance, time, grid=grid, tx=tx, ty=ty,
                                     wavelengths=POLARISED_PLANES, name=name)
        return out

    def add_rendered_view(self, loader, lat, lon, time, distance=AU_IN_SOLAR_RADII, wl=None, resolution=None, center=None,
                          key: str = 'image', scale: float = 1.0, **kwargs) -> int:
        """Renders the loader's model from (lat, lon, distance) at ``time`` with ``render_observer_image(as_numpy=False)`` and
        adds the frame -- which never leaves the device -- with the loader's own pixel grid.  ``wl``: the channels of a
        density-temperature rendering (``ModelLoader``); they become the view's ``wavelengths``.  ``scale`` multiplies the
        frame (on the device), e.g. to images of order one as the reference's loaders normalise them."""
        extra = {} if wl is None else {'wl': wl}
        frame = loader.render_observer_image(lat, lon, time, distance=distance, center=center, resolution=resolution,
                                             as_numpy=False, **extra)
        image = frame[key].permute(2, 0, 1).contiguous()
        if scale != 1.0:
            image = image * scale
        if isinstance(loader.ref_map, dict):
            grid = resampled_grid(loader.ref_map, image.shape[1:]) if resolution is not None else dict(loader.ref_map)
            return self.add_view(image, lat, lon, distance, time, grid=grid, wavelengths=wl, center=center, **kwargs)
        tx, ty = loader._pixel_angles(resolution)
        return self.add_view(image, lat, lon, distance, time, tx=tx, ty=ty, wavelengths=wl, center=center, **kwargs)

    def hold_out(self, which='reference'):
        """``'reference'``: view ``len(views) // 6``, resolved when a pool is built; or an index / indices; None: nothing."""
        if which is not None and not isinstance(which, str):
            which = [int(which)] if np.isscalar(which) else [int(i) for i in which]
        elif isinstance(which, str) and which != 'reference':
            raise ValueError("hold_out takes 'reference', indices or None")
        self._held = which
        self._tables = {}

    @property
    def held_out(self) -> List[int]:
        if self._held is None:
            return []
        if isinstance(self._held, str):
            return [hold_out_index(len(self.views))] if self.views else []
        for i in self._held:
            if not 0 <= i < len(self.views):
                raise IndexError(f'held-out view {i} of {len(self.views)}')
        return sorted(set(self._held))

    @property
    def training_views(self) -> List[int]:
        held = set(self.held_out)
        return [i for i in range(len(self.views)) if i not in held]

    def _table(self, indices: Sequence[int], drop_nonfinite: bool) -> _Table:
        key = (tuple(indices), bool(drop_nonfinite))
        if key not in self._tables:
            self._tables[key] = _Table([self.views[i] for i in indices], self.device, drop_nonfinite)
        return self._tables[key]

    # ---------------------------------------------------------------- outputs
    def pool(self, batch_size: int = 2 ** 13, rank: int = 0, world: int = 1, seed: int = 0, reshuffle: str = 'batches',
             drop_nonfinite: bool = True, drop_last: bool = False) -> ObservationPool:
        """The training views as a device-resident :class:`ObservationPool`: rank ``rank`` of ``world`` holds slots
        ``shard_range(V, rank, world)`` of one permutation of the ``V`` valid pixels."""
        return ObservationPool(self._table(self.training_views, drop_nonfinite), not self._single, batch_size, rank, world,
                               seed, reshuffle, drop_last)

    def patch_pool(self, instrument, patch: int = 16, patches_per_batch=None, rank: int = 0, world: int = 1, seed: int = 0):
        """The training views as a :class:`sunerf_hip.patch.PatchPool` for training THROUGH ``instrument``:
        patches of ``patch x patch`` detector pixels on the lattice 0, P, 2 P, ... of every view, the last patch of an axis
        shifted inward so that it ends at the edge (every pixel is covered, a few twice); a view smaller than ``patch`` raises.
        Patches whose target holds a non-finite value are dropped and counted (``pool.dropped``).  Epoch ``e`` visits the
        patches in the order ``np.random.default_rng([seed, e]).permutation(n_patches)``, rank ``r`` taking ``[r::world]``:
        ranks need nothing from each other.  ``patches_per_batch``: default what brings a batch nearest to 8192 rays.  The
        views must have uniform 1-d axes and ``downscale == 1`` (the instrument's ``bin`` does the averaging)."""
        from .patch import PatchPool
        return PatchPool([self.views[i] for i in self.training_views], instrument, self.device, not self._single, patch,
                         patches_per_batch, rank, world, seed)

    def validation_batches(self, batch_size: int = 2 ** 13) -> List[dict]:
        """One entry per held-out view: ``{'name', 'index', 'image_shape': (H, W), 'batches': [...]}`` with the view's rays in
        pixel order (nothing dropped, nothing shuffled) as the batch dicts ``validation_step`` reads; ``image_shape`` is
        what ``validation_metrics`` takes."""
        out = []
        for i in self.held_out:
            table = self._table([i], False)
            data = table.empty(table.n_pixels, not self._single)
            table.build(data, 0, table.n_pixels, False)
            batches = [{k: v[b:b + batch_size] for k, v in data.items()} for b in range(0, table.n_pixels, int(batch_size))]
            v = self.views[i]
            out.append({'name': v.name, 'index': i, 'image_shape': (v.height, v.width), 'batches': batches})
        return out

    def write_npy(self, working_dir: str, seed: int = 0, drop_nonfinite: bool = True, chunk_rays: int = 1 << 22) -> Dict[str, str]:
        """The reference's files -- ``rays_batches.npy (P,2,3)``, ``times_batches.npy (P,1)``, ``images_batches.npy (P,C)`` and,
        for a multi-channel set, ``wavelengths_batches.npy (P,C)`` -- holding the records of ``pool(world=1, seed=seed)``,
        streamed chunk by chunk through ``np.lib.format.open_memmap``.  Returns name -> path as ``MmapDataset`` /
        ``RayPool.from_files`` take it."""
        os.makedirs(working_dir, exist_ok=True)
        table = self._table(self.training_views, drop_nonfinite)
        chunk_rays = max(1, min(int(chunk_rays), table.n_valid))
        stage = table.empty(chunk_rays, not self._single)
        paths = {k: os.path.join(working_dir, FILE_NAMES[k]) for k in stage}
        files = {k: np.lib.format.open_memmap(paths[k], mode='w+', dtype=np.float32, shape=(table.n_valid,) + tuple(v.shape[1:]))
                 for k, v in stage.items()}
        for begin in range(0, table.n_valid, chunk_rays):
            n = min(chunk_rays, table.n_valid - begin)
            table.build(stage, begin, n, True, seed, 0)
            for k, v in stage.items():
                files[k][begin:begin + n] = v[:n].cpu().numpy()
        for f in files.values():
            f.flush()
        return paths

    # ---------------------------------------------------------------- reprojection baseline
    def _baseline_index(self, index: Optional[int]) -> int:
        if index is None:
            held = self.held_out
            if not held:
                raise ValueError('no view is held out: name the view (index=) or call hold_out first')
            return held[0]
        if not 0 <= int(index) < len(self.views):
            raise IndexError(f'view {index} of {len(self.views)}')
        return int(index)

    def synchronic_map(self, indices: Optional[Sequence[int]] = None, **kw):
        """The :class:`sunerf_hip.reprojection.SynchronicMap` of the training views (default: ``training_views``, so a held-out
        view is never part of its own baseline) or of the views ``indices``; ``kw`` as ``reprojection.synchronic_map`` takes
        them (``shape``, ``lat_range``, ``lon_range``, ``fill``, ``rank``, ``world``)."""
        from .reprojection import synchronic_map
        indices = self.training_views if indices is None else [int(i) for i in indices]
        kw.setdefault('Rs_per_ds', self.Rs_per_ds)
        return synchronic_map([self.views[i] for i in indices], **kw)

    def baseline_view(self, index: Optional[int] = None, off_disk=None, **kw) -> torch.Tensor:
        """The held-out view (the first one; or view ``index``) as the reprojection baseline predicts it: the synchronic map
        of the training views -- without view ``index`` -- seen from that view's pose on its own (downscaled) pixel grid,
        ``(H, W, C)`` fp32 with the set's channels.  Off the disk NaN, or ``off_disk``.  ``kw``: as :meth:`synchronic_map`."""
        from .reprojection import Observer
        index = self._baseline_index(index)
        observer = Observer.of_view(self.views[index])              # (refuses per-pixel grids before anything is built)
        indices = kw.pop('indices', None)
        if indices is None:
            indices = [i for i in self.training_views if i != index]
        return self.synchronic_map(indices, **kw).reproject_many([observer], off_disk)[0]

    def baseline_metrics(self, index: Optional[int] = None, data_range: float = 1.0, normalize=None, **kw) -> Dict[str, torch.Tensor]:
        """``image_metrics`` of :meth:`baseline_view` against the view's own image, per channel the view has, as
        ``baseline_simulation.py:35-42`` scores it: ``nan_to_num(prediction, nan=0)``, then ``normalize`` (an optional callable,
        e.g. the scripts' asinh stretch) on both.  Keys and shapes ``(C_present,)`` as ``image_metrics``."""
        from .metrics import image_metrics
        index = self._baseline_index(index)
        view = self.views[index]
        pred = self.baseline_view(index, **kw).permute(2, 0, 1)
        present = torch.as_tensor(np.nonzero(view.plane >= 0)[0], device=pred.device)
        pred = torch.nan_to_num(pred.index_select(0, present), nan=0.0)
        target = view.image
        if view.downscale > 1:
            f = view.downscale
            target = (target.double().view(-1, view.height, f, view.width, f).sum((2, 4)) / float(f * f)).float()
        if normalize is not None:
            pred, target = normalize(pred), normalize(target)
        return image_metrics(pred.contiguous(), target.contiguous(), data_range)

    # ---------------------------------------------------------------- registration
    def register_views(self, indices: Optional[Sequence[int]] = None, reference: Optional[int] = None, **kw) -> dict:
        """The views ``indices`` (default: all) put onto the grid, observer and time of view ``reference`` (default: the first of
        ``indices``): :func:`sunerf_hip.register.register_frames` with each view's own ``c2w``, axes and normalised time.  The
        ``image`` of the result, ``[T, C, H, W]``, is the stack that ``combine``, ``background`` and ``noise_gate`` take.  ``kw`` as
        ``register_frames`` takes them (``rotation``, ``order``, ``off_disk``, ``shifts``, ...); ``Rs_per_ds`` and ``seconds_per_dt``
        default to the set's.  Views with per-pixel angles or a downscale are refused."""
        from .register import register_frames
        indices = list(range(len(self.views))) if indices is None else [int(i) for i in indices]
        if not indices:
            raise ValueError('register_views: no views')
        reference = indices[0] if reference is None else int(reference)
        for i in indices + [reference]:
            if not 0 <= i < len(self.views):
                raise IndexError(f'view {i} of {len(self.views)}')
            v = self.views[i]
            if v.per_pixel:
                raise ValueError(f'{v.name}: registration needs a view with 1-d pixel axes (per-pixel angles are not supported)')
            if v.downscale != 1:
                raise ValueError(f'{v.name}: registration samples the image planes as they are (downscale {v.downscale} is not supported)')
        views = [self.views[i] for i in indices]
        kw.setdefault('Rs_per_ds', self.Rs_per_ds)
        kw.setdefault('seconds_per_dt', self.seconds_per_dt)
        return register_frames([v.image for v in views], views, [v.time for v in views], reference=self.views[reference],
                               reference_time=self.views[reference].time, **kw)

    # ---------------------------------------------------------------- co-alignment
    def _pixel_sizes(self, view: View):
        """Refuses a view whose pointing cannot be moved by a shift of its axes, as ``patch_pool`` refuses; for a view without
        a plate-scale dict the pixel sizes ``(delta_x, delta_y)`` of its uniform axes (read on the host), else None."""
        from .patch import UNIFORM_TOLERANCE
        if view.per_pixel:
            raise ValueError(f'{view.name}: co-alignment needs a view with 1-d pixel axes (per-pixel angles are not supported)')
        if view.grid is not None:
            return None
        deltas = []
        for axis in (view.tx, view.ty):
            a = axis.detach().cpu().numpy()
            if a.shape[0] < 2:
                raise ValueError(f'{view.name}: an axis of one pixel has no pixel size')
            delta = (a[-1] - a[0]) / (a.shape[0] - 1)
            if delta == 0 or np.abs(a - (a[0] + np.arange(a.shape[0]) * delta)).max() > UNIFORM_TOLERANCE * abs(delta):
                raise ValueError(f'{view.name}: co-alignment needs a uniform pixel axis')
            deltas.append(float(delta))
        return tuple(deltas)

    def _move_pointing(self, view: View, dy: float, dx: float, deltas) -> None:
        from sunerf.evaluation.loader import linear_plate_scale_axes
        from .coalign import shifted_grid
        if view.grid is not None:
            view.grid = shifted_grid(view.grid, dy, dx)
            view.tx, view.ty = linear_plate_scale_axes(view.grid, None, self.device)
        else:          # new[c + dx] = old[c] on a uniform axis: every angle moves by -dx pixel sizes
            view.tx = (view.tx - dx * deltas[0]).contiguous()
            view.ty = (view.ty - dy * deltas[1]).contiguous()
        self._tables = {}

    def coalign_view(self, index: int, reference='baseline', max_shift=8, min_overlap: float = 0.5, measure: str = 'zncc',
                     combine: str = 'shared', apply: bool = True, **baseline_kw) -> dict:
        """Finds the pointing offset of view ``index`` against a prediction of it and, with ``apply``, moves the view's pixel
        grid by it (``sunerf_hip.coalign``).  The image itself is never resampled.

        The view's image (the mean over its ``downscale`` blocks, as :meth:`baseline_metrics` forms it) is correlated with
        ``reference`` over the shifts ``|dy|, |dx| <= max_shift``: ``'baseline'``, :meth:`baseline_view` of the view on its
        present channels -- without that view; its off-disk NaN takes no part (``baseline_kw`` go to it) -- or a tensor
        ``[C_present, H, W]`` on the view's grid, e.g. a model's render of that view.  ``min_overlap``, ``measure`` and
        ``combine`` as ``coalign.coalign`` takes them.

        With ``apply`` (it needs ``combine='shared'``: a view has one pointing) and a status free of ``NO_PEAK``, the view's
        ``grid`` becomes ``shifted_grid(grid, dy, dx)``, its ``tx`` / ``ty`` are rebuilt and the cached pools' tables are dropped;
        a view added with uniform 1-d ``tx`` / ``ty`` and no ``grid`` has its axes moved by the same rule.  A view with per-pixel
        angles or a non-uniform axis is refused.  Returns the dict of ``coalign.coalign`` plus ``applied``.  The one host wait is
        reading the shift in order to apply it."""
        from .coalign import NO_PEAK, coalign
        index = self._baseline_index(int(index))
        view = self.views[index]
        if apply and combine != 'shared':
            raise ValueError("apply needs combine='shared': a view has one pointing")
        deltas = self._pixel_sizes(view)
        present = torch.as_tensor(np.nonzero(view.plane >= 0)[0], device=self.device)
        target = view.image
        if view.downscale > 1:
            f = view.downscale
            target = (target.double().view(-1, view.height, f, view.width, f).sum((2, 4)) / float(f * f)).float()
        if isinstance(reference, str):
            if reference != 'baseline':
                raise ValueError(f"reference must be 'baseline' or a tensor [C_present, H, W], got {reference!r}")
            template = self.baseline_view(index, **baseline_kw).permute(2, 0, 1).index_select(0, present)
        else:
            template = torch.as_tensor(reference)
            template = template[None] if template.dim() == 2 else template
            if tuple(template.shape) != tuple(target.shape):
                raise ValueError(f'{view.name}: reference must be {tuple(target.shape)} (the view\'s present channels on its grid), '
                                 f'got {tuple(template.shape)}')
            template = template.to(device=self.device, dtype=torch.float32)
        out = coalign(target.contiguous(), template.contiguous(), max_shift, measure=measure, min_overlap=min_overlap, combine=combine)
        out['applied'] = False
        if apply:
            dy, dx, status = torch.cat([out['shift'], out['status'].double()[None]]).tolist()          # the one host wait
            if not int(status) & NO_PEAK:
                self._move_pointing(view, dy, dx, deltas)
                out['applied'] = True
        return out

    def coalign_views(self, indices: Optional[Sequence[int]] = None, anchor: Optional[int] = None, passes: int = 1, **kw) -> List[dict]:
        """Co-aligns the training views (or ``indices``) with each other: each pass estimates every one of them except
        ``anchor`` against the reprojection baseline of the OTHER training views as they stand (:meth:`coalign_view` with
        ``apply=False``) and then applies all shifts together -- those whose status is free of ``NO_PEAK`` and of ``EDGE``: a peak
        on the border of the window is no located maximum (a view of a bland part of the scene gives such peaks), and moving a
        view by it would spoil the baselines of the next pass.  Returns one dict per pass, view index -> ``{'shift': (dy, dx),
        'status', 'score', 'applied'}`` as Python numbers.

        A shift common to all views cannot be observed -- every baseline moves with it -- so the mean pointing of the set stays
        what the headers said; ``anchor`` names a view whose pointing is trusted and fixes it: that view is never moved, and
        further passes pull the others towards it.  ``kw``: as :meth:`coalign_view` takes them (``apply`` is not among them)."""
        from .coalign import EDGE, NO_PEAK
        if 'apply' in kw or 'reference' in kw:
            raise ValueError('coalign_views estimates against the baseline and applies all shifts of a pass together')
        indices = self.training_views if indices is None else [int(i) for i in indices]
        indices = [i for i in indices if anchor is None or i != int(anchor)]
        history = []
        for _ in range(int(passes)):
            found = [self.coalign_view(i, apply=False, **kw) for i in indices]
            if not found:
                history.append({})
                continue
            rows = torch.stack([torch.cat([f['shift'], f['status'].double()[None], f['score'][None]]) for f in found]).tolist()
            result = {}
            for i, (dy, dx, status, score) in zip(indices, rows):          # one host wait per pass, then every view moves
                applied = not int(status) & (NO_PEAK | EDGE)
                if applied:
                    self._move_pointing(self.views[i], dy, dx, self._pixel_sizes(self.views[i]))
                result[i] = {'shift': (dy, dx), 'status': int(status), 'score': score, 'applied': applied}
            history.append(result)
        return history

    @property
    def config(self) -> dict:
        """What ``save_state`` stores as ``data_config`` (single_channel.py:82-84, multi_thermal_loader.py:88-90), with ``wcs``
        the plate-scale dict of the held-out (else first) view so that ``SuNeRFLoader`` renders that view's frame."""
        held = self.held_out
        ref = self.views[held[0] if held else 0] if self.views else None
        config = {'type': 'emission' if self._single else 'D_T', 'Rs_per_ds': self.Rs_per_ds,
                  'seconds_per_dt': self.seconds_per_dt, 'ref_time': self.ref_time,
                  'wcs': None if ref is None else ref.grid,
                  'resolution': None if ref is None else (ref.height, ref.width),
                  'times': [v.raw_time for v in self.views]}
        if self._single:
            config['wavelength'] = self.wavelength
        else:
            config['wavelengths'] = None if ref is None else ref.wavelength.copy()
        return config
