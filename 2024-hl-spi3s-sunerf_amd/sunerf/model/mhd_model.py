"""Mirror of the reference's ``sunerf/model/mhd_model.py``: a PSI MHD simulation (density ``rho`` and temperature ``t``
cubes, one HDF5 file per frame and variable) that pretends to be a trained ``NeRF_DT`` when synthetic observations are
rendered (evaluation/image_render.py:244-269).

Same constructor arguments (plus ``reader`` and ``max_frames``), parameters and state-dict keys; the field is evaluated by
``sunerf_mhd_field`` / ``sunerf_mhd_field_points`` (csrc/mhd.hip) on frames kept resident on the device, instead of a
scipy ``RegularGridInterpolator`` built on the CPU from the files for every batch (mhd_model.py:45-75, :114-138).

One deliberate deviation: the answer of :meth:`MHDModel.forward` carries ``'inferences'`` -- the same tensor as ``'rho_T'``
-- because the density / temperature renderer reads that key (density_temperature.py:181); with ``'rho_T'`` alone the
reference's own renderer fails with a ``KeyError``."""
import ctypes
import glob
import os
import weakref
from collections import OrderedDict

import numpy as np
import torch
from torch import nn

from sunerf.model.model import absorption_scalars
from sunerf_hip import ops

FILL_VALUE = 1e-10              # mhd_model.py:45 / :108: outside the grid, and the clamp of negative data (:64)
VARIABLES = ('rho', 't')


def frame_number(path: str) -> int:
    """mhd_model.py:29-30: ``int(name.split('00')[1].split('.h5')[0])`` -- e.g. ``rho002531.h5`` -> 2531.

    The parse is kept with its quirk: a frame number that itself contains ``00`` is cut at it (``rho002500.h5`` -> 25,
    ``rho001005.h5`` -> 1), so a directory gives exactly the reference's frames.  It is applied to the file
    NAME: the reference splits the whole path, so there a ``00`` anywhere in the directory names breaks the parse."""
    return int(os.path.basename(path).split('00')[1].split('.h5')[0])


def frame_file(data_path: str, var: str, frame: int) -> str:
    """mhd_model.py:62: ``{data_path}/{var}/{var}00{frame}.h5``."""
    return os.path.join(data_path, var, f'{var}00{frame}.h5')


def read_psi_hdf5(path: str):
    """``(r, theta, phi, data)`` of a PSI 3-D HDF5 file: the ``Data`` dataset, indexed ``data[i_phi, i_theta, i_r]``, and
    the dimension scales attached to its dimensions in PSI's own order, which is the Fortran one: ``Data.dims[0]`` carries
    r (``dim1``, the length of the LAST data axis), ``dims[1]`` theta, ``dims[2]`` phi -- what PSI's ``rdhdf_3d`` returns as
    ``(x, y, z, f)`` and mhd_model.py:62 unpacks as ``r, th, phi``."""
    try:
        import h5py
    except ImportError as err:
        raise ImportError(f'reading {path} needs h5py; install it, or pass MHDModel(..., reader=callable) with a callable '
                          'path -> (r, theta, phi, data)') from err
    with h5py.File(path, 'r') as h5:
        ds = h5['Data']
        if ds.ndim != 3 or any(len(ds.dims[k]) == 0 for k in range(3)):
            raise ValueError(f'{path}: expected a 3-D "Data" dataset with a dimension scale on every dimension')
        r, theta, phi = (np.asarray(ds.dims[k][0][...]).reshape(-1) for k in range(3))
        return r, theta, phi, np.asarray(ds[...])


class FrameCache:
    """The frames of one simulation resident on one device, shared by every ``MHDModel`` of the same directory and reader
    (the coarse and the fine model of a renderer): at most ``capacity`` frames, least recently used evicted first.

    ``frames`` (uint8 records of ``ops.MhdFrame``, one per slot) and ``slot`` (int32, the slot of frame ffirst + i or -1) are
    the kernel's tables.  They are rewritten only when a frame is uploaded, by copies on the current stream, i.e. after
    every kernel already queued there; the tensors of an evicted frame are released to PyTorch's allocator, which holds
    their memory until the streams they were used on (``record_stream``) have passed that point."""

    def __init__(self, ffirst: int, flast: int, device: torch.device, capacity: int):
        self.ffirst, self.flast, self.device = ffirst, flast, device
        self.capacity = 0
        self.resident = OrderedDict()           # frame -> (slot, tensors), oldest use first
        self.uploads = self.hits = self.evictions = 0
        self._slot_host = torch.full((flast - ffirst + 1,), -1, dtype=torch.int32)
        self.slot = self._slot_host.to(device)
        self.frames = torch.zeros(0, dtype=torch.uint8, device=device)
        self._free = []
        self.grow(capacity)

    def grow(self, capacity: int):
        if capacity <= self.capacity:
            return
        size = ctypes.sizeof(ops.MhdFrame)
        frames = torch.zeros(capacity * size, dtype=torch.uint8, device=self.device)
        frames[:self.frames.numel()].copy_(self.frames)
        self.frames = frames
        self._free += range(self.capacity, capacity)
        self.capacity = capacity

    def ensure(self, needed, load):
        """Makes the frames ``needed`` resident (``load(frame) -> (data (n_phi, n_theta, n_r, 2) fp32, (phi, theta, r))``
        for the missing ones) and marks them used."""
        if len(needed) > self.capacity:
            raise ValueError(f'this batch needs {len(needed)} MHD frames at once ({needed[0]} ... {needed[-1]}), more than '
                             f'max_frames = {self.capacity}: render fewer distinct times per batch or raise max_frames')
        for f in needed:
            if f in self.resident:
                self.resident.move_to_end(f)
                self.hits += 1
        changed = False
        for f in needed:
            if f in self.resident:
                continue
            if not self._free:
                victim = next(v for v in self.resident if v not in needed)
                slot, _ = self.resident.pop(victim)
                self._slot_host[victim - self.ffirst] = -1
                self._free.append(slot)
                self.evictions += 1
            data, axes = load(f)
            data = torch.from_numpy(data).to(self.device)
            axes = [torch.from_numpy(a).to(self.device) for a in axes]
            desc, keep = ops.mhd_frame(data, axes)
            slot = self._free.pop(0)
            size = ctypes.sizeof(ops.MhdFrame)
            self.frames[slot * size:(slot + 1) * size].copy_(torch.frombuffer(bytearray(bytes(desc)), dtype=torch.uint8))
            self._slot_host[f - self.ffirst] = slot
            self.resident[f] = (slot, keep)
            self.uploads += 1
            changed = True
        if changed:
            self.slot.copy_(self._slot_host)
        stream = torch.cuda.current_stream(self.device)
        for f in needed:
            for t in self.resident[f][1]:
                t.record_stream(stream)


_CACHES = weakref.WeakValueDictionary()     # (directory, reader, device) -> FrameCache, alive while a model holds it


class MHDModel(nn.Module):
    """mhd_model.py:11-142.

    ``reader``: callable ``path -> (r, theta, phi, data)`` with ``data[i_phi, i_theta, i_r]`` (default
    :func:`read_psi_hdf5`, which needs ``h5py``).  ``max_frames``: frames kept on a device, shared with every other
    ``MHDModel`` of the same directory and reader there.  The frames of a batch are uploaded on first use; a batch may
    span at most ``max_frames`` frames (two per distinct time, one at an exact frame).

    Per frame, ``rho`` and ``t`` must share a grid (as PSI's do); the two frames of a pair may have different grids: each
    is interpolated on its own grid, then the two are blended in time.  Grids and data are held in fp32 (the coordinates
    are fp32 in the reference too).  No gradient w.r.t. the cube or the points (a ``NeRF`` has one: DESIGN.md section 8c);
    ``log_absortpion`` and ``volumetric_constant`` receive theirs through the DT integral."""

    time_dependent = True       # functional.dt_pass hands the rays' times to field_on_rays

    def __init__(self, data_path, device=None, reader=None, max_frames=4, channels=None):
        super().__init__()
        device = torch.device("cuda" if torch.cuda.is_available() else "cpu") if device is None else device
        self.device = device
        self.data_path = data_path
        self.density_files = sorted(glob.glob(os.path.join(data_path, 'rho', '*.h5')))
        self.temperature_files = sorted(glob.glob(os.path.join(data_path, 't', '*.h5')))
        if not self.density_files:
            raise FileNotFoundError(f'no MHD density frames: {os.path.join(data_path, "rho", "*.h5")} matches nothing')
        self.ffirst = frame_number(self.density_files[0])
        self.flast = frame_number(self.density_files[-1])
        self.log_absortpion = absorption_scalars(channels)
        self.volumetric_constant = nn.Parameter(torch.tensor(1.0, dtype=torch.float32, requires_grad=True))
        # NeRF_DT adds these to its raw output (model.py:182-183); the simulation is already physical
        self.base_log_density = 0.0
        self.base_log_temperature = 0.0
        self.reader = read_psi_hdf5 if reader is None else reader
        self.max_frames = int(max_frames)
        if self.max_frames < 2:
            raise ValueError('max_frames must be at least 2 (a time between two frames needs both)')
        self._caches = {}

    # ---- frames --------------------------------------------------------------------------------------------------------
    def load_frame(self, frame: int):
        """Host arrays of one frame: ``(data (n_phi, n_theta, n_r, 2) fp32 = (rho, T) with negatives set to 1e-10 (:64),
        (phi, theta, r) fp32)``."""
        grid, first, parts = None, None, []
        for var in VARIABLES:
            path = frame_file(self.data_path, var, frame)
            if not os.path.exists(path):
                raise FileNotFoundError(f'MHD frame {frame}: {path} does not exist')
            r, theta, phi, data = self.reader(path)
            axes = tuple(np.asarray(a, dtype=np.float64).reshape(-1) for a in (phi, theta, r))
            data = np.asarray(data)
            if data.shape != tuple(a.size for a in axes):
                raise ValueError(f'{path}: data of shape {data.shape} on a (phi, theta, r) grid of '
                                 f'{tuple(a.size for a in axes)} nodes')
            if grid is None:
                grid, first = axes, path
            elif not all(np.array_equal(a, b) for a, b in zip(grid, axes)):
                raise ValueError(f'{path}: its grid differs from the grid of {first}; rho and t of one frame must share a grid')
            parts.append(np.where(data < 0, FILL_VALUE, data).astype(np.float32))
        return np.ascontiguousarray(np.stack(parts, -1)), tuple(a.astype(np.float32) for a in grid)

    def frame_cache(self, device) -> FrameCache:
        """The frame cache of this simulation on ``device`` (created on first use)."""
        device = torch.device(device)
        if device.type == 'cuda' and device.index is None:
            device = torch.device('cuda', torch.cuda.current_device())
        key = (os.path.realpath(self.data_path), self.reader, str(device))
        cache = self._caches.get(key)
        if cache is None:
            cache = _CACHES.get(key)
            if cache is None:
                cache = FrameCache(self.ffirst, self.flast, device, self.max_frames)
                _CACHES[key] = cache
            self._caches[key] = cache
        cache.grow(self.max_frames)
        return cache

    def frames_for(self, times: torch.Tensor):
        """Sorted frame numbers the points at ``times`` interpolate between (mhd_model.py:112-124, fp32; one host copy of
        the unique times, like the reference's loop)."""
        t = torch.unique(times.detach()).cpu().to(torch.float32)
        t = t[~torch.isnan(t)]
        f = t * (self.flast - self.ffirst) + self.ffirst
        frames = sorted(set(torch.floor(f).to(torch.int64).tolist()) | set(torch.ceil(f).to(torch.int64).tolist()))
        outside = [v for v in frames if not self.ffirst <= v <= self.flast]
        if outside:
            raise ValueError(f'times outside [0, 1] need frames {outside}; the simulation has {self.ffirst} ... {self.flast}')
        return frames

    def _resident(self, times: torch.Tensor) -> FrameCache:
        cache = self.frame_cache(times.device)
        cache.ensure(self.frames_for(times), self.load_frame)
        return cache

    # ---- field ---------------------------------------------------------------------------------------------------------
    def field_on_rays(self, rays_o, rays_d, z_vals, times):
        """(N, S, 2) = (ln rho, log10 T) at o + d z at every ray's time ``times`` (N, 1) (sunerf_mhd_field)."""
        with torch.no_grad():
            cache = self._resident(times)
            return ops.mhd_field(rays_o, rays_d, z_vals, times, cache.frames, cache.slot, self.ffirst, self.flast)

    def forward(self, query_points):
        """(M, 4) query points (x, y, z, t) -> ``{'rho_T': (M, 2), 'inferences': the same tensor, 'log_abs', 'vol_c'}``
        (mhd_model.py:76-142; ``'inferences'`` added, see the module docstring)."""
        with torch.no_grad():
            pts = query_points.reshape(-1, 4).detach()
            cache = self._resident(pts[:, 3])
            rho_t = ops.mhd_field_points(pts, cache.frames, cache.slot, self.ffirst, self.flast)
        return {'rho_T': rho_t, 'inferences': rho_t, 'log_abs': self.log_absortpion, 'vol_c': self.volumetric_constant}

    def __getstate__(self):
        state = self.__dict__.copy()
        state['_caches'] = {}
        return state
