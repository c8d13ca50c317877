"""Training through the instrument (include/sunerf_hip_patch.h): batches of detector-pixel PATCHES instead of
shuffled rays.  A patch of ``P x P`` detector pixels is handed out as the rays of the ``hw x ww`` sub-pixels its pixels read
through the instrument -- ``hw = (P - 1) bin + kh``, ``kh x kw`` the shape of ``Instrument.effective_kernel()``, the PSF halo
included -- with the ``P x P`` observed pixels as the target.  The training step renders the window, observes it
(``Instrument.expected_windows``, differentiable) and compares detector pixels: the model is fitted to ``instrument(render)``,
so what it learns is the scene in front of the telescope (forward-model deconvolution).

Past the frame's edge the window holds real rays: the sub-pixel axes of a view are EXTENDED by the halo
(:func:`extended_axis`), and the patch path has no boundary rule.  One launch (``sunerf_patch_records``) writes a whole batch.
There is no CPU path for the records; the lattice, the order and the axes are plain host code."""
from typing import Dict, Iterator, List, Sequence, Tuple

import numpy as np
import torch

from . import lib as _l
from ._ffi import _ptr, _stream
from .instrument import Instrument
from .observations import MAX_CHANNELS, View

TARGET_RAYS = 8192          # rays per batch that the default patches_per_batch comes nearest to
UNIFORM_TOLERANCE = 1e-6    # of the pixel size: how far an axis may stray from uniform

# struct SunerfPatchViewDesc (include/sunerf_hip_patch.h: SUNERF_PATCH_VIEW_DESC_BYTES)
PATCH_VIEW_DESC = np.dtype({
    'names': ['tx', 'ty', 'image', 'height', 'width', 'c2w', 'time', 'n_planes', 'plane', 'wavelength'],
    'formats': ['<u8', '<u8', '<u8', '<i4', '<i4', ('<f4', 12), '<f4', '<i4', ('<i4', MAX_CHANNELS), ('<f4', MAX_CHANNELS)],
    'offsets': [0, 8, 16, 24, 28, 32, 80, 84, 88, 88 + 4 * MAX_CHANNELS],
    'itemsize': 88 + 8 * MAX_CHANNELS})


def extended_axis(axis, bin_factor: int, k_eff: int, anchor: int) -> np.ndarray:
    """The sub-pixel axis of a detector axis ``axis`` (n uniform pixel-centre angles, n >= 2), extended by the halo of a kernel
    of ``k_eff`` taps with anchor ``anchor``: ``(n - 1) bin + k_eff`` angles, entry ``m`` that of sub-pixel ``m - anchor`` of the
    frame, ``t0 + (c + (s + 0.5) / bin - 0.5) delta`` with ``m - anchor = c bin + s``, ``0 <= s < bin`` (``c`` may lie outside
    the frame) and ``delta = (axis[-1] - axis[0]) / (n - 1)``, in fp64 and rounded to fp32 once (returned as float64)."""
    axis = np.asarray(axis.detach().cpu().numpy() if isinstance(axis, torch.Tensor) else axis, dtype=np.float64)
    if axis.ndim != 1:
        raise ValueError('patches need a view with 1-d pixel axes (per-pixel angles are not supported)')
    n = axis.shape[0]
    if n < 2:
        raise ValueError('an axis of one pixel has no pixel size')
    t0 = axis[0]
    delta = (axis[-1] - axis[0]) / (n - 1)
    if delta == 0 or np.abs(axis - (t0 + np.arange(n) * delta)).max() > UNIFORM_TOLERANCE * abs(delta):
        raise ValueError('patches need a uniform pixel axis')
    b = int(bin_factor)
    q = np.arange((n - 1) * b + int(k_eff), dtype=np.int64) - int(anchor)
    c = np.floor_divide(q, b)
    s = q - c * b
    angle = t0 + (c.astype(np.float64) + (s.astype(np.float64) + 0.5) / b - 0.5) * delta
    return angle.astype(np.float32).astype(np.float64)


def lattice(n: int, patch: int) -> List[int]:
    """First pixels of the patches of one axis of ``n`` pixels: 0, P, 2 P, ... and the last one shifted inward so that it ends
    at the edge."""
    n, patch = int(n), int(patch)
    if patch < 1:
        raise ValueError(f'patch must be >= 1, got {patch}')
    if n < patch:
        raise ValueError(f'a view of {n} pixels is smaller than the patch of {patch}')
    starts = list(range(0, n - patch + 1, patch))
    if starts[-1] + patch < n:
        starts.append(n - patch)
    return starts


def epoch_order(n_patches: int, seed: int, epoch: int, rank: int = 0, world: int = 1) -> np.ndarray:
    """Rank ``rank``'s patches of one epoch: every ``world``-th entry of one permutation that all ranks compute alike."""
    return np.random.default_rng([int(seed), int(epoch)]).permutation(int(n_patches))[int(rank)::int(world)]


def patch_view_descriptors(views: Sequence[View], axes: Sequence[Tuple[torch.Tensor, torch.Tensor]]) -> np.ndarray:
    rows = np.zeros(len(views), dtype=PATCH_VIEW_DESC)
    for row, v, (tx, ty) in zip(rows, views, axes):
        row['tx'], row['ty'], row['image'] = tx.data_ptr(), ty.data_ptr(), v.image.data_ptr()
        row['height'], row['width'] = v.height, v.width
        row['c2w'] = np.asarray(v.c2w[:3, :4].reshape(-1).tolist(), dtype=np.float32)
        row['time'] = np.float32(v.time)
        row['n_planes'] = v.image.shape[0]
        row['plane'][:] = -1
        row['plane'][:v.plane.size] = v.plane
        row['wavelength'][:v.wavelength.size] = v.wavelength
    return rows


def records(desc: torch.Tensor, n_views: int, triples: torch.Tensor, n_channels: int, patch: int, bin_factor: int, kh: int, kw: int,
            with_wavelength: bool) -> Dict[str, torch.Tensor]:
    """``sunerf_patch_records`` on a device table ``desc`` and device int32 triples [n, 3] = (view, R0, C0)."""
    dev = desc.device
    if dev.type != 'cuda':
        raise _l.SunerfHipError('patch records are written by sunerf_patch_records on a ROCm device (there is no CPU path)')
    if triples.dtype != torch.int32 or triples.dim() != 2 or triples.shape[1] != 3 or triples.device != dev:
        raise ValueError('triples must be int32 [n, 3] on the table\'s device')
    triples = triples.contiguous()
    n = triples.shape[0]
    hw, ww = (patch - 1) * bin_factor + kh, (patch - 1) * bin_factor + kw
    out = {'rays': torch.empty(n, hw, ww, 2, 3, dtype=torch.float32, device=dev),
           'time': torch.empty(n * hw * ww, 1, dtype=torch.float32, device=dev),
           'target_image': torch.empty(n, n_channels, patch, patch, dtype=torch.float32, device=dev)}
    if with_wavelength:
        out['wavelength'] = torch.empty(n * hw * ww, n_channels, dtype=torch.float32, device=dev)
    _l.call(dev, 'sunerf_patch_records', _ptr(desc), n_views, _ptr(triples), n, n_channels, patch, bin_factor, kh, kw,
            _ptr(out['rays']), _ptr(out['time']), _ptr(out['target_image']), _ptr(out.get('wavelength')), _stream(dev))
    return out


class PatchPool:
    """The patches of the training views of an ``ObservationSet`` as seen through ``instrument``; iterating yields one epoch of
    batches ``{'rays', 'time', 'target_image', ['wavelength'], 'patch': spec}`` (what ``training_batches`` wraps into
    ``{'tracing': ...}`` and the modules' ``training_step`` reads).  ``dropped`` counts the patches left out because their target
    holds a non-finite value."""

    def __init__(self, views: Sequence[View], instrument: Instrument, device, with_wavelength: bool, patch: int = 16,
                 patches_per_batch=None, rank: int = 0, world: int = 1, seed: int = 0):
        if not views:
            raise ValueError('no views to cut patches from')
        if torch.device(device).type != 'cuda':
            raise _l.SunerfHipError('patch records are written by sunerf_patch_records on a ROCm device (there is no CPU path)')
        if not 0 <= int(rank) < int(world):
            raise ValueError(f'rank {rank} of {world}')
        self.instrument, self.patch, self.rank, self.world, self.seed = instrument, int(patch), int(rank), int(world), int(seed)
        self.with_wavelength = bool(with_wavelength)
        K, (ay, ax) = instrument.effective_kernel()
        self.kh, self.kw = int(K.shape[1]), int(K.shape[2])
        self.n_channels = int(views[0].plane.size)
        if K.shape[0] not in (1, self.n_channels):
            raise ValueError(f'the psf has {K.shape[0]} channels, the views {self.n_channels}')
        self.hw, self.ww = instrument.window_shape(self.patch)
        self.views, self.axes, triples, self.dropped = list(views), [], [], 0
        for k, v in enumerate(self.views):
            if v.per_pixel:
                raise ValueError(f'{v.name}: patches need a view with 1-d pixel axes (per-pixel angles are not supported)')
            if v.downscale != 1:
                raise ValueError(f'{v.name}: downscale {v.downscale} != 1; use the instrument\'s bin for the averaging')
            tx = torch.from_numpy(extended_axis(v.tx, instrument.bin, self.kw, ax)).to(device)
            ty = torch.from_numpy(extended_axis(v.ty, instrument.bin, self.kh, ay)).to(device)
            self.axes.append((tx, ty))
            finite = torch.isfinite(v.image).all(0)          # torch ops (plumbing): a patch is kept when its whole target is finite
            for r0 in lattice(v.height, self.patch):
                for c0 in lattice(v.width, self.patch):
                    if bool(finite[r0:r0 + self.patch, c0:c0 + self.patch].all()):
                        triples.append((k, r0, c0))
                    else:
                        self.dropped += 1
        if not triples:
            raise ValueError('no patch with a finite target in the views')
        self.triples = np.asarray(triples, dtype=np.int32)
        self.n_patches = len(triples)
        self.device = torch.device(device)
        self.desc = torch.from_numpy(patch_view_descriptors(self.views, self.axes).view(np.uint8).reshape(-1).copy()).to(device)
        self._triples_dev = torch.from_numpy(self.triples).to(device)
        if patches_per_batch is None:
            patches_per_batch = max(1, int(round(TARGET_RAYS / (self.hw * self.ww))))
        self.patches_per_batch = int(patches_per_batch)
        if self.patches_per_batch < 1:
            raise ValueError('patches_per_batch must be >= 1')
        self.epoch = 0

    @property
    def rays_per_batch(self) -> int:
        return self.patches_per_batch * self.hw * self.ww

    @property
    def halo_overhead(self) -> float:
        """Rays rendered per sub-pixel a patch owns: ``hw ww / (P bin)^2``."""
        return self.hw * self.ww / float((self.patch * self.instrument.bin) ** 2)

    def order(self, epoch=None) -> np.ndarray:
        return epoch_order(self.n_patches, self.seed, self.epoch if epoch is None else epoch, self.rank, self.world)

    def __len__(self) -> int:
        """Batches per epoch of this rank."""
        return -(-len(self.order(0)) // self.patches_per_batch)

    def batch(self, indices) -> Dict[str, torch.Tensor]:
        """The batch of patches ``indices`` (numbers into ``triples``): one launch."""
        index = torch.as_tensor(np.asarray(indices, dtype=np.int64), device=self.device)
        triples = self._triples_dev.index_select(0, index)
        out = records(self.desc, len(self.views), triples, self.n_channels, self.patch, self.instrument.bin, self.kh, self.kw,
                      self.with_wavelength)
        out['patch'] = {'n': int(triples.shape[0]), 'C': self.n_channels, 'P': self.patch, 'hw': self.hw, 'ww': self.ww,
                        'instrument': self.instrument}
        return out

    def __iter__(self) -> Iterator[Dict[str, torch.Tensor]]:
        order = self.order()
        self.epoch += 1
        for b in range(0, len(order), self.patches_per_batch):
            yield self.batch(order[b:b + self.patches_per_batch])
