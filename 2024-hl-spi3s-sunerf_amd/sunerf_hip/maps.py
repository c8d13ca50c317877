"""Heliographic maps and radial profiles of the corona: the reference's science products after training,
``sunerf/evaluation/stash/`` (topographical_map.py:36-66, topographical_profile.py:33-58, topographical_slice.py:119-140,
eruption_profile.py:76-101), on the device.

Every one of those scripts casts radial columns outward from the solar surface, one per (latitude, longitude), puts a fixed
radial grid on each column, evaluates the fine model and reduces along the column.  Here a column is a ray of the fused render
path: ``rays_o = 0``, ``rays_d = fp32(u(lat, lon))`` (``sunerf_column_rays``), one shared ``z`` row ``r_j / Rs_per_ds``; the
MLP and the emission / DT integrals are the existing kernels', and ``sunerf_column_stats`` adds what the integral does not
produce (emission-weighted height, optically thin column, per-sample profiles).  ``render_columns`` drives it tile by tile,
like ``rays.render_frame``, and shards the map's rows over the ranks of a process group.
"""
import math
from typing import Dict, Optional, Sequence, Tuple

import torch

from . import lib as _l
from ._ffi import _dev, _ptr, _stream

TILE_SCRATCH_BYTES = 1 << 30        # default tile: a tile's per-sample scratch stays under about this


def column_directions(lat: torch.Tensor, lon: torch.Tensor) -> torch.Tensor:
    """Host fp64 restatement of the kernel's column direction: ``u(lat, lon) = (-cos lat sin lon, cos lat cos lon, -sin lat)``
    for per-column angles of equal shape -> (..., 3) float64.  ``u`` is the normalised camera position of
    ``pose_spherical(-lon, lat, d)`` (train/coordinate_transformation.py:36-54): the column lies straight below the observer
    that ``render_observer_image(lat, lon)`` places."""
    lat, lon = torch.as_tensor(lat, dtype=torch.float64), torch.as_tensor(lon, dtype=torch.float64)
    cb = torch.cos(lat)
    return torch.stack([-cb * torch.sin(lon), cb * torch.cos(lon), -torch.sin(lat)], -1)


def grid_columns(lat: torch.Tensor, lon: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
    """Per-column angles (n_lat * n_lon,) of a regular grid, column ``p = row * n_lon + col``: row 0 is the first latitude
    (the south for an ascending axis), column 0 the first longitude -- the layout of the scripts' ``imshow(origin='lower')``."""
    return lat[:, None].expand(-1, lon.shape[0]).reshape(-1), lon[None, :].expand(lat.shape[0], -1).reshape(-1)


def radial_row(r_range: Sequence[float], n_samples: int, Rs_per_ds: float) -> torch.Tensor:
    """The shared ``z`` row (S,) float32: ``r_j / Rs_per_ds`` with ``r_j = linspace(r_in, r_out, S)`` [solar radii], in fp64
    then rounded."""
    r_in, r_out = float(r_range[0]), float(r_range[1])
    return (torch.linspace(r_in, r_out, int(n_samples), dtype=torch.float64) / float(Rs_per_ds)).float()


def check_columns(lat, lon, grid: bool, r_range: Sequence[float], n_samples: int) -> Tuple[int, int]:
    """Argument checks of :func:`render_columns` / :func:`column_rays`, before anything touches the device.  Returns
    ``(rows, columns per row)``: ``(n_lat, n_lon)`` of a grid, ``(n, 1)`` for per-column angles."""
    if int(n_samples) != n_samples or n_samples < 2:
        raise ValueError(f'n_samples must be an integer >= 2, not {n_samples!r}')
    if len(r_range) != 2 or not all(math.isfinite(float(v)) for v in r_range) or not float(r_range[1]) > float(r_range[0]):
        raise ValueError(f'r_range must be (r_in, r_out) with r_out > r_in, not {tuple(r_range)!r}')
    for name, t in (('lat', lat), ('lon', lon)):
        if not isinstance(t, torch.Tensor) or t.dim() != 1:
            raise ValueError(f'{name} must be a 1-d tensor')
    if grid:
        if lat.shape[0] == 0 or lon.shape[0] == 0:
            raise ValueError(f'empty grid: {lat.shape[0]} latitudes x {lon.shape[0]} longitudes')
        return lat.shape[0], lon.shape[0]
    if lat.shape != lon.shape:
        raise ValueError(f'per-column lat / lon must have the same length, got {lat.shape[0]} and {lon.shape[0]}')
    if lat.shape[0] == 0:
        raise ValueError('no columns')
    return lat.shape[0], 1


def column_rays(lat: torch.Tensor, lon: torch.Tensor, grid: bool = True, col_begin: int = 0, n_cols: Optional[int] = None,
                time: Optional[float] = None):
    """Rays of columns ``[col_begin, col_begin + n_cols)`` (``sunerf_column_rays``).

    ``lat`` / ``lon`` [rad] (float64, on the ROCm device): the two axes of a regular grid (``grid=True``; column
    ``p = row * n_lon + col``) or per-column angles of equal length (``grid=False``).  Returns ``rays_o (n,3)`` (zeros),
    ``rays_d (n,3)`` = fp32 of :func:`column_directions` and, if ``time`` is given, ``times (n,1)``."""
    if not isinstance(lat, torch.Tensor) or not isinstance(lon, torch.Tensor) or not lat.is_cuda \
            or lat.dtype != torch.float64 or lon.dtype != torch.float64 or lon.device != lat.device:
        raise _l.SunerfHipError('column_rays: lat / lon must be float64 tensors on one ROCm device (there is no CPU path)')
    rows, per_row = check_columns(lat, lon, grid, (0., 1.), 2)
    total = rows * (lon.shape[0] if grid else 1)
    n_cols = total - col_begin if n_cols is None else n_cols
    if col_begin < 0 or n_cols < 0 or col_begin + n_cols > total:
        raise ValueError(f'columns [{col_begin}, {col_begin + n_cols}) are outside the {total} of the map')
    lat, lon = lat.contiguous(), lon.contiguous()
    dev = lat.device
    rays_o = torch.empty(n_cols, 3, dtype=torch.float32, device=dev)
    rays_d = torch.empty(n_cols, 3, dtype=torch.float32, device=dev)
    times = torch.empty(n_cols, 1, dtype=torch.float32, device=dev) if time is not None else None
    _l.call(dev, 'sunerf_column_rays', _ptr(lat), _ptr(lon), 0 if grid else 1, lon.shape[0] if grid else 1, col_begin, n_cols,
            float(time) if time is not None else 0.0, _ptr(rays_o), _ptr(rays_d), _ptr(times), _stream(dev))
    return (rays_o, rays_d) if time is None else (rays_o, rays_d, times)


def column_stats(raw: torch.Tensor, z_row: torch.Tensor, rays_d: torch.Tensor, height_scale: float = 1.0,
                 profiles: bool = False) -> Dict[str, torch.Tensor]:
    """``sunerf_column_stats`` on a fused pass's ``raw`` (N, S, 2) over columns sharing ``z_row`` (S,):
    ``emission_height`` (N,) = height_scale * sum r e / sum e (r = z |rays_d|), ``emission_column`` (N,) = sum e dr and, with
    ``profiles``, ``emission`` (N, S) = e and ``absorption`` (N, S) = 1 - exp(-relu(raw1) dr); e = exp(raw0), dr the emission
    integral's own interval (model units)."""
    n, s = raw.shape[0], raw.shape[1]
    raw = _dev(raw, 'raw', (n, s, 2)); z_row = _dev(z_row, 'z_row', (s,)); rays_d = _dev(rays_d, 'rays_d', (n, 3))
    dev = raw.device
    f32 = dict(dtype=torch.float32, device=dev)
    out = {'emission_height': torch.empty(n, **f32), 'emission_column': torch.empty(n, **f32)}
    if profiles:
        out['emission'], out['absorption'] = torch.empty(n, s, **f32), torch.empty(n, s, **f32)
    _l.call(dev, 'sunerf_column_stats', _ptr(raw), _ptr(z_row), _ptr(rays_d), n, s, float(height_scale),
            _ptr(out['emission_height']), _ptr(out['emission_column']), _ptr(out.get('emission')), _ptr(out.get('absorption')),
            _stream(dev))
    return out


def _kind(rendering) -> str:
    """'emission' / 'dt' for the fused passes, 'hooks' for a subclass with its own ``_render`` (or a foreign field module)."""
    from sunerf.rendering.density_temperature import DensityTemperatureRadiativeTransfer
    from sunerf.rendering.emission import EmissionRadiativeTransfer
    from sunerf.rendering.thompson import ThompsonScattering
    if isinstance(rendering, ThompsonScattering):
        raise ValueError('render_columns: ThompsonScattering has no heliographic map -- a column from inside the corona has no '
                         'line of sight to an observer, so the scattering geometry of tB / pB is undefined there')
    for cls, kind in ((EmissionRadiativeTransfer, 'emission'), (DensityTemperatureRadiativeTransfer, 'dt')):
        if isinstance(rendering, cls):
            return 'hooks' if rendering._hooks_replaced(cls) else kind
    return 'hooks'


def _bytes_per_column(kind: str, n_samples: int, profiles: bool) -> int:
    """Device bytes a column needs while its tile is rendered: the per-sample fp32 tensors of the pass (raw x 2, weights,
    absorption, regularization, z) plus the profiles."""
    per_sample = 6 + (2 if profiles else 0) + (2 if kind != 'emission' else 0)
    return 4 * n_samples * per_sample + 64


def _tile(rendering, rays_o, rays_d, times, z, wl, kind: str, profiles: bool) -> Dict[str, torch.Tensor]:
    """One tile of columns through the fine model: the fused pass (+ column statistics) or the subclass's own ``_render``."""
    from sunerf.rendering import functional as F
    from sunerf.rendering.base_tracing import ray_query_points
    from sunerf_hip import ops
    model = rendering.fine_model
    scale = float(rendering.Rs_per_ds)
    if kind == 'emission':
        if hasattr(model, 'field_on_rays'):                    # a grid field: its own gather, then the same integral
            out = F._field_emission_pass(model, rays_o, rays_d, times, z, 1.2 / rendering.Rs_per_ds, True, want_raw=True)
        else:
            out = ops.emission_render_fwd(model.packed(), rays_o, rays_d, times, z, 1.2 / rendering.Rs_per_ds,
                                          want_raw=True, want_epilogues=True)
        res = {'image': out['image'], 'height_map': out['height_map'] * scale, 'absorption_map': out['absorption_map']}
        res.update(column_stats(out['raw'], z[0], rays_d, scale, profiles))
        return res
    if kind == 'dt':
        tables = rendering._tables()      # the AIA pair, or the rendering's response set
        out = F.dt_pass(model, tables, rendering.pixel_intensity_factor, rays_o, rays_d, times, z, wl, 1.25 / rendering.Rs_per_ds,
                        want_epilogues=True)
        res = {'image': out['image'], 'height_map': out['height_map'] * scale, 'absorption_map': out['absorption_map']}
        if profiles:
            if hasattr(model, 'field_on_rays'):
                res['inferences'] = F._field_raw(model, rays_o, rays_d, z, times)
            else:
                raw = F.mlp_on_rays(model, rays_o, rays_d, times, z)
                res['inferences'] = raw + raw.new_tensor([model.base_log_density, model.base_log_temperature])
        return res
    extra = () if wl is None else (wl,)
    query = ray_query_points(rays_o, rays_d, times, z)
    out = rendering._render(model, query, rays_d, rays_o, z, *extra)
    distance = query[..., :3].pow(2).sum(-1).pow(0.5)
    return {'image': out['image'], 'height_map': (out['weights'] * distance).sum(-1) * scale,
            'absorption_map': (1 - out['regularizing_quantity']).sum(-1)}


def _process_group(rank: Optional[int], world: Optional[int]) -> Tuple[int, int]:
    import torch.distributed as dist
    active = dist.is_available() and dist.is_initialized()
    rank = (dist.get_rank() if active else 0) if rank is None else int(rank)
    world = (dist.get_world_size() if active else 1) if world is None else int(world)
    if world < 1 or not 0 <= rank < world:
        raise ValueError(f'rank {rank} is outside a world of {world}')
    if world > 1 and not active:
        raise ValueError(f'world={world}: the slabs are gathered over the default process group, which is not initialised')
    return rank, world


def _gather_rows(part: torch.Tensor, counts: Sequence[int]) -> torch.Tensor:
    """All-gather of every rank's slab (first dimension: its columns, ``counts[rank]`` of them) into the whole map on every
    rank.  Slabs are padded to the largest for the collective; under gloo it runs on CPU copies."""
    import torch.distributed as dist
    on_device = dist.get_backend() == 'nccl'
    most = max(counts)
    buf = part.new_zeros((most,) + tuple(part.shape[1:]))
    buf[:part.shape[0]] = part
    if not on_device:
        buf = buf.cpu()
    slabs = [torch.empty_like(buf) for _ in counts]
    dist.all_gather(slabs, buf)
    return torch.cat([s[:c] for s, c in zip(slabs, counts)]).to(part.device)


@torch.no_grad()
def render_columns(rendering, lat, lon, time: float, r_range: Sequence[float] = (1.0, 1.3), n_samples: int = 512,
                   wavelengths: Optional[torch.Tensor] = None, tile_rays: Optional[int] = None,
                   keys: Optional[Sequence[str]] = None, profiles: bool = False, grid: bool = True,
                   rank: Optional[int] = None, world: Optional[int] = None) -> Dict[str, torch.Tensor]:
    """Radial columns through the fine model of ``rendering``, assembled on the device.

    ``lat`` / ``lon`` [rad]: the axes of a regular grid (``grid=True``: outputs shaped ``(n_lat, n_lon, ...)``, row 0 the first
    latitude) or per-column angles of equal length (``grid=False``: outputs ``(n, ...)``), in the convention of
    ``render_observer_image``.  ``time``: the normalised time of every column.  Each column samples ``n_samples`` radii
    ``linspace(*r_range)`` [solar radii], ``z = r / Rs_per_ds``.

    Emission renderings return ``image`` (.., 1) (emission integral with absorption, topographical_map.py:55-60),
    ``height_map`` (sum w |p|) and ``absorption_map`` of the fused pass, ``emission_height`` (sum r e / sum e with
    e = exp(raw0), topographical_profile.py:57) and ``emission_column`` (sum e dr, the optically thin column,
    topographical_slice.py:131-135 with dr), and with ``profiles`` the per-sample ``emission`` e and ``absorption``
    1 - exp(-relu(raw1) dr) (.., S) (eruption_profile.py:89-94).  Density-temperature renderings (``NeRF_DT``, ``SimpleStar``,
    ``MHDModel``; ``wavelengths`` (W,) required) return ``image`` (.., W), ``height_map`` and ``absorption_map``, and with
    ``profiles`` the per-sample ``inferences`` (.., S, 2) (base offsets included).  A subclass with its own ``_render`` goes
    through it and returns the three maps.  ``ThompsonScattering`` is refused.  Heights are in solar radii (x ``Rs_per_ds``);
    ``dr`` and the integrals are in the model's length unit, like the fused pass's.

    ``tile_rays``: columns per tile (default: a tile's scratch stays under about 1 GiB).  ``keys``: outputs to keep.
    ``rank`` / ``world`` (default: the initialised process group, else a single process): each rank renders its
    ``shard_range`` of the rows and, with ``world > 1``, every rank ends with the whole map."""
    from .dist import shard_range
    kind = _kind(rendering)
    dev = next(rendering.fine_model.parameters(), None)
    dev = dev.device if dev is not None else torch.device('cuda')
    lat = lat if isinstance(lat, torch.Tensor) else torch.as_tensor(lat, dtype=torch.float64)
    lon = lon if isinstance(lon, torch.Tensor) else torch.as_tensor(lon, dtype=torch.float64)
    rows, per_row = check_columns(lat, lon, grid, r_range, n_samples)
    if kind == 'dt' and wavelengths is None:
        raise ValueError('render_columns: a density-temperature rendering needs the wavelengths (W,)')
    if kind == 'emission' and wavelengths is not None:
        raise ValueError('render_columns: an emission rendering takes no wavelengths')
    if tile_rays is not None and int(tile_rays) < 1:
        raise ValueError(f'tile_rays must be positive, not {tile_rays!r}')
    rank, world = _process_group(rank, world)
    if rows < world:
        raise ValueError(f'render_columns: {rows} rows cannot be shared by {world} ranks (a rank would render nothing)')
    if dev.type != 'cuda':
        raise _l.SunerfHipError('render_columns: the rendering module is on the CPU; the map runs on a ROCm device only')
    lat = lat.to(device=dev, dtype=torch.float64).contiguous()
    lon = lon.to(device=dev, dtype=torch.float64).contiguous()
    row_begin, row_end = shard_range(rows, rank, world)
    c_begin, c_end = row_begin * per_row, row_end * per_row
    n_local = c_end - c_begin
    tile = int(tile_rays) if tile_rays is not None else max(64, TILE_SCRATCH_BYTES // _bytes_per_column(kind, n_samples, profiles))
    z_row = radial_row(r_range, n_samples, rendering.Rs_per_ds).to(dev)
    wl_all = None if wavelengths is None else torch.as_tensor(wavelengths).to(device=dev, dtype=torch.float32).reshape(-1)
    part: Dict[str, torch.Tensor] = {}
    z_tile = wl_tile = None
    for begin in range(c_begin, c_end, tile):
        n = min(tile, c_end - begin)
        rays_o, rays_d, times = column_rays(lat, lon, grid, begin, n, time=time)
        if z_tile is None or z_tile.shape[0] != n:          # built once per tile size
            z_tile = z_row[None, :].expand(n, -1).contiguous()
            wl_tile = None if wl_all is None else wl_all[None, :].expand(n, -1).contiguous()
        out = _tile(rendering, rays_o, rays_d, times, z_tile, wl_tile, kind, profiles)
        for k, v in out.items():
            if keys is not None and k not in keys:
                continue
            if k not in part:
                part[k] = torch.empty((n_local,) + tuple(v.shape[1:]), dtype=v.dtype, device=v.device)
            part[k][begin - c_begin:begin - c_begin + n] = v
    if world > 1:
        counts = [(e - b) * per_row for b, e in (shard_range(rows, r, world) for r in range(world))]
        part = {k: _gather_rows(v, counts) for k, v in sorted(part.items())}
    shape = (rows, lon.shape[0]) if grid else (rows,)
    return {k: v.view(*shape, *v.shape[1:]) for k, v in part.items()}
