"""Line-of-sight differential emission measure of a density-temperature model: DEM(log T) per pixel,
total emission measure, emission-measure-weighted log T and column density -- what a DT reconstruction is compared with a DEM
inversion by -- on the device.

``dem_integral`` is the kernel (``sunerf_dem_integral``, csrc/dem.hip) on a given ``raw`` (N, S, 2); ``render_dem_frame`` /
``render_dem_columns`` drive ``DensityTemperatureRadiativeTransfer.render_dem`` tile by tile over an observer's frame or over
the radial columns of a heliographic map, like ``rays.render_frame`` and ``maps.render_columns``; ``per_dex`` and ``fold`` are
pure post-processing.  Everything integrates in the model's length unit, like the render itself; ``length_scale`` converts.
"""
import math
from typing import Dict, Optional, Sequence

import torch

from . import lib as _l
from ._ffi import _dev, _ptr, _stream

MAX_NODES = 128
OUTPUTS = ('dem', 'em', 'logt_mean', 'column')


def dem_integral(raw, z_vals, logt_nodes, base=(0., 0.), log_abs=None, rays_o=None, rays_d=None, r_range=(0., math.inf),
                 want: Sequence[str] = OUTPUTS, length_scale: float = 1.0) -> Dict[str, torch.Tensor]:
    """``sunerf_dem_integral`` on the raw field output ``raw`` (N, S, 2) at the samples ``z_vals`` (N, S) of N rays.

    With ``rho = exp(relu(raw0 + base[0]))``, ``logT = relu(raw1 + base[1])`` and the quadrature points ``j = 0..S-2`` of the DT
    render (trapezoid weights ``q_j`` on ``z_0..z_{S-2}``), ``v_j = q_j t_j m_j rho_j^2``:

    * ``dem`` (N, K): ``v_j`` deposited with linear weights onto the two nodes of ``logt_nodes`` (K,) (strictly increasing,
      2 <= K <= 128, float32 on the device) around ``logT_j``; a sample outside ``[nodes[0], nodes[-1]]`` deposits nothing;
    * ``em`` (N,) = sum v_j (every sample); ``logt_mean`` (N,) = sum v_j logT_j / em (NaN where em = 0);
    * ``column`` (N,) = sum q_j m_j rho_j (not attenuated).

    ``log_abs``: None (optically thin), a number, or a one-element device tensor: the absorption scalar of one channel,
    ``t_j = exp(-A_{j+1})`` with ``A = cumulative_trapezoid(rho relu(log_abs), z)`` as in the render.  ``r_range = (r_in,
    r_out)``: only samples with ``r_in <= |rays_o + rays_d z| <= r_out`` count (``m_j``; then ``rays_o`` / ``rays_d`` (N, 3)
    are needed); the default is no mask.  ``want``: the outputs to return.  ``length_scale`` multiplies ``dem``, ``em`` and
    ``column`` (e.g. the centimetres of the model's length unit); the default keeps the render's model units."""
    unknown = [k for k in want if k not in OUTPUTS]
    if unknown:
        raise ValueError(f'dem_integral: unknown outputs {unknown}; choose from {OUTPUTS}')
    if not isinstance(z_vals, torch.Tensor) or z_vals.dim() != 2:
        raise ValueError('z_vals must be a (N, S) tensor')
    if not isinstance(logt_nodes, torch.Tensor) or logt_nodes.dim() != 1:
        raise ValueError('logt_nodes must be a 1-d tensor')
    n, s = z_vals.shape
    k = logt_nodes.shape[0]
    raw = _dev(raw, 'raw', (n, s, 2)); z_vals = _dev(z_vals, 'z_vals', (n, s))
    logt_nodes = _dev(logt_nodes, 'logt_nodes', (k,))
    if s < 2:
        raise ValueError(f'dem_integral needs at least 2 samples per ray, got {s}')
    if not 2 <= k <= MAX_NODES:
        raise ValueError(f'dem_integral: unsupported number of log T nodes {k} (2 ... {MAX_NODES})')
    r_in, r_out = float(r_range[0]), float(r_range[1])
    if math.isnan(r_in) or math.isnan(r_out):
        raise ValueError(f'r_range must not hold NaN, got {tuple(r_range)!r}')
    masked = not (r_in <= 0. and r_out == math.inf)
    if masked and (rays_o is None or rays_d is None):
        raise ValueError('dem_integral: a radius mask (r_range) needs rays_o and rays_d')
    if rays_o is not None:
        rays_o = _dev(rays_o, 'rays_o', (n, 3))
    if rays_d is not None:
        rays_d = _dev(rays_d, 'rays_d', (n, 3))
    dev = z_vals.device
    if log_abs is not None:
        if not isinstance(log_abs, torch.Tensor):
            log_abs = torch.tensor([float(log_abs)], dtype=torch.float32, device=dev)
        log_abs = _dev(log_abs.detach().reshape(-1), 'log_abs', (1,))
    f32 = dict(dtype=torch.float32, device=dev)
    out = {'dem': torch.empty(n, k, **f32) if 'dem' in want else None, 'em': torch.empty(n, **f32),
           'logt_mean': torch.empty(n, **f32) if 'logt_mean' in want else None,
           'column': torch.empty(n, **f32) if 'column' in want else None}
    _l.call(dev, 'sunerf_dem_integral', _ptr(raw), _ptr(z_vals), _ptr(rays_o), _ptr(rays_d), _ptr(logt_nodes), k, float(base[0]),
            float(base[1]), _ptr(log_abs), r_in, r_out, n, s, _ptr(out['dem']), _ptr(out['em']), _ptr(out['logt_mean']),
            _ptr(out['column']), _stream(dev))
    if float(length_scale) != 1.0:
        for key in ('dem', 'em', 'column'):
            if out[key] is not None:
                out[key] *= float(length_scale)
    return {key: out[key] for key in OUTPUTS if key in want}


def node_widths(nodes):
    """Width of log T that each node of ``nodes`` (K,) stands for: ``(x_{k+1} - x_{k-1}) / 2``, half a cell at the two ends
    (the integral of the node's hat function); they add up to ``x_{K-1} - x_0``."""
    nodes = torch.as_tensor(nodes)
    if nodes.dim() != 1 or nodes.shape[0] < 2:
        raise ValueError('nodes must be a 1-d tensor of at least two log T values')
    d = nodes[1:] - nodes[:-1]
    w = torch.zeros_like(nodes)
    w[:-1] += d / 2
    w[1:] += d / 2
    return w


def per_dex(dem, nodes):
    """DEM per unit of log T: ``dem`` (..., K) (emission measure per node, what the kernel returns) divided by
    :func:`node_widths`."""
    dem = torch.as_tensor(dem)
    return dem / node_widths(nodes).to(device=dem.device, dtype=dem.dtype)


def fold(dem, response_rows):
    """``dem @ R``: ``dem`` (..., K) folded with response rows ``(W, K)`` (or one row ``(K,)``) sampled on the DEM's own nodes
    -> (..., W) (or (...)).  On the response table's grid, times ``volumetric_constant * pixel_intensity_factor``, this is the
    DT render's image."""
    dem, rows = torch.as_tensor(dem), torch.as_tensor(response_rows)
    rows = rows.to(device=dem.device, dtype=dem.dtype)
    if rows.shape[-1] != dem.shape[-1]:
        raise ValueError(f'fold: the response has {rows.shape[-1]} nodes, the DEM {dem.shape[-1]}')
    return dem @ rows.T if rows.dim() == 2 else dem @ rows


def _dt_rendering(rendering, what: str):
    from sunerf.rendering.density_temperature import DensityTemperatureRadiativeTransfer
    if not isinstance(rendering, DensityTemperatureRadiativeTransfer) or not callable(getattr(rendering, 'render_dem', None)):
        raise TypeError(f'{what}: a DEM needs a density-temperature rendering (DensityTemperatureRadiativeTransfer); '
                        f'{type(rendering).__name__} has no temperature')
    return rendering


def _scaled(out: Dict[str, torch.Tensor], length_scale: float) -> Dict[str, torch.Tensor]:
    if float(length_scale) != 1.0:
        for key in ('dem', 'em', 'column'):
            out[key] = out[key] * float(length_scale)
    return out


@torch.no_grad()
def render_dem_frame(rendering, tx: torch.Tensor, ty: torch.Tensor, c2w: torch.Tensor, time: float, logt_nodes=None,
                     attenuation_wavelength=None, r_range=(0., math.inf), tile_rays: int = 1 << 18,
                     length_scale: float = 1.0) -> Dict[str, torch.Tensor]:
    """``rendering.render_dem`` over all pixels of an observer's frame (``tx`` / ``ty`` / ``c2w`` as ``rays.render_frame``),
    tile by tile, assembled on the device: ``dem`` (H, W, K), ``em`` / ``logt_mean`` / ``column`` (H, W) and ``logt_nodes``
    (K,)."""
    from .rays import grid_rays
    rendering = _dt_rendering(rendering, 'render_dem_frame')
    if int(tile_rays) < 1:
        raise ValueError(f'tile_rays must be positive, not {tile_rays!r}')
    if tx.dim() == 2:
        height, width = tx.shape
    else:
        width, height = tx.shape[0], ty.shape[0]
    total = width * height
    frame: Dict[str, torch.Tensor] = {}
    nodes = None
    for begin in range(0, total, int(tile_rays)):
        n = min(int(tile_rays), total - begin)
        rays_o, rays_d, times = grid_rays(tx, ty, c2w, begin, n, time=time)
        out = rendering.render_dem(rays_o, rays_d, times, logt_nodes, attenuation_wavelength, r_range)
        nodes = out['logt_nodes']
        for k in OUTPUTS:
            v = out[k]
            if k not in frame:
                frame[k] = torch.empty((total,) + tuple(v.shape[1:]), dtype=v.dtype, device=v.device)
            frame[k][begin:begin + n] = v
    res = _scaled({k: v.view(height, width, *v.shape[1:]) for k, v in frame.items()}, length_scale)
    res['logt_nodes'] = nodes
    return res


@torch.no_grad()
def render_dem_columns(rendering, lat, lon, time: float, r_range: Sequence[float] = (1.0, 1.3), n_samples: int = 512,
                       logt_nodes=None, attenuation_wavelength=None, tile_rays: Optional[int] = None, grid: bool = True,
                       length_scale: float = 1.0) -> Dict[str, torch.Tensor]:
    """The DEM of radial columns through the fine model (the columns of ``maps.render_columns``: ``rays_o = 0``, one shared
    row of ``n_samples`` radii ``linspace(*r_range)`` [solar radii]): ``dem`` (n_lat, n_lon, K), ``em`` / ``logt_mean`` /
    ``column`` (n_lat, n_lon) for the axes of a grid, ``(n, ...)`` for per-column angles (``grid=False``), and ``logt_nodes``.
    The column's ``r_range`` also is the kernel's radius mask."""
    from sunerf.rendering import functional as F
    from . import maps
    rendering = _dt_rendering(rendering, 'render_dem_columns')
    model = rendering.fine_model
    dev = next(model.parameters(), None)
    dev = dev.device if dev is not None else torch.device('cuda')
    lat = lat if isinstance(lat, torch.Tensor) else torch.as_tensor(lat, dtype=torch.float64)
    lon = lon if isinstance(lon, torch.Tensor) else torch.as_tensor(lon, dtype=torch.float64)
    rows, per_row = maps.check_columns(lat, lon, grid, r_range, n_samples)
    if tile_rays is not None and int(tile_rays) < 1:
        raise ValueError(f'tile_rays must be positive, not {tile_rays!r}')
    if dev.type != 'cuda':
        raise _l.SunerfHipError('render_dem_columns: the rendering module is on the CPU; the map runs on a ROCm device only')
    lat = lat.to(device=dev, dtype=torch.float64).contiguous()
    lon = lon.to(device=dev, dtype=torch.float64).contiguous()
    total = rows * per_row
    tile = int(tile_rays) if tile_rays is not None else max(64, maps.TILE_SCRATCH_BYTES // maps._bytes_per_column('dt', n_samples, False))
    z_row = maps.radial_row(r_range, n_samples, rendering.Rs_per_ds).to(dev)
    nodes = rendering.dem_nodes(logt_nodes)
    log_abs = rendering.attenuation_scalar(attenuation_wavelength)
    scale = float(rendering.Rs_per_ds)
    # the mask in model units, 1e-6 wider than the column: its two end samples lie ON the bounds, where the rounding of the fp32
    # unit direction would otherwise decide
    mask = (float(r_range[0]) / scale * (1 - 1e-6), float(r_range[1]) / scale * (1 + 1e-6))
    part: Dict[str, torch.Tensor] = {}
    z_tile = None
    for begin in range(0, total, tile):
        n = min(tile, total - begin)
        rays_o, rays_d, times = maps.column_rays(lat, lon, grid, begin, n, time=time)
        if z_tile is None or z_tile.shape[0] != n:
            z_tile = z_row[None, :].expand(n, -1).contiguous()
        raw = rendering.fine_raw(rays_o, rays_d, times, z_tile)
        out = dem_integral(raw, z_tile, nodes, (model.base_log_density, model.base_log_temperature), log_abs, rays_o, rays_d,
                           mask)
        for k, v in out.items():
            if k not in part:
                part[k] = torch.empty((total,) + tuple(v.shape[1:]), dtype=v.dtype, device=v.device)
            part[k][begin:begin + n] = v
    shape = (rows, lon.shape[0]) if grid else (rows,)
    res = _scaled({k: v.view(*shape, *v.shape[1:]) for k, v in part.items()}, length_scale)
    res['logt_nodes'] = nodes
    return res
