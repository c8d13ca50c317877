"""Per-pixel DEM inversion of multi-channel images: the classical answer to "what is the thermal
structure behind this pixel", on the device, to set next to a density-temperature model's own line-of-sight DEM
(``sunerf_hip.dem``).  It needs no 3-D model.

``invert_dem`` is the kernel (``sunerf_dem_invert``, csrc/dem_inversion.hip): for every pixel the unique minimiser over
``x >= 0`` of ``1/2 sum_w ((G x - y)_w / sigma_w)^2 + lam/2 sum_k (x_k / p_k)^2``, with ``lam`` given or chosen per pixel by the
discrepancy principle.  ``response_on_nodes`` samples response rows on the DEM's nodes, ``default_errors`` is the one error
model offered.  The result is an emission measure per node like ``dem.dem_integral``'s: ``dem.fold``, ``dem.per_dex`` and
``dem.node_widths`` apply to it unchanged.  Optically thin: no attenuation is inverted.
"""
import math
from typing import Dict, Optional, Sequence

import torch

from . import lib as _l
from ._ffi import _dev, _ptr, _stream
from .dem import MAX_NODES

MAX_CHANNELS = 8
OUTPUTS = ('dem', 'em', 'logt_mean', 'chi2', 'lam', 'status')
# bits of ``status`` (the Newton steps of all solves of the pixel sit in bits 8..)
STATUS_NOT_CONVERGED, STATUS_NO_CHANNEL, STATUS_LAM_MIN, STATUS_LAM_MAX, STATUS_BAD_LAM = 1, 2, 4, 8, 16


def iterations(status):
    """The number of Newton steps in a ``status`` word (all solves of the pixel in discrepancy mode)."""
    return status >> 8


def response_on_nodes(logte_rows, response_rows, nodes):
    """Response rows ``(M, n)`` given on ``logte_rows`` (``(M, n)``, or one grid ``(n,)`` for all rows; strictly increasing)
    sampled on ``nodes`` (K,) -> ``(M, K)`` float64: linear interpolation, 0 outside the table (the DT render's
    ``Interp1D(extrap=0)`` rule).  A node that is a table node gets the table's value, bit for bit."""
    rows = torch.as_tensor(response_rows)
    x = torch.as_tensor(logte_rows).to(device=rows.device, dtype=torch.float64)
    nodes = torch.as_tensor(nodes).to(device=rows.device, dtype=torch.float64)
    if rows.dim() != 2 or nodes.dim() != 1:
        raise ValueError('response_on_nodes: response_rows must be (M, n) and nodes 1-d')
    rows = rows.to(torch.float64)
    if x.dim() == 1:
        x = x[None].expand(rows.shape[0], -1)
    if x.shape != rows.shape or x.shape[1] < 2:
        raise ValueError(f'response_on_nodes: grid {tuple(x.shape)} does not match the rows {tuple(rows.shape)}')
    x = x.contiguous()
    q = nodes[None].expand(rows.shape[0], -1).contiguous()
    i = (torch.searchsorted(x, q, right=True) - 1).clamp(0, x.shape[1] - 2)
    x0, x1 = x.gather(1, i), x.gather(1, i + 1)
    f = (q - x0) / (x1 - x0)
    val = rows.gather(1, i) * (1 - f) + rows.gather(1, i + 1) * f
    inside = (q >= x[:, :1]) & (q <= x[:, -1:])
    return torch.where(inside, val, torch.zeros_like(val))


def default_errors(images, relative: float = 0.05, floor_fraction: float = 1e-3):
    """``relative * |y| + floor_fraction * (the channel's largest finite value)`` for ``images`` (..., M): a calibration-style
    error with a floor.  This is the ONLY error model offered -- no photon statistics, no read noise; pass ``errors`` where
    those matter.  A non-finite ``y`` keeps a non-finite error (the channel is left out for that pixel either way)."""
    y = torch.as_tensor(images)
    flat = y.reshape(-1, y.shape[-1])
    finite = torch.isfinite(flat)
    top = torch.where(finite, flat, torch.full_like(flat, -math.inf)).amax(dim=0).clamp_min(0.0) if flat.shape[0] else flat.new_zeros(y.shape[-1])
    return float(relative) * y.abs() + float(floor_fraction) * top


def flat_prior(images, G):
    """The flat DEM (one value for every node) that reproduces the typical pixel: the median over finite pixels and channels
    of ``y_w / sum_k G[w, k]``, on the device, as (K,) float64; 1 where that median is not positive (a dark frame: every
    solution is 0 whatever the scale)."""
    y = images.reshape(-1, images.shape[-1]).to(torch.float64)
    ratio = y / G.sum(dim=1)
    med = torch.nanmedian(torch.where(torch.isfinite(ratio), ratio, torch.full_like(ratio, math.nan)).reshape(-1)) \
        if ratio.numel() else ratio.new_tensor(math.nan)
    med = torch.where(med > 0, med, torch.ones_like(med))
    return med.expand(G.shape[1]).contiguous()


@torch.no_grad()
def invert_dem(images, G, logt_nodes, errors=None, lam=None, prior=None, chi2_target: Optional[float] = None,
               lam_range=(1e-4, 1e4), n_bisect: int = 20, tol: float = 1e-10, max_iter: int = 64,
               want: Sequence[str] = OUTPUTS, tile_pixels: int = 1 << 20) -> Dict[str, torch.Tensor]:
    """``sunerf_dem_invert`` on ``images`` (..., M) (float32 on the device, 1 <= M <= 8): per pixel

        x* = argmin_{x >= 0} 1/2 sum_w ((G x - y)_w / sigma_w)^2 + lam/2 sum_k (x_k / p_k)^2

    with ``G`` (M, K) >= 0 the channels' response on ``logt_nodes`` (K,) (2 <= K <= 128) times the render's constants
    (:func:`response_on_nodes`), ``errors`` (..., M) the ``sigma`` (default :func:`default_errors`) and ``prior`` (K,) > 0 the
    scale ``p`` per node (default :func:`flat_prior`).  A channel whose value is not finite, or whose error is not finite or
    <= 0, is left out for that pixel (absent channels, saturated pixels).  A ``G`` that is not finite and >= 0 or a ``prior``
    that is not finite and > 0 raises ``ValueError`` (one host read per call).

    ``lam``: a number, or a tensor of the leading shape: that ``lam``.  None: discrepancy mode -- per pixel ``log10 lam`` is
    bisected ``n_bisect`` times on ``lam_range`` until ``chi2 = chi2_target`` (default: the number of channels the pixel
    uses); a pixel that even ``lam_range[0]`` cannot fit gets that end and status bit 4 (the positivity constraint binds), one
    that ``lam_range[1]`` over-fits gets that end and bit 8.  ``tol`` / ``max_iter``: the Newton iteration stops at
    ``max |F| <= tol max |y / sigma|`` or after ``max_iter`` steps (status bit 0).

    Returns the outputs named in ``want``, each with the leading shape of ``images``: ``dem`` (..., K) [emission measure per
    node, like ``dem_integral``'s], ``em``, ``logt_mean`` (NaN where em = 0), ``chi2``, ``lam`` (float32) and ``status``
    (int32: bit 0 not converged, 2 no channel left, 4 / 8 the ends of ``lam_range``, 16 a ``lam`` that is not positive;
    :func:`iterations` of it: the Newton steps) -- and always ``prior`` (K,) float64, which defines what ``lam`` means, and
    ``logt_nodes``.  ``tile_pixels`` pixels per launch; a pixel's result does not depend on the tiling."""
    unknown = [k for k in want if k not in OUTPUTS]
    if unknown:
        raise ValueError(f'invert_dem: unknown outputs {unknown}; choose from {OUTPUTS}')
    if not isinstance(images, torch.Tensor) or images.dim() < 1:
        raise ValueError('images must be a (..., M) tensor')
    if int(tile_pixels) < 1:
        raise ValueError(f'tile_pixels must be positive, not {tile_pixels!r}')
    nodes = torch.as_tensor(logt_nodes)
    if nodes.dim() != 1:
        raise ValueError('logt_nodes must be a 1-d tensor')
    lead, m = tuple(images.shape[:-1]), images.shape[-1]
    y = _dev(images.reshape(-1, m), 'images')
    dev, n = y.device, y.shape[0]
    k = nodes.shape[0]
    if not 1 <= m <= MAX_CHANNELS:
        raise ValueError(f'invert_dem: unsupported number of channels {m} (1 ... {MAX_CHANNELS})')
    if not 2 <= k <= MAX_NODES:
        raise ValueError(f'invert_dem: unsupported number of log T nodes {k} (2 ... {MAX_NODES})')
    nodes = nodes.to(device=dev, dtype=torch.float32).contiguous()
    G = torch.as_tensor(G).to(device=dev, dtype=torch.float64).contiguous()
    if tuple(G.shape) != (m, k):
        raise ValueError(f'G has shape {tuple(G.shape)}, expected {(m, k)}')
    sigma = default_errors(y) if errors is None else _dev(torch.as_tensor(errors).reshape(-1, m), 'errors', (n, m))
    if prior is None:
        prior = flat_prior(y, G)
    else:
        prior = torch.as_tensor(prior).to(device=dev, dtype=torch.float64).contiguous()
        if tuple(prior.shape) != (k,):
            raise ValueError(f'prior has shape {tuple(prior.shape)}, expected {(k,)}')
    # one host read: a NaN in G or the prior would come back as NaN results under a clean status
    if not bool(torch.isfinite(G).all() & (G >= 0).all() & torch.isfinite(prior).all() & (prior > 0).all()):
        raise ValueError('invert_dem: G must be finite and >= 0, prior finite and > 0')
    discrepancy = lam is None
    lam_t, per_pixel = None, False
    if not discrepancy:
        if isinstance(lam, torch.Tensor) and lam.dim() > 0:
            if tuple(lam.shape) != lead:
                raise ValueError(f'lam has shape {tuple(lam.shape)}, expected {lead}')
            lam_t, per_pixel = _dev(lam.to(torch.float32).reshape(-1), 'lam'), True
        else:
            if not (float(lam) > 0 and math.isfinite(float(lam))):
                raise ValueError(f'lam must be positive, not {lam!r}')
            lam_t = torch.tensor([float(lam)], dtype=torch.float32, device=dev)
    lam_min, lam_max = float(lam_range[0]), float(lam_range[1])
    if not (0 < lam_min <= lam_max < math.inf):
        raise ValueError(f'lam_range must be 0 < lam_min <= lam_max, not {tuple(lam_range)!r}')
    target = -1.0 if chi2_target is None else float(chi2_target)
    if chi2_target is not None and not target >= 0:
        raise ValueError(f'chi2_target must not be negative, not {chi2_target!r}')
    f32 = dict(dtype=torch.float32, device=dev)
    out = {'dem': torch.empty(n, k, **f32) if 'dem' in want else None,
           'em': torch.empty(n, **f32) if 'em' in want else None,
           'logt_mean': torch.empty(n, **f32) if 'logt_mean' in want else None,
           'chi2': torch.empty(n, **f32) if 'chi2' in want else None,
           'lam': torch.empty(n, **f32) if 'lam' in want else None,
           'status': torch.empty(n, dtype=torch.int32, device=dev)}

    def part(t, begin, count):
        return None if t is None else _ptr(t[begin:begin + count])

    for begin in range(0, n, int(tile_pixels)):
        count = min(int(tile_pixels), n - begin)
        _l.call(dev, 'sunerf_dem_invert', part(y, begin, count), part(sigma, begin, count), _ptr(G), _ptr(prior), _ptr(nodes),
                part(lam_t, begin, count) if per_pixel else _ptr(lam_t), int(per_pixel), int(discrepancy), target, lam_min,
                lam_max, int(n_bisect), float(tol), int(max_iter), count, m, k, part(out['dem'], begin, count),
                part(out['em'], begin, count), part(out['logt_mean'], begin, count), part(out['chi2'], begin, count),
                part(out['lam'], begin, count), part(out['status'], begin, count), _stream(dev))
    if n == 0:      # the argument checks of the library still apply to an empty batch
        _l.call(dev, 'sunerf_dem_invert', None, None, _ptr(G), _ptr(prior), _ptr(nodes), _ptr(lam_t), int(per_pixel),
                int(discrepancy), target, lam_min, lam_max, int(n_bisect), float(tol), int(max_iter), 0, m, k, None, None, None,
                None, None, None, _stream(dev))
    res = {key: out[key].reshape(lead + tuple(out[key].shape[1:])) for key in OUTPUTS if key in want}
    res['prior'] = prior
    res['logt_nodes'] = nodes
    return res
