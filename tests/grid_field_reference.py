"""float64 restatement of the voxel-grid field in plain torch: coordinates, ``searchsorted`` cells,
gather; autograd through the gather is the adjoint.  The checker of csrc/grid_field.hip -- it shares no code with it or with
``sunerf_hip.grid_field`` (a grid of ``sunerf_hip.volume`` is read as data: axes, origin, basis).

Points are taken in fp32, as the kernel takes them, and promoted exactly; everything after that is float64.
"""
import math

import torch

TWO_PI = 2.0 * math.pi
LON_MODES = ('patch', 'closed', 'open')


def ray_points(rays_o, rays_d, z_vals):
    """(N, S, 3) fp32 sample points ``o + d z``: one fp32 multiply, one fp32 add, as the kernel forms them."""
    o, d, z = rays_o.float().cpu(), rays_d.float().cpu(), z_vals.float().cpu()
    return o[:, None, :] + d[:, None, :] * z[..., None]


def grid_coordinates(grid, points, Rs_per_ds=1.0, lon_mode='patch'):
    """(M, 3) float64 grid coordinates ``u`` of fp32 ``points (M, >= 3)``: the inverse of the grid's node map.

    Affine: ``u = inverse(basis^T) (X - origin)``.  Spherical (nodes ``X = r (-cos b sin l, cos b cos l, -sin b)``):
    ``(lat, lon, r) = (asin(-Z / r), atan2(-X, Y), r)`` with the longitude reduced into ``[lon[0], lon[0] + 2 pi)``."""
    X = points[:, :3].double() * float(Rs_per_ds)
    if grid.kind == 'affine':
        d = X - grid.origin
        m = torch.linalg.inv(grid.basis.T.contiguous())
        return torch.stack([(m[k, 0] * d[:, 0] + m[k, 1] * d[:, 1]) + m[k, 2] * d[:, 2] for k in range(3)], -1)
    r = torch.sqrt((X[:, 0] * X[:, 0] + X[:, 1] * X[:, 1]) + X[:, 2] * X[:, 2])
    s = -X[:, 2] / r
    s = torch.where(s > 1, torch.ones_like(s), torch.where(s < -1, -torch.ones_like(s), s))     # (NaN stays NaN)
    lat = torch.asin(s)
    lon = torch.atan2(-X[:, 0], X[:, 1])
    lon0 = grid.axes[1][0]
    lon = lon - TWO_PI * torch.floor((lon - lon0) / TWO_PI)
    lon = torch.where(lon < lon0, lon + TWO_PI, lon)
    lon = torch.where(lon >= lon0 + TWO_PI, lon - TWO_PI, lon)
    return torch.stack([lat, lon, r], -1)


def locate(grid, u, lon_mode='patch'):
    """Per axis the lower node ``i0``, the upper node ``i1`` (both (M, 3) long) and the weight ``t`` (M, 3) of the upper node,
    and ``inside (M,)``.  Cell: ``searchsorted(axis, u, 'left') - 1`` clipped to ``[0, n - 2]``; on an open periodic longitude
    the wrap cell joins node ``n - 1`` to node 0 at ``lon[0] + 2 pi``.  Outside samples get cell 0 and weight 0."""
    assert lon_mode in LON_MODES
    periodic = grid.kind == 'spherical' and lon_mode != 'patch'
    m = u.shape[0]
    inside = torch.ones(m, dtype=torch.bool)
    for k, axis in enumerate(grid.axes):
        if k == 1 and periodic:
            inside &= ~torch.isnan(u[:, 1])
        else:
            inside &= (u[:, k] >= axis[0]) & (u[:, k] <= axis[-1])        # (False for a NaN)
    i0 = torch.zeros(m, 3, dtype=torch.long)
    i1 = torch.zeros(m, 3, dtype=torch.long)
    t = torch.zeros(m, 3, dtype=torch.float64)
    for k, axis in enumerate(grid.axes):
        n = axis.shape[0]
        uk = torch.where(inside, u[:, k], axis[0].expand(m))
        cell = (torch.searchsorted(axis, uk.contiguous(), right=False) - 1).clamp(0, n - 2)
        lo, hi = axis[cell], axis[cell + 1]
        tk = (uk - lo) / (hi - lo)
        upper = cell + 1
        if k == 1 and periodic and lon_mode == 'open':
            wrap = uk > axis[-1]
            cell = torch.where(wrap, torch.full_like(cell, n - 1), cell)
            upper = torch.where(wrap, torch.zeros_like(cell), upper)
            tk = torch.where(wrap, (uk - axis[-1]) / ((axis[0] + TWO_PI) - axis[-1]), tk)
        i0[:, k], i1[:, k], t[:, k] = cell, upper, torch.where(inside, tk, torch.zeros_like(tk))
    return i0, i1, t, inside


def field(grid, values, points, fill, Rs_per_ds=1.0, lon_mode='patch'):
    """The field at fp32 ``points (M, >= 3)``: ``(raw (M, C) float64, abs_sum (M, C) = sum over corners |w| |v|, inside (M,))``.
    ``values (n0, n1, n2, C)`` (promoted; gradients flow to a float64 leaf passed in), ``fill (C,)``."""
    v = values.double()
    u = grid_coordinates(grid, points, Rs_per_ds, lon_mode)
    i0, i1, t, inside = locate(grid, u, lon_mode)
    raw = torch.zeros(points.shape[0], v.shape[-1], dtype=torch.float64)
    abs_sum = torch.zeros_like(raw)
    for d0 in (0, 1):
        for d1 in (0, 1):
            for d2 in (0, 1):
                idx = [(i1 if d else i0)[:, k] for k, d in enumerate((d0, d1, d2))]
                w = torch.ones(points.shape[0], dtype=torch.float64)
                for k, d in enumerate((d0, d1, d2)):
                    w = w * (t[:, k] if d else 1 - t[:, k])
                corner = v[idx[0], idx[1], idx[2]]
                raw = raw + w[:, None] * corner
                abs_sum = abs_sum + w.abs()[:, None] * corner.detach().abs()
    fill = torch.as_tensor(fill, dtype=torch.float64).reshape(1, -1)
    raw = torch.where(inside[:, None], raw, fill.expand_as(raw))
    abs_sum = torch.where(inside[:, None], abs_sum, torch.zeros_like(abs_sum))
    return raw, abs_sum, inside


def field_on_rays(grid, values, rays_o, rays_d, z_vals, fill, Rs_per_ds=1.0, lon_mode='patch'):
    """:func:`field` at the samples of a ray batch: ``(raw (N, S, C), abs_sum (N, S, C), inside (N, S))``."""
    pts = ray_points(rays_o, rays_d, z_vals)
    n, s = pts.shape[:2]
    raw, abs_sum, inside = field(grid, values, pts.reshape(-1, 3), fill, Rs_per_ds, lon_mode)
    return raw.reshape(n, s, -1), abs_sum.reshape(n, s, -1), inside.reshape(n, s)


def boundary_distance(grid, points, Rs_per_ds=1.0, lon_mode='patch'):
    """(M,) distance [coordinate units] of every point's grid coordinates from the nearest face of the domain (a periodic
    longitude has none); NaN coordinates give +inf (they are outside whatever the rounding)."""
    u = grid_coordinates(grid, points, Rs_per_ds, lon_mode)
    periodic = grid.kind == 'spherical' and lon_mode != 'patch'
    dist = torch.full((points.shape[0],), float('inf'), dtype=torch.float64)
    for k, axis in enumerate(grid.axes):
        if k == 1 and periodic:
            continue
        dk = torch.minimum((u[:, k] - axis[0]).abs(), (u[:, k] - axis[-1]).abs())
        dist = torch.minimum(dist, torch.where(torch.isnan(dk), torch.full_like(dk, float('inf')), dk))
    return dist


def node_terms(grid, points, g_raw, Rs_per_ds=1.0, lon_mode='patch'):
    """What bounds one node of the adjoint on its own, from this restatement's cells and weights: ``(A (n0, n1, n2, C), n (n0,
    n1, n2) long)`` with ``A = sum_s |w_s| |g_s|`` over the inside samples whose cell touches the node (``w_s``: the sample's
    float64 corner weight at the node) and ``n`` their number.  ``points (M, >= 3)`` fp32, ``g_raw (M, C)``."""
    u = grid_coordinates(grid, points, Rs_per_ds, lon_mode)
    i0, i1, t, inside = locate(grid, u, lon_mode)
    n0, n1, n2 = (int(a.shape[0]) for a in grid.axes)
    g = g_raw.reshape(points.shape[0], -1).double().abs()
    terms = torch.zeros(n0 * n1 * n2, g.shape[1], dtype=torch.float64)
    count = torch.zeros(n0 * n1 * n2, dtype=torch.long)
    for d0 in (0, 1):
        for d1 in (0, 1):
            for d2 in (0, 1):
                idx = [(i1 if d else i0)[:, k] for k, d in enumerate((d0, d1, d2))]
                w = torch.ones(points.shape[0], dtype=torch.float64)
                for k, d in enumerate((d0, d1, d2)):
                    w = w * (t[:, k] if d else 1 - t[:, k])
                flat = ((idx[0] * n1 + idx[1]) * n2 + idx[2])[inside]
                terms.index_add_(0, flat, (w.abs()[:, None] * g)[inside])
                count.index_add_(0, flat, torch.ones_like(flat))
    return terms.reshape(n0, n1, n2, -1), count.reshape(n0, n1, n2)


def smoothness(grid, values, lon_mode='patch'):
    """Hand computation of ``GridField.smoothness()`` with Python loops over the axes' differences (float64)."""
    v = values.double()
    total = 0.0
    for k, axis in enumerate(grid.axes):
        terms = []
        for i in range(axis.shape[0] - 1):
            step = (axis[i + 1] - axis[i]).item()
            terms.append(((v.select(k, i + 1) - v.select(k, i)) / step) ** 2)
        if k == 1 and grid.kind == 'spherical' and lon_mode != 'patch':
            n = axis.shape[0]
            seam = (axis[0] + TWO_PI - axis[-1]).item() if lon_mode == 'open' else ((axis[-1] - axis[0]) / (n - 1)).item()
            terms.append(((v.select(1, 0) - v.select(1, n - 1)) / seam) ** 2)
        total = total + torch.stack(terms).mean()
    return total / 3.0
