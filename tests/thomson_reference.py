"""float64 restatement of the white-light Thomson-scattering integral, written from the equations of
Howard & Tappin 2009 as the issue states them -- the checker of csrc/thomson.hip -- plus an fp32 "literal" variant that
evaluates the reference's expressions (sin / cos of asin(R / r), 10 ** raw) in fp32, to document the reference's own drift.

Both take torch tensors on the CPU and are differentiable w.r.t. ``raw`` through torch autograd."""
import math

import torch

LN10 = math.log(10.)
KEYS = ('pixel_B', 'pixel_density', 'distance_from_sun', 'distance_from_obs', 'weights')


def geometry_factors(sin_omega: torch.Tensor):
    """(A, B, C, D) of Howard & Tappin 2009 eqs. 23, 24, 29 for sin(Omega) = R / r (any dtype, no masking)."""
    s = sin_omega
    c = torch.sqrt(1 - s * s)
    L = torch.log((1 + s) / c)
    k = c * c / s * L
    A = c * s * s
    B = -(1 / 8) * (1 - 3 * s * s - k * (1 + 3 * s * s))
    C = 4 / 3 - c - c ** 3 / 3
    D = (1 / 8) * (5 + s * s - k * (5 - s * s))
    return A, B, C, D


def _geometry(r, rays_o, rays_d, R, u, dtype):
    s = R / r
    A, B, C, D = geometry_factors(s)
    cross = torch.cross(rays_o.to(dtype), rays_d.to(dtype), dim=-1).pow(2).sum(-1)
    sin2chi = cross[:, None] / (rays_d.to(dtype).pow(2).sum(-1)[:, None] * r * r)
    i_t = (1 - u) * C + u * D
    i_p = sin2chi * ((1 - u) * A + u * B)
    i_tot = 2 * i_t - i_p
    i_tot, i_p = i_tot.abs(), i_p.abs()
    bad = ~(r > R) | ~torch.isfinite(i_tot) | ~torch.isfinite(i_p)
    zero = torch.zeros((), dtype=dtype)
    return torch.where(bad, zero, i_tot), torch.where(bad, zero, i_p)


def thomson_integral(raw, z_vals, rays_o, rays_d, kappa, solar_radius=1.0, limb=0.63, c0=1.0, dtype=torch.float64):
    """The five outputs of ``ThompsonScattering.raw2outputs`` in ``dtype`` (fp32 inputs converted exactly).  ``raw`` (N,S,C):
    rho = exp(kappa raw[..., 0]); solar_radius / limb / c0 as Python floats (the fp32 buffer values)."""
    raw, z, o, d = (t.to(dtype) for t in (raw, z_vals, rays_o, rays_d))
    rho = torch.exp(kappa * raw[..., 0])
    length = d.norm(dim=-1)
    pts = o[:, None, :] + d[:, None, :] * z[..., None]
    r = pts.norm(dim=-1)
    i_tot, i_p = _geometry(r, rays_o, rays_d, solar_radius, limb, dtype)
    dz = z[:, 1:] - z[:, :-1]
    dists = torch.cat([dz[:, :1], dz], -1) * length[:, None]
    if z.shape[1] == 1:
        tb = pb = den = torch.zeros(z.shape[0], dtype=dtype)          # no line element: the empty sums of the reference
    else:
        tb = (c0 * rho * i_tot * dists).sum(-1)
        pb = (c0 * rho * i_p * dists).sum(-1)
        den = (rho * dists).sum(-1)
    m = rho.sum(-1) + 1e-10
    return {'pixel_B': torch.stack([tb, pb], -1), 'pixel_density': den, 'distance_from_sun': (rho * r).sum(-1) / m,
            'distance_from_obs': (rho * z * length[:, None]).sum(-1) / m, 'weights': rho / m[:, None]}


def thomson_literal_fp32(raw, z_vals, rays_o, rays_d, log10=True, solar_radius=1.0, limb=0.63, c0=1.0):
    """The reference's own arithmetic in fp32 (thompson.py:25-101: 10 ** raw, omega = asin(R / r), its sin / cos powers),
    restricted to the spatial radius: the drift the fp64 kernel removes."""
    raw, z, o, d = (t.float() for t in (raw, z_vals, rays_o, rays_d))
    rho = 10 ** raw[..., 0] if log10 else torch.exp(raw[..., 0])
    length = d.norm(dim=-1)
    pts = o[:, None, :] + d[:, None, :] * z[..., None]
    r = pts.norm(dim=-1)
    omega = torch.asin(solar_radius / r)
    s, c = torch.sin(omega), torch.cos(omega)
    L = torch.log((1 + s) / c)
    k = c ** 2 / s
    A = c * s ** 2
    B = -(1 / 8) * (1 - 3 * s ** 2 - k * (1 + 3 * s ** 2) * L)
    C = (4 / 3) - c - c ** 3 / 3
    D = (1 / 8) * (5 + s ** 2 - k * (5 - s ** 2) * L)
    sin2chi = torch.cross(o, d, dim=-1).pow(2).sum(-1)[:, None] / pts.pow(2).sum(-1)
    i_tot = (2 * ((1 - limb) * C + limb * D) - sin2chi * ((1 - limb) * A + limb * B)).abs()
    i_p = (sin2chi * ((1 - limb) * A + limb * B)).abs()
    i_tot = torch.nan_to_num(i_tot, nan=0., posinf=0., neginf=0.)
    i_p = torch.nan_to_num(i_p, nan=0., posinf=0., neginf=0.)
    dz = z[:, 1:] - z[:, :-1]
    dists = torch.cat([dz[:, :1], dz], -1) * length[:, None]
    tb = (c0 * rho * i_tot * dists).sum(-1)
    pb = (c0 * rho * i_p * dists).sum(-1)
    return torch.stack([tb, pb], -1)
