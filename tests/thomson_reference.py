"""float64 restatement of the white-light Thomson-scattering integral, written from the equations of
Howard & Tappin 2009 as the issue states them -- the checker of csrc/thomson.hip -- plus an fp32 "literal" variant that
evaluates the reference's expressions (sin / cos of asin(R / r), 10 ** raw) in fp32, to document the reference's own drift.

Both take torch tensors on the CPU and are differentiable w.r.t. ``raw`` through torch autograd."""
import math

import numpy as np
import torch

LN10 = math.log(10.)
KEYS = ('pixel_B', 'pixel_density', 'distance_from_sun', 'distance_from_obs', 'weights')


def geometry_factors(sin_omega: torch.Tensor, cos2_omega=None):
    """(A, B, C, D) of Howard & Tappin 2009 eqs. 23, 24, 29 for sin(Omega) = R / r (any dtype, no masking).  ``cos2_omega``:
    cos^2(Omega) where the caller holds it more exactly than 1 - sin^2 (next to the limb, see :func:`_geometry`)."""
    s = sin_omega
    c2 = 1 - s * s if cos2_omega is None else cos2_omega
    c = torch.sqrt(c2)
    L = torch.log((1 + s) / c)
    k = c2 / s * L
    A = c * s * s
    B = -(1 / 8) * (1 - 3 * s * s - k * (1 + 3 * s * s))
    C = 4 / 3 - c - c ** 3 / 3
    D = (1 / 8) * (5 + s * s - k * (5 - s * s))
    return A, B, C, D


def _geometry(r2, rays_o, rays_d, R, u, dtype):
    """|I_tot|, |I_P| per sample from its squared radius.  cos^2(Omega) = (r^2 - R^2) / r^2: next to the limb the difference
    of the squares is exact, where 1 - (R / r)^2 keeps only the rounding of r (one step of z outside a limb at R = 1 / 0.7 that
    is 1e-3 of cos(Omega), and all of I_P = cos(Omega) sin^2(Omega) sin^2(chi) when u = 0)."""
    r = torch.sqrt(r2)
    s = R / r
    A, B, C, D = geometry_factors(s, (r2 - R * R) / r2)
    cross = torch.cross(rays_o.to(dtype), rays_d.to(dtype), dim=-1).pow(2).sum(-1)
    sin2chi = cross[:, None] / (rays_d.to(dtype).pow(2).sum(-1)[:, None] * r2)
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
    r2 = pts.pow(2).sum(-1)
    r = torch.sqrt(r2)
    i_tot, i_p = _geometry(r2, rays_o, rays_d, solar_radius, limb, dtype)
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


# ---- the limb: a second, cancellation-free evaluation and the seam cases --------------------------------------------------
LONG_DOUBLE_IS_WIDER = np.finfo(np.longdouble).eps < np.finfo(np.float64).eps


def intensities_longdouble(z_vals, rays_o, rays_d, solar_radius=1.0, limb=0.63):
    """(|I_tot|, |I_P|, r - R) per sample in numpy ``longdouble``, written from Howard & Tappin's eqs. 23, 24, 29 in forms that
    do not cancel at the limb: c^2 = (r - R)(r + R) / r^2 instead of 1 - s^2, L = log1p(2 s / (1 - s)) / 2 instead of
    ln((1 + s) / c), C = s^2 / (1 + c) (4 + c + c^2) / 3 instead of 4/3 - c - c^3/3.  Measures the rounding noise of
    :func:`thomson_integral`'s fp64 geometry where c -> 0; zero where r <= R or a value is not finite."""
    ld = np.longdouble
    z, o, d = (np.asarray(t.detach().cpu().numpy(), dtype=np.float64).astype(ld) for t in (z_vals, rays_o, rays_d))
    R, u = ld(solar_radius), ld(limb)
    pts = o[:, None, :] + d[:, None, :] * z[..., None]
    r2 = (pts * pts).sum(-1)
    r = np.sqrt(r2)
    with np.errstate(all='ignore'):
        s = R / r
        c2 = (r - R) * (r + R) / r2
        c = np.sqrt(c2)
        L = np.log1p(2 * s / (1 - s)) / 2
        k = c2 / s * L
        A = c * s * s
        B = -(1 - 3 * s * s - k * (1 + 3 * s * s)) / 8
        C = s * s / (1 + c) * (4 + c + c2) / 3
        D = (5 + s * s - k * (5 - s * s)) / 8
        cross = np.cross(o, d)
        sin2chi = (cross * cross).sum(-1)[:, None] / ((d * d).sum(-1)[:, None] * r2)
        i_p = sin2chi * ((1 - u) * A + u * B)
        i_tot = np.abs(2 * ((1 - u) * C + u * D) - i_p)
        i_p = np.abs(i_p)
        bad = ~(r > R) | ~np.isfinite(i_tot) | ~np.isfinite(i_p)
    return np.where(bad, ld(0), i_tot), np.where(bad, ld(0), i_p), r - R


def intensities_fp64(z_vals, rays_o, rays_d, solar_radius=1.0, limb=0.63):
    """(|I_tot|, |I_P|, r - R) per sample as :func:`thomson_integral` evaluates them (fp64 torch tensors)."""
    z, o, d = (t.double() for t in (z_vals, rays_o, rays_d))
    r2 = (o[:, None, :] + d[:, None, :] * z[..., None]).pow(2).sum(-1)
    i_tot, i_p = _geometry(r2, rays_o, rays_d, solar_radius, limb, torch.float64)
    return i_tot, i_p, torch.sqrt(r2) - solar_radius


SEAM_SCALES = (1.0, 0.5, 2.0)      # |d| of the seam rays (powers of two: d z stays exact)


def _step(x, towards):
    return float(np.nextafter(np.float32(x), np.float32(towards)))


def seam_cases(solar_radius, c=1, seed=0):
    """Two-sample rays whose sample 0 lies on the limb by bits, or one fp32 step of z beside it; sample 1 is a far point muted
    with raw0 = -inf (rho = 0 in every precision).  Axis-aligned rays, so o + d z, r^2 and r are exact in fp64 on the limb and
    no contraction of a multiply-add can move the decision.  Per |d| in SEAM_SCALES (z scaled inversely):

      tangent ray o = (0, -8, R), d = (0, |d|, 0): z |d| = 8 is on the limb (r == R), both neighbours are outside;
      radial ray  o = (0, -2R, 0), d = (0, |d|, 0): z |d| = R is on the limb, one step towards 0 is outside, one step away is
                  inside; |o x d| = 0, so pB is exactly 0 for all three.

    Returns (raw (N,2,c), z (N,2), o, d fp32 CPU tensors, info): ``info[i] = dict(name, side, radial, scale)`` with
    ``side`` = 0 on the limb, +1 outside (live), -1 inside; the live-or-seam sample is index 0 of every ray."""
    R = float(np.float32(solar_radius))
    assert R == solar_radius, 'solar_radius must be an fp32 value'
    o, d, z, info = [], [], [], []
    for scale in SEAM_SCALES:
        z0 = 8.0 / scale
        for name, zz, side in (('on', z0, 0), ('below', _step(z0, 0.), 1), ('above', _step(z0, np.inf), 1)):
            o.append([0., -8., R]); d.append([0., scale, 0.]); z.append([zz, 16.0 / scale])
            info.append(dict(name=f'tangent-{name}', side=side, radial=False, scale=scale))
        z0 = R / scale
        for name, zz, side in (('on', z0, 0), ('before', _step(z0, 0.), 1), ('after', _step(z0, np.inf), -1)):
            o.append([0., -2 * R, 0.]); d.append([0., scale, 0.]); z.append([zz, 4 * R / scale])
            info.append(dict(name=f'radial-{name}', side=side, radial=True, scale=scale))
    n = len(info)
    gen = torch.Generator().manual_seed(seed)
    raw = torch.randn(n, 2, c, generator=gen) * 0.5
    raw[:, 1, 0] = float('-inf')
    f32 = lambda x: torch.tensor(x, dtype=torch.float64).float().contiguous()
    o, d, z = f32(o), f32(d), f32(z)
    return raw.float().contiguous(), z, o, d, info


def chunk_seam_case(solar_radius, s, index, c=1, seed=0):
    """One tangent ray o = (0, -8, R), d = (0, 1, 0) of ``s`` sorted samples whose sample ``index`` is the limb point z = 8
    (r == R by bits); every other sample is live and outside, at steps of 0.05 ... 0.1.  The limb sample carries the largest
    density (raw0 + 1.5), so a kernel that let it through would move tB far past the gate."""
    R = float(np.float32(solar_radius))
    gen = torch.Generator().manual_seed(seed + 131 * s + index)
    steps = 0.05 + 0.05 * torch.rand(s, generator=gen, dtype=torch.float64)
    z = torch.cumsum(steps, 0)
    z = (z - z[index]).float().double() + 8.0
    z = z.float()
    assert z[index].item() == 8.0 and bool((z[1:] > z[:-1]).all())
    raw = torch.randn(1, s, c, generator=gen) * 0.5
    raw[0, index, 0] += 1.5
    o = torch.tensor([[0., -8., R]], dtype=torch.float32)
    d = torch.tensor([[0., 1., 0.]], dtype=torch.float32)
    return raw.float().contiguous(), z[None].contiguous(), o, d


def degenerate_rays(solar_radius, s, c=1, seed=0):
    """Four rays of ``s`` samples (s >= 8) that the integral defines but ordinary batches never hold, and their names:

      centre : o = (120, -150, 90) R / 64, d = -o / 128: o x d = 0 by bits (every product of the cross is exact in fp64), pB = 0
      null-d : d = (0, 0, 0): |o x d|^2 / |d|^2 = 0 / 0; every line element is 0, r = |o| for every sample
      origin : o = (0, -2R, 0), d = (0, 1, 0) with one sample at z = 2R: r = 0, R / r = inf
      repeats: an ordinary oblique ray whose z comes in runs of three equal values (D_j = 0 inside a run)"""
    assert s >= 8
    R = float(np.float32(solar_radius))
    gen = torch.Generator().manual_seed(seed)
    o = torch.tensor([[120., -150., 90.], [3., -2., 1.5], [0., -128., 0.], [0.5, -100., 1.25]], dtype=torch.float64) * (R / 64)
    o[1] *= 64
    d = torch.stack([-o[0] / 128, torch.zeros(3, dtype=torch.float64), torch.tensor([0., 1., 0.], dtype=torch.float64),
                     torch.tensor([0.1, 1., -0.05], dtype=torch.float64)])
    o, d = o.float(), d.float()
    z = torch.empty(4, s, dtype=torch.float64)
    z[0] = torch.sort(torch.rand(s, generator=gen, dtype=torch.float64)).values * 256          # through the centre at z = 128
    z[1] = torch.sort(torch.rand(s, generator=gen, dtype=torch.float64)).values * 10
    z[2] = torch.sort(torch.rand(s, generator=gen, dtype=torch.float64)).values * 4 * R
    z[2, s // 2] = 2 * R
    z[2] = torch.sort(z[2]).values
    runs = torch.sort(torch.rand((s + 2) // 3, generator=gen, dtype=torch.float64)).values * 4 * R
    z[3] = runs.repeat_interleave(3)[:s]
    z = z.float()
    assert bool((z[2] == np.float32(2 * R)).any()) and bool((z[3, 1:] == z[3, :-1]).any())
    raw = (torch.randn(4, s, c, generator=gen) * 0.7).float()
    names = ('centre', 'null-d', 'origin', 'repeats')
    return raw.contiguous(), z.contiguous(), o.contiguous(), d.contiguous(), names
