"""fp64 restatement of the reference's ``MHDModel`` (sunerf/model/mhd_model.py) for the MHD tests, and the synthetic cubes
they run on.

Coordinates and time are computed with torch fp32 on the CPU exactly as the reference writes them (:100-103, :121-124); the
trilinear interpolation of ``RegularGridInterpolator(method='linear', bounds_error=False, fill_value=1e-10)`` over the
axes (phi, theta, r) (:45-75) is restated in float64; the interpolated values are rounded to fp32 (``torch.Tensor`` of the
float64 result, :127-134) and blended in time and taken to logarithms in fp32 (:137-138)."""
import os

import numpy as np
import torch

FILL = 1e-10


def spherical(points):
    """mhd_model.py:100-103 on (M, >=3) fp32 points -> (r, theta, phi) fp32."""
    x, y, z = points[:, 0], points[:, 1], points[:, 2]
    r = torch.sqrt(x ** 2 + y ** 2 + z ** 2)
    th = torch.arccos(z / r)
    phi = torch.arctan2(y, x)
    phi[phi < 0] += 2 * np.pi
    return r, th, phi


def frame_pair(t, ffirst, flast):
    """mhd_model.py:121-124 per point, fp32: (f1, f2, w)."""
    f = t.to(torch.float32) * (flast - ffirst) + ffirst
    w = f - torch.trunc(f)
    return torch.floor(f).to(torch.int64), torch.ceil(f).to(torch.int64), w


def interp_linear(axes, data, coords):
    """RegularGridInterpolator(axes, data, method='linear', bounds_error=False, fill_value=1e-10)(coords) in float64.
    ``axes`` = (phi, theta, r), ``data[i_phi, i_theta, i_r]`` (negatives NOT yet clamped), ``coords`` (M, 3)."""
    data = np.where(data < 0, FILL, data).astype(np.float64)       # mhd_model.py:64
    coords = np.asarray(coords, dtype=np.float64)
    idx, wts = [], []
    out_of_bounds = np.zeros(coords.shape[0], dtype=bool)
    for k, g in enumerate(axes):
        g = np.asarray(g, dtype=np.float64)
        x = coords[:, k]
        i = np.clip(np.searchsorted(g, x) - 1, 0, g.size - 2)
        idx.append(i)
        wts.append((x - g[i]) / (g[i + 1] - g[i]))
        out_of_bounds |= (x < g[0]) | (x > g[-1])
    value = np.zeros(coords.shape[0])
    for corner in range(8):
        bits = [(corner >> (2 - k)) & 1 for k in range(3)]
        w = np.ones(coords.shape[0])
        for k in range(3):
            w = w * (wts[k] if bits[k] else 1 - wts[k])
        value += w * data[idx[0] + bits[0], idx[1] + bits[1], idx[2] + bits[2]]
    value[out_of_bounds] = FILL
    value[np.isnan(coords).any(1)] = np.nan
    return value


def mhd_field(points, frames, ffirst, flast):
    """MHDModel.forward (mhd_model.py:76-142) on (M, 4) fp32 points -> (M, 2) fp32 (ln rho, log10 T).
    ``frames[f] = (r, theta, phi, rho, T)`` as a reader returns them."""
    points = points.to(torch.float32)
    r, th, phi = spherical(points)
    f1, f2, w = frame_pair(points[:, 3], ffirst, flast)
    coords = torch.stack([phi, th, r], -1).numpy()
    out = torch.full((points.shape[0], 2), float('nan'), dtype=torch.float32)
    ok = ~torch.isnan(points[:, 3])
    pairs = torch.stack([f1, f2], -1)
    for pair in torch.unique(pairs[ok], dim=0).tolist():
        sel = ok & (f1 == pair[0]) & (f2 == pair[1])
        vals = []
        for f in pair:
            fr_r, fr_th, fr_phi, rho, temp = frames[f]
            axes = (fr_phi, fr_th, fr_r)
            vals.append([torch.tensor(interp_linear(axes, v, coords[sel.numpy()]), dtype=torch.float64).to(torch.float32)
                         for v in (rho, temp)])
        ws = w[sel]
        out[sel, 0] = torch.log((1 - ws) * vals[0][0] + ws * vals[1][0])
        out[sel, 1] = torch.log10(1e6 * ((1 - ws) * vals[0][1] + ws * vals[1][1]))
    return out


# ---- synthetic cubes ------------------------------------------------------------------------------------------------------
def _f32(a):
    return np.asarray(a, dtype=np.float32).astype(np.float64)      # nodes that fp32 holds exactly (the model keeps fp32 grids)


def synthetic_frame(seed, n_phi=23, n_theta=17, n_r=29, r_range=(1.02, 1.4), phi_end=0.96 * 2 * np.pi):
    """(r, theta, phi, rho, T) of one frame on non-uniform grids: r clustered at the inner boundary like PSI's, theta and
    phi jittered, phi stopping short of 2 pi; a smooth positive density ~1e8 and temperature ~1.5 (MK) with a few negative
    entries (clamped to 1e-10 by the model, mhd_model.py:64)."""
    rng = np.random.default_rng(seed)
    u = np.linspace(0., 1., n_r)
    r = _f32(r_range[0] + (r_range[1] - r_range[0]) * u ** 2.2)
    th_u = np.linspace(0., 1., n_theta) + np.r_[0., rng.uniform(-0.3, 0.3, n_theta - 2) / n_theta, 0.]
    th = _f32(0.02 + (np.pi - 0.04) * th_u)
    ph_u = np.linspace(0., 1., n_phi) + np.r_[0., rng.uniform(-0.3, 0.3, n_phi - 2) / n_phi, 0.]
    phi = _f32(0.01 + (phi_end - 0.01) * ph_u)
    P, T_, R = np.meshgrid(phi, th, r, indexing='ij')
    a = rng.uniform(0.5, 1.5, 3)
    rho = 1e8 * np.exp(-(R - 1.) / 0.05) * (1.2 + 0.3 * np.sin(a[0] * P) * np.sin(T_) + 0.1 * np.cos(a[1] * T_))
    temp = 1.2 + 0.4 * (R - 1.) / 0.25 + 0.2 * np.cos(a[2] * P + T_) * np.sin(T_)
    for v in (rho, temp):
        flat = v.reshape(-1)
        flat[rng.choice(flat.size, 6, replace=False)] *= -1.
    return r, th, phi, rho, temp


class DictReader:
    """``reader=`` for MHDModel: placeholder files in ``root`` mapped to in-memory frames (path -> (r, theta, phi, data))."""

    def __init__(self, frames):
        self.frames = frames
        self.calls = 0

    def __call__(self, path):
        self.calls += 1
        name = os.path.basename(path)
        var = os.path.basename(os.path.dirname(path))
        f = int(name.split('00')[1].split('.h5')[0])
        r, th, phi, rho, temp = self.frames[f]
        return r, th, phi, (rho if var == 'rho' else temp)


def write_placeholders(root, frame_numbers, variables=('rho', 't')):
    """Empty ``{var}/{var}00{f}.h5`` files (mhd_model.py:27-30, :62) under ``root``."""
    for var in variables:
        os.makedirs(os.path.join(root, var), exist_ok=True)
        for f in frame_numbers:
            open(os.path.join(root, var, f'{var}00{f}.h5'), 'wb').close()
    return str(root)


def psi_clustered_r(n_r=301):
    """PSI-like r grid: 1 ... 30 solar radii, strongly clustered at 1 (smallest spacing ~1e-6, span / spacing ~2.7e7)."""
    return _f32(1. + 29. * np.linspace(0., 1., n_r) ** 3)


def psi_clustered_frame(seed, n_phi=9, n_theta=7, n_r=301):
    """(r, theta, phi, rho, T) on :func:`psi_clustered_r` with a few theta and phi nodes: smooth, positive."""
    rng = np.random.default_rng(seed)
    r = psi_clustered_r(n_r)
    th = _f32(np.linspace(0.05, np.pi - 0.05, n_theta))
    phi = _f32(np.linspace(0.01, 2 * np.pi - 0.01, n_phi))
    P, T_, R = np.meshgrid(phi, th, r, indexing='ij')
    a = rng.uniform(0.5, 1.5, 2)
    rho = 1e8 * np.exp(-(R - 1.) / 0.1) * (1.2 + 0.3 * np.sin(a[0] * P) * np.sin(T_)) + 1e3 / R ** 2
    temp = 1.2 + 0.3 * np.cos(a[1] * P + T_) * np.sin(T_) + 0.01 * R
    return r, th, phi, rho, temp
