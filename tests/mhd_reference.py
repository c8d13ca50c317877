"""fp64 restatement of the reference's ``MHDModel`` (sunerf/model/mhd_model.py) for the MHD tests, and the synthetic cubes
they run on.

Coordinates and time are computed with torch fp32 on the CPU exactly as the reference writes them (:100-103, :121-124); the
trilinear interpolation of ``RegularGridInterpolator(method='linear', bounds_error=False, fill_value=1e-10)`` over the
axes (phi, theta, r) (:45-75) is restated in float64; the interpolated values are rounded to fp32 (``torch.Tensor`` of the
float64 result, :127-134) and blended in time and taken to logarithms in fp32 (:137-138).

The second half serves the seam tests (tests/test_gpu_mhd_seams.py): the field with its intermediates, cubes whose nodes fp32
holds exactly, the points and times that sit on their seams, grids built from a set of points' own angles, and an fp64 grid
that fp32 cannot hold."""
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


# ---- the field with its intermediates, and cubes whose seams a point can sit on exactly -------------------------------------
def in_bounds(axes, coords):
    """scipy's bounds test of ``RegularGridInterpolator`` (inclusive on both ends; False for a NaN coordinate)."""
    coords = np.asarray(coords, dtype=np.float64)
    ok = np.ones(coords.shape[0], dtype=bool)
    for k, g in enumerate(axes):
        ok &= (coords[:, k] >= np.float64(g[0])) & (coords[:, k] <= np.float64(g[-1]))
    return ok


def mhd_field_parts(points, frames, ffirst, flast):
    """:func:`mhd_field` with what it went through: ``(out (M, 2) fp32, (r, theta, phi) fp32 as the reference computes them,
    (f1, f2, w), inside (M, 2) bool: the point is within the grid of frame f1 / f2)``."""
    points = points.to(torch.float32)
    r, th, phi = spherical(points.clone())
    f1, f2, w = frame_pair(points[:, 3], ffirst, flast)
    coords = torch.stack([phi, th, r], -1).numpy()
    ok = ~torch.isnan(points[:, 3])
    inside = torch.zeros(points.shape[0], 2, dtype=torch.bool)
    vals = torch.full((points.shape[0], 2, 2), float('nan'), dtype=torch.float32)          # [point, frame of the pair, variable]
    for k, fk in enumerate((f1, f2)):
        for f in torch.unique(fk[ok]).tolist():
            sel = (ok & (fk == f)).numpy()
            fr_r, fr_th, fr_phi, rho, temp = frames[f]
            axes = (fr_phi, fr_th, fr_r)
            inside[sel, k] = torch.from_numpy(in_bounds(axes, coords[sel]))
            for j, v in enumerate((rho, temp)):
                vals[sel, k, j] = torch.tensor(interp_linear(axes, v, coords[sel]), dtype=torch.float64).to(torch.float32)
    out = torch.stack([torch.log((1 - w) * vals[:, 0, 0] + w * vals[:, 1, 0]),
                       torch.log10(1e6 * ((1 - w) * vals[:, 0, 1] + w * vals[:, 1, 1]))], -1)
    return out, (r, th, phi), (f1, f2, w), inside


def fl32(x):
    return np.float64(np.float32(x))


PI32, HALF_PI32, TWO_PI32 = fl32(np.pi), fl32(np.pi / 2), fl32(2 * np.pi)
QUARTER_PI32 = fl32(np.pi / 4)
THREE_HALF_PI32 = np.float64(np.float32(-np.pi / 2) + np.float32(2 * np.pi))     # atan2(-1, 0) + 2 pi as fp32 adds it
SEAM_R_WIDE = (1.0, 1.03125, 1.0625, 1.125, 1.25, 1.5, 2.0)                         # few mantissa bits: sqrt(r^2) = r in any sqrt
SEAM_R_NARROW = (1.0625, 1.125, 1.25, 1.5)
SEAM_THETA = (0., 0.5, 1.0, HALF_PI32, 2.0, 2.5, PI32)
SEAM_PHI = (0., 0.5, QUARTER_PI32, HALF_PI32, 2.5, PI32, 4.0, THREE_HALF_PI32, 5.5, TWO_PI32)


def seam_frame(seed, r_nodes=SEAM_R_WIDE, theta_nodes=SEAM_THETA, phi_nodes=SEAM_PHI):
    """(r, theta, phi, rho, T) of one frame whose nodes fp32 holds exactly and whose special angles are the fp32 values the
    coordinate functions return on the axes: theta from 0 to fl32(pi) through fl32(pi / 2); phi from 0 to fl32(2 pi) through
    fl32(pi / 2), fl32(pi) and fl32(-pi / 2) + fl32(2 pi).  Smooth positive data, no negative entries, distinct at
    every node."""
    rng = np.random.default_rng(seed)
    r, th, phi = (np.asarray(a, dtype=np.float64) for a in (r_nodes, theta_nodes, phi_nodes))
    for a in (r, th, phi):
        assert np.array_equal(a, _f32(a)) and (np.diff(a) > 0).all()
    P, T_, R = np.meshgrid(phi, th, r, indexing='ij')
    a = rng.uniform(0.5, 1.5, 3)
    rho = 1e8 * np.exp(-(R - 1.) / 0.3) * (1.3 + 0.3 * np.sin(a[0] * P + 0.3) * np.sin(T_) + 0.1 * np.cos(a[1] * T_))
    temp = 1.2 + 0.4 * (R - 1.) + 0.2 * np.cos(a[2] * P + T_) * np.sin(T_ + 0.2)
    assert rho.min() > 0 and temp.min() > 0
    return r, th, phi, rho, temp


def general_position_frames(points, seeds=(21, 22)):
    """Frames (one per seed, on one grid) whose interior theta and phi nodes are the reference's own fp32 theta and phi of
    ``points`` (M, >=3), between bounds well outside ([-0.25, 3.5] and [-0.25, 6.75]): every point lies on a node of both
    angular axes, up to the difference between the device's and the host's acosf / atan2f."""
    _, th, phi = spherical(points.to(torch.float32).clone())
    th = np.r_[-0.25, np.unique(th.numpy().astype(np.float64)), 3.5]
    phi = np.r_[-0.25, np.unique(phi.numpy().astype(np.float64)), 6.75]
    return [seam_frame(s, theta_nodes=th, phi_nodes=phi) for s in seeds]


def unrounded_frame(seed, n_phi=27, n_theta=19, n_r=31):
    """(r, theta, phi, rho, T) on ``np.linspace`` grids as a simulation writes them in fp64: almost no node is an fp32 number,
    so the model's fp32 copy of the grid differs from the grid the reference interpolates on."""
    rng = np.random.default_rng(seed)
    r = np.linspace(1.01, 1.7, n_r)
    th = np.linspace(0.03, np.pi - 0.03, n_theta)
    phi = np.linspace(0.013, 2 * np.pi - 0.017, n_phi)
    assert all((a != _f32(a)).mean() > 0.8 for a in (r, th, phi))
    P, T_, R = np.meshgrid(phi, th, r, indexing='ij')
    a = rng.uniform(0.5, 1.5, 3)
    rho = 1e8 * np.exp(-(R - 1.) / 0.05) * (1.2 + 0.3 * np.sin(a[0] * P) * np.sin(T_) + 0.1 * np.cos(a[1] * T_))
    temp = 1.2 + 0.4 * (R - 1.) / 0.25 + 0.2 * np.cos(a[2] * P + T_) * np.sin(T_)
    return r, th, phi, rho, temp


SEAM_TIMES = (0., 0.25, float(np.nextafter(np.float32(0.5), np.float32(0.))), 0.5,
              float(np.nextafter(np.float32(0.5), np.float32(1.))), 0.75, float(np.nextafter(np.float32(1.), np.float32(0.))), 1.)


def seam_points():
    """``(xyz (P, 3) fp32, category [P], intended (P, 3) float64 = the (r, theta, phi) the point is meant to have, NaN where
    none is claimed)``.  Zeros are +0.  Categories: 'axis' (the six axis directions at every r node of the wide grid: a node of
    all three axes), 'r-edge' (one fp32 step inside / outside the first and last r node of both grids, on +x and -y),
    'diagonal' ((s, s, 0): phi = fl32(pi / 4), theta = fl32(pi / 2), r general), 'nan', 'origin'."""
    xyz, cat, want = [], [], []
    nan = float('nan')
    directions = (((1, 0, 0), HALF_PI32, 0.), ((-1, 0, 0), HALF_PI32, PI32), ((0, 1, 0), HALF_PI32, HALF_PI32),
                  ((0, -1, 0), HALF_PI32, THREE_HALF_PI32), ((0, 0, 1), 0., 0.), ((0, 0, -1), PI32, 0.))
    for r in SEAM_R_WIDE:
        for u, th, phi in directions:
            xyz.append([0. if c == 0 else c * r for c in u]); cat.append('axis'); want.append([r, th, phi])
    for nodes in (SEAM_R_WIDE, SEAM_R_NARROW):
        for node in (nodes[0], nodes[-1]):
            for towards in (0., 4.):
                r = float(np.nextafter(np.float32(node), np.float32(towards)))
                xyz.append([r, 0., 0.]); cat.append('r-edge'); want.append([r, HALF_PI32, 0.])
                xyz.append([0., -r, 0.]); cat.append('r-edge'); want.append([r, HALF_PI32, THREE_HALF_PI32])
    for s in (0.75, 0.875, 1.0, 1.25):
        xyz.append([s, s, 0.]); cat.append('diagonal'); want.append([nan, HALF_PI32, QUARTER_PI32])
    xyz.append([nan, 1.1, 0.]); cat.append('nan'); want.append([nan, nan, nan])
    xyz.append([0., 0., 0.]); cat.append('origin'); want.append([0., nan, 0.])
    return torch.tensor(xyz, dtype=torch.float32), cat, np.array(want, dtype=np.float64)


def seam_cases(times=SEAM_TIMES):
    """Every seam point at every seam time -> ``(points (P * T, 4) fp32, category [P * T], intended (P * T, 3))``."""
    xyz, cat, want = seam_points()
    t = torch.tensor(times, dtype=torch.float32)
    pts = torch.cat([xyz[:, None, :].expand(-1, t.numel(), -1), t[None, :, None].expand(xyz.shape[0], -1, 1)], -1).reshape(-1, 4)
    return pts.contiguous(), [c for c in cat for _ in times], np.repeat(want, t.numel(), 0)


def qualifying(coords, intended):
    """Points whose reference fp32 (r, theta, phi) equal the intended values bit for bit, wherever one is claimed."""
    got = np.stack([c.numpy().astype(np.float64) for c in coords], -1)
    return ((got == intended) | np.isnan(intended)).all(1)
