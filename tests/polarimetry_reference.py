"""NumPy fp64 restatement of include/sunerf_hip_polarimetry.h, operation for operation in the header's order, and of
``sunerf_hip.polarimetry.polarise``.  NumPy rounds every fp64 operation on its own, as the kernels do (-ffp-contract=off), so what
is built from ``+ - * /`` alone agrees with the device by value; ``sqrt`` is correctly rounded on both sides; ``log1p`` is the one
library function, and its few-ulp freedom is what ``E_F`` below accounts for.

    python tests/polarimetry_reference.py          # prints the measurement behind E_F
"""
import numpy as np

DETERMINED, UNDETERMINED, CENTRE = 0, 1, 2
OK, ABOVE, BELOW, CLOSE, DEGENERATE, INVALID = 0, 1, 2, 3, 4, 5
MIN_FRAMES, MAX_FRAMES = 3, 8
MIN_IMPACT = 1.25
STEPS = 64
EPS = 2.0 ** -40

# The lattice of the ratio_depth round trip (tests/test_gpu_polarimetry.py): impact parameter in solar radii, distance from the
# closest-approach point in impact parameters, limb darkening, solar radius in model units, |d|.
LATTICE_B = (1.26, 1.5, 2.0, 4.0, 10.0, 30.0, 215.0)
LATTICE_X = (0.1, 0.5, 1.0, 3.0)
LATTICE_U = (0.0, 0.63, 1.0)
LATTICE_R = (1.0, 0.25)
LATTICE_L = (1.0, 0.5)

# The largest |f_fp64 - f_longdouble| over LATTICE_B x LATTICE_X x LATTICE_U x LATTICE_R, from `measure_f_error()` below
# (`python tests/polarimetry_reference.py` printed 1.647e-11 at R = 1, u = 1, b = 215 R, x = 0.5 b, where B and D cancel to
# s^2 = 2e-5 of their terms; rounded up).  The GPU test allows 4 E_F: the device's log1p, divide and sqrt may differ from the
# host's by a few ulp each.
E_F = 1.7e-11


# ---- polarise: the forward model -----------------------------------------------------------------------------------------------------
def design(angles, throughput=None, efficiency=None):
    angles = np.atleast_1d(np.asarray(angles, dtype=np.float64))
    n = angles.shape[0]
    thr = np.broadcast_to(np.asarray(1.0 if throughput is None else throughput, dtype=np.float64), (n,)).copy()
    eff = np.broadcast_to(np.asarray(1.0 if efficiency is None else efficiency, dtype=np.float64), (n,)).copy()
    return np.cos(2.0 * angles), np.sin(2.0 * angles), thr, eff


def rows(cos2, sin2, throughput, efficiency):
    """The design rows as the entry point forms them on the host."""
    g0 = 0.5 * np.asarray(throughput, dtype=np.float64)
    h = g0 * np.asarray(efficiency, dtype=np.float64)
    return np.stack([g0, h * np.asarray(cos2, dtype=np.float64), h * np.asarray(sin2, dtype=np.float64)], axis=1)


def rotation(height, width, cy, cx):
    dy = (np.arange(height, dtype=np.float64) - cy)[:, None]
    dx = (np.arange(width, dtype=np.float64) - cx)[None, :]
    with np.errstate(all='ignore'):
        n = dx * dx + dy * dy
        return (dx * dx - dy * dy) / n, (2.0 * (dx * dy)) / n


def polarise(tb, pb, angles, center, throughput=None, efficiency=None):
    """``tb``, ``pb`` [..., H, W] fp64 -> frames [N, ..., H, W] fp64: y_k = (t_k / 2) (I + e_k (Q cos2_k + U sin2_k)), Q = -pb C2,
    U = -pb S2, the pixel on the centre unpolarised."""
    cos2, sin2, thr, eff = design(angles, throughput, efficiency)
    tb, pb = np.asarray(tb, dtype=np.float64), np.asarray(pb, dtype=np.float64)
    c2, s2 = (np.nan_to_num(v, nan=0.0) for v in rotation(tb.shape[-2], tb.shape[-1], *center))
    q, u = -(pb * c2), -(pb * s2)
    return np.stack([(0.5 * t) * (tb + e * (q * c + u * s)) for c, s, t, e in zip(cos2, sin2, thr, eff)])


# ---- stokes ----------------------------------------------------------------------------------------------------------------------------
def stokes(frames, cos2, sin2, throughput, efficiency, cy, cx, bad=None, a=None, b=None, rounded=True):
    """``frames`` [N, C, H, W] float32 (or float64 for the fp64 round trip: ``rounded=False`` keeps every output in fp64).
    Returns the dict of the kernel's outputs."""
    frames = np.asarray(frames)
    n, c, h, w = frames.shape
    g = rows(cos2, sin2, throughput, efficiency)
    model = a is not None
    y_all = frames.astype(np.float64)
    z = np.zeros((c, h, w))
    m00, m01, m02, m11, m12, m22, r0, r1, r2 = (z.copy() for _ in range(9))
    n_valid = np.zeros((c, h, w), dtype=np.int64)
    valid_k, w_k = [], []
    with np.errstate(all='ignore'):
        for k in range(n):
            y = y_all[k]
            valid = np.isfinite(y)
            if bad is not None:
                valid &= np.asarray(bad)[k] == 0
            wk = np.ones((c, h, w))
            if model:
                var = np.asarray(a, dtype=np.float64)[:, None, None] + np.asarray(b, dtype=np.float64)[:, None, None] * np.where(y > 0.0, y, 0.0)
                valid &= (var > 0.0) & (var < np.inf)
                wk = 1.0 / var
            p0, p1, p2 = wk * g[k, 0], wk * g[k, 1], wk * g[k, 2]
            m00 = np.where(valid, m00 + p0 * g[k, 0], m00); m01 = np.where(valid, m01 + p0 * g[k, 1], m01)
            m02 = np.where(valid, m02 + p0 * g[k, 2], m02); m11 = np.where(valid, m11 + p1 * g[k, 1], m11)
            m12 = np.where(valid, m12 + p1 * g[k, 2], m12); m22 = np.where(valid, m22 + p2 * g[k, 2], m22)
            r0 = np.where(valid, r0 + p0 * y, r0); r1 = np.where(valid, r1 + p1 * y, r1); r2 = np.where(valid, r2 + p2 * y, r2)
            n_valid += valid
            valid_k.append(valid); w_k.append(wk)
        d0 = m00
        l10, l20 = m01 / d0, m02 / d0
        d1 = m11 - l10 * m01
        t21 = m12 - l20 * m01
        l21 = t21 / d1
        d2 = (m22 - l20 * m02) - l21 * t21
        solved = (n_valid >= MIN_FRAMES) & (d0 > EPS * m00) & (d1 > EPS * m11) & (d2 > EPS * m22)
        z0, z1 = r0, r1 - l10 * r0
        z2 = (r2 - l20 * z0) - l21 * z1
        U = z2 / d2
        Q = z1 / d1 - l21 * U
        I = (z0 / d0 - l10 * Q) - l20 * U
        chi = np.zeros((c, h, w))
        for k in range(n):
            e = y_all[k] - ((g[k, 0] * I + g[k, 1] * Q) + g[k, 2] * U)
            chi = np.where(valid_k[k], chi + (w_k[k] * e) * e, chi)
        C2, S2 = rotation(h, w, cy, cx)
        centre = np.broadcast_to(np.isnan(C2), (c, h, w))
        pb = -(Q * C2 + U * S2)
        cross = Q * S2 - U * C2
        gg = l10 * l21 - l20
        c22, c12, c11 = 1.0 / d2, -l21 / d2, 1.0 / d1 + (l21 * l21) / d2
        c00 = (1.0 / d0 + (l10 * l10) / d1) + (gg * gg) / d2
        s_tb = np.sqrt(c00)
        s_pb = np.sqrt((c11 * (C2 * C2) + 2.0 * (c12 * (C2 * S2))) + c22 * (S2 * S2))
    rot = solved & ~centre
    nan = np.nan
    out = {'stokes': np.where(solved[None], np.stack([I, Q, U]), nan), 'tb': np.where(solved, I, nan), 'pb': np.where(rot, pb, nan),
           'pb_cross': np.where(rot, cross, nan), 'chi2': np.where(solved, chi, nan),
           'sigma_tb': np.where(solved & model, s_tb, nan), 'sigma_pb': np.where(rot & model, s_pb, nan)}
    if rounded:
        out = {k: v.astype(np.float32) for k, v in out.items()}
    status = np.where(~solved, UNDETERMINED, np.where(centre, CENTRE, DETERMINED)).astype(np.uint8)
    out['status'] = status
    out['counts'] = np.stack([(status == DETERMINED).sum(axis=(1, 2)), (status == UNDETERMINED).sum(axis=(1, 2)),
                              (status == CENTRE).sum(axis=(1, 2)), (n_valid < n).sum(axis=(1, 2))], axis=1).astype(np.int64)
    return out


# ---- the single-electron ratio ---------------------------------------------------------------------------------------------------------
def intensity(r2, r, R, u, p2):
    """csrc/thomson_math.h in the dtype of its arguments (fp64, or numpy.longdouble for the measurement of E_F): (I_tot, I_P)."""
    s = R / r
    s2 = s * s
    c2 = (r2 - R * R) / r2
    c = np.sqrt(c2)
    L = 0.5 * np.log1p(2.0 * s / (1.0 - s))
    k = c2 * r / R * L
    A = c * s2
    B = -0.125 * ((1.0 - 3.0 * s2) - k * (1.0 + 3.0 * s2))
    Cc = s2 / (1.0 + c) * (4.0 + c + c2) / 3.0
    D = 0.125 * ((5.0 + s2) - k * (5.0 - s2))
    sin2chi = p2 / r2
    it = (1.0 - u) * Cc + u * D
    ip = sin2chi * ((1.0 - u) * A + u * B)
    return 2.0 * it - ip, ip


def ratio(x, b2, R, u):
    """f(x) = I_P / I_tot of one electron at the distance x from the closest-approach point of a line of sight with squared
    impact parameter b2."""
    r2 = b2 + x * x
    itot, ip = intensity(r2, np.sqrt(r2), R, u, b2)
    return ip / itot


def ray_geometry(rays_o, rays_d, dtype=np.float64):
    """``(l2, l, z0, b2, b)`` of fp32 rays in ``dtype``, in the header's order."""
    o, d = np.asarray(rays_o).astype(dtype), np.asarray(rays_d).astype(dtype)
    ox, oy, oz, dx, dy, dz = o[:, 0], o[:, 1], o[:, 2], d[:, 0], d[:, 1], d[:, 2]
    with np.errstate(all='ignore'):
        l2 = (dx * dx + dy * dy) + dz * dz
        l = np.sqrt(l2)
        z0 = -((ox * dx + oy * dy) + oz * dz) / l2
        cx, cy, cz = oy * dz - oz * dy, oz * dx - ox * dz, ox * dy - oy * dx
        b2 = ((cx * cx + cy * cy) + cz * cz) / l2
        return l2, l, z0, b2, np.sqrt(b2)


def ratio_depth(tb, pb, rays_o, rays_d, solar_radius, limb_darkening_coeff, x_max_factor=64.0, rounded=True):
    """The kernel per ray, vectorised: dict of depth, z_front, z_back, radius, slope (fp32, or fp64 without ``rounded``), status."""
    tb, pb = np.asarray(tb, dtype=np.float32).astype(np.float64), np.asarray(pb, dtype=np.float32).astype(np.float64)
    R, u = float(np.float32(solar_radius)), float(np.float32(limb_darkening_coeff))
    l2, l, z0, b2, b = ray_geometry(np.asarray(rays_o, dtype=np.float32), np.asarray(rays_d, dtype=np.float32))
    n = tb.shape[0]
    status = np.full(n, OK, dtype=np.uint8)
    with np.errstate(all='ignore'):
        invalid = ~np.isfinite(tb) | ~np.isfinite(pb) | ~(tb > 0.0)
        degenerate = ~(l2 > 0.0) | ~(l2 < np.inf) | ~np.isfinite(z0) | ~(b2 < np.inf)
        close = ~(b >= MIN_IMPACT * R) | (not R > 0.0)
        status[close] = CLOSE
        status[degenerate] = DEGENERATE
        status[invalid] = INVALID
        run = status == OK
        bb2 = np.where(run, b2, (2.0 * R) ** 2)          # (a stand-in where nothing is inverted: keeps the arithmetic quiet)
        bb = np.where(run, b, 2.0 * R)
        q = np.where(run, pb / tb, 0.0)
        x_max = x_max_factor * bb
        above = run & (q > ratio(np.zeros(n), bb2, R, u))
        below = run & ~above & (q < ratio(x_max, bb2, R, u))
        lo, hi = np.zeros(n), x_max.copy()
        for _ in range(STEPS):
            m = 0.5 * (lo + hi)
            up = ratio(m, bb2, R, u) > q
            lo, hi = np.where(up, m, lo), np.where(up, hi, m)
        x = np.where(above, 0.0, np.where(below, x_max, 0.5 * (lo + hi)))
        status[above] = ABOVE
        status[below] = BELOW
        h = bb / 4096.0
        one_sided = x < h
        f1 = ratio(x + h, bb2, R, u)
        f0 = ratio(np.where(one_sided, x, x - h), bb2, R, u)
        slope = np.where(one_sided, (f1 - f0) / h, (f1 - f0) / (2.0 * h))
        out = {'depth': x, 'z_front': z0 - x / l, 'z_back': z0 + x / l, 'radius': np.sqrt(bb2 + x * x), 'slope': slope}
    out = {k: np.where(run, v, np.nan) for k, v in out.items()}
    if rounded:
        out = {k: v.astype(np.float32) for k, v in out.items()}
    out['status'] = status
    return out


def measure_f_error():
    """max |f_fp64 - f_longdouble| over the lattice, with where it is attained."""
    ld = np.longdouble
    worst = (0.0, None)
    for R in LATTICE_R:
        for u in LATTICE_U:
            for b in LATTICE_B:
                for xb in LATTICE_X:
                    bb, x = np.float64(b * R), np.float64(xb * b * R)
                    f64 = ratio(x, bb * bb, np.float64(R), np.float64(u))
                    f80 = ratio(ld(x), ld(bb) * ld(bb), ld(R), ld(u))
                    err = float(abs(ld(f64) - f80))
                    if err > worst[0]:
                        worst = (err, (R, u, b, xb))
    return worst


if __name__ == '__main__':
    err, at = measure_f_error()
    print(f'longdouble has {np.finfo(np.longdouble).nmant} mantissa bits; max |f_fp64 - f_longdouble| = {err:.3e} at (R, u, b / R, x / b) = {at}')
