"""Numpy restatement of the reprojection baseline (``csrc/reprojection.hip``, ``include/sunerf_hip.h``), written
from the formulas of the header: the axis coordinate, the bilinear sample, the projection of a map pixel into a view, the
projection of an observer's pixel onto the map, the coadd and the fill.  Geometry runs in ``dtype`` (``np.float64``, or
``np.longdouble`` to measure the fp64 restatement's own rounding noise).  numpy only; not a test module.

A view is a dict: ``planes`` (C_present, H f, W f) fp32, ``wavelengths`` (C,) with 0 for absent channels, ``downscale`` f,
``tx`` (W,) / ``ty`` (H,) fp64 axes of the reduced grid, ``c2w`` (3, 4) fp32.  An observer is a dict ``tx``, ``ty``, ``c2w``."""
import numpy as np

from observations_reference import block_mean

LONG_DOUBLE_IS_WIDER = np.finfo(np.longdouble).eps < np.finfo(np.float64).eps


def axis_coord(axis, t, dtype=np.float64):
    """Fractional pixel coordinate of the angles ``t`` on a monotone axis of pixel centres: the interval by search, linear
    inside it, the end intervals extrapolated outside the axis.  An axis of one pixel: 0 at its own angle, NaN elsewhere."""
    axis = np.asarray(axis, dtype=np.float64)
    t = np.asarray(t, dtype=dtype)
    n = axis.shape[0]
    if n == 1:
        return np.where(t == axis[0], dtype(0), dtype(np.nan))
    if axis[-1] > axis[0]:
        lo = np.searchsorted(axis, t.astype(np.float64), side='right') - 1          # last k with axis[k] <= t
    else:
        lo = np.searchsorted(-axis, -t.astype(np.float64), side='right') - 1
    lo = np.clip(lo, 0, n - 2)
    lo = np.where(np.isnan(t), 0, lo)
    a0, a1 = axis[lo].astype(dtype), axis[lo + 1].astype(dtype)
    return lo.astype(dtype) + (t - a0) / (a1 - a0)


def bilinear(plane, y, x, with_taps=False):
    """``scipy.ndimage.map_coordinates(plane, [y, x], order=1, mode='constant', cval=nan)``: NaN outside
    [0, n_y - 1] x [0, n_x - 1]; inside the four-term weighted sum in fp64 of the fp32 taps, i1 = min(i0 + 1, n - 1)."""
    plane = np.asarray(plane, dtype=np.float32)
    ny, nx = plane.shape
    y, x = np.asarray(y, dtype=np.float64), np.asarray(x, dtype=np.float64)
    with np.errstate(invalid='ignore'):
        inside = (y >= 0) & (y <= ny - 1) & (x >= 0) & (x <= nx - 1)
    ys, xs = np.where(inside, y, 0.), np.where(inside, x, 0.)
    fy, fx = np.floor(ys), np.floor(xs)
    y0, x0 = fy.astype(np.int64), fx.astype(np.int64)
    y1, x1 = np.minimum(y0 + 1, ny - 1), np.minimum(x0 + 1, nx - 1)
    wy, wx = ys - fy, xs - fx
    taps = np.stack([plane[y0, x0], plane[y0, x1], plane[y1, x0], plane[y1, x1]]).astype(np.float64)
    with np.errstate(invalid='ignore', over='ignore'):
        value = (((1. - wy) * (1. - wx) * taps[0] + (1. - wy) * wx * taps[1]) + wy * (1. - wx) * taps[2]) + wy * wx * taps[3]
    value = np.where(inside, value, np.nan)
    return (value, taps, inside) if with_taps else value


def column_points(lat, lon, radius, dtype=np.float64):
    """p = radius * u(lat, lon) for the grid of two axes -> (n_lat, n_lon, 3)."""
    b, l = np.asarray(lat, dtype=dtype)[:, None], np.asarray(lon, dtype=dtype)[None, :]
    cb = np.cos(b)
    return dtype(radius) * np.stack(np.broadcast_arrays(-cb * np.sin(l), cb * np.cos(l), -np.sin(b)), -1)


def pixel_directions(tx, ty, c2w, dtype=np.float64):
    """World direction of every pixel of the axes' grid -> (H, W, 3): c2w[:3,:3] (sin Tx, -sin Ty cos Tx, -cos Tx cos Ty)."""
    Tx, Ty = np.asarray(tx, dtype=dtype)[None, :], np.asarray(ty, dtype=dtype)[:, None]
    cam = np.stack(np.broadcast_arrays(np.sin(Tx), -np.sin(Ty) * np.cos(Tx), -np.cos(Tx) * np.cos(Ty)), -1)
    rot = np.asarray(c2w, dtype=np.float32)[:3, :3].astype(dtype)
    return np.stack([(rot[r, 0] * cam[..., 0] + rot[r, 1] * cam[..., 1]) + rot[r, 2] * cam[..., 2] for r in range(3)], -1)


def view_coords(view, points, radius, dtype=np.float64):
    """(x, y, margin) of surface points (..., 3) in a view: the inverse of :func:`pixel_directions` on the view's axes and
    ``p . o - radius^2`` (> 0: the point is the near intersection of its own line of sight)."""
    c2w = np.asarray(view['c2w'], dtype=np.float32)[:3, :4].astype(dtype)
    o = c2w[:, 3]
    p = np.asarray(points, dtype=dtype)
    q = p - o
    margin = ((p[..., 0] * o[0] + p[..., 1] * o[1]) + p[..., 2] * o[2]) - dtype(radius) * dtype(radius)
    a, b, c = c2w[0, :3], c2w[1, :3], c2w[2, :3]            # c2w[:3,:3]^-1 by cofactors (the fp32 pose is orthonormal to 1e-7 only)
    cross = lambda u, v: [u[1] * v[2] - u[2] * v[1], u[2] * v[0] - u[0] * v[2], u[0] * v[1] - u[1] * v[0]]      # noqa: E731
    bc, ca, ab = cross(b, c), cross(c, a), cross(a, b)
    det = (a[0] * bc[0] + a[1] * bc[1]) + a[2] * bc[2]
    cam = [((bc[i] * q[..., 0] + ca[i] * q[..., 1]) + ab[i] * q[..., 2]) / det for i in range(3)]
    Tx = np.arctan2(cam[0], np.hypot(cam[1], cam[2]))
    Ty = np.arctan2(-cam[1], -cam[2])
    return axis_coord(view['tx'], Tx, dtype), axis_coord(view['ty'], Ty, dtype), margin


def reduced_planes(view):
    """Per output channel the (H, W) fp32 plane after the downscale, or None for a channel the view lacks."""
    wl = np.asarray(view['wavelengths'], dtype=np.float32).reshape(-1)
    out, k = [], 0
    for c in range(wl.size):
        if wl[c] != 0:
            out.append(block_mean(view['planes'][k], view['downscale']))
            k += 1
        else:
            out.append(None)
    assert k == len(view['planes'])
    return out


def synchronic_map(views, lat, lon, radius):
    """The coadd.  Returns a dict: ``map`` (C, n_lat, n_lon) fp32 with NaN where nothing covers, ``footprint`` int32, and for
    the value bound ``tap_max`` = max |tap|, ``tap_lo`` / ``tap_hi`` = min / max tap over the taps of all covering views."""
    points = column_points(lat, lon, radius)
    n_c = np.asarray(views[0]['wavelengths']).reshape(-1).size
    shape = (n_c,) + points.shape[:2]
    total, count = np.zeros(shape), np.zeros(shape, dtype=np.int32)
    tap_max, tap_lo, tap_hi = np.zeros(shape), np.full(shape, np.inf), np.full(shape, -np.inf)
    for view in views:
        x, y, margin = view_coords(view, points, radius)
        for c, plane in enumerate(reduced_planes(view)):
            if plane is None:
                continue
            value, taps, inside = bilinear(plane, y, x, with_taps=True)
            covers = (margin > 0) & ~np.isnan(value)
            with np.errstate(invalid='ignore'):
                total[c] = np.where(covers, total[c] + np.where(covers, value, 0.), total[c])
            count[c] += covers
            tap_max[c] = np.where(covers, np.maximum(tap_max[c], np.abs(taps).max(0)), tap_max[c])
            tap_lo[c] = np.where(covers, np.minimum(tap_lo[c], taps.min(0)), tap_lo[c])
            tap_hi[c] = np.where(covers, np.maximum(tap_hi[c], taps.max(0)), tap_hi[c])
    with np.errstate(invalid='ignore', divide='ignore'):
        image = np.where(count > 0, total / count, np.nan).astype(np.float32)
    return {'map': image, 'footprint': count, 'tap_max': tap_max, 'tap_lo': tap_lo, 'tap_hi': tap_hi}


def fill(image, fill='mean'):
    """``nan_to_num(image, nan=nanmean(image))`` per channel of (C, ...) fp32.  Returns (filled, mean per channel fp64, number
    of non-NaN pixels per channel).  ``fill``: 'mean', None (NaNs stay) or a number."""
    image = np.asarray(image, dtype=np.float32)
    flat = image.reshape(image.shape[0], -1)
    valid = ~np.isnan(flat)
    count = valid.sum(1)
    with np.errstate(invalid='ignore', divide='ignore', over='ignore'):
        mean = np.where(valid, flat.astype(np.float64), 0.).sum(1) / count
    mean = np.where(count > 0, mean, np.nan)
    out = image.copy()
    if fill is not None:
        for c in range(image.shape[0]):
            value = np.float32(mean[c]) if isinstance(fill, str) else np.float32(fill)
            out[c][np.isnan(image[c])] = value
    return out, mean, count


def surface_points(observer, radius, dtype=np.float64):
    """Near intersection of every pixel's line of sight with the sphere: (p as three (H, W) arrays, m / radius^2, on_disk)
    with c = o x d, m = radius^2 - |c|^2, on the disk iff m > 0 and o . d < 0, p = o + d (-(o . d) - sqrt(m))."""
    c2w = np.asarray(observer['c2w'], dtype=np.float32)[:3, :4].astype(dtype)
    o = c2w[:, 3]
    d = pixel_directions(observer['tx'], observer['ty'], c2w, dtype)
    c0 = o[1] * d[..., 2] - o[2] * d[..., 1]
    c1 = o[2] * d[..., 0] - o[0] * d[..., 2]
    c2 = o[0] * d[..., 1] - o[1] * d[..., 0]
    r2 = dtype(radius) * dtype(radius)
    m = r2 - ((c0 * c0 + c1 * c1) + c2 * c2)
    od = (o[0] * d[..., 0] + o[1] * d[..., 1]) + o[2] * d[..., 2]
    on_disk = (m > 0) & (od < 0)
    with np.errstate(invalid='ignore'):
        s = -od - np.sqrt(np.where(on_disk, m, 0))
    return [o[k] + d[..., k] * s for k in range(3)], m / r2, on_disk


def observer_coords(observer, lat, lon, radius, dtype=np.float64):
    """(x on the longitude axis, y on the latitude axis, m / radius^2, on_disk) for every pixel (H, W) of an observer."""
    p, mrel, on_disk = surface_points(observer, radius, dtype)
    b = np.arctan2(-p[2], np.hypot(p[0], p[1]))
    l = np.arctan2(-p[0], p[1])
    two_pi = dtype(2) * np.arctan2(dtype(0), dtype(-1))          # fp64: the kernel's constant 2 pi
    l0 = dtype(np.asarray(lon, dtype=np.float64)[0])
    l = l - two_pi * np.floor((l - l0) / two_pi)
    l = np.where(l < l0, l + two_pi, l)
    l = np.where(l >= l0 + two_pi, l - two_pi, l)
    x = np.where(on_disk, axis_coord(lon, l, dtype), dtype(np.nan))
    y = np.where(on_disk, axis_coord(lat, b, dtype), dtype(np.nan))
    return x, y, mrel, on_disk


def reproject(image, lat, lon, radius, observer, off_disk=np.nan):
    """The map (C, n_lat, n_lon) fp32 seen by one observer.  Returns a dict: ``image`` (H, W, C) fp32 (NaN outside the map's
    axes, ``off_disk`` off the disk), ``on_disk`` (H, W), and ``tap_max`` / ``tap_lo`` / ``tap_hi`` (H, W, C) as above."""
    image = np.asarray(image, dtype=np.float32)
    x, y, _, on_disk = observer_coords(observer, lat, lon, radius)
    x, y = x.astype(np.float64), y.astype(np.float64)
    out, tmax, tlo, thi = [], [], [], []
    for plane in image:
        value, taps, inside = bilinear(plane, y, x, with_taps=True)
        out.append(np.where(on_disk, value, off_disk).astype(np.float32))
        tmax.append(np.abs(taps).max(0)), tlo.append(taps.min(0)), thi.append(taps.max(0))
    return {'image': np.stack(out, -1), 'on_disk': on_disk, 'tap_max': np.stack(tmax, -1), 'tap_lo': np.stack(tlo, -1),
            'tap_hi': np.stack(thi, -1)}


# ------------------------------------------------------------------------------------------------- decision margins
def nan_undecided(plane, y, x, eps=1e-9):
    """Samples whose coordinate lies within ``eps`` of an integer AND whose two candidate cells differ in whether the result
    is NaN: the coverage decision there depends on the coordinate's last bits."""
    y, x = np.asarray(y, dtype=np.float64), np.asarray(x, dtype=np.float64)
    ny, nx = plane.shape
    with np.errstate(invalid='ignore'):
        near = ((np.abs(y - np.rint(y)) <= eps) | (np.abs(x - np.rint(x)) <= eps)) & (y >= 0) & (y <= ny - 1) & (x >= 0) & (x <= nx - 1)
    if not near.any():
        return near
    yy, xx = y[near], x[near]
    nan = []
    for dy in (-2 * eps, 2 * eps):
        for dx in (-2 * eps, 2 * eps):
            nan.append(np.isnan(bilinear(plane, np.clip(yy + dy, 0, ny - 1), np.clip(xx + dx, 0, nx - 1))))
    out = np.zeros(near.shape, dtype=bool)
    nan.append(np.isnan(bilinear(plane, yy, xx)))
    out[near] = np.any(nan, 0) != np.all(nan, 0)
    return out


def edge_distance(coord, n):
    """Distance [pixels] of finite coordinates to the nearer end of an axis of ``n`` pixels (inf for NaN)."""
    coord = np.asarray(coord, dtype=np.float64)
    with np.errstate(invalid='ignore'):
        d = np.minimum(np.abs(coord), np.abs(coord - (n - 1)))
    return np.where(np.isnan(coord), np.inf, d)


def view_margins(view, lat, lon, radius, eps=1e-9):
    """Undecided map pixels of one view (bool (n_lat, n_lon)) under the three rules: visibility ``|p . o - R^2| <= eps R |o|``,
    a coordinate within ``eps`` pixels of a hull edge (views of at least 2 x 2 pixels), a NaN-deciding cell boundary; and the
    minima (visibility margin / (R |o|), edge distance) for the record."""
    points = column_points(lat, lon, radius)
    x, y, margin = view_coords(view, points, radius)
    o = np.asarray(view['c2w'], dtype=np.float64)[:3, 3]
    rel = np.abs(margin) / (radius * np.linalg.norm(o))
    undecided = rel <= eps
    n_y, n_x = len(view['ty']), len(view['tx'])
    edge = np.inf
    if n_y >= 2 and n_x >= 2:
        ex, ey = edge_distance(x, n_x), edge_distance(y, n_y)
        # an edge matters where the other coordinate is inside (or as close to its own edge)
        with np.errstate(invalid='ignore'):
            in_x, in_y = (x >= -eps) & (x <= n_x - 1 + eps), (y >= -eps) & (y <= n_y - 1 + eps)
        ex, ey = np.where(in_y, ex, np.inf), np.where(in_x, ey, np.inf)
        undecided |= (ex <= eps) | (ey <= eps)
        edge = min(ex.min(), ey.min())
    for plane in reduced_planes(view):
        if plane is not None and not np.isfinite(plane).all():
            undecided |= nan_undecided(plane, y, x, eps)
    return undecided, float(rel.min()), float(edge)


def observer_margins(observer, image, lat, lon, radius, eps=1e-9):
    """Undecided pixels of one observer (bool (H, W)): ``|1 - |c|^2 / R^2| <= eps``, a map coordinate within ``eps`` of a hull
    edge (maps of at least 2 x 2 pixels), a NaN-deciding cell boundary of the map; and the two minima."""
    x, y, mrel, on_disk = observer_coords(observer, lat, lon, radius)
    undecided = np.abs(mrel) <= eps
    edge = np.inf
    if len(lat) >= 2 and len(lon) >= 2:
        ex, ey = edge_distance(x, len(lon)), edge_distance(y, len(lat))
        with np.errstate(invalid='ignore'):
            in_x, in_y = (x >= -eps) & (x <= len(lon) - 1 + eps), (y >= -eps) & (y <= len(lat) - 1 + eps)
        ex, ey = np.where(in_y, ex, np.inf), np.where(in_x, ey, np.inf)
        undecided |= (ex <= eps) | (ey <= eps)
        edge = min(ex.min(), ey.min())
    for plane in np.asarray(image, dtype=np.float32):
        if not np.isfinite(plane).all():
            undecided |= nan_undecided(plane, y, x, eps)
    return undecided, float(np.abs(mrel).min()), float(edge)


def coordinate_noise(fp64, wide):
    """max |fp64 - long double| over the positions where both are finite (the restatement's own rounding noise)."""
    a, b = np.asarray(fp64, dtype=np.longdouble), np.asarray(wide, dtype=np.longdouble)
    both = np.isfinite(a) & np.isfinite(b)
    return float(np.abs(a - b)[both].max()) if both.any() else 0.0


def coordinate_bound(noise, n_x, n_y):
    """The GPU tests' coordinate bound: 8 x the restatement's own fp64-vs-long-double noise (the device's fp64 sin / cos / atan2 /
    sqrt are allowed a few ulp where numpy's stay under one, four calls deep), floored at 64 x 2^-52 x max(n_x, n_y)."""
    return max(8.0 * noise, 64 * 2.0 ** -52 * max(n_x, n_y))


# ------------------------------------------------------------------------------------------------------ test inputs
WL7 = [94., 131., 171., 193., 211., 304., 335.]
MAPS = {'full': dict(shape=(91, 181), lat_range=(-np.pi / 2, np.pi / 2), lon_range=(-np.pi, np.pi)),
        'strip': dict(shape=(7, 4099), lat_range=(-0.3, 0.4), lon_range=(-2.0, 2.5))}


def view_specs():
    """Six views of one 7-channel set, of the kind tests/test_gpu_observations.py uses: an odd size, a 1 x 1 view, a downscale-2
    view with an off-centre grid, a 3-of-7-channel view on non-uniform axes (one of them descending) with a shifted centre, a
    view with NaN / Inf pixels, a downscale-3 view with a non-finite block.  Poses: 100 to 215 solar radii."""
    rng = np.random.default_rng(5)

    def planes(c, h, w):
        return (rng.uniform(0.0, 2.0, size=(c, h, w)) * 10.0 ** rng.integers(-3, 4, size=(c, h, w))).astype(np.float32)
    views = []
    views.append(dict(planes=planes(7, 37, 53), wavelengths=WL7, downscale=1, lat=0.1, lon=0.3, distance=215.0,
                      grid={'shape': (37, 53), 'cdelt': (60., 80.)}))
    views.append(dict(planes=planes(1, 1, 1), wavelengths=[0, 0, 171., 0, 0, 0, 0], downscale=1, lat=-0.2, lon=1.3,
                      distance=200.0, grid={'shape': (1, 1), 'cdelt': (2400., 2400.)}))
    views.append(dict(planes=planes(7, 24, 40), wavelengths=WL7, downscale=2, lat=0.0, lon=2.0, distance=215.0,
                      grid={'shape': (24, 40), 'cdelt': (100., 100.), 'crpix': (19.0, 11.5), 'crval': (30., -20.)}))
    s = np.linspace(0., 1., 9)
    t = np.linspace(0., 1., 16)
    views.append(dict(planes=planes(3, 16, 9), wavelengths=[0, 131., 0, 193., 211., 0, 0], downscale=1, lat=0.3, lon=-0.8,
                      distance=150.0, tx=-6.1e-3 + 1.3e-2 * (0.7 * s + 0.3 * s * s), ty=7.3e-3 - 1.4e-2 * (0.8 * t + 0.2 * t ** 3),
                      center=(0.01, -0.02, 0.03)))
    nan_planes = planes(2, 20, 31)
    nan_planes[0, 3, 4] = np.nan
    nan_planes[1, 3, 4] = np.nan
    nan_planes[1, 19, 30] = np.nan
    nan_planes[0, 0, 0] = np.inf
    nan_planes[1, 7, 7] = -np.inf
    views.append(dict(planes=nan_planes, wavelengths=[94., 0, 0, 0, 0, 0, 335.], downscale=1, lat=-0.1, lon=3.0, distance=215.0,
                      grid={'shape': (20, 31), 'cdelt': (110., 110.)}))
    block = planes(7, 9, 12)
    block[2, 4, 7] = np.nan                                        # inside block (1, 2) of the 3 x 4 reduced frame
    views.append(dict(planes=block, wavelengths=WL7, downscale=3, lat=0.2, lon=-2.0, distance=100.0,
                      grid={'shape': (9, 12), 'cdelt': (200., 200.)}))
    return views


def observer_specs():
    """Named observers: 64 x 64, 37 x 53 (shifted centre), 1 x 1, and ``grid``: the 19 x 37 observers of a 10-degree grid on
    16 x 16 pixels each (the batch)."""
    fov = 2400. * np.pi / 180. / 3600.
    axis16 = np.linspace(-fov / 2, fov / 2, 16)
    out = {'square': [dict(lat=0.15, lon=0.9, distance=215.0, tx=np.linspace(-fov / 2, fov / 2, 64), ty=np.linspace(-fov / 2, fov / 2, 64))],
           'odd': [dict(lat=-0.4, lon=-2.2, distance=100.0, center=(0.02, 0.01, -0.03),
                        tx=np.linspace(-1.1e-2, 1.2e-2, 53), ty=np.linspace(1.05e-2, -0.95e-2, 37))],
           'single': [dict(lat=0.05, lon=2.9, distance=160.0, tx=np.array([1.1e-4]), ty=np.array([-2.3e-4]))]}
    coords = np.stack(np.mgrid[-90:91:10, :361:10], -1).astype(np.float32).reshape((-1, 2))
    out['grid'] = [dict(lat=float(np.deg2rad(b)), lon=float(np.deg2rad(l)), distance=215.03215567054764, tx=axis16, ty=axis16)
                   for b, l in coords]
    return out


def observation_set(specs, device):
    """The ``ObservationSet`` of ``specs`` on ``device`` and the restatement's view dicts read back from its ``View`` objects
    (axes and poses as the set computed them)."""
    import torch
    from sunerf_hip.observations import ObservationSet
    obs = ObservationSet(device=device)
    for v in specs:
        kw = {k: v[k] for k in ('grid', 'tx', 'ty', 'center') if k in v}
        obs.add_view(torch.from_numpy(v['planes']).to(device), v['lat'], v['lon'], v['distance'], v.get('time', 0.0),
                     wavelengths=v['wavelengths'], downscale=v['downscale'], **kw)
    views = [dict(planes=v['planes'], wavelengths=v['wavelengths'], downscale=v['downscale'], tx=ov.tx.cpu().numpy(),
                  ty=ov.ty.cpu().numpy(), c2w=ov.c2w[:3, :4].numpy()) for v, ov in zip(specs, obs.views)]
    return obs, views


def observer_dict(spec):
    """The restatement's observer dict of an ``Observer`` argument dict."""
    from sunerf_hip.rays import pose_spherical
    c2w = pose_spherical(-spec['lon'], spec['lat'], spec['distance'], spec.get('center'))
    return dict(tx=np.asarray(spec['tx'], dtype=np.float64), ty=np.asarray(spec['ty'], dtype=np.float64), c2w=c2w[:3, :4].numpy())


def map_axes(name):
    m = MAPS[name]
    return (np.linspace(m['lat_range'][0], m['lat_range'][1], m['shape'][0]),
            np.linspace(m['lon_range'][0], m['lon_range'][1], m['shape'][1]))


def random_case(seed):
    """One case of the randomised sweep: 1 to 3 single-channel views and one observer with shapes 1 ... 300, distances 3 ... 300
    solar radii, ``center`` shifts and ascending or descending axes, a map of random shape and ranges, a random ``Rs_per_ds``."""
    rng = np.random.default_rng(1000 + seed)

    def axis(n, half):
        a = np.linspace(-half, half, n) + rng.uniform(-0.2, 0.2) * half if n > 1 else np.array([rng.uniform(-0.1, 0.1) * half])
        return a[::-1].copy() if rng.random() < 0.3 else a

    def pose():
        d = float(np.exp(rng.uniform(np.log(3.), np.log(300.))))
        center = tuple(rng.uniform(-0.05, 0.05, 3)) if rng.random() < 0.5 else None
        half = 1.3 * np.arcsin(min(1.0, 1.0 / d)) * rng.uniform(0.5, 1.2)
        return d, center, half
    Rs_per_ds = float(rng.choice([1.0, 1.0, 0.5, 2.0]))
    views = []
    for _ in range(int(rng.integers(1, 4))):
        h, w = (int(np.exp(rng.uniform(0, np.log(300.)))) for _ in range(2))
        f = int(rng.choice([1, 1, 2]))
        d, center, half = pose()
        image = rng.uniform(0.5, 1.5, size=(1, h * f, w * f)).astype(np.float32)
        if rng.random() < 0.3:
            image[0, rng.integers(0, h * f), rng.integers(0, w * f)] = np.nan
        v = dict(planes=image, wavelengths=[193.], downscale=f, lat=float(rng.uniform(-1.2, 1.2)), lon=float(rng.uniform(-3.1, 3.1)),
                 distance=d / Rs_per_ds, tx=axis(w, half), ty=axis(h, half))
        if center is not None:
            v['center'] = tuple(c / Rs_per_ds for c in center)
        views.append(v)
    n_lat, n_lon = int(rng.integers(2, 120)), int(rng.integers(2, 300))
    lat0, lon0 = rng.uniform(-np.pi / 2, 0.), rng.uniform(-np.pi, 0.)
    full = rng.random() < 0.5
    m = dict(shape=(n_lat, n_lon), lat_range=(-np.pi / 2, np.pi / 2) if full else (lat0, lat0 + rng.uniform(0.5, 1.5)),
             lon_range=(-np.pi, np.pi) if full else (lon0, lon0 + rng.uniform(1.0, 3.0)))
    d, center, half = pose()
    h, w = (int(np.exp(rng.uniform(0, np.log(300.)))) for _ in range(2))
    observer = dict(lat=float(rng.uniform(-1.2, 1.2)), lon=float(rng.uniform(-3.1, 3.1)), distance=d / Rs_per_ds, tx=axis(w, half),
                    ty=axis(h, half))
    if center is not None:
        observer['center'] = tuple(c / Rs_per_ds for c in center)
    return dict(views=views, map=m, observer=observer, Rs_per_ds=Rs_per_ds)
