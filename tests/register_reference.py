"""NumPy fp64 restatement of the registration map (include/sunerf_hip_register.h), written from the header,
operation by operation, and the cases the host and GPU tests share.  Besides the outputs it returns every quantity a decision
hangs on -- ``m / radius^2``, the visibility dot, the distances of the coordinates from the edge rule's ends -- and the first-order
bound of the coordinates, from which the tests tell the pixels whose status rounding can flip."""
import functools
import math

import numpy as np
from scipy import ndimage

ON_DISK, OFF_DISK, BEHIND, OUTSIDE = 1, 2, 4, 8
MISSING, CLOSEST = 0, 1
PROPAGATE = 1
EDGE_EPS = 2.0 ** -20
U = 2.0 ** -53
CHAIN_OPS = 64            # rounded operations between the reference axes and a coordinate, counted generously (about 50)
DECISION_REACH = 1e-9     # of m / radius^2 and of the visibility dot / (radius |o_k|)
MAX_UNDECIDABLE = 0.02


# ---- poses ----------------------------------------------------------------------------------------------------------------------
def unit(lat, lon):
    """u(lat, lon) of the header: (-cos b sin l, cos b cos l, -sin b)."""
    return np.array([-math.cos(lat) * math.sin(lon), math.cos(lat) * math.cos(lon), -math.sin(lat)])


def look_at_pose(lat, lon, distance, roll=0.0):
    """A camera-to-world pose [3][4] in fp32 for an observer at ``distance u(lat, lon)`` looking at the centre: the camera looks
    along -z, so the third column is the unit vector from the centre to the observer; x is east, y is south (the header's
    direction ``(sin Tx, -sin Ty cos Tx, -cos Tx cos Ty)`` has Ty positive towards -y).  Independent of sunerf_hip.rays."""
    z = unit(lat, lon)
    north = np.array([0.0, 0.0, -1.0])
    x = np.cross(north, z)
    x = x / np.linalg.norm(x)
    y = np.cross(z, x)
    if roll:
        x, y = math.cos(roll) * x + math.sin(roll) * y, -math.sin(roll) * x + math.cos(roll) * y
    pose = np.stack([x, y, z, distance * z], axis=1)
    return pose.astype(np.float32)


def axes_for(shape, half_width, descending_y=False, offset=(0.0, 0.0)):
    """Linear fp64 axes of pixel centres (tx [W], ty [H]) spanning +-half_width [rad] along the longer side."""
    h, w = shape
    pitch = 2.0 * half_width / max(max(h, w) - 1, 1)
    tx = (np.arange(w) - (w - 1) / 2.0) * pitch + offset[1]
    ty = (np.arange(h) - (h - 1) / 2.0) * pitch + offset[0]
    return tx, (ty[::-1].copy() if descending_y else ty)


# ---- the map --------------------------------------------------------------------------------------------------------------------
def axis_coord(axis, t):
    """The header's ``axis``: bisection to the interval [lo, lo + 1], linear inside, the outermost interval beyond the ends."""
    axis = np.asarray(axis, dtype=np.float64)
    n = axis.shape[0]
    if n == 1:
        return np.where(t == axis[0], 0.0, np.nan)
    ascending = axis[-1] > axis[0]
    lo = np.zeros(t.shape, dtype=np.int64)
    hi = np.full(t.shape, n - 1, dtype=np.int64)
    while np.any(hi - lo > 1):
        active = hi - lo > 1
        mid = (lo + hi) >> 1
        a = axis[mid]
        left = (a <= t) if ascending else (a >= t)
        lo = np.where(active & left, mid, lo)
        hi = np.where(active & ~left, mid, hi)
    a0, a1 = axis[lo], axis[lo + 1]
    return lo + (t - a0) / (a1 - a0)


def snap_edge(v, n):
    last = float(n - 1)
    v = np.where((v < 0.0) & (v >= -EDGE_EPS), 0.0, v)
    return np.where((v > last) & (v <= last + EDGE_EPS), last, v)


def _dot(a, b):
    return (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]


def map_frame(c2w_ref, tx_ref, ty_ref, frame, radius=1.0, rates=(0.0, 0.0, 0.0), off_disk=CLOSEST):
    """Steps 1 .. 6 of the header for one frame ``{'c2w', 'tx', 'ty', 'dt', 'shift_y', 'shift_x'}``: a dict of [H, W] arrays --
    ``cy``, ``cx`` (the header's ``coords``), ``status``, ``sample``, the decision quantities ``mrel`` = m / radius^2, ``vis`` = the
    visibility dot over radius |o_k|, ``edge`` = the smallest distance of a formed coordinate from -eps and n - 1 + eps, ``bound`` =
    the first-order bound of the coordinates [pixel] and ``undecidable``."""
    with np.errstate(all='ignore'):
        c2w_ref = np.asarray(c2w_ref, dtype=np.float32).reshape(3, 4).astype(np.float64)
        c2w = np.asarray(frame['c2w'], dtype=np.float32).reshape(3, 4).astype(np.float64)
        tx_k, ty_k = np.asarray(frame['tx'], dtype=np.float64), np.asarray(frame['ty'], dtype=np.float64)
        h, w = ty_k.shape[0], tx_k.shape[0]
        A, B, C = rates
        dt = float(frame.get('dt', 0.0))
        Ty, Tx = np.meshgrid(np.asarray(ty_ref, dtype=np.float64), np.asarray(tx_ref, dtype=np.float64), indexing='ij')
        # 1
        sx, cTx, sy, cTy = np.sin(Tx), np.cos(Tx), np.sin(Ty), np.cos(Ty)
        e = (sx, -sy * cTx, -cTx * cTy)
        d = [(c2w_ref[i, 0] * e[0] + c2w_ref[i, 1] * e[1]) + c2w_ref[i, 2] * e[2] for i in range(3)]
        o = [c2w_ref[i, 3] for i in range(3)]
        v = (o[1] * d[2] - o[2] * d[1], o[2] * d[0] - o[0] * d[2], o[0] * d[1] - o[1] * d[0])
        R2 = radius * radius
        m = R2 - _dot(v, v)
        od = _dot(o, d)
        on_disk = (m > 0.0) & (od < 0.0)
        # 2
        s = np.where(on_disk, -od - np.sqrt(np.where(on_disk, m, 0.0)), -od)
        p = [o[i] + d[i] * s for i in range(3)]
        # 3
        rho = np.sqrt(_dot(p, p))
        lat = np.arctan2(-p[2], np.hypot(p[0], p[1]))
        lon = np.arctan2(-p[0], p[1])
        sl, cl = np.sin(lat), np.cos(lat)
        s2 = sl * sl
        rate = (A + B * s2) + C * (s2 * s2)
        lon_k = lon + rate * dt
        q = [rho * (-cl * np.sin(lon_k)), rho * (cl * np.cos(lon_k)), rho * (-sl)]
        # 4
        ok = [c2w[i, 3] for i in range(3)]
        margin = _dot(q, ok) - R2
        behind = on_disk & ~(margin > 0.0)
        # 5
        rel = [q[i] - ok[i] for i in range(3)]
        a_, b_, c_ = c2w[0, :3], c2w[1, :3], c2w[2, :3]
        bc = (b_[1] * c_[2] - b_[2] * c_[1], b_[2] * c_[0] - b_[0] * c_[2], b_[0] * c_[1] - b_[1] * c_[0])
        ca = (c_[1] * a_[2] - c_[2] * a_[1], c_[2] * a_[0] - c_[0] * a_[2], c_[0] * a_[1] - c_[1] * a_[0])
        ab = (a_[1] * b_[2] - a_[2] * b_[1], a_[2] * b_[0] - a_[0] * b_[2], a_[0] * b_[1] - a_[1] * b_[0])
        det = (a_[0] * bc[0] + a_[1] * bc[1]) + a_[2] * bc[2]
        cam = [((bc[i] * rel[0] + ca[i] * rel[1]) + ab[i] * rel[2]) / det for i in range(3)]
        Txk = np.arctan2(cam[0], np.hypot(cam[1], cam[2]))
        Tyk = np.arctan2(-cam[1], -cam[2])
        cx = axis_coord(tx_k, Txk) + float(frame.get('shift_x', 0.0))
        cy = axis_coord(ty_k, Tyk) + float(frame.get('shift_y', 0.0))
        # 6
        ey, ex = snap_edge(cy, h), snap_edge(cx, w)
        inside = (ey >= 0.0) & (ey <= h - 1) & (ex >= 0.0) & (ex <= w - 1)
        formed = on_disk | (off_disk == CLOSEST)
        formed = formed & ~behind
        sample = formed & inside
        status = np.where(on_disk, ON_DISK, OFF_DISK)
        status = np.where(behind, BEHIND, status)
        status = np.where(formed & ~inside, OUTSIDE, status).astype(np.uint8)
        out_cy = np.where(sample, ey, np.where(formed, cy, np.nan))
        out_cx = np.where(sample, ex, np.where(formed, cx, np.nan))
        # ---- the decision quantities and the bound
        mrel = m / R2
        norm_o, norm_ok = math.sqrt(_dot(o, o)), math.sqrt(_dot(ok, ok))
        vis = margin / (radius * norm_ok)
        root = np.where(on_disk, np.sqrt(np.abs(mrel)), 1.0)
        distance = np.sqrt(_dot(rel, rel))
        reach = norm_o * (1.0 + 1.0 / root) + norm_ok + rho * (8.0 + np.abs(rate * dt))          # [length] x U: the error of q - o_k
        pitch_y = np.abs(np.diff(ty_k)).min() if h > 1 else np.inf
        pitch_x = np.abs(np.diff(tx_k)).min() if w > 1 else np.inf
        angle = CHAIN_OPS * U * (reach / distance + 4.0)                                         # [rad]
        bound_y, bound_x = angle / pitch_y + CHAIN_OPS * U * h, angle / pitch_x + CHAIN_OPS * U * w
        bound = np.maximum(bound_y, bound_x)
        edge = np.minimum(np.minimum(np.abs(cy + EDGE_EPS), np.abs(cy - (h - 1 + EDGE_EPS))),
                          np.minimum(np.abs(cx + EDGE_EPS), np.abs(cx - (w - 1 + EDGE_EPS))))
        undecidable = np.abs(mrel) < DECISION_REACH
        undecidable |= on_disk & (np.abs(vis) < DECISION_REACH)
        near_edge = (np.abs(cy + EDGE_EPS) <= bound_y) | (np.abs(cy - (h - 1 + EDGE_EPS)) <= bound_y)
        near_edge |= (np.abs(cx + EDGE_EPS) <= bound_x) | (np.abs(cx - (w - 1 + EDGE_EPS)) <= bound_x)
        undecidable |= formed & near_edge
        if h == 1:          # one centre: the coordinate exists only where the angle equals it
            undecidable |= formed & (Tyk != ty_k[0]) & (np.abs(Tyk - ty_k[0]) < DECISION_REACH)
        if w == 1:
            undecidable |= formed & (Txk != tx_k[0]) & (np.abs(Txk - tx_k[0]) < DECISION_REACH)
    return {'cy': out_cy, 'cx': out_cx, 'status': status, 'sample': sample, 'mrel': mrel, 'vis': vis, 'edge': edge, 'bound': bound,
            'bound_y': bound_y, 'bound_x': bound_x, 'undecidable': undecidable, 'on_disk': on_disk, 'raw_cy': cy, 'raw_cx': cx}


def tap_switch(geo, order, masked=False):
    """Sampled pixels at which rounding decides the tap set (``prep_start``: ``floor(c + 1/2)`` at even orders, ``floor(c)`` at odd
    ones): a coordinate within the bound of a half at an even order -- at order 0 the value jumps there -- and, where a mask is
    propagated, within the bound of a whole number at an odd order (the value is continuous there, the taps read are not)."""
    cy, cx = np.where(geo['sample'], geo['cy'], 0.25), np.where(geo['sample'], geo['cx'], 0.25)
    near = np.zeros(cy.shape, dtype=bool)
    if order % 2 == 0:
        near |= (np.abs(cy - np.floor(cy) - 0.5) <= geo['bound_y']) | (np.abs(cx - np.floor(cx) - 0.5) <= geo['bound_x'])
    elif masked:
        near |= (np.abs(cy - np.round(cy)) <= geo['bound_y']) | (np.abs(cx - np.round(cx)) <= geo['bound_x'])
    return near & geo['sample']


# ---- the value ------------------------------------------------------------------------------------------------------------------
def coefficients(planes, order):
    """fp64 spline coefficients of fp32 planes [C, h, w], non-finite pixels taken as 0 (sunerf_prep_spline_prefilter)."""
    planes = np.asarray(planes, dtype=np.float64)
    planes = np.where(np.isfinite(planes), planes, 0.0)
    return np.stack([ndimage.spline_filter(p, order=order, mode='mirror', output=np.float64) if order > 1 else p.copy() for p in planes])


def sample_planes(planes, cy, cx, where, order):
    """[C, H, W] fp64: ``map_coordinates`` of the prefiltered planes at (cy, cx) where ``where``, NaN elsewhere."""
    coef = coefficients(planes, order)
    out = np.full((coef.shape[0],) + cy.shape, np.nan)
    if where.any():
        at = np.stack([cy[where], cx[where]])
        for i, plane in enumerate(coef):
            out[i][where] = ndimage.map_coordinates(plane, at, order=order, mode='mirror', prefilter=False)
    return out


def _mirror(i, n):
    if n <= 1:
        return np.zeros_like(i)
    period = 2 * n - 2
    i = np.mod(i, period)
    return np.where(i < n, i, period - i)


def tap_hits(mask, cy, cx, where, order):
    """[C, H, W] bool: the sampled pixels whose (order + 1)^2 taps, mirrored at the edges, read a flagged pixel of ``mask`` [C, h, w]."""
    c, h, w = mask.shape
    y, x = np.where(where, cy, 0.0), np.where(where, cx, 0.0)
    sy = (np.floor(y) if order & 1 else np.floor(y + 0.5)).astype(np.int64) - order // 2
    sx = (np.floor(x) if order & 1 else np.floor(x + 0.5)).astype(np.int64) - order // 2
    hit = np.zeros((c,) + cy.shape, dtype=bool)
    for i in range(order + 1):
        for j in range(order + 1):
            hit |= mask[:, _mirror(sy + i, h), _mirror(sx + j, w)] != 0
    return hit & where


def register_frames(frames, c2w_ref, tx_ref, ty_ref, radius=1.0, rates=(0.0, 0.0, 0.0), order=3, off_disk=CLOSEST,
                    missing=np.nan, flags=0, coords=None):
    """The whole call.  ``frames``: dicts with ``planes`` fp32 [C, h, w], an optional ``mask`` uint8 [C, h, w] and the fields of
    :func:`map_frame`.  ``coords``: sample at these [T, 2, H, W] (a device's own) instead of the restatement's.  Returns ``(out
    [T, C, H, W] float32, status [T, H, W], coords [T, 2, H, W], state [T, 4], detail)``, ``detail`` a list of :func:`map_frame`'s
    dicts with ``excluded`` = the undecidable pixels and those at a tap switch."""
    outs, stats, cos, states, detail = [], [], [], [], []
    for k, frame in enumerate(frames):
        geo = map_frame(c2w_ref, tx_ref, ty_ref, frame, radius, rates, off_disk)
        cy, cx = (geo['cy'], geo['cx']) if coords is None else (coords[k][0], coords[k][1])
        where = geo['sample'] if coords is None else geo['sample'] & np.isfinite(cy) & np.isfinite(cx)
        values = sample_planes(frame['planes'], cy, cx, where, order)
        image = np.where(where[None], values, np.float64(missing)).astype(np.float32)
        if flags & PROPAGATE and frame.get('mask') is not None:
            mask = np.asarray(frame['mask']) != 0
            mask = mask | ~np.isfinite(np.asarray(frame['planes'], dtype=np.float64))
            image[tap_hits(mask, cy, cx, where, order)] = np.nan
        geo['excluded'] = geo['undecidable'] | tap_switch(geo, order, bool(flags & PROPAGATE) and frame.get('mask') is not None)
        outs.append(image)
        stats.append(geo['status'])
        cos.append(np.stack([geo['cy'], geo['cx']]))
        states.append([int((geo['status'] == s).sum()) for s in (ON_DISK, OFF_DISK, BEHIND, OUTSIDE)])
        detail.append(geo)
    return np.stack(outs), np.stack(stats), np.stack(cos), np.asarray(states, dtype=np.int64), detail


# ---- the closed scene -----------------------------------------------------------------------------------------------------------
def surface(c2w, tx, ty, radius=1.0):
    """(lat, lon, m / radius^2, on the disk) [H, W] of the pixels of an observer: steps 1 .. 3 of the header without the rotation,
    off the disk at the point of closest approach."""
    frame = {'c2w': c2w, 'tx': tx, 'ty': ty}
    geo = map_frame(c2w, tx, ty, frame, radius, off_disk=MISSING)
    with np.errstate(all='ignore'):
        c2w = np.asarray(c2w, dtype=np.float32).reshape(3, 4).astype(np.float64)
        Ty, Tx = np.meshgrid(np.asarray(ty, dtype=np.float64), np.asarray(tx, dtype=np.float64), indexing='ij')
        e = (np.sin(Tx), -np.sin(Ty) * np.cos(Tx), -np.cos(Tx) * np.cos(Ty))
        d = [(c2w[i, 0] * e[0] + c2w[i, 1] * e[1]) + c2w[i, 2] * e[2] for i in range(3)]
        o = c2w[:, 3]
        s = -_dot(o, d) - np.where(geo['on_disk'], np.sqrt(np.maximum(geo['mrel'], 0.0) * radius * radius), 0.0)          # off the disk: CLOSEST
        p = [o[i] + d[i] * s for i in range(3)]
        return np.arctan2(-p[2], np.hypot(p[0], p[1])), np.arctan2(-p[0], p[1]), geo['mrel'], geo['on_disk']


def painted(lat, lon):
    """A smooth function on the sphere: what the closed scene shows."""
    return 1.0 + 0.5 * np.sin(3.0 * lon) * np.cos(2.0 * lat) + 0.3 * np.sin(4.0 * lat + lon) + 0.2 * np.cos(2.0 * lon - lat)


def closed_scene(shape=(64, 64), dt=4.0, rates=None, distance_ratio=0.97):
    """The closed scene of DESIGN.md 8aa: ``painted`` turns under the differential law; the reference sees it at dt = 0 from 1 au, the
    frame ``dt`` days later from the same direction at ``distance_ratio`` of the distance, on the same angular grid.  Returns ``(truth
    on the reference grid [H, W], the frame dict, c2w_ref, tx, ty, m / radius^2 of the reference pixels)``."""
    rates = RATES if rates is None else rates
    tx, ty = axes_for(shape, 1.25 * DISK)
    c2w_ref = look_at_pose(0.05, 0.1, AU)
    c2w_k = look_at_pose(0.05, 0.1, distance_ratio * AU)
    lat, lon, mrel, on_disk = surface(c2w_ref, tx, ty)
    truth = painted(lat, lon)
    lat_k, lon_k, _, on_k = surface(c2w_k, tx, ty)
    sl2 = np.sin(lat_k) ** 2
    rate = (rates[0] + rates[1] * sl2) + rates[2] * sl2 * sl2
    image = painted(lat_k, lon_k - rate * dt)          # (continued off the disk, so that no edge rings into it)
    # the plasma now at lon_k sat at lon_k - rate dt at dt = 0
    frame = {'planes': image[None].astype(np.float32), 'c2w': c2w_k, 'tx': tx, 'ty': ty, 'dt': dt, 'shift_y': 0.0, 'shift_x': 0.0, 'mask': None}
    return truth, frame, c2w_ref, tx, ty, mrel


# ---- the cases of tests/test_gpu_register.py ------------------------------------------------------------------------------------
AU = 215.03215567054764
DISK = 1.0 / AU                     # angular radius of the unit sphere from 1 au, to first order [rad]
SIDEREAL = (2.851e-6, -0.343e-6, -0.474e-6)
CARRINGTON = 2.86533e-6
# per day, relative to the Carrington frame: explicit triples, never the presets
RATES = ((SIDEREAL[0] - CARRINGTON) * 86400.0, SIDEREAL[1] * 86400.0, SIDEREAL[2] * 86400.0)
FAST = (0.2298, -0.03, -0.04)      # rad per day: a Sun that turns visibly in hours, so that small grids see BEHIND and OUTSIDE


@functools.lru_cache(maxsize=None)
def frame_planes(shape, n_planes, seed):
    """Smooth positive planes (a few waves and a blob) plus 5 % noise, fp32; read-only."""
    rng = np.random.default_rng(1000 * shape[0] + shape[1] + seed)
    h, w = shape
    y, x = np.meshgrid(np.arange(h), np.arange(w), indexing='ij')
    planes = np.stack([3.0 + np.sin(0.7 * x + 0.3 * p) * np.cos(0.5 * y - 0.2 * p) + np.exp(-((y - h / 2.0) ** 2 + (x - w / 3.0) ** 2) / 9.0)
                       for p in range(n_planes)])
    planes = (planes * (1.0 + 0.05 * rng.standard_normal(planes.shape))).astype(np.float32)
    planes.setflags(write=False)
    return planes


def _frame(shape, lat_deg, lon_deg, distance, dt, n_planes, seed, half_width=1.25 * DISK, shift=(0.0, 0.0), descending_y=False,
           roll=0.0, with_mask=False, offset=(0.0, 0.0)):
    tx, ty = axes_for(shape, half_width, descending_y, offset)
    frame = {'planes': frame_planes(shape, n_planes, seed), 'c2w': look_at_pose(math.radians(lat_deg), math.radians(lon_deg), distance, roll),
             'tx': tx, 'ty': ty, 'dt': dt, 'shift_y': shift[0], 'shift_x': shift[1], 'mask': None}
    if with_mask:
        planes = frame['planes'].copy()
        planes.reshape(-1)[5::23] = np.nan
        planes.setflags(write=False)
        mask = np.zeros(planes.shape, dtype=np.uint8)
        mask.reshape(-1)[3::17] = 1
        frame['planes'], frame['mask'] = planes, mask
    return frame


def _case(name, target, frames, rates=RATES, radius=1.0, ref=(0.0, 0.0, AU), half_width=1.25 * DISK, **kw):
    tx, ty = axes_for(target, half_width, kw.pop('descending_ref', False))
    case = {'name': name, 'c2w_ref': look_at_pose(math.radians(ref[0]), math.radians(ref[1]), ref[2]), 'tx_ref': tx, 'ty_ref': ty,
            'frames': frames, 'rates': rates, 'radius': radius, 'flags': 0}
    case.update(kw)
    return case


@functools.lru_cache(maxsize=None)
def cases():
    """name -> case: the geometries of the issue.  Every case is run at the orders and off-disk modes of ``variants``."""
    out = []
    # 24 x 20 from itself: the identity (reference = frame, dt = 0, no shift)
    out.append(_case('identity', (24, 20), [_frame((24, 20), 0.0, 0.0, AU, 0.0, 2, 0)], rates=RATES))
    # 24 x 20 from 21 x 19: observer 20 deg east, 5 deg north, 0.97 of the distance, dt = 2 days
    out.append(_case('east', (24, 20), [_frame((21, 19), 5.0, 20.0, 0.97 * AU, 2.0, 2, 1)]))
    # 33 x 17 from 16 x 40: observer -35 deg, -7 deg, dt = -3.5 days: BEHIND and OUTSIDE occur
    out.append(_case('west', (33, 17), [_frame((16, 40), -7.0, -35.0, AU, -3.5, 1, 2)]))
    # 1 x 1 from 1 x 1: the exact pose (the observer on the y axis, no rounding anywhere) and one beside it
    exact = _frame((1, 1), 0.0, 0.0, AU, 0.0, 1, 3)
    exact['c2w'] = np.array([[1, 0, 0, 0], [0, 0, 1, 215], [0, -1, 0, 0]], dtype=np.float32)
    case = _case('one', (1, 1), [exact, _frame((1, 1), 3.0, 4.0, AU, 1.0, 1, 4)])
    case['c2w_ref'] = exact['c2w'].copy()
    out.append(case)
    # 5 x 35 from 3 x 3: wider than two tiles
    out.append(_case('wide', (5, 35), [_frame((3, 3), 2.0, 6.0, AU, 0.5, 1, 5)]))
    # three frames of different shapes, C = 3, fractional shifts, a roll
    out.append(_case('three', (19, 23), [_frame((21, 19), 5.0, 20.0, 0.97 * AU, 2.0, 3, 6, shift=(0.37, -1.21)),
                                          _frame((18, 30), -3.0, -12.0, 1.02 * AU, -1.0, 3, 7, shift=(-0.62, 0.45), roll=0.21),
                                          _frame((7, 9), 0.0, 0.0, AU, 0.0, 3, 8, shift=(0.25, 0.4))]))
    # a descending ty on the frame and on the reference
    out.append(_case('descending', (17, 18), [_frame((20, 16), 4.0, -15.0, AU, 1.5, 2, 9, descending_y=True)], descending_ref=True))
    # a mask with PROPAGATE
    out.append(_case('masked', (18, 21), [_frame((17, 22), -4.0, 10.0, AU, 1.0, 2, 10, with_mask=True, shift=(0.3, 0.2))], flags=PROPAGATE))
    # a non-default radius (the grids widen with it) and a fast law: the limb of a larger sphere
    out.append(_case('radius', (20, 22), [_frame((23, 18), 6.0, 25.0, AU, 0.25, 1, 11, half_width=1.5 * DISK)], rates=FAST, radius=1.2,
                     half_width=1.5 * DISK))
    return {c['name']: c for c in out}


VARIANTS = [(0, CLOSEST), (1, CLOSEST), (3, CLOSEST), (5, CLOSEST), (3, MISSING), (2, MISSING)]


@functools.lru_cache(maxsize=None)
def case_reference(name, order, off_disk, missing=-7.5):
    case = cases()[name]
    return register_frames(case['frames'], case['c2w_ref'], case['tx_ref'], case['ty_ref'], case['radius'], case['rates'], order, off_disk,
                           missing, case['flags'])


def excluded_share(detail):
    return max(float(g['excluded'].mean()) for g in detail)
