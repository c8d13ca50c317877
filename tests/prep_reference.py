"""fp64 restatement of the image preparation (``sunerf_hip/prep.py``, ``csrc/prep.hip``), built on
``scipy.ndimage.affine_transform``, ``np.sort`` and ``np.percentile``, and the geometry cases the host and GPU tests share.

The geometry is written out independently of ``sunerf_hip.prep``: the FITS linear WCS with 1-based pixels,

    [Tx - crval_x, Ty - crval_y] = diag(cdelt) . PC . [x - crpix_x, y - crpix_y],

the north-up output grid ``T - crval = s (p' - crpix')`` and hence ``p = crpix + PC^-1 diag(1 / cdelt) s (p' - crpix')``.
"""
import functools
import math

import numpy as np
from scipy import ndimage

TWO_M23 = 2.0 ** -23
COORD_NOISE = 1e-9            # of max |image|: fp64 coordinate and prefilter noise (the issue's measurements: <= 5.3e-11, 2.3e-14)


# ---- geometry -------------------------------------------------------------------------------------------------------------------
def pc_matrix(wcs):
    if 'pc' in wcs:
        return np.asarray(wcs['pc'], dtype=np.float64)
    a = float(wcs.get('crota', 0.0))
    cdx, cdy = wcs['cdelt']
    return np.array([[math.cos(a), -math.sin(a) * cdy / cdx], [math.sin(a) * cdx / cdy, math.cos(a)]])


def crpix_of(grid):
    h, w = grid['shape']
    return np.asarray(grid.get('crpix', ((w + 1) / 2.0, (h + 1) / 2.0)), dtype=np.float64)


def scipy_matrix(wcs, grid):
    """(matrix, offset) as ``scipy.ndimage.affine_transform`` takes them: 0-based (row, column) of the source pixel of the 0-based
    output pixel."""
    s = float(grid['cdelt'][0])
    a = np.linalg.inv(np.diag(np.asarray(wcs['cdelt'], dtype=np.float64)) @ pc_matrix(wcs)) * s       # (x, y) order
    off = (crpix_of(wcs) - 1.0) - a @ (crpix_of(grid) - 1.0)
    return a[::-1, ::-1].copy(), off[::-1].copy()


def source_coordinates(matrix, offset, out_shape):
    """fp64 source (row, column) of every output pixel, in scipy's order of operations."""
    r, c = np.meshgrid(np.arange(out_shape[0], dtype=np.float64), np.arange(out_shape[1], dtype=np.float64), indexing='ij')
    return (offset[0] + matrix[0, 0] * r) + matrix[0, 1] * c, (offset[1] + matrix[1, 0] * r) + matrix[1, 1] * c


def centred_grid(out_shape, s, crval=(0.0, 0.0)):
    h, w = out_shape
    return {'shape': (int(h), int(w)), 'cdelt': (s, s), 'crpix': ((w + 1) / 2.0, (h + 1) / 2.0), 'crval': tuple(crval)}


# ---- resample and epilogue ------------------------------------------------------------------------------------------------------
def zero_nonfinite(image):
    image = np.asarray(image, dtype=np.float64)
    return np.where(np.isfinite(image), image, 0.0)


def resample(image, matrix, offset, out_shape, order, missing=0.0):
    """(C, H', W') fp64: scipy on every plane of ``image`` (C, H, W), non-finite pixels taken as 0."""
    planes = zero_nonfinite(image)
    return np.stack([ndimage.affine_transform(p, matrix, offset, tuple(out_shape), np.float64, order, 'constant', missing, True)
                     for p in planes])


def _mirror(i, n):
    if n <= 1:
        return np.zeros_like(i)
    period = 2 * n - 2
    i = np.mod(i, period)
    return np.where(i < n, i, period - i)


def nan_footprint(image, matrix, offset, out_shape, order):
    """(C, H', W') bool: the output pixels inside the frame whose (order + 1) x (order + 1) tap box, mirrored at the edges,
    holds a non-finite input pixel."""
    bad = ~np.isfinite(np.asarray(image, dtype=np.float64))
    c, h, w = bad.shape
    y, x = source_coordinates(matrix, offset, out_shape)
    inside = (y >= 0) & (y <= h - 1) & (x >= 0) & (x <= w - 1)
    sy = (np.floor(y) if order & 1 else np.floor(y + 0.5)).astype(np.int64) - order // 2
    sx = (np.floor(x) if order & 1 else np.floor(x + 0.5)).astype(np.int64) - order // 2
    hit = np.zeros((c,) + tuple(out_shape), dtype=bool)
    for i in range(order + 1):
        for j in range(order + 1):
            hit |= bad[:, _mirror(sy + i, h), _mirror(sx + j, w)]
    return hit & inside


def _per_plane(v, c):
    v = np.atleast_1d(np.asarray(v, dtype=np.float64)).reshape(-1)
    return np.broadcast_to(v, (c,)).reshape(c, 1, 1)


def prepare(image, matrix, offset, out_shape, order=3, missing=0.0, factor=1.0, norm=None, clip_negative=True,
            clip_to_input_range=True, nan_policy='zero'):
    """(fp64 values before the one rounding to fp32, the fp32 result): the resample and the epilogue, step by step."""
    image = np.asarray(image, dtype=np.float32)
    c = image.shape[0]
    v = resample(image, matrix, offset, out_shape, order, missing)
    if clip_to_input_range:
        lo = np.empty((c, 1, 1))
        hi = np.empty((c, 1, 1))
        for k, p in enumerate(image):
            f = p[np.isfinite(p)].astype(np.float64)
            lo[k] = min(f.min(), missing) if f.size else missing
            hi[k] = max(f.max(), missing) if f.size else missing
        v = np.clip(v, lo, hi)
    v = v * _per_plane(factor, c)
    if norm is not None:
        vmin, vmax = _per_plane(norm[0], c), _per_plane(norm[1], c)
        with np.errstate(all='ignore'):
            v = (v - vmin) / (vmax - vmin)
        if len(norm) == 3 and norm[2]:
            v = np.clip(v, 0.0, 1.0)
    if clip_negative:
        v = np.where(v < 0, 0.0, v)
    with np.errstate(over='ignore'):
        out = v.astype(np.float32)
    bad = ~np.isfinite(out)
    out[bad] = 0.0
    v = np.where(bad, 0.0, v)
    if nan_policy == 'propagate':
        hit = nan_footprint(image, matrix, offset, out_shape, order)
        out[hit] = np.nan
        v = np.where(hit, np.nan, v)
    return v, out


def gate(got, want, scale):
    """The largest |got - want| / (2^-23 |want| + 1e-9 scale): the one rounding to fp32, and the fp64 coordinate and prefilter noise
    relative to ``scale`` = max |image| carried through the epilogue's linear map.  NaNs must coincide."""
    got = np.asarray(got, dtype=np.float64)
    want = np.asarray(want, dtype=np.float64)
    assert np.array_equal(np.isnan(got), np.isnan(want)), 'NaN sets differ'
    ok = ~np.isnan(want)
    if not ok.any():
        return 0.0
    return float((np.abs(got[ok] - want[ok]) / (TWO_M23 * np.abs(want[ok]) + COORD_NOISE * scale)).max())


# ---- quantiles ------------------------------------------------------------------------------------------------------------------
def sorted_valid(x):
    """(ascending non-NaN values of one plane, NaN count): np.sort puts NaNs last."""
    x = np.asarray(x, dtype=np.float32).reshape(-1)
    n_nan = int(np.isnan(x).sum())
    return np.sort(x)[:x.size - n_nan], n_nan


def percentile(x, q):
    """np.percentile (linear) of the non-NaN values, computed on fp64 copies and cast to fp32."""
    v, _ = sorted_valid(x)
    if not v.size:
        return np.float32(np.nan)
    with np.errstate(invalid='ignore'):
        return np.float32(np.percentile(v.astype(np.float64), q))


# ---- the cases ------------------------------------------------------------------------------------------------------------------
def _case(name, shape, cdelt, crpix, out_shape, s, crota=None, pc=None, exact=False):
    wcs = {'shape': shape, 'cdelt': cdelt, 'crpix': crpix, 'crval': (12.5, -30.25)}
    if crota is not None:
        wcs['crota'] = crota
    if pc is not None:
        wcs['pc'] = pc
    return {'name': name, 'wcs': wcs, 'out_shape': out_shape, 's': s, 'exact': exact}


def geometry_cases(segment, horizon):
    """Every geometry the GPU tests resample.  ``exact`` cases map output pixels onto input pixels exactly on at least one axis
    (their coordinates are integers in fp64 there); on every other axis the coordinates keep clear of the borders."""
    cases = [
        _case('t0', (37, 53), (.6, .6), (27.3, 18.9), (41, 47), 0.731, crota=0.3217),
        _case('t1', (33, 65), (1.59, 1.59), (30.2, 17.7), (50, 50), 1.2, crota=-2.4871),
        _case('t2', (5, 7), (1.0, 1.3), (3.9, 2.6), (9, 8), 0.57, crota=1.0103),
        _case('t3', (130, 259), (4.4, 4.4), (120.7, 61.2), (97, 131), 5.13, crota=3.0519),
        _case('one', (1, 1), (1.0, 1.0), (1.0, 1.0), (3, 3), 1.0, crota=0.0, exact=True),
        _case('two', (2, 2), (1.0, 1.0), (1.4, 1.6), (4, 4), 0.6, crota=0.7),
        _case('column', (3, 1), (0.5, 0.8), (1.0, 2.1), (5, 1), 0.5, crota=0.0, exact=True),
        _case('strip', (1, 9), (1.0, 1.0), (5.0, 1.0), (3, 9), 1.0, crota=0.0, exact=True),
        _case('pc', (23, 19), (1.1, 0.9), (9.3, 12.2), (21, 26), 1.07, pc=[[0.8, -0.55], [0.62, 0.79]]),
        _case('short', (22, 46), (2.0, 2.0), (23.9, 11.3), (19, 33), 2.9, crota=0.52),
    ]
    for k, n in enumerate((segment - 1, segment, segment + 1, 2 * segment + 1)):
        cases.append(_case(f'x{n}', (9, n), (1.0, 1.0), (n / 2.0 + 0.37, 5.21), (17, 41), n / 36.3, crota=0.11 + 0.07 * k))
        cases.append(_case(f'y{n}', (n, 9), (1.0, 1.0), (5.21, n / 2.0 + 0.37), (41, 17), n / 36.3, crota=0.13 + 0.07 * k))
    assert any(min(c['wcs']['shape']) < horizon[o] for c in cases for o in (2, 3, 4, 5))
    return cases


def case_matrix(case):
    grid = centred_grid(case['out_shape'], case['s'], case['wcs']['crval'])
    return grid, scipy_matrix(case['wcs'], grid)


@functools.lru_cache(maxsize=None)
def case_image(shape, n_planes, seed=0):
    """Random planes in [0, 1000); with three planes the second is a spike and the third a constant."""
    rng = np.random.default_rng(1000 * shape[0] + shape[1] + seed)
    img = (rng.random((n_planes,) + tuple(shape)) * 1000.0).astype(np.float32)
    if n_planes == 3:
        img[1] = 0.0
        img[1, shape[0] // 2, shape[1] // 3] = 999.0
        img[2] = 417.25
    img.setflags(write=False)
    return img


def border_clearance(coords, n, order):
    """(all coordinates are integers, the smallest distance of a coordinate to a border 0 / n - 1 -- and for order 0 to a
    half-integer)."""
    coords = np.asarray(coords)
    if np.array_equal(coords, np.round(coords)):
        return True, np.inf
    d = min(np.abs(coords).min(), np.abs(coords - (n - 1)).min())
    if order == 0:
        d = min(d, np.abs(coords - np.floor(coords) - 0.5).min())
    return False, float(d)
