"""NumPy restatement of the co-alignment step, written from include/sunerf_hip_coalign.h and the formulas of
sunerf_hip/coalign.py's docstrings: the six sums by plain loops over the shifts, the scores, the peak with its
parabola and status bits, the shifted plate-scale dict -- and the analytic scene of the sub-pixel tests."""
import math

import numpy as np

NO_PEAK, EDGE, FLAT = 1, 2, 4
BOUNDS = {'zncc': 1.0, 'ssd': 0.0}
MAX_SHIFT = 32


def valid_mask(values, bad=None):
    ok = np.isfinite(values)
    return ok if bad is None else ok & (np.asarray(bad) == 0)


def _overlap(n, d):
    """Template rows (or columns) r with r and r + d inside 0 .. n - 1, as a pair of slices (template, image), or None."""
    lo, hi = max(0, -d), min(n, n - d)
    return None if lo >= hi else (slice(lo, hi), slice(lo + d, hi + d))


def pairs(image, templ, bad_image, bad_template, p, dy, dx):
    """(a, b) as fp64 vectors: the pair set of plane ``p`` at shift (dy, dx)."""
    h, w = image.shape[1:]
    rows, cols = _overlap(h, dy), _overlap(w, dx)
    if rows is None or cols is None:
        return np.zeros(0), np.zeros(0)
    a = image[p][rows[1], cols[1]]
    b = templ[p][rows[0], cols[0]]
    ok = valid_mask(a, None if bad_image is None else bad_image[p][rows[1], cols[1]])
    ok &= valid_mask(b, None if bad_template is None else bad_template[p][rows[0], cols[0]])
    return a[ok].astype(np.float64), b[ok].astype(np.float64)


def shift_sums(image, templ, max_dy, max_dx, bad_image=None, bad_template=None, exact=None):
    """[C, 2 max_dy + 1, 2 max_dx + 1, 6] fp64: n, Sa, Sb, Saa, Sbb, Sab.  ``exact``: None sums with ``np.sum`` (fp64, pairwise:
    exact whenever no addition can round, as with dyadic inputs); ``'fsum'`` with ``math.fsum`` (the correctly rounded sum);
    ``'longdouble'`` in ``np.longdouble``, rounded to fp64 once."""
    image, templ = np.asarray(image, dtype=np.float32), np.asarray(templ, dtype=np.float32)
    c = image.shape[0]
    out = np.zeros((c, 2 * max_dy + 1, 2 * max_dx + 1, 6))
    if exact == 'fsum':
        total = lambda v: math.fsum(v.tolist())                                      # noqa: E731
    elif exact == 'longdouble':
        total = lambda v: float(np.sum(v.astype(np.longdouble)))                     # noqa: E731
    else:
        total = lambda v: float(np.sum(v))                                           # noqa: E731
    for p in range(c):
        for i, dy in enumerate(range(-max_dy, max_dy + 1)):
            for j, dx in enumerate(range(-max_dx, max_dx + 1)):
                a, b = pairs(image, templ, bad_image, bad_template, p, dy, dx)
                if a.size:
                    out[p, i, j] = [a.size, total(a), total(b), total(a * a), total(b * b), total(a * b)]
    return out


def sum_bounds(image, templ, max_dy, max_dx, bad_image=None, bad_template=None):
    """[C, Sy, Sx, 6]: ``N 2^-53 sum |term|`` per sum, N the shift's pair count -- the bound of any order of N - 1 fp64 additions
    of exact terms (each rounds by at most 2^-53 of a partial sum, which never exceeds sum |term|); 0 for n itself."""
    image, templ = np.asarray(image, dtype=np.float32), np.asarray(templ, dtype=np.float32)
    out = np.zeros((image.shape[0], 2 * max_dy + 1, 2 * max_dx + 1, 6))
    for p in range(image.shape[0]):
        for i, dy in enumerate(range(-max_dy, max_dy + 1)):
            for j, dx in enumerate(range(-max_dx, max_dx + 1)):
                a, b = pairs(image, templ, bad_image, bad_template, p, dy, dx)
                if a.size:
                    mag = [0.0, np.abs(a).sum(), np.abs(b).sum(), (a * a).sum(), (b * b).sum(), np.abs(a * b).sum()]
                    out[p, i, j] = a.size * 2.0 ** -53 * np.asarray(mag)
    return out


def scores_from_sums(sums, measure='zncc', min_overlap=0.5):
    n, sa, sb, saa, sbb, sab = (sums[..., k] for k in range(6))
    with np.errstate(invalid='ignore', divide='ignore'):
        refused = (n < min_overlap * n.max(axis=(1, 2), keepdims=True)) | (n <= 0)
        if measure == 'zncc':
            cov = n * sab - sa * sb
            va = n * saa - sa * sa
            vb = n * sbb - sb * sb
            refused = refused | (va <= 0) | (vb <= 0)
            score = cov / np.sqrt(va * vb)
        else:
            score = -((saa - 2.0 * sab) + sbb) / n
    return np.where(refused, np.nan, score)


def _peak_of_map(m, bound=None):
    sy, sx = m.shape
    finite = np.isfinite(m)
    if not finite.any():
        return np.zeros(2), np.zeros(2, dtype=np.int64), np.nan, NO_PEAK
    iy, ix = np.unravel_index(int(np.argmax(np.where(finite, m, -np.inf))), m.shape)          # the first maximum, row-major
    padded = np.full((sy + 2, sx + 2), np.nan)
    padded[1:-1, 1:-1] = m
    s0 = m[iy, ix]
    status, offset = 0, [0.0, 0.0]
    integer = np.array([iy - sy // 2, ix - sx // 2], dtype=np.int64)
    if bound is not None and s0 == bound:          # an exact copy on the pair set: the whole-pixel shift is the answer
        return integer.astype(np.float64), integer, s0, 0
    for axis, (i, size, lo, hi) in enumerate(((iy, sy, padded[iy, ix + 1], padded[iy + 2, ix + 1]),
                                              (ix, sx, padded[iy + 1, ix], padded[iy + 1, ix + 2]))):
        if size == 1:
            continue
        if i == 0 or i == size - 1:
            status |= EDGE
            continue
        second = (lo - 2.0 * s0) + hi
        if not second < 0:
            status |= FLAT
            continue
        offset[axis] = min(0.5, max(-0.5, 0.5 * (lo - hi) / second))
    return integer + np.array(offset), integer, s0, status


def peak(scores, combine='shared', bound=None):
    scores = np.asarray(scores, dtype=np.float64)
    if combine == 'shared':
        used = np.isfinite(scores).reshape(scores.shape[0], -1).any(axis=1)
        m = scores[used].sum(axis=0) / used.sum() if used.any() else np.full(scores.shape[1:], np.nan)
        shift, integer, score, status = _peak_of_map(m, bound)
        return {'shift': shift, 'integer': integer, 'score': score, 'status': status}
    found = [_peak_of_map(m, bound) for m in scores]
    return {'shift': np.stack([f[0] for f in found]), 'integer': np.stack([f[1] for f in found]),
            'score': np.array([f[2] for f in found]), 'status': np.array([f[3] for f in found], dtype=np.int64)}


def coalign(image, templ, max_shift, bad_image=None, bad_template=None, measure='zncc', min_overlap=0.5, combine='shared'):
    my, mx = (max_shift, max_shift) if np.isscalar(max_shift) else max_shift
    sums = shift_sums(image, templ, my, mx, bad_image, bad_template)
    scores = scores_from_sums(sums, measure, min_overlap)
    out = peak(scores, combine, BOUNDS[measure])
    out.update(scores=scores, sums=sums)
    return out


def shifted_grid(grid, dy, dx):
    h, w = grid['shape']
    cpx, cpy = grid.get('crpix', ((w + 1) / 2., (h + 1) / 2.))
    out = dict(grid)
    out['crpix'] = (cpx + dx, cpy + dy)
    return out


def plate_scale_axes(grid):
    """``linear_plate_scale_axes`` without the conversion to radians: (tx, ty) in the units of cdelt."""
    h, w = grid['shape']
    cdx, cdy = grid['cdelt']
    cpx, cpy = grid.get('crpix', ((w + 1) / 2., (h + 1) / 2.))
    cvx, cvy = grid.get('crval', (0., 0.))
    return (np.arange(1, w + 1, dtype=np.float64) - cpx) * cdx + cvx, (np.arange(1, h + 1, dtype=np.float64) - cpy) * cdy + cvy


# ---- the analytic scene of the sub-pixel tests ----------------------------------------------------------------------------------
SCENE_SHAPE = (96, 80)
SCENE_SHIFTS = ((3.0, -5.0), (2.3, -1.6), (-4.5, 0.5), (0.25, 6.75))


def scene(dy=0.0, dx=0.0, seed=11, n_blobs=40):
    """[1, 96, 80] float32: ``n_blobs`` Gaussians (sigma 2 .. 6 px, amplitude 0.3 .. 1) on a pedestal of 0.2, with the content
    moved ``dy`` rows and ``dx`` columns further along: value(r, c) = f(r - dy, c - dx)."""
    rng = np.random.default_rng(seed)
    h, w = SCENE_SHAPE
    cy, cx = rng.uniform(0, h, n_blobs), rng.uniform(0, w, n_blobs)
    sigma, amp = rng.uniform(2.0, 6.0, n_blobs), rng.uniform(0.3, 1.0, n_blobs)
    r, c = np.mgrid[0:h, 0:w].astype(np.float64)
    r, c = r - dy, c - dx
    out = np.full((h, w), 0.2)
    for k in range(n_blobs):
        out += amp[k] * np.exp(-((r - cy[k]) ** 2 + (c - cx[k]) ** 2) / (2.0 * sigma[k] ** 2))
    return out[None].astype(np.float32)


def scene_pair(dy, dx):
    """(image, template, bad_template): the image is the scene moved by (dy, dx); the template is the scene in place, NaN outside
    a disk of radius 44 about the frame's centre, with a lattice of bad pixels (every 7th row x every 5th column)."""
    h, w = SCENE_SHAPE
    image, templ = scene(dy, dx), scene()
    r, c = np.mgrid[0:h, 0:w]
    templ[0][(r - (h - 1) / 2.0) ** 2 + (c - (w - 1) / 2.0) ** 2 > 44.0 ** 2] = np.nan
    bad = np.zeros((1, h, w), dtype=np.uint8)
    bad[0, 3::7, 2::5] = 1
    return image, templ, bad
