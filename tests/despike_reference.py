"""NumPy restatement (fp64) of the despiking algorithm of include/sunerf_hip_despike.h, DESIGN.md 8v: written from the header's
text, with sorts where the kernel has networks, whole-plane arrays where it has tiles and no early exit but the header's rule.

``despike(x, ...)`` takes one plane [H, W] or planes [C, H, W] of float32 and returns ``image`` (float32), ``mask`` (uint8) and
``state`` [C, 6] (float64) as the entry point writes them.  Every decision uses + - * max and comparisons on float64 only, in the
header's order, so that the device agrees by value and not to a tolerance."""
import numpy as np

SPIKE, INVALID, UNFILLED = 1, 2, 4
MODEL, MAD = 0, 1
TWO_SIDED, FILL_NAN = 1, 2
N_STATE = 6


def neighbours(x, mask, r):
    """[H, W, (2r+1)^2 - 1] float64: the window's values without the centre; NaN where the neighbour lies outside the frame or
    carries a bit in ``mask``."""
    h, w = x.shape
    xp = np.full((h + 2 * r, w + 2 * r), np.nan)
    xp[r:r + h, r:r + w] = np.where(mask != 0, np.nan, x.astype(np.float64))
    out = [xp[r + dy:r + dy + h, r + dx:r + dx + w] for dy in range(-r, r + 1) for dx in range(-r, r + 1) if (dy, dx) != (0, 0)]
    return np.stack(out, axis=-1)


def masked_median(v):
    """``(med, n)`` along the last axis of ``v`` whose NaN entries take no part: the mean of the order statistics of ranks
    ``(n - 1) // 2`` and ``n // 2``, ``0.5 * (lo + hi)`` in float64; NaN where n = 0."""
    n = (~np.isnan(v)).sum(axis=-1)
    s = np.sort(v, axis=-1)                      # NaN last
    lo = np.take_along_axis(s, np.maximum((n - 1) // 2, 0)[..., None], axis=-1)[..., 0]
    hi = np.take_along_axis(s, (n // 2)[..., None].clip(0, v.shape[-1] - 1), axis=-1)[..., 0]
    with np.errstate(invalid='ignore'):
        return 0.5 * (lo + hi), n


def has_spike_neighbour(mask):
    h, w = mask.shape
    mp = np.zeros((h + 2, w + 2), dtype=bool)
    mp[1:1 + h, 1:1 + w] = (mask & SPIKE) != 0
    out = np.zeros((h, w), dtype=bool)
    for dy in (-1, 0, 1):
        for dx in (-1, 0, 1):
            if (dy, dx) != (0, 0):
                out |= mp[1 + dy:1 + dy + h, 1 + dx:1 + dx + w]
    return out


def detection_pass(x, mask, r, mode, a, b, floor, n_sigma, grow_sigma, min_valid, two_sided):
    """The pixels (bool [H, W]) one pass adds to ``mask``."""
    v = neighbours(x, mask, r)
    med, n = masked_median(v)
    t = np.where(has_spike_neighbour(mask), np.float64(grow_sigma), np.float64(n_sigma))
    with np.errstate(invalid='ignore'):
        d = x.astype(np.float64) - med
        if mode == MODEL:
            var = a + b * np.maximum(med, 0.0)
            lim = (t * t) * var
            hit = ((d != 0.0) if two_sided else (d > 0.0)) & (d * d > lim)
        else:
            mad, _ = masked_median(np.abs(v - med[..., None]))
            s = np.maximum(1.4826 * mad, floor)
            hit = (np.abs(d) if two_sided else d) > t * s
    return (mask == 0) & (n >= min_valid) & hit


def despike_plane(x, bad=None, a=0.0, b=0.0, floor=0.0, radius=2, mode=MODEL, flags=0, n_sigma=5.0, grow_sigma=3.0, min_valid=3,
                  max_iterations=4):
    x = np.asarray(x, dtype=np.float32)
    mask = np.where(~np.isfinite(x), INVALID, 0).astype(np.uint8)
    if bad is not None:
        mask[np.asarray(bad) != 0] = INVALID
    xs = np.where(np.isfinite(x), x, np.float32(0.0))          # the values of INVALID pixels are never read
    n_invalid = int((mask != 0).sum())
    passes, converged, n_spike = 0, 0, 0
    for _ in range(max_iterations):
        new = detection_pass(xs, mask, radius, mode, float(a), float(b), float(floor), n_sigma, grow_sigma, min_valid,
                             bool(flags & TWO_SIDED))
        if not new.any():
            converged = 1
            break
        mask = mask | np.where(new, SPIKE, 0).astype(np.uint8)          # Jacobi: the whole pass read the old mask
        n_spike += int(new.sum())
        passes += 1
    med, n = masked_median(neighbours(xs, mask, radius))
    flagged = mask != 0
    out = x.copy()
    if flags & FILL_NAN:
        out[flagged] = np.nan
        n_unfilled = 0
    else:
        fill = flagged & (n >= min_valid)
        unfilled = flagged & (n < min_valid)
        out[fill] = med[fill].astype(np.float32)
        out[unfilled] = np.nan
        mask = mask | np.where(unfilled, UNFILLED, 0).astype(np.uint8)
        n_unfilled = int(unfilled.sum())
    return out, mask, np.array([n_spike, n_invalid, n_unfilled, passes, converged, 0], dtype=np.float64)


def despike(x, bad=None, params=None, **kw):
    """Planes [C, H, W] (or one [H, W]); ``params`` [C, 3+] = a, b, floor per plane (default zeros).  Returns ``(image, mask, state)``."""
    x = np.asarray(x, dtype=np.float32)
    single = x.ndim == 2
    planes = x[None] if single else x
    c = planes.shape[0]
    params = np.zeros((c, 4)) if params is None else np.asarray(params, dtype=np.float64).reshape(c, -1)
    bad = None if bad is None else np.asarray(bad).reshape(planes.shape)
    outs = [despike_plane(planes[i], None if bad is None else bad[i], a=params[i, 0], b=params[i, 1], floor=params[i, 2], **kw)
            for i in range(c)]
    image, mask, state = (np.stack([o[k] for o in outs]) for k in range(3))
    return (image[0], mask[0], state) if single else (image, mask, state)


# ---- the fixed scene of the host test ---------------------------------------------------------------------------------------------
SCENE = dict(unit=100.0, exposure=2.9, dn_per_photon=1.2, read_noise=1.2)


def scene(size=96):
    """``(truth, a, b)``: the noise-free 96 x 96 scene (a disc with structure inside a falling corona, blurred by a Gaussian of
    FWHM 2.5) and the variance parameters of the instrument it is seen through."""
    from scipy.ndimage import gaussian_filter
    yy, xx = np.mgrid[:size, :size]
    rr = np.hypot(yy - size / 2, xx - size / 2)
    truth = np.where(rr < 30, 1.0 + 0.3 * np.sin(xx / 5.0) * np.cos(yy / 7.0), 0.05 + 1.2 * np.exp(-(rr - 30) / 8.0))
    truth = gaussian_filter(truth, 2.5 / 2.3548, mode='nearest')
    ue = SCENE['unit'] * SCENE['exposure']
    return truth, SCENE['read_noise'] ** 2 / ue ** 2, SCENE['dn_per_photon'] / ue


def observed_scene(rng, truth):
    ue, g = SCENE['unit'] * SCENE['exposure'], SCENE['dn_per_photon']
    return (rng.poisson(truth * ue / g) * g + rng.normal(0.0, SCENE['read_noise'], truth.shape)) / ue


def add_hits(rng, obs, sigma, fraction=0.01, amplitude=(10.0, 50.0)):
    """``(image, truth)``: ``fraction`` of the pixels hit, every fourth hit a 3-pixel track along the row, amplitudes uniform in
    ``amplitude`` times the local ``sigma``."""
    h, w = obs.shape
    x = obs.copy()
    truth = np.zeros((h, w), dtype=bool)
    idx = rng.choice(h * w, h * w // int(round(1 / fraction)), replace=False)
    ys, xs = np.unravel_index(idx, (h, w))
    for k, (y, xq) in enumerate(zip(ys, xs)):
        for j in range(3 if k % 4 == 0 else 1):
            if xq + j < w:
                x[y, xq + j] += rng.uniform(*amplitude) * sigma[y, xq + j]
                truth[y, xq + j] = True
    return x, truth
