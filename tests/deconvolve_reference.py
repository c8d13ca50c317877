"""fp64 NumPy restatement of include/sunerf_hip_deconvolve.h's Richardson-Lucy iteration, exactly as the header words it (the order
of every operation of a pixel included; NumPy never fuses a multiply with an add), for tests/test_deconvolve_host.py and the GPU
tests of the deconvolution table.  The two correlations are the restatements the instrument and patch tables are held to:
``instrument_reference.correlate_bin`` and ``patch_reference.correlate_bin_adjoint`` both return their fp64 sums before ``scale``.

What is by bits and what is not: ``u`` after any number of updates is made of +, * and / in a pinned order, so the kernel must
give these bits.  The deviance is a sum of many terms whose order the header pins for the kernel's tiles; here it is
``numpy.sum`` (pairwise), and ``log`` is NumPy's: `ratio_pass` returns beside it ``scale``, the sum of
|L| + |N| + |N log(N / L)| over the plane, on which the GPU tests bound the difference."""
import numpy as np

from instrument_reference import correlate_bin
from patch_reference import correlate_bin_adjoint

# (planes, H, W, kh, kw, bin, anchor, per-plane K): the cases of the issue, every one for both boundaries
CASES = [
    (1, 5, 7, 1, 1, 1, (0, 0), False),
    (2, 9, 11, 3, 5, 1, (1, 2), True),
    (1, 9, 11, 4, 2, 2, (3, 1), False),
    (3, 13, 10, 5, 5, 3, (2, 2), True),
    (1, 2, 3, 7, 7, 1, (3, 3), False),           # the plane is smaller than the kernel
    (1, 70, 67, 9, 9, 2, (4, 4), False),         # several tiles of both kernels
    (1, 32, 32, 5, 5, 2, (2, 2), False),         # exactly one update tile
    (2, 45, 71, 7, 5, 3, (3, 1), True),          # partial last tiles
    (1, 40, 40, 96, 96, 8, (48, 48), False),     # the limits
]
BOUNDARIES = ('zero', 'nearest')


def photon_params(unit, exposure, dn_per_photon, read_noise, quantise=False):
    """(c, v): photons per image unit and the read variance in photons^2."""
    c = unit * exposure / dn_per_photon
    v = (read_noise * read_noise + (1.0 / 12.0 if quantise else 0.0)) / (dn_per_photon * dn_per_photon)
    return c, v


def valid_mask(d, bad=None):
    d = np.asarray(d, dtype=np.float32)
    return np.isfinite(d) if bad is None else np.isfinite(d) & (np.asarray(bad) == 0)


def norm_of(d, bad, K, height, width, bin_factor, anchor, scale, boundary):
    """norm = A^T(valid as 1.0f / 0.0f): fp32 [P, height, width]."""
    return correlate_bin_adjoint(valid_mask(d, bad).astype(np.float32), K, height, width, bin_factor, anchor, scale, boundary)[0]


def initial_image(d, bad, bin_factor, bin_mode='mean', init='image'):
    """sunerf_hip.deconvolve.initial_image: every detector pixel replicated bin x bin (over bin^2 under 'sum'), invalid or
    non-positive pixels replaced by the plane's mean over its valid positive pixels; 'flat': that mean everywhere."""
    d = np.asarray(d, dtype=np.float32)
    x = d / np.float32(bin_factor * bin_factor) if bin_mode == 'sum' else d
    with np.errstate(invalid='ignore'):
        good = valid_mask(d, bad) & (x > 0)
    out = np.empty_like(x)
    for p in range(x.shape[0]):
        mean = np.float32(x[p][good[p]].astype(np.float64).sum() / good[p].sum()) if good[p].any() else np.float32(1.0)
        out[p] = mean if init == 'flat' else np.where(good[p], x[p], mean)
    return np.repeat(np.repeat(out, bin_factor, axis=1), bin_factor, axis=2)


def ratio_pass(u, d, bad, K, bin_factor, anchor, scale, boundary, c, v):
    """One pass over planes u [P, H, W] fp32 with per-plane c, v [P]: (ratio fp32 [P, h, w], deviance [P], n_valid [P],
    scale of the deviance's terms [P])."""
    u = np.asarray(u, dtype=np.float32)
    d = np.asarray(d, dtype=np.float32)
    c = np.asarray(c, dtype=np.float64).reshape(-1, 1, 1)
    v = np.asarray(v, dtype=np.float64).reshape(-1, 1, 1)
    off = v / c
    valid = valid_mask(d, bad)
    with np.errstate(all='ignore'):
        acc = correlate_bin(u, K, bin_factor, anchor, 1.0, boundary)[1]
        e = scale * acc
        den = e + off
        num = np.where(valid, d.astype(np.float64) + off, 0.0)
        num = np.where(num > 0.0, num, 0.0)
        fit = valid & (den > 0.0)
        r = np.where(fit, num / np.where(fit, den, 1.0), 0.0).astype(np.float32)
        L, N = c * den, c * num
        pos = fit & (N > 0.0)
        nlog = np.where(pos, N * np.log(np.where(pos, N, 1.0) / np.where(pos, L, 1.0)), 0.0)
        term = np.where(fit, 2.0 * ((L - N) + nlog), 0.0)
        size = np.where(fit, np.abs(L) + np.abs(N) + np.abs(nlog), 0.0)
    return r, term.sum(axis=(1, 2)), valid.sum(axis=(1, 2)).astype(np.float64), size.sum(axis=(1, 2))


def update(u, r, norm, K, bin_factor, anchor, scale, boundary):
    """u' = norm > 0 ? (float) (((double) u * t) / (double) norm) : u with t = scale * A^T r."""
    u = np.asarray(u, dtype=np.float32)
    t = scale * correlate_bin_adjoint(r, K, u.shape[1], u.shape[2], bin_factor, anchor, 1.0, boundary)[1]
    with np.errstate(all='ignore'):
        live = norm > 0
        new = (u.astype(np.float64) * t) / np.where(live, norm, 1.0).astype(np.float64)
    return np.where(live, new.astype(np.float32), u)


def richardson_lucy(u0, d, bad, norm, K, bin_factor, anchor, scale, boundary, c, v, n_iterations, stop=0.0, history=None, iterates=None):
    """The header's call on planes u0 [P, H, W]: (u fp32, state [P, 4] = deviance, n_valid, iterations_applied, stopped, scale
    [P] of the reported deviance's terms).  Every plane runs on its own, with its kernel and its (c, v).  ``history``: a list
    that receives, per plane, the list of (deviance, n_valid, scale) of every pass -- pass k describes the iterate after k updates, so
    one run of n updates holds the state of every shorter run; ``iterates``: a list that receives, per plane, those iterates."""
    u0 = np.asarray(u0, dtype=np.float32)
    d = np.asarray(d, dtype=np.float32)
    K = np.asarray(K, dtype=np.float64)
    K = K[None] if K.ndim == 2 else K
    planes = u0.shape[0]
    c = np.broadcast_to(np.asarray(c, dtype=np.float64), (planes,))
    v = np.broadcast_to(np.asarray(v, dtype=np.float64), (planes,))
    out = u0.copy()
    state = np.zeros((planes, 4))
    sizes = np.zeros(planes)
    for p in range(planes):
        sl = slice(p, p + 1)
        Kp = K[sl] if K.shape[0] > 1 else K
        badp = None if bad is None else np.asarray(bad)[sl]
        u = u0[sl].copy()
        applied, trace, seen = 0, [], []
        for k in range(n_iterations + 1):
            r, dev, nv, size = ratio_pass(u, d[sl], badp, Kp, bin_factor, anchor, scale, boundary, c[sl], v[sl])
            trace.append((float(dev[0]), float(nv[0]), float(size[0])))
            seen.append(u[0].copy())
            stopped = bool(stop > 0.0 and dev[0] <= stop * nv[0])
            if stopped or k == n_iterations:
                break
            u = update(u, r, np.asarray(norm)[sl], Kp, bin_factor, anchor, scale, boundary)
            applied += 1
        out[sl] = u
        state[p] = (dev[0], nv[0], applied, float(stopped))
        sizes[p] = size[0]
        if history is not None:
            history.append(trace)
        if iterates is not None:
            iterates.append(seen)
    return out, state, sizes


def case_data(case, seed=0, read_noise=1.2):
    """Inputs of a by-bits case: a non-negative K [1 or P, kh, kw] (a few exact zeros among its taps), a positive u0 [P, H, W] of
    several magnitudes, d [P, h, w] with a few negative values, one NaN and (``bad``) one flagged pixel per plane, and per-plane
    (c, v) of a detector with read noise."""
    planes, h, w, kh, kw, b, _, per_plane = case
    rng = np.random.default_rng([seed, planes, h, w, kh, kw, b])
    K = rng.uniform(0.0, 1.0, size=(planes if per_plane else 1, kh, kw)) * 10.0 ** rng.integers(-2, 1, size=(1, kh, kw))
    K[rng.uniform(size=K.shape) < 0.1] = 0.0
    if not K.any():
        K[:, 0, 0] = 0.5
    K = K / K.sum(axis=(1, 2), keepdims=True)
    u0 = (rng.uniform(0.2, 1.0, size=(planes, h, w)) * 10.0 ** rng.integers(-1, 2, size=(planes, h, w))).astype(np.float32)
    oh, ow = h // b, w // b
    d = (rng.uniform(0.2, 1.0, size=(planes, oh, ow)) * 10.0 ** rng.integers(-1, 2, size=(planes, oh, ow))).astype(np.float32)
    bad = np.zeros((planes, oh, ow), dtype=np.uint8)
    n = oh * ow
    for p in range(planes):
        flat = rng.permutation(n)
        neg = flat[:max(1, n // 16)]
        d[p].reshape(-1)[neg] = -d[p].reshape(-1)[neg] * 0.01          # a few negatives: some stay above -off, some fall below
        if n >= 3:
            d[p].reshape(-1)[flat[-1]] = np.nan
            bad[p].reshape(-1)[flat[-2]] = 1
    unit = rng.uniform(20.0, 200.0, size=planes)
    c, v = photon_params(unit, 2.9, 1.2, read_noise)
    return K, u0, d, bad, c, np.broadcast_to(v, (planes,)).copy()


# ---- the 48 x 48 case of the host tests: a smooth disc with a few compact sources, seen through the closed loop's detector ----
HOST_FWHM, HOST_RADIUS = 2.5, 8
HOST_DETECTOR = dict(unit=1000.0, exposure=2.9, dn_per_photon=1.2, read_noise=1.2)


def gaussian_psf(fwhm, radius):
    sigma = fwhm / (2.0 * np.sqrt(2.0 * np.log(2.0)))
    ax = np.arange(-radius, radius + 1, dtype=np.float64)
    k = np.exp(-(ax[:, None] ** 2 + ax[None, :] ** 2) / (2.0 * sigma * sigma))
    return k / k.sum()


def effective_kernel(psf, b):
    """Instrument.effective_kernel: the flipped PSF convolved with the bin x bin box, and its anchor."""
    kh, kw = psf.shape
    K = np.zeros((1, kh + b - 1, kw + b - 1))
    for dy in range(b):
        for dx in range(b):
            K[0, dy:dy + kh, dx:dx + kw] += psf[::-1, ::-1]
    return K, (kh // 2, kw // 2)


def host_truth(size=48):
    """[1, size, size] fp32, positive: a limb-brightened disc on a faint background with four compact sources."""
    y, x = np.mgrid[0:size, 0:size].astype(np.float64)
    cy = cx = (size - 1) / 2.0
    rr = np.hypot(y - cy, x - cx) / (0.4 * size)
    img = 0.05 + 0.6 * np.where(rr < 1.0, 0.6 + 0.4 * rr ** 2, np.exp(-(rr - 1.0) / 0.15))
    for sy, sx, amp, wid in ((0.3, 0.35, 2.0, 1.2), (0.55, 0.6, 1.5, 0.9), (0.7, 0.3, 1.0, 1.5), (0.4, 0.7, 2.5, 0.8)):
        img += amp * np.exp(-((y - sy * size) ** 2 + (x - sx * size) ** 2) / (2.0 * wid * wid))
    return img[None].astype(np.float32)


def host_case(b=1, boundary='nearest', size=48, seed=5, read_noise=None, noise=True, unit=None):
    """The observed frame of the host tests: dict(truth, d, K, anchor, scale, c, v, expected).  ``d`` is ``expected`` (the
    restatement's A truth, 'mean' binning) with Poisson counts and Gaussian read noise drawn by NumPy (``noise=False``: d =
    expected)."""
    det = dict(HOST_DETECTOR)
    if read_noise is not None:
        det['read_noise'] = read_noise
    if unit is not None:
        det['unit'] = unit
    truth = host_truth(size)
    K, anchor = effective_kernel(gaussian_psf(HOST_FWHM, HOST_RADIUS), b)
    scale = 1.0 / (b * b)
    expected = correlate_bin(truth, K, b, anchor, scale, boundary)[0]
    c, v = photon_params(det['unit'], det['exposure'], det['dn_per_photon'], det['read_noise'])
    d = expected
    if noise:
        rng = np.random.default_rng(seed)
        counts = rng.poisson(np.maximum(expected.astype(np.float64), 0.0) * c)
        dn = counts * det['dn_per_photon'] + det['read_noise'] * rng.standard_normal(expected.shape)
        d = (dn / det['exposure'] / det['unit']).astype(np.float32)
    return dict(truth=truth, d=d, K=K, anchor=anchor, scale=scale, bin=b, boundary=boundary, c=c, v=v, expected=expected)
