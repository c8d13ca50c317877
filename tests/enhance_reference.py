"""NumPy fp64 restatement of include/sunerf_hip_enhance.h, written from the header operation by operation: multi-scale Gaussian
normalisation (MGN), ring statistics and the normalising radial graded filter (NRGF) -- and the error bounds the GPU tests hold the
device to, each derived from the restatement's own quantities (never from a device result).

Rounding model of the device (u = 2^-24 for fp32, u64 = 2^-53 for fp64):
* a tap sum of nt = 2 R + 1 fused multiply-adds in a fixed order is off by at most gamma = nt u (1 + small) of the sum of the
  absolute products; a row pass followed by a column pass by at most 2 gamma of G[|f|] (the second pass sums the rounded first);
* one fp32 operation (+, -, x, /, sqrt: all correctly rounded) costs u relative; ``atanf`` and ``powf`` are held to ATAN_ULPS and
  POW_ULPS units of u (the vendor's math library documents 2 and 1);
* an fp64 sum of n terms in any order is off by at most (n - 1) u64 of the sum of the absolute terms."""
import numpy as np

U32, U64 = 2.0 ** -24, 2.0 ** -53
ATAN_ULPS, POW_ULPS = 4.0, 4.0
SLACK = 1.01                       # second-order terms of every first-order bound
DEFAULT_SIGMA = (1.25, 2.5, 5.0, 10.0, 20.0, 40.0)
KEEP, MISSING = 0, 1


# ---- MGN ----------------------------------------------------------------------------------------------------------------------------
def radius_of(sigma, truncate):
    return int(truncate * sigma + 0.5)


def taps(sigma, truncate, exact=False):
    """The 2 R + 1 weights: fp64, rounded to fp32 once (``exact``: left in fp64, for the comparison with scipy)."""
    r = radius_of(sigma, truncate)
    if r == 0:
        return np.ones(1)
    j = np.arange(-r, r + 1, dtype=np.float64)
    w = np.exp(-(j * j) / (2.0 * sigma * sigma))
    return w if exact else w.astype(np.float32).astype(np.float64)


def correlate_axis(f, w, axis):
    """sum_j w_j f[. + j] along ``axis`` with edge replication."""
    r = (w.shape[0] - 1) // 2
    pad = [(0, 0)] * f.ndim
    pad[axis] = (r, r)
    g = np.pad(f, pad, mode='edge')
    n = f.shape[axis]
    out = np.zeros_like(f, dtype=np.float64)
    for j in range(2 * r + 1):
        out += w[j] * np.take(g, np.arange(j, j + n), axis=axis)
    return out


def window_sums(f, w):
    """sum_y w sum_x w f: rows first, then columns."""
    return correlate_axis(correlate_axis(f, w, f.ndim - 1), w, f.ndim - 2)


def gaussian(f, mask, w):
    """G[f] normalised over valid taps; ``mask`` 1 at a valid pixel.  0 / 0 = NaN where no tap is valid."""
    with np.errstate(invalid='ignore', divide='ignore'):
        return window_sums(np.where(mask > 0, f, 0.0) * mask, w) / window_sums(mask, w)


def validity(x, bad=None):
    ok = np.isfinite(x)
    return ok if bad is None else ok & (np.asarray(bad) == 0)


def _per_plane(v, c):
    """None, a scalar or one value per plane -> None or float32 [c]."""
    if v is None:
        return None
    v = np.asarray(v, dtype=np.float32).reshape(-1)
    return np.repeat(v, c) if v.shape[0] == 1 else v


def mgn(image, sigma=DEFAULT_SIGMA, weights=None, k=0.7, gamma=3.2, h=0.7, truncate=3.0, lo=None, hi=None, floor=None, bad=None):
    """``image`` float32 [C, H, W].  Returns ``out`` (fp64), ``lo``, ``hi`` (float32 [C]), ``state`` (int64 [C, 3]) and ``detail``:
    ``bound`` (fp64, the device's admissible error per pixel) and ``t`` ([n, C, H, W], the terms t_i)."""
    x32 = np.asarray(image, dtype=np.float32)
    c, hgt, wid = x32.shape
    n = len(sigma)
    weights = np.ones(n) if weights is None else np.asarray(weights, dtype=np.float32).astype(np.float64)
    k, h, gamma = (float(np.float32(v)) for v in (k, h, gamma))
    cf, eg = float(np.float32((1.0 - h) / n)), float(np.float32(1.0 / gamma))
    lo_in, hi_in, floor_in = _per_plane(lo, c), _per_plane(hi, c), _per_plane(floor, c)
    out = np.full(x32.shape, np.nan)
    bound = np.full(x32.shape, np.nan)
    terms = np.zeros((n,) + x32.shape)
    lo_out, hi_out = np.full(c, np.nan, dtype=np.float32), np.full(c, np.nan, dtype=np.float32)
    state = np.zeros((c, 3), dtype=np.int64)
    ok_all = validity(x32, bad)
    for p in range(c):
        ok = ok_all[p]
        state[p, 0] = (~ok).sum()
        if not ok.any():
            continue
        l32 = np.float32(x32[p][ok].min() + np.float32(0.0)) if lo_in is None else lo_in[p]
        h32 = np.float32(x32[p][ok].max() + np.float32(0.0)) if hi_in is None else hi_in[p]
        fl32 = np.float32(max(abs(l32), abs(h32))) * np.float32(2.0 ** -16) if floor_in is None else floor_in[p]
        f2 = float(np.float32(fl32 * fl32))
        lo_out[p], hi_out[p] = l32, h32
        l, hh = float(l32), float(h32)
        x = np.where(ok, x32[p].astype(np.float64), 0.0)
        m = ok.astype(np.float64)
        masked = state[p, 0] > 0
        state[p, 1], state[p, 2] = (ok & (x < l)).sum(), (ok & (x > hh)).sum()
        acc, e_acc, mag = np.zeros((hgt, wid)), np.zeros((hgt, wid)), np.zeros((hgt, wid))
        with np.errstate(invalid='ignore', divide='ignore', over='ignore'):
            for i in range(n):
                w = taps(sigma[i], truncate)
                nt = w.shape[0]
                g_tap = SLACK * nt * U32
                factor = (4.0 * g_tap + 2.0 * U32) if masked else (2.0 * g_tap + 2.0 * U32)      # numerator (and denominator); scale or quotient
                den = window_sums(m, w)
                gx, gax = window_sums(x * m, w) / den, window_sums(np.abs(x) * m, w) / den
                r = np.where(ok, x - gx, 0.0)
                e_r = np.where(ok, SLACK * (factor * gax + U32 * np.abs(r)), 0.0)
                e_sq = 2.0 * np.abs(r) * e_r + e_r * e_r + U32 * (np.abs(r) + e_r) ** 2
                v = window_sums(r * r * m, w) / den
                moved = window_sums(e_sq * m, w) / den
                e_v = moved + factor * (v + moved)
                s = np.sqrt(v + f2)
                e_a = e_v + U32 * (v + e_v + f2)
                e_s = e_a / s + U32 * (s + e_a / s)
                q = k * r / s
                e_kr = abs(k) * e_r + U32 * abs(k) * (np.abs(r) + e_r)
                s_low = s - e_s
                e_q = e_kr / s_low + np.abs(k * r) * e_s / (s * s_low)
                e_q = SLACK * (e_q + U32 * (np.abs(q) + e_q))
                t = np.where(s == 0.0, 0.0, np.arctan(q))
                e_t = e_q / (1.0 + np.maximum(np.abs(q) - e_q, 0.0) ** 2) + ATAN_ULPS * U32 * (np.pi / 2)
                e_t = np.where((s_low > 0.0) & np.isfinite(e_t), np.minimum(e_t, np.pi), np.pi)      # nothing is known below the floor
                t, e_t = np.where(ok, t, 0.0), np.where(ok, e_t, 0.0)
                terms[i, p] = t
                acc += weights[i] * t
                e_acc += abs(weights[i]) * (e_t + U32 * (np.abs(t) + e_t))
                mag += abs(weights[i]) * (np.abs(t) + e_t)
            e_acc += n * U32 * mag
            g = np.zeros((hgt, wid))
            if hh > l:
                g = np.clip((x - l) / (hh - l), 0.0, 1.0) ** eg
            e_g = SLACK * (POW_ULPS + 3.0 * eg) * U32 * g
            res = h * g + cf * acc
            e_res = abs(h) * e_g + abs(cf) * e_acc + 3.0 * U32 * (abs(h) * g + abs(cf) * (np.abs(acc) + e_acc))
        out[p] = np.where(ok, res, np.nan)
        bound[p] = np.where(ok, e_res, np.nan)
    return out, lo_out, hi_out, state, {'bound': bound, 't': terms}


# ---- rings ------------------------------------------------------------------------------------------------------------------------------
def squared_distance(shape, center):
    cy, cx = center
    dy = (np.arange(shape[0], dtype=np.float64) - cy)[:, None]
    dx = (np.arange(shape[1], dtype=np.float64) - cx)[None, :]
    return dy * dy + dx * dx, np.broadcast_to(dy, shape), np.broadcast_to(dx, shape)


def membership(shape, center, edges):
    """The ring of every pixel, -1 outside ``[edges[0], edges[-1])``: decided on squares, no root taken."""
    edges = np.asarray(edges, dtype=np.float64)
    d2, _, _ = squared_distance(shape, center)
    e2 = edges * edges
    ring = np.searchsorted(e2, d2.reshape(-1), side='right').reshape(shape) - 1
    return np.where((d2 >= e2[0]) & (d2 < e2[-1]), ring, -1)


def segments(shape, center, n_segments):
    """``(segment, undecidable)``: a pixel whose angle lies within 8 ulp of a segment boundary is undecidable."""
    _, dy, dx = squared_distance(shape, center)
    turn = (np.arctan2(dy, dx) + np.pi) / (2.0 * np.pi) * n_segments
    seg = np.minimum(np.floor(turn).astype(np.int64), n_segments - 1)
    tol = 8.0 * np.spacing(np.pi) / (2.0 * np.pi) * n_segments + 4.0 * np.spacing(float(n_segments))
    return seg, np.abs(turn - np.rint(turn)) <= tol


def radial_statistics(image, center, edges, n_segments=1, bad=None):
    """``image`` float32 [C, H, W].  Returns count (int64), mean, std, min, max (fp64) [C, R, S] and ``detail``: ``ring``, ``segment``,
    ``undecidable`` ([H, W]) and the bounds ``mean_bound``, ``std_bound`` ([C, R, S]) -- both sides' rounding, twice one side's."""
    x32 = np.asarray(image, dtype=np.float32)
    c, hgt, wid = x32.shape
    n_rings = len(edges) - 1
    ring = membership((hgt, wid), center, edges)
    seg, undecidable = segments((hgt, wid), center, n_segments) if n_segments > 1 else (np.zeros((hgt, wid), dtype=np.int64), np.zeros((hgt, wid), dtype=bool))
    bins = n_rings * n_segments
    index = np.where(ring >= 0, ring * n_segments + seg, -1)
    ok_all = validity(x32, bad)
    count = np.zeros((c, bins), dtype=np.int64)
    mean, std, mn, mx, mean_bound, std_bound = (np.full((c, bins), np.nan) for _ in range(6))
    for p in range(c):
        sel = ok_all[p] & (index >= 0)
        b, x = index[sel], x32[p][sel].astype(np.float64)
        cnt = np.bincount(b, minlength=bins)
        count[p] = cnt
        some = cnt > 0
        with np.errstate(invalid='ignore', divide='ignore'):
            m = np.bincount(b, weights=x, minlength=bins) / cnt
            a = np.bincount(b, weights=np.abs(x), minlength=bins)
            e_m = 2.0 * (cnt + 1) * U64 * a / cnt
            d = x - m[b]
            d2, d1 = np.bincount(b, weights=d * d, minlength=bins), np.bincount(b, weights=np.abs(d), minlength=bins)
            var = d2 / cnt
            sd = np.sqrt(var)
            e_var = (2.0 * (cnt + 3) * U64 * d2 + 2.0 * e_m * d1 + cnt * e_m * e_m) / cnt
            e_sd = np.where(sd > 0, np.minimum(e_var / sd, np.sqrt(e_var)), np.sqrt(e_var)) + 2.0 * U64 * sd
        low, high = np.full(bins, np.inf), np.full(bins, -np.inf)
        np.minimum.at(low, b, x)
        np.maximum.at(high, b, x)
        mean[p], std[p], mn[p], mx[p] = (np.where(some, v, np.nan) for v in (m, sd, low, high))
        mean_bound[p], std_bound[p] = np.where(some, e_m, np.nan), np.where(some, e_sd, np.nan)
    shape = (c, n_rings, n_segments)
    detail = {'ring': ring, 'segment': seg, 'undecidable': undecidable, 'mean_bound': mean_bound.reshape(shape), 'std_bound': std_bound.reshape(shape)}
    return count.reshape(shape), mean.reshape(shape), std.reshape(shape), mn.reshape(shape), mx.reshape(shape), detail


def nrgf(image, center, edges, outside=KEEP, missing=np.nan, bad=None, statistics=None):
    """Returns ``out`` (fp64 of the fp32 result), ``state`` (int64 [C, 3]), the statistics ``(count, mean, std, min, max)`` [C, R] and
    ``detail``: ``bound`` (2^-23 |want| plus the statistics' bounds carried through the quotient; 0 where the value is copied)."""
    x32 = np.asarray(image, dtype=np.float32)
    c, hgt, wid = x32.shape
    ring = membership((hgt, wid), center, edges)
    if statistics is None:
        count, mean, std, mn, mx, sdetail = radial_statistics(x32, center, edges, 1, bad)
        count, mean, std, mn, mx = (v[..., 0] for v in (count, mean, std, mn, mx))
        e_m, e_s = sdetail['mean_bound'][..., 0], sdetail['std_bound'][..., 0]
    else:
        count, mean, std = statistics
        mn = mx = None
        e_m, e_s = np.zeros(mean.shape), np.zeros(std.shape)
    ok_all = validity(x32, bad)
    out, bound = np.zeros(x32.shape), np.zeros(x32.shape)
    state = np.zeros((c, 3), dtype=np.int64)
    for p in range(c):
        ok, inside = ok_all[p], ring >= 0
        b = np.where(inside, ring, 0)
        with np.errstate(invalid='ignore', divide='ignore'):
            degenerate = (count[p][b] < 2) | ~(std[p][b] > 0)
            want = (x32[p].astype(np.float64) - mean[p][b]) / std[p][b]
            low = std[p][b] - e_s[p][b]
            e = SLACK * (e_m[p][b] + np.abs(want) * e_s[p][b]) / low + 2.0 ** -23 * np.abs(want)
            e = np.where(low > 0, e, np.inf)
        res = np.where(degenerate, 0.0, want.astype(np.float32).astype(np.float64))
        err = np.where(degenerate, 0.0, e)
        res = np.where(inside, res, x32[p].astype(np.float64) if outside == KEEP else float(np.float32(missing)))
        err = np.where(inside, err, 0.0)
        out[p], bound[p] = np.where(ok, res, np.nan), np.where(ok, err, 0.0)
        state[p] = [(~ok).sum(), (ok & ~inside).sum(), (ok & inside & degenerate).sum()]
    return out, state, (count, mean, std, mn, mx), {'bound': bound, 'ring': ring}
