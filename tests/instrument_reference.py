"""fp64 NumPy restatement of the three kernels of include/sunerf_hip_instrument.h, exactly as the header words them (the order of
every operation included; NumPy never fuses a multiply with an add), for tests/test_instrument_host.py and
tests/test_gpu_instrument.py.

Beside its values :func:`noise` records, per element, the smallest relative margin of every comparison it decided: ``u > s`` of the
inversion, ``V <= vr``, ``us`` against 0.07 and 0.013 and the log test of PTRS, the tie of ``rint`` and ``dn >= saturation``.  exp,
log, lgamma and cos of another implementation differ from NumPy's in their last bits, so an element whose margin is below
``MARGIN`` may legitimately be decided the other way; a case is chosen so that no element is (the tests assert the count is 0).
A margin is |a - b| over the larger of |a| and |b|; for the log test, where ``lam``, ``k log lam`` and ``lgamma(k + 1)`` cancel, over
the larger of that and 2^-10 of the largest term of either side (a few ulps of that term are 1e-15 of it: below ``MARGIN`` times
the scale by a factor of a thousand); for ``rint`` the distance of ``dn`` from the nearest half-integer over ``max(|dn|, 1)``.
``rint`` and ``dn >= saturation`` are recorded only with READ: without the read noise ``dn`` is made of +, * and an integer ``n``
alone and has the same bits everywhere, exact ties included (those are then a check of half-to-even)."""
import numpy as np
from scipy.special import gammaln

M0, M1 = 0xD2511F53, 0xCD9E8D57
W0, W1 = 0x9E3779B9, 0xBB67AE85
MASK = np.uint64(0xFFFFFFFF)
POISSON, READ, QUANTISE, SATURATE = 1, 2, 4, 8
MAX_ROUNDS = 256
MARGIN = 1e-9
TWO52 = 4503599627370496.0


def philox(ctr, key0, key1):
    """Philox4x32-10 of counters [n, 4] (uint32) under one key, or per-counter keys [n]: [n, 4] uint32."""
    c = [np.asarray(ctr)[..., k].astype(np.uint64) for k in range(4)]
    k0, k1 = np.asarray(key0).astype(np.uint64), np.asarray(key1).astype(np.uint64)
    for _ in range(10):
        p0, p1 = np.uint64(M0) * c[0], np.uint64(M1) * c[2]
        c = [(p1 >> np.uint64(32)) ^ c[1] ^ k0, p1 & MASK, (p0 >> np.uint64(32)) ^ c[3] ^ k1, p0 & MASK]
        k0, k1 = (k0 + np.uint64(W0)) & MASK, (k1 + np.uint64(W1)) & MASK
    return np.stack(c, -1).astype(np.uint32)


def _uniform53(hi, lo):
    return ((hi >> np.uint32(5)).astype(np.float64) * 67108864.0 + (lo >> np.uint32(6)).astype(np.float64) + 1.0) * 2.0 ** -53


def uniforms(e, j, stream, seed):
    """(u_a, u_b) of block(e, j, stream): ``e`` uint64 [n], ``j`` scalar or [n]."""
    e = np.asarray(e, dtype=np.uint64)
    ctr = np.stack([e & MASK, e >> np.uint64(32), np.broadcast_to(np.asarray(j, dtype=np.uint64), e.shape),
                    np.full(e.shape, stream, dtype=np.uint64)], -1)
    seed = int(seed)
    w = philox(ctr, seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF)
    return _uniform53(w[:, 0], w[:, 1]), _uniform53(w[:, 2], w[:, 3])


def _margin(a, b, scale=None):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    s = np.maximum(np.abs(a), np.abs(b)) if scale is None else scale
    with np.errstate(invalid='ignore', divide='ignore'):
        m = np.abs(a - b) / s
    return np.where(np.isfinite(m), m, np.inf)


def poisson(lam, e, seed):
    """n ~ Poisson(lam) per element (lam finite, >= 0): (n, smallest margin, rounds used; 0 rounds for the inversion)."""
    lam = np.asarray(lam, dtype=np.float64)
    e = np.asarray(e, dtype=np.uint64)
    n = np.zeros(lam.shape)
    margin = np.full(lam.shape, np.inf)
    rounds = np.zeros(lam.shape, dtype=np.int64)
    small = lam < 10.0
    if small.any():
        idx = np.nonzero(small)[0]
        l = lam[idx]
        u = uniforms(e[idx], 0, 0, seed)[0]
        k = np.zeros(l.shape)
        p = np.exp(-l)
        s = p.copy()
        mg = np.full(l.shape, np.inf)
        live = np.ones(l.shape, dtype=bool)
        while True:
            mg = np.where(live, np.minimum(mg, _margin(u, s)), mg)
            live = live & (u > s) & (k < 200.0)
            if not live.any():
                break
            k = np.where(live, k + 1.0, k)
            with np.errstate(divide='ignore', invalid='ignore'):
                p = np.where(live, p * (l / np.where(live, k, 1.0)), p)
            s = np.where(live, s + p, s)
        n[idx], margin[idx] = k, mg
    big = ~small
    if big.any():
        idx = np.nonzero(big)[0]
        l = lam[idx]
        slam, loglam = np.sqrt(l), np.log(l)
        b = 0.931 + 2.53 * slam
        a = -0.059 + 0.02483 * b
        invalpha = 1.1239 + 1.1328 / (b - 3.4)
        vr = 0.9277 - 3.6224 / (b - 2.0)
        out = np.rint(l)
        mg = np.full(l.shape, np.inf)
        used = np.zeros(l.shape, dtype=np.int64)
        todo = np.arange(l.shape[0])
        for j in range(MAX_ROUNDS):
            if todo.size == 0:
                break
            t = todo
            ua, V = uniforms(e[idx][t], j, 0, seed)
            U = ua - 0.5
            us = 0.5 - np.abs(U)
            with np.errstate(divide='ignore', invalid='ignore'):
                k = np.floor(((2.0 * a[t]) / us + b[t]) * U + l[t] + 0.43)
                m = np.minimum(_margin(us, 0.07), _margin(V, vr[t]))
                quick = (us >= 0.07) & (V <= vr[t])
                m = np.minimum(m, np.where(quick, np.inf, np.minimum(_margin(us, 0.013), _margin(V, us))))
                skip = ~quick & ((k < 0.0) | ((us < 0.013) & (V > us)))
                test = ~quick & ~skip
                kk = np.where(test, k, 1.0)
                t1, t2, t3 = np.log(V), np.log(invalpha[t]), np.log(a[t] / (us * us) + b[t])
                r1, r2 = kk * loglam[t], gammaln(kk + 1.0)
                lhs = (t1 + t2) - t3
                rhs = (-l[t] + r1) - r2
                scale = np.maximum.reduce([np.abs(t1), np.abs(t2), np.abs(t3), l[t], np.abs(r1), np.abs(r2)])
                scale = np.maximum.reduce([np.abs(lhs), np.abs(rhs), scale * 2.0 ** -10])
                m = np.minimum(m, np.where(test, _margin(lhs, rhs, scale), np.inf))
                accept = quick | (test & (lhs <= rhs))
            mg[t] = np.minimum(mg[t], m)
            used[t] = j + 1
            out[t[accept]] = k[accept]
            todo = t[~accept]
        n[idx], margin[idx], rounds[idx] = out, mg, used
    return n, margin, rounds


def normal(e, seed):
    ua, ub = uniforms(e, 0, 1, seed)
    return np.sqrt(-2.0 * np.log(ua)) * np.cos(6.283185307179586 * ub)


def noise(expected, params, seed, index_offset=0, flags=POISSON | READ):
    """The header's sunerf_instrument_noise on ``expected`` [P, H, W] fp32 with ``params`` [P, 8] fp64.  Returns a dict of [P, H, W]
    arrays: image, sigma (fp32), saturated (uint8), and in fp64 lam, n, z, dn (before the unit round trip), margin; ``valid`` marks
    the elements whose lam is finite and <= 2^52."""
    x = np.asarray(expected, dtype=np.float32)
    par = np.asarray(params, dtype=np.float64)
    shape = x.shape
    px = shape[1] * shape[2]
    flat = x.reshape(-1).astype(np.float64)
    plane = np.arange(flat.size) // max(px, 1)
    unit, exposure, g, rn, ped, satur = (par[plane, k] for k in range(6))
    e = np.uint64(index_offset) + np.arange(flat.size, dtype=np.uint64)
    with np.errstate(all='ignore'):
        v = flat * unit
        v = np.where(v < 0.0, 0.0, v)
        lam = (v * exposure) / g
        valid = np.abs(lam) <= TWO52
        safe = np.where(valid, lam, 0.0)
        margin = np.full(flat.shape, np.inf)
        if flags & POISSON:
            n, margin, _ = poisson(safe, e, seed)
        else:
            n = safe
        dn = n * g + ped
        z = np.zeros(flat.shape)
        if flags & READ:
            z = normal(e, seed)
            dn = dn + rn * z
        if flags & QUANTISE:
            if flags & READ:
                tie = np.abs(np.abs(dn - np.floor(dn)) - 0.5)
                margin = np.minimum(margin, tie / np.maximum(np.abs(dn), 1.0))
            dn = np.rint(dn)
        sat = np.zeros(flat.shape, dtype=np.uint8)
        if flags & SATURATE:
            if flags & READ:
                margin = np.minimum(margin, _margin(dn, satur))
            hit = dn >= satur
            sat = hit.astype(np.uint8)
            dn = np.where(hit, satur, dn)
        image = ((dn - ped) / exposure) / unit
        q = 1.0 / 12.0 if flags & QUANTISE else 0.0
        sigma = (np.sqrt((lam * (g * g) + rn * rn) + q) / exposure) / unit
        image = np.where(valid, image, np.nan).astype(np.float32)
        sigma = np.where(valid, sigma, np.nan).astype(np.float32)
        sat = np.where(valid, sat, 0).astype(np.uint8)
        margin = np.where(valid, margin, np.inf)
    r = lambda t: t.reshape(shape)          # noqa: E731
    return {'image': r(image), 'sigma': r(sigma), 'saturated': r(sat), 'lam': r(lam), 'n': r(np.where(valid, n, np.nan)),
            'z': r(z), 'dn': r(np.where(valid, dn, np.nan)), 'margin': r(margin), 'valid': r(valid)}


def correlate_bin(img, K, bin_factor, anchor, scale=1.0, boundary='zero'):
    """The header's strided correlation of ``img`` [P, H, W] fp32 with ``K`` [1 or P, kh, kw] fp64: [P, H // b, W // b] fp32, the taps
    in the header's order, the first product starting the sum."""
    img = np.asarray(img, dtype=np.float32)
    K = np.asarray(K, dtype=np.float64)
    K = K[None] if K.ndim == 2 else K
    p_, h, w = img.shape
    kh, kw = K.shape[1:]
    b = int(bin_factor)
    ay, ax = anchor
    oh, ow = h // b, w // b
    rows = np.arange(oh) * b - ay
    cols = np.arange(ow) * b - ax
    acc = np.full((p_, oh, ow), -0.0)
    x = img.astype(np.float64)
    with np.errstate(all='ignore'):
        for i in range(kh):
            y = rows + i
            for j in range(kw):
                xx = cols + j
                if boundary == 'nearest':
                    tap = x[:, np.clip(y, 0, h - 1)][:, :, np.clip(xx, 0, w - 1)]
                else:
                    tap = x[:, np.clip(y, 0, h - 1)][:, :, np.clip(xx, 0, w - 1)]
                    inside = ((y >= 0) & (y < h))[:, None] & ((xx >= 0) & (xx < w))[None, :]
                    tap = np.where(inside[None], tap, 0.0)
                wgt = K[:, i, j][:, None, None] if K.shape[0] == p_ and p_ > 1 else K[0, i, j]
                acc = acc + wgt * tap
        return (scale * acc).astype(np.float32), acc


def chi_square_poisson(counts_of, lam):
    """Chi-square p-value of sampled counts against scipy.stats.poisson(lam): bins over [ppf(1e-9), ppf(1 - 1e-9)] with both tails
    merged in, neighbours merged until each expects at least 5."""
    from scipy import stats
    n = np.asarray(counts_of).reshape(-1)
    total = n.size
    lo, hi = int(stats.poisson.ppf(1e-9, lam)), int(stats.poisson.ppf(1 - 1e-9, lam))
    ks = np.arange(lo, hi + 1)
    prob = stats.poisson.pmf(ks, lam)
    prob[0] += stats.poisson.cdf(lo - 1, lam)
    prob[-1] += stats.poisson.sf(hi, lam)
    obs = np.bincount(np.clip(n, lo, hi).astype(np.int64) - lo, minlength=ks.size).astype(np.float64)
    exp = prob * total
    merged_o, merged_e = [], []
    o_acc = e_acc = 0.0
    for o, x in zip(obs, exp):
        o_acc, e_acc = o_acc + o, e_acc + x
        if e_acc >= 5.0:
            merged_o.append(o_acc)
            merged_e.append(e_acc)
            o_acc = e_acc = 0.0
    if e_acc > 0.0 or o_acc > 0.0:
        if merged_e:
            merged_o[-1] += o_acc
            merged_e[-1] += e_acc
        else:
            merged_o.append(o_acc)
            merged_e.append(e_acc)
    merged_o, merged_e = np.array(merged_o), np.array(merged_e)
    if merged_e.size < 2:
        return 1.0 if merged_o.sum() == total else 0.0, merged_e.size
    stat = float(((merged_o - merged_e) ** 2 / merged_e).sum())
    return float(stats.chi2.sf(stat, merged_e.size - 1)), merged_e.size


DIST_SEED = 2024
DIST_E0 = 5 * 2 ** 18
DIST_N = 2 ** 18
DIST_LAMS = (0.05, 3.0, 9.99, 10.0, 37.5, 1e4)
DIST_GATE = 1e-4
