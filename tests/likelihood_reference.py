"""fp64 NumPy restatement of include/sunerf_hip_likelihood.h: the Gaussian noise likelihood of the detector model with per-row gains.
The reference project has no such loss, so this file is the yardstick of tests/test_likelihood_host.py (which holds its gradients to
central finite differences) and of tests/test_gpu_likelihood.py.  Written from the header's formulas on whole arrays: every slot
is evaluated and masked ones are multiplied out, sums are ``numpy.sum`` over the flattened arrays (pairwise, nothing like the
kernel's wave, workgroup and ticket order)."""
import numpy as np

OBSERVED, MODEL = 0, 1


def variance(x, noise_rows):
    """``(max(x, 0) U E G + R^2 + extra_var) / (U E)^2`` with the scalars of ``noise_rows`` [..., 8] broadcast against ``x``."""
    unit, exposure, gain, read, extra = (noise_rows[..., k] for k in range(5))
    return (np.maximum(x, 0.0) * unit * exposure * gain + read * read + extra) / (unit * exposure) ** 2


def rows_of(codes, row_codes, shape):
    """(row [N, W] int, -1 where the code is no row; positive [N, W] bool)."""
    if codes is None:
        return np.zeros(shape, dtype=np.int64), np.ones(shape, dtype=bool)
    codes = np.asarray(codes, dtype=np.float32)
    table = np.asarray(row_codes, dtype=np.float32)
    hit = codes[..., None] == table
    row = np.where(hit.any(-1), hit.argmax(-1), -1)
    with np.errstate(invalid='ignore'):
        positive = codes > 0
    return row, positive


def terms(p, t, gain, slope, s2_dark, mode):
    """(term, d term / d m, m, magnitude of the derivative's terms) of predictions ``p`` against targets ``t``; ``slope`` is
    G / (U E), ``s2_dark`` the variance of a dark pixel plus floor^2."""
    m = gain * p
    d = m - t
    if mode == OBSERVED:
        s2 = np.maximum(t, 0.0) * slope + s2_dark
        return d * d / s2, 2.0 * d / s2, m, np.abs(2.0 * d / s2)
    s2 = np.maximum(m, 0.0) * slope + s2_dark
    open_ = (m > 0.0).astype(np.float64)
    q = d * d / s2
    extra = open_ * slope * (1.0 - q) / s2
    return q + np.log(s2), 2.0 * d / s2 + extra, m, np.abs(2.0 * d / s2) + open_ * slope * (1.0 + q) / s2


def evaluate(coarse, fine, target, codes, row_codes, noise, log_gain, mode, reg=None, lambda_image=1.0, lambda_regularization=1.0,
             finite_check=()):
    """Every output of ``sunerf_likelihood_loss`` in fp64, and the gradients of the loss itself:

    g_coarse, g_fine, g_log_gain, channel_stats, stats   as the header lays them out (gradients of the SUM of terms)
    loss                                                  stats[0]
    d_coarse, d_fine, d_log_gain, d_reg                   d loss / d input (``lambda_image / n_valid`` applied)
    m_coarse, m_fine                                      magnitudes of the terms of d_coarse and d_fine (for relative bounds)
    """
    coarse, fine, target = (np.asarray(a, dtype=np.float32).astype(np.float64) for a in (coarse, fine, target))
    noise = np.asarray(noise, dtype=np.float64)
    log_gain32 = np.asarray(log_gain, dtype=np.float32)
    n_rows = noise.shape[0]
    row, positive = rows_of(codes, row_codes, coarse.shape)
    finite_t = np.isfinite(target)
    valid = positive & (row >= 0) & finite_t
    unknown = positive & (row < 0)
    r = np.where(row >= 0, row, 0)
    par = noise[r]
    gain = np.exp(log_gain32.astype(np.float64))[r]
    slope = par[..., 2] / (par[..., 0] * par[..., 1])
    s2_dark = (par[..., 3] ** 2 + par[..., 4]) / (par[..., 0] * par[..., 1]) ** 2 + par[..., 5] ** 2
    t = np.where(finite_t, target, 0.0)
    w = valid.astype(np.float64)
    with np.errstate(all='ignore'):
        term_c, dm_c, m_c, mag_c = terms(np.where(valid, coarse, 0.0), t, gain, slope, s2_dark, mode)
        term_f, dm_f, m_f, mag_f = terms(np.where(valid, fine, 0.0), t, gain, slope, s2_dark, mode)
    # non-finite predictions at valid slots are counted and reach the sums; the tests' parity inputs hold none
    bad = int((valid & ~np.isfinite(coarse)).sum() + (valid & ~np.isfinite(fine)).sum())
    term_c, term_f = np.where(valid, term_c, 0.0), np.where(valid, term_f, 0.0)
    g_coarse, g_fine = w * dm_c * gain, w * dm_f * gain
    per_slot_gain = w * (dm_c * m_c + dm_f * m_f)
    sq = w * (m_f - t) ** 2
    channel_stats = np.zeros((n_rows, 4))
    g_log_gain = np.zeros(n_rows)
    magnitude = np.zeros((n_rows, 5))          # sums of magnitudes: what a summation-order allowance is relative to
    for k in range(n_rows):
        sel = valid & (row == k)
        channel_stats[k] = [sel.sum(), term_c[sel].sum(), term_f[sel].sum(), sq[sel].sum()]
        g_log_gain[k] = per_slot_gain[sel].sum()
        magnitude[k] = [sel.sum(), np.abs(term_c[sel]).sum(), np.abs(term_f[sel]).sum(), sq[sel].sum(),
                        (np.abs(dm_c * m_c) + np.abs(dm_f * m_f))[sel].sum()]
    n_valid = int(valid.sum())
    mean_c = term_c.sum() / n_valid if n_valid else 0.0
    mean_f = term_f.sum() / n_valid if n_valid else 0.0
    reg64 = None if reg is None else np.asarray(reg, dtype=np.float32).astype(np.float64)
    n_reg = 0 if reg64 is None else reg64.size
    reg_mean = reg64.sum() / n_reg if n_reg else 0.0
    if n_reg:
        bad += int((~np.isfinite(reg64)).sum())
    for extra in finite_check:
        bad += int((~np.isfinite(np.asarray(extra, dtype=np.float64))).sum())
    lam, lam_r = float(np.float32(lambda_image)), float(np.float32(lambda_regularization))
    loss = lam * (mean_c + mean_f) + lam_r * reg_mean
    with np.errstate(divide='ignore'):
        psnr = -10.0 * np.log10(sq.sum() / n_valid) if n_valid else 0.0
    stats = np.array([loss, mean_c, mean_f, reg_mean, psnr, bad, n_valid, int(unknown.sum())], dtype=np.float64)
    scale = lam / max(n_valid, 1)
    return {'g_coarse': g_coarse, 'g_fine': g_fine, 'g_log_gain': g_log_gain, 'channel_stats': channel_stats, 'stats': stats,
            'loss': loss, 'd_coarse': g_coarse * scale, 'd_fine': g_fine * scale, 'd_log_gain': g_log_gain * scale,
            'd_reg': None if reg64 is None else np.full(reg64.shape, lam_r / n_reg if n_reg else 0.0),
            'm_coarse': w * mag_c * gain * scale, 'm_fine': w * mag_f * gain * scale, 'magnitude': magnitude, 'valid': valid}


def loss_parts_fp64(coarse, fine, target, codes, row_codes, noise, log_gain, mode, reg=None, lambda_image=1.0,
                    lambda_regularization=1.0):
    """``(parts [N, W], regularization term)`` with fp64 inputs taken as they are (no rounding to fp32 on the way in): the loss is
    ``parts.sum() + term``, slot by slot, so that a finite difference of ONE slot's share is not drowned in the rounding of the
    whole sum."""
    coarse, fine, target = (np.asarray(a, dtype=np.float64) for a in (coarse, fine, target))
    noise = np.asarray(noise, dtype=np.float64)
    row, positive = rows_of(codes, row_codes, coarse.shape)
    finite_t = np.isfinite(target)
    valid = positive & (row >= 0) & finite_t
    r = np.where(row >= 0, row, 0)
    par = noise[r]
    gain = np.exp(np.asarray(log_gain, dtype=np.float64))[r]
    slope = par[..., 2] / (par[..., 0] * par[..., 1])
    s2_dark = (par[..., 3] ** 2 + par[..., 4]) / (par[..., 0] * par[..., 1]) ** 2 + par[..., 5] ** 2
    t = np.where(finite_t, target, 0.0)
    parts = np.zeros(coarse.shape)
    for p in (coarse, fine):
        parts = parts + np.where(valid, terms(np.where(valid, p, 0.0), t, gain, slope, s2_dark, mode)[0], 0.0)
    n_valid = int(valid.sum())
    reg_mean = 0.0 if reg is None or np.size(reg) == 0 else np.asarray(reg, dtype=np.float64).mean()
    return parts * (lambda_image / max(n_valid, 1)), lambda_regularization * reg_mean


def make_case(n, w, m, seed, with_codes=True, masked=True):
    """Inputs of a parity case: every ray draws its own codes from a table of ``m`` rows; at most a quarter of the slots are
    masked (code 0, NaN target, unknown code); predictions and targets include values at and below 0; per-row noise scalars
    and gains differ.  Returns a dict of fp32 / fp64 arrays."""
    rng = np.random.default_rng([n, w, m, seed])
    row_codes = (np.sort(rng.choice(np.arange(90, 2000), size=m, replace=False)) if m > 1 else np.array([171])).astype(np.float32)
    noise = np.zeros((m, 8))
    noise[:, 0] = rng.uniform(5.0, 80.0, m)           # unit
    noise[:, 1] = rng.uniform(0.5, 3.0, m)            # exposure
    noise[:, 2] = rng.uniform(0.5, 2.0, m)            # dn_per_photon
    noise[:, 3] = rng.uniform(0.8, 3.0, m)            # read_noise
    noise[:, 4] = np.where(rng.random(m) < 0.5, 1.0 / 12.0, 0.0)
    noise[:, 5] = rng.uniform(0.0, 0.02, m)           # floor
    log_gain = rng.uniform(-0.4, 0.4, m).astype(np.float32)
    truth = rng.uniform(0.0, 2.0, (n, w)) * 10.0 ** rng.integers(-2, 2, (n, w))
    coarse = (truth * rng.uniform(0.6, 1.5, (n, w))).astype(np.float32)
    fine = (truth * rng.uniform(0.8, 1.25, (n, w))).astype(np.float32)
    target = (truth + rng.normal(0.0, 0.05, (n, w)) * (1.0 + truth)).astype(np.float32)
    edge = rng.random((n, w))
    coarse[edge < 0.05] = 0.0
    fine[(edge >= 0.05) & (edge < 0.10)] *= -1.0
    target[(edge >= 0.10) & (edge < 0.15)] = 0.0
    target[(edge >= 0.15) & (edge < 0.20)] *= -0.5
    codes = None
    if with_codes:
        codes = row_codes[rng.integers(0, m, (n, w))]
    if masked:
        chosen = rng.permutation(n * w)[:(n * w) // 4]          # a quarter of the slots, rounded down, in three kinds
        kinds = np.array_split(chosen, 3)
        target.reshape(-1)[kinds[0]] = np.nan
        if with_codes:
            codes.reshape(-1)[kinds[1]] = 0.0
            codes.reshape(-1)[kinds[2]] = 2500.0          # positive, in no table
    reg = rng.uniform(0.0, 1.0, n * 3).astype(np.float32)
    return {'coarse': coarse, 'fine': fine, 'target': target, 'codes': codes, 'row_codes': row_codes, 'noise': noise,
            'log_gain': log_gain, 'reg': reg}
