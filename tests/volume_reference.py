"""fp64 restatements for the volume tests: the physical quantities of a field's answer from the formulas of the
reference (voxel_volume.py:47, emission.py:31-37, density_temperature.py:237-263, thompson.py:39), and the weighted, masked sums
of ``volume_metrics`` in numpy.  Inputs are taken as given (fp32 values) and everything after is float64."""
import numpy as np

AIA = (94., 131., 171., 193., 211., 304., 335.)


def response_f64(logte_row, resp_row, x):
    """Linear interpolation of one channel's response on its 101-node grid, 0 outside it (Interp1D(..., extrap=0))."""
    lt, rs, x = np.asarray(logte_row, np.float64), np.asarray(resp_row, np.float64), np.asarray(x, np.float64)
    inside = (x >= lt[0]) & (x <= lt[-1])
    i = np.clip(np.searchsorted(lt, x, side='right') - 1, 0, lt.shape[0] - 2)
    val = rs[i] + (x - lt[i]) * (rs[i + 1] - rs[i]) / (lt[i + 1] - lt[i])
    return np.where(inside, val, 0.0)


def outside(radius, r_in, r_out):
    """The mask of the kernel: the fp32 radius against the fp32 bounds; a NaN radius is outside."""
    radius = np.asarray(radius, np.float32)
    return ~((radius >= np.float32(r_in)) & (radius <= np.float32(r_out)))


def field_quantities_f64(kind, inferences, radius, r_in=1.0, r_out=np.inf, fill=np.nan, kappa=1.0, wavelengths=None,
                         logte=None, resp=None, log_abs=None):
    inf = np.asarray(inferences, np.float64)
    out = {}
    with np.errstate(over='ignore'):
        if kind == 'emission':
            out['emission'] = np.exp(inf[:, 0])
            out['absorption'] = np.maximum(inf[:, 1], 0.0)
        elif kind == 'white_light':
            out['electron_density'] = np.exp(np.float64(np.float32(kappa)) * inf[:, 0])
        else:
            rho = np.exp(np.maximum(inf[:, 0], 0.0))
            logt = np.maximum(inf[:, 1], 0.0)
            out['density'], out['log_temperature'] = rho, logt
            if wavelengths is not None:
                em = np.zeros((inf.shape[0], len(wavelengths)))
                ab = np.zeros_like(em)
                for w, wl in enumerate(wavelengths):
                    if float(wl) not in AIA:
                        continue
                    c = AIA.index(float(wl))
                    em[:, w] = rho * rho * response_f64(logte[c], resp[c], logt)
                    ab[:, w] = rho * max(float(log_abs[c]), 0.0)
                out['emissivity'], out['absorption'] = em, ab
    mask = outside(radius, r_in, r_out)
    for v in out.values():
        v[mask] = fill
    return out, mask


TERMS = ('w', 'wa', 'wb', 'wd', 'wabs', 'wd2', 'wa2', 'wb2', 'wab')


def volume_terms(a, b, weights):
    """Per-voxel terms of the nine sums (fp64, masked voxels removed), the count and max |a - b|."""
    a, b = np.asarray(a, np.float32), np.asarray(b, np.float32)
    w = weights[0][:, None, None] * weights[1][None, :, None] * weights[2][None, None, :]
    ok = np.isfinite(a) & np.isfinite(b)
    x, y, w = a[ok].astype(np.float64), b[ok].astype(np.float64), np.asarray(w, np.float64)[ok]
    d = x - y
    terms = {'w': w, 'wa': w * x, 'wb': w * y, 'wd': w * d, 'wabs': w * np.abs(d), 'wd2': w * (d * d), 'wa2': w * (x * x),
             'wb2': w * (y * y), 'wab': w * (x * y)}
    return terms, int(ok.sum()), (float(np.abs(d).max()) if d.size else 0.0)


def weighted_statistics(a, b, weights):
    """me, mae, rmse, pearson, means straight from their definitions (two-pass, numpy fp64)."""
    terms, count, max_abs = volume_terms(a, b, weights)
    ok = np.isfinite(np.asarray(a, np.float32)) & np.isfinite(np.asarray(b, np.float32))
    x, y, w = np.asarray(a, np.float64)[ok], np.asarray(b, np.float64)[ok], terms['w']
    sw = w.sum()
    ma, mb = (w * x).sum() / sw, (w * y).sum() / sw
    d = x - y
    cov = (w * (x - ma) * (y - mb)).sum()
    return {'me': (w * d).sum() / sw, 'mae': (w * np.abs(d)).sum() / sw, 'rmse': np.sqrt((w * d * d).sum() / sw),
            'pearson': cov / np.sqrt((w * (x - ma) ** 2).sum() * (w * (y - mb) ** 2).sum()), 'mean_a': ma, 'mean_b': mb,
            'max_abs': max_abs, 'count': count}
