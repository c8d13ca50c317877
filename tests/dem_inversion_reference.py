"""float64 reference of the per-pixel DEM inversion, numpy / scipy only.

For one pixel with channel values ``y`` (M,), errors ``sigma`` (M,), response ``G`` (M, K) >= 0, prior ``p`` (K,) > 0 and
``lam`` > 0 the inversion is the unique minimiser over x >= 0 of

    1/2 sum_w ((G x - y)_w / sigma_w)^2 + lam/2 sum_k (x_k / p_k)^2.

``invert_reference`` solves it with ``scipy.optimize.nnls`` on the stacked system (Lawson-Hanson active set: independent of the
device's algorithm); ``newton_reference`` restates the device's semismooth Newton iteration on the dual in plain numpy;
``make_cases`` generates pixels from the project's own response table.
"""
import numpy as np
from scipy.optimize import nnls

AIA_SCALE = 1e17        # the generator's response rows: table x exposure time x 1e17 (the pixel factor of the tests)


def used_channels(y, sigma):
    """The channels of one pixel that take part: finite ``y``, finite ``sigma`` > 0."""
    y, sigma = np.asarray(y, dtype=np.float64), np.asarray(sigma, dtype=np.float64)
    return np.isfinite(y) & np.isfinite(sigma) & (sigma > 0)


def invert_reference(y, sigma, G, prior, lam):
    """x* (K,) of one pixel by ``nnls`` on ``[G / sigma ; sqrt(lam) diag(1 / p)] x = [y / sigma ; 0]`` over the used channels.
    No channel left: zeros."""
    y, sigma = np.asarray(y, dtype=np.float64), np.asarray(sigma, dtype=np.float64)
    G, prior = np.asarray(G, dtype=np.float64), np.asarray(prior, dtype=np.float64)
    use = used_channels(y, sigma)
    k = G.shape[1]
    if not use.any():
        return np.zeros(k)
    a = np.concatenate([G[use] / sigma[use, None], np.sqrt(float(lam)) * np.diag(1.0 / prior)])
    b = np.concatenate([y[use] / sigma[use], np.zeros(k)])
    scale = np.linalg.norm(b)      # nnls stops on an absolute tolerance: solve for a right-hand side of norm 1 (x is linear in b)
    if scale == 0:
        return np.zeros(k)
    x, _ = nnls(a, b / scale, maxiter=100 * (k + a.shape[0]))
    return x * scale


def chi2_of(x, y, sigma, G):
    """sum over the used channels of ((G x - y) / sigma)^2."""
    y, sigma = np.asarray(y, dtype=np.float64), np.asarray(sigma, dtype=np.float64)
    use = used_channels(y, sigma)
    r = (np.asarray(G, dtype=np.float64)[use] @ x - y[use]) / sigma[use]
    return float(r @ r)


def summaries(x, logt_nodes):
    """(em, logt_mean) of a DEM ``x`` (K,): sum_k x_k and sum_k x_k logT_k / em (NaN where em = 0)."""
    em = float(x.sum())
    with np.errstate(invalid='ignore', divide='ignore'):
        return em, float(np.float64(x @ np.asarray(logt_nodes, dtype=np.float64)) / np.float64(em))


def newton_reference(y, sigma, G, prior, lam, tol=1e-10, max_iter=64, v0=None, max_trials=30):
    """The device's algorithm for one pixel, in float64 numpy.

    In the whitened dual variable ``v = (y - G x) / sigma`` (the residual in units of the error), with ``Gs = G / sigma``,
    ``ys = y / sigma`` and ``x(v) = max(0, P^2 Gs^T v) / lam``, the KKT conditions are ``F(v) = v + Gs x(v) - ys = 0``, the
    gradient of the strongly convex, piecewise quadratic ``D(v) = |v|^2 / 2 + sum_k p_k^2 max(0, (Gs^T v)_k)^2 / (2 lam) -
    ys . v``.  Semismooth Newton: ``J = I + Gs_A P_A^2 Gs_A^T / lam`` over the nodes A with ``(Gs^T v)_k >= 0`` (at the start
    v = 0 that is every node: the first step is the unconstrained ridge solution), step ``d = -J^-1 F``, then a line search for
    the minimum of the convex ``phi(t) = D(v + t d)``: every trial point yields ``phi'(t) = F(v + t d) . d`` and ``phi''(t) =
    d^T J(v + t d) d``; a trial is accepted when ``|phi'(t)| <= 1e-3 |phi'(0)|`` or max |F| meets the stop, else the next trial is
    the 1-D Newton point ``t - phi' / phi''`` if it lies inside the bracket the trials have built, else the bracket's middle
    (twice t while there is no upper end).  Start at ``v0`` (default 0), stop at max |F| <= tol max |ys|, after ``max_iter``
    steps or ``max_trials`` trials of one step.  A left-out channel has Gs = 0 and ys = 0: its v stays 0 and its row of J is the
    unit row.  Returns ``(x, v, iterations, converged)``; ``newton_reference.passes`` counts the evaluations of the last call."""
    y, sigma = np.asarray(y, dtype=np.float64), np.asarray(sigma, dtype=np.float64)
    G, prior = np.asarray(G, dtype=np.float64), np.asarray(prior, dtype=np.float64)
    use = used_channels(y, sigma)
    inv_s = np.where(use, 1.0 / np.where(use, sigma, 1.0), 0.0)
    gs = G * inv_s[:, None]
    ys = np.where(use, y, 0.0) * inv_s
    p2 = prior * prior / float(lam)
    stop = tol * np.abs(ys).max() if use.any() else 0.0

    def evaluate(v):
        newton_reference.passes += 1
        t = gs.T @ v
        c = np.where(t >= 0, p2, 0.0)
        x = c * t
        return x, v + gs @ x - ys, np.eye(len(v)) + (gs * c) @ gs.T

    newton_reference.passes = 0
    v = np.zeros(len(y)) if v0 is None else np.array(v0, dtype=np.float64)
    x, f, jac = evaluate(v)
    it = 0
    while True:
        nf = np.abs(f).max()
        if nf <= stop:
            return x, v, it, True
        if it == max_iter:
            return x, v, it, False
        step = -np.linalg.solve(jac, f)
        slope = f @ step
        t, lo, hi = 1.0, 0.0, np.inf
        for _ in range(max_trials):
            x2, f2, jac2 = evaluate(v + t * step)
            g, h = f2 @ step, step @ jac2 @ step
            if abs(g) <= 1e-3 * abs(slope) or np.abs(f2).max() <= stop:
                break
            if g < 0:
                lo = t
            else:
                hi = t
            t_new = t - g / h
            if not lo < t_new < hi:
                t_new = 0.5 * (lo + hi) if hi < np.inf else 2.0 * t
            t = t_new
        else:
            return x, v, it, False
        v, x, f, jac = v + t * step, x2, f2, jac2
        it += 1


def response_rows(golden, n_channels, nodes=None):
    """Response rows (n_channels, K) float64 of fixture ``g6_dt_e2e`` (``aia_tresp x aia_exp_time``) times ``AIA_SCALE``, on
    the table's own grid or interpolated (numpy.interp, 0 outside) onto ``nodes``; more than 7 channels repeat rows."""
    lt = golden['aia_logte'][0].double().numpy()
    rows = (golden['aia_tresp'] * float(golden['aia_exp_time'])).float().double().numpy() * AIA_SCALE
    rows = rows[np.arange(n_channels) % rows.shape[0]]
    if nodes is None:
        return lt, rows
    nodes = np.asarray(nodes, dtype=np.float64)
    return nodes, np.stack([np.interp(nodes, lt, r, left=0.0, right=0.0) for r in rows])


def make_cases(golden, n, n_channels=7, n_nodes=101, seed=0):
    """``n`` generated pixels: true DEMs that are sums of 1 - 2 Gaussians in log T (centre 5.6 - 7.0, width 0.08 - 0.3,
    amplitude 10^+-1; the width at least half a cell of the grid) folded with the response, ``sigma = 0.03 y + 1e-3 max y``, seeded Gaussian noise of that size; ``y`` and
    ``sigma`` are rounded to float32 (what both sides see).  Nodes: the table's grid for 101, else ``linspace(5.5, 7.5)``
    (where the channels respond).
    Returns a dict of float64 arrays: ``y`` / ``sigma`` (n, M), ``G`` (M, K), ``nodes`` (K,), ``prior`` (K,), ``x_true``."""
    rng = np.random.default_rng(seed)
    lt = golden['aia_logte'][0].double().numpy()
    nodes = None if n_nodes == lt.shape[0] else np.linspace(5.5, 7.5, n_nodes).astype(np.float32).astype(np.float64)
    nodes, G = response_rows(golden, n_channels, nodes)
    x_true = np.zeros((n, len(nodes)))
    for i in range(n):
        for _ in range(rng.integers(1, 3)):
            centre, width, amp = rng.uniform(5.6, 7.0), rng.uniform(0.08, 0.3), 10.0 ** rng.uniform(-1, 1)
            width = max(width, 0.5 * float(np.diff(nodes).max()))      # a grid cannot hold a DEM narrower than its own cells
            x_true[i] += amp * np.exp(-0.5 * ((nodes - centre) / width) ** 2)
    clean = x_true @ G.T
    sigma = 0.03 * clean + 1e-3 * clean.max(axis=1, keepdims=True)
    y = clean + sigma * rng.standard_normal(clean.shape)
    y, sigma = y.astype(np.float32).astype(np.float64), sigma.astype(np.float32).astype(np.float64)
    flat = np.median(y / G.sum(axis=1))
    return {'y': y, 'sigma': sigma, 'G': G, 'nodes': nodes, 'prior': np.full(len(nodes), flat), 'x_true': x_true}


# ---- the cases the host test and the GPU test share -------------------------------------------------------------------------
CONFIGS = ((2, 1), (21, 2), (101, 7), (128, 8), (101, 6))        # (K, M)
LAMS = (1e-4, 1.0, 1e4)
POOL = 65                                                        # unique pixels per configuration (nnls costs 10 - 20 ms each)
# ceiling of the agreement of ``newton_reference`` with nnls on these pools, asserted by tests/test_dem_inversion_host.py (measured
# 2.1e-11 of the pixel's largest node); the GPU test derives its bound from it
HOST_WORST = 2.5e-11
_POOLS = {}


def pool(golden, n_nodes, n_channels):
    """``POOL`` generated pixels of configuration (K, M) with their ``nnls`` solutions at every lam of ``LAMS``:
    ``ref[lam] = {'dem' (P, K), 'em', 'logt_mean', 'chi2' (P,)}``, float64.  Computed once per process."""
    key = (n_nodes, n_channels)
    if key not in _POOLS:
        c = make_cases(golden, POOL, n_channels, n_nodes, seed=1000 + 10 * n_nodes + n_channels)
        c['ref'] = {lam: solve_all(c['y'], c['sigma'], c['G'], c['prior'], c['nodes'], np.full(POOL, lam)) for lam in LAMS}
        _POOLS[key] = c
    return _POOLS[key]


def solve_all(y, sigma, G, prior, nodes, lam):
    """``invert_reference`` of every row with its own ``lam[i]`` -> ``{'dem', 'em', 'logt_mean', 'chi2'}``."""
    x = np.stack([invert_reference(y[i], sigma[i], G, prior, lam[i]) for i in range(len(y))])
    sums = [summaries(xi, nodes) for xi in x]
    return {'dem': x, 'em': np.array([s[0] for s in sums]), 'logt_mean': np.array([s[1] for s in sums]),
            'chi2': np.array([chi2_of(x[i], y[i], sigma[i], G) for i in range(len(y))])}


def chi2_tolerance(ref, y, sigma, G, x_rel, out_rel):
    """Bound on |chi2 - chi2_ref| per pixel when every node of x is within ``x_rel max_k x_ref`` of the reference and the
    output is rounded to ``out_rel``: the whitened residual moves by at most dr = x_rel max x_ref |Gs 1|_2, so chi2 by
    2 sqrt(chi2_ref) dr + dr^2, plus out_rel chi2_ref."""
    tol = np.zeros(len(y))
    for i in range(len(y)):
        use = used_channels(y[i], sigma[i])
        dr = x_rel * ref['dem'][i].max() * np.linalg.norm(G[use].sum(axis=1) / sigma[i][use])
        tol[i] = 2 * np.sqrt(ref['chi2'][i]) * dr + dr * dr + out_rel * ref['chi2'][i]
    return tol
