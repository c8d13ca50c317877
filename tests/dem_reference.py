"""float64 numpy restatement of the line-of-sight DEM (include/sunerf_hip.h: sunerf_dem_integral), the reference of
tests/test_dem_host.py and tests/test_gpu_dem.py.  Independent of the kernel: plain loops over rays, numpy's searchsorted.

Input is what the kernel adds up itself -- ``inf = fp32(raw + base)`` -- as in tests/test_gpu_dt_integral.py, so that the
comparison is about the integral and not about the rounding of that sum."""
import numpy as np


def trapezoid_weights(z):
    """(N, P) weights of the trapezoid rule on the points z (N, P): sum(w * y) = trapezoid(y, z).  P = 1: a single 0."""
    z = np.asarray(z, dtype=np.float64)
    w = np.zeros_like(z)
    d = np.diff(z, axis=1)
    w[:, :-1] += d / 2
    w[:, 1:] += d / 2
    return w


def dem_reference(inf, z, nodes, log_abs=None, rays_o=None, rays_d=None, r_range=(0.0, np.inf)):
    """``inf`` (N, S, 2) = raw + base, ``z`` (N, S), ``nodes`` (K,) strictly increasing, ``log_abs``: None or a number.
    Returns float64 ``dem`` (N, K), ``em``, ``logt_mean``, ``column`` (N,) and the per-sample ``v`` (N, S-1), ``logt`` (N, S-1),
    ``inside`` (N, S-1; the sample deposits) and ``radius`` (N, S-1; None without rays)."""
    inf = np.asarray(inf, dtype=np.float64)
    z = np.asarray(z, dtype=np.float64)
    nodes = np.asarray(nodes, dtype=np.float64)
    n, s = z.shape
    k = nodes.shape[0]
    assert s >= 2 and k >= 2 and bool((np.diff(nodes) > 0).all())
    rho = np.exp(np.maximum(inf[..., 0], 0.0))
    logt = np.maximum(inf[..., 1], 0.0)[:, :s - 1]
    q = trapezoid_weights(z[:, :s - 1])
    kappa = 0.0 if log_abs is None else max(float(log_abs), 0.0)
    ab = rho * kappa
    # A_{j+1} = cumulative_trapezoid(ab, z)[j], j = 0..S-2: the attenuation of quadrature point j (the render's index shift)
    A = np.cumsum((ab[:, 1:] + ab[:, :-1]) * np.diff(z, axis=1) / 2, axis=1)
    t = np.exp(-A)
    r_in, r_out = float(r_range[0]), float(r_range[1])
    radius = None
    m = np.ones((n, s - 1), dtype=bool)
    if not (r_in <= 0 and r_out == np.inf):
        p = np.asarray(rays_o, dtype=np.float64)[:, None, :] + np.asarray(rays_d, dtype=np.float64)[:, None, :] * z[:, :s - 1, None]
        radius = np.sqrt((p ** 2).sum(-1))
        with np.errstate(invalid='ignore'):
            m = (radius >= r_in) & (radius <= r_out)
    rho_q = rho[:, :s - 1]
    v = np.where(m, q * t * rho_q ** 2, 0.0)
    column = np.where(m, q * rho_q, 0.0).sum(1)
    em = v.sum(1)
    with np.errstate(invalid='ignore', divide='ignore'):
        logt_mean = (v * logt).sum(1) / em
    inside = (logt >= nodes[0]) & (logt <= nodes[-1])
    idx = np.clip(np.searchsorted(nodes, logt, side='right') - 1, 0, k - 2)
    f = (logt - nodes[idx]) / (nodes[idx + 1] - nodes[idx])
    dem = np.zeros((n, k))
    for r in range(n):
        sel = inside[r]
        np.add.at(dem[r], idx[r][sel], (v[r] * (1 - f[r]))[sel])
        np.add.at(dem[r], idx[r][sel] + 1, (v[r] * f[r])[sel])
    return {'dem': dem, 'em': em, 'logt_mean': logt_mean, 'column': column, 'v': v, 'logt': logt, 'inside': inside & m,
            'radius': radius}


# ---- inputs of the direct-op tests -------------------------------------------------------------------------------------------
BASE = (10.0, 5.0)          # NeRF_DT's base offsets


def make_case(n, s, nodes, seed, all_inside=False):
    """Rays like tests/test_gpu_dt_integral.py's ``make_case`` on the log T grid ``nodes`` (K,) float32 (numpy arrays out):
    inf0 ~ 10 +- 0.6 with ~8 % of the samples at relu(inf0) = 0 (exactly 0 or below); log T inside the grid, on knots (first and
    last included), one fp32 step outside on either side, well outside (2.0, 11.5), exactly 0 and below 0; every sample of the
    rays 2, 7, ... outside the grid and of the rays 4, 9, ... in the top interval.  ``all_inside``: every log T strictly inside.
    ``raw`` = fp32(inf - base); ``inf`` = fp32(raw + base) is what the kernel adds up and the reference takes."""
    import math
    import torch
    gen = torch.Generator().manual_seed(seed)

    def rnd(*shape):
        return torch.rand(*shape, generator=gen)

    knots = torch.as_tensor(nodes, dtype=torch.float32)
    k = knots.numel()
    o = torch.randn(n, 3, generator=gen) * 0.3
    d = torch.nn.functional.normalize(torch.randn(n, 3, generator=gen), dim=-1) * (0.8 + 0.4 * rnd(n, 1))
    z = (0.5 + 1.5 * rnd(n, 1)) + (1.0 + 2.0 * rnd(n, 1)) * torch.sort(rnd(n, s), -1).values
    inf0 = 10.0 + 0.6 * torch.randn(n, s, generator=gen)
    m = rnd(n, s)
    inf0 = torch.where(m < 0.04, torch.zeros(()), inf0)
    inf0 = torch.where((m >= 0.04) & (m < 0.08), -0.5 - rnd(n, s), inf0)
    lo, hi = knots[0], knots[-1]
    below, above = torch.nextafter(lo, torch.tensor(-math.inf)).reshape(1), torch.nextafter(hi, torch.tensor(math.inf)).reshape(1)
    span = hi - lo
    inf1 = lo + 0.05 * span + 0.9 * span * rnd(n, s)
    if not all_inside:
        pool = torch.cat([knots, knots[[0, 0, 1, k - 2, k - 1, k - 1]], below, above, torch.tensor([2.0, 11.5]),
                          knots[k - 2] + (knots[k - 1] - knots[k - 2]) * rnd(8), knots[0] + (knots[1] - knots[0]) * rnd(4)])
        edge = rnd(n, s) < 0.3
        inf1 = torch.where(edge, pool[torch.randint(pool.numel(), (n, s), generator=gen)], inf1)
        outside = torch.cat([below, above, torch.tensor([2.0, 11.5])])
        inf1 = torch.where((torch.arange(n) % 5 == 2)[:, None], outside[torch.randint(outside.numel(), (n, s), generator=gen)], inf1)
        top = torch.cat([knots[[k - 2, k - 1]], knots[k - 2] + (knots[k - 1] - knots[k - 2]) * rnd(14)])
        inf1 = torch.where((torch.arange(n) % 5 == 4)[:, None], top[torch.randint(top.numel(), (n, s), generator=gen)], inf1)
        m = rnd(n, s)
        plain = (torch.arange(n) % 5 != 4)[:, None]
        inf1 = torch.where((m < 0.02) & plain, torch.zeros(()), inf1)
        inf1 = torch.where((m >= 0.02) & (m < 0.04) & plain, -0.3 * torch.ones(()), inf1)
    raw = torch.stack([inf0 - BASE[0], inf1 - BASE[1]], -1).float().contiguous()
    inf = torch.stack([raw[..., 0] + BASE[0], raw[..., 1] + BASE[1]], -1)
    # optical depth of the thickest ray at kappa = 1
    a1 = float(torch.trapezoid(torch.exp(torch.relu(inf[..., 0])).double(), z.double(), dim=-1).max()) if n else 1.0
    return {'n': n, 's': s, 'nodes': knots.numpy(), 'raw': raw.numpy(), 'inf': inf.numpy(), 'z': z.contiguous().numpy(),
            'o': o.numpy(), 'd': d.contiguous().numpy(), 'tau1': a1}


def add_mask(c, margin=1e-4):
    """A radius mask for case ``c`` that cuts some samples of some rays, every sample of ray 1 (moved far away) and, through a
    NaN direction, every sample of ray 3.  The two radii sit in gaps of the samples' own radii, at least ``margin`` (relative)
    from any sample, so that fp32 and fp64 agree on every decision.  Returns a copy of ``c`` with ``r_range`` set."""
    c = dict(c)
    o, d = c['o'].copy(), c['d'].copy()
    if c['n'] >= 2:
        o[1] = (50.0, 0.0, 0.0)
    if c['n'] >= 4:
        d[3] = np.nan
    p = o.astype(np.float64)[:, None, :] + d.astype(np.float64)[:, None, :] * c['z'].astype(np.float64)[:, :-1, None]
    radii = np.sort(np.sqrt((p ** 2).sum(-1)).reshape(-1))
    radii = radii[np.isfinite(radii) & (radii < 40.0)]

    def gap_near(frac):
        i = int(frac * (radii.size - 1))
        for j in list(range(i, radii.size - 1)) + list(range(i - 1, -1, -1)):
            if radii[j + 1] - radii[j] > 4 * margin * radii[j + 1]:
                return float(np.float32(0.5 * (radii[j] + radii[j + 1])))
        return float(np.float32(radii[0] * 0.5 if frac < 0.5 else radii[-1] * 2))
    c.update(o=o, d=d, r_range=(gap_near(0.25), gap_near(0.8)) if radii.size >= 2 else (0.5 * float(radii[0]), 30.0))
    return c


def log_abs_of(c, mode):
    """None, a negative scalar (kappa = relu = 0) or the scalar that gives the thickest ray an optical depth of 3."""
    return {'none': None, 'negative': float(np.float32(-0.7 / c['tau1'])), 'thick': float(np.float32(3.0 / c['tau1']))}[mode]


def grid_nodes(k, table_grid=None, uniform=True, seed=0):
    """(K,) float32 nodes: the table's own grid for K = its length, else K nodes spanning log T 5.5 ... 7.5, uniform or with
    random steps."""
    if uniform and table_grid is not None and k == len(table_grid):
        return np.asarray(table_grid, dtype=np.float32)
    if uniform:
        return np.linspace(5.5, 7.5, k).astype(np.float32)
    steps = 0.2 + np.random.default_rng(seed).random(k - 1)
    x = np.concatenate([[0.0], np.cumsum(steps)])
    nodes = (5.5 + 2.0 * x / x[-1]).astype(np.float32)
    assert bool((np.diff(nodes) > 0).all())
    return nodes
