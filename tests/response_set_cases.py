"""The 11-channel response set and the case maker of the response-set tests (tests/test_gpu_response_set.py on the GPU,
tests/test_response_set_host.py for the conditions the cases must meet).

The set: the 7 AIA rows of golden ``g6_dt_e2e`` (codes 94 ... 335, one shared 101-node grid) and four synthetic channels with
smooth positive bumps of the AIA rows' size:
  174    2 nodes                      (one interval: both end intervals are the same one)
  10171  3 nodes                      (a second instrument's "171": shares rows with AIA's 171)
  10195  37 nodes, non-uniform, smallest spacing 0.01 dex
  20001  256 nodes from log T 6.25 up to 8.8: samples inside AIA's table (4 ... 9) lie outside it on both sides, and the
         2-, 3- and 37-node grids end below 8.8: every grid has samples of the others outside it

``make_case`` follows ``test_gpu_dt_integral.make_case``: the same density and relu patterns, one negative ``log_abs``, optical
depths 1e-3 ... 100 spread over the 11 channels, log T drawn from every grid's knots, one fp32 step outside both ends of every
grid, both end intervals of every grid and values outside all grids; wavelength rows with permuted codes, 0, -1, the unknown
1600, duplicated codes and both "171"s in one row.
"""
import functools
import math

import torch

from test_gpu_dt_integral import BASES, PIXEL, tables

AIA = (94, 131, 171, 193, 211, 304, 335)
NEW_CODES = (174, 10171, 10195, 20001)
CODES = AIA + NEW_CODES
UNKNOWN = 1600.
# optical depth along the thickest ray per channel, in set order; None: log_abs < 0, kappa = relu(log_abs) = 0, no gradient
TAUS = (1e-3, 0.03, 0.3, 3.0, None, 30.0, 100.0, 0.01, 0.1, 1.0, 10.0)
REG_RADIUS = 1.25


def _bump(x, centre, width, height, floor):
    return (height * torch.exp(-((x.double() - centre) / width) ** 2) + floor).float()


@functools.lru_cache(maxsize=None)
def synthetic_channels():
    """[(code, name, logt fp32, resp fp32)] of the four synthetic channels."""
    x2 = torch.tensor([5.5, 7.0])
    x3 = torch.tensor([5.0, 6.1, 7.3])
    steps = torch.tensor([0.01 + 0.019 * ((7 * i) % 11) for i in range(36)], dtype=torch.float64)
    x37 = (4.5 + torch.cat([torch.zeros(1, dtype=torch.float64), torch.cumsum(steps, 0)])).float()
    x256 = torch.linspace(6.25, 8.8, 256, dtype=torch.float64).float()
    assert float((x37[1:] - x37[:-1]).min()) >= 0.0099 and x37.numel() == 37
    return ((174, 'EUI 174', x2, _bump(x2, 6.0, 0.6, 3e-25, 2e-26)),
            (10171, 'EUVI-A 171', x3, _bump(x3, 5.95, 0.5, 2e-25, 1e-26)),
            (10195, 'EUVI-A 195', x37, _bump(x37, 6.2, 0.35, 4e-25, 5e-27)),
            (20001, 'hot channel', x256, _bump(x256, 7.0, 0.3, 1e-25, 1e-27)))


def channels():
    """[(code, name, logt, resp)] of all 11 channels, in set order."""
    lt, resp = tables()
    return [(c, f'AIA {c}', lt[i].clone(), resp[i].clone()) for i, c in enumerate(AIA)] + list(synthetic_channels())


def response_set():
    from sunerf_hip.response import ResponseSet
    return ResponseSet(channels())


def aia_set():
    from sunerf_hip.response import ResponseSet
    return ResponseSet(channels()[:7])


def grids():
    """The distinct log T grids of the set: AIA's and the four synthetic ones."""
    return [tables()[0][0]] + [ch[2] for ch in synthetic_channels()]


def _pool(gen):
    """log T values the edge samples are drawn from: per grid its knots, its ends and their inner neighbours twice, one fp32
    step outside both ends, points inside both end intervals; and two values outside all grids."""
    inf = torch.tensor(math.inf)
    parts = [torch.tensor([2.0, 11.5])]
    for x in grids():
        n = x.numel()
        parts += [x, x[[0, 0, 1, n - 2, n - 1, n - 1]], torch.nextafter(x[0], -inf).reshape(1).repeat(3),
                  torch.nextafter(x[-1], inf).reshape(1).repeat(3),
                  x[0] + (x[1] - x[0]) * torch.rand(4, generator=gen), x[n - 2] + (x[n - 1] - x[n - 2]) * torch.rand(4, generator=gen)]
    return torch.cat(parts)


def make_case(n, s, w, base, seed):
    gen = torch.Generator().manual_seed(seed)

    def rnd(*shape):
        return torch.rand(*shape, generator=gen)

    knots = tables()[0][0]
    b_rho, b_t = BASES[base]
    o = torch.randn(n, 3, generator=gen) * 0.3
    d = torch.nn.functional.normalize(torch.randn(n, 3, generator=gen), dim=-1) * (0.8 + 0.4 * rnd(n, 1))
    z = (0.5 + 1.5 * rnd(n, 1)) + (1.0 + 2.0 * rnd(n, 1)) * torch.sort(rnd(n, s), -1).values
    # density: relu(inf0) exactly 0 and below 0 on ~8 % of the samples
    inf0 = (1.0 if base == 'generic' else 10.0) + 0.6 * torch.randn(n, s, generator=gen)
    m = rnd(n, s)
    inf0 = torch.where(m < 0.04, torch.zeros(()), inf0)
    inf0 = torch.where((m >= 0.04) & (m < 0.08), -0.5 - rnd(n, s), inf0)
    # temperature: inside AIA's table, or (30 %, and every sample of every 5th ray) drawn from the pool of edge values; every
    # sample of another 5th of the rays from the top interval of one grid (the grids in turn) and one step beyond it
    lo, hi = knots[0], knots[100]
    pool = _pool(gen)
    inf1 = lo + 0.2 + (hi - lo - 0.4) * rnd(n, s)
    edge = (rnd(n, s) < 0.3) | (torch.arange(n) % 5 == 2)[:, None]
    inf1 = torch.where(edge, pool[torch.randint(pool.numel(), (n, s), generator=gen)], inf1)
    tops = []
    for x in grids():
        k = x.numel()
        tops.append(torch.cat([x[[k - 2, k - 1]], torch.nextafter(x[-1], torch.tensor(math.inf)).reshape(1),
                               x[k - 2] + (x[k - 1] - x[k - 2]) * rnd(13)]))
    tops = torch.stack(tops)                                   # (5, 16)
    which = (torch.arange(n) // 5) % tops.shape[0]
    top = tops[which[:, None].expand(n, s), torch.randint(tops.shape[1], (n, s), generator=gen)]
    inf1 = torch.where((torch.arange(n) % 5 == 4)[:, None], top, inf1)
    m = rnd(n, s)
    inf1 = torch.where(m < 0.02, torch.zeros(()), inf1)
    inf1 = torch.where((m >= 0.02) & (m < 0.04), -0.3 * torch.ones(()), inf1)
    raw = torch.stack([inf0 - b_rho, inf1 - b_t], -1).float().contiguous()
    # what the kernel adds up (raw + base in fp32) is the oracle's input: NeRF_DT.forward's fp32 sum
    inf = torch.stack([raw[..., 0] + b_rho, raw[..., 1] + b_t], -1)
    # wavelength rows: a random permutation of the 11 codes per ray, entries replaced by 0 / -1 / 1600 or a duplicate
    codes = torch.tensor(CODES, dtype=torch.float32)
    wl = codes[torch.argsort(rnd(n, len(CODES)), -1)[:, :w]]
    if w == 8:
        wl[wl == 131.] = UNKNOWN                     # one channel absent from every ray
    m = rnd(n, w)
    wl = torch.where(m < 0.08, torch.zeros(()), wl)
    wl = torch.where((m >= 0.08) & (m < 0.12), -torch.ones(()), wl)
    wl = torch.where((m >= 0.12) & (m < 0.16), torch.tensor(UNKNOWN), wl)
    wl = torch.where((m >= 0.16) & (m < 0.24), wl.roll(1, -1), wl).contiguous()
    if w >= 2:                                       # both instruments' 171 in one row, every 7th ray
        both = torch.arange(n) % 7 == 3
        wl[both, 0], wl[both, 1] = 171., 10171.
    # kappa_c = tau_c / (optical depth of the thickest ray at kappa = 1): channel c's optical depth reaches tau_c
    a1 = torch.trapezoid(torch.exp(torch.relu(inf[..., 0])).double(), z.double(), dim=-1).max().item() if n else 1.0
    log_abs = torch.tensor([-0.7 / a1 if t is None else t / a1 for t in TAUS])
    return {'n': n, 's': s, 'w': w, 'base': base, 'raw': raw, 'inf': inf, 'z': z.contiguous(), 'o': o, 'd': d.contiguous(),
            'wl': wl, 'log_abs': log_abs, 'vol_c': torch.tensor([0.7]), 'pixel': PIXEL[base], 'g_image': 0.25 + rnd(n, w)}


# ---- the shapes of group 1 (kernels against fp64): shared by the GPU test and the host test of the conditions ---------------
S_VALUES = (3, 31, 32, 33, 65, 300)
N_VALUES = (1, 7, 16389)
W_VALUES = (1, 3, 8)
GROUP1 = [(9, s, W_VALUES[(i + b) % 3], base) for i, s in enumerate(S_VALUES) for b, base in enumerate(('generic', 'nerf_dt'))] + \
         [(n, 33, W_VALUES[(i + b + 2) % 3], base) for i, n in enumerate(N_VALUES) for b, base in enumerate(('generic', 'nerf_dt'))]


def group1_case(n, s, w, base):
    return make_case(n, s, w, base, seed=1000 * n + 10 * s + w + (base == 'nerf_dt'))
