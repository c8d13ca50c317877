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

For the limits of the header (1 ... 64 channels, 4096 nodes; tests/test_gpu_response_set_sizes.py): ``rough_channels`` makes
sets of any size with non-uniform grids and responses drawn node by node, ``SET_NODES`` names the five sets R1, R32, R33, R64
and R64r, ``make_case(..., channels=)`` makes a case for any set and ``SIZE_CASES`` lists the shapes they are run at.
"""
import functools
import math
import random

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


def grids(channels=None):
    """The log T grids the edge samples of a case are drawn from.  Without ``channels``: the distinct grids of the 11-channel
    set, AIA's and the four synthetic ones.  With ``channels`` ([(code, name, logt, resp)]): at most six of the set's grids,
    the first, the last and the largest among them, in set order."""
    if channels is None:
        return [tables()[0][0]] + [ch[2] for ch in synthetic_channels()]
    return [torch.as_tensor(channels[i][2]) for i in pool_rows(channels)]


def pool_rows(channels):
    """The rows of ``channels`` whose grids ``grids(channels)`` returns."""
    m = len(channels)
    largest = max(range(m), key=lambda i: len(channels[i][2]))
    return sorted({0, m - 1, largest, m // 4, m // 2, (3 * m) // 4})[:6] if m > 6 else list(range(m))


def _pool(gen, channels=None):
    """log T values the edge samples are drawn from: per grid its knots, its ends and their inner neighbours twice, one fp32
    step outside both ends, points inside both end intervals; and two values outside all grids.  Of a set's grid with more than
    64 nodes, 64 knots drawn at random: the thousands of knots of one table would leave the other kinds no share of the pool."""
    inf = torch.tensor(math.inf)
    parts = [torch.tensor([2.0, 11.5])]
    for x in grids(channels):
        n = x.numel()
        knots = x if channels is None or n <= 64 else x[torch.randperm(n, generator=gen)[:64]]
        parts += [knots, x[[0, 0, 1, n - 2, n - 1, n - 1]], torch.nextafter(x[0], -inf).reshape(1).repeat(3),
                  torch.nextafter(x[-1], inf).reshape(1).repeat(3),
                  x[0] + (x[1] - x[0]) * torch.rand(4, generator=gen), x[n - 2] + (x[n - 1] - x[n - 2]) * torch.rand(4, generator=gen)]
    return torch.cat(parts)


def make_case(n, s, w, base, seed, channels=None, tau_scale=1.0):
    """A case on the 11-channel set, or on ``channels`` = [(code, name, logt, resp)] (module docstring; the wavelength rows
    of a set: :func:`set_rows`), its optical depths times ``tau_scale``."""
    gen = torch.Generator().manual_seed(seed)

    def rnd(*shape):
        return torch.rand(*shape, generator=gen)

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
    lo, hi = _inside(channels)
    pool = _pool(gen, channels)
    inf1 = lo + 0.2 + (hi - lo - 0.4) * rnd(n, s)
    edge = (rnd(n, s) < 0.3) | (torch.arange(n) % 5 == 2)[:, None]
    inf1 = torch.where(edge, pool[torch.randint(pool.numel(), (n, s), generator=gen)], inf1)
    tops = []
    for x in grids(channels):
        k = x.numel()
        tops.append(torch.cat([x[[k - 2, k - 1]], torch.nextafter(x[-1], torch.tensor(math.inf)).reshape(1),
                               x[k - 2] + (x[k - 1] - x[k - 2]) * rnd(13)]))
    tops = torch.stack(tops)                                   # (grids, 16)
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
    if channels is None:
        codes = torch.tensor(CODES, dtype=torch.float32)
        wl = codes[torch.argsort(rnd(n, len(CODES)), -1)[:, :w]]
        if w == 8:
            wl[wl == 131.] = UNKNOWN                     # one channel absent from every ray
    else:
        wl = base_rows(n, w, [ch[0] for ch in channels])
    m = rnd(n, w)
    wl = torch.where(m < 0.08, torch.zeros(()), wl)
    wl = torch.where((m >= 0.08) & (m < 0.12), -torch.ones(()), wl)
    wl = torch.where((m >= 0.12) & (m < 0.16), torch.tensor(UNKNOWN), wl)
    wl = torch.where((m >= 0.16) & (m < 0.24), wl.roll(1, -1), wl).contiguous()
    if channels is not None:
        wl = set_rows(wl, [ch[0] for ch in channels])
    elif w >= 2:                                     # both instruments' 171 in one row, every 7th ray
        both = torch.arange(n) % 7 == 3
        wl[both, 0], wl[both, 1] = 171., 10171.
    # kappa_c = tau_c / (optical depth of the thickest ray at kappa = 1): channel c's optical depth reaches tau_c
    a1 = torch.trapezoid(torch.exp(torch.relu(inf[..., 0])).double(), z.double(), dim=-1).max().item() if n else 1.0
    taus = TAUS if channels is None else set_taus(len(channels))
    log_abs = torch.tensor([-0.7 / a1 if t is None else tau_scale * t / a1 for t in taus])
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


# ---- sets at the limits of the header: 1 ... 64 channels, 4096 nodes -------------------------------------------------------------
TOP_CODE = (1 << 24) - 1                  # the largest code a set takes (exact in fp32)
FIRST_CODES = (1, TOP_CODE, TOP_CODE - 1)   # rows 0, 1, 2: the smallest code, the largest, and its neighbour one below
# the five absent values a set's rows carry besides 0, -1 and 1600; ``None``: a code of the set + 0.5 (``half_code``)
ODD_VALUES = (math.nan, math.inf, None, 16777216.0, 1e-40)


def rough_channels(node_counts, seed, avoid=()):
    """[(code, name, logt fp32, resp fp32)], one channel per entry of ``node_counts``.  Grid: start in [4, 6], length 1 ... 3 dex,
    steps with random ratios of 1 : 6.  Response: every node drawn on its own, log-uniform over one decade at the size of the AIA
    rows -- neighbouring intervals and the same interval of two rows differ by O(1), so a sample resolved to the neighbouring
    interval or to another row cannot pass the gate (smooth bumps would let it).  Codes: ``FIRST_CODES`` on rows 0, 1, 2, then
    distinct integers in [30000, 2^23) (a code + 0.5 is exact in fp32 there) outside ``avoid``."""
    gen = torch.Generator().manual_seed(seed)
    rng = random.Random(seed)
    taken = set(FIRST_CODES) | {int(UNKNOWN)} | set(avoid)
    out = []
    for i, k in enumerate(node_counts):
        code = FIRST_CODES[i] if i < 3 else rng.randrange(30000, 1 << 23)
        while i >= 3 and code in taken:
            code = rng.randrange(30000, 1 << 23)
        taken.add(code)
        start = 4.0 + 2.0 * torch.rand((), generator=gen, dtype=torch.float64)
        length = 1.0 + 2.0 * torch.rand((), generator=gen, dtype=torch.float64)
        steps = 1.0 + 5.0 * torch.rand(k - 1, generator=gen, dtype=torch.float64)
        x = (start + length * torch.cat([torch.zeros(1, dtype=torch.float64), torch.cumsum(steps, 0)]) / steps.sum()).float()
        assert x.numel() == k and bool((x[1:] > x[:-1]).all()), (i, k)
        resp = (2e-26 * 10.0 ** torch.rand(k, generator=gen, dtype=torch.float64)).float()
        out.append((code, f'rough {i}', x, resp))
    return out


SET_NODES = {'R1': [4096], 'R32': list(range(2, 34)), 'R33': list(range(2, 35)), 'R64': [64] * 64,
             'R64r': [2] * 40 + [3969] + [2] * 22 + [3]}
SET_SEEDS = {'R1': 101, 'R32': 132, 'R33': 133, 'R64': 164, 'R64r': 165}


@functools.lru_cache(maxsize=None)
def set_channels(name):
    """The channels of one of the five sets of ``SET_NODES``, fixed by its seed."""
    return tuple(rough_channels(SET_NODES[name], SET_SEEDS[name]))


def set_of(name):
    from sunerf_hip.response import ResponseSet
    return ResponseSet(list(set_channels(name)))


def set_taus(m):
    """``TAUS`` repeated with period 11: one channel in eleven with a negative ``log_abs``, optical depths 1e-3 ... 100."""
    return tuple(TAUS[i % len(TAUS)] for i in range(m))


def _inside(channels):
    """(lo, hi) of the log T range the ordinary samples of a case are drawn from (``lo + 0.2 ... hi - 0.2``).  Without
    ``channels`` AIA's table, 4 ... 9; for a set the range most of its grids cover: from the upper quartile of the grids' first
    nodes to the lower quartile of their last ones, widened by the margins the draw takes off -- or, where the two cross, the
    span of all grids."""
    if channels is None:
        knots = tables()[0][0]
        return knots[0], knots[100]
    first = torch.stack([torch.as_tensor(ch[2])[0] for ch in channels]).double()
    last = torch.stack([torch.as_tensor(ch[2])[-1] for ch in channels]).double()
    lo, hi = torch.quantile(first, 0.75) - 0.2, torch.quantile(last, 0.25) + 0.2
    if not float(hi - lo) > 0.5:
        lo, hi = first.min(), last.max()
    return lo.float(), hi.float()


def half_code(codes):
    """A value half a step above a code of the set that fp32 holds exactly: the last row's code, or row 0's."""
    return (codes[-1] if codes[-1] < (1 << 23) else codes[0]) + 0.5


def base_rows(n, w, codes):
    """(n, w) fp32: ray ``i``, column ``c`` holds the code of row ``(7 i + 9 c) mod M``."""
    row = (7 * torch.arange(n)[:, None] + 9 * torch.arange(w)[None, :]) % len(codes)
    return torch.tensor(codes, dtype=torch.float64)[row].float()


def set_rows(wl, codes):
    """The replacements a set's rows get after those of ``make_case`` (0, -1, 1600, duplicates).  With ``k = i mod 18``: ray
    ``i`` carries ``ODD_VALUES[k]`` in column 0 for ``k < 5`` and ``ODD_VALUES[k - 4]`` in the last column for ``4 <= k < 9``
    (W = 1: the one column takes ``ODD_VALUES[k]`` for ``k < 5``); the kernel must treat all five as absent.  Then, for M >= 33
    and W >= 2, every 7th ray holds the codes of rows ``m`` and ``m + 32`` -- the two codes one lane of the lookup looks at -- in
    adjacent columns, away from columns 0 and W - 1 where W allows."""
    n, w = wl.shape
    m_ch = len(codes)
    wl = wl.clone()
    odd = [half_code(codes) if v is None else v for v in ODD_VALUES]
    for i in range(n):
        k = i % 18
        if k < 5:
            wl[i, 0] = odd[k]
        if 4 <= k < 9 and w > 1:
            wl[i, w - 1] = odd[k - 4]
    if m_ch >= 33 and w >= 2:
        for j, i in enumerate(range(3, n, 7)):
            m = j % (m_ch - 32)
            c = 1 + j % (w - 3) if w >= 4 else w - 2
            wl[i, c], wl[i, c + 1] = float(codes[m]), float(codes[m + 32])
    return wl.contiguous()


# (set, rays, samples, columns, base): the smallest shapes that reach each seam (tests/test_gpu_response_set_sizes.py)
SIZE_CASES = [('R1', 9, 33, 1, 'generic'), ('R1', 9, 33, 8, 'nerf_dt'),
              ('R32', 72, 33, 8, 'generic'),
              ('R33', 72, 33, 8, 'nerf_dt'), ('R33', 9, 65, 3, 'generic'),
              ('R64', 72, 33, 8, 'generic'), ('R64', 72, 33, 8, 'nerf_dt'), ('R64', 9, 3, 8, 'generic'),
              ('R64', 9, 31, 8, 'nerf_dt'), ('R64', 9, 32, 8, 'generic'), ('R64', 72, 129, 8, 'generic'),
              ('R64', 9, 508, 8, 'generic'),
              ('R64r', 72, 129, 8, 'nerf_dt'), ('R64r', 72, 33, 3, 'generic')]
# (set, n, s, w, base) -> seed, where the default seed misses a condition of tests/test_response_set_host.py
SIZE_SEEDS = {('R33', 72, 33, 8, 'nerf_dt'): 3300,        # the default seed leaves row 32's code (two rays per column) out of column 0
              ('R33', 9, 65, 3, 'generic'): 3351}        # ... lights 13 of the 27 image entries (17 hold a code): this one 17
# Optical depths of the 3-sample case: 1e-4 ... 10.  An image of 3 samples is one or two terms exp(-A) rho^2 R; where the first
# sample lies outside the channel's grid it is the second term alone, and at A > 30 that term (R ~ 1e-25) lies below fp32's
# normal range, 1.2e-38, in the kernel and in the fp32 restatement alike: the image would measure denormal rounding (7 gate
# units between the fp32 and the fp64 restatement at depths up to 100).  Longer rays have thin terms in front.
SIZE_TAU_SCALE = {('R64', 9, 3, 8, 'generic'): 0.1}


def size_case_id(shape):
    name, n, s, w, base = shape
    return f'{name}-N{n}-S{s}-W{w}-{base}'


@functools.lru_cache(maxsize=None)
def size_case(name, n, s, w, base):
    """The case of one entry of ``SIZE_CASES``; shared (and left unchanged) by the tests that use it."""
    seed = SIZE_SEEDS.get((name, n, s, w, base), 7000 + 1000 * n + 10 * s + w + (base == 'nerf_dt') + 100000 * SET_SEEDS[name])
    return make_case(n, s, w, base, seed, channels=list(set_channels(name)),
                     tau_scale=SIZE_TAU_SCALE.get((name, n, s, w, base), 1.0))


# ---- the 11-channel set inside a 64-channel one (embedding invariance) ----------------------------------------------------------
EMBED_PERM = (3, 9, 0, 7, 10, 1, 5, 8, 2, 6, 4)       # row 53 + j of the embedding set holds channel EMBED_PERM[j] of the 11


@functools.lru_cache(maxsize=None)
def embedded_channels():
    """64 channels: ``rough_channels`` filler in rows 0 ... 52 (2 ... 114 nodes each) and the 11 channels of the existing set in
    rows 53 ... 63, in the order ``EMBED_PERM``."""
    filler = rough_channels([2 + (29 * i) % 113 for i in range(53)], seed=53, avoid=CODES)
    eleven = channels()
    return tuple(filler + [eleven[p] for p in EMBED_PERM])


# ---- smooth sets for the module-level tests (plumbing and set order, kept apart from interval selection) ------------------------
def _stepped(start, end, k, phase=0):
    """(k,) fp32 grid from ``start`` to ``end`` whose steps cycle through ratios of 1 : 3."""
    steps = torch.tensor([1.0 + 0.2 * ((7 * (j + phase)) % 11) for j in range(k - 1)], dtype=torch.float64)
    x = (start + (end - start) * torch.cat([torch.zeros(1, dtype=torch.float64), torch.cumsum(steps, 0)]) / steps.sum()).float()
    assert bool((x[1:] > x[:-1]).all())
    return x


def _smooth(grids, first_code):
    return [(first_code + 13 * i, f'smooth {i}', x,
             _bump(x, 5.9 + 0.06 * ((7 * i) % 16), 0.3 + 0.02 * (i % 11), (1 + i % 5) * 1e-25, (1 + i % 3) * 1e-27))
            for i, x in enumerate(grids)]


@functools.lru_cache(maxsize=None)
def smooth_channels_64():
    """64 channels of smooth bumps (as ``synthetic_channels``), every one on a grid of its own (2 ... 60 nodes) that contains
    log T 6.3 ... 6.65, where ``_g6_mlp(all_grids=True)`` of tests/test_gpu_response_set.py puts both models."""
    return tuple(_smooth([_stepped(4.5 + 0.025 * (i % 50), 7.0 + 0.03 * (i % 40), 2 + (5 * i) % 59, i) for i in range(64)], 50001))


@functools.lru_cache(maxsize=None)
def smooth_channels_40():
    """40 channels of smooth bumps on ONE non-uniform 100-node grid from log T 4 to 9: 4000 nodes, M > 32, and a shared grid,
    which is what ``render_dem`` takes as the DEM's default nodes."""
    x = _stepped(4.0, 9.0, 100)
    return tuple(_smooth([x.clone() for _ in range(40)], 70001))
