"""DT radiative-transfer integral kernels (csrc/dt.hip: sunerf_dt_integral_fwd / _bwd / _bwd_full) called directly, against
``sunerf_oracle.dt_integral`` evaluated in float64 on the same fp32 inputs, at the shapes where the kernels branch.

The kernels give a ray 32 lanes that walk its samples in chunks of 32; every sequential quantity (optical depth, neighbour
terms, the backward's suffix sums, the recomputed term of the sample below a chunk) crosses a chunk seam through a scalar
carry.  The backward keeps exp(-A) of 8 rays in LDS (more than 64 KiB above S = 267, at most S = 705) and walks batches of
more than 8192 rays grid-stride.  So S runs over 3 and both sides of 32, 64, 128, 256 and 267 up to 705, and N over 1, 7,
9 and 16389 (more than two grid-stride sweeps, a partial last group).

Inputs: wavelength rows of 1, 3 and 7 columns that differ from ray to ray (permuted channels, 0, -1, the non-AIA 1600,
duplicated channels); the generic bases (0, 0) and NeRF_DT's (10, 5); relu(inf0) and relu(inf1) at and below 0; logT on
the table knots (lt[0] and lt[100] included), one fp32 step outside the table and well outside it; one negative log_abs;
absorption scaled so that the channels' optical depths along the thickest ray run from 1e-3 to 100; every 5th ray with
all its logT in the table's top interval.  The table is g6's.

Bounds, with the worst values measured on an MI355X over all cases:
  image            gate_units vs fp64, floor 2 |ref32 - ref64| (the fp32 reference's own noise)      <= 1   (0.50)
                   absent / unknown / empty channel columns exactly 0
  reg_q            bit-identical to the fp32 oracle expression
  regularization   within 2 ulp of |p| (x q, + 1 ulp) of the fp32 expression relu(|p| - R) q   (1.97 ulp; differs on
                   up to 21 % of the samples)
  weights          1e-5 relative per element                                                          (2.0e-7)
  height_map       1e-5 relative per ray                                                              (2.5e-7)
  absorption_map   1e-5 of sum_s |1 - q_s| per ray                                                    (1.6e-7)
  g_raw            per ray: max |got - ref64| / (1e-4 max_ray |ref64| + 2 |ref32 - ref64|
                   + 1e-16 max_batch |ref64|)                                                   <= 1   (0.008)
                   exactly 0 where inf0 <= 0 (component 0) / inf1 <= 0 (component 1)
  g_log_abs, g_vol_c  1e-4 relative                                                                   (1.7e-6)
                   exactly 0 where log_abs <= 0 or the channel is absent from every ray
Forward outputs and g_raw are bit-identical across reruns (g_log_abs / g_vol_c add with float atomics: not asserted).
"""
import math

import pytest
import torch

import sunerf_oracle as orc
from conftest import gate_units, load_golden

pytestmark = pytest.mark.gpu

AIA = orc.AIA_WAVELENGTHS
BASES = {'generic': (0.0, 0.0), 'nerf_dt': (10.0, 5.0)}
# images of order 1 on either base (fp32-representable factors: the kernel takes a float)
PIXEL = {'generic': float(torch.tensor(1e26)), 'nerf_dt': float(torch.tensor(1e17))}
# optical depth along a ray per channel (94 ... 335); None: log_abs < 0, kappa = relu(log_abs) = 0 and no gradient
TAUS = (1e-3, 0.03, 0.3, 3.0, None, 30.0, 100.0)
REG_RADIUS = 1.25
SCALAR_GRADIENT_REL = 1e-4      # g_log_abs / g_vol_c against fp64 (float atomics: the order of the adds is free)
CHUNK = 1024            # oracle rays per evaluation: the scalar gradients are sums over rays, added over chunks in fp64


@pytest.fixture(scope='module')
def ops():
    assert torch.cuda.is_available(), 'GPU tests need a ROCm device'
    from sunerf_hip import ops as _ops
    return _ops


_TABLES = {}


def tables():
    """g6's (logT grid, response x exposure time), both (7, 101) fp32.  All seven rows share one logT grid."""
    if not _TABLES:
        g = load_golden('g6_dt_e2e')
        _TABLES['t'] = (g['aia_logte'].contiguous(), (g['aia_tresp'] * float(g['aia_exp_time'])).float().contiguous())
    return _TABLES['t']


def make_case(n, s, w, base, seed):
    gen = torch.Generator().manual_seed(seed)

    def rnd(*shape):
        return torch.rand(*shape, generator=gen)

    lt, _ = tables()
    knots = lt[0]
    b_rho, b_t = BASES[base]
    # geometry: sample radii ~0.3 ... 5 around the regularization radius
    o = torch.randn(n, 3, generator=gen) * 0.3
    d = torch.nn.functional.normalize(torch.randn(n, 3, generator=gen), dim=-1) * (0.8 + 0.4 * rnd(n, 1))
    z = (0.5 + 1.5 * rnd(n, 1)) + (1.0 + 2.0 * rnd(n, 1)) * torch.sort(rnd(n, s), -1).values
    # density: relu(inf0) exactly 0 and below 0 on ~8 % of the samples
    inf0 = (1.0 if base == 'generic' else 10.0) + 0.6 * torch.randn(n, s, generator=gen)
    m = rnd(n, s)
    inf0 = torch.where(m < 0.04, torch.zeros(()), inf0)
    inf0 = torch.where((m >= 0.04) & (m < 0.08), -0.5 - rnd(n, s), inf0)
    # temperature: inside the table, or (30 %, and every sample of every 5th ray) drawn from the edge values; every sample of
    # another 5th of the rays from the top interval [lt[99], lt[100]] and beyond, where those rays' whole signal comes from
    lo, hi = knots[0], knots[100]
    pool = torch.cat([knots, knots[[0, 0, 1, 98, 99, 99, 100, 100]],
                      torch.nextafter(lo, torch.tensor(-math.inf)).reshape(1), torch.nextafter(hi, torch.tensor(math.inf)).reshape(1),
                      torch.tensor([2.0, 11.5]),
                      knots[99] + (knots[100] - knots[99]) * rnd(8), knots[0] + (knots[1] - knots[0]) * rnd(4)])
    inf1 = lo + 0.2 + (hi - lo - 0.4) * rnd(n, s)
    edge = (rnd(n, s) < 0.3) | (torch.arange(n) % 5 == 2)[:, None]
    inf1 = torch.where(edge, pool[torch.randint(pool.numel(), (n, s), generator=gen)], inf1)
    top = torch.cat([knots[[99, 100]], torch.nextafter(hi, torch.tensor(math.inf)).reshape(1),
                     knots[99] + (knots[100] - knots[99]) * rnd(13)])
    inf1 = torch.where((torch.arange(n) % 5 == 4)[:, None], top[torch.randint(top.numel(), (n, s), generator=gen)], inf1)
    m = rnd(n, s)
    inf1 = torch.where(m < 0.02, torch.zeros(()), inf1)
    inf1 = torch.where((m >= 0.02) & (m < 0.04), -0.3 * torch.ones(()), inf1)
    raw = torch.stack([inf0 - b_rho, inf1 - b_t], -1).float().contiguous()
    # what the kernel adds up (raw + base in fp32) is the oracle's input: NeRF_DT.forward's fp32 sum
    inf = torch.stack([raw[..., 0] + b_rho, raw[..., 1] + b_t], -1)
    # wavelength rows: a random permutation of the channels per ray, entries replaced by 0 / -1 / 1600 or a duplicate
    aia = torch.tensor(AIA, dtype=torch.float32)
    wl = aia[torch.argsort(rnd(n, 7), -1)[:, :w]]
    if w == 7:
        wl[wl == 131.] = 1600.                       # one channel absent from every ray
    m = rnd(n, w)
    wl = torch.where(m < 0.08, torch.zeros(()), wl)
    wl = torch.where((m >= 0.08) & (m < 0.12), -torch.ones(()), wl)
    wl = torch.where((m >= 0.12) & (m < 0.16), torch.tensor(1600.), wl)
    wl = torch.where((m >= 0.16) & (m < 0.24), wl.roll(1, -1), wl).contiguous()
    # kappa_c = tau_c / (optical depth of the thickest ray at kappa = 1): channel c's optical depth reaches tau_c
    a1 = torch.trapezoid(torch.exp(torch.relu(inf[..., 0])).double(), z.double(), dim=-1).max().item() if n else 1.0
    log_abs = torch.tensor([-0.7 / a1 if t is None else t / a1 for t in TAUS])
    return {'n': n, 's': s, 'w': w, 'base': base, 'raw': raw, 'inf': inf, 'z': z.contiguous(), 'o': o, 'd': d.contiguous(),
            'wl': wl, 'log_abs': log_abs, 'vol_c': torch.tensor([0.7]), 'pixel': PIXEL[base], 'g_image': 0.25 + rnd(n, w)}


def oracle(c, dtype, rest=None):
    """dt_integral + the epilogues of base_tracing.py:99-110 in ``dtype`` on the fp32 inputs of case ``c``, over chunks of rays.
    Gradients of L = sum(g_image image) [+ sum(g_reg regularization) + sum(g_weights weights) + sum(g_reg_q reg_q) with
    ``rest``] w.r.t. the inferences (= raw), the seven log_abs and vol_c, the scalar ones summed over the chunks in fp64."""
    lt, resp = (t.to(dtype) for t in tables())
    keys = ('image', 'weights', 'reg_q', 'regularization', 'dist_k', 'height_map', 'absorption_map', 'g_raw')
    out = {k: [] for k in keys}
    g_la, g_vc = torch.zeros(7, dtype=torch.float64), torch.zeros((), dtype=torch.float64)
    for a in range(0, c['n'], CHUNK):
        sl = slice(a, a + CHUNK)
        inf = c['inf'][sl].to(dtype).requires_grad_(True)
        la = [c['log_abs'][i].to(dtype).requires_grad_(True) for i in range(7)]
        vc = c['vol_c'][0].to(dtype).requires_grad_(True)
        z = c['z'][sl].to(dtype)
        f = orc.dt_integral(inf, {str(wv): t for wv, t in zip(AIA, la)}, vc, z, c['wl'][sl].to(dtype), lt, resp, c['pixel'])
        pts = orc.points_on_rays(c['o'][sl].to(dtype), c['d'][sl].to(dtype), z)
        dist = pts.pow(2).sum(-1).pow(0.5)
        q = f['regularizing_quantity']
        reg = torch.relu(dist - REG_RADIUS) * torch.relu(q)
        # |p| as the kernel forms it: (x^2 + y^2) + z^2 elementwise (no reduction kernel) and sqrt for pow(0.5)
        dist_k = ((pts[..., 0] * pts[..., 0] + pts[..., 1] * pts[..., 1]) + pts[..., 2] * pts[..., 2]).sqrt()
        loss = (f['image'] * c['g_image'][sl].to(dtype)).sum()
        if rest is not None:
            loss = loss + sum((t * rest[k][sl].to(dtype)).sum() for k, t in (('g_reg', reg), ('g_weights', f['weights']),
                                                                             ('g_reg_q', q)))
        grads = torch.autograd.grad(loss, [inf, vc] + la, allow_unused=True)
        with torch.no_grad():
            for k, v in (('image', f['image']), ('weights', f['weights']), ('reg_q', q), ('regularization', reg),
                         ('dist_k', dist_k),
                         ('height_map', (f['weights'] * dist).sum(-1)), ('absorption_map', (1 - q).sum(-1)), ('g_raw', grads[0])):
                out[k].append(v.detach())
            g_vc += grads[1].double()
            g_la += torch.stack([torch.zeros((), dtype=torch.float64) if g is None else g.double() for g in grads[2:]])
    res = {k: torch.cat(v) for k, v in out.items()}
    res.update(g_log_abs=g_la, g_vol_c=g_vc)
    return res


def make_rest(c, ref64):
    """g_reg / g_weights / g_reg_q for the full backward, scaled per ray to the size of the image part of that ray's g_raw so
    that no term hides the others: regularization and reg_q enter g_raw with factors of order 1, weights with 1 / sum q."""
    gen = torch.Generator().manual_seed(c['n'] * 1000 + c['s'])
    scale = ref64['g_raw'].abs().amax((1, 2))
    scale = torch.where(scale > 0, scale, scale[scale > 0].median() if bool((scale > 0).any()) else torch.ones(()))[:, None]
    denom = torch.relu(c['inf'][..., 0]).double().sum(1, keepdim=True) + 1e-10
    n, s = c['n'], c['s']
    return {'g_reg': (scale * 0.5 * torch.randn(n, s, generator=gen)).float(),
            'g_weights': (scale * denom * torch.randn(n, s, generator=gen)).float(),
            'g_reg_q': (scale * torch.randn(n, s, generator=gen)).float()}


def ray_units(got, ref64, ref32):
    """Per ray: max over samples and both components of |got - ref64| / (1e-4 max |ref64 of the ray| + 2 |ref32 - ref64|
    + 1e-16 max |ref64 of the batch|).
    A seam error touches one sample in 32: a norm over the batch would dilute it."""
    got = got.detach().cpu().double()
    err = (got - ref64).abs()
    # (+ 1e-16 of the batch's largest gradient: a ray whose every attenuated term underflows fp32's normal range -- optically
    # thick from its first step -- has gradients ~1e-30 of the others, made of denormals on both sides)
    bound = (1e-4 * ref64.abs().amax((1, 2), keepdim=True) + 2 * (ref32.double() - ref64).abs()
             + 1e-16 * ref64.abs().max())
    zero = bound == 0
    assert bool((err[zero] == 0).all()), 'nonzero gradient where the reference is exactly 0'
    return (err / torch.where(zero, torch.ones(()), bound)).max().item()


def ulp_of(x):
    """fp32 spacing at |x| (float64)."""
    x = x.abs()
    return torch.nextafter(x, torch.tensor(math.inf)).double() - x.double()


def scalar_rel(got, ref, must_be_zero):
    got = got.detach().cpu().double().reshape(-1)
    ref = ref.reshape(-1)
    assert bool((got[must_be_zero] == 0).all()), (got, must_be_zero)
    keep = ~must_be_zero & (ref != 0)
    assert bool((got[~must_be_zero & (ref == 0)] == 0).all())
    return ((got[keep] - ref[keep]).abs() / ref[keep].abs()).max().item() if bool(keep.any()) else 0.0


def dev_args(c):
    lt, resp = tables()
    b_rho, b_t = BASES[c['base']]
    return (c['raw'].cuda(), c['z'].cuda(), c['o'].cuda(), c['d'].cuda(), c['wl'].cuda(), lt.cuda(), resp.cuda(),
            c['log_abs'].cuda(), c['vol_c'].cuda(), b_rho, b_t, c['pixel'], REG_RADIUS)


def check_case(ops, c):
    args = dev_args(c)
    f = ops.dt_integral_fwd(*args, want_epilogues=True)
    f_again = ops.dt_integral_fwd(*args, want_epilogues=True)
    g_img = c['g_image'].cuda()
    bwd = ops.dt_integral_bwd(*args, g_img, None)
    bwd_again = ops.dt_integral_bwd(*args, g_img, None)
    torch.cuda.synchronize()
    for k in f:
        assert torch.equal(f[k], f_again[k]), f'forward {k} differs between two runs'
    assert torch.equal(bwd[0], bwd_again[0]), 'g_raw differs between two runs'

    ref64, ref32 = oracle(c, torch.float64), oracle(c, torch.float32)
    m = {}
    # ---- forward
    m['image'] = gate_units(f['image'], ref64['image'], floor=2 * (ref32['image'].double() - ref64['image']).abs())
    absent = ~torch.isin(c['wl'], torch.tensor(AIA, dtype=torch.float32))
    assert bool((f['image'].cpu()[absent] == 0).all()), 'absent / unknown channel column not exactly 0'
    assert torch.equal(f['reg_q'].cpu(), ref32['reg_q']), 'reg_q'
    # regularization = relu(|p| - R) q: within 2 ulp of |p| (times q) of the fp32 expression.  Not asserted bit for bit: the
    # reference's pow(., 0.5) is not correctly rounded on the CPU (1 ulp off on ~0.7 % of random points) and even with
    # sqrt and the kernel's association the fp32 expression differed from the kernel on the test machine
    dist, reg = ref32['dist_k'].double(), f['regularization'].cpu().double()
    reg32 = torch.relu(ref32['dist_k'] - REG_RADIUS) * ref32['reg_q']
    spacing = torch.nextafter(ref32['dist_k'], torch.tensor(math.inf)).double() - dist
    err = (reg - reg32.double()).abs()
    m['reg_ulp_of_p'] = (err / (spacing * ref32['reg_q'].double()).clamp_min(1e-300)).max().item()
    m['reg_differ'] = (err > 0).double().mean().item()
    assert bool((err <= 2 * spacing * ref32['reg_q'].double() + ulp_of(reg32)).all()), ('regularization', m)
    w_err = (f['weights'].cpu().double() - ref64['weights']).abs()
    assert bool((w_err[ref64['weights'] == 0] == 0).all())
    m['weights'] = (w_err / ref64['weights'].abs().clamp_min(1e-300)).max().item()
    m['height_map'] = ((f['height_map'].cpu().double() - ref64['height_map']).abs() / ref64['height_map'].abs()).max().item()
    q = ref64['reg_q']
    m['absorption_map'] = ((f['absorption_map'].cpu().double() - ref64['absorption_map']).abs()
                           / (1 - q).abs().sum(-1)).max().item()
    # ---- image-only backward
    inf = c['inf']
    present = torch.tensor([bool((c['wl'] == wv).any()) for wv in AIA])
    la_zero = (c['log_abs'] <= 0) | ~present
    g_raw, g_la, g_vc, absmax = bwd
    g_cpu = g_raw.cpu()
    assert bool((g_cpu[..., 0][inf[..., 0] <= 0] == 0).all()), 'g_raw[..., 0] nonzero where relu(inf0) is flat'
    assert bool((g_cpu[..., 1][inf[..., 1] <= 0] == 0).all()), 'g_raw[..., 1] nonzero where relu(inf1) is flat'
    assert absmax.view(torch.float32).item() == g_cpu.abs().max().item()
    m['g_raw'] = ray_units(g_raw, ref64['g_raw'], ref32['g_raw'])
    m['g_log_abs'] = scalar_rel(g_la, ref64['g_log_abs'], la_zero)
    m['g_vol_c'] = scalar_rel(g_vc, ref64['g_vol_c'], ~present.any().reshape(1))
    # ---- full backward: gradients arriving at regularization, weights and reg_q as well
    rest = make_rest(c, ref64)
    full64, full32 = oracle(c, torch.float64, rest)['g_raw'], oracle(c, torch.float32, rest)['g_raw']
    rd = {k: v.cuda() for k, v in rest.items()}
    full = ops.dt_integral_bwd_full(*args, g_img, rd['g_reg'], rd['g_weights'], rd['g_reg_q'])
    full_again = ops.dt_integral_bwd_full(*args, g_img, rd['g_reg'], rd['g_weights'], rd['g_reg_q'])
    torch.cuda.synchronize()
    assert torch.equal(full[0], full_again[0]), 'full g_raw differs between two runs'
    assert bool((full[0].cpu()[..., 0][inf[..., 0] <= 0] == 0).all())
    m['g_raw_full'] = ray_units(full[0], full64, full32)
    m['g_log_abs_full'] = scalar_rel(full[1], ref64['g_log_abs'], la_zero)
    m['g_vol_c_full'] = scalar_rel(full[2], ref64['g_vol_c'], ~present.any().reshape(1))

    tau = torch.trapezoid(torch.exp(torch.relu(inf[..., 0])).double() * torch.relu(c['log_abs'][-1]).double(), c['z'].double(), dim=-1)
    on_knot = torch.isin(inf[..., 1], tables()[0][0])
    print(f"N={c['n']} S={c['s']} W={c['w']} {c['base']}: " + ' '.join(f'{k} {v:.2e}' for k, v in m.items())
          + f' | optical depth (335) {tau.min().item():.1e}..{tau.max().item():.1e}, {int(on_knot.sum())} logT on knots')
    assert bool(on_knot.any()), 'no logT on a table knot'
    assert m['image'] <= 1.0, m
    assert m['weights'] <= 1e-5 and m['height_map'] <= 1e-5 and m['absorption_map'] <= 1e-5, m
    assert m['g_raw'] <= 1.0 and m['g_raw_full'] <= 1.0, m
    for k in ('g_log_abs', 'g_vol_c', 'g_log_abs_full', 'g_vol_c_full'):
        assert m[k] <= SCALAR_GRADIENT_REL, (k, m)


S_VALUES = (3, 31, 32, 33, 34, 63, 64, 65, 129, 256, 257, 300, 705)


@pytest.mark.parametrize('base', ['generic', 'nerf_dt'])
@pytest.mark.parametrize('s', S_VALUES)
def test_dt_integral_samples_per_ray(ops, s, base):
    """Chunk seams (31 ... 65, 129, 257), the >64 KiB LDS backward (300) and the largest accepted S (705); 21 rays: two full
    groups of 8 and a partial one."""
    w = (7, 3, 1)[(S_VALUES.index(s) + (base == 'nerf_dt')) % 3]
    check_case(ops, make_case(21, s, w, base, seed=s * 2 + (base == 'nerf_dt')))


@pytest.mark.parametrize('base', ['generic', 'nerf_dt'])
@pytest.mark.parametrize('n', [1, 7, 9, 16389])
def test_dt_integral_batch_sizes(ops, n, base):
    """A lone ray, one partial group, a partial second group, and 16389 rays: the backward's 1024 workgroups walk 2049 groups
    of 8 (more than two sweeps) and the last one has 5 rays."""
    check_case(ops, make_case(n, 33, 7 if base == 'generic' else 3, base, seed=n + 7 * (base == 'nerf_dt')))


def test_dt_integral_config5_shape(ops):
    """Config 5: 8192 rays x 256 samples x 7 channels on NeRF_DT's bases."""
    check_case(ops, make_case(8192, 256, 7, 'nerf_dt', seed=5))


def test_dt_integral_no_channel_present(ops):
    """Rows without a single AIA channel: image, g_log_abs and g_vol_c exactly 0."""
    c = make_case(9, 40, 3, 'generic', seed=3)
    c['wl'] = torch.tensor([0., -1., 1600.]).repeat(9, 1)
    args = dev_args(c)
    f = ops.dt_integral_fwd(*args)
    g_raw, g_la, g_vc, _ = ops.dt_integral_bwd(*args, c['g_image'].cuda(), None)
    torch.cuda.synchronize()
    assert bool((f['image'] == 0).all()) and bool((g_la == 0).all()) and bool((g_vc == 0).all())
    assert bool((g_raw == 0).all())


def _bwd_raw(ops, c, n, small):
    """sunerf_dt_integral_bwd through the C entry point, the three small outputs in caller-owned (prefilled) memory."""
    from sunerf_hip import lib as _l
    args = dev_args(c)
    raw, z, o, d, wl, lt, resp, la, vc = (t[:n] if i < 5 else t for i, t in enumerate(args[:9]))
    g_image = c['g_image'][:n].cuda()
    g_raw = torch.empty(n, c['s'], 2, device='cuda')
    dev = z.device
    _l.call(dev, 'sunerf_dt_integral_bwd', ops._ptr(raw), ops._ptr(z), ops._ptr(o), ops._ptr(d), ops._ptr(wl), c['w'],
            ops._ptr(lt), ops._ptr(resp), ops._ptr(la), ops._ptr(vc), *args[9:13], n, c['s'], ops._ptr(g_image), None,
            ops._ptr(g_raw), ops._ptr(small[0]), ops._ptr(small[1]), ops._ptr(small[2]), ops._stream(dev))
    return g_raw


def test_dt_integral_bwd_empty_batch(ops):
    """n_rays = 0 clears g_log_abs, g_vol_c and the absmax word, whether the three share one buffer or not."""
    c = make_case(1, 33, 7, 'generic', seed=1)
    joint = torch.full((9,), float('nan'), device='cuda')
    _bwd_raw(ops, c, 0, (joint[:7], joint[7:8], joint[8:9]))
    apart = [torch.full((k,), float('nan'), device='cuda') for k in (7, 1, 1)]
    _bwd_raw(ops, c, 0, apart)
    torch.cuda.synchronize()
    assert bool((joint == 0).all()), joint
    assert all(bool((t == 0).all()) for t in apart), apart
    out = ops.dt_integral_bwd(*dev_args(make_case(0, 33, 7, 'generic', seed=1)), torch.zeros(0, 7, device='cuda'), None)
    torch.cuda.synchronize()
    assert out[0].numel() == 0 and bool((out[1] == 0).all()) and bool((out[2] == 0).all()) and out[3].item() == 0


def test_dt_integral_bwd_lds_limit(ops):
    """S = 706 needs 163 848 B of LDS, more than a CU's 160 KiB: refused with SUNERF_E_UNSUPPORTED before anything is queued
    (the caller's outputs stay as they were); S = 705 (163 624 B) runs and matches the oracle in the tests above."""
    c = make_case(9, 706, 7, 'generic', seed=2)
    with pytest.raises(ValueError, match='unsupported'):
        ops.dt_integral_bwd(*dev_args(c), c['g_image'].cuda(), None)
    with pytest.raises(ValueError, match='unsupported'):
        ops.dt_integral_bwd_full(*dev_args(c), c['g_image'].cuda(), None, None, None)
    small = torch.full((9,), float('nan'), device='cuda')
    with pytest.raises(ValueError, match='unsupported'):
        _bwd_raw(ops, c, 9, (small[:7], small[7:8], small[8:9]))
    torch.cuda.synchronize()
    assert bool(torch.isnan(small).all()), 'outputs cleared although the call was refused'
    f = ops.dt_integral_fwd(*dev_args(c))                     # the forward has no LDS that grows with S
    torch.cuda.synchronize()
    assert bool(torch.isfinite(f['image']).all())
