"""Emission / absorption integral kernels against ``sunerf_oracle.emission_outputs`` evaluated in float64 on the same fp32 inputs:
the stand-alone forward and backward (csrc/render_bwd.hip: sunerf_emission_integral_fwd / _bwd) and the epilogue fused behind the
MLP in the render kernel (csrc/render_fwd.hip), at the shapes where the kernels branch and in the regimes where fp32 runs out.
The two forwards take the integral's per-chunk step from one text, csrc/emission_sweep.h (``test_fused_integral_is_the_stand_alone_integral``);
sweep 1 of the backward keeps the same arithmetic in its own text.

The kernels give a ray 32 lanes that walk its samples in chunks of 32; the transmittance, the previous z and the backward's
suffix sum cross a chunk seam through a scalar carry, and the g_weights path reduces sum(em) and sum(g_weights em) over all
chunks.  The backward keeps three floats per sample of 8 rays in LDS: more than 64 KiB from S = 673, at most S = 1696 (S = 1697
is refused), and walks batches of more than 2048 workgroups x 8 rays = 16384 grid-stride.  So S runs over 2, 3, both sides of
32, 64, 672 / 673 and up to 1696, N over 1, 7, 8, 9 at every S and 16384 ... 32771 at a few.

Cases (``make_case``): every ray has one kind -- transparent (relu(r1) = 0 everywhere, exact 0.0 and -0.0 included), thin
(tau 1e-6 ... 1e-3 per sample), moderate (tau 0.01 ... 1, 1 ... 30 along the ray), tau ~ 23 (a ~ the + 1e-10), opaque (runs of
tau >= 104 where expf gives 0 and the transmittance underflows through the subnormals to 0; for S > 32 across the seam at 32),
dark (raw0 <= -30: sum em below the + 1e-10 of the denominators), bright (raw0 up to 60).  Every ray also has r1 = +-0 and
r1 < 0 samples, duplicate z (every third ray z0 == z1), |d| from 0.25 to 4 and sample radii on both sides of REG_RADIUS.

Bounds, with the worst values measured on an MI355X over all cases:
  image, height_map  gate_units vs fp64, floor 2 |ref32 - ref64|                                   <= 1    (image 0.064, fused 0.015; height_map 0.004)
  absorption_map     the same, floor + S 6e-8 (a sum of fp32 differences 1 - a)                  <= 1    (0.10)
  weights, absorption, regularization   per element |got - ref64| / (REL |ref64| + 2 |ref32 - ref64|
                     + 1e-7 max_ray |ref64| [+ 2^-22 (relu(|p| - R) + |p| (1 - a)) for regularization])   <= 1
                     (weights 0.58, absorption 0.50, regularization 0.21).
                     REL = 1e-5.  The 1e-7 term: a subnormal transmittance carries no more bits than that.  The
                     regularization term: |p| and 1 - a are fp32 quantities the kernel forms with its own association and
                     expf; 2 ulp of each (the fp32 reference's |p| is pow(sum of squares, 0.5)).
  g_raw              per ray: max |got - ref64| / (1e-4 max_ray |ref64| + 2 |ref32 - ref64|
                     + 1e-16 max_batch |ref64| + fp32_floor)                                     <= 1    (0.54)
                     fp32_floor: 2^-22 of the terms that cancel in the g_weights and regularization paths (see
                     ``fp32_floor``).  Without it a ray whose weight sits on one sample (w -> 1: d weights / d raw0 ~ 1 - w,
                     below fp32's resolution of its terms) measured 9 and up to 8e3 -- the fp32 reference rounds those terms
                     in another order and cannot define the value there.
                     exactly 0 where r1 <= 0 (component 1)
  absmax             the bit pattern of max |g_raw| exactly; reset per call; 0 for N = 0
Forward outputs and g_raw are bit-identical across reruns and do not depend on where a ray sits in the batch.
"""
import pytest
import torch

import sunerf_oracle as orc
from conftest import gate_units

pytestmark = pytest.mark.gpu

REG_RADIUS = 1.0
REL = 1e-5
G_REG_CONST = 0.37
KINDS = ('transparent', 'thin', 'moderate', 'tau23', 'opaque', 'dark', 'bright')
CONFIGS = ('image', 'weights', 'absorption', 'reg', 'reg_const', 'all')
REF_CHUNK = 4096        # rays per oracle evaluation on the GPU (large batches)


# ---- cases (no GPU needed: tests/test_emission_oracle_host.py checks the regimes they claim) ----------------------------
def make_case(n, s, seed):
    """Deterministic rays, z and raw of ``n`` x ``s`` samples, ray i of kind KINDS[(i + seed) % 7]; see the module docstring."""
    gen = torch.Generator().manual_seed(seed)
    f64 = dict(dtype=torch.float64)

    def rnd(*shape):
        return torch.rand(*shape, generator=gen, **f64)

    kind = (torch.arange(n) + seed) % len(KINDS)
    # geometry: |d| log-uniform in 0.25 ... 4, unnormalised; o = -215 d + b e (e a unit vector normal to d, impact parameter b
    # < 1.4) -- z around 215 reaches the sun as the observer rays do, sample radii sqrt(((z - 215) |d|)^2 + b^2) across R = 1
    dhat = torch.nn.functional.normalize(torch.randn(n, 3, generator=gen, **f64), dim=-1)
    e = torch.nn.functional.normalize(torch.cross(dhat, torch.randn(n, 3, generator=gen, **f64), dim=-1), dim=-1)
    mag = 0.25 * 16.0 ** rnd(n, 1)
    d = (mag * dhat).float()
    o = (-215.0 * d.double() + 1.4 * rnd(n, 1) * e).float()
    lo, hi = 213.7 + 0.6 * rnd(n, 1), 216.3 - 0.6 * rnd(n, 1)
    z = torch.sort((lo + (hi - lo) * rnd(n, s)).float(), -1).values
    k = kind[:, None].expand(n, s)
    # samples that carry a kind's regime: the opaque runs (for S > 32 across the seam at 32) and, on tau23 rays, sample S/2 and
    # a few random ones
    opq = torch.zeros(n, s, dtype=torch.bool)
    if s > 32:
        opq[:, min(30, s - 5):min(35, s)] = True
        opq[:, 2] = True
    else:
        a0 = max(0, min(s // 2 - 3, s - 5))
        opq[:, a0:a0 + 5] = True
    opq &= k == KINDS.index('opaque')
    t23 = (rnd(n, s) < 0.05) | (torch.arange(s) == s // 2)
    t23 &= k == KINDS.index('tau23')
    special = opq | t23
    # duplicate z: z0 == z1 on every third ray (not on opaque / tau23 ones), z_i == z_{i-1} on ~4 % of the other samples
    dup = rnd(n, s) < 0.04
    if s > 2:
        dup |= torch.arange(s) == 2 + (5 * torch.arange(n)[:, None]) % (s - 2)
    dup &= ~special
    dup[:, :2] = False
    z = torch.where(dup, z.roll(1, -1), z)
    zeq = ((torch.arange(n) + seed) % 3 == 0) & (kind != KINDS.index('opaque')) & (kind != KINDS.index('tau23'))
    z[zeq, 1] = z[zeq, 0]
    # tau per sample -> r1 = tau / dist, dist as the kernel forms it (to within fp32 rounding)
    dz = z[:, 1:].double() - z[:, :-1].double()
    dist = torch.cat([dz[:, :1], dz], -1) * d.double().norm(dim=-1, keepdim=True)
    log_u = lambda a, b: 10.0 ** (a + (b - a) * rnd(n, s))              # noqa: E731
    cum = 1.0 + 29.0 * rnd(n, 1)
    tau = (cum / s * (0.5 + rnd(n, s))).clamp(0.01, 1.0)                 # moderate: the base of every kind but thin
    tau = torch.where(k == KINDS.index('thin'), log_u(-6, -3), tau)
    r1 = torch.where(dist > 0, tau / dist, -1.0 + 6.0 * rnd(n, s))
    # relu edge: r1 = +0.0 / -0.0 / negative on ~5 % each and on two samples of every ray; every sample of a transparent ray
    m = rnd(n, s)
    ray = torch.arange(n)[:, None]
    transparent = k == KINDS.index('transparent')
    pos0 = (torch.arange(s) == (7 * ray) % s) | (m < 0.05) | (transparent & (m < 0.3))
    neg0 = (torch.arange(s) == (7 * ray + 1) % s) | ((m >= 0.05) & (m < 0.1)) | (transparent & (m >= 0.3) & (m < 0.6))
    r1 = torch.where(transparent, -3.0 * rnd(n, s), r1)
    r1 = torch.where((m >= 0.1) & (m < 0.15), -rnd(n, s), r1)
    r1 = torch.where(pos0, torch.zeros((), **f64), r1)
    r1 = torch.where(neg0 & ~pos0, torch.tensor(-0.0, **f64), r1)
    # the regimes last: nothing above overwrites them (no duplicate z there)
    r1 = torch.where(t23 & (dist > 0), (22.5 + rnd(n, s)) / dist, r1)
    r1 = torch.where(opq & (dist > 0), (104.0 + 200.0 * rnd(n, s)) / dist, r1)
    r0 = -3.0 + 6.0 * rnd(n, s)
    r0 = torch.where(k == KINDS.index('dark'), -45.0 + 15.0 * rnd(n, s), r0)
    r0 = torch.where(k == KINDS.index('bright'), 20.0 + 40.0 * rnd(n, s), r0)
    r0[kind == KINDS.index('bright'), s // 2] = 60.0
    raw = torch.stack([r0, r1], -1).float().contiguous()
    return {'n': n, 's': s, 'seed': seed, 'kind': kind, 'raw': raw, 'z': z.contiguous(), 'o': o.contiguous(),
            'd': d.contiguous()}


def claims(c):
    """The regimes case ``c`` must contain (what the kinds present and S allow)."""
    present = {KINDS[i] for i in c['kind'].tolist()}
    out = set()
    if c['n'] * c['s'] >= 60:
        out.update(('r1 == +0 and -0', 'duplicate z'))
    if 'opaque' in present:
        out.add('tau >= 104')
        if c['s'] >= 8:
            out.add('T == 0 in fp32')
        if c['s'] > 32:
            out.add('tau >= 104 across the seam at 32')
    if 'dark' in present:
        out.add('sum em < 1e-10')
    if 'tau23' in present:
        out.add('tau ~ 23')
    if bool(((torch.arange(c['n']) + c['seed']) % 3 == 0).any()):
        out.update(('z0 == z1', 'duplicate z'))
    if c['n'] >= 7:
        out.update(('every kind', 'radii on both sides of R'))
    return out


def regimes_found(c):
    """The regimes case ``c`` does contain, measured on its fp32 inputs."""
    raw, z, d = c['raw'], c['z'], c['d']
    r1 = raw[..., 1]
    dz = torch.cat([z[:, 1:2] - z[:, :1], z[:, 1:] - z[:, :-1]], -1)
    tau = torch.relu(r1).double() * dz.double() * d.double().norm(dim=-1, keepdim=True)
    f32 = orc.emission_outputs(raw, z, c['o'], d, REG_RADIUS)
    T = orc.cumprod_exclusive(f32['regularizing_quantity'] + 1e-10)
    em64 = orc.emission_outputs(raw.double(), z, c['o'], d, REG_RADIUS)['image']
    radius = f32['points'].double().norm(dim=-1)
    found = set()
    if bool(((r1 == 0) & torch.signbit(r1)).any()) and bool(((r1 == 0) & ~torch.signbit(r1)).any()):
        found.add('r1 == +0 and -0')
    if bool((z[:, 1:] == z[:, :-1]).any()):
        found.add('duplicate z')
    if bool((z[:, 1] == z[:, 0]).any()):
        found.add('z0 == z1')
    if bool((tau >= 104).any()):
        found.add('tau >= 104')
    if c['s'] > 32 and bool(((tau[:, 31] >= 104) & (tau[:, 32] >= 104)).any()):
        found.add('tau >= 104 across the seam at 32')
    if bool((T == 0).any()):
        found.add('T == 0 in fp32')
    if bool((em64 < 1e-10).any()):
        found.add('sum em < 1e-10')
    if bool(((tau > 22) & (tau < 24)).any()):
        found.add('tau ~ 23')
    if set(c['kind'].tolist()) == set(range(len(KINDS))):
        found.add('every kind')
    if bool((radius < REG_RADIUS).any()) and bool((radius > REG_RADIUS).any()):
        found.add('radii on both sides of R')
    return found


def upstream(c):
    """Gradients arriving at the five outputs: g_image with random sign, zero on every 5th ray and divided by the ray's image
    where that exceeds 1 (bright rays: g_raw of order 1 everywhere, so no ray's gradient hides the others behind the batch
    term of the bound); g_weights, g_absorption and g_reg standard normal."""
    gen = torch.Generator().manual_seed(c['seed'] + 99)
    n, s = c['n'], c['s']
    image = orc.emission_integral(c['raw'].double(), c['z'].double(), c['d'].double())['image'][:, 0]
    sign = torch.where(torch.rand(n, generator=gen) < 0.5, -1.0, 1.0).double()
    g_image = sign * (0.5 + torch.rand(n, generator=gen).double()) / image.clamp_min(1.0)
    g_image[torch.arange(n) % 5 == 1] = 0.0
    return {'g_image': g_image.float(), 'g_weights': torch.randn(n, s, generator=gen),
            'g_absorption': torch.randn(n, s, generator=gen), 'g_reg': torch.randn(n, s, generator=gen)}


def _loss(out, g, config, dt):
    terms = {'image': lambda: (out['image'][:, 0] * g['g_image'].to(dt)).sum(),
             'weights': lambda: (out['weights'] * g['g_weights'].to(dt)).sum(),
             'absorption': lambda: (out['regularizing_quantity'] * g['g_absorption'].to(dt)).sum(),
             'reg': lambda: (out['regularization'] * g['g_reg'].to(dt)).sum(),
             'reg_const': lambda: G_REG_CONST * out['regularization'].sum()}
    if config == 'all':
        return terms['image']() + terms['weights']() + terms['absorption']() + terms['reg']()
    return terms[config]()


FWD_KEYS = ('image', 'weights', 'regularizing_quantity', 'height_map', 'absorption_map', 'regularization', 'points')


def oracle(c, g, dtype, device='cpu', configs=CONFIGS):
    """emission_outputs in ``dtype`` on ``device`` over chunks of rays: the forward outputs and d/d raw for each config."""
    res = {k: [] for k in FWD_KEYS + tuple('g_' + k for k in configs)}
    step = REF_CHUNK if device != 'cpu' else max(c['n'], 1)
    for a in range(0, c['n'], step):
        sl = slice(a, a + step)
        raw = c['raw'][sl].to(device=device, dtype=dtype).requires_grad_(True)
        z, o, d = (c[k][sl].to(device) for k in ('z', 'o', 'd'))
        out = orc.emission_outputs(raw, z, o, d, REG_RADIUS)
        gs = {k: v[sl].to(device) for k, v in g.items()}
        for cfg in configs:
            res['g_' + cfg].append(torch.autograd.grad(_loss(out, gs, cfg, dtype), raw, retain_graph=True)[0].detach())
            if dtype == torch.float64:
                res.setdefault('floor_' + cfg, []).append(fp32_floor(out, raw.detach(), z, d, gs, cfg))
        for k in FWD_KEYS:
            res[k].append(out[k].detach())
    return {k: torch.cat(v) for k, v in res.items()}


def fp32_floor(out, raw, z, d, g, cfg):
    """What fp32 cannot resolve in g_raw (float64, (N, S, 2)): 2^-22 of the terms that cancel before they are summed.
    g_weights: d weights / d em_i = (g_w,i - sum_k g_w,k w_k) / D cancels to ~(1 - w_i) of its terms when one sample carries
    the ray (w_i -> 1: a lone emitting sample, a dark ray's 1e-10 in D), and the suffix sums of the r1 component carry that
    rounding along the ray; the fp32 reference rounds in another order, so 2 |ref32 - ref64| does not cover it.
    Regularization: relu(|p| - R) cancels near |p| = R, and |p| is an fp32 quantity (2 ulp)."""
    floor = torch.zeros_like(raw)
    dz = z[:, 1:].double() - z[:, :-1].double()
    dist = torch.cat([dz[:, :1], dz], -1) * d.double().norm(dim=-1, keepdim=True)
    a = out['regularizing_quantity']
    slope = dist * a / (a + 1e-10) * (raw[..., 1] > 0)          # |d g_raw1 / d ga|
    if cfg in ('weights', 'all'):
        w, gw = out['weights'], g['g_weights'].double()
        gi = g['g_image'].double().abs()[:, None] if cfg == 'all' else 0.0
        # em_k (|g_image| + |g_w,k| / D + |sum g_w w| / D), D = image + 1e-10, em_k = w_k D
        big = w * ((out['image'] + 1e-10) * gi + gw.abs() + (gw * w).sum(-1, keepdim=True).abs())
        floor[..., 0] += 2.0 ** -22 * big
        floor[..., 1] += 2.0 ** -22 * slope * (big.flip(-1).cumsum(-1).flip(-1) - big)
    if cfg in ('reg', 'reg_const', 'all'):
        gr = g['g_reg'].double().abs() if cfg != 'reg_const' else G_REG_CONST
        floor[..., 1] += 2.0 ** -22 * out['points'].norm(dim=-1) * gr * slope
    return floor


# ---- measures ---------------------------------------------------------------------------------------------------------------
def ray_units(got, ref64, ref32, floor=0.0):
    """Per ray: max over samples and both components of |got - ref64| / (1e-4 max |ref64 of the ray| + 2 |ref32 - ref64|
    + 1e-16 max |ref64 of the batch| + floor).  A seam error touches one sample in 32: a norm over the batch would dilute it."""
    got, ref32 = got.detach().to(ref64.device).double(), ref32.to(ref64.device).double()
    err = (got - ref64).abs()
    bound = 1e-4 * ref64.abs().amax((1, 2), keepdim=True) + 2 * (ref32 - ref64).abs() + 1e-16 * ref64.abs().max() + floor
    zero = bound == 0
    assert bool((err[zero] == 0).all()), 'nonzero gradient where the reference is exactly 0'
    return (err / torch.where(zero, torch.ones((), dtype=bound.dtype, device=bound.device), bound)).max().item()


def elem_units(got, ref64, ref32, extra=None):
    """Per element: |got - ref64| / (REL |ref64| + 2 |ref32 - ref64| + 1e-7 max_ray |ref64| [+ extra])."""
    got, ref32 = got.detach().to(ref64.device).double(), ref32.to(ref64.device).double()
    err = (got - ref64).abs()
    bound = REL * ref64.abs() + 2 * (ref32 - ref64).abs() + 1e-7 * ref64.abs().amax(-1, keepdim=True)
    if extra is not None:
        bound = bound + extra
    zero = bound == 0
    assert bool((err[zero] == 0).all()), 'nonzero value where the reference is exactly 0'
    return (err / torch.where(zero, torch.ones((), dtype=bound.dtype, device=bound.device), bound)).max().item()


def reg_extra(ref32):
    """2 ulp (2^-22 relative) of |p| and of 1 - a, the fp32 quantities regularization = relu(|p| - R) (1 - a) is formed from."""
    p = ref32['points'].double().norm(dim=-1)
    q = ref32['regularizing_quantity'].double()
    return 2.0 ** -22 * (torch.relu(p - REG_RADIUS) + p * (1 - q))


def fwd_units(got, ref64, ref32, s):
    """{output: units} of image / weights / absorption [/ height_map / absorption_map / regularization] (those in ``got``)."""
    dev = ref64['image'].device

    def gate(k, floor=0.0):
        r64, r32 = ref64[k].reshape(-1), ref32[k].reshape(-1).to(dev).double()
        g = got[k].detach().reshape(-1).to(dev).double()
        return gate_units(g.cpu(), r64.cpu(), floor=(2 * (r32 - r64).abs() + floor).cpu())

    m = {'image': gate('image'),
         'weights': elem_units(got['weights'], ref64['weights'], ref32['weights']),
         'absorption': elem_units(got['absorption'], ref64['regularizing_quantity'], ref32['regularizing_quantity'])}
    if 'height_map' in got:
        m['height_map'] = gate('height_map')
        m['absorption_map'] = gate('absorption_map', floor=s * 6e-8)
        m['regularization'] = elem_units(got['regularization'], ref64['regularization'], ref32['regularization'],
                                         extra=reg_extra(ref32).to(dev))
    return m


@pytest.fixture(scope='module')
def ops():
    assert torch.cuda.is_available(), 'GPU tests need a ROCm device'
    from sunerf_hip import ops as _ops
    return _ops


def dev_inputs(c):
    return c['raw'].cuda(), c['z'].cuda(), c['d'].cuda()


def run_bwd(ops, c, g, config):
    """The stand-alone backward for one upstream-gradient config -> (g_raw, absmax as float32)."""
    raw, z, d = dev_inputs(c)
    kw = {'rays_o': c['o'].cuda(), 'reg_radius': REG_RADIUS, 'return_absmax': True}
    gd = {k: v.cuda() for k, v in g.items()}
    if config in ('image', 'all'):
        kw['g_image'] = gd['g_image']
    if config in ('weights', 'all'):
        kw['g_weights'] = gd['g_weights']
    if config in ('absorption', 'all'):
        kw['g_absorption'] = gd['g_absorption']
    if config in ('reg', 'all'):
        kw['g_reg'] = gd['g_reg']
    if config == 'reg_const':
        kw['g_reg_const'] = G_REG_CONST
    g_raw, absmax = ops.emission_integral_bwd(raw, z, d, **kw)
    return g_raw, absmax.view(torch.float32)


def check_case(ops, c, device='cpu'):
    """Forward and every backward config of case ``c`` against the oracle; returns the measures."""
    raw, z, d = dev_inputs(c)
    f = ops.emission_integral_fwd(raw, z, d)
    f_again = ops.emission_integral_fwd(raw, z, d)
    g = upstream(c)
    bwd = {cfg: run_bwd(ops, c, g, cfg) for cfg in CONFIGS}
    again = run_bwd(ops, c, g, 'all')
    torch.cuda.synchronize()
    for a, b in zip(f, f_again):
        assert torch.equal(a, b), 'forward differs between two runs'
    assert torch.equal(bwd['all'][0], again[0]) and torch.equal(bwd['all'][1], again[1]), 'backward differs between two runs'

    ref64 = oracle(c, g, torch.float64, device)
    ref32 = oracle(c, g, torch.float32, device)
    m = fwd_units({'image': f[0], 'weights': f[1], 'absorption': f[2]}, ref64, ref32, c['s'])
    flat = c['raw'][..., 1].to(device) <= 0
    for cfg in CONFIGS:
        g_raw, absmax = bwd[cfg]
        m['g_' + cfg] = ray_units(g_raw, ref64['g_' + cfg], ref32['g_' + cfg], ref64['floor_' + cfg])
        g1 = g_raw[..., 1].to(device)
        assert bool((g1[flat] == 0).all()), (cfg, 'g_raw[..., 1] nonzero where relu(r1) is flat')
        assert absmax.item() == g_raw.abs().max().item(), (cfg, 'absmax is not max |g_raw|', absmax.item(), g_raw.abs().max().item())
    print(f"N={c['n']} S={c['s']}: " + ' '.join(f'{k} {v:.2e}' for k, v in m.items()))
    for k in ('image', 'weights', 'absorption'):
        assert m[k] <= 1.0, (k, m)
    for cfg in CONFIGS:
        assert m['g_' + cfg] <= 1.0, (cfg, m)
    return m


S_VALUES = (2, 3, 31, 32, 33, 63, 64, 65, 128, 192, 257, 672, 673, 1024, 1696)


@pytest.mark.parametrize('n', [1, 7, 8, 9])
@pytest.mark.parametrize('s', S_VALUES)
def test_emission_integral_edge_shapes(ops, s, n):
    """Chunk seams (31 ... 65, 257), the backward's > 64 KiB LDS path (673 and up) and its largest S (1696); one ray, a partial
    group of 8, a full one and one ray into the second group."""
    check_case(ops, make_case(n, s, seed=s * 10 + n))


@pytest.mark.parametrize('n, s', [(16384, 64), (16385, 33), (16389, 257), (32771, 128)])
def test_emission_integral_large_batches(ops, n, s):
    """2048 workgroups x 8 rays exactly, one ray into a second grid-stride sweep, a partial last group, two sweeps and a bit.
    The references run on the GPU (plain torch); a slice of them is checked against the CPU."""
    c = make_case(n, s, seed=n + s)
    sl = slice(n - 70, n)
    part = {k: (v[sl] if torch.is_tensor(v) and v.dim() and v.shape[0] == n else v) for k, v in c.items()}
    part['n'] = 70
    g = upstream(c)
    cpu = oracle(part, {k: v[sl] for k, v in g.items()}, torch.float64, 'cpu', configs=('all',))
    gpu = oracle(part, {k: v[sl] for k, v in g.items()}, torch.float64, 'cuda', configs=('all',))
    for k in ('image', 'weights', 'g_all'):
        err = (gpu[k].cpu() - cpu[k]).abs().reshape(70, -1).amax(-1)
        assert bool((err <= 1e-12 * cpu[k].abs().reshape(70, -1).amax(-1)).all()), k
    check_case(ops, c, device='cuda')


# ---- absmax ---------------------------------------------------------------------------------------------------------------
def _bwd_raw_call(ops, c, g_image, absmax):
    """sunerf_emission_integral_bwd through the C entry point, image gradient only, the absmax word caller-owned."""
    from sunerf_hip import lib as _l
    raw, z, d = dev_inputs(c)
    o = c['o'].cuda()
    g_raw = torch.empty(c['n'], c['s'], 2, device='cuda')
    _l.call(z.device, 'sunerf_emission_integral_bwd', ops._ptr(raw), ops._ptr(z), ops._ptr(o), ops._ptr(d), ops._ptr(g_image),
            None, None, None, 0.0, 0.0, c['n'], c['s'], ops._ptr(g_raw), ops._ptr(absmax), ops._stream(z.device))
    return g_raw


def test_emission_integral_absmax(ops):
    """The absmax word equals max |g_raw| bit for bit at N = 16389 when the batch's largest gradient sits in rays 0..7 (workgroup
    0's first grid-stride sweep; its second takes rays 16384 ... 16388), is reset per call, and is 0 for N = 0."""
    c = make_case(16389, 33, seed=5)
    g = upstream(c)
    g_image = g['g_image'].clone()
    g_image[3] = 1e3 * g_image.abs().max().item()           # ray 3 (kind 'thin' or better): the batch maximum
    g_raw, absmax = ops.emission_integral_bwd(*dev_inputs(c), g_image=g_image.cuda(), return_absmax=True)
    torch.cuda.synchronize()
    mag = g_raw.abs()
    assert int(mag.amax((1, 2)).argmax()) < 8, 'the largest gradient is not in rays 0..7'
    assert absmax.view(torch.float32).item() == mag.max().item()
    # a second call with smaller gradients reports the smaller maximum (the word is cleared, not max-accumulated)
    g_raw2, absmax2 = ops.emission_integral_bwd(*dev_inputs(c), g_image=(g_image * 0.25).cuda(), return_absmax=True)
    torch.cuda.synchronize()
    assert absmax2.view(torch.float32).item() == g_raw2.abs().max().item() < mag.max().item()
    # the same with a caller-owned word prefilled with garbage
    word = torch.full((1,), 3e38, device='cuda')
    _bwd_raw_call(ops, c, (g_image * 0.25).cuda(), word)
    torch.cuda.synchronize()
    assert word.item() == g_raw2.abs().max().item()
    # N = 0: the word is cleared
    e = make_case(0, 33, seed=1)
    word = torch.full((1,), float('nan'), device='cuda')
    _bwd_raw_call(ops, e, torch.zeros(0, device='cuda'), word)
    out, absmax0 = ops.emission_integral_bwd(*dev_inputs(e), g_image=torch.zeros(0, device='cuda'), return_absmax=True)
    torch.cuda.synchronize()
    assert word.item() == 0 and out.numel() == 0 and absmax0.item() == 0


# ---- placement ------------------------------------------------------------------------------------------------------------
def _embed(base, part, at):
    c = dict(base)
    for k in ('raw', 'z', 'o', 'd'):
        v = base[k].clone()
        v[at:at + part['n']] = part[k]
        c[k] = v
    return c


def test_emission_integral_ray_placement(ops):
    """Nine rays give bit-identical outputs and g_raw alone and at rays 0, 4093 and 16380 ... 16388 of a 16389-ray batch (the
    last straddle the second grid-stride sweep of the backward and fill its partial last group)."""
    part = make_case(9, 65, seed=11)
    gp = upstream(part)
    alone_f = ops.emission_integral_fwd(*dev_inputs(part))
    alone_b = {cfg: run_bwd(ops, part, gp, cfg)[0] for cfg in ('all', 'reg_const')}
    base = make_case(16389, 65, seed=12)
    gb = upstream(base)
    for at in (0, 4093, 16380):
        c = _embed(base, part, at)
        g = {k: v.clone() for k, v in gb.items()}
        for k in g:
            g[k][at:at + 9] = gp[k]
        f = ops.emission_integral_fwd(*dev_inputs(c))
        for a, b in zip(f, alone_f):
            assert torch.equal(a[at:at + 9], b), ('forward', at)
        for cfg, want in alone_b.items():
            got = run_bwd(ops, c, g, cfg)[0]
            assert torch.equal(got[at:at + 9], want), ('backward', cfg, at)
    torch.cuda.synchronize()


# ---- limits and NaN rows --------------------------------------------------------------------------------------------------
def test_emission_integral_sample_limits(ops):
    """S = 1 (no first distance) is refused by both entry points; S = 1697 (163 968 B of LDS) by the backward, before anything is
    queued: a caller-owned absmax word keeps its value.  S = 1696 runs in the tests above."""
    c = make_case(9, 2, seed=3)
    one = {'raw': c['raw'][:, :1].contiguous(), 'z': c['z'][:, :1].contiguous(), 'd': c['d'], 'o': c['o'], 'n': 9, 's': 1}
    with pytest.raises(ValueError, match='bad argument'):
        ops.emission_integral_fwd(*dev_inputs(one))
    with pytest.raises(ValueError, match='bad argument'):
        ops.emission_integral_bwd(*dev_inputs(one), g_image=torch.ones(9, device='cuda'))
    big = make_case(9, 1697, seed=4)
    with pytest.raises(ValueError, match='unsupported'):
        ops.emission_integral_bwd(*dev_inputs(big), g_image=torch.ones(9, device='cuda'))
    word = torch.full((1,), float('nan'), device='cuda')
    with pytest.raises(ValueError, match='unsupported'):
        _bwd_raw_call(ops, big, torch.ones(9, device='cuda'), word)
    f = ops.emission_integral_fwd(*dev_inputs(big))                # the forward has no LDS that grows with S
    torch.cuda.synchronize()
    assert bool(torch.isnan(word).all()), 'absmax cleared although the call was refused'
    assert bool(torch.isfinite(f[0]).all())


def test_emission_integral_nan_row(ops):
    """A ray with NaN z (one that missed the spherical sampler): the forward's NaN pattern is the fp32 oracle's, the other rows
    are bit-identical to a batch without that ray, and absmax is the maximum over the finite entries of g_raw."""
    c = make_case(9, 40, seed=6)
    c['z'][4] = float('nan')
    keep = [i for i in range(9) if i != 4]
    sub = {k: (v[keep] if torch.is_tensor(v) and v.dim() else v) for k, v in c.items()}
    sub['n'] = 8
    g = upstream(make_case(9, 40, seed=6))
    gs = {k: v[keep] for k, v in g.items()}
    f = ops.emission_integral_fwd(*dev_inputs(c))
    fs = ops.emission_integral_fwd(*dev_inputs(sub))
    b, absmax = run_bwd(ops, c, g, 'all')
    bs, _ = run_bwd(ops, sub, gs, 'all')
    torch.cuda.synchronize()
    ref = orc.emission_integral(c['raw'], c['z'], c['d'])
    for got, k in zip(f, ('image', 'weights', 'regularizing_quantity')):
        assert torch.equal(torch.isnan(got.cpu()), torch.isnan(ref[k])), k
    for got, want in zip(f, fs):
        assert torch.equal(got[keep], want)
    assert torch.equal(b[keep], bs)
    finite = b[torch.isfinite(b)]
    assert absmax.item() == finite.abs().max().item()
    assert bool(torch.isnan(f[0][4]).all())


# ---- the integral fused behind the MLP ----------------------------------------------------------------------------------------
# out-layer (weight scale, bias r0, bias r1): raw ~ bias + small, driving the integral into the regimes above
OUT_LAYERS = ((0.5, 0.0, -1.0), (0.3, 1.0, 0.0), (0.5, 0.5, 3.0), (1.0, -35.0, 30.0), (1.0, 2.0, 300.0), (0.3, 40.0, 3.0))


def fused_case(ops, d_filter, n_layers, n, s, precision, seed):
    c = make_case(n, s, seed)
    params = orc.init_params(d_filter=d_filter, n_layers=n_layers, seed=seed)
    W, b = params[-1]
    eps, b0, b1 = OUT_LAYERS[seed % len(OUT_LAYERS)]
    params[-1] = (W * eps, torch.tensor([b0, b1]) + b * eps)
    packed = ops.PackedMLP([W.cuda() for W, _ in params], [b.cuda() for _, b in params], precision=precision)
    t = torch.rand(n, generator=torch.Generator().manual_seed(seed))
    return c, packed, t


def check_fused(ops, c, packed, t, training=False):
    out = ops.emission_render_fwd(packed, c['o'].cuda(), c['d'].cuda(), t.cuda(), c['z'].cuda(), REG_RADIUS, want_raw=True,
                                  want_epilogues=True, training=training)
    torch.cuda.synchronize()
    raw = out['raw'].cpu()
    assert bool(torch.isfinite(raw).all())
    ref64 = orc.emission_outputs(raw.double(), c['z'], c['o'], c['d'], REG_RADIUS)
    ref32 = orc.emission_outputs(raw, c['z'], c['o'], c['d'], REG_RADIUS)
    m = fwd_units(out, ref64, ref32, c['s'])
    tau = torch.relu(raw[..., 1]).double() * (c['z'][:, 1:] - c['z'][:, :-1]).double().abs().max()
    print(f"fused N={c['n']} S={c['s']} D={packed.d_filter} p={packed.precision} training={training}: "
          + ' '.join(f'{k} {v:.2e}' for k, v in m.items()) + f' | r0 {raw[..., 0].min():.1f}..{raw[..., 0].max():.1f}'
          + f' tau <= {tau.max():.1e}')
    for k, v in m.items():
        assert v <= 1.0, (k, m)
    return out, m


FUSED_S = (2, 31, 33, 65, 257)


@pytest.mark.parametrize('precision', ['fast', 'exact', 'half'])
@pytest.mark.parametrize('s', FUSED_S)
def test_fused_integral_regimes(ops, precision, s):
    """The render kernel's integral and epilogues on its own raw output, every out-layer regime at each S and precision."""
    p = {'fast': ops.PRECISION_FAST, 'exact': ops.PRECISION_EXACT, 'half': ops.PRECISION_HALF}[precision]
    for seed in range(FUSED_S.index(s) * 6, FUSED_S.index(s) * 6 + 6):
        c, packed, t = fused_case(ops, 64, 2, 13, s, p, seed)
        check_fused(ops, c, packed, t)


@pytest.mark.parametrize('d_filter, stash', [(64, 'fp16'), (256, 'phase')])
def test_fused_integral_training_stash(ops, monkeypatch, d_filter, stash):
    """training=True: the stash-writing instantiations (fp16 sin / cos fragments at width 64, 16-bit phases at width 256)."""
    for k in ('SUNERF_BACKWARD', 'SUNERF_STASH', 'SUNERF_BACKWARD_PRECISION'):
        monkeypatch.delenv(k, raising=False)
    monkeypatch.setattr(ops, '_backward_forced', None)
    for seed in range(6):
        c, packed, t = fused_case(ops, d_filter, 2, 11, 65 if seed % 2 else 33, ops.PRECISION_EXACT if seed % 3 else ops.PRECISION_FAST,
                                  seed + 40)
        want = ops.STASH_PHASE if stash == 'phase' else ops.STASH_FP16
        assert ops.training_stash_format(packed, c['n'], c['s']) == want, 'not the stash format this test is for'
        out, _ = check_fused(ops, c, packed, t, training=True)
        assert ops.stash_format_of(out['stash'], c['n'], c['s'], packed) == want


@pytest.mark.parametrize('precision', ['fast', 'exact'])
def test_fused_integral_width_512(ops, precision):
    """d_filter = 512: the instantiation whose layers spill their activations to scratch."""
    p = ops.PRECISION_FAST if precision == 'fast' else ops.PRECISION_EXACT
    for seed in (60, 63, 64):
        c, packed, t = fused_case(ops, 512, 2, 9, 40, p, seed)
        check_fused(ops, c, packed, t)


def test_fused_integral_is_the_stand_alone_integral(ops):
    """One text (csrc/emission_sweep.h): the render kernel's image, weights and absorption are, bit for bit, the stand-alone
    forward applied to the raw the same call returned.  Width 64, EXACT, N = 9, one chunk, a partial one and both sides of a
    seam, every out-layer regime at each S."""
    for s in (2, 31, 33, 65):
        for seed in range(FUSED_S.index(s) * 6, FUSED_S.index(s) * 6 + 6):
            c, packed, t = fused_case(ops, 64, 2, 9, s, ops.PRECISION_EXACT, seed)
            out = ops.emission_render_fwd(packed, c['o'].cuda(), c['d'].cuda(), t.cuda(), c['z'].cuda(), REG_RADIUS, want_raw=True)
            alone = ops.emission_integral_fwd(out['raw'], c['z'].cuda(), c['d'].cuda())
            torch.cuda.synchronize()
            assert bool(torch.isfinite(out['raw']).all())
            for k, want in zip(('image', 'weights', 'absorption'), alone):
                assert torch.equal(out[k], want), (k, s, seed, (out[k] - want).abs().max().item())


@pytest.mark.parametrize('cap', [1, 3])
def test_fused_integral_grid_stride(ops, monkeypatch, cap):
    """SUNERF_GRID_CAP_FWD = 1 / 3 workgroups: the render kernel walks 4-ray groups grid-stride, N = 23 (a partial last group).
    Outputs are bit-identical to the uncapped launch and match the oracle."""
    c, packed, t = fused_case(ops, 64, 2, 23, 70, ops.PRECISION_EXACT, 70 + cap)
    ref, _ = check_fused(ops, c, packed, t)
    monkeypatch.setenv('SUNERF_GRID_CAP_FWD', str(cap))
    out, _ = check_fused(ops, c, packed, t)
    for k in ('image', 'weights', 'absorption', 'raw', 'height_map', 'absorption_map', 'regularization'):
        assert torch.equal(out[k], ref[k]), k
