"""csrc/thomson.hip where its decisions are discontinuous and off its default constants, against the fp64 restatement of
tests/thomson_reference.py: the three device constants away from (1, 0.63, 1), samples on the limb by bits and one fp32 step
of z beside it, the limb sample at the 32-lane chunk positions, degenerate rays (through the centre, d = 0, a sample at the
origin, repeated z), batches past the backward's grid cap, and the module with its buffers changed in place.

Bounds are those of tests/test_gpu_thomson.py: every forward output at the parity gate (gate_units, exact zero where the
reference is zero); |g_raw - fp64 autograd| <= 1e-5 max|g_ref| + 8 * 2^-24 * (the ratio outputs' terms); channel 1 of g_raw
zero; g_absmax = max|g_raw| by bits; reruns bit-identical."""
import math

import numpy as np
import pytest
import torch

import thomson_reference as tr
from conftest import gate_units
from test_gpu_thomson import (_cuda, _grad_check, _nerf_module, _oracle_pass, _params, _ratio_terms, _star_ln_rho, _star_module,
                              make_case)

pytestmark = pytest.mark.gpu

LN10 = math.log(10.)
KEYS = tr.KEYS
ALONE_AND_TOGETHER = [(k,) for k in KEYS] + [KEYS]


def f32(x):
    return float(np.float32(x))


R_07 = f32(1 / 0.7)
C0_TINY = f32(7.95e-26)       # the order of the physical constant thompson.py:11 comments out; tB stays a normal fp32 (asserted)


@pytest.fixture(scope='module')
def ops():
    assert torch.cuda.is_available(), 'GPU tests need a ROCm device'
    from sunerf_hip import ops as _ops
    return _ops


class Case:
    """A batch on the CPU, its constants (fp32 values as Python floats) and its fp64 reference, computed once."""

    def __init__(self, raw, z, o, d, c, R, u, c0):
        self.raw, self.z, self.o, self.d = (t.contiguous() for t in (raw, z, o, d))
        self.kappa = LN10 if c == 2 else 1.0
        self.R, self.u, self.c0 = f32(R), f32(u), f32(c0)
        self.consts = tuple(torch.tensor(v, dtype=torch.float32, device='cuda') for v in (self.R, self.u, self.c0))
        self.want = self.reference(self.raw)

    def reference(self, raw):
        return tr.thomson_integral(raw, self.z, self.o, self.d, self.kappa, solar_radius=self.R, limb=self.u, c0=self.c0)

    def inputs(self):
        return _cuda(self.raw, self.z, self.o, self.d)


def check_forward(ops, case, what):
    got = ops.thomson_integral_fwd(*case.inputs(), case.consts, case.kappa)
    units = {k: gate_units(got[k], case.want[k]) for k in KEYS}
    print(f'{what}: gate units', {k: round(v, 4) for k, v in units.items()})
    assert all(v <= 1.0 for v in units.values()), (what, units)
    again = ops.thomson_integral_fwd(*case.inputs(), case.consts, case.kappa)
    assert all(torch.equal(got[k], again[k]) for k in KEYS), what
    return {k: v.cpu() for k, v in got.items()}, max(units.values())


def _poison(numel):
    """Best effort against a g_raw that is not written: the allocator hands the next request of this size the same block."""
    t = torch.full((numel,), float('nan'), device='cuda')
    del t


def check_backward(ops, case, upstream, chosen_sets, what):
    """g_raw and g_absmax for each set of outputs in ``chosen_sets`` against fp64 autograd -> {chosen: g_raw (CPU, fp64)};
    prints the worst error as a fraction of its bound."""
    raw = case.raw
    n, s, c = raw.shape
    out, worst = {}, 0.0
    for chosen in chosen_sets:
        leaf = raw.double().requires_grad_(True)
        ref = case.reference(leaf)
        loss = sum((ref[k] * upstream[k]).sum() for k in chosen)
        g_ref = torch.autograd.grad(loss, leaf)[0]
        assert bool(torch.isfinite(g_ref).all())
        gs = [upstream[k].float().cuda() if k in chosen else None for k in KEYS]
        _poison(raw.numel())
        g_raw, absmax = ops.thomson_integral_bwd(*case.inputs(), case.consts, case.kappa, *gs)
        g = g_raw.cpu().double()
        assert g.shape == (n, s, c)
        if c == 2:
            assert bool((g[..., 1] == 0).all()), (what, chosen)
        scale = g_ref.abs().max().item()
        err = (g - g_ref).abs().max().item()
        floor = 8 * 2.0 ** -24 * _ratio_terms(raw, case.z, case.o, case.d, case.kappa, {k: upstream[k] for k in chosen})
        bound = 1e-5 * scale + floor
        worst = max(worst, err / bound)
        assert err <= bound, (what, chosen, err, scale, floor)
        m = g_raw.abs().max().float().item()
        assert absmax.view(torch.float32).item() == m, (what, chosen, absmax.view(torch.float32).item(), m)
        _poison(raw.numel())
        g2, absmax2 = ops.thomson_integral_bwd(*case.inputs(), case.consts, case.kappa, *gs)
        assert torch.equal(g_raw, g2) and torch.equal(absmax, absmax2), (what, chosen)
        out[chosen] = g
    print(f'{what}: worst |g - g_ref| / bound = {worst:.3f} over {len(chosen_sets)} sets of outputs')
    return out


def _upstream(want, seed):
    gen = torch.Generator().manual_seed(seed)
    return {k: torch.randn(want[k].shape, generator=gen, dtype=torch.float64) for k in KEYS}


def scaled_case(n, s, c, seed, R):
    """``make_case`` in units of R: origins, impact parameters and sample distances times R (directions as they are)."""
    raw, z, o, d, _ = make_case(n, s, c, seed)
    return raw, (z * np.float32(R)).contiguous(), (o * np.float32(R)).contiguous(), d


def impact_parameters(o, d):
    o, d = o.double(), d.double()
    return torch.cross(o, d, dim=-1).norm(dim=-1) / d.norm(dim=-1)


# ---- a. the three constants ------------------------------------------------------------------------------------------------
# every value of each constant once, the other two off their defaults (1, 0.63, 1)
CONSTANTS = [(4.0, 0.0, 2.5), (0.5, 1.0, C0_TINY), (R_07, 0.37, 2.5)]


@pytest.mark.parametrize('c', [1, 2])
@pytest.mark.parametrize('n,s', [(9, 31), (33, 33)])
@pytest.mark.parametrize('R,u,c0', CONSTANTS)
def test_constants_sweep(ops, R, u, c0, n, s, c):
    raw, z, o, d = scaled_case(n, s, c, seed=77 * s + n + c, R=R)
    case = Case(raw, z, o, d, c, R, u, c0)
    p = impact_parameters(o, d)
    assert bool((p < 0.9 * case.R).any()) and bool((p > 1.1 * case.R).any())     # some rays cross the disk, some do not
    tb = case.want['pixel_B'][:, 0]
    assert bool((tb > 0).all()) and tb.min().item() > 2.0 ** -126                 # normal in fp32, also at the tiny C_0
    what = f'constants R={case.R:.4g} u={case.u:.2f} c0={case.c0:.3g} N={n} S={s} C={c}'
    check_forward(ops, case, what)
    check_backward(ops, case, _upstream(case.want, s + n), ALONE_AND_TOGETHER, what)


# ---- b. on the limb and one step beside it ----------------------------------------------------------------------------------
def seam_batch(R, c):
    """61 two-sample rays (seven full workgroups and a ragged one): three copies of the 18 seam rays with different densities and
    seven ordinary rays, shuffled so that the seam rays sit at different sub-groups and workgroups."""
    parts, info = [], []
    for rep in range(3):
        raw, z, o, d, inf = tr.seam_cases(R, c=c, seed=rep)
        parts.append((raw, z, o, d))
        info += inf
    parts.append(scaled_case(7, 2, c, seed=5, R=R))
    info += [None] * 7
    raw, z, o, d = (torch.cat([p[i] for p in parts]) for i in range(4))
    perm = torch.randperm(len(info), generator=torch.Generator().manual_seed(9))
    return raw[perm], z[perm], o[perm], d[perm], [info[i] for i in perm.tolist()]


@pytest.mark.parametrize('c', [1, 2])
@pytest.mark.parametrize('u', [0.0, 0.63, 1.0])
@pytest.mark.parametrize('R', [1.0, 4.0, 0.5, R_07])
def test_samples_on_the_limb_and_one_step_beside_it(ops, R, u, c):
    raw, z, o, d, info = seam_batch(R, c)
    assert len(info) == 61
    case = Case(raw, z, o, d, c, R, u, 2.5)
    what = f'seams R={case.R:.4g} u={case.u:.2f} C={c}'
    got, _ = check_forward(ops, case, what)
    seam = [i for i, x in enumerate(info) if x is not None]
    live = [i for i in seam if info[i]['side'] > 0]
    dark = [i for i in seam if info[i]['side'] <= 0]
    assert len(live) == 27 and len(dark) == 27
    # the limb is inside: no brightness from r == R (the gate already demands it, the reference being zero; stated for the reader)
    assert bool((case.want['pixel_B'][dark] == 0).all()) and bool((got['pixel_B'][dark] == 0).all())
    assert bool((got['pixel_B'][live, 0] > 0).all())
    radial = [i for i in seam if info[i]['radial']]
    assert bool((got['pixel_B'][radial, 1] == 0).all())
    # ... but the masked sample is there for everything else
    assert bool((got['pixel_density'][dark] > 0).all()) and bool((got['weights'][dark, 0] > 0.999999).all())
    on_tangent = [i for i in seam if info[i]['side'] == 0 and not info[i]['radial']]
    assert torch.allclose(got['distance_from_sun'][on_tangent].double(), torch.tensor(case.R, dtype=torch.float64), rtol=1e-6)
    up = _upstream(case.want, 3)
    g = check_backward(ops, case, up, [('pixel_B',), KEYS], what)
    assert bool((g[('pixel_B',)][dark, 0, 0] == 0).all()) and bool((g[('pixel_B',)][live, 0, 0] != 0).all())
    assert bool((g[('pixel_B',)][seam, 1] == 0).all()) and bool((g[KEYS][seam, 1] == 0).all())      # the muted far samples


# ---- c. the limb sample at the chunk positions ------------------------------------------------------------------------------
@pytest.mark.parametrize('c', [1, 2])
@pytest.mark.parametrize('R', [1.0, R_07])
@pytest.mark.parametrize('s', [33, 64, 65])
def test_limb_sample_at_chunk_positions(ops, s, R, c):
    positions = [0, 31, 32, s - 1]
    rows = [tr.chunk_seam_case(R, s, index, c=c, seed=rep) for rep in range(3) for index in positions]
    raw, z, o, d = (torch.cat([r[i] for r in rows]) for i in range(4))
    index = torch.tensor(positions * 3)
    case = Case(raw, z, o, d, c, R, 0.37, 2.5)
    n = len(rows)
    rho = torch.exp(case.kappa * raw[..., 0].double())
    r = (o[:, None, :].double() + d[:, None, :].double() * z[..., None].double()).norm(dim=-1)
    assert bool((r[torch.arange(n), index] == case.R).all())                       # on the limb by bits
    others = torch.ones(n, s, dtype=torch.bool)
    others[torch.arange(n), index] = False
    assert bool((r[others] > case.R).all())
    # what the limb sample would add if it were let through: far beyond the gate
    dz = z[:, 1:].double() - z[:, :-1].double()
    dl = torch.cat([dz[:, :1], dz], -1)[torch.arange(n), index]
    limb_value = 2 * ((1 - case.u) * 4 / 3 + case.u * 0.75) - case.u / 4
    leak = case.c0 * rho[torch.arange(n), index] * limb_value * dl / case.want['pixel_B'][:, 0]
    assert leak.min().item() > 1e-2
    what = f'chunk seams S={s} R={case.R:.4g} C={c}'
    check_forward(ops, case, what)
    g = check_backward(ops, case, _upstream(case.want, s), [('pixel_B',), KEYS], what)
    assert bool((g[('pixel_B',)][torch.arange(n), index, 0] == 0).all())
    assert bool((g[('pixel_B',)][..., 0][others] != 0).all())


# ---- d. degenerate rays among ordinary ones ---------------------------------------------------------------------------------
@pytest.mark.parametrize('c', [1, 2])
@pytest.mark.parametrize('R', [1.0, 4.0])
def test_degenerate_rays_among_ordinary_ones(ops, R, c):
    s = 40
    plain = scaled_case(13, s, c, seed=21 + c, R=R)
    odd = tr.degenerate_rays(R, s, c=c, seed=4)
    names = odd[4]
    at = {'centre': 0, 'null-d': 5, 'origin': 9, 'repeats': 16}                 # rows of the mixed batch of 17
    order, k = [], 0
    for row in range(17):
        hit = [nm for nm, pos in at.items() if pos == row]
        if hit:
            order.append(13 + names.index(hit[0]))
        else:
            order.append(k)
            k += 1
    order = torch.tensor(order)
    raw, z, o, d = (torch.cat([plain[i], odd[i]])[order] for i in range(4))
    case = Case(raw, z, o, d, c, R, 0.63, 2.5)
    what = f'degenerate rays R={R} C={c}'
    got, _ = check_forward(ops, case, what)
    # the ordinary rays do not notice their neighbours: the same bits as in a batch of their own
    alone = ops.thomson_integral_fwd(*_cuda(*plain), case.consts, case.kappa)
    keep = order < 13
    for key in KEYS:
        assert torch.equal(got[key][keep], alone[key].cpu()), key
    assert bool(torch.isfinite(torch.cat([got[key].reshape(17, -1) for key in KEYS], 1)).all())
    j = at['centre']
    assert got['pixel_B'][j, 1].item() == 0.0 and got['pixel_B'][j, 0].item() > 0
    j = at['null-d']
    assert got['pixel_B'][j].abs().sum().item() == 0.0 and got['pixel_density'][j].item() == 0.0
    assert got['distance_from_obs'][j].item() == 0.0
    assert got['distance_from_sun'][j].item() == pytest.approx(o[j].double().norm().item(), rel=1e-6)
    j = at['origin']
    assert got['pixel_B'][j, 1].item() == 0.0 and got['pixel_B'][j, 0].item() > 0
    assert got['pixel_B'][at['repeats'], 0].item() > 0
    g = check_backward(ops, case, _upstream(case.want, 8), ALONE_AND_TOGETHER, what)
    g_alone, _ = ops.thomson_integral_bwd(*_cuda(*plain), case.consts, case.kappa,
                                          *[_upstream(case.want, 8)[key][keep].float().cuda() for key in KEYS])
    assert torch.equal(g[KEYS][keep].float(), g_alone.cpu())


# ---- e. past the backward's grid cap ------------------------------------------------------------------------------------------
TH_RAYS, TH_MAX_GRID = 8, 1024                       # csrc/thomson.hip: rays per workgroup, workgroups of the backward's grid


@pytest.mark.parametrize('c', [1, 2])
@pytest.mark.parametrize('n', [2 * TH_RAYS * TH_MAX_GRID + 3, TH_RAYS * TH_MAX_GRID + 1])
def test_batches_past_the_backward_grid_cap(ops, n, c):
    """More than 8192 rays: the backward's workgroups walk the batch in laps, and the maximum a workgroup found in a later lap has
    to reach g_absmax.  The upstream gradients put max|g_raw| into the last rays (the ragged last lap) and, in a second run, into
    a ray of the second lap that workgroup 700 takes."""
    s, R = 3, 4.0
    raw, z, o, d = scaled_case(n, s, c, seed=n + c, R=R)
    case = Case(raw, z, o, d, c, R, 0.37, 2.5)
    what = f'laps N={n} C={c}'
    check_forward(ops, case, what)
    base = _upstream(case.want, 12)
    check_backward(ops, case, base, [KEYS], what + ' (plain)')
    tail = 3 if n % TH_RAYS == 3 else 1
    mid = TH_RAYS * TH_MAX_GRID + TH_RAYS * 700 + 5 if n > 2 * TH_RAYS * TH_MAX_GRID else None
    for name, rows in (('last rays', slice(n - tail, n)), ('second lap, workgroup 700', slice(mid, mid + 1) if mid else None)):
        if rows is None:
            continue
        up = {k: v.clone() for k, v in base.items()}
        for k in KEYS:
            up[k][rows] *= 1e6
        g = check_backward(ops, case, up, [KEYS], f'{what} (peak in the {name})')[KEYS]
        peak = int(g.abs().reshape(n, -1).max(dim=1).values.argmax())
        assert rows.start <= peak < rows.stop, (name, peak)


# ---- f. through the module, its buffers changed in place ----------------------------------------------------------------------
def _rays_in_units_of(R, n, seed):
    gen = torch.Generator().manual_seed(seed)
    o = (torch.tensor([-63.2288, 204.4016, -21.4674]) * R).expand(n, 3).contiguous()
    target = (torch.rand(n, 3, generator=gen) * 2 - 1) * 1.3 * R
    d = target - o
    return o, (d / d.norm(dim=1, keepdim=True)).contiguous(), torch.rand(n, 1, generator=gen)


def _off_default_module():
    mod = _nerf_module(64, Rs_per_ds=0.25)
    with torch.no_grad():
        mod.limb_darkening_coeff.fill_(0.0)
        mod.C_0.fill_(2.5)
    assert mod.solar_radius.item() == 4.0 and mod.solar_radius.is_cuda
    return mod, dict(solar_radius=4.0, limb=0.0, c0=2.5)


def test_module_off_default_render_matches_oracle(precision):
    mod, constants = _off_default_module()
    o, d, t = _rays_in_units_of(4.0, 200, seed=64)
    p = impact_parameters(o, d)
    assert bool((p < 4.0).any()) and bool((p > 4.0).any()) and p.max().item() < 1.3 * 4.0 * math.sqrt(3)
    with torch.no_grad():
        got = mod(*_cuda(o, d, t))
    z_c = got['z_vals_stratified'].cpu()
    z_f = torch.sort(torch.cat([z_c, got['z_vals_hierarchical'].cpu()], -1), -1).values
    coarse = _oracle_pass(_params(mod.coarse_model), o, d, t, z_c, **constants)
    fine = _oracle_pass(_params(mod.fine_model), o, d, t, z_f, **constants)
    assert bool((fine['pixel_B'][:, 0] > 0).all())
    units = {'coarse_image': gate_units(got['coarse_image'], coarse['pixel_B']),
             'fine_image': gate_units(got['fine_image'], fine['pixel_B']),
             'height_map': gate_units(got['height_map'], fine['distance_from_sun'])}
    for k in ('pixel_density', 'distance_from_sun', 'distance_from_obs'):
        units[k] = gate_units(got[k], fine[k])
    print(f'module at R=4 u=0 C_0=2.5 {precision}: gate units', {k: round(v, 3) for k, v in units.items()})
    assert all(v <= 1.0 for v in units.values()), units
    # the defaults would not have passed: the constants are read, not assumed
    default = _oracle_pass(_params(mod.fine_model), o, d, t, z_f)
    assert gate_units(got['fine_image'], default['pixel_B']) > 100.


def test_module_off_default_parameter_gradients(precision):
    from sunerf.rendering.functional import thomson_pass
    mod, constants = _off_default_module()
    model = mod.fine_model
    o, d, t = _rays_in_units_of(4.0, 64, seed=3)
    z = mod.sampler.z_vals(*_cuda(o, d)).cpu()
    p64 = _params(model, requires_grad=True)
    want = _oracle_pass(p64, o, d, t, z, **constants)
    target = (want['pixel_B'] * 0.8).detach()
    ((want['pixel_B'] - target) ** 2).mean().backward()
    out = thomson_pass(model, mod._constants(), *_cuda(o, d, t, z))
    loss = ((out['pixel_B'] - target.float().cuda()) ** 2).mean()
    loss.backward()
    _grad_check(model, p64, f'module at R=4 u=0 C_0=2.5 {precision}')


def test_simple_star_off_default_render_and_stellar_gradients():
    """SimpleStar (ln rho, kappa = 1, one channel) behind a Sun of radius 4 in the renderer's units with u = 0 and C_0 = 2.5: the
    bounds of test_simple_star_render_and_stellar_gradients."""
    import sunerf_oracle as orc
    mod = _star_module(Rs_per_ds=0.25)
    with torch.no_grad():
        mod.limb_darkening_coeff.fill_(0.0)
        mod.C_0.fill_(2.5)
    constants = dict(solar_radius=4.0, limb=0.0, c0=2.5)
    o, d, t = _rays_in_units_of(4.0, 96, seed=8)
    out = mod(*_cuda(o, d, t))
    z_c = out['z_vals_stratified'].detach().cpu()
    z_f = torch.sort(torch.cat([z_c, out['z_vals_hierarchical'].detach().cpu()], -1), -1).values
    leaves, want = {}, {}
    for name, m, z in (('coarse', mod.coarse_model, z_c), ('fine', mod.fine_model, z_f)):
        sp = {k: m.stellar_parameters[k].detach().cpu().double().requires_grad_(True) for k in ('rho_0', 'h0', 'Rs', 'T0')}
        leaves[name] = sp
        ln_rho = _star_ln_rho(sp, orc.points_on_rays(o, d, z))
        want[name] = tr.thomson_integral(ln_rho[..., None], z, o, d, 1.0, **constants)
    assert bool((want['fine']['pixel_B'][:, 0] > 0).all())
    units = {'coarse_image': gate_units(out['coarse_image'], want['coarse']['pixel_B']),
             'fine_image': gate_units(out['fine_image'], want['fine']['pixel_B']),
             'pixel_density': gate_units(out['pixel_density'], want['fine']['pixel_density']),
             'distance_from_sun': gate_units(out['distance_from_sun'], want['fine']['distance_from_sun'])}
    print('SimpleStar at R=4 u=0 C_0=2.5: gate units', {k: round(v, 3) for k, v in units.items()})
    assert all(v <= 1.0 for v in units.values()), units
    target = want['fine']['pixel_B'].detach() * 0.9
    (((want['coarse']['pixel_B'] - target) ** 2).mean() + ((want['fine']['pixel_B'] - target) ** 2).mean()).backward()
    loss = ((out['coarse_image'] - target.float().cuda()) ** 2).mean() + ((out['fine_image'] - target.float().cuda()) ** 2).mean()
    loss.backward()
    for name, m in (('coarse', mod.coarse_model), ('fine', mod.fine_model)):
        for k in ('rho_0', 'h0'):
            ref, got = leaves[name][k].grad.item(), m.stellar_parameters[k].grad.item()
            print(f'SimpleStar at R=4 {name} d/d{k}: relative error {abs(got - ref) / abs(ref):.1e}')
            assert abs(got - ref) <= 1e-3 * abs(ref), (name, k, got, ref)
