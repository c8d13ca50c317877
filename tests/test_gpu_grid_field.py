"""The voxel-grid field on a real MI355X: csrc/grid_field.hip against the float64 restatement of
tests/grid_field_reference.py on the same fp32 points -- forward, adjoint, through the three renderings, a fit and a bake.

Bounds.  Forward: |got - ref| <= 1e-4 |ref| + 2^-19 sum_corners |w||v| per element (conftest.gate_units; the floor is 32 fp32
roundings of the absolute corner sum: three weight products, eight terms and their additions, with margin).  Gradients: per-tensor
relative L2 <= 1e-3, the project's gradient gate."""
import datetime
import math

import numpy as np
import pytest
import torch

import grid_field_reference as ref
import sunerf_oracle as orc
import thomson_reference as tr
from conftest import gate_units, load_golden

pytestmark = pytest.mark.gpu

N_RAYS, N_SAMPLES = 257, 67
FLOOR = 2.0 ** -19
FILL = (-50.0, 0.25, 3.0, -1.5)
GRIDS = ('cell', 'nonuniform', 'rotated', 'sph_closed', 'sph_open', 'sph_patch')
IDENTITY = ('cell', 'nonuniform')                       # identity basis: inside / outside is exact in both implementations
LON = {'sph_closed': 'closed', 'sph_open': 'open', 'sph_patch': 'patch'}


# ---- cases ------------------------------------------------------------------------------------------------------------------
def make_grid(name):
    from sunerf_hip.volume import CartesianGrid, SphericalGrid
    # dyadic nodes: an fp32 point can sit exactly on one
    ax = ([-1.0, -0.375, 0.125, 0.25, 1.25], [-0.875, -0.25, 0.5, 0.75], [-1.125, 0.0625, 0.75])
    if name == 'cell':
        return CartesianGrid([-0.5, 0.75], [-0.25, 0.5], [-0.75, 0.625])
    if name == 'nonuniform':
        return CartesianGrid(*ax)
    if name == 'rotated':
        a, b = 0.4, -0.7
        rz = torch.tensor([[math.cos(a), -math.sin(a), 0.], [math.sin(a), math.cos(a), 0.], [0., 0., 1.]], dtype=torch.float64)
        rx = torch.tensor([[1., 0., 0.], [0., math.cos(b), -math.sin(b)], [0., math.sin(b), math.cos(b)]], dtype=torch.float64)
        return CartesianGrid(*ax, origin=(0.2, -0.1, 0.15), basis=(rz @ rx) * torch.tensor([[1.0], [1.3], [0.8]], dtype=torch.float64))
    lat, r = np.linspace(-1.2, 1.2, 7), np.array([1.0, 1.1, 1.25, 1.5, 2.0])
    lon = {'sph_closed': np.linspace(-math.pi, math.pi, 12), 'sph_open': np.linspace(-math.pi, math.pi, 12, endpoint=False),
           'sph_patch': np.linspace(-0.7, 1.1, 12)}[name]
    return SphericalGrid(lat, lon, r)


def make_rays(name, seed, inside_only=False):
    """257 rays x 67 samples through and around the grid's domain (fixed seed); the identity-basis grids get the special
    points as further rays with d = 0 (o + 0 z = o exactly): on a node, on the last node of every axis, one ulp outside
    either end, NaN, far outside."""
    gen = torch.Generator().manual_seed(seed)
    grid = make_grid(name)
    if inside_only:                                   # every sample in the one cell of the 2 x 2 x 2 grid
        o = torch.rand(N_RAYS, 3, generator=gen) * 0.2 - 0.1
        d = torch.rand(N_RAYS, 3, generator=gen) * 0.2 - 0.1
        z = torch.rand(N_RAYS, N_SAMPLES, generator=gen).sort(1).values
        return o.float(), d.float(), z.float()
    if grid.kind == 'affine':
        o = torch.rand(N_RAYS, 3, generator=gen) * 3.6 - 1.8
        target = torch.rand(N_RAYS, 3, generator=gen) * 1.6 - 0.8
        d = (target - o) * (0.5 + torch.rand(N_RAYS, 1, generator=gen))
        z = (torch.rand(N_RAYS, N_SAMPLES, generator=gen) * 2.2).sort(1).values
    else:
        o = torch.randn(N_RAYS, 3, generator=gen)
        o = o / o.norm(dim=1, keepdim=True) * (2.2 + torch.rand(N_RAYS, 1, generator=gen))
        target = torch.randn(N_RAYS, 3, generator=gen)
        target = target / target.norm(dim=1, keepdim=True) * (0.9 + 0.8 * torch.rand(N_RAYS, 1, generator=gen))
        d = target - o
        z = (torch.rand(N_RAYS, N_SAMPLES, generator=gen) * 1.6).sort(1).values
    o, d, z = o.float(), d.float(), z.float()
    if name in IDENTITY:
        a = [t.float() for t in grid.axes]
        up = lambda v: torch.nextafter(v, torch.tensor(float('inf')))           # noqa: E731
        down = lambda v: torch.nextafter(v, torch.tensor(float('-inf')))        # noqa: E731
        special = [torch.stack([a[0][0], a[1][1], a[2][0]]),                     # on a node
                   torch.stack([a[0][-1], a[1][-1], a[2][-1]]),                  # the last node of every axis
                   torch.stack([a[0][0], a[1][0], a[2][0]]),                     # the first node of every axis
                   torch.stack([up(a[0][-1]), a[1][0], a[2][0]]),                # one ulp outside, either end, every axis
                   torch.stack([a[0][0], up(a[1][-1]), a[2][0]]),
                   torch.stack([a[0][0], a[1][0], up(a[2][-1])]),
                   torch.stack([down(a[0][0]), a[1][0], a[2][0]]),
                   torch.stack([a[0][0], down(a[1][0]), a[2][0]]),
                   torch.stack([a[0][0], a[1][0], down(a[2][0])]),
                   torch.stack([down(a[0][-1]), down(a[1][-1]), down(a[2][-1])]),  # one ulp inside
                   torch.tensor([float('nan'), 0.1, 0.1]), torch.tensor([0.1, 0.1, float('nan')]),
                   torch.tensor([100., 100., 100.]), torch.tensor([0.1, -1e30, 0.1])]
        sp = torch.stack(special)
        o = torch.cat([o, sp])
        d = torch.cat([d, torch.zeros_like(sp)])
        z = torch.cat([z, z[:sp.shape[0]]])
    return o.contiguous(), d.contiguous(), z.contiguous()


_CASES = {}


def case(name, c):
    """One (grid, channel count) case, its restatement computed once and shared: inputs, values, fp64 raw / floor / gradient."""
    key = (name, c)
    if key in _CASES:
        return _CASES[key]
    grid = make_grid(name)
    lon = LON.get(name, 'patch')
    o, d, z = make_rays(name, seed=100 + GRIDS.index(name))
    gen = torch.Generator().manual_seed(7 + c)
    values = torch.randn(*grid.shape, c, generator=gen).float()
    g_raw = torch.randn(*z.shape, c, generator=gen).float()
    leaf = values.double().requires_grad_(True)
    raw, abs_sum, inside = ref.field_on_rays(grid, leaf, o, d, z, FILL[:c], 1.0, lon)
    (raw * g_raw.double()).sum().backward()
    if name not in IDENTITY:
        dist = ref.boundary_distance(grid, ref.ray_points(o, d, z).reshape(-1, 3), 1.0, lon)
        assert dist.min().item() > 1e-6, (name, dist.min().item())      # no sample where the two could disagree on inside
    frac = inside.float().mean().item()
    assert 0.05 < frac < 0.95, (name, frac)
    _CASES[key] = dict(grid=grid, lon=lon, o=o, d=d, z=z, values=values, g_raw=g_raw, raw=raw.detach(), abs_sum=abs_sum,
                       inside=inside, grad=leaf.grad.clone(), c=c)
    return _CASES[key]


def make_field(cs, trainable=True, fill=None):
    from sunerf.model.grid_model import GridField
    from sunerf_hip.grid_field import longitude_mode, LON_NAMES
    f = GridField(cs['grid'], d_output=cs['c'], init=cs['values'], fill=FILL[:cs['c']] if fill is None else fill,
                  trainable=trainable).cuda()
    assert LON_NAMES[longitude_mode(cs['grid'])] == cs['lon']
    return f


def rel_l2(got, want):
    return ((got.detach().cpu().double() - want).norm() / want.norm()).item()


# ---- 1. forward -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('c', [1, 2, 4])
@pytest.mark.parametrize('name', GRIDS)
def test_forward_matches_the_restatement(name, c):
    cs = case(name, c)
    field = make_field(cs, trainable=False)
    o, d, z = (t.cuda() for t in (cs['o'], cs['d'], cs['z']))
    with torch.no_grad():
        got = field.field_on_rays(o, d, z)
        pts = ref.ray_points(cs['o'], cs['d'], cs['z']).reshape(-1, 3)
        by_points = field(torch.cat([pts, torch.full_like(pts[:, :1], 0.37)], 1).cuda())['inferences']      # a time column
        by_points3 = field(pts.cuda())['inferences']
    torch.cuda.synchronize()
    assert got.shape == (*cs['z'].shape, c) and by_points.shape == (pts.shape[0], c)
    units = gate_units(got, cs['raw'], floor=FLOOR * cs['abs_sum'])
    print(f'grid field forward {name} C={c}: {units:.3f} gate units, {cs["inside"].float().mean().item():.2f} of the samples inside')
    assert units <= 1.0
    # ray mode and points mode: identical bits for identical points (NaN fill patterns included: compare the words)
    assert torch.equal(got.reshape(-1, c).view(torch.int32), by_points.view(torch.int32))
    assert torch.equal(by_points.view(torch.int32), by_points3.view(torch.int32))
    # outside / NaN samples: exactly the fill
    outside = ~cs['inside']
    fill = torch.tensor(FILL[:c])
    assert torch.equal(got.cpu()[outside], fill.expand(int(outside.sum()), c))
    if name in IDENTITY:
        n_special = cs['o'].shape[0] - N_RAYS
        flags = cs['inside'][N_RAYS:, 0].tolist()
        assert n_special == 14 and flags == [True] * 3 + [False] * 6 + [True] + [False] * 4


# ---- 2. backward ------------------------------------------------------------------------------------------------------------
def _index(field, cs):
    from sunerf_hip import grid_field as gf
    o, d, z = (t.cuda() for t in (cs['o'], cs['d'], cs['z']))
    raw, index = gf.grid_field_rays(field.descriptor(), field.values.detach(), o, d, z, want_index=True)
    return raw, index


@pytest.mark.parametrize('c', [1, 2, 4])
@pytest.mark.parametrize('name', GRIDS)
def test_backward_is_the_adjoint(name, c):
    from sunerf_hip import grid_field as gf
    cs = case(name, c)
    field = make_field(cs)
    raw, index = _index(field, cs)
    g_raw = cs['g_raw'].cuda()
    got = gf.grid_field_bwd(field.descriptor(), g_raw, index)
    again = gf.grid_field_bwd(field.descriptor(), g_raw, index)
    torch.cuda.synchronize()
    err = rel_l2(got, cs['grad'])
    print(f'grid field backward {name} C={c}: relative L2 {err:.2e} (bound 1e-3)')
    assert err <= 1e-3
    assert torch.equal(got.view(torch.int32), again.view(torch.int32))                    # bit-identical reruns
    # through autograd: the same bits, and a second backward accumulates
    out = field.field_on_rays(*(t.cuda() for t in (cs['o'], cs['d'], cs['z'])))
    assert torch.equal(out.detach().view(torch.int32), raw.view(torch.int32))
    out.backward(g_raw)
    assert torch.equal(field.values.grad.view(torch.int32), got.view(torch.int32))
    # accumulate adds onto what is there
    base = torch.randn_like(got)
    acc = gf.grid_field_bwd(field.descriptor(), g_raw, index, out=base.clone(), accumulate=True)
    assert torch.equal(acc, base + got)
    # outside / NaN samples contribute exactly nothing
    only_outside = g_raw * (~cs['inside']).cuda()[..., None]
    assert gf.grid_field_bwd(field.descriptor(), only_outside, index).abs().max().item() == 0.0
    # the adjoint identity <A v, g> = <v, A^T g> in fp64 (fill 0: A v is linear in v)
    lin = make_field(cs, fill=(0.0,) * c)
    with torch.no_grad():
        av = lin.field_on_rays(*(t.cuda() for t in (cs['o'], cs['d'], cs['z'])))
    lhs = (av.double() * g_raw.double()).sum().item()
    rhs = (lin.values.detach().double() * got.double()).sum().item()
    assert abs(lhs - rhs) <= 1e-4 * abs(lhs), (lhs, rhs)


@pytest.mark.parametrize('c', [1, 4])
def test_backward_of_one_long_segment(c):
    """All 257 x 67 samples in the single cell of the 2 x 2 x 2 grid: the segment is cut into 270 pieces, summed by as many
    waves and added in order."""
    from sunerf_hip import grid_field as gf
    from sunerf.model.grid_model import GridField
    grid = make_grid('cell')
    o, d, z = make_rays('cell', seed=31, inside_only=True)
    gen = torch.Generator().manual_seed(3)
    values, g_raw = torch.randn(2, 2, 2, c, generator=gen), torch.randn(N_RAYS, N_SAMPLES, c, generator=gen)
    leaf = values.double().requires_grad_(True)
    raw, _, inside = ref.field_on_rays(grid, leaf, o, d, z, FILL[:c])
    assert bool(inside.all())
    (raw * g_raw.double()).sum().backward()
    field = GridField(grid, d_output=c, init=values, fill=FILL[:c]).cuda()
    _, index = gf.grid_field_rays(field.descriptor(), field.values.detach(), o.cuda(), d.cuda(), z.cuda(), want_index=True)
    assert int(index[0].max()) == 0
    got = gf.grid_field_bwd(field.descriptor(), g_raw.cuda(), index)
    again = gf.grid_field_bwd(field.descriptor(), g_raw.cuda(), index)
    err = rel_l2(got, leaf.grad)
    print(f'grid field backward, one segment of {N_RAYS * N_SAMPLES} samples, C={c}: relative L2 {err:.2e} (bound 1e-3)')
    assert err <= 1e-3
    assert torch.equal(got.view(torch.int32), again.view(torch.int32))


# ---- 3. through the renderings ----------------------------------------------------------------------------------------------
def sampling():
    """Fresh sampler configurations (the renderings pop 'type' from the dicts they are given)."""
    return dict(sampling_config={'type': 'stratified', 'n_samples': 24, 'perturb': False},
                hierarchical_sampling_config={'type': 'hierarchical', 'n_samples': 24})


def _cube(n=(9, 8, 7), half=1.2):
    from sunerf_hip.volume import CartesianGrid
    return CartesianGrid(*(np.linspace(-half, half, k) for k in n))


def _z(out):
    z_c = out['z_vals_stratified'].detach().cpu()
    z_f = torch.sort(torch.cat([z_c, out['z_vals_hierarchical'].detach().cpu()], -1), -1).values
    return z_c, z_f


def _emission_module(seed, lambda_smoothness=0.0, n=(9, 8, 7), **kwargs):
    from sunerf.model.grid_model import GridField
    from sunerf.model.sunerf import EmissionSuNeRFModule
    torch.manual_seed(seed)
    grid = _cube(n)
    lm = EmissionSuNeRFModule(Rs_per_ds=1.0, seconds_per_dt=1.0, image_scaling_config={'vmax': 1, 'a': 0.005}, model=GridField,
                              model_config={'grid': grid}, lambda_smoothness=lambda_smoothness, **sampling(), **kwargs)
    with torch.no_grad():
        for m in (lm.rendering.coarse_model, lm.rendering.fine_model):
            m.values.copy_(torch.randn(m.values.shape) * torch.tensor([0.6, 0.8]) + torch.tensor([-0.5, 0.0]))
    return lm.cuda(), grid


def _emission_reference(lm, grid, o, d, z_c, z_f):
    leaves, want = {}, {}
    for name, m, z in (('coarse', lm.rendering.coarse_model, z_c), ('fine', lm.rendering.fine_model, z_f)):
        leaves[name] = m.values.detach().cpu().double().requires_grad_(True)
        raw, _, _ = ref.field_on_rays(grid, leaves[name], o, d, z, m.fill.cpu().tolist())
        want[name] = orc.emission_outputs(raw, z, o, d, 1.2)
    return leaves, want


def test_emission_rendering_and_gradients():
    lm, grid = _emission_module(seed=1)
    o, d = orc.synthetic_rays(10)
    gen = torch.Generator().manual_seed(2)
    t = torch.rand(o.shape[0], 1, generator=gen)
    target = torch.rand(o.shape[0], 1, generator=gen) * 2.0
    batch = {'tracing': {'rays': torch.stack([o, d], 1).cuda(), 'time': t.cuda(), 'target_image': target.cuda()}}
    out = lm.rendering(o.cuda(), d.cuda(), t.cuda())
    assert set(out) == {'z_vals_stratified', 'coarse_image', 'z_vals_hierarchical', 'fine_image', 'image', 'height_map',
                        'absorption_map', 'regularization'}
    assert out['image'].requires_grad and out['regularization'].requires_grad and not out['height_map'].requires_grad
    z_c, z_f = _z(out)
    leaves, want = _emission_reference(lm, grid, o, d, z_c, z_f)
    s = z_f.shape[1]
    dist = want['fine']['points'].norm(dim=-1)
    # (1 - absorption): the fp32 difference of two numbers near 1 carries 2^-24 absolute, twice (the exponential's rounding and
    # the subtraction's); regularization multiplies it by relu(|p| - 1.2), absorption_map adds S of them.  |p| itself is an
    # fp32 sum of three squares and a root, 4 roundings of 2^-24 |p|, which relu(|p| - 1.2) keeps in full next to the radius
    units = {'coarse_image': gate_units(out['coarse_image'], want['coarse']['image']),
             'fine_image': gate_units(out['fine_image'], want['fine']['image']),
             'height_map': gate_units(out['height_map'], want['fine']['height_map']),
             'absorption_map': gate_units(out['absorption_map'], want['fine']['absorption_map'], floor=s * 2.0 ** -23),
             'regularization': gate_units(out['regularization'], want['fine']['regularization'],
                                          floor=(torch.relu(dist - 1.2) * 2.0 ** -23 + 4 * 2.0 ** -24 * dist *
                                                 (1 - want['fine']['regularizing_quantity'])).detach())}
    print('grid field emission render: gate units', {k: round(v, 3) for k, v in units.items()})
    assert bool((want['fine']['image'] > 0).all()) and all(v <= 1.0 for v in units.values()), units
    # the training loss and its gradient w.r.t. both grids
    loss = lm.training_step(batch, 0)
    loss.backward()
    outs = {'coarse_image': want['coarse']['image'], 'fine_image': want['fine']['image'],
            'regularization': want['fine']['regularization']}
    want_loss = orc.emission_training_loss(outs, target.double())['loss']
    want_loss.backward()
    assert abs(loss.item() - want_loss.item()) <= 1e-4 * abs(want_loss.item())
    for name, m in (('coarse', lm.rendering.coarse_model), ('fine', lm.rendering.fine_model)):
        err = rel_l2(m.values.grad, leaves[name].grad)
        print(f'grid field emission training loss: d/d {name} values relative L2 {err:.2e} (bound 1e-3)')
        assert err <= 1e-3


def test_density_temperature_rendering_and_gradients():
    from sunerf.model.grid_model import GridFieldDT
    from sunerf.model.sunerf import DensityTemperatureSuNeRFModule
    g = load_golden('g6_dt_e2e')
    pf = float(g['pixel_intensity_factor'])
    grid = _cube()
    torch.manual_seed(4)
    lm = DensityTemperatureSuNeRFModule(Rs_per_ds=1.0, seconds_per_dt=1.0, image_scaling_config={}, model=GridFieldDT,
                                        model_config={'grid': grid}, pixel_intensity_factor=pf,
                                        response_table=(g['aia_logte'].numpy(), g['aia_tresp'].numpy()), **sampling())
    with torch.no_grad():
        for k, m in enumerate((lm.rendering.coarse_model, lm.rendering.fine_model)):
            m.values.copy_(torch.rand(m.values.shape) * torch.tensor([1.6, 1.4]) + torch.tensor([-0.2, 5.5]))
            for i, w in enumerate(orc.AIA_WAVELENGTHS):
                m.log_absortpion[str(w)].fill_(0.05 + 0.06 * i + 0.01 * k if i != 3 else -0.3)      # one relu(negative): no gradient
            m.volumetric_constant.fill_(0.7 + 0.2 * k)
    lm = lm.cuda()
    o, d = orc.synthetic_rays(10)
    gen = torch.Generator().manual_seed(5)
    t = torch.rand(o.shape[0], 1, generator=gen)
    wl = torch.tensor([94., 131., 171., 193., 0., 304., 335.]).expand(o.shape[0], 7).contiguous()   # 211 absent
    out = lm.rendering(o.cuda(), d.cuda(), t.cuda(), wl.cuda())
    z_c, z_f = _z(out)
    logte, resp = lm.rendering.response_logte.cpu().double(), lm.rendering.response_table.cpu().double()
    leaves, want = {}, {}
    for name, m, z in (('coarse', lm.rendering.coarse_model, z_c), ('fine', lm.rendering.fine_model, z_f)):
        lv = {'values': m.values.detach().cpu().double().requires_grad_(True),
              'vol_c': m.volumetric_constant.detach().cpu().double().requires_grad_(True),
              'la': {k: p.detach().cpu().double().requires_grad_(True) for k, p in m.log_absortpion.items()}}
        raw, _, _ = ref.field_on_rays(grid, lv['values'], o, d, z, m.fill.cpu().tolist())
        w = orc.dt_integral(raw, lv['la'], lv['vol_c'], z.double(), wl.double(), logte, resp, pf)
        dist = ref.ray_points(o, d, z).double().norm(dim=-1)
        w['height_map'] = (w['weights'] * dist).sum(-1)
        w['absorption_map'] = (1 - w['regularizing_quantity']).sum(-1)
        w['regularization'] = torch.relu(dist - 1.25) * torch.relu(w['regularizing_quantity'])
        leaves[name], want[name] = lv, w
    s = z_f.shape[1]
    units = {'coarse_image': gate_units(out['coarse_image'], want['coarse']['image']),
             'fine_image': gate_units(out['fine_image'], want['fine']['image']),
             'height_map': gate_units(out['height_map'], want['fine']['height_map']),
             'absorption_map': gate_units(out['absorption_map'], want['fine']['absorption_map'], floor=s * 2.0 ** -23),
             # relu(|p| - 1.25) relu(q): |p| is an fp32 sum of three squares and a root, 4 roundings of 2^-24 |p|, which the
             # difference keeps in full next to the radius
             'regularization': gate_units(out['regularization'], want['fine']['regularization'],
                                          floor=(4 * 2.0 ** -24 * dist * torch.relu(want['fine']['regularizing_quantity'])).detach())}
    print('grid field DT render: gate units', {k: round(v, 3) for k, v in units.items()})
    assert bool((want['fine']['image'][:, [0, 1, 2, 3, 5, 6]] > 0).all()) and bool((out['image'][:, 4] == 0).all())
    assert all(v <= 1.0 for v in units.values()), units
    target = (want['fine']['image'].detach() * (0.5 + torch.rand(o.shape[0], 7, generator=gen).double())).float()
    batch = {'tracing': {'rays': torch.stack([o, d], 1).cuda(), 'time': t.cuda(), 'target_image': target.cuda(),
                         'wavelength': wl.cuda()}}
    loss = lm.training_step(batch, 0)
    loss.backward()
    mse = lambda a: ((a - target.double()) ** 2).mean()                          # noqa: E731
    want_loss = mse(want['coarse']['image']) + mse(want['fine']['image']) + want['fine']['regularization'].mean()
    want_loss.backward()
    assert abs(loss.item() - want_loss.item()) <= 1e-4 * abs(want_loss.item())
    for name, m in (('coarse', lm.rendering.coarse_model), ('fine', lm.rendering.fine_model)):
        lv = leaves[name]
        errs = {'values': rel_l2(m.values.grad, lv['values'].grad),
                'volumetric_constant': rel_l2(m.volumetric_constant.grad, lv['vol_c'].grad)}
        got_la = torch.stack([m.log_absortpion[str(w)].grad for w in orc.AIA_WAVELENGTHS]).cpu()
        want_la = torch.stack([lv['la'][str(w)].grad if lv['la'][str(w)].grad is not None else torch.zeros((), dtype=torch.float64)
                               for w in orc.AIA_WAVELENGTHS])
        assert got_la[3].item() == 0.0 and want_la[3].item() == 0.0 and got_la[4].item() == 0.0      # relu(negative); absent channel
        errs['log_absortpion'] = rel_l2(got_la, want_la)
        print(f'grid field DT training loss, {name}: relative L2', {k: f'{v:.2e}' for k, v in errs.items()}, '(bound 1e-3)')
        assert all(v <= 1e-3 for v in errs.values()), (name, errs)


def test_thomson_rendering_with_one_channel():
    from sunerf.model.grid_model import GridField
    from sunerf.rendering.thompson import ThompsonScattering
    grid = _cube()
    torch.manual_seed(6)
    mod = ThompsonScattering(Rs_per_ds=1.0, model=GridField, model_config={'grid': grid, 'd_output': 1}, **sampling())
    with torch.no_grad():
        for m in (mod.coarse_model, mod.fine_model):
            m.values.copy_(torch.randn(m.values.shape) * 1.2)
    mod = mod.cuda()
    o, d = orc.synthetic_rays(10)
    t = torch.zeros(o.shape[0], 1)
    out = mod(o.cuda(), d.cuda(), t.cuda())
    z_c, z_f = _z(out)
    want, leaves = {}, {}
    for name, m, z in (('coarse', mod.coarse_model, z_c), ('fine', mod.fine_model, z_f)):
        leaves[name] = m.values.detach().cpu().double().requires_grad_(True)
        raw, _, _ = ref.field_on_rays(grid, leaves[name], o, d, z, m.fill.cpu().tolist())
        want[name] = tr.thomson_integral(raw, z, o, d, 1.0)
    units = {'coarse_image': gate_units(out['coarse_image'], want['coarse']['pixel_B']),
             'fine_image': gate_units(out['fine_image'], want['fine']['pixel_B']),
             'pixel_density': gate_units(out['pixel_density'], want['fine']['pixel_density'])}
    print('grid field white light: gate units', {k: round(v, 3) for k, v in units.items()})
    assert bool((want['fine']['pixel_B'][:, 0] > 0).all()) and all(v <= 1.0 for v in units.values()), units
    target = want['fine']['pixel_B'].detach() * 0.9
    (((want['coarse']['pixel_B'] - target) ** 2).mean() + ((want['fine']['pixel_B'] - target) ** 2).mean()).backward()
    (((out['coarse_image'] - target.float().cuda()) ** 2).mean() + ((out['fine_image'] - target.float().cuda()) ** 2).mean()).backward()
    for name, m in (('coarse', mod.coarse_model), ('fine', mod.fine_model)):
        err = rel_l2(m.values.grad, leaves[name].grad)
        print(f'grid field white light: d/d {name} values relative L2 {err:.2e} (bound 1e-3)')
        assert err <= 1e-3


# ---- 4. fitting -------------------------------------------------------------------------------------------------------------
def test_fit_steps_match_a_torch_loop_on_the_restatement():
    """Five ``fit_steps`` of a 6 x 6 x 6 grid with a smoothness prior against loss.backward(); clip_grad_norm_(0.5); Adam.step()
    on the float64 restatement, fed with the z the device chose in every step; the tolerances of
    test_gpu_e2e.test_fit_steps_matches_torch_adam_and_clip."""
    from sunerf.model.sunerf import fit_steps
    lam, steps = 0.05, 5
    lm, grid = _emission_module(seed=8, lambda_smoothness=lam, n=(6, 6, 6),
                                lr_config={'start': 1e-3, 'end': 1e-4, 'iterations': 100})
    start = {k: v.detach().cpu().double().clone() for k, v in (('coarse', lm.rendering.coarse_model.values),
                                                              ('fine', lm.rendering.fine_model.values))}
    fill = lm.rendering.fine_model.fill.cpu().tolist()
    o, d = orc.synthetic_rays(8)
    gen = torch.Generator().manual_seed(9)
    t = torch.rand(o.shape[0], 1, generator=gen)
    target = torch.rand(o.shape[0], 1, generator=gen) * 2.0
    batch = {'tracing': {'rays': torch.stack([o, d], 1).cuda(), 'time': t.cuda(), 'target_image': target.cuda()}}
    chosen = []
    handle = lm.rendering.register_forward_hook(lambda mod, args, out: chosen.append(_z(out)))
    losses = fit_steps(lm, [batch] * steps)
    handle.remove()
    assert len(chosen) == steps and lm.optimizer.step_count == steps

    params = [start['coarse'].clone().requires_grad_(True), start['fine'].clone().requires_grad_(True)]
    opt = torch.optim.Adam(params, lr=1e-3)
    sched = torch.optim.lr_scheduler.ExponentialLR(opt, gamma=(1e-4 / 1e-3) ** (1 / 100))
    want_losses = []
    for z_c, z_f in chosen:
        opt.zero_grad(set_to_none=True)
        outs = {}
        for name, leaf, z in (('coarse', params[0], z_c), ('fine', params[1], z_f)):
            raw, _, _ = ref.field_on_rays(grid, leaf, o, d, z, fill)
            outs[name] = orc.emission_outputs(raw, z, o, d, 1.2)
        loss = orc.emission_training_loss({'coarse_image': outs['coarse']['image'], 'fine_image': outs['fine']['image'],
                                           'regularization': outs['fine']['regularization']}, target.double())['loss']
        loss = loss + lam * (ref.smoothness(grid, params[0]) + ref.smoothness(grid, params[1]))
        loss.backward()
        torch.nn.utils.clip_grad_norm_(params, 0.5)
        opt.step()
        if sched.get_last_lr()[0] > 5e-5:
            sched.step()
        want_losses.append(loss.detach())
    for a, b in zip(losses, want_losses):
        assert abs(a.item() - b.item()) <= 1e-4 * abs(b.item()), (a.item(), b.item())
    for name, p, q in (('coarse', lm.rendering.coarse_model.values, params[0]), ('fine', lm.rendering.fine_model.values, params[1])):
        diff = (p.detach().cpu().double() - q.detach()).abs()
        moved = (q.detach() - start[name]).abs().max().item()
        print(f'grid field fit, {name}: moved {moved:.2e}, differs by max {diff.max().item():.2e} mean {diff.mean().item():.2e}')
        assert moved > 1e-3
        assert diff.max().item() < 1e-4 and diff.mean().item() < 1e-6, (name, diff.max().item(), diff.mean().item())


# ---- 5. baking --------------------------------------------------------------------------------------------------------------
def test_bake_a_network_and_render_from_the_cube(tmp_path):
    from sunerf.evaluation.loader import ModelLoader, SuNeRFLoader
    from sunerf.model.grid_model import GridField
    from sunerf.model.sunerf import save_state
    from sunerf.rendering.emission import EmissionRadiativeTransfer
    from sunerf_hip.volume import CartesianGrid, sample_volume
    torch.manual_seed(12)
    net = EmissionRadiativeTransfer(Rs_per_ds=1.0, model_config={'d_filter': 64}, **sampling()).cuda()
    grid = CartesianGrid.cube(1.3, 24)
    volume = sample_volume(net, grid, 0.5)
    baked = EmissionRadiativeTransfer(Rs_per_ds=1.0, model=GridField, model_config={'grid': grid},
                                      **sampling())
    baked.fine_model = GridField.bake(net, grid, 0.5)
    baked.coarse_model = GridField.bake(net, grid, 0.5, model='coarse')
    baked = baked.cuda()
    held = baked.fine_model.values.detach()
    assert torch.equal(held.view(torch.int32), volume['inferences'].view(torch.int32))
    assert not held.requires_grad and baked.fine_model.Rs_per_ds == 1.0
    assert not torch.equal(baked.coarse_model.values, held)
    # a frame through ModelLoader
    ref_map = {'shape': (32, 32), 'cdelt': (75., 75.), 'meta': {'t_obs': '2022-01-01T00:00:00.000'}}
    loader = ModelLoader(rendering=baked, model=baked.fine_model, ref_map=ref_map, device='cuda')
    frame = loader.render_observer_image(0.1, 0.3, 0.5, batch_size=300)
    assert frame['image'].shape[:2] == (32, 32) and np.isfinite(frame['image']).all() and frame['image'].max() > 0
    # sample_volume of the baked field on its own grid: the restatement at the fp32 node points, at the forward gate ...
    again = sample_volume(baked, grid, 0.5)
    pts = grid.points_f64(1.0).float().reshape(-1, 3)
    want, abs_sum, inside = ref.field(grid, held.cpu(), pts, baked.fine_model.fill.cpu().tolist())
    assert bool(inside.all())
    units = gate_units(again['inferences'].reshape(-1, 2), want, floor=FLOOR * abs_sum)
    # ... and the values it holds: the fp32 node coordinate is off by at most 2^-24 max|x|, i.e. 2^-24 max|x| / step of a cell
    # per axis, which moves the trilinear value by at most that times the spread of the values (<= 2 max|v|), three axes
    step = (grid.axes[0][1] - grid.axes[0][0]).item()
    slack = 3 * 2.0 ** -24 * (1.3 / step) * 2 * held.abs().max().item()
    units_held = gate_units(again['inferences'].reshape(-1, 2), held.cpu().reshape(-1, 2), floor=FLOOR * abs_sum + slack)
    print(f'baked volume sampled on its own grid: {units:.3f} gate units (restatement), {units_held:.3f} (held values)')
    assert units <= 1.0 and units_held <= 1.0
    # .snf round trip: the same bits

    class _Holder:
        rendering = baked

    class _Data:
        config = {'wavelength': None, 'times': [datetime.datetime(2022, 1, 1), datetime.datetime(2022, 1, 3)],
                  'resolution': (32, 32), 'wcs': {'shape': (32, 32), 'cdelt': (75., 75.)}}
        Rs_per_ds, seconds_per_dt, ref_time = 1.0, 86400., datetime.datetime(2022, 1, 1)
    path = str(tmp_path / 'run' / 'save_state.snf')
    save_state(_Holder(), _Data(), path)
    snf = SuNeRFLoader(path, device='cuda')
    assert isinstance(snf.rendering.fine_model, GridField)
    back = snf.render_observer_image(0.1, 0.3, datetime.datetime(2022, 1, 1, 12), batch_size=300)
    assert np.array_equal(back['image'], frame['image']) and np.array_equal(back['height_map'], frame['height_map'])
