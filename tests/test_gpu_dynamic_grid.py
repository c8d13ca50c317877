"""The voxel-grid field with a time axis on a real MI355X: csrc/dynamic_grid.hip against the float64 restatement
of tests/dynamic_grid_reference.py on the same fp32 points and times -- forward, adjoint, long segments, through the three
renderings, a fit and a bake.  Grids and rays are those of tests/test_gpu_grid_field.py, with the same seeds.

Bounds.  Forward: |got - ref| <= 1e-4 |ref| + 2^-19 sum_corners |w||v| per element (conftest.gate_units): a corner term passes
through at most 12 roundings (4 rounded weights, 4 products, 4 additions); 32 x 2^-24 keeps the margin of section 8j.
Gradients: per-tensor relative L2 <= 1e-3, the project's gradient gate.  The time decision is exact in both implementations,
because an fp32 time promotes exactly."""
import datetime
import math

import numpy as np
import pytest
import torch

import dynamic_grid_reference as ref
import grid_field_reference as sref
import sunerf_oracle as orc
import test_gpu_grid_field as static
import thomson_reference as tr
from conftest import gate_units, load_golden

pytestmark = pytest.mark.gpu

N_RAYS, N_SAMPLES, FLOOR, FILL = static.N_RAYS, static.N_SAMPLES, static.FLOOR, static.FILL
FRAME_TIMES = {5: (0.0, 0.25, 0.375, 0.75, 1.0), 2: (0.25, 0.75)}
_F32 = torch.float32
RAY_TIMES = torch.cat([torch.tensor([0.0, 0.25, 0.375, 0.75, 1.0, 0.125, 0.3125, 0.5, 0.875, 0.3], dtype=_F32),
                       torch.nextafter(torch.tensor([0.0], dtype=_F32), torch.tensor([-math.inf], dtype=_F32)),
                       torch.nextafter(torch.tensor([1.0], dtype=_F32), torch.tensor([math.inf], dtype=_F32)),
                       torch.tensor([-0.5, 1.5, math.nan], dtype=_F32)])
CASES = (('cell', 1, 2), ('nonuniform', 2, 5), ('rotated', 4, 5), ('sph_open', 2, 5), ('sph_closed', 1, 2))
MODES = ('clamp', 'fill')


def ray_times(n):
    """Ray ``i`` takes entry ``i mod 15`` of ``RAY_TIMES``: the frames, times between them, one ulp either side of 0 and of 1,
    far outside and a NaN."""
    return RAY_TIMES[torch.arange(n) % RAY_TIMES.shape[0]].reshape(n, 1).contiguous()


# ---- cases ------------------------------------------------------------------------------------------------------------------
_CASES = {}


def case(name, c, n_frames, mode):
    """One (grid, channel count, frame count, time mode) case, its restatement computed once and shared."""
    key = (name, c, n_frames, mode)
    if key in _CASES:
        return _CASES[key]
    grid = static.make_grid(name)
    lon = static.LON.get(name, 'patch')
    o, d, z = static.make_rays(name, seed=100 + static.GRIDS.index(name))
    t = ray_times(o.shape[0])
    tau = FRAME_TIMES[n_frames]
    gen = torch.Generator().manual_seed(7 + c)
    values = torch.randn(n_frames, *grid.shape, c, generator=gen).float()
    g_raw = torch.randn(*z.shape, c, generator=gen).float()
    leaf = values.double().requires_grad_(True)
    raw, abs_sum, inside = ref.field_on_rays(grid, tau, leaf, o, d, z, t, FILL[:c], 1.0, lon, mode)
    (raw * g_raw.double()).sum().backward()
    if name not in static.IDENTITY:
        dist = sref.boundary_distance(grid, sref.ray_points(o, d, z).reshape(-1, 3), 1.0, lon)
        assert dist.min().item() > 1e-6, (name, dist.min().item())      # no sample where the two could disagree on inside
    spatial = sref.field_on_rays(grid, torch.zeros(*grid.shape, 1, dtype=torch.float64), o, d, z, (0.0,), 1.0, lon)[2]
    frac = spatial.float().mean().item()
    assert 0.05 < frac < 0.95 and bool(inside.any()), (name, frac)
    _CASES[key] = dict(spatial=spatial, grid=grid, lon=lon, o=o, d=d, z=z, t=t, tau=tau, mode=mode, values=values, g_raw=g_raw, raw=raw.detach(),
                       abs_sum=abs_sum, inside=inside, grad=leaf.grad.clone(), c=c, n_frames=n_frames)
    return _CASES[key]


def make_field(cs, trainable=True, fill=None):
    from sunerf.model.grid_model import DynamicGridField
    return DynamicGridField(cs['grid'], d_output=cs['c'], init=cs['values'], fill=FILL[:cs['c']] if fill is None else fill,
                            trainable=trainable, frame_times=cs['tau'], time_mode=cs['mode']).cuda()


def rel_l2(got, want):
    return ((got.detach().cpu().double() - want).norm() / want.norm()).item()


def _inputs(cs):
    return tuple(x.cuda() for x in (cs['o'], cs['d'], cs['z'], cs['t']))


# ---- 1. forward -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('mode', MODES)
@pytest.mark.parametrize('name,c,n_frames', CASES)
def test_forward_matches_the_restatement(name, c, n_frames, mode):
    from sunerf.model.grid_model import GridField
    cs = case(name, c, n_frames, mode)
    field = make_field(cs, trainable=False)
    o, d, z, t = _inputs(cs)
    n, s = cs['z'].shape
    with torch.no_grad():
        got = field.field_on_rays(o, d, z, t)
        pts = sref.ray_points(cs['o'], cs['d'], cs['z'])
        pts4 = torch.cat([pts, cs['t'].reshape(n, 1, 1).expand(n, s, 1)], -1).reshape(-1, 4).contiguous()
        by_points = field(pts4.cuda())['inferences']
    torch.cuda.synchronize()
    assert got.shape == (n, s, c) and by_points.shape == (n * s, c)
    units = gate_units(got, cs['raw'], floor=FLOOR * cs['abs_sum'])
    print(f'dynamic grid forward {name} C={c} T={n_frames} {mode}: {units:.3f} gate units, '
          f'{cs["inside"].float().mean().item():.2f} of the samples inside')
    assert units <= 1.0
    # ray mode and points mode: identical bits for identical points and times
    assert torch.equal(got.reshape(-1, c).view(torch.int32), by_points.view(torch.int32))
    # outside in space or time, or a NaN: exactly the fill
    outside = ~cs['inside']
    fill = torch.tensor(FILL[:c])
    assert torch.equal(got.cpu()[outside], fill.expand(int(outside.sum()), c))
    # the time rule, by the rays: NaN is outside in both modes, -0.5 / 1.5 and one ulp off the frames only under 'fill'
    t64 = cs['t'].double().reshape(n, 1)
    in_time = ~torch.isnan(t64) if mode == 'clamp' else (t64 >= cs['tau'][0]) & (t64 <= cs['tau'][-1])
    assert torch.equal(cs['inside'], cs['spatial'] & in_time)
    # at a frame time the answer is the static field's on that frame, as numbers
    for f, tau_f in enumerate(cs['tau']):
        with torch.no_grad():
            at_frame = field.field_on_rays(o, d, z, torch.full_like(t, tau_f))
            frame = GridField(cs['grid'], d_output=c, init=cs['values'][f], fill=FILL[:c], trainable=False).cuda()
            want = frame.field_on_rays(o, d, z)
        assert torch.equal(at_frame, want), (f, tau_f)


# ---- 2. backward ------------------------------------------------------------------------------------------------------------
def _index(field, cs):
    from sunerf_hip import dynamic_grid as dg
    return dg.dynamic_grid_rays(field.descriptor(), field.values.detach(), *_inputs(cs), want_index=True)


@pytest.mark.parametrize('mode', MODES)
@pytest.mark.parametrize('name,c,n_frames', CASES)
def test_backward_is_the_adjoint(name, c, n_frames, mode):
    from sunerf_hip import dynamic_grid as dg
    cs = case(name, c, n_frames, mode)
    field = make_field(cs)
    raw, index = _index(field, cs)
    assert index[0].shape == (raw.shape[0] * raw.shape[1],) and index[1].shape == (index[0].shape[0], 8)
    n_ids = field.descriptor().n_ids
    assert int(index[0].max()) == n_ids and int(index[0].min()) >= 0                     # the sentinel is there, and the largest
    assert torch.equal((index[0] == n_ids).cpu(), ~cs['inside'].reshape(-1))
    g_raw = cs['g_raw'].cuda()
    got = dg.dynamic_grid_bwd(field.descriptor(), g_raw, index)
    again = dg.dynamic_grid_bwd(field.descriptor(), g_raw, index)
    torch.cuda.synchronize()
    err = rel_l2(got, cs['grad'])
    print(f'dynamic grid backward {name} C={c} T={n_frames} {mode}: relative L2 {err:.2e} (bound 1e-3)')
    assert got.shape == cs['values'].shape and err <= 1e-3
    assert torch.equal(got.view(torch.int32), again.view(torch.int32))                    # bit-identical reruns
    # through autograd: the same bits
    out = field.field_on_rays(*_inputs(cs))
    assert torch.equal(out.detach().view(torch.int32), raw.view(torch.int32))
    out.backward(g_raw)
    assert torch.equal(field.values.grad.view(torch.int32), got.view(torch.int32))
    # accumulate adds onto what is there
    base = torch.randn_like(got)
    acc = dg.dynamic_grid_bwd(field.descriptor(), g_raw, index, out=base.clone(), accumulate=True)
    assert torch.equal(acc, base + got)
    # samples outside in space or time contribute exactly nothing
    only_outside = g_raw * (~cs['inside']).cuda()[..., None]
    assert dg.dynamic_grid_bwd(field.descriptor(), only_outside, index).abs().max().item() == 0.0
    # the adjoint identity <A v, g> = <v, A^T g> in fp64 (fill 0: A v is linear in v)
    lin = make_field(cs, fill=(0.0,) * c)
    with torch.no_grad():
        av = lin.field_on_rays(*_inputs(cs))
    lhs = (av.double() * g_raw.double()).sum().item()
    rhs = (lin.values.detach().double() * got.double()).sum().item()
    assert abs(lhs - rhs) <= 1e-4 * abs(lhs), (lhs, rhs)


# ---- 3. long segments -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('c', [1, 4])
@pytest.mark.parametrize('which', ['one_interval', 'four_intervals'])
def test_backward_of_long_segments(which, c):
    """All 257 x 67 samples in the single cell of the 2 x 2 x 2 grid.  (a) T = 2, every time 0.5: one segment of 17 219 samples,
    cut into 270 pieces.  (b) T = 5, the times cycling over four intervals: four long segments that share the pieces at their
    boundaries (both slots of a piece in use)."""
    from sunerf.model.grid_model import DynamicGridField
    from sunerf_hip import dynamic_grid as dg
    grid = static.make_grid('cell')
    o, d, z = static.make_rays('cell', seed=31, inside_only=True)
    if which == 'one_interval':
        tau, t = FRAME_TIMES[2], torch.full((N_RAYS, 1), 0.5)
    else:
        tau, t = FRAME_TIMES[5], torch.tensor([0.125, 0.3125, 0.5, 0.875])[torch.arange(N_RAYS) % 4].reshape(N_RAYS, 1)
    gen = torch.Generator().manual_seed(3)
    values, g_raw = torch.randn(len(tau), 2, 2, 2, c, generator=gen), torch.randn(N_RAYS, N_SAMPLES, c, generator=gen)
    leaf = values.double().requires_grad_(True)
    raw, _, inside = ref.field_on_rays(grid, tau, leaf, o, d, z, t, FILL[:c])
    assert bool(inside.all())
    (raw * g_raw.double()).sum().backward()
    field = DynamicGridField(grid, d_output=c, init=values, fill=FILL[:c], frame_times=tau).cuda()
    _, index = dg.dynamic_grid_rays(field.descriptor(), field.values.detach(), o.cuda(), d.cuda(), z.cuda(), t.cuda(),
                                    want_index=True)
    counts = torch.bincount(index[0].cpu().long())
    if which == 'one_interval':
        assert counts.tolist() == [N_RAYS * N_SAMPLES] and math.ceil(N_RAYS * N_SAMPLES / 64) == 270
    else:
        assert counts.shape[0] == 4 and int(counts.min()) > 64 * 60 and any(int(x) % 64 for x in counts.cumsum(0)[:-1])
    got = dg.dynamic_grid_bwd(field.descriptor(), g_raw.cuda(), index)
    again = dg.dynamic_grid_bwd(field.descriptor(), g_raw.cuda(), index)
    err = rel_l2(got, leaf.grad)
    print(f'dynamic grid backward, long segments ({which}, {counts.tolist()} samples), C={c}: relative L2 {err:.2e} (bound 1e-3)')
    assert err <= 1e-3
    assert torch.equal(got.view(torch.int32), again.view(torch.int32))


# ---- 3a. the backward at a frame time: the static backward, by bits ------------------------------------------------------------
def _backward_at_every_frame_time(grid, tau, mode, values, g_raw, o, d, z):
    """With every ray at ``tau[f]`` (dyadic: exact in fp32), frame ``f`` of the gradient is the static field's on the same grid,
    rays and ``g_raw`` as int32 words, and every other frame is 0.  The temporal weights are (1, 0) in interval 0 at ``tau[0]``
    and (0, 1) in interval ``f - 1`` after it; the ids are the static ones plus a constant with the sentinel still the largest,
    so the stable sort gives the same permutation and pieces; ``((w0 w1) w2) * 1`` is the static weight, and the node thread
    walks its one non-empty interval in the static order."""
    from sunerf.model.grid_model import DynamicGridField, GridField
    from sunerf_hip import dynamic_grid as dg, grid_field as gf
    c = values.shape[-1]
    field = DynamicGridField(grid, d_output=c, init=values, fill=FILL[:c], frame_times=tau, time_mode=mode).cuda()
    frame = GridField(grid, d_output=c, init=values[0], fill=FILL[:c]).cuda()
    o, d, z, g_raw = (x.cuda() for x in (o, d, z, g_raw))
    _, index = gf.grid_field_rays(frame.descriptor(), frame.values.detach(), o, d, z, want_index=True)
    want = gf.grid_field_bwd(frame.descriptor(), g_raw, index)                 # linear: the same whatever the frame holds
    assert float(want.abs().max()) > 0
    for f, tau_f in enumerate(tau):
        t = torch.full((o.shape[0], 1), tau_f, dtype=_F32, device='cuda')
        assert float(t[0, 0]) == tau_f
        _, index = dg.dynamic_grid_rays(field.descriptor(), field.values.detach(), o, d, z, t, want_index=True)
        got = dg.dynamic_grid_bwd(field.descriptor(), g_raw, index)
        assert torch.equal(got[f].view(torch.int32), want.view(torch.int32)), (f, tau_f)
        assert bool((got[[k for k in range(len(tau)) if k != f]] == 0).all()), (f, tau_f)


@pytest.mark.parametrize('mode', MODES)
@pytest.mark.parametrize('name,c,n_frames', CASES)
def test_backward_at_a_frame_time_is_the_static_backward(name, c, n_frames, mode):
    cs = case(name, c, n_frames, mode)
    _backward_at_every_frame_time(cs['grid'], cs['tau'], mode, cs['values'], cs['g_raw'], cs['o'], cs['d'], cs['z'])


@pytest.mark.parametrize('c', [1, 4])
@pytest.mark.parametrize('n_frames', [2, 5])
def test_backward_at_a_frame_time_is_the_static_backward_of_a_long_segment(n_frames, c):
    """The input of :func:`test_backward_of_long_segments`: all 257 x 67 samples in the one cell, 270 pieces."""
    grid = static.make_grid('cell')
    o, d, z = static.make_rays('cell', seed=31, inside_only=True)
    gen = torch.Generator().manual_seed(3)
    values, g_raw = torch.randn(n_frames, 2, 2, 2, c, generator=gen), torch.randn(N_RAYS, N_SAMPLES, c, generator=gen)
    _backward_at_every_frame_time(grid, FRAME_TIMES[n_frames], 'clamp', values, g_raw, o, d, z)


# ---- 4. through the renderings ----------------------------------------------------------------------------------------------
TAU3 = (0.0, 0.5, 1.0)
sampling, _cube, _z = static.sampling, static._cube, static._z


def _emission_module(seed, n=(9, 8, 7), **kwargs):
    from sunerf.model.grid_model import DynamicGridField
    from sunerf.model.sunerf import EmissionSuNeRFModule
    torch.manual_seed(seed)
    grid = _cube(n)
    lm = EmissionSuNeRFModule(Rs_per_ds=1.0, seconds_per_dt=1.0, image_scaling_config={'vmax': 1, 'a': 0.005},
                              model=DynamicGridField, model_config={'grid': grid, 'frame_times': TAU3}, **sampling(), **kwargs)
    with torch.no_grad():
        for m in (lm.rendering.coarse_model, lm.rendering.fine_model):
            m.values.copy_(torch.randn(m.values.shape) * torch.tensor([0.6, 0.8]) + torch.tensor([-0.5, 0.0]))
    return lm.cuda(), grid


def test_emission_rendering_and_gradients():
    lm, grid = _emission_module(seed=1)
    assert lm.rendering.fine_model.values.shape == (3, 9, 8, 7, 2)
    o, d = orc.synthetic_rays(10)
    gen = torch.Generator().manual_seed(2)
    t = torch.rand(o.shape[0], 1, generator=gen)
    target = torch.rand(o.shape[0], 1, generator=gen) * 2.0
    batch = {'tracing': {'rays': torch.stack([o, d], 1).cuda(), 'time': t.cuda(), 'target_image': target.cuda()}}
    out = lm.rendering(o.cuda(), d.cuda(), t.cuda())
    assert out['image'].requires_grad and out['regularization'].requires_grad and not out['height_map'].requires_grad
    z_c, z_f = _z(out)
    leaves, want = {}, {}
    for name, m, z in (('coarse', lm.rendering.coarse_model, z_c), ('fine', lm.rendering.fine_model, z_f)):
        leaves[name] = m.values.detach().cpu().double().requires_grad_(True)
        raw, _, _ = ref.field_on_rays(grid, TAU3, leaves[name], o, d, z, t, m.fill.cpu().tolist())
        want[name] = orc.emission_outputs(raw, z, o, d, 1.2)
    s = z_f.shape[1]
    dist = want['fine']['points'].norm(dim=-1)
    # the floors of tests/test_gpu_grid_field.py::test_emission_rendering_and_gradients, for the reasons given there
    units = {'coarse_image': gate_units(out['coarse_image'], want['coarse']['image']),
             'fine_image': gate_units(out['fine_image'], want['fine']['image']),
             'height_map': gate_units(out['height_map'], want['fine']['height_map']),
             'absorption_map': gate_units(out['absorption_map'], want['fine']['absorption_map'], floor=s * 2.0 ** -23),
             'regularization': gate_units(out['regularization'], want['fine']['regularization'],
                                          floor=(torch.relu(dist - 1.2) * 2.0 ** -23 + 4 * 2.0 ** -24 * dist *
                                                 (1 - want['fine']['regularizing_quantity'])).detach())}
    print('dynamic grid emission render: gate units', {k: round(v, 3) for k, v in units.items()})
    assert bool((want['fine']['image'] > 0).all()) and all(v <= 1.0 for v in units.values()), units
    loss = lm.training_step(batch, 0)
    loss.backward()
    outs = {'coarse_image': want['coarse']['image'], 'fine_image': want['fine']['image'],
            'regularization': want['fine']['regularization']}
    want_loss = orc.emission_training_loss(outs, target.double())['loss']
    want_loss.backward()
    assert abs(loss.item() - want_loss.item()) <= 1e-4 * abs(want_loss.item())
    for name, m in (('coarse', lm.rendering.coarse_model), ('fine', lm.rendering.fine_model)):
        err = rel_l2(m.values.grad, leaves[name].grad)
        print(f'dynamic grid emission training loss: d/d {name} values relative L2 {err:.2e} (bound 1e-3)')
        assert err <= 1e-3
        assert all(float(leaves[name].grad[f].abs().max()) > 0 for f in range(3))          # every frame takes part


def test_density_temperature_rendering_and_gradients():
    from sunerf.model.grid_model import DynamicGridFieldDT
    from sunerf.model.sunerf import DensityTemperatureSuNeRFModule
    g = load_golden('g6_dt_e2e')
    pf = float(g['pixel_intensity_factor'])
    grid = _cube()
    torch.manual_seed(4)
    lm = DensityTemperatureSuNeRFModule(Rs_per_ds=1.0, seconds_per_dt=1.0, image_scaling_config={}, model=DynamicGridFieldDT,
                                        model_config={'grid': grid, 'frame_times': TAU3}, pixel_intensity_factor=pf,
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
        raw, _, _ = ref.field_on_rays(grid, TAU3, lv['values'], o, d, z, t, m.fill.cpu().tolist())
        w = orc.dt_integral(raw, lv['la'], lv['vol_c'], z.double(), wl.double(), logte, resp, pf)
        dist = sref.ray_points(o, d, z).double().norm(dim=-1)
        w['height_map'] = (w['weights'] * dist).sum(-1)
        w['absorption_map'] = (1 - w['regularizing_quantity']).sum(-1)
        w['regularization'] = torch.relu(dist - 1.25) * torch.relu(w['regularizing_quantity'])
        leaves[name], want[name] = lv, w
    s = z_f.shape[1]
    # the floors of tests/test_gpu_grid_field.py::test_density_temperature_rendering_and_gradients
    units = {'coarse_image': gate_units(out['coarse_image'], want['coarse']['image']),
             'fine_image': gate_units(out['fine_image'], want['fine']['image']),
             'height_map': gate_units(out['height_map'], want['fine']['height_map']),
             'absorption_map': gate_units(out['absorption_map'], want['fine']['absorption_map'], floor=s * 2.0 ** -23),
             'regularization': gate_units(out['regularization'], want['fine']['regularization'],
                                          floor=(4 * 2.0 ** -24 * dist * torch.relu(want['fine']['regularizing_quantity'])).detach())}
    print('dynamic grid DT render: gate units', {k: round(v, 3) for k, v in units.items()})
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
        print(f'dynamic grid DT training loss, {name}: relative L2', {k: f'{v:.2e}' for k, v in errs.items()}, '(bound 1e-3)')
        assert all(v <= 1e-3 for v in errs.values()), (name, errs)


def test_thomson_rendering_with_one_channel():
    from sunerf.model.grid_model import DynamicGridField
    from sunerf.rendering.thompson import ThompsonScattering
    grid = _cube()
    torch.manual_seed(6)
    mod = ThompsonScattering(Rs_per_ds=1.0, model=DynamicGridField,
                             model_config={'grid': grid, 'd_output': 1, 'frame_times': TAU3}, **sampling())
    with torch.no_grad():
        for m in (mod.coarse_model, mod.fine_model):
            m.values.copy_(torch.randn(m.values.shape) * 1.2)
    mod = mod.cuda()
    o, d = orc.synthetic_rays(10)
    t = torch.rand(o.shape[0], 1, generator=torch.Generator().manual_seed(7))
    out = mod(o.cuda(), d.cuda(), t.cuda())
    z_c, z_f = _z(out)
    want, leaves = {}, {}
    for name, m, z in (('coarse', mod.coarse_model, z_c), ('fine', mod.fine_model, z_f)):
        leaves[name] = m.values.detach().cpu().double().requires_grad_(True)
        raw, _, _ = ref.field_on_rays(grid, TAU3, leaves[name], o, d, z, t, m.fill.cpu().tolist())
        want[name] = tr.thomson_integral(raw, z, o, d, 1.0)
    units = {'coarse_image': gate_units(out['coarse_image'], want['coarse']['pixel_B']),
             'fine_image': gate_units(out['fine_image'], want['fine']['pixel_B']),
             'pixel_density': gate_units(out['pixel_density'], want['fine']['pixel_density'])}
    print('dynamic grid white light: gate units', {k: round(v, 3) for k, v in units.items()})
    assert bool((want['fine']['pixel_B'][:, 0] > 0).all()) and all(v <= 1.0 for v in units.values()), units
    target = want['fine']['pixel_B'].detach() * 0.9
    (((want['coarse']['pixel_B'] - target) ** 2).mean() + ((want['fine']['pixel_B'] - target) ** 2).mean()).backward()
    (((out['coarse_image'] - target.float().cuda()) ** 2).mean() + ((out['fine_image'] - target.float().cuda()) ** 2).mean()).backward()
    for name, m in (('coarse', mod.coarse_model), ('fine', mod.fine_model)):
        err = rel_l2(m.values.grad, leaves[name].grad)
        print(f'dynamic grid white light: d/d {name} values relative L2 {err:.2e} (bound 1e-3)')
        assert err <= 1e-3


# ---- 5. fitting -------------------------------------------------------------------------------------------------------------
def test_fit_steps_match_a_torch_loop_on_the_restatement():
    """Five ``fit_steps`` of a 6 x 6 x 6 grid x 3 frames with a spatial and a temporal prior against loss.backward();
    clip_grad_norm_(0.5); Adam.step() on the float64 restatement, fed with the z the device chose in every step; the tolerances
    of tests/test_gpu_grid_field.py::test_fit_steps_match_a_torch_loop_on_the_restatement."""
    from sunerf.model.sunerf import fit_steps
    lam, lam_t, steps = 0.05, 0.05, 5
    lm, grid = _emission_module(seed=8, n=(6, 6, 6), lambda_smoothness=lam, lambda_temporal=lam_t,
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
            raw, _, _ = ref.field_on_rays(grid, TAU3, leaf, o, d, z, t, fill)
            outs[name] = orc.emission_outputs(raw, z, o, d, 1.2)
        loss = orc.emission_training_loss({'coarse_image': outs['coarse']['image'], 'fine_image': outs['fine']['image'],
                                           'regularization': outs['fine']['regularization']}, target.double())['loss']
        loss = loss + lam * (ref.smoothness(grid, params[0]) + ref.smoothness(grid, params[1]))
        loss = loss + lam_t * (ref.temporal_smoothness(TAU3, params[0]) + ref.temporal_smoothness(TAU3, params[1]))
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
        print(f'dynamic grid fit, {name}: moved {moved:.2e}, differs by max {diff.max().item():.2e} mean {diff.mean().item():.2e}')
        assert moved > 1e-3
        assert diff.max().item() < 1e-4 and diff.mean().item() < 1e-6, (name, diff.max().item(), diff.mean().item())


# ---- 6. baking --------------------------------------------------------------------------------------------------------------
def test_bake_a_network_at_three_times_and_render_between_them(tmp_path):
    from sunerf.evaluation.loader import ModelLoader, SuNeRFLoader
    from sunerf.model.grid_model import DynamicGridField
    from sunerf.model.sunerf import save_state
    from sunerf.rendering.emission import EmissionRadiativeTransfer
    from sunerf_hip.volume import CartesianGrid, sample_volume
    torch.manual_seed(12)
    times = (0.25, 0.5, 0.75)
    net = EmissionRadiativeTransfer(Rs_per_ds=1.0, model_config={'d_filter': 64}, **sampling()).cuda()
    grid = CartesianGrid.cube(1.3, 16)
    volume = sample_volume(net, grid, list(times))
    baked = EmissionRadiativeTransfer(Rs_per_ds=1.0, model=DynamicGridField, model_config={'grid': grid, 'frame_times': times},
                                      **sampling())
    baked.fine_model = DynamicGridField.bake(net, grid, times)
    baked.coarse_model = DynamicGridField.bake(net, grid, times, model='coarse')
    baked = baked.cuda()
    held = baked.fine_model.values.detach()
    assert held.shape == (3, 16, 16, 16, 2)
    assert torch.equal(held.view(torch.int32), volume['inferences'].view(torch.int32))
    assert not held.requires_grad and baked.fine_model.Rs_per_ds == 1.0
    assert baked.fine_model.frame_times.dtype == torch.float64 and baked.fine_model.frame_times.tolist() == list(times)
    assert not torch.equal(baked.coarse_model.values, held)
    assert not torch.equal(held[0], held[2])                                      # the network moves in time
    # a frame between two baked times through ModelLoader
    ref_map = {'shape': (32, 32), 'cdelt': (75., 75.), 'meta': {'t_obs': '2022-01-01T00:00:00.000'}}
    loader = ModelLoader(rendering=baked, model=baked.fine_model, ref_map=ref_map, device='cuda')
    frame = loader.render_observer_image(0.1, 0.3, 0.6, batch_size=300)
    assert frame['image'].shape[:2] == (32, 32) and np.isfinite(frame['image']).all() and frame['image'].max() > 0
    # sample_volume of the baked field on its own grid at its own times: the restatement at the fp32 node points, at the forward
    # gate, and the values it holds with the node-coordinate slack of tests/test_gpu_grid_field.py's bake test
    again = sample_volume(baked, grid, list(times))
    pts = grid.points_f64(1.0).float().reshape(-1, 3)
    step = (grid.axes[0][1] - grid.axes[0][0]).item()
    slack = 3 * 2.0 ** -24 * (1.3 / step) * 2 * held.abs().max().item()
    for f, tau_f in enumerate(times):
        pts4 = torch.cat([pts, torch.full_like(pts[:, :1], tau_f)], 1)
        want, abs_sum, inside = ref.field(grid, times, held.cpu(), pts4, baked.fine_model.fill.cpu().tolist())
        assert bool(inside.all())
        units = gate_units(again['inferences'][f].reshape(-1, 2), want, floor=FLOOR * abs_sum)
        units_held = gate_units(again['inferences'][f].reshape(-1, 2), held[f].cpu().reshape(-1, 2), floor=FLOOR * abs_sum + slack)
        print(f'baked sequence sampled on its own grid at t={tau_f}: {units:.3f} gate units (restatement), {units_held:.3f} (held)')
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
    assert isinstance(snf.rendering.fine_model, DynamicGridField)
    assert snf.rendering.fine_model.frame_times.dtype == torch.float64
    back = snf.render_observer_image(0.1, 0.3, datetime.datetime(2022, 1, 1, 14, 24), batch_size=300)      # 0.6 days
    assert np.array_equal(back['image'], frame['image']) and np.array_equal(back['height_map'], frame['height_map'])
