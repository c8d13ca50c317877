"""Gradients of the density/temperature family where the reference's autograd gives them and the fused kernels did not:
the trainable SimpleStar (stellar parameters, absorption scalars, volumetric constant; sunerf_simple_star_field_dev /
sunerf_simple_star_bwd) and the generic DT path's ``weights`` / ``regularizing_quantity`` (sunerf_dt_integral_bwd_full).

The checker is the committed CPU restatement (oracle/sunerf_oracle.py, pinned to the reference through g6 / g9): its
autograd over the same composition of passes."""
import math

import pytest
import torch

from conftest import gate_units, load_golden

pytestmark = pytest.mark.gpu

STAR_KEYS = ('Rs', 'h0', 'T0', 'rho_0')
T_PHOTOSPHERE = 5777.


def _g9():
    g = load_golden('g9_simple_star')
    g['resp'] = (g['aia_tresp'] * float(g['aia_exp_time'])).float()      # density_temperature.py:137-146, as the module builds it
    return g


def _star_module(g, n_coarse=24, n_fine=24, trainer=False):
    """DT rendering (or its training module) with SimpleStar fields carrying g9's absorption scalars / volumetric constant."""
    from sunerf.model.stellar_model import SimpleStar
    from sunerf.model.sunerf import DensityTemperatureSuNeRFModule
    from sunerf.rendering.density_temperature import DensityTemperatureRadiativeTransfer
    kw = dict(Rs_per_ds=1, model=SimpleStar, model_config={},
              sampling_config={'type': 'stratified', 'n_samples': n_coarse, 'perturb': False},
              hierarchical_sampling_config={'type': 'hierarchical', 'n_samples': n_fine},
              pixel_intensity_factor=float(g['pixel_intensity_factor']),
              response_table=(g['aia_logte'].numpy(), g['aia_tresp'].numpy()))
    if trainer:
        lm = DensityTemperatureSuNeRFModule(seconds_per_dt=1.0, image_scaling_config={}, **kw)
        mod = lm.rendering
    else:
        lm = mod = DensityTemperatureRadiativeTransfer(**kw)
    with torch.no_grad():
        for m in (mod.coarse_model, mod.fine_model):
            for w in (94, 131, 171, 193, 211, 304, 335):
                m.log_absortpion[str(w)].copy_(g[f'la__{w}'])
            m.volumetric_constant.copy_(g['vol_c'])
        # the two stars differ, so that a gradient landing in the wrong instance shows
        mod.fine_model.stellar_parameters['h0'].mul_(1.05)
        mod.fine_model.stellar_parameters['T0'].mul_(0.97)
        mod.fine_model.log_absortpion['171'].mul_(1.5)
    return lm.cuda()


def _oracle_star(model, requires_grad=True):
    """(stellar parameters, absorption scalars, volumetric constant) of a SimpleStar as CPU fp32 leaves."""
    leaf = lambda p: p.detach().cpu().clone().requires_grad_(requires_grad)      # noqa: E731
    return ({k: leaf(model.stellar_parameters[k]) for k in STAR_KEYS},
            {k: leaf(v) for k, v in model.log_absortpion.items()}, leaf(model.volumetric_constant))


def oracle_star_render(coarse, fine, rays_o, rays_d, wavelengths, logte, resp, n_coarse, n_fine, pixel_factor,
                       reg_radius=1.25, distance=1.3):
    """DensityTemperatureRadiativeTransfer(model=SimpleStar).forward on the oracle with separate coarse and fine stars
    (``render_dt_analytic`` uses one field for both)."""
    import sunerf_oracle as orc
    f32 = torch.float32
    z_vals = orc.stratified_z(rays_o, rays_d, orc.linspace_t_vals(n_coarse), torch.tensor(distance, dtype=f32),
                              torch.tensor(1., dtype=f32))

    def one_pass(star, z):
        sp, la, vc = star
        pts = orc.points_on_rays(rays_o, rays_d, z)
        inf = orc.simple_star_field(pts.reshape(-1, 3), sp['rho_0'], sp['h0'], sp['T0'], sp['Rs']).reshape(*pts.shape[:-1], 2)
        out = orc.dt_integral(inf, la, vc, z, wavelengths, logte, resp, pixel_factor)
        out['points'] = pts
        return out
    c = one_pass(coarse, z_vals)
    _, z_comb = orc.hierarchical_z(z_vals, c['weights'], n_fine)
    f = one_pass(fine, z_comb)
    dist = f['points'].pow(2).sum(-1).pow(0.5)
    return {'coarse_image': c['image'], 'fine_image': f['image'], 'height_map': (f['weights'] * dist).sum(-1),
            'regularization': torch.relu(dist - reg_radius) * torch.relu(f['regularizing_quantity'])}


def _named_oracle_leaves(prefix, star):
    sp, la, vc = star
    out = {f'{prefix}.stellar_parameters.{k}': v for k, v in sp.items()}
    out.update({f'{prefix}.log_absortpion.{k}': v for k, v in la.items()})
    out[f'{prefix}.volumetric_constant'] = vc
    return out


def _compare_grads(named_params, ref_leaves, bound, what):
    worst = {}
    for name, p in named_params:
        ref = ref_leaves[name].grad
        assert ref is not None, name
        got = p.grad
        assert got is not None, (what, name, 'no gradient')
        got = got.detach().cpu()
        if ref.abs().max() == 0:
            assert got.abs().max() == 0, (what, name)
            continue
        err = ((got.double() - ref.double()).norm() / ref.double().norm()).item()
        worst[name] = err
    for name, err in sorted(worst.items()):
        print(f'{what}: {name:40s} rel err {err:.2e} (bound {bound:.0e})')
    bad = {k: v for k, v in worst.items() if not v < bound}
    assert not bad, (what, bad)


# ---- 1. kernels -------------------------------------------------------------------------------------------------------
def _star_batch(n_rays=5000, n_samples=64, seed=3):
    """Rays from 3 solar radii through and around the sun (samples inside it, on the ramp up to Rs, beyond), plus rays of a
    SphericalSampler that miss its sphere (NaN z -> NaN radius)."""
    import sunerf_oracle as orc
    gen = torch.Generator().manual_seed(seed)
    o = torch.tensor([0.4, -2.9, 0.6]).expand(n_rays, 3).contiguous()
    centre = -o[0] / o[0].norm()
    u = torch.linalg.cross(centre, torch.tensor([0., 0., 1.]))
    u = u / u.norm()
    v = torch.linalg.cross(centre, u)
    ang = (torch.rand(n_rays, 2, generator=gen) * 2 - 1) * 0.45
    d = centre + ang[:, :1] * u + ang[:, 1:] * v
    d = (d / d.norm(dim=-1, keepdim=True) * (0.8 + 0.4 * torch.rand(n_rays, 1, generator=gen))).contiguous()
    dist_o = o.norm(dim=-1, keepdim=True)
    z = dist_o / d.norm(dim=-1, keepdim=True) * (0.45 + 1.1 * torch.rand(n_rays, n_samples, generator=gen))
    z = torch.sort(z, -1).values
    n_miss = 64           # the last rays: a SphericalSampler (radius 1.3) z of rays passing 3 radii from the centre
    d[-n_miss:] = u + 0.05 * (torch.rand(n_miss, 1, generator=gen) - 0.5) * v
    z[-n_miss:] = orc.spherical_z(o[-n_miss:], d[-n_miss:], orc.linspace_t_vals(n_samples), torch.tensor(1.3), torch.tensor(1.))
    assert bool(torch.isnan(z[-n_miss:]).all())
    return o.contiguous(), d.contiguous(), z.contiguous().float()


def test_simple_star_kernels_match_oracle_autograd():
    import sunerf_oracle as orc
    from sunerf_hip import ops
    o, d, z = _star_batch()
    n, s = z.shape
    sp = {'Rs': 1.1, 'h0': 0.1, 'T0': 1.2e6, 'rho_0': 3.0e8}
    params = torch.tensor([sp[k] for k in STAR_KEYS], dtype=torch.float32)
    oc, dc, zc, pc = o.cuda(), d.cuda(), z.cuda(), params.cuda()

    # field from device parameters: bit for bit the host-float kernel, NaN rule included (log(0) = -inf)
    raw_dev = ops.simple_star_field_dev(oc, dc, zc, pc, T_PHOTOSPHERE)
    raw_host = ops.simple_star_field(oc, dc, zc, *(float(params[STAR_KEYS.index(k)]) for k in ('rho_0', 'h0', 'T0', 'Rs')),
                                     T_PHOTOSPHERE)
    assert torch.equal(raw_dev, raw_host)
    assert bool((raw_dev[-64:] == -math.inf).all())

    gen = torch.Generator().manual_seed(11)
    g_raw = (torch.randn(n, s, 2, generator=gen) + 0.5).float()
    # the oracle takes fp64 points; a sample whose fp32 and fp64 radius could fall on different sides of a mask edge (1, Rs)
    # would compare two different piecewise definitions: such samples get no gradient on either side
    pts = orc.points_on_rays(o.double(), d.double(), z.double())
    r = pts.norm(dim=-1)
    edge = ((r - 1).abs() < 1e-5) | ((r - sp['Rs']).abs() < 1e-5)
    g_raw[edge] = 0.
    radius = r[torch.isfinite(r)]
    counts = {'inside': int((radius <= 1).sum()), 'ramp': int(((radius > 1) & (radius <= sp['Rs'])).sum()),
              'beyond': int((radius > sp['Rs']).sum()), 'nan radius': int(torch.isnan(r).sum())}
    print('samples', counts)
    assert min(counts.values()) > 1000, counts

    leaves = {k: torch.tensor(v, dtype=torch.float32, requires_grad=True) for k, v in sp.items()}
    inf = orc.simple_star_field(pts.reshape(-1, 3), leaves['rho_0'], leaves['h0'], leaves['T0'], leaves['Rs'])
    inf.backward(g_raw.double().reshape(-1, 2))
    ref = torch.stack([leaves[k].grad.double() for k in STAR_KEYS])

    got = ops.simple_star_bwd(oc, dc, zc, pc, T_PHOTOSPHERE, g_raw.cuda())
    again = ops.simple_star_bwd(oc, dc, zc, pc, T_PHOTOSPHERE, g_raw.cuda())
    torch.cuda.synchronize()
    assert bool(torch.isfinite(got).all()), got
    assert torch.equal(got, again), 'the reduction is not deterministic'
    err = ((got.cpu().double() - ref).abs() / ref.abs())
    for k, e, a, b in zip(STAR_KEYS, err.tolist(), got.tolist(), ref.tolist()):
        print(f'd/d{k:6s} kernel {a: .8e} oracle {b: .8e} rel err {e:.1e} (bound 1e-4)')
    assert bool((err < 1e-4).all()), err

    # accumulate mode adds to what is there
    acc = torch.full((4,), 2.0, device='cuda')
    ops.simple_star_bwd(oc, dc, zc, pc, T_PHOTOSPHERE, g_raw.cuda(), out=acc)
    assert torch.allclose(acc.cpu().double(), got.cpu().double() + 2.0, rtol=1e-6)


def test_dt_integral_bwd_full_weights_and_reg_q():
    """The new backward w.r.t. weights / regularizing_quantity against the oracle's autograd of dt_integral."""
    import sunerf_oracle as orc
    from sunerf_hip import ops
    g = load_golden('g6_dt_e2e')
    resp = (g['aia_tresp'] * float(g['aia_exp_time'])).float()
    gen = torch.Generator().manual_seed(5)
    n, s = 300, 48
    o, d = g['rays_o'][:1].expand(n, 3).contiguous(), g['rays_d'].repeat(n // 16 + 1, 1)[:n].contiguous()
    z = torch.sort(torch.rand(n, s, generator=gen), -1).values * 2.6 + 213.8
    inf = torch.stack([torch.randn(n, s, generator=gen) * 0.5 + 0.2, torch.rand(n, s, generator=gen) * 3 + 4.5], -1)
    inf[:, ::7, 0] = -0.3                                   # some relu(inf0) = 0: no gradient there
    wl = g['wavelengths'].repeat(n // 16 + 1, 1)[:n].contiguous()
    la = {str(w): torch.tensor(v) for w, v in zip(orc.AIA_WAVELENGTHS, (1e-9, 2e-9, 3e-9, -1e-9, 5e-9, 6e-9, 7e-9))}
    vc = torch.tensor(0.7)
    g_img, g_w, g_q = (torch.randn(n, 7, generator=gen), torch.randn(n, s, generator=gen), torch.randn(n, s, generator=gen))
    x = inf.clone().requires_grad_(True)
    out = orc.dt_integral(x, la, vc, z, wl, g['aia_logte'], resp, 1e10)
    scale = out['image'].detach().abs().mean()
    torch.autograd.backward([out['image'], out['weights'], out['regularizing_quantity']], [g_img / scale, g_w, g_q])
    la_vec = torch.stack([la[str(w)] for w in orc.AIA_WAVELENGTHS]).cuda()
    args = (inf.cuda(), z.cuda(), torch.zeros_like(o).cuda(), d.cuda(), wl.cuda(), g['aia_logte'].cuda(), resp.cuda(), la_vec,
            vc.reshape(1).cuda(), 0.0, 0.0, 1e10, 0.0, (g_img / scale).cuda(), None)
    g_raw, _, _, _ = ops.dt_integral_bwd_full(*args, g_w.cuda(), g_q.cuda())
    ref = x.grad
    err = ((g_raw.cpu().double() - ref.double()).norm() / ref.double().norm()).item()
    print(f'dt_integral_bwd_full: g_raw rel err {err:.2e} (bound 1e-4)')
    assert err < 1e-4
    # without the two extra gradients it is the image-only backward, bit for bit
    only_img, la_a, vc_a, _ = ops.dt_integral_bwd_full(*args, None, None)
    base, la_b, vc_b, _ = ops.dt_integral_bwd(*args)
    assert torch.equal(only_img, base)


# ---- 2. module: DensityTemperatureSuNeRFModule(model=SimpleStar) ----------------------------------------------------------
def _star_batch_dict(g, target):
    rays = torch.stack([g['rays_o'], g['rays_d']], 1).cuda()
    return {'tracing': {'rays': rays, 'time': g['times'].cuda(), 'target_image': target.cuda(),
                        'wavelength': g['wavelengths'].cuda()}}


@pytest.mark.parametrize('flat_bucket', [False, True])
def test_simple_star_training_step_gradients(flat_bucket):
    import sunerf_oracle as orc  # noqa: F401
    g = _g9()
    lm = _star_module(g, trainer=True)
    rnd = lm.rendering
    coarse, fine = _oracle_star(rnd.coarse_model), _oracle_star(rnd.fine_model)
    want = oracle_star_render(coarse, fine, g['rays_o'], g['rays_d'], g['wavelengths'], g['aia_logte'], g['resp'], 24, 24,
                              float(g['pixel_intensity_factor']))
    target = (want['fine_image'] * 0.8).detach()
    ref_loss = (torch.nn.functional.mse_loss(want['coarse_image'], target) + torch.nn.functional.mse_loss(want['fine_image'], target)
                + want['regularization'].mean())
    ref_loss.backward()
    if flat_bucket:
        (optimizer,), _ = lm.configure_optimizers()
        optimizer.zero_grad()
        from sunerf_hip.train import bucket_of
        assert all(bucket_of(p) is not None for p in rnd.parameters())
        slots = {id(p): p.grad.data_ptr() for p in rnd.parameters()}
    loss = lm.training_step(_star_batch_dict(g, target), 0)
    assert abs(loss.item() - ref_loss.item()) < 2e-4 * abs(ref_loss.item()), (loss.item(), ref_loss.item())
    loss.backward()
    if flat_bucket:        # the kernels wrote into the bucket: nothing replaced a .grad view
        assert all(p.grad.data_ptr() == slots[id(p)] for p in rnd.parameters())
    leaves = {**_named_oracle_leaves('coarse_model', coarse), **_named_oracle_leaves('fine_model', fine)}
    _compare_grads(rnd.named_parameters(), leaves, 1e-3, f'SimpleStar training step (flat bucket {flat_bucket})')


# ---- 3. optimiser coherence -----------------------------------------------------------------------------------------------
def test_simple_star_render_after_clip_adam_step():
    g = _g9()
    lm = _star_module(g, trainer=True)
    rnd = lm.rendering
    for m in (rnd.coarse_model, rnd.fine_model):   # the stellar parameters alone: an Adam step of lr on a 1e-9 scalar is no test
        for p in [*m.log_absortpion.values(), m.volumetric_constant]:
            p.requires_grad_(False)
    (optimizer,), _ = lm.configure_optimizers()     # lr 1e-4: h0 (0.086) moves by 1e-4, the image by ~1e-2
    before = {k: rnd.fine_model.stellar_parameters[k].item() for k in STAR_KEYS}
    with torch.no_grad():
        out0 = rnd(g['rays_o'].cuda(), g['rays_d'].cuda(), g['times'].cuda(), g['wavelengths'].cuda())
    optimizer.zero_grad()
    lm.training_step(_star_batch_dict(g, out0['fine_image'].cpu() * 0.8), 0).backward()
    optimizer.step()
    after = {k: rnd.fine_model.stellar_parameters[k].item() for k in STAR_KEYS}
    assert after['h0'] != before['h0'] and after['Rs'] != before['Rs'], (before, after)
    want = oracle_star_render(_oracle_star(rnd.coarse_model, False), _oracle_star(rnd.fine_model, False), g['rays_o'],
                              g['rays_d'], g['wavelengths'], g['aia_logte'], g['resp'], 24, 24, float(g['pixel_intensity_factor']))
    args = (g['rays_o'].cuda(), g['rays_d'].cuda(), g['times'].cuda(), g['wavelengths'].cuda())
    got_train = rnd(*args)                 # training path: parameters read from the optimiser's buffer on the device
    with torch.no_grad():
        got_infer = rnd(*args)             # inference path: host copies of the parameters, refreshed after the step
    for what, got in (('training path', got_train), ('inference path', got_infer)):
        units = {k: gate_units(got[k], want[k]) for k in ('coarse_image', 'fine_image')}
        print(what, {k: round(v, 3) for k, v in units.items()}, '(bound 1)')
        assert all(v <= 1.0 for v in units.values()), (what, units)
    # and the step did move the image by far more than the gate
    assert gate_units(out0['fine_image'], want['fine_image']) > 10


# ---- 4. generic DT path: a subclass that only changes the regularization radius ------------------------------------------
@pytest.mark.parametrize('pixel_factor,height_weight', [(None, 1e-3), (1e15, 1.0)])
def test_generic_dt_path_regularization_and_height_map_gradients(pixel_factor, height_weight):
    """Loss MSE(coarse) + MSE(fine) + regularization.mean() + height_weight * height_map.sum().  With g6's pixel factor the
    image terms dominate every gradient; the second composition gives all four terms a real share of it."""
    import sunerf_oracle as orc
    from sunerf.model.model import NeRF_DT
    from sunerf.rendering.density_temperature import DensityTemperatureRadiativeTransfer

    class WiderRegularization(DensityTemperatureRadiativeTransfer):
        def regularization(self, distance, regularizing_quantity):
            return torch.relu(distance - 1.1 / self.Rs_per_ds) * torch.relu(regularizing_quantity)

    g = load_golden('g6_dt_e2e')
    resp = (g['aia_tresp'] * float(g['aia_exp_time'])).float()
    pf = float(g['pixel_intensity_factor']) if pixel_factor is None else pixel_factor
    mod = WiderRegularization(
        Rs_per_ds=1.0, sampling_config={'type': 'stratified', 'n_samples': 16, 'perturb': False},
        hierarchical_sampling_config={'type': 'hierarchical', 'n_samples': 16}, model_config={'d_filter': 64}, model=NeRF_DT,
        pixel_intensity_factor=pf, response_table=(g['aia_logte'].numpy(), g['aia_tresp'].numpy()))
    sd = {k[4:].replace('__', '.'): v for k, v in g.items() if k.startswith('sd__')}
    mod.load_state_dict(sd, strict=True)
    mod = mod.cuda()
    assert mod._hooks_replaced(DensityTemperatureRadiativeTransfer)
    target = g['target'] * (pf / float(g['pixel_intensity_factor']))

    def loss_of(out, mse=torch.nn.functional.mse_loss):
        return (mse(out['coarse_image'], target.to(out['coarse_image'].device))
                + mse(out['fine_image'], target.to(out['fine_image'].device))
                + out['regularization'].mean() + height_weight * out['height_map'].sum())

    # oracle: the same composition, fp32 autograd
    leaves = {k: v.clone().requires_grad_(True) for k, v in sd.items() if k.endswith(('weight', 'bias')) or 'log_absortpion' in k
              or k.endswith('volumetric_constant')}

    def params_of(prefix):
        return orc.params_from_state_dict({k: leaves.get(k, v) for k, v in sd.items()}, prefix)
    la = {p: {str(w): leaves[f'{p}.log_absortpion.{w}'] for w in orc.AIA_WAVELENGTHS} for p in ('coarse_model', 'fine_model')}
    t_vals = sd['sampler.t_vals']
    o, d, t, wl = g['rays_o'], g['rays_d'], g['times'], g['wavelengths']
    z = orc.stratified_z(o, d, t_vals, torch.tensor(1.3), torch.tensor(1.))
    c = orc.render_pass_dt(params_of('coarse_model.'), la['coarse_model'], leaves['coarse_model.volumetric_constant'], o, d, t,
                           z, wl, g['aia_logte'], resp, pf)
    _, z_comb = orc.hierarchical_z(z, c['weights'], 16)
    f = orc.render_pass_dt(params_of('fine_model.'), la['fine_model'], leaves['fine_model.volumetric_constant'], o, d, t,
                           z_comb, wl, g['aia_logte'], resp, pf)
    dist = f['points'].pow(2).sum(-1).pow(0.5)
    want = {'coarse_image': c['image'], 'fine_image': f['image'], 'height_map': (f['weights'] * dist).sum(-1),
            'regularization': torch.relu(dist - 1.1) * torch.relu(f['regularizing_quantity'])}
    # the two terms this path used to drop carry a real share of the MLP gradients
    first = leaves['fine_model.layers.0.weight']
    total = torch.autograd.grad(loss_of(want), [first], retain_graph=True)[0].norm()
    parts = {'image': torch.nn.functional.mse_loss(want['fine_image'], target), 'regularization': want['regularization'].mean(),
             'height_map': height_weight * want['height_map'].sum()}
    share = {k: (torch.autograd.grad(v, [first], retain_graph=True)[0].norm() / total).item() for k, v in parts.items()}
    print('share of the fine model\'s first-layer gradient', {k: f'{v:.1e}' for k, v in share.items()})
    if pixel_factor is not None:
        assert all(v > 1e-2 for v in share.values()), share
    loss_of(want).backward()

    got = mod(o.cuda(), d.cuda(), t.cuda(), wl.cuda())
    loss = loss_of(got)
    assert abs(loss.item() - loss_of(want).item()) < 2e-4 * abs(loss_of(want).item())
    loss.backward()
    named = [(k, p) for k, p in mod.named_parameters()]
    assert {k for k, _ in named} == set(leaves), set(leaves) ^ {k for k, _ in named}
    _compare_grads(named, leaves, 1e-3, 'generic DT path')


def test_generic_path_simple_star_gradients():
    """SimpleStar through the generic path (its own forward on the query points, raw2outputs on the DT integral node)."""
    from sunerf.rendering.density_temperature import DensityTemperatureRadiativeTransfer

    class WiderRegularization(DensityTemperatureRadiativeTransfer):
        def regularization(self, distance, regularizing_quantity):
            return torch.relu(distance - 1.1 / self.Rs_per_ds) * torch.relu(regularizing_quantity)
    g = _g9()
    fused = _star_module(g)
    mod = WiderRegularization(Rs_per_ds=1, model=type(fused.coarse_model), model_config={},
                              sampling_config={'type': 'stratified', 'n_samples': 24, 'perturb': False},
                              hierarchical_sampling_config={'type': 'hierarchical', 'n_samples': 24},
                              pixel_intensity_factor=float(g['pixel_intensity_factor']),
                              response_table=(g['aia_logte'].numpy(), g['aia_tresp'].numpy())).cuda()
    mod.load_state_dict(fused.state_dict())
    assert mod._hooks_replaced(DensityTemperatureRadiativeTransfer)
    coarse, fine = _oracle_star(mod.coarse_model), _oracle_star(mod.fine_model)
    want = oracle_star_render(coarse, fine, g['rays_o'], g['rays_d'], g['wavelengths'], g['aia_logte'], g['resp'], 24, 24,
                              float(g['pixel_intensity_factor']), reg_radius=1.1)
    target = (want['fine_image'] * 0.8).detach()

    def loss_of(out):
        return (torch.nn.functional.mse_loss(out['coarse_image'], target.to(out['coarse_image'].device))
                + torch.nn.functional.mse_loss(out['fine_image'], target.to(out['fine_image'].device))
                + out['regularization'].mean())
    loss_of(want).backward()
    got = mod(g['rays_o'].cuda(), g['rays_d'].cuda(), g['times'].cuda(), g['wavelengths'].cuda())
    loss_of(got).backward()
    leaves = {**_named_oracle_leaves('coarse_model', coarse), **_named_oracle_leaves('fine_model', fine)}
    _compare_grads(mod.named_parameters(), leaves, 1e-3, 'generic path, SimpleStar')


# ---- 5. end to end: recover h0 and T0 ---------------------------------------------------------------------------------
def test_fit_simple_star_recovers_h0_and_T0():
    """Targets rendered from the default star; a second star starts from h0 + 20 % and T0 - 15 % and is fitted with Adam
    (the other parameters fixed) on g9's limb-crossing rays.  On the oracle the same schedule recovers both to ~1e-6."""
    g = _g9()
    mod = _star_module(g)
    with torch.no_grad():
        for m in (mod.coarse_model, mod.fine_model):           # both stars at the defaults for the targets
            m.stellar_parameters['h0'].copy_(g['sp__h0'])
            m.stellar_parameters['T0'].copy_(g['sp__T0'])
            m.log_absortpion['171'].copy_(g['la__171'])
    args = (g['rays_o'].cuda(), g['rays_d'].cuda(), g['times'].cuda(), g['wavelengths'].cuda())
    with torch.no_grad():
        target = mod(*args)
    mask = target['fine_image'] > 0
    h0_true, T0_true = g['sp__h0'].item(), g['sp__T0'].item()
    h0s, T0s = [], []
    for p in mod.parameters():
        p.requires_grad_(False)
    with torch.no_grad():
        for m in (mod.coarse_model, mod.fine_model):
            m.stellar_parameters['h0'].mul_(1.2).requires_grad_(True)
            m.stellar_parameters['T0'].mul_(0.85).requires_grad_(True)
            h0s.append(m.stellar_parameters['h0'])
            T0s.append(m.stellar_parameters['T0'])
    steps = 300
    opt = torch.optim.Adam([{'params': h0s, 'lr': 3e-3}, {'params': T0s, 'lr': 4e4}])
    sched = torch.optim.lr_scheduler.ExponentialLR(opt, gamma=0.1 ** (1 / steps))

    def rel_mse(img, tgt):
        return ((img[mask] - tgt[mask]) / tgt[mask]).pow(2).mean()
    for i in range(steps):
        opt.zero_grad()
        out = mod(*args)
        loss = rel_mse(out['coarse_image'], target['coarse_image']) + rel_mse(out['fine_image'], target['fine_image'])
        loss.backward()
        opt.step()
        sched.step()
        if i % 50 == 0 or i == steps - 1:
            print(f'step {i:3d} loss {loss.item():.3e} h0 {h0s[1].item() / h0_true - 1:+.2e} T0 {T0s[1].item() / T0_true - 1:+.2e}')
    for name, ps, true in (('h0', h0s, h0_true), ('T0', T0s, T0_true)):
        for which, p in zip(('coarse', 'fine'), ps):
            err = abs(p.item() / true - 1)
            print(f'{which} {name}: recovered {p.item():.6g}, true {true:.6g}, rel err {err:.1e} (bound 2e-2)')
            assert err < 2e-2, (which, name, err)
