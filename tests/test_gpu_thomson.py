"""White-light Thomson scattering on MI355X (csrc/thomson.hip, sunerf/rendering/thompson.py) against the fp64 restatement
of tests/thomson_reference.py: the integral kernels alone, the fused NeRF pass against the oracle MLP, the generic path,
the SimpleStar and MHD fields, and the loader.

Bounds: every forward output at the parity gate (gate_units, 1e-4 per element); g_raw within 1e-5 of the batch's max |g|;
parameter gradients within 1e-3 (norm-relative) of fp64 autograd."""
import datetime
import math

import numpy as np
import pytest
import torch

import thomson_reference as tr
from conftest import gate_units

pytestmark = pytest.mark.gpu

LN10 = math.log(10.)
KEYS = tr.KEYS


@pytest.fixture(scope='module')
def ops():
    assert torch.cuda.is_available(), 'GPU tests need a ROCm device'
    from sunerf_hip import ops as _ops
    return _ops


def _consts(radius=1.0, limb=0.63, c0=1.0):
    return tuple(torch.tensor(v, dtype=torch.float32, device='cuda') for v in (radius, limb, c0))


def make_case(n, s, c, seed, impact=(0.0, 3.0), far=False):
    """Rays from ~215 R towards targets at impact parameters ``impact`` (some through the Sun, one grazing the limb), a third of
    them with non-unit directions; samples from the observer to past the Sun (out to 215 R).  ``far``: samples only at
    r = 50 ... 215 R."""
    gen = torch.Generator().manual_seed(seed)
    o = torch.randn(n, 3, generator=gen)
    o = o / o.norm(dim=1, keepdim=True) * (200. + 30. * torch.rand(n, 1, generator=gen))
    t = torch.randn(n, 3, generator=gen)
    t = t - (t * o).sum(1, keepdim=True) / o.pow(2).sum(1, keepdim=True) * o        # perpendicular to o
    p = impact[0] + (impact[1] - impact[0]) * torch.rand(n, 1, generator=gen)
    if not far:
        p[0] = 1.0                                                                      # grazes the limb
    target = t / t.norm(dim=1, keepdim=True) * p
    d = target - o
    dist = d.norm(dim=1, keepdim=True)
    d = d / dist
    scale = torch.where(torch.arange(n)[:, None] % 3 == 0, 0.5 + 1.5 * torch.rand(n, 1, generator=gen), torch.ones(n, 1))
    d = (d * scale).float()
    if far:
        z = dist * (0.05 + 0.7 * torch.rand(n, s, generator=gen))
    else:
        z = dist * 2 * torch.rand(n, s, generator=gen)
        z[0, s // 2] = dist[0, 0]                                                      # the limb sample of ray 0
    z = (z / scale).sort(dim=1).values.float()
    kappa = LN10 if c == 2 else 1.0
    raw = torch.randn(n, s, c, generator=gen) * (0.7 if c == 2 else 1.6)
    return raw.float().contiguous(), z.contiguous(), o.float().contiguous(), d.contiguous(), kappa


def _cuda(*ts):
    return [t.cuda() for t in ts]


def _ratio_terms(raw, z, o, d, kappa, grads):
    """max over samples of kappa rho_j (|g_sun| r_j + |g_obs| z_j |d| + |g_w,j| + sum_k |g_w,k| w_k) / (M + 1e-10)."""
    rho = torch.exp(kappa * raw[..., 0].double())
    m = rho.sum(-1, keepdim=True) + 1e-10
    r = (o[:, None, :].double() + d[:, None, :].double() * z[..., None].double()).norm(dim=-1)
    t = torch.zeros_like(rho)
    if 'distance_from_sun' in grads:
        t = t + grads['distance_from_sun'].abs()[:, None] * r
    if 'distance_from_obs' in grads:
        t = t + grads['distance_from_obs'].abs()[:, None] * z.double() * d.double().norm(dim=-1, keepdim=True)
    if 'weights' in grads:
        gw = grads['weights'].abs()
        t = t + gw + (gw * rho / m).sum(-1, keepdim=True)
    return (kappa * rho * t / m).max().item()


SHAPES = [(1, 1), (7, 2), (9, 31), (13, 32), (33, 33), (5, 64), (130, 192), (17, 320)]


@pytest.mark.parametrize('c', [1, 2])
@pytest.mark.parametrize('n,s', SHAPES)
def test_integral_forward_and_backward_match_fp64(ops, n, s, c):
    raw, z, o, d, kappa = make_case(n, s, c, seed=1000 * s + n + c)
    want = tr.thomson_integral(raw, z, o, d, kappa)
    consts = _consts()
    got = ops.thomson_integral_fwd(*_cuda(raw, z, o, d), consts, kappa)
    units = {k: gate_units(got[k], want[k]) for k in KEYS}
    print(f'N={n} S={s} C={c}: gate units', {k: round(v, 3) for k, v in units.items()})
    assert all(v <= 1.0 for v in units.values()), units
    if s > 1:
        assert bool((want['pixel_B'][:, 0] > 0).any())
    # reruns are bit-identical
    again = ops.thomson_integral_fwd(*_cuda(raw, z, o, d), consts, kappa)
    assert all(torch.equal(got[k], again[k]) for k in KEYS)

    # backward: each output's gradient alone, then all five together, against fp64 autograd
    gen = torch.Generator().manual_seed(s + n)
    upstream = {k: torch.randn(want[k].shape, generator=gen, dtype=torch.float64) for k in KEYS}
    for chosen in [(k,) for k in KEYS] + [KEYS]:
        leaf = raw.double().requires_grad_(True)
        ref = tr.thomson_integral(leaf, z, o, d, kappa)
        loss = sum((ref[k] * upstream[k]).sum() for k in chosen)
        # S = 1: tB, pB and pixel_density are the empty sums, independent of raw
        g_ref = torch.autograd.grad(loss, leaf)[0] if loss.requires_grad else torch.zeros_like(leaf)
        gs = {k: (upstream[k].float().cuda() if k in chosen else None) for k in KEYS}
        g_raw, absmax = ops.thomson_integral_bwd(*_cuda(raw, z, o, d), consts, kappa, gs['pixel_B'], gs['pixel_density'],
                                                 gs['distance_from_sun'], gs['distance_from_obs'], gs['weights'])
        g = g_raw.cpu().double()
        assert g.shape == (n, s, c)
        if c == 2:
            assert bool((g[..., 1] == 0).all())
        scale = g_ref.abs().max().item()
        err = (g - g_ref).abs().max().item()
        # the ratio outputs' gradient is a difference of two terms of size kappa rho (|g| r) / M: fp32 holds it to a few ulp of
        # those terms, and with S = 1 it cancels to the 1e-10 of the denominator alone
        floor = 8 * 2.0 ** -24 * _ratio_terms(raw, z, o, d, kappa, {k: upstream[k] for k in chosen})
        assert err <= 1e-5 * scale + floor, (chosen, err, scale, floor)
        m = g_raw.abs().max().float().item()
        assert absmax.view(torch.float32).item() == m, (absmax.view(torch.float32).item(), m)
        g2, _ = ops.thomson_integral_bwd(*_cuda(raw, z, o, d), consts, kappa, gs['pixel_B'], gs['pixel_density'],
                                         gs['distance_from_sun'], gs['distance_from_obs'], gs['weights'])
        assert torch.equal(g_raw, g2)


def test_far_field_holds_the_gate_where_the_literal_fp32_formula_does_not(ops):
    """Samples at r = 50 ... 215 R: the reference's fp32 geometry misses the gate, the kernel's fp64 geometry holds it."""
    raw, z, o, d, kappa = make_case(64, 96, 2, seed=5, impact=(50., 190.), far=True)
    pts = o[:, None, :].double() + d[:, None, :].double() * z[..., None].double()
    r = pts.norm(dim=-1)
    assert r.min() > 45. and r.max() < 232.
    want = tr.thomson_integral(raw, z, o, d, kappa)
    got = ops.thomson_integral_fwd(*_cuda(raw, z, o, d), _consts(), kappa)
    literal = tr.thomson_literal_fp32(raw, z, o, d)
    kernel_units, literal_units = gate_units(got['pixel_B'], want['pixel_B']), gate_units(literal, want['pixel_B'])
    print(f'far field: kernel {kernel_units:.3f} gate units, literal fp32 {literal_units:.1f}')
    assert kernel_units <= 1.0
    assert literal_units > 1.0


def test_non_finite_inputs_propagate(ops):
    raw, z, o, d, kappa = make_case(8, 40, 2, seed=3)
    z[2, 5] = float('nan')
    raw[4, 7, 0] = 40.                # 10^40 overflows fp32
    got = ops.thomson_integral_fwd(*_cuda(raw, z, o, d), _consts(), kappa)
    want = tr.thomson_integral(raw, z, o, d, kappa, dtype=torch.float32)
    for k in ('pixel_B', 'pixel_density', 'distance_from_sun', 'distance_from_obs'):
        fin = torch.isfinite(got[k].cpu())
        assert torch.equal(fin, torch.isfinite(want[k])), k
        assert not bool(fin[2].all()) and not bool(fin[4].all())
        assert bool(fin[[0, 1, 3, 5, 6, 7]].all())


# ---- the fused NeRF pass --------------------------------------------------------------------------------------------------
def _nerf_module(d_filter, n_coarse=48, n_fine=48, seed=0, cls=None, Rs_per_ds=1.0):
    from sunerf.rendering.thompson import ThompsonScattering
    torch.manual_seed(seed)
    return (cls or ThompsonScattering)(Rs_per_ds=Rs_per_ds, sampling_config={'type': 'stratified', 'n_samples': n_coarse, 'perturb': False},
                              hierarchical_sampling_config={'type': 'hierarchical', 'n_samples': n_fine},
                              model_config={'d_filter': d_filter}).cuda()


def _rays(n, seed=0):
    gen = torch.Generator().manual_seed(seed)
    o = torch.tensor([-63.2288, 204.4016, -21.4674]).expand(n, 3).contiguous()
    target = (torch.rand(n, 3, generator=gen) * 2 - 1) * 1.3
    d = target - o
    return o, (d / d.norm(dim=1, keepdim=True)).contiguous(), torch.rand(n, 1, generator=gen)


def _oracle_pass(params64, o, d, t, z, **constants):
    import sunerf_oracle as orc
    pts = orc.points_on_rays(o, d, z)
    q = torch.cat([pts, t.reshape(-1, 1, 1).expand(-1, z.shape[1], 1)], -1).double()
    raw = orc.mlp_forward(params64, q.reshape(-1, 4)).reshape(*z.shape, -1)
    return tr.thomson_integral(raw, z, o, d, LN10, **constants)


def _params(model, requires_grad=False):
    import sunerf_oracle as orc
    sd = {k: v.detach().cpu() for k, v in model.state_dict().items()}
    return [(W.double().requires_grad_(requires_grad), b.double().requires_grad_(requires_grad))
            for W, b in orc.params_from_state_dict(sd, '')]


@pytest.mark.parametrize('d_filter', [64, 256])
def test_fused_render_matches_oracle(precision, d_filter):
    mod = _nerf_module(d_filter)
    o, d, t = _rays(200, seed=d_filter)
    with torch.no_grad():
        got = mod(*_cuda(o, d, t))
    assert got['image'].shape == (200, 2) and got['coarse_image'].shape == (200, 2)
    z_c = got['z_vals_stratified'].cpu()
    z_f = torch.sort(torch.cat([z_c, got['z_vals_hierarchical'].cpu()], -1), -1).values
    coarse = _oracle_pass(_params(mod.coarse_model), o, d, t, z_c)
    fine = _oracle_pass(_params(mod.fine_model), o, d, t, z_f)
    assert bool((fine['pixel_B'][:, 0] > 0).all())
    units = {'coarse_image': gate_units(got['coarse_image'], coarse['pixel_B']),
             'fine_image': gate_units(got['fine_image'], fine['pixel_B']),
             'height_map': gate_units(got['height_map'], fine['distance_from_sun'])}       # sum w r = sum rho r / (M + 1e-10)
    for k in ('pixel_density', 'distance_from_sun', 'distance_from_obs'):
        units[k] = gate_units(got[k], fine[k])
    print(f'fused d_filter={d_filter} {precision}: gate units', {k: round(v, 3) for k, v in units.items()})
    assert all(v <= 1.0 for v in units.values()), units
    assert torch.equal(got['absorption_map'], torch.zeros_like(got['absorption_map']))
    assert torch.equal(got['regularization'], torch.zeros_like(got['regularization']))
    assert got['regularization'].shape == z_f.shape


def _grad_check(model, params64, what, bound=1e-3):
    n_hidden = len(params64) - 2
    names = ['in_layer.1'] + [f'layers.{i}' for i in range(n_hidden)] + ['out_layer']
    named = dict(model.named_parameters())
    worst = {}
    pairs = []
    for prefix, (W, b) in zip(names, params64):
        pairs += [(prefix + '.weight', W), (prefix + '.bias', b)]
    assert len(pairs) == len(named)
    for name, ref in pairs:
        p = named[name]
        assert p.grad is not None, (what, name)
        err = ((p.grad.detach().cpu().double() - ref.grad).norm() / ref.grad.norm()).item()
        worst[name] = err
    print(what, {k: f'{v:.1e}' for k, v in worst.items()})
    assert all(v < bound for v in worst.values()), worst


@pytest.mark.parametrize('flat_bucket', [False, True])
@pytest.mark.parametrize('d_filter', [64, 256])
def test_fused_pass_parameter_gradients(precision, d_filter, flat_bucket):
    from sunerf.rendering.functional import thomson_pass
    from sunerf_hip.train import ClipAdam
    mod = _nerf_module(d_filter)
    model = mod.fine_model
    o, d, t = _rays(64, seed=3)
    z = mod.sampler.z_vals(*_cuda(o, d)).cpu()
    assert z.numel() <= 4096
    p64 = _params(model, requires_grad=True)
    want = _oracle_pass(p64, o, d, t, z)
    target = (want['pixel_B'] * 0.8).detach()
    ((want['pixel_B'] - target) ** 2).mean().backward()
    if flat_bucket:
        opt = ClipAdam(list(model.parameters()), lr=1e-3)
        opt.zero_grad()
        slots = {id(p): p.grad.data_ptr() for p in model.parameters()}
    out = thomson_pass(model, mod._constants(), *_cuda(o, d, t, z))
    assert out['pixel_B'].requires_grad and not out['weights'].requires_grad
    loss = ((out['pixel_B'] - target.float().cuda()) ** 2).mean()
    loss.backward()
    if flat_bucket:
        assert all(p.grad.data_ptr() == slots[id(p)] for p in model.parameters())
    _grad_check(model, p64, f'fused pass d_filter={d_filter} {precision} flat={flat_bucket}')


def test_fused_forward_equals_generic_path():
    from sunerf.rendering.thompson import ThompsonScattering

    class Generic(ThompsonScattering):
        def raw2outputs(self, **state):
            return super().raw2outputs(**state)

    fused = _nerf_module(64, seed=4)
    generic = _nerf_module(64, seed=5, cls=Generic)
    generic.load_state_dict(fused.state_dict())
    assert generic._hooks_replaced(ThompsonScattering) and not fused._hooks_replaced(ThompsonScattering)
    o, d, t = _cuda(*_rays(64, seed=6))
    a, b = fused(o, d, t), generic(o, d, t)
    for k in ('z_vals_stratified', 'z_vals_hierarchical'):
        assert torch.equal(a[k], b[k]), k
    units = {k: gate_units(b[k], a[k].cpu()) for k in ('coarse_image', 'fine_image', 'image', 'height_map')}
    print('fused vs generic: gate units', units)
    assert all(v <= 1.0 for v in units.values()), units
    assert torch.equal(b['absorption_map'].cpu(), a['absorption_map'].cpu())
    assert torch.equal(b['regularization'].cpu(), a['regularization'].cpu())
    target = a['image'].detach() * 0.8
    for m, out in ((fused, a), (generic, b)):
        m.zero_grad()
        (((out['coarse_image'] - target) ** 2).mean() + ((out['fine_image'] - target) ** 2).mean()).backward()
    for (name, p), q in zip(fused.named_parameters(), generic.parameters()):
        err = ((p.grad - q.grad).norm() / q.grad.norm()).item()
        assert err < 1e-3, (name, err)


# ---- field modules --------------------------------------------------------------------------------------------------------
def _star_module(Rs_per_ds=1.0):
    from sunerf.model.stellar_model import SimpleStar
    from sunerf.rendering.thompson import ThompsonScattering
    return ThompsonScattering(Rs_per_ds=Rs_per_ds, model=SimpleStar, model_config={},
                              sampling_config={'type': 'stratified', 'n_samples': 40, 'perturb': False},
                              hierarchical_sampling_config={'type': 'hierarchical', 'n_samples': 40}).cuda()


def _star_ln_rho(sp, pts):
    """SimpleStar's ln rho in fp64 (stellar_model.py:53-102): ln rho_0 inside r <= 1, ln rho_0 + (1/r - 1) / h0 beyond."""
    r = pts.double().norm(dim=-1)
    ln0 = torch.log(sp['rho_0'])
    return torch.where(r <= 1, ln0.expand_as(r), ln0 + (1 / r - 1) / sp['h0'])


def test_simple_star_render_and_stellar_gradients():
    import sunerf_oracle as orc
    mod = _star_module()
    o, d, t = _rays(96, seed=8)
    out = mod(*_cuda(o, d, t))
    z_c = out['z_vals_stratified'].detach().cpu()
    z_f = torch.sort(torch.cat([z_c, out['z_vals_hierarchical'].detach().cpu()], -1), -1).values
    leaves = {}
    want = {}
    for name, m, z in (('coarse', mod.coarse_model, z_c), ('fine', mod.fine_model, z_f)):
        sp = {k: m.stellar_parameters[k].detach().cpu().double().requires_grad_(True) for k in ('rho_0', 'h0', 'Rs', 'T0')}
        leaves[name] = sp
        ln_rho = _star_ln_rho(sp, orc.points_on_rays(o, d, z))
        want[name] = tr.thomson_integral(ln_rho[..., None], z, o, d, 1.0)
    assert bool((want['fine']['pixel_B'][:, 0] > 0).all())
    units = {'coarse_image': gate_units(out['coarse_image'], want['coarse']['pixel_B']),
             'fine_image': gate_units(out['fine_image'], want['fine']['pixel_B']),
             'pixel_density': gate_units(out['pixel_density'], want['fine']['pixel_density']),
             'distance_from_sun': gate_units(out['distance_from_sun'], want['fine']['distance_from_sun'])}
    print('SimpleStar white light: gate units', units)
    assert all(v <= 1.0 for v in units.values()), units
    target = want['fine']['pixel_B'].detach() * 0.9
    (((want['coarse']['pixel_B'] - target) ** 2).mean() + ((want['fine']['pixel_B'] - target) ** 2).mean()).backward()
    loss = ((out['coarse_image'] - target.float().cuda()) ** 2).mean() + ((out['fine_image'] - target.float().cuda()) ** 2).mean()
    loss.backward()
    for name, m in (('coarse', mod.coarse_model), ('fine', mod.fine_model)):
        for k in ('rho_0', 'h0'):
            ref, got = leaves[name][k].grad.item(), m.stellar_parameters[k].grad.item()
            assert abs(got - ref) <= 1e-3 * abs(ref), (name, k, got, ref)
        for k in ('Rs', 'T0'):          # temperature does not enter white light
            g = m.stellar_parameters[k].grad
            assert g is None or g.item() == 0.0, (name, k)


def test_mhd_cube_renders_in_white_light(tmp_path):
    import mhd_reference as mref
    import sunerf_oracle as orc
    from sunerf.model.mhd_model import MHDModel
    from sunerf.rendering.thompson import ThompsonScattering
    frames = {10: mref.synthetic_frame(1), 11: mref.synthetic_frame(2), 12: mref.synthetic_frame(3)}
    root = mref.write_placeholders(tmp_path / 'run', sorted(frames))
    mod = ThompsonScattering(Rs_per_ds=1.0, model=MHDModel, model_config={'data_path': str(root), 'reader': mref.DictReader(frames)},
                             sampling_config={'type': 'stratified', 'n_samples': 32, 'perturb': False},
                             hierarchical_sampling_config={'type': 'hierarchical', 'n_samples': 32}).cuda()
    o, d, _ = _rays(128, seed=9)
    t = torch.full((128, 1), 0.3)
    with torch.no_grad():
        out = mod(*_cuda(o, d, t))
    z_c = out['z_vals_stratified'].cpu()
    z_f = torch.sort(torch.cat([z_c, out['z_vals_hierarchical'].cpu()], -1), -1).values
    for key, z in (('coarse_image', z_c), ('fine_image', z_f)):
        pts = orc.points_on_rays(o, d, z)
        q = torch.cat([pts, torch.full_like(pts[..., :1], 0.3)], -1).reshape(-1, 4)
        raw = mref.mhd_field(q, frames, 10, 12).reshape(*z.shape, 2)
        want = tr.thomson_integral(raw, z, o, d, 1.0)
        assert bool((want['pixel_B'][:, 0] > 0).any())
        u = gate_units(out[key], want['pixel_B'])
        print(f'MHD white light {key}: {u:.3f} gate units')
        assert u <= 1.0


def test_loader_frame_equals_direct_render(tmp_path):
    from sunerf.evaluation.loader import SuNeRFLoader, linear_plate_scale_axes
    from sunerf.model.sunerf import save_state
    from sunerf_hip.rays import grid_rays, pose_spherical
    rendering = _nerf_module(64, n_coarse=16, n_fine=16, seed=11)

    class _Module:
        pass

    class _Data:
        config = {'wavelength': None, 'times': [datetime.datetime(2022, 1, 1), datetime.datetime(2022, 1, 3)],
                  'resolution': (16, 16), 'wcs': {'shape': (16, 16), 'cdelt': (150., 150.)}}
        Rs_per_ds, seconds_per_dt, ref_time = 1.0, 86400., datetime.datetime(2022, 1, 1)
    holder = _Module()
    holder.rendering = rendering
    path = str(tmp_path / 'run' / 'save_state.snf')
    save_state(holder, _Data(), path)
    loader = SuNeRFLoader(path, device='cuda')
    when = datetime.datetime(2022, 1, 2, 12)
    out = loader.render_observer_image(lat=0.1, lon=0.3, time=when, batch_size=100)
    assert out['pixel_B'].shape == (16, 16, 2) and out['image'].shape == (16, 16, 2)
    assert np.isfinite(out['pixel_B']).all() and out['pixel_B'][..., 0].max() > 0
    tx, ty = linear_plate_scale_axes(_Data.config['wcs'], None, 'cuda')
    o, d, t = grid_rays(tx, ty, pose_spherical(-0.3, 0.1, 215.03215567054764), time=1.5)
    with torch.no_grad():
        ref = rendering(o, d, t)
    assert np.array_equal(out['pixel_B'].reshape(-1), ref['image'].cpu().numpy().reshape(-1))
    assert np.array_equal(out['distance_from_obs'].reshape(-1), ref['distance_from_obs'].cpu().numpy().reshape(-1))
