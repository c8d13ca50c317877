"""MHD simulation cube behind the DT integral on MI355X (csrc/mhd.hip, sunerf/model/mhd_model.py) against the fp64
restatement of the reference's MHDModel (tests/mhd_reference.py) and the oracle's DT renderer around it.

Synthetic frames 10, 11, 12 (frame 11 on another grid), r from 1.02 (1.03) to 1.4 (1.35) solar radii: the rays cross the inner and the
outer bound of the cube, the theta grid stops short of the poles and the phi grid short of 2 pi."""
import numpy as np
import pytest
import torch

import mhd_reference as ref
from conftest import gate_units, load_golden

pytestmark = pytest.mark.gpu

FFIRST, FLAST = 10, 12
WAVELENGTHS = (94, 131, 171, 193, 211, 304, 335)
LOG_ABS = (2e-9, 3e-9, 4e-9, 5e-9, 6e-9, 7e-9, 8e-9)     # optical depths of order one for densities ~1e8


def _frames():
    return {10: ref.synthetic_frame(1),
            11: ref.synthetic_frame(2, n_phi=19, n_theta=21, n_r=33, r_range=(1.03, 1.35), phi_end=0.93 * 2 * np.pi),
            12: ref.synthetic_frame(3)}


def _simulation(tmp_path):
    frames = _frames()
    root = ref.write_placeholders(tmp_path / 'run', sorted(frames))
    return root, ref.DictReader(frames), frames


def _points(n, seed, times):
    """Points at radii 0.9 ... 1.5 in every direction (inside, in and beyond the cube), each at one of ``times``."""
    gen = torch.Generator().manual_seed(seed)
    d = torch.randn(n, 3, generator=gen)
    d = d / d.norm(dim=1, keepdim=True)
    rad = 0.9 + 0.6 * torch.rand(n, 1, generator=gen)
    t = torch.tensor(times, dtype=torch.float32)[torch.randint(len(times), (n,), generator=gen)]
    return torch.cat([d * rad, t[:, None]], 1).float()


def _check_field(got, want, what):
    got = got.detach().cpu()
    nan = torch.isnan(want)
    assert torch.equal(torch.isnan(got), nan), what
    fill = torch.tensor([np.log(np.float32(1e-10)), np.log10(np.float32(1e6) * np.float32(1e-10))], dtype=torch.float32)
    is_fill = (want == fill).all(-1)
    assert is_fill.any() and (~is_fill & ~nan.any(-1)).sum() > 0.2 * want.shape[0], what
    err_fill = (got[is_fill] - want[is_fill]).abs().max().item()
    inside = ~is_fill & ~nan.any(-1)
    err = (got[inside] - want[inside]).abs().max(0).values
    print(f'{what}: {inside.sum().item()} in-bounds, {is_fill.sum().item()} filled, {nan.any(-1).sum().item()} NaN; '
          f'max |err| ln rho {err[0]:.2e}, log10 T {err[1]:.2e}, fill {err_fill:.1e}')
    assert err_fill <= 1e-6, what
    assert (err <= 2e-5).all(), (what, err)


def test_points_and_rays_kernels_match_restatement(tmp_path):
    from sunerf.model.mhd_model import MHDModel
    root, reader, frames = _simulation(tmp_path)
    model = MHDModel(root, reader=reader).cuda()
    times = (0.0, 0.5, 1.0, 0.3, 0.8)           # exact frames 10 / 11 (w = 0), t = 1 (f1 = f2 = 12), between frames
    pts = _points(6000, 1, times)
    pts[7, 0] = float('nan')                    # NaN coordinate
    pts[8, :3] = 0.                             # r = 0: theta = acos(0 / 0) = NaN
    out = model(pts.cuda())
    assert set(out) == {'rho_T', 'inferences', 'log_abs', 'vol_c'} and out['rho_T'] is out['inferences']
    want = ref.mhd_field(pts, frames, FFIRST, FLAST)
    assert torch.isnan(want[7]).all() and torch.isnan(want[8]).all()
    _check_field(out['inferences'], want, 'points mode')
    # rays mode: o + d z formed in the kernel, one time per ray
    gen = torch.Generator().manual_seed(2)
    n, s = 300, 40
    o = torch.tensor([0.3, -2.8, 0.5]).expand(n, 3).contiguous()
    target = torch.randn(n, 3, generator=gen) * 0.7
    d = (target - o)
    d = (d / d.norm(dim=1, keepdim=True)).contiguous()
    z = torch.sort(torch.rand(n, s, generator=gen), -1).values * 2.4 + 1.7
    t = torch.tensor(times)[torch.randint(len(times), (n,), generator=gen)][:, None].contiguous()
    raw = model.field_on_rays(o.cuda(), d.cuda(), z.cuda(), t.cuda())
    assert raw.shape == (n, s, 2)
    p = o[:, None, :] + d[:, None, :] * z[..., None]
    want = ref.mhd_field(torch.cat([p, t[:, None, :].expand(n, s, 1)], -1).reshape(-1, 4), frames, FFIRST, FLAST)
    _check_field(raw.reshape(-1, 2), want, 'rays mode')


def test_non_resident_frame_is_reported(tmp_path):
    from sunerf.model.mhd_model import MHDModel
    from sunerf_hip import ops
    from sunerf_hip.lib import SunerfHipError
    root, reader, _ = _simulation(tmp_path)
    model = MHDModel(root, reader=reader)
    cache = model.frame_cache('cuda')
    no_slots = torch.full((FLAST - FFIRST + 1,), -1, dtype=torch.int32, device='cuda')
    with pytest.raises(SunerfHipError, match='not resident'):
        ops.mhd_field_points(_points(10, 3, (0.3,)).cuda(), cache.frames, no_slots, FFIRST, FLAST)


def _renderer(root, reader, n_coarse=32, n_fine=32):
    from sunerf.model.mhd_model import MHDModel
    from sunerf.rendering.density_temperature import DensityTemperatureRadiativeTransfer
    g = load_golden('g9_simple_star')
    mod = DensityTemperatureRadiativeTransfer(
        Rs_per_ds=1, model=MHDModel, model_config={'data_path': root, 'reader': reader},
        sampling_config={'type': 'stratified', 'n_samples': n_coarse, 'perturb': False},
        hierarchical_sampling_config={'type': 'hierarchical', 'n_samples': n_fine},
        pixel_intensity_factor=float(g['pixel_intensity_factor']),
        response_table=(g['aia_logte'].numpy(), g['aia_tresp'].numpy())).cuda()
    with torch.no_grad():
        for m in (mod.coarse_model, mod.fine_model):
            for w, v in zip(WAVELENGTHS, LOG_ABS):
                m.log_absortpion[str(w)].fill_(v)
            m.volumetric_constant.fill_(0.8)
    resp = (g['aia_tresp'] * float(g['aia_exp_time'])).float()
    return mod, g['aia_logte'], resp, float(g['pixel_intensity_factor'])


def _rays(n=64, seed=4):
    """Rays from 1 AU through a disk of radius 1.4 around the sun: some end on the surface (inside the cube's inner bound),
    all leave through its outer bound."""
    gen = torch.Generator().manual_seed(seed)
    o = torch.tensor([-63.2288, 204.4016, -21.4674]).expand(n, 3).contiguous()
    axis = -o[0] / o[0].norm()
    u = torch.linalg.cross(axis, torch.tensor([0., 0., 1.]))
    u = u / u.norm()
    v = torch.linalg.cross(axis, u)
    a = torch.rand(n, generator=gen) * 2 * np.pi
    rad = 1.4 * torch.rand(n, generator=gen).sqrt()
    target = rad[:, None] * (torch.cos(a)[:, None] * u + torch.sin(a)[:, None] * v)
    d = target - o
    return o, (d / d.norm(dim=1, keepdim=True)).contiguous()


def _oracle_render(leaves, o, d, t, wl, logte, resp, pixel_factor, frames, t_vals, n_fine):
    """DensityTemperatureRadiativeTransfer(model=MHDModel).forward on the oracle with separate coarse / fine scalars
    ``leaves = ((la dict, vol_c), (la dict, vol_c))`` and the restated field at each ray's time."""
    import sunerf_oracle as orc
    f32 = torch.float32
    z_vals = orc.stratified_z(o, d, t_vals, torch.tensor(1.3, dtype=f32), torch.tensor(1., dtype=f32))

    def one_pass(scalars, z):
        la, vc = scalars
        pts = orc.points_on_rays(o, d, z)
        q = torch.cat([pts, t.reshape(-1, 1, 1).expand(-1, z.shape[1], 1)], -1).reshape(-1, 4)
        inf = ref.mhd_field(q, frames, FFIRST, FLAST).reshape(*pts.shape[:-1], 2)
        out = orc.dt_integral(inf, la, vc, z, wl, logte, resp, pixel_factor)
        out['points'] = pts
        return out
    c = one_pass(leaves[0], z_vals)
    new_z, z_comb = orc.hierarchical_z(z_vals, c['weights'], n_fine)
    f = one_pass(leaves[1], z_comb)
    q = f['regularizing_quantity']
    dist = f['points'].pow(2).sum(-1).pow(0.5)
    return {'z_vals_stratified': z_vals, 'coarse_image': c['image'], 'z_vals_hierarchical': new_z, 'fine_image': f['image'],
            'image': f['image'], 'height_map': (f['weights'] * dist).sum(-1), 'absorption_map': (1 - q).sum(-1),
            'regularization': torch.relu(dist - 1.25) * torch.relu(q)}


def test_two_pass_render_matches_oracle(tmp_path):
    import sunerf_oracle as orc
    root, reader, frames = _simulation(tmp_path)
    mod, logte, resp, pixel_factor = _renderer(root, reader)
    assert set(mod.state_dict()) >= {'fine_model.volumetric_constant', 'coarse_model.log_absortpion.193'}
    assert not any('data' in k or 'frame' in k for k in mod.state_dict())
    o, d = _rays()
    t = torch.full((o.shape[0], 1), 0.3)                  # frames 10 and 11, on different grids
    wl = torch.tensor(WAVELENGTHS, dtype=torch.float32).expand(o.shape[0], 7).contiguous()
    with torch.no_grad():
        got = mod(o.cuda(), d.cuda(), t.cuda(), wl.cuda())
    la = {str(w): torch.tensor(v, dtype=torch.float32) for w, v in zip(WAVELENGTHS, LOG_ABS)}
    want = orc.render_dt_analytic(lambda p: ref.mhd_field(torch.cat([p, torch.full_like(p[:, :1], 0.3)], 1), frames, FFIRST,
                                                          FLAST),
                                  la, torch.tensor(0.8), o, d, wl, logte, resp, Rs_per_ds=1., n_coarse=32, n_fine=32,
                                  pixel_intensity_factor=pixel_factor, t_vals=mod.sampler.t_vals.cpu())
    assert bool((want['image'] > 0).any())
    assert torch.equal(got['z_vals_stratified'].cpu(), want['z_vals_stratified'])
    units = {k: gate_units(got[k], want[k]) for k in ('coarse_image', 'fine_image', 'image', 'height_map', 'absorption_map')}
    print('MHD two-pass render, gate units', {k: round(v, 3) for k, v in units.items()})
    assert all(v <= 1.0 for v in units.values()), units
    # z_vals_hierarchical within 2e-4, but for samples the reference's own inverse CDF may throw a whole coarse bin: where the
    # cube's fill makes the weights exactly zero, a bin's pdf (w + 1e-5) / sum falls below 1e-5 and sampling.py:160's
    # `denom < 1e-5 -> 1` puts the sample at the bin's start, so the CDF is flat there and a 1e-7 change of it moves a
    # sample by up to one bin (the images above carry any effect and are gated per ray)
    dz = (got['z_vals_hierarchical'].cpu() - want['z_vals_hierarchical']).abs()
    bin_width = (want['z_vals_stratified'][:, 1:] - want['z_vals_stratified'][:, :-1]).max().item()
    print(f'z_vals_hierarchical: {(dz >= 2e-4).sum().item()} of {dz.numel()} samples beyond 2e-4, max {dz.max().item():.2e}')
    assert (dz >= 2e-4).float().mean().item() <= 0.01 and dz.max().item() <= 1.01 * bin_width
    reg = want['regularization']
    assert (got['regularization'].cpu() - reg).abs().max().item() / reg.abs().max().item() < 2e-4


@pytest.mark.parametrize('flat_bucket', [False, True])
def test_absorption_and_volumetric_gradients_match_oracle_autograd(tmp_path, flat_bucket):
    """``flat_bucket``: with a ``ClipAdam`` over the module's parameters (gradients are views of one flat buffer) the DT
    backward adds the seven absorption scalars' and the volumetric constant's gradients straight into that buffer."""
    root, reader, frames = _simulation(tmp_path)
    mod, logte, resp, pixel_factor = _renderer(root, reader, 24, 24)
    with torch.no_grad():
        mod.fine_model.log_absortpion['171'].mul_(1.5)     # coarse and fine differ: a gradient in the wrong instance shows
        mod.fine_model.volumetric_constant.mul_(1.2)
    o, d = _rays(48, 5)
    t = torch.full((o.shape[0], 1), 0.8)
    wl = torch.tensor(WAVELENGTHS, dtype=torch.float32).expand(o.shape[0], 7).clone()
    wl[::5, 2] = 0.                                         # some absent channels
    leaf = lambda p: p.detach().cpu().clone().requires_grad_(True)      # noqa: E731
    leaves = {name: leaf(p) for name, p in mod.named_parameters()}
    scalars = [({str(w): leaves[f'{m}.log_absortpion.{w}'] for w in WAVELENGTHS}, leaves[f'{m}.volumetric_constant'])
               for m in ('coarse_model', 'fine_model')]
    want = _oracle_render(scalars, o, d, t, wl, logte, resp, pixel_factor, frames, mod.sampler.t_vals.cpu(), 24)
    target = (want['fine_image'] * 0.5).detach()        # residuals of one sign: the scalar gradients do not cancel
    mse = torch.nn.functional.mse_loss
    ref_loss = mse(want['coarse_image'], target) + mse(want['fine_image'], target) + want['regularization'].mean()
    ref_loss.backward()
    if flat_bucket:
        from sunerf_hip.train import ClipAdam, bucket_of
        optimizer = ClipAdam(mod.parameters())       # (held: a parameter's bucket tag refers to its optimiser weakly)
        optimizer.zero_grad()
        assert all(bucket_of(p) is not None for p in mod.parameters())
    got = mod(o.cuda(), d.cuda(), t.cuda(), wl.cuda())
    tc = target.cuda()
    loss = mse(got['coarse_image'], tc) + mse(got['fine_image'], tc) + got['regularization'].mean()
    assert abs(loss.item() - ref_loss.item()) < 2e-4 * abs(ref_loss.item()), (loss.item(), ref_loss.item())
    loss.backward()
    if flat_bucket:        # every .grad is still its slot of the bucket: nothing replaced a view
        for name, p in mod.named_parameters():
            owner, off, k = bucket_of(p)
            assert p.grad.data_ptr() == owner.flat_grads[off:off + k].data_ptr(), name
    for name, p in mod.named_parameters():
        ref_g = leaves[name].grad
        assert p.grad is not None and ref_g is not None, name
        err = ((p.grad.cpu().double() - ref_g.double()).norm() / ref_g.double().norm()).item()
        print(f'MHD scalar gradients: {name:36s} rel err {err:.2e} (bound 1e-3)')
        assert err < 1e-3, (name, err)


def test_model_loader_renders_mhd_frames_and_shares_uploads(tmp_path):
    from sunerf.evaluation.loader import ModelLoader, linear_plate_scale_axes
    from sunerf_hip.rays import grid_rays, pose_spherical
    root, reader, frames = _simulation(tmp_path)
    mod, _, _, _ = _renderer(root, reader)
    grid = {'shape': (12, 12), 'cdelt': (250., 250.), 'meta': {'t_obs': '2022-01-01T00:00:00.000'}}
    loader = ModelLoader(rendering=mod, model=mod.fine_model, ref_map=grid)
    wl = np.array([171, 193, 211])
    out = loader.render_observer_image(lat=0.1, lon=0.3, time=0.3, wl=wl)
    assert out['image'].shape == (12, 12, 3) and np.isfinite(out['image']).all() and out['image'].max() > 0
    assert out['height_map'].shape == (12, 12) and np.isfinite(out['height_map']).all()
    cache = mod.coarse_model.frame_cache('cuda')
    assert cache is mod.fine_model.frame_cache('cuda')
    assert (cache.uploads, sorted(cache.resident)) == (2, [10, 11]) and cache.hits >= 2      # one upload per frame
    assert reader.calls == 4                                                                   # rho and t of two frames
    # the same rays in one shot
    tx, ty = linear_plate_scale_axes(grid, None, 'cuda')
    o, d, t = grid_rays(tx, ty, pose_spherical(-0.3, 0.1, 215.03215567054764), time=0.3)
    with torch.no_grad():
        one = mod(o, d, t, torch.tensor(wl, dtype=torch.float32, device='cuda')[None].expand(o.shape[0], -1).contiguous())
    for k in ('image', 'coarse_image', 'height_map', 'absorption_map'):
        assert np.array_equal(out[k].reshape(-1), one[k].cpu().numpy().reshape(-1)), k
    assert cache.uploads == 2
    # point queries through the loader (loader.py:119-134)
    pts = _points(300, 6, (0.3, 0.5)).numpy().reshape(20, 15, 4)
    got = loader.load_coords(pts, batch_size=128)
    assert got.shape == (20, 15, 2)
    _check_field(torch.from_numpy(got.reshape(-1, 2)), ref.mhd_field(torch.from_numpy(pts.reshape(-1, 4)), frames, FFIRST, FLAST),
                 'load_coords')
    assert cache.uploads == 2


def test_batch_spanning_two_frame_pairs_matches_separate_renders(tmp_path):
    root, reader, _ = _simulation(tmp_path)
    mod, _, _, _ = _renderer(root, reader)
    o, d = _rays(64, 7)
    t = torch.where(torch.arange(64)[:, None] % 2 == 0, torch.tensor(0.3), torch.tensor(0.8)).float()   # pairs (10,11), (11,12)
    wl = torch.tensor(WAVELENGTHS, dtype=torch.float32).expand(64, 7).contiguous()
    o, d, t, wl = o.cuda(), d.cuda(), t.cuda(), wl.cuda()
    with torch.no_grad():
        both = mod(o, d, t, wl)
        assert sorted(mod.fine_model.frame_cache('cuda').resident) == [10, 11, 12]
        for parity in (0, 1):
            sel = torch.arange(parity, 64, 2, device='cuda')
            alone = mod(o[sel], d[sel], t[sel], wl[sel])
            for k, v in alone.items():
                a, b = both[k][sel].double(), v.double()
                assert torch.equal(torch.isnan(a), torch.isnan(b)), k
                scale = b.abs().max().clamp_min(1e-30)
                assert ((a - b).abs().nan_to_num() <= 1e-6 * scale).all(), (k, ((a - b).abs().nan_to_num().max() / scale).item())


def test_points_on_a_psi_clustered_r_grid(tmp_path):
    """Points mode on PSI's kind of r grid (1 ... 30 solar radii clustered at 1, 301 nodes): the bucket table is capped at
    MHD_MAX_BUCKETS and its first buckets hold several nodes, which the kernel's walk crosses."""
    from sunerf.model.mhd_model import MHDModel
    from sunerf_hip import ops
    frames = {10: ref.psi_clustered_frame(1), 11: ref.psi_clustered_frame(2)}
    r = frames[10][0]
    assert (r[-1] - r[0]) / np.diff(r).min() > ops.MHD_MAX_BUCKETS
    root = ref.write_placeholders(tmp_path / 'run', sorted(frames))
    model = MHDModel(root, reader=ref.DictReader(frames))
    gen = torch.Generator().manual_seed(9)
    n = 8000
    d = torch.randn(n, 3, generator=gen)
    d = d / d.norm(dim=1, keepdim=True)
    u = torch.rand(n, 1, generator=gen)
    # radii kept a few fp32 ulps off the bounds r = 1 and 30: the device's sqrtf and torch's sqrt may round |x| to either
    # side of a bound there, and scipy's inclusive bounds then fill one and interpolate the other
    rad = torch.where(u < 0.15, 0.97 + 0.029 * u / 0.15,                        # inside the inner bound
                      torch.where(u > 0.92, 30.001 + (u - 0.92) * 20.,          # beyond the outer bound
                                  1. + 2e-6 + 28.999 * ((u - 0.15) / 0.77) ** 4))   # clustered at 1 like the grid
    t = torch.tensor([0.0, 0.4, 1.0])[torch.randint(3, (n,), generator=gen)]
    pts = torch.cat([d * rad, t[:, None]], 1).float()
    got = model(pts.cuda())['inferences']
    want = ref.mhd_field(pts, frames, 10, 11)
    near = (rad[:, 0] > 1.) & (rad[:, 0] < 1.01)
    assert near.sum() > 500
    _check_field(got, want, 'clustered r grid')
