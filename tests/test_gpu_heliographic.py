"""Heliographic maps and radial profiles on MI355X: the column geometry kernel against its fp64 restatement, the
emission map against the fp64 oracle, the column statistics against the fp64 formulas of the reference's stash scripts, the
DT renderings (NeRF_DT, SimpleStar, MHDModel) against the oracle's DT integral, the loader API, and the map sharded over two
ranks.  Bit-for-bit comparisons run under an explicit SUNERF_FORWARD_PRECISION."""
import datetime
import math
import os
import sys

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (os.path.join(ROOT, '2024-hl-spi3s-sunerf_amd'), os.path.join(ROOT, 'oracle'), os.path.join(ROOT, 'tests')):
    if _p not in sys.path:          # (also when a spawned rank imports this module for its worker)
        sys.path.insert(0, _p)

import sunerf_oracle as orc  # noqa: E402
from conftest import GOLDEN, gate_units, load_golden  # noqa: E402

pytestmark = pytest.mark.gpu


def _axes(n_lat, n_lon, device='cuda'):
    lat = torch.linspace(-math.pi / 2, math.pi / 2, n_lat, dtype=torch.float64, device=device)
    lon = torch.linspace(-math.pi, math.pi, n_lon, dtype=torch.float64, device=device)
    return lat, lon


def _within_one_ulp(got, ref64, what):
    got = got.cpu()
    ref32 = ref64.float()
    ulp = torch.nextafter(ref32.abs(), torch.tensor(float('inf'))) - ref32.abs()
    err = (got - ref32).abs()
    assert bool((err <= ulp).all()), (what, (err / ulp).max().item())


def _emission(d_filter=64, Rs_per_ds=1.0, seed=3):
    from sunerf.rendering.emission import EmissionRadiativeTransfer
    torch.manual_seed(seed)
    return EmissionRadiativeTransfer(Rs_per_ds=Rs_per_ds, sampling_config={'type': 'stratified', 'n_samples': 32, 'perturb': False},
                                     hierarchical_sampling_config={'type': 'hierarchical', 'n_samples': 32},
                                     model_config={'d_filter': d_filter}).cuda()


# ---- geometry ---------------------------------------------------------------------------------------------------------------
def test_column_rays_match_host_restatement():
    from sunerf_hip.maps import column_directions, column_rays, grid_columns
    lat, lon = _axes(19, 31)
    plat, plon = grid_columns(lat.cpu(), lon.cpu())
    ref = column_directions(plat, plon)
    o, d, t = column_rays(lat, lon, time=0.75)
    assert o.shape == d.shape == (19 * 31, 3) and t.shape == (19 * 31, 1)
    assert (o == 0).all() and (t == 0.75).all()
    _within_one_ulp(d, ref, 'grid')
    o2, d2 = column_rays(lat, lon, col_begin=17, n_cols=101)                # a tile at an odd offset
    assert torch.equal(d2, d[17:118]) and (o2 == 0).all()
    gen = torch.Generator().manual_seed(2)
    alat = ((torch.rand(257, generator=gen, dtype=torch.float64) - 0.5) * math.pi).cuda()
    alon = ((torch.rand(257, generator=gen, dtype=torch.float64) - 0.5) * 2 * math.pi).cuda()
    _, dc = column_rays(alat, alon, grid=False)
    _within_one_ulp(dc, column_directions(alat.cpu(), alon.cpu()), 'per column')
    _, dc2 = column_rays(alat, alon, grid=False, col_begin=33, n_cols=99)
    assert torch.equal(dc2, dc[33:132])
    with pytest.raises(ValueError):
        column_rays(lat, lon, col_begin=500, n_cols=100)


def test_column_lies_below_the_observer():
    """The centre pixel of an odd-resolution frame seen from pose_spherical(-lon, lat, 215) looks along -u(lat, lon)."""
    from sunerf_hip.maps import column_directions
    from sunerf_hip.rays import fov_axis, grid_rays, pose_spherical
    for b, l in ((0.3, -1.2), (-0.9, 2.5), (0.0, 0.0), (1.2, 3.0)):
        axis = fov_axis(9, 0.01, 'cuda')
        o, d = grid_rays(axis, axis, pose_spherical(-l, b, 215.))
        u = column_directions(torch.tensor(b), torch.tensor(l))
        centre = d[4 * 9 + 4].cpu().double()
        assert (centre / centre.norm() + u).abs().max().item() < 1e-6, (b, l)
        assert (o[0].cpu().double() / 215. - u).abs().max().item() < 1e-6


# ---- emission map -----------------------------------------------------------------------------------------------------------
_ORACLE = {}


def _f64_stats(raw, z, rays_d):
    """The stash scripts' column statistics in fp64 on a given raw (N, S, 2)."""
    raw, z, d = raw.double(), z.double(), rays_d.double()
    dnorm = d.norm(dim=-1, keepdim=True)
    dz = z[:, 1:] - z[:, :-1]
    dr = torch.cat([dz[:, :1], dz], 1) * dnorm
    e = torch.exp(raw[..., 0])
    r = z * dnorm
    return {'emission_height': (r * e).sum(1) / e.sum(1), 'emission_column': (e * dr).sum(1), 'emission': e,
            'absorption': 1 - torch.exp(-torch.relu(raw[..., 1]) * dr)}


@pytest.mark.parametrize('d_filter', [64, 256])
def test_emission_map_matches_fp64_oracle(d_filter, precision):
    from sunerf_hip import ops
    from sunerf_hip.maps import column_rays, radial_row, render_columns
    rendering = _emission(d_filter)
    lat, lon = _axes(37, 53)
    S = 96
    m = render_columns(rendering, lat, lon, 0.3, (1.0, 1.3), S, profiles=True)
    assert m['image'].shape == (37, 53, 1) and m['height_map'].shape == (37, 53)
    assert m['emission'].shape == m['absorption'].shape == (37, 53, S)
    o, d, t = column_rays(lat, lon, time=0.3)
    z = radial_row((1.0, 1.3), S, 1.0).cuda()[None].expand(o.shape[0], -1).contiguous()
    if d_filter not in _ORACLE:
        sd = {k: v.cpu() for k, v in rendering.state_dict().items()}
        _ORACLE[d_filter] = orc.render_pass_f64(orc.params_from_state_dict(sd, 'fine_model.'), o.cpu(), d.cpu(), t.cpu(), z.cpu())
    want = _ORACLE[d_filter]
    units = {k: gate_units(m[k].reshape(-1), want[k].reshape(-1), floor=S * 6e-8 if k == 'absorption_map' else 0.0)
             for k in ('image', 'height_map', 'absorption_map')}
    print(f'd_filter {d_filter} {precision}: gate units', {k: round(v, 3) for k, v in units.items()})
    assert all(v <= 1.0 for v in units.values()), units
    # the statistics kernel against the scripts' formulas in fp64 on the kernel's own raw: fp32 sums of 96 terms
    raw = ops.emission_render_fwd(rendering.fine_model.packed(), o, d, t, z, 1.2, want_raw=True)['raw']
    mine = _f64_stats(raw.cpu(), z.cpu(), d.cpu())
    for k, tol in (('emission_height', 2e-6), ('emission_column', 2e-6), ('emission', 2e-6)):
        err = ((m[k].cpu().double().reshape(mine[k].shape) - mine[k]).abs() / mine[k].abs()).max().item()
        assert err < tol, (k, err)
    err = (m['absorption'].cpu().double().reshape(-1, S) - mine['absorption']).abs().max().item()
    assert err < 1e-6, ('absorption', err)
    # ... and on the fp64 oracle's raw: the statistics of the whole path
    full = _f64_stats(want['raw'], z.cpu(), d.cpu())
    # bounds |got - ref| <= rel |ref| + floor (floor: absorption ~ relu(raw1) dr vanishes where raw1 crosses zero)
    bounds = {'emission_height': (1e-5, 0.0), 'emission_column': (5e-5, 0.0), 'emission': (1e-4, 0.0), 'absorption': (1e-4, 1e-6)}
    units = {}
    for k, (rel, floor) in bounds.items():
        got = m[k].cpu().double().reshape(full[k].shape)
        units[k] = ((got - full[k]).abs() / (rel * full[k].abs() + floor)).max().item()
    print(f'd_filter {d_filter} {precision}: statistics against the fp64 oracle (units of their bounds)',
          {k: round(v, 3) for k, v in units.items()})
    assert all(v <= 1.0 for v in units.values()), units


@pytest.mark.parametrize('mode', ['fast', 'exact'])
def test_driver_adds_nothing(mode, monkeypatch):
    monkeypatch.setenv('SUNERF_FORWARD_PRECISION', mode)
    from sunerf.rendering.functional import emission_pass
    from sunerf_hip.maps import column_rays, radial_row, render_columns
    rendering = _emission(64)
    lat, lon = _axes(37, 53)
    one = render_columns(rendering, lat, lon, 0.2, n_samples=80, profiles=True)
    tiled = render_columns(rendering, lat, lon, 0.2, n_samples=80, profiles=True, tile_rays=1000)
    assert set(one) == set(tiled) == {'image', 'height_map', 'absorption_map', 'emission_height', 'emission_column',
                                       'emission', 'absorption'}
    for k in one:
        assert torch.equal(one[k], tiled[k]), k
    o, d, t = column_rays(lat, lon, col_begin=600, n_cols=1, time=0.2)
    z = radial_row((1.0, 1.3), 80, 1.0).cuda()[None]
    with torch.no_grad():
        ref = emission_pass(rendering.fine_model, o, d, t, z, 1.2, want_epilogues=True)
    for k in ('image', 'height_map', 'absorption_map'):
        assert torch.equal(one[k].reshape(37 * 53, -1)[600], ref[k].reshape(1, -1)[0]), k
    keep = render_columns(rendering, lat, lon, 0.2, n_samples=80, keys=('image',))
    assert set(keep) == {'image'} and torch.equal(keep['image'], one['image'])


# ---- density-temperature renderings -----------------------------------------------------------------------------------------
WL3 = (171., 193., 211.)


def test_nerf_dt_map_matches_oracle():
    from sunerf.model.model import NeRF_DT
    from sunerf.rendering.density_temperature import DensityTemperatureRadiativeTransfer
    from sunerf_hip.maps import column_rays, radial_row, render_columns
    g = load_golden('g6_dt_e2e')
    mod = DensityTemperatureRadiativeTransfer(
        Rs_per_ds=1.0, sampling_config={'type': 'stratified', 'n_samples': 16, 'perturb': False},
        hierarchical_sampling_config={'type': 'hierarchical', 'n_samples': 16}, model_config={'d_filter': 64}, model=NeRF_DT,
        pixel_intensity_factor=float(g['pixel_intensity_factor']), response_table=(g['aia_logte'].numpy(), g['aia_tresp'].numpy()))
    mod.load_state_dict({k[4:].replace('__', '.'): v for k, v in g.items() if k.startswith('sd__')}, strict=True)
    mod = mod.cuda()
    lat, lon = _axes(11, 17)
    S = 64
    m = render_columns(mod, lat, lon, 0.4, (1.0, 1.3), S, wavelengths=torch.tensor(WL3), profiles=True)
    assert m['image'].shape == (11, 17, 3) and m['inferences'].shape == (11, 17, S, 2)
    o, d, t = column_rays(lat, lon, time=0.4)
    n = o.shape[0]
    z = radial_row((1.0, 1.3), S, 1.0)[None].expand(n, -1).contiguous()
    sd = {k: v.cpu() for k, v in mod.state_dict().items()}
    la = {str(w): sd[f'fine_model.log_absortpion.{w}'] for w in (94, 131, 171, 193, 211, 304, 335)}
    fine = mod.fine_model
    want = orc.render_pass_dt(orc.params_from_state_dict(sd, 'fine_model.'), la, sd['fine_model.volumetric_constant'], o.cpu(),
                              d.cpu(), t.cpu(), z, torch.tensor(WL3).expand(n, 3), mod.response_logte.cpu(),
                              mod.response_table.cpu(), mod.pixel_intensity_factor, fine.base_log_density,
                              fine.base_log_temperature)
    u = gate_units(m['image'].reshape(n, 3), want['image'])
    dist_pts = want['points'].pow(2).sum(-1).sqrt()
    uh = gate_units(m['height_map'].reshape(-1), (want['weights'] * dist_pts).sum(-1))
    print(f'NeRF_DT map: image {u:.3f}, height_map {uh:.3f} gate units')
    assert u <= 1.0 and uh <= 1.0
    err = (m['inferences'].reshape(n, S, 2).cpu() - want['inferences']).abs().max().item()
    assert err < 1e-4 * want['inferences'].abs().max().item(), err


def test_simple_star_map_behind_model_loader():
    from sunerf.evaluation.loader import ModelLoader
    from sunerf.model.stellar_model import SimpleStar
    from sunerf.rendering.density_temperature import DensityTemperatureRadiativeTransfer
    from sunerf_hip.maps import column_rays, radial_row
    g = load_golden('g9_simple_star')
    mod = DensityTemperatureRadiativeTransfer(
        Rs_per_ds=1, model=SimpleStar, model_config={}, sampling_config={'type': 'stratified', 'n_samples': 16, 'perturb': False},
        hierarchical_sampling_config={'type': 'hierarchical', 'n_samples': 16},
        pixel_intensity_factor=float(g['pixel_intensity_factor']), response_table=(g['aia_logte'].numpy(), g['aia_tresp'].numpy()))
    loader = ModelLoader(rendering=mod, model=mod.fine_model, ref_map={'meta': {'t_obs': '2022-01-01T00:00:00.000'}})
    S = 48
    out = loader.render_heliographic_map(0.0, shape=(9, 13), n_samples=S, wl=np.array(WL3), profiles=True)
    assert out['image'].shape == (9, 13, 3) and isinstance(out['image'], np.ndarray)
    assert out['inferences'].shape == (9, 13, S, 2)
    lat = torch.from_numpy(np.linspace(-np.pi / 2, np.pi / 2, 9)).cuda()
    lon = torch.from_numpy(np.linspace(-np.pi, np.pi, 13)).cuda()
    o, d = column_rays(lat, lon)
    n = o.shape[0]
    z = radial_row((1.0, 1.3), S, 1.0)[None].expand(n, -1).contiguous()
    star = mod.fine_model
    inf = orc.simple_star_field(orc.points_on_rays(o.cpu(), d.cpu(), z).reshape(-1, 3),
                                *(star.stellar_parameters[k].detach().cpu() for k in ('rho_0', 'h0', 'T0', 'Rs'))).reshape(n, S, 2)
    la = {str(w): star.log_absortpion[str(w)].detach().cpu() for w in (94, 131, 171, 193, 211, 304, 335)}
    want = orc.dt_integral(inf, la, star.volumetric_constant.detach().cpu(), z, torch.tensor(WL3).expand(n, 3),
                           mod.response_logte.cpu(), mod.response_table.cpu(), mod.pixel_intensity_factor)
    u = gate_units(torch.from_numpy(out['image']).reshape(n, 3), want['image'])
    print(f'SimpleStar map: image {u:.3f} gate units')
    assert u <= 1.0
    err = np.abs(out['inferences'].reshape(n, S, 2) - inf.numpy()).max()
    assert err < 1e-5 * np.abs(inf.numpy()).max(), err


def test_mhd_map_equals_dt_integral_of_the_sampled_cube(tmp_path):
    import mhd_reference as ref
    from sunerf.model.mhd_model import MHDModel
    from sunerf.rendering.density_temperature import DensityTemperatureRadiativeTransfer
    from sunerf_hip.maps import column_rays, radial_row, render_columns
    frames = {10: ref.synthetic_frame(1), 11: ref.synthetic_frame(2), 12: ref.synthetic_frame(3)}
    root = ref.write_placeholders(tmp_path / 'run', sorted(frames))
    g = load_golden('g9_simple_star')
    mod = DensityTemperatureRadiativeTransfer(
        Rs_per_ds=1, model=MHDModel, model_config={'data_path': root, 'reader': ref.DictReader(frames)},
        sampling_config={'type': 'stratified', 'n_samples': 16, 'perturb': False},
        hierarchical_sampling_config={'type': 'hierarchical', 'n_samples': 16},
        pixel_intensity_factor=float(g['pixel_intensity_factor']),
        response_table=(g['aia_logte'].numpy(), g['aia_tresp'].numpy())).cuda()
    with torch.no_grad():
        for w, v in zip((94, 131, 171, 193, 211, 304, 335), (2e-9, 3e-9, 4e-9, 5e-9, 6e-9, 7e-9, 8e-9)):
            mod.fine_model.log_absortpion[str(w)].fill_(v)
        mod.fine_model.volumetric_constant.fill_(0.8)
    lat, lon = _axes(13, 19)
    S = 40
    m = render_columns(mod, lat, lon, 0.3, (1.0, 1.35), S, wavelengths=torch.tensor(WL3))
    o, d, t = column_rays(lat, lon, time=0.3)
    n = o.shape[0]
    z = radial_row((1.0, 1.35), S, 1.0).cuda()[None].expand(n, -1).contiguous()
    pts = torch.cat([orc.points_on_rays(o.cpu(), d.cpu(), z.cpu()), torch.full((n, S, 1), 0.3)], -1).reshape(-1, 4)
    with torch.no_grad():
        inf = mod.fine_model(pts.cuda())['inferences'].cpu().reshape(n, S, 2)
    fm = mod.fine_model
    la = {str(w): fm.log_absortpion[str(w)].detach().cpu() for w in (94, 131, 171, 193, 211, 304, 335)}
    want = orc.dt_integral(inf, la, fm.volumetric_constant.detach().cpu(), z.cpu(), torch.tensor(WL3).expand(n, 3),
                           mod.response_logte.cpu(), mod.response_table.cpu(), mod.pixel_intensity_factor)
    assert bool((want['image'] > 0).any())
    u = gate_units(m['image'].reshape(n, 3), want['image'])
    print(f'MHD map: image {u:.3f} gate units')
    assert u <= 1.0


# ---- loader -----------------------------------------------------------------------------------------------------------------
def test_loader_maps_and_profiles(tmp_path, monkeypatch):
    monkeypatch.setenv('SUNERF_FORWARD_PRECISION', 'exact')
    from sunerf.evaluation.loader import SuNeRFLoader
    from sunerf.model.sunerf import save_state
    from sunerf.rendering.functional import emission_pass
    from sunerf_hip.maps import column_rays, radial_row, render_columns

    class _Module:
        pass

    def data(Rs_per_ds):
        class _Data:
            config = {'wavelength': 193, 'times': [datetime.datetime(2022, 1, 1), datetime.datetime(2022, 1, 3)],
                      'resolution': (16, 16), 'wcs': {'shape': (16, 16), 'cdelt': (150., 150.)}}
            seconds_per_dt, ref_time = 86400., datetime.datetime(2022, 1, 1)
        _Data.Rs_per_ds = Rs_per_ds
        return _Data()
    mod = _Module()
    mod.rendering = _emission(64)
    path = str(tmp_path / 'a' / 'save_state.snf')
    save_state(mod, data(1.0), path)
    loader = SuNeRFLoader(path, device='cuda')
    when = datetime.datetime(2022, 1, 2, 12)
    out = loader.render_heliographic_map(when, shape=(7, 11), n_samples=64)
    assert out['image'].shape == (7, 11, 1) and isinstance(out['image'], np.ndarray)
    assert np.isfinite(out['image']).all() and out['image'].max() > 0
    lat = torch.from_numpy(np.linspace(-np.pi / 2, np.pi / 2, 7)).cuda()
    lon = torch.from_numpy(np.linspace(-np.pi, np.pi, 11)).cuda()
    direct = render_columns(loader.rendering, lat, lon, 1.5, n_samples=64)          # time normalised: 1.5 days
    for k, v in direct.items():
        assert np.array_equal(out[k], v.cpu().numpy()), k
    prof = loader.render_radial_profile(np.linspace(-0.6, -0.1, 23), np.full(23, 2.0), when, n_samples=50)
    assert prof['emission'].shape == prof['absorption'].shape == (23, 50) and prof['emission_height'].shape == (23,)
    assert ((prof['emission_height'] >= 1.0 - 1e-6) & (prof['emission_height'] <= 1.3 + 1e-6)).all()
    # Rs_per_ds = 2: the columns sample z = r / 2, heights come back in solar radii
    mod.rendering = _emission(64, Rs_per_ds=2.0)
    path2 = str(tmp_path / 'b' / 'save_state.snf')
    save_state(mod, data(2.0), path2)
    loader2 = SuNeRFLoader(path2, device='cuda')
    m2 = loader2.render_heliographic_map(when, shape=(7, 11), n_samples=64, as_numpy=False)
    eh = m2['emission_height']
    assert bool(((eh >= 1.0 - 1e-6) & (eh <= 1.3 + 1e-6)).all()), (eh.min().item(), eh.max().item())
    o, d, t = column_rays(lat, lon, time=1.5)
    z = radial_row((1.0, 1.3), 64, 2.0).cuda()[None].expand(o.shape[0], -1).contiguous()
    assert z[0, -1].item() == pytest.approx(0.65)
    with torch.no_grad():
        ref = emission_pass(loader2.rendering.fine_model, o, d, t, z, 0.6, want_epilogues=True)
    assert torch.equal(m2['height_map'].reshape(-1), ref['height_map'] * 2)
    assert torch.equal(m2['image'].reshape(-1), ref['image'].reshape(-1))
    # the reference-written state file renders a map
    g10 = SuNeRFLoader(os.path.join(GOLDEN, 'g10_reference_state.snf'), device='cuda')
    frame = g10.render_heliographic_map(datetime.datetime(2022, 3, 2), shape=(5, 8), n_samples=32)
    assert frame['image'].shape == (5, 8, 1) and np.isfinite(frame['image']).all()
    assert np.isfinite(frame['emission_height']).all()


def test_thomson_rendering_is_refused():
    from sunerf.rendering.thompson import ThompsonScattering
    from sunerf_hip.maps import render_columns
    th = ThompsonScattering(Rs_per_ds=1.0, sampling_config={'type': 'stratified', 'n_samples': 8, 'perturb': False},
                            hierarchical_sampling_config={'type': 'hierarchical', 'n_samples': 8},
                            model_config={'d_filter': 64}).cuda()
    lat, lon = _axes(3, 4)
    with pytest.raises(ValueError, match='ThompsonScattering'):
        render_columns(th, lat, lon, 0.0)


# ---- sharding ---------------------------------------------------------------------------------------------------------------
def _shard_worker(rank, world, port, out_dir):
    os.environ.update(MASTER_ADDR='127.0.0.1', MASTER_PORT=str(port))
    torch.cuda.set_device(0)
    dist.init_process_group('gloo', rank=rank, world_size=world)
    from sunerf_hip.maps import render_columns
    lat, lon = _axes(11, 13)
    m = render_columns(_emission(64), lat, lon, 0.6, n_samples=48, profiles=True)
    torch.save({k: v.cpu() for k, v in m.items()}, os.path.join(out_dir, f'rank{rank}.pt'))
    dist.destroy_process_group()


def test_two_rank_map_equals_single_process(tmp_path, monkeypatch):
    monkeypatch.setenv('SUNERF_FORWARD_PRECISION', 'exact')       # inherited by the spawned ranks
    from sunerf_hip.maps import render_columns
    mp.spawn(_shard_worker, args=(2, 29563, str(tmp_path)), nprocs=2, join=True)
    lat, lon = _axes(11, 13)
    one = render_columns(_emission(64), lat, lon, 0.6, n_samples=48, profiles=True)
    for rank in (0, 1):
        got = torch.load(tmp_path / f'rank{rank}.pt')
        assert set(got) == set(one)
        for k, v in one.items():
            assert torch.equal(got[k], v.cpu()), (rank, k)
