"""3-D volumes on MI355X: the grid-point kernel against its host fp64 restatement bit for bit, the physical
quantities against the fp64 formulas, sample_volume against the model's own forward (nothing added to the field), tiles, times,
masks and two ranks, volume_metrics against numpy fp64 sums, and the loader API.  Bit-for-bit comparisons of the field run
under an explicit SUNERF_FORWARD_PRECISION."""
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

import volume_reference as vref  # noqa: E402
from conftest import GOLDEN, load_golden  # noqa: E402

pytestmark = pytest.mark.gpu

REL = 4e-6          # fp32 rounding of the stated formulas: 5.2e-7 in a CPU fp32 emulation, x 8 for a device exp two ulps off
WL3 = (171., 193., 211.)


def _bits(t):
    return t.detach().contiguous().view(torch.int32)


def _same_bits(a, b):
    return a.shape == b.shape and torch.equal(_bits(a), _bits(b))


def _emission(d_filter=64, Rs_per_ds=1.0, seed=3):
    from sunerf.rendering.emission import EmissionRadiativeTransfer
    torch.manual_seed(seed)
    return EmissionRadiativeTransfer(Rs_per_ds=Rs_per_ds, sampling_config={'type': 'stratified', 'n_samples': 32, 'perturb': False},
                                     hierarchical_sampling_config={'type': 'hierarchical', 'n_samples': 32},
                                     model_config={'d_filter': d_filter}).cuda()


# ---- grid points ------------------------------------------------------------------------------------------------------------
def _check_points(grid, Rs_per_ds, time, what):
    from sunerf_hip.volume import grid_points
    pts, rad = grid_points(grid, Rs_per_ds, time)
    n = grid.n_voxels
    assert pts.shape == (n, 4) and pts.dtype == torch.float32 and rad.shape == (n,) and rad.dtype == torch.float32
    want = grid.points_f64(Rs_per_ds).float().reshape(n, 3)
    want_r = grid.radius_f64().float().reshape(n)
    assert torch.equal(pts[:, :3].cpu(), want), (what, (pts[:, :3].cpu() - want).abs().max().item())
    assert torch.equal(rad.cpu(), want_r), (what, (rad.cpu() - want_r).abs().max().item())
    assert bool((pts[:, 3] == torch.tensor(time, dtype=torch.float32).item()).all()), what
    return pts, rad


def test_grid_points_are_the_host_restatement_bit_for_bit():
    from sunerf_hip.volume import CartesianGrid, Plane, SphericalGrid, grid_points
    gen = np.random.default_rng(8)
    basis = np.array([[0.9, 0.2, -0.1], [0.15, 1.1, 0.3], [-0.25, 0.05, 0.8]])
    box = CartesianGrid(np.linspace(-1.3, 1.3, 13), np.sort(gen.uniform(-1.5, 1.5, 11)), np.linspace(-1.1, 1.4, 17),
                        origin=(0.05, -0.1, 0.02), basis=basis)
    pts, rad = _check_points(box, 1.7, 0.375, 'oblique box')
    _check_points(CartesianGrid.cube(1.3, 16), 1.0, 0.1, 'cube')
    _check_points(Plane((0.1, 0.2, -0.3), (0.6, 0.8, 0.), (0., -0.6, 0.8), np.linspace(-1.5, 1.5, 33), np.linspace(-1.2, 1.2, 21)),
                  0.8, 0.7, 'plane')
    shell = SphericalGrid(np.linspace(-np.pi / 2, np.pi / 2, 19), np.linspace(-np.pi, np.pi, 37), np.linspace(1.0, 1.3, 11))
    assert shell.axes[0][0] == -np.pi / 2 and shell.axes[0][-1] == np.pi / 2 and shell.axes[2][0] == 1.0
    assert shell.axes[1][0] == -np.pi and shell.axes[1][-1] == np.pi
    spts, srad = _check_points(shell, 0.9, 0.25, 'spherical shell')
    assert bool((srad.view(19, 37, 11)[:, :, 0] == 1.0).all())           # the axis value itself: no sqrt taken
    _check_points(CartesianGrid([1.25], [-0.5], [0.75], origin=(0.1, 0.1, 0.1), basis=basis), 1.3, 0.5, 'single voxel')
    _check_points(SphericalGrid([0.3], [-1.0], [1.1]), 1.0, 0.0, 'single spherical voxel')
    # ranges that split rows
    for grid, whole, whole_r, scale, t in ((box, pts, rad, 1.7, 0.375), (shell, spts, srad, 0.9, 0.25)):
        for first, count in ((5, 1000), (17 * 11 + 3, 2 * 17 + 1), (grid.n_voxels - 7, 7), (0, 1), (123, 0)):
            p, r = grid_points(grid, scale, t, first, count)
            assert p.shape == (count, 4) and torch.equal(p, whole[first:first + count]), (first, count)
            assert torch.equal(r, whole_r[first:first + count]), (first, count)
    with pytest.raises(ValueError):
        grid_points(box, 1.7, 0.0, first=box.n_voxels - 3, count=4)


# ---- field quantities -------------------------------------------------------------------------------------------------------
def _relative(got, want):
    """max |got - want| / |want| over the finite, non-zero reference values; zeros and infinities must be met exactly."""
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    assert got.shape == want.shape, (got.shape, want.shape)
    nan = np.isnan(want)
    assert np.array_equal(np.isnan(got), nan)
    over = ~nan & (np.abs(want) > np.finfo(np.float32).max)              # fp32 overflow to inf is kept
    assert np.array_equal(got[over], np.sign(want[over]) * np.inf)
    zero = ~nan & (want == 0)
    assert (got[zero] == 0).all()
    rest = ~nan & ~over & ~zero
    return float((np.abs(got[rest] - want[rest]) / np.abs(want[rest])).max()) if rest.any() else 0.0


def _radii(m, gen):
    rad = (0.9 + 0.5 * torch.rand(m, generator=gen)).float()
    rad[:4] = torch.tensor([1.0, 1.3, float('nan'), 0.0])
    rad[4] = float(np.nextafter(np.float32(1.0), np.float32(0.0)))
    rad[5] = float(np.nextafter(np.float32(1.3), np.float32(2.0)))
    return rad


def test_emission_and_white_light_quantities():
    from sunerf_hip.volume import LN10, field_quantities
    gen = torch.Generator().manual_seed(21)
    m = 200001
    raw = torch.stack([torch.rand(m, generator=gen) * 30 - 20, torch.rand(m, generator=gen) * 6 - 3], -1).float()
    raw[10, 0], raw[11, 0], raw[12, 1] = 100.0, -80.0, 0.0
    rad = _radii(m, gen)
    rad[10:13] = 1.1
    got = field_quantities(raw.cuda(), rad.cuda(), 'emission', r_range=(1.0, 1.3))
    want, mask = vref.field_quantities_f64('emission', raw.numpy(), rad.numpy(), 1.0, 1.3)
    assert set(got) == {'emission', 'absorption'} and mask[2] and mask[3] and mask[4] and mask[5] and not mask[0] and not mask[1]
    assert np.array_equal(np.isnan(got['emission'].cpu().numpy()), mask) and 0.1 < mask.mean() < 0.9       # the mask, exactly
    assert np.array_equal(got['absorption'].cpu().numpy(), want['absorption'].astype(np.float32), equal_nan=True)      # exact
    assert got['emission'][10].item() == math.inf
    err = _relative(got['emission'].cpu().numpy(), want['emission'])
    print(f'emission: max relative error {err:.2e} (bound {REL:.0e})')
    assert err <= REL
    # a finite fill, no outer mask, one quantity, and an unaligned slice (scalar accesses) against the aligned call
    one = field_quantities(raw.cuda(), rad.cuda(), 'emission', quantities=('emission',), r_range=(1.0, None), fill=-1.0)
    assert set(one) == {'emission'}
    inner = vref.outside(rad.numpy(), 1.0, np.inf)
    assert np.array_equal((one['emission'] == -1.0).cpu().numpy(), inner)
    keep = ~torch.from_numpy(mask).cuda()
    assert _same_bits(one['emission'][keep], got['emission'][keep])
    odd_raw, odd_rad = raw.cuda()[1:].contiguous(), rad.cuda()[1:]
    buf = torch.empty(m, device='cuda')
    sliced = field_quantities(odd_raw, odd_rad, 'emission', quantities=('emission',), r_range=(1.0, 1.3), out={'emission': buf[1:]})
    assert sliced['emission'].data_ptr() == buf[1:].data_ptr() and _same_bits(sliced['emission'], got['emission'][1:])
    # white light: exp(kappa raw0), kappa in fp32.  The fp32 product kappa * raw0 carries 2^-24 |kappa raw0| into the exponent,
    # on top of the rounding of exp itself
    raw1 = (torch.rand(m, 1, generator=gen) * 12 - 4).float()
    gw = field_quantities(raw1.cuda(), rad.cuda(), 'white_light', kappa=LN10)
    ww, wmask = vref.field_quantities_f64('white_light', raw1.numpy(), rad.numpy(), 1.0, np.inf, kappa=LN10)
    assert set(gw) == {'electron_density'} and np.array_equal(np.isnan(gw['electron_density'].cpu().numpy()), wmask)
    g, w = gw['electron_density'].cpu().numpy().astype(np.float64)[~wmask], ww['electron_density'][~wmask]
    bound = REL + 2.0 ** -24 * np.abs(np.float64(np.float32(LN10)) * raw1.numpy()[~wmask, 0].astype(np.float64))
    assert (np.abs(g - w) / w <= bound).all(), (np.abs(g - w) / w / bound).max()
    assert field_quantities(raw.cuda()[:0], rad.cuda()[:0], 'emission')['emission'].shape == (0,)


def test_density_temperature_quantities():
    from sunerf_hip.volume import field_quantities
    g = load_golden('g6_dt_e2e')
    logte, resp = g['aia_logte'].float(), (g['aia_tresp'] * 2.9).float()
    assert logte.shape == resp.shape == (7, 101)
    gen = torch.Generator().manual_seed(22)
    m = 300007
    inf0 = (torch.rand(m, generator=gen) * 27 - 2).float()
    logt = (torch.rand(m, generator=gen) * 3.7 + 3.9).float()
    lo, hi = logte[:, 0].min().item(), logte[:, -1].max().item()
    special = torch.cat([logte.reshape(-1),                                # every knot of every channel
                         torch.from_numpy(np.array([lo, hi, np.nextafter(np.float32(lo), np.float32(-1)),
                                                    np.nextafter(np.float32(hi), np.float32(99)),
                                                    np.nextafter(np.float32(lo), np.float32(99)),
                                                    np.nextafter(np.float32(hi), np.float32(-1)), -0.5, 0.0], np.float32))])
    logt[100:100 + special.shape[0]] = special
    inf0[10:18] = torch.tensor([40.0, 39.5, 0.0, -0.0, -1.0, 25.0, 30.0, 35.0])     # <= 40: density^2 stays finite
    inf = torch.stack([inf0, logt], -1)
    rad = _radii(m, gen)
    rad[6:200] = 1.15
    rad[100:100 + special.shape[0]] = 1.15
    log_abs = torch.tensor([2e-9, 3e-9, -4e-9, 5e-9, 6e-9, 7e-9, 8e-9])            # one negative: relu -> 0
    for wl in ((171., 193., 94., 500., 335., 211., 131.), WL3, (304.,)):
        got = field_quantities(inf.cuda(), rad.cuda(), 'dt', quantities=('density', 'log_temperature', 'emissivity', 'absorption'),
                               r_range=(1.0, 1.3), wavelengths=torch.tensor(wl), response_table=(logte, resp), log_abs=log_abs.cuda())
        want, mask = vref.field_quantities_f64('dt', inf.numpy(), rad.numpy(), 1.0, 1.3, wavelengths=wl, logte=logte.numpy(),
                                               resp=resp.numpy(), log_abs=log_abs.numpy())
        w = len(wl)
        assert got['emissivity'].shape == got['absorption'].shape == (m, w) and got['density'].shape == (m,)
        host = {k: v.cpu().numpy() for k, v in got.items()}
        for k in host:                                                     # the mask positions, exactly
            assert np.array_equal(np.isnan(host[k]), mask if host[k].ndim == 1 else np.repeat(mask[:, None], w, 1)), k
        assert np.array_equal(host['log_temperature'], want['log_temperature'].astype(np.float32), equal_nan=True)     # exact
        for c, wave in enumerate(wl):
            if wave == 500.:                                               # not an AIA channel: exactly 0
                assert (host['emissivity'][~mask, c] == 0).all() and (host['absorption'][~mask, c] == 0).all()
            if wave == 171.:                                               # log_abs < 0
                assert (host['absorption'][~mask, c] == 0).all()
        out_of_table = ~mask & ((logt.numpy() < lo) | (logt.numpy() > hi))
        assert out_of_table.sum() >= 3 and (host['emissivity'][out_of_table] == 0).all()
        errs = {k: _relative(host[k], want[k]) for k in ('density', 'emissivity', 'absorption')}
        print(f'{w} channels: max relative errors', {k: f'{v:.2e}' for k, v in errs.items()}, f'(bound {REL:.0e})')
        assert all(v <= REL for v in errs.values()), errs
        assert np.isfinite(host['emissivity'][~mask]).all() and (want['emissivity'][~mask] > 0).mean() > 0.5
    # density / temperature alone need neither channels nor tables; an unaligned slice gives the same bits
    plain = field_quantities(inf.cuda(), rad.cuda(), 'dt', r_range=(1.0, 1.3))
    assert set(plain) == {'density', 'log_temperature'} and _same_bits(plain['density'], got['density'])
    odd = field_quantities(inf.cuda()[1:].contiguous(), rad.cuda()[1:], 'dt', quantities=('emissivity', 'absorption', 'density'),
                           r_range=(1.0, 1.3), wavelengths=torch.tensor(WL3), response_table=(logte, resp), log_abs=log_abs.cuda(),
                           out={'emissivity': torch.empty(m, 3, device='cuda')[1:], 'density': torch.empty(m, device='cuda')[1:]})
    ref3 = field_quantities(inf.cuda(), rad.cuda(), 'dt', quantities=('emissivity', 'absorption', 'density'), r_range=(1.0, 1.3),
                            wavelengths=torch.tensor(WL3), response_table=(logte, resp), log_abs=log_abs.cuda())
    for k in ('emissivity', 'absorption', 'density'):
        assert _same_bits(odd[k], ref3[k][1:]), k


def test_absent_channel_is_zero_where_the_density_overflowed():
    """exp(100) is inf in fp32 and is kept; a wavelength that is no AIA channel still gives exactly 0, not inf * 0."""
    from sunerf_hip.volume import field_quantities
    g = load_golden('g6_dt_e2e')
    logte, resp = g['aia_logte'].float(), (g['aia_tresp'] * 2.9).float()
    inf = torch.tensor([[100.0, 6.0], [3.0, 6.0], [100.0, 6.0]]).cuda()
    rad = torch.tensor([1.1, 1.1, 0.5]).cuda()
    got = field_quantities(inf, rad, 'dt', quantities=('density', 'emissivity', 'absorption'), wavelengths=torch.tensor([500., 171.]),
                           response_table=(logte, resp), log_abs=torch.full((7,), 1e-9).cuda())
    assert got['density'][0].item() == math.inf
    for k in ('emissivity', 'absorption'):
        host = got[k].cpu().numpy()
        assert host[0, 0] == 0 and host[1, 0] == 0 and host[0, 1] == np.inf and 0 < host[1, 1] < np.inf, (k, host)
        assert np.isnan(host[2]).all(), (k, host)                          # inside the Sun: the fill, absent channel or not


# ---- sample_volume ----------------------------------------------------------------------------------------------------------
def _dt_rendering(model, model_config, g):
    from sunerf.rendering.density_temperature import DensityTemperatureRadiativeTransfer
    return DensityTemperatureRadiativeTransfer(
        Rs_per_ds=1.0, sampling_config={'type': 'stratified', 'n_samples': 16, 'perturb': False},
        hierarchical_sampling_config={'type': 'hierarchical', 'n_samples': 16}, model_config=model_config, model=model,
        pixel_intensity_factor=float(g['pixel_intensity_factor']), response_table=(g['aia_logte'].numpy(), g['aia_tresp'].numpy()))


def _field(name, tmp_path):
    """(rendering, wavelengths, quantity names, times)"""
    if name in ('nerf64', 'nerf256'):
        return _emission(int(name[4:]), Rs_per_ds=2.0 if name == 'nerf256' else 1.0), None, ('emission', 'absorption'), (0.3, 0.8)
    dt_names = ('density', 'log_temperature', 'emissivity')
    if name == 'nerf_dt':
        from sunerf.model.model import NeRF_DT
        g = load_golden('g6_dt_e2e')
        mod = _dt_rendering(NeRF_DT, {'d_filter': 64}, g)
        mod.load_state_dict({k[4:].replace('__', '.'): v for k, v in g.items() if k.startswith('sd__')}, strict=True)
        return mod.cuda(), WL3, dt_names, (0.4, 0.1)
    if name == 'simple_star':
        from sunerf.model.stellar_model import SimpleStar
        return _dt_rendering(SimpleStar, {}, load_golden('g9_simple_star')).cuda(), WL3, dt_names, (0.0, 0.5)
    import mhd_reference as ref                                            # an MHDModel built as in test_gpu_mhd.py
    from sunerf.model.mhd_model import MHDModel
    frames = {10: ref.synthetic_frame(1),
              11: ref.synthetic_frame(2, n_phi=19, n_theta=21, n_r=33, r_range=(1.03, 1.35), phi_end=0.93 * 2 * np.pi),
              12: ref.synthetic_frame(3)}
    root = ref.write_placeholders(tmp_path / 'run', sorted(frames))
    mod = _dt_rendering(MHDModel, {'data_path': root, 'reader': ref.DictReader(frames)}, load_golden('g9_simple_star')).cuda()
    return mod, WL3, dt_names, (0.3, 0.75)


@pytest.mark.parametrize('name', ['nerf64', 'nerf256', 'nerf_dt', 'simple_star', 'mhd'])
def test_sample_volume_adds_nothing_to_the_field(name, precision, tmp_path):
    from sunerf_hip.volume import CartesianGrid, SphericalGrid, grid_points, sample_volume
    rendering, wl, names, times = _field(name, tmp_path)
    net = rendering.fine_model
    scale = float(rendering.Rs_per_ds)
    basis = np.array([[1.0, 0.1, 0.0], [0.0, 0.9, 0.2], [0.1, 0.0, 1.1]])
    for grid in (CartesianGrid(np.linspace(-1.3, 1.3, 11), np.linspace(-1.3, 1.3, 9), np.linspace(-1.2, 1.4, 13), basis=basis),
                 SphericalGrid(np.linspace(-np.pi / 2, np.pi / 2, 7), np.linspace(-np.pi, np.pi, 12), np.linspace(0.95, 1.35, 17))):
        vol = sample_volume(rendering, grid, times[0], wavelengths=wl)
        assert set(names) <= set(vol) and vol['grid'] is grid and vol['times'] == times[0] and vol['Rs_per_ds'] == scale
        n = grid.n_voxels
        pts, rad = grid_points(grid, scale, times[0])
        with torch.no_grad():
            ref = net(pts)['inferences']
        assert vol['inferences'].shape == grid.shape + (2,) and vol['radius'].shape == grid.shape
        assert _same_bits(vol['inferences'].reshape(n, 2), ref), name       # the volume path adds no arithmetic to the field
        assert torch.equal(vol['radius'].reshape(n), rad)
        inside = (rad >= 1.0)
        assert 0.2 < inside.float().mean().item() < 1.0
        for q in names:
            assert vol[q].shape == grid.shape + ((3,) if q == 'emissivity' else ()), q
            flat = vol[q].reshape(n, -1)
            assert bool(torch.isnan(flat[~inside]).all()) and not bool(torch.isnan(flat[inside]).any()), q
        # tiles: odd sizes, so tiles start at odd voxels and split rows
        for tile in (101, 1000):
            tiled = sample_volume(rendering, grid, times[0], wavelengths=wl, tile_points=tile)
            for k in ('inferences', 'radius') + names:
                assert _same_bits(tiled[k], vol[k]), (name, tile, k)
        # a sequence of times: a leading axis on everything but the radius
        both = sample_volume(rendering, grid, list(times), wavelengths=wl, tile_points=777)
        assert both['times'] == list(times) and both['radius'].shape == grid.shape
        later = sample_volume(rendering, grid, times[1], wavelengths=wl)
        for k in ('inferences',) + names:
            assert both[k].shape == (2,) + vol[k].shape, k
            assert _same_bits(both[k][0], vol[k]) and _same_bits(both[k][1], later[k]), (name, k)
        assert not _same_bits(later['inferences'], vol['inferences']) or name == 'simple_star'      # (a static star)
        # r_range masks exactly the voxels the fp32 radius says; a finite fill marks them
        shell = sample_volume(rendering, grid, times[0], wavelengths=wl, r_range=(1.05, 1.25), fill=-7.0)
        masked = torch.from_numpy(vref.outside(rad.cpu().numpy(), 1.05, 1.25)).cuda()
        assert 0.1 < masked.float().mean().item() < 0.95
        for q in names:
            flat = shell[q].reshape(n, -1)
            assert bool((flat[masked] == -7.0).all()) and bool((flat[~masked] >= 0).all()), q
            assert _same_bits(flat[~masked], vol[q].reshape(n, -1)[~masked]), q
        assert _same_bits(shell['inferences'], vol['inferences'])          # the answer itself is never masked
    # the coarse model, one quantity, and a bare field module with kind=
    coarse = sample_volume(rendering, grid, times[0], wavelengths=None, quantities=(names[0],), model='coarse')
    with torch.no_grad():
        ref = rendering.coarse_model(pts)['inferences']
    assert _same_bits(coarse['inferences'].reshape(n, 2), ref) and set(coarse) & set(names) == {names[0]}
    bare = sample_volume(net, grid, times[0], quantities=(names[0],), kind='dt' if wl else 'emission', Rs_per_ds=scale)
    assert _same_bits(bare[names[0]], vol[names[0]])


def test_white_light_volume():
    from sunerf.rendering.thompson import ThompsonScattering
    from sunerf_hip.volume import LN10, CartesianGrid, grid_points, sample_volume
    torch.manual_seed(5)
    th = ThompsonScattering(Rs_per_ds=1.0, sampling_config={'type': 'stratified', 'n_samples': 8, 'perturb': False},
                            hierarchical_sampling_config={'type': 'hierarchical', 'n_samples': 8},
                            model_config={'d_filter': 64}).cuda()
    grid = CartesianGrid.cube(1.4, 9)
    vol = sample_volume(th, grid, 0.2)
    pts, rad = grid_points(grid, 1.0, 0.2)
    with torch.no_grad():
        ref = th.fine_model(pts)['inferences']
    c = ref.shape[-1]
    assert _same_bits(vol['inferences'].reshape(-1, c), ref)
    want, mask = vref.field_quantities_f64('white_light', ref.cpu().numpy(), rad.cpu().numpy(), kappa=LN10)
    got = vol['electron_density'].reshape(-1).cpu().numpy().astype(np.float64)
    assert np.array_equal(np.isnan(got), mask)
    bound = REL + 2.0 ** -24 * np.abs(LN10 * ref[:, 0].cpu().numpy().astype(np.float64))[~mask]
    assert (np.abs(got[~mask] - want['electron_density'][~mask]) / want['electron_density'][~mask] <= bound).all()


def _rank_volume():
    from sunerf_hip.volume import SphericalGrid, sample_volume
    grid = SphericalGrid(np.linspace(-1.4, 1.4, 7), np.linspace(-3.0, 3.0, 5), np.linspace(0.9, 1.3, 6))
    vol = sample_volume(_emission(64), grid, [0.6, 0.1], tile_points=37)
    return {k: v.cpu() for k, v in vol.items() if isinstance(v, torch.Tensor)}


def _shard_worker(rank, world, port, out_dir):
    os.environ.update(MASTER_ADDR='127.0.0.1', MASTER_PORT=str(port))
    torch.cuda.set_device(0)
    dist.init_process_group('gloo', rank=rank, world_size=world)
    torch.save(_rank_volume(), os.path.join(out_dir, f'rank{rank}.pt'))
    dist.destroy_process_group()


def test_two_rank_volume_equals_single_process(tmp_path, monkeypatch):
    monkeypatch.setenv('SUNERF_FORWARD_PRECISION', 'exact')       # inherited by the spawned ranks
    mp.spawn(_shard_worker, args=(2, 29571, str(tmp_path)), nprocs=2, join=True)
    one = _rank_volume()
    assert {'inferences', 'radius', 'emission', 'absorption'} <= set(one) and one['emission'].shape == (2, 7, 5, 6)
    for rank in (0, 1):
        got = torch.load(tmp_path / f'rank{rank}.pt')
        assert set(got) == set(one)
        for k, v in one.items():
            assert _same_bits(got[k], v), (rank, k)


# ---- volume metrics ---------------------------------------------------------------------------------------------------------
def _volumes(seed=31):
    rng = np.random.default_rng(seed)
    shape = (37, 29, 23)
    a = rng.normal(3.0, 2.0, shape).astype(np.float32)
    b = (0.8 * a + rng.normal(0.0, 1.0, shape)).astype(np.float32)
    for v, bad in ((a, np.nan), (b, np.inf), (a, -np.inf), (b, np.nan)):
        v[rng.random(shape) < 0.027] = bad                                 # about 10 % of the voxels lose one of the two
    return a, b


@pytest.mark.parametrize('weighting', ['unit', 'spherical'])
def test_volume_metrics_match_numpy_fp64(weighting):
    from sunerf_hip.volume import SphericalGrid, volume_metrics
    a, b = _volumes()
    grid = SphericalGrid(np.linspace(-np.pi / 2, np.pi / 2, 37), np.linspace(-np.pi, np.pi, 29), np.linspace(1.0, 1.3, 23))
    weights = [np.ones(n) for n in a.shape] if weighting == 'unit' else [w.numpy() for w in grid.cell_weights()]
    ta, tb = torch.from_numpy(a).cuda(), torch.from_numpy(b).cuda()
    got = volume_metrics(ta, tb, None if weighting == 'unit' else grid)
    terms, count, max_abs = vref.volume_terms(a, b, weights)
    assert 0.85 * a.size < count < 0.95 * a.size
    assert got['count'] == count and got['max_abs'] == max_abs             # exact
    for k in vref.TERMS:
        # at most a few hundred sequential fp64 additions per thread before the trees: tens of times above n 2^-53
        bound = 1e-12 * np.abs(terms[k]).sum()
        assert abs(got['sum_' + k] - terms[k].sum()) <= bound, (k, got['sum_' + k], terms[k].sum(), bound)
    want = vref.weighted_statistics(a, b, weights)
    for k in ('me', 'mae', 'rmse', 'pearson', 'mean_a', 'mean_b'):
        assert got[k] == pytest.approx(want[k], rel=1e-10, abs=1e-12), k
    assert got == volume_metrics(ta, tb, None if weighting == 'unit' else grid)      # bit-identical reruns
    assert got == volume_metrics(ta, tb, None if weighting == 'unit' else tuple(torch.from_numpy(w) for w in weights))
    # a volume against itself
    same = volume_metrics(ta, ta, None if weighting == 'unit' else grid)
    assert same['me'] == 0.0 and same['mae'] == 0.0 and same['rmse'] == 0.0 and same['max_abs'] == 0.0
    assert same['pearson'] == pytest.approx(1.0, abs=1e-12) and same['count'] == int(np.isfinite(a).sum())
    assert same['mean_a'] == same['mean_b']
    # every voxel masked: nothing counted, nan statistics, no fault
    none = volume_metrics(ta, torch.full_like(tb, float('nan')), None if weighting == 'unit' else grid)
    assert none['count'] == 0 and none['max_abs'] == 0.0 and none['sum_w'] == 0.0
    assert all(math.isnan(none[k]) for k in ('me', 'mae', 'rmse', 'pearson', 'mean_a', 'mean_b'))


def test_volume_metrics_shapes():
    from sunerf_hip.volume import Plane, volume_metrics
    gen = torch.Generator().manual_seed(2)
    a, b = torch.rand(33, 21, generator=gen).cuda(), torch.rand(33, 21, generator=gen).cuda()
    plane = Plane((0, 0, 0), (1, 0, 0), (0, 2, 0), np.linspace(-1, 1, 33), np.linspace(-1, 1, 21))
    got = volume_metrics(a, b, plane)                                      # a 2-d slice: n2 = 1
    assert got['count'] == 33 * 21 and got['sum_w'] == pytest.approx(2 * 2 * 2.0, rel=1e-13)
    d = (a.double() - b.double()).cpu().numpy()
    w = plane.cell_weights()
    ww = (w[0][:, None] * w[1][None, :]).numpy()
    assert got['mae'] == pytest.approx((ww * np.abs(d)).sum() / ww.sum(), rel=1e-12)
    big = torch.rand(129, 130, 131, generator=gen).cuda()                   # more voxels than one pass of the grid: the stride loop
    shifted = big + 0.25
    got = volume_metrics(shifted, big)
    d = (shifted.double() - big.double()).cpu().numpy()
    assert got['count'] == big.numel() and got['me'] == pytest.approx(d.mean(), rel=1e-12)
    assert got['max_abs'] == np.abs(d).max()
    one = volume_metrics(torch.ones(1, 1, 1).cuda(), torch.zeros(1, 1, 1).cuda())
    assert one['count'] == 1 and one['me'] == 1.0 and one['rmse'] == 1.0


# ---- loader -----------------------------------------------------------------------------------------------------------------
def test_loader_volume_and_slice_on_the_reference_state(tmp_path, monkeypatch):
    monkeypatch.setenv('SUNERF_FORWARD_PRECISION', 'exact')
    from sunerf.evaluation.loader import EnsembleLoader, SuNeRFLoader
    from sunerf_hip.volume import grid_points, load_volume, save_volume
    path = os.path.join(GOLDEN, 'g10_reference_state.snf')
    g10 = SuNeRFLoader(path, device='cuda')
    when = datetime.datetime(2022, 3, 2)
    vol = g10.render_volume(when, half_width=1.3, shape=24)
    assert vol['emission'].shape == vol['absorption'].shape == vol['radius'].shape == (24, 24, 24)
    assert vol['inferences'].shape == (24, 24, 24, 2) and all(isinstance(vol[k], np.ndarray) for k in ('emission', 'inferences'))
    grid = vol['grid']
    assert grid.shape == (24, 24, 24) and vol['times'] == g10.normalize_datetime(when) and vol['Rs_per_ds'] == float(g10.Rs_per_ds)
    pts, rad = grid_points(grid, vol['Rs_per_ds'], vol['times'])
    raw = g10.load_coords(pts.cpu().numpy().reshape(24, 24, 24, 4))        # the reference's point-query path, through the host
    assert np.array_equal(vol['inferences'], raw)
    inside = vol['radius'] >= 1.0
    assert np.array_equal(np.isnan(vol['emission']), ~inside) and 0.3 < inside.mean() < 0.95
    want = np.exp(raw[..., 0].astype(np.float64))
    err = (np.abs(vol['emission'][inside] - want[inside]) / want[inside]).max()
    print(f'render_volume emission against exp(load_coords): max relative error {err:.2e} (bound {REL:.0e})')
    assert err <= REL
    assert np.array_equal(vol['absorption'][inside], np.maximum(raw[..., 1], 0)[inside])
    dev = g10.render_volume(when, half_width=1.3, shape=24, batch_size=1000, as_numpy=False)
    assert dev['emission'].is_cuda and np.array_equal(dev['emission'].cpu().numpy(), vol['emission'], equal_nan=True)
    # a slice: the plane z = 0.1 of the same cube, and the file format on a real volume
    sl = g10.render_slice(when, origin=(0., 0., 0.1), half_width=1.3, shape=(24, 16), r_range=(1.0, 1.3))
    assert sl['emission'].shape == (24, 16) and sl['inferences'].shape == (24, 16, 2)
    assert np.array_equal(np.isnan(sl['emission']), vref.outside(sl['radius'], 1.0, 1.3))
    save_volume(tmp_path / 'cube.npz', vol)
    back = load_volume(tmp_path / 'cube.npz')
    assert np.array_equal(back['emission'], vol['emission'], equal_nan=True) and back['grid'].shape == (24, 24, 24)
    # an ensemble of the same member twice: the mean is the member, the spread zero
    ens = EnsembleLoader([path, path], device='cuda').render_volume(when, shape=12)
    single = g10.render_volume(when, shape=12)
    assert ens['emission_mean'].shape == (12, 12, 12)
    assert np.array_equal(ens['emission_mean'], single['emission'], equal_nan=True)
    assert (ens['emission_std'][~np.isnan(ens['emission_std'])] == 0).all()
    assert np.array_equal(np.isnan(ens['emission_std']), np.isnan(single['emission']))
