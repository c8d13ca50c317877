"""Line-of-sight DEM on MI355X (csrc/dem.hip: sunerf_dem_integral) against its float64 restatement
(tests/dem_reference.py) at the shapes where the kernel branches, and through ``render_dem``, the frame / column drivers and
the loaders.

The kernel gives a ray 32 lanes that walk its S - 1 quadrature points in chunks of 32 (the optical depth crosses a chunk seam
through a scalar carry) and keeps the K <= 128 bins in registers, four per lane.  So S runs over 2 (one point of weight 0),
3, 4, both sides of the seams at 33 / 34 and 65 / 66, and 1000 (nothing per sample lives in LDS); N over a lone ray, a partial
workgroup and a second workgroup (the grid is one workgroup per 8 rays: no grid-stride walk); K over 2, 3, both sides of 32 and
64, the table's 101 and the largest 128, plus a non-uniform grid.  Every case runs with NULL, a negative and an optically
thick (total optical depth 3 along the thickest ray) absorption scalar, without and with a radius mask that cuts some samples
of some rays and every sample of two (one far away, one with a NaN direction).  Inputs: ``dem_reference.make_case``.

Bounds, with the worst values measured on an MI355X over all direct-op cases:
  dem         gate_units vs fp64, floor 1e-6 em_ref (a bin fed by near-zero hat weights; an fp32 hat weight carries
              ~2e-7 absolute error, the floor is 5 x that)                                         <= 1   (0.008)
              exactly 0 where the reference bin is 0 (rays with every log T outside the grid: all bins)
  em, column  gate_units vs fp64 (1e-4 relative)                                                   <= 1   (0.002, 0.0014)
  logt_mean   1e-5 relative; NaN exactly where em_ref = 0                                                 (2.0e-7)
  sum_k dem = em to 1e-5 relative on rays with every sample inside the grid                               (1.3e-7)
  dem folded with the response rows x vol_c x pixel factor vs ops.dt_integral_fwd's image: gate_units <= 1 (0.002;
  0.003 through render_dem against a NeRF_DT's and a SimpleStar's own image)
Two runs, and a ray alone or inside a batch of 9, give the same bits.
"""
import numpy as np
import pytest
import torch

import dem_reference as ref
from conftest import gate_units, load_golden

pytestmark = pytest.mark.gpu

AIA = (94, 131, 171, 193, 211, 304, 335)
ABSORB = ('none', 'negative', 'thick')


@pytest.fixture(scope='module')
def dem():
    assert torch.cuda.is_available(), 'GPU tests need a ROCm device'
    from sunerf_hip import dem as _dem
    return _dem


_TABLES = {}


def tables():
    """g6's (logT grid (7, 101), response x exposure time (7, 101)), fp32.  All seven rows share one logT grid."""
    if not _TABLES:
        g = load_golden('g6_dt_e2e')
        _TABLES['t'] = (g['aia_logte'].contiguous(), (g['aia_tresp'] * float(g['aia_exp_time'])).float().contiguous())
    return _TABLES['t']


def table_grid():
    return tables()[0][0].numpy()


def same_bits(a, b):
    """Bit-for-bit equality of two fp32 tensors (NaN == NaN)."""
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def run(dem, c, log_abs, masked):
    cu = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()      # noqa: E731
    kw = dict(rays_o=cu(c['o']), rays_d=cu(c['d']), r_range=c['r_range']) if masked else {}
    return dem.dem_integral(cu(c['raw']), cu(c['z']), cu(c['nodes']), ref.BASE, log_abs, **kw)


def check_case(dem, c, worst):
    """All absorption modes x (no mask, mask) of case ``c`` against the reference; updates ``worst``."""
    cm = ref.add_mask(c)
    for masked, case in ((False, c), (True, cm)):
        for mode in ABSORB:
            log_abs = ref.log_abs_of(c, mode)
            got = run(dem, case, log_abs, masked)
            torch.cuda.synchronize()
            want = ref.dem_reference(case['inf'], case['z'], case['nodes'], log_abs,
                                     *((case['o'], case['d'], case['r_range']) if masked else ()))
            if masked and want['radius'] is not None:      # no sample near a mask radius: fp32 and fp64 decide alike
                rad = want['radius'][np.isfinite(want['radius'])]
                for edge in case['r_range']:
                    assert (np.abs(rad - edge) > 1e-5 * edge).all()
            em_ref = torch.from_numpy(want['em'])
            dem_ref = torch.from_numpy(want['dem'])
            what = f"N={c['n']} S={c['s']} K={len(c['nodes'])} {mode} mask={masked}"
            g_dem = got['dem'].cpu()
            assert g_dem.shape == dem_ref.shape
            assert bool((g_dem[dem_ref == 0] == 0).all()), f'{what}: a bin with a zero reference is not exactly 0'
            m = {'dem': gate_units(got['dem'], dem_ref, floor=1e-6 * em_ref[:, None]),
                 'em': gate_units(got['em'], em_ref), 'column': gate_units(got['column'], torch.from_numpy(want['column']))}
            lm, lm_ref = got['logt_mean'].cpu().double(), torch.from_numpy(want['logt_mean'])
            nan = em_ref == 0
            assert torch.equal(torch.isnan(lm), nan), f'{what}: logt_mean is NaN exactly where em = 0'
            m['logt_mean'] = ((lm - lm_ref).abs() / lm_ref.abs())[~nan].max().item() if bool((~nan).any()) else 0.0
            print(f'{what}: ' + ' '.join(f'{k} {v:.2e}' for k, v in m.items()))
            for k, v in m.items():
                worst[k] = max(worst.get(k, 0.0), v)
            assert m['dem'] <= 1.0 and m['em'] <= 1.0 and m['column'] <= 1.0, (what, m)
            assert m['logt_mean'] <= 1e-5, (what, m)
            if c['s'] > 2:
                outside = [r for r in range(2, c['n'], 5)]           # every log T outside the grid
                assert bool((g_dem[outside] == 0).all())
                if not masked:
                    assert bool((got['em'].cpu()[outside] > 0).all())
                    assert bool((got['em'].cpu() > 0).all()) and bool((got['column'].cpu() > 0).all())
            else:
                assert bool((g_dem == 0).all()) and bool((got['em'] == 0).all()) and bool((got['column'] == 0).all())
            if masked and c['n'] >= 2:
                assert got['em'][1].item() == 0 and got['column'][1].item() == 0          # the ray that is masked out whole
            if masked and c['n'] >= 4:
                assert got['em'][3].item() == 0 and got['column'][3].item() == 0          # NaN radius
            if mode == 'thick' and c['s'] > 3 and not masked:
                thin = run(dem, case, None, False)
                assert bool((got['em'] < thin['em']).all()) and same_bits(got['column'], thin['column'])


WORST = {}


@pytest.mark.parametrize('s', [2, 3, 4, 32, 33, 34, 65, 66, 257, 1000])
def test_dem_samples_per_ray(dem, s):
    """One quadrature point (S = 2) up to 1000 samples, the chunk seams at S - 1 = 32 / 33 and 64 / 65; 9 rays (two workgroups)
    on the table's 101 nodes."""
    check_case(dem, ref.make_case(9, s, table_grid(), seed=2 * s + 1), WORST)
    print('worst so far', WORST)


@pytest.mark.parametrize('n', [1, 7, 9])
def test_dem_batch_sizes(dem, n):
    """A lone ray, a partial workgroup, a second workgroup with one ray."""
    check_case(dem, ref.make_case(n, 34, table_grid(), seed=50 + n), WORST)


@pytest.mark.parametrize('uniform', [True, False])
@pytest.mark.parametrize('k', [2, 3, 32, 33, 64, 65, 101, 128])
def test_dem_node_counts(dem, k, uniform):
    """One interval up to the 128 nodes a lane's four registers hold, both sides of a register slot (32 / 33, 64 / 65), uniform
    and with random steps (K = 101 uniform: the table's own grid)."""
    nodes = ref.grid_nodes(k, table_grid(), uniform, seed=k)
    check_case(dem, ref.make_case(9, 66, nodes, seed=300 + k + 7 * uniform), WORST)
    print('worst so far', WORST)


def test_dem_conserves_the_emission_measure(dem):
    """Every sample inside the grid: the bins add up to em (1e-5 relative), with and without absorption."""
    for k, s in ((101, 66), (128, 257), (2, 33)):
        c = ref.make_case(9, s, ref.grid_nodes(k, table_grid()), seed=11 + k, all_inside=True)
        for mode in ABSORB:
            got = run(dem, c, ref.log_abs_of(c, mode), False)
            total, em = got['dem'].double().sum(1).cpu(), got['em'].double().cpu()
            rel = ((total - em).abs() / em).max().item()
            print(f'K={k} S={s} {mode}: sum_k dem vs em {rel:.2e}')
            assert bool((em > 0).all()) and rel <= 1e-5, (k, s, mode, rel)
            lo, hi = float(c['nodes'][0]), float(c['nodes'][-1])
            assert bool((got['logt_mean'] > lo).all()) and bool((got['logt_mean'] < hi).all())


def test_dem_folded_with_the_response_is_the_dt_image(dem):
    """On the table's grid: dem @ R_w x vol_c x pixel factor against ``ops.dt_integral_fwd``'s image for the same raw, optically
    thin for all seven channels and, with one channel's positive log_abs, for that channel."""
    from sunerf_hip import ops
    lt, resp = tables()
    c = ref.make_case(9, 66, table_grid(), seed=77)
    cu = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()      # noqa: E731
    raw, z, o, d = cu(c['raw']), cu(c['z']), cu(c['o']), cu(c['d'])
    wl = torch.tensor(AIA, dtype=torch.float32).expand(9, 7).contiguous().cuda()
    vol_c, pixel = torch.tensor([0.7]), float(torch.tensor(1e17))       # images of order 1 on NeRF_DT's bases
    thick = ref.log_abs_of(c, 'thick')
    for name, la in (('thin', torch.full((7,), -0.3 / c['tau1'])), ('thick 193', torch.tensor([-1., 0., -1., thick, 0., -1., 0.]))):
        la = la.float()
        image = ops.dt_integral_fwd(raw, z, o, d, wl, lt.cuda(), resp.cuda(), la.cuda(), vol_c.cuda(), *ref.BASE, pixel, 1.25)['image']
        channels = range(7) if name == 'thin' else (3,)
        got = dem.dem_integral(raw, z, cu(c['nodes']), ref.BASE, None if name == 'thin' else la[3:4].cuda())
        folded = dem.fold(got['dem'].double(), resp.double().cuda()) * float(vol_c) * pixel
        for ch in channels:
            assert bool((image[:, ch] > 0).any())
            u = gate_units(folded[:, ch], image[:, ch].cpu())
            print(f'{name}: channel {AIA[ch]} folded DEM vs DT image {u:.3f} gate units')
            assert u <= 1.0, (name, ch, u)
    # a thick DEM folded against the thin image must NOT agree: the attenuation is in the DEM
    thin_image = ops.dt_integral_fwd(raw, z, o, d, wl, lt.cuda(), resp.cuda(), torch.full((7,), -1.).cuda(), vol_c.cuda(), *ref.BASE,
                                     pixel, 1.25)['image']
    assert gate_units(folded[:, 3], thin_image[:, 3].cpu()) > 100.


def test_dem_is_deterministic(dem):
    """Two runs give the same bits; so does a ray alone and inside a batch of 9 (no atomics, one summation order)."""
    c = ref.add_mask(ref.make_case(9, 257, table_grid(), seed=9))
    log_abs = ref.log_abs_of(c, 'thick')
    a, b = run(dem, c, log_abs, True), run(dem, c, log_abs, True)
    for k in a:
        assert same_bits(a[k], b[k]), k
    for r in range(9):
        one = {k: v[r:r + 1] if k in ('raw', 'z', 'o', 'd', 'inf') else v for k, v in c.items()}
        alone = run(dem, one, log_abs, True)
        for k in a:
            assert same_bits(alone[k], a[k][r:r + 1]), (k, r)


def test_dem_optional_outputs_and_length_scale(dem):
    c = ref.make_case(7, 40, table_grid(), seed=4)
    cu = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()      # noqa: E731
    full = run(dem, c, None, False)
    part = dem.dem_integral(cu(c['raw']), cu(c['z']), cu(c['nodes']), ref.BASE, want=('em',))
    assert set(part) == {'em'} and same_bits(part['em'], full['em'])
    part = dem.dem_integral(cu(c['raw']), cu(c['z']), cu(c['nodes']), ref.BASE, want=('dem', 'logt_mean'))
    assert set(part) == {'dem', 'logt_mean'} and same_bits(part['dem'], full['dem']) and same_bits(part['logt_mean'], full['logt_mean'])
    scaled = dem.dem_integral(cu(c['raw']), cu(c['z']), cu(c['nodes']), ref.BASE, length_scale=4.0)
    for k in ('dem', 'em', 'column'):
        assert same_bits(scaled[k], full[k] * 4.0), k
    assert same_bits(scaled['logt_mean'], full['logt_mean'])
    with pytest.raises(ValueError, match='unsupported'):
        dem.dem_integral(cu(c['raw']), cu(c['z']), torch.linspace(5, 7, 129).cuda(), ref.BASE)
    with pytest.raises(ValueError, match='needs rays_o'):
        dem.dem_integral(cu(c['raw']), cu(c['z']), cu(c['nodes']), ref.BASE, r_range=(1.0, 2.0))
    per_dex = dem.per_dex(full['dem'], cu(c['nodes']))
    assert per_dex.shape == full['dem'].shape and per_dex.is_cuda


# ---- render_dem, drivers, loaders -------------------------------------------------------------------------------------------
def _nerf_dt():
    from sunerf.model.model import NeRF_DT
    from sunerf.rendering.density_temperature import DensityTemperatureRadiativeTransfer
    g = load_golden('g6_dt_e2e')
    mod = DensityTemperatureRadiativeTransfer(
        Rs_per_ds=1.0, sampling_config={'type': 'stratified', 'n_samples': 16, 'perturb': False},
        hierarchical_sampling_config={'type': 'hierarchical', 'n_samples': 16, 'perturb': False}, model_config={'d_filter': 64},
        model=NeRF_DT, pixel_intensity_factor=float(g['pixel_intensity_factor']),
        response_table=(g['aia_logte'].numpy(), g['aia_tresp'].numpy()))
    mod.load_state_dict({k[4:].replace('__', '.'): v for k, v in g.items() if k.startswith('sd__')}, strict=True)
    return mod.cuda()


def _star(n_samples=24):
    from sunerf.model.stellar_model import SimpleStar
    from sunerf.rendering.density_temperature import DensityTemperatureRadiativeTransfer
    g = load_golden('g9_simple_star')
    return DensityTemperatureRadiativeTransfer(
        Rs_per_ds=1, model=SimpleStar, model_config={},
        sampling_config={'type': 'stratified', 'n_samples': n_samples, 'perturb': False},
        hierarchical_sampling_config={'type': 'hierarchical', 'n_samples': n_samples, 'perturb': False},
        pixel_intensity_factor=float(g['pixel_intensity_factor']),
        response_table=(g['aia_logte'].numpy(), g['aia_tresp'].numpy())).cuda()


def _set_absorption(mod, values):
    with torch.no_grad():
        for m in (mod.coarse_model, mod.fine_model):
            for w, v in zip(AIA, values):
                m.log_absortpion[str(w)].fill_(v)


def _observer_rays(resolution=8):
    from sunerf_hip.rays import observer_rays
    o, d = observer_rays(resolution, device='cuda')
    t = torch.full((o.shape[0], 1), 0.4, device='cuda')
    return o, d, t


def _identity(mod, dem, what):
    """Folded ``render_dem`` against the module's own image: thin for all channels, then with one positive scalar."""
    o, d, t = _observer_rays()
    n = o.shape[0]
    wl = torch.tensor(AIA, dtype=torch.float32, device='cuda').expand(n, 7).contiguous()
    factor = float(mod.fine_model.volumetric_constant.detach()) * mod.pixel_intensity_factor
    _set_absorption(mod, (-1e-3, 0., -1e-3, 0., -1e-3, 0., -1e-3))
    with torch.no_grad():
        image = mod(o, d, t, wl)['image']
    out = mod.render_dem(o, d, t)
    assert out['dem'].shape == (n, 101) and out['em'].shape == out['logt_mean'].shape == out['column'].shape == (n,)
    assert torch.equal(out['logt_nodes'], mod.response_logte[0]) and out['z_vals'].shape[0] == n
    assert bool((image > 0).any()) and bool((out['em'] > 0).all())
    folded = dem.fold(out['dem'].double(), mod.response_table.double()) * factor
    u = gate_units(folded, image.cpu())
    print(f'{what}: folded render_dem vs image, optically thin, {u:.3f} gate units')
    assert u <= 1.0, (what, u)
    # one positive scalar: optical depth of order 1 along the thickest ray
    tau1 = float((out['column'] / 1.0).max())            # column = integral of rho: the optical depth at kappa = 1
    _set_absorption(mod, (0., 0., 0., 1.0 / tau1, 0., 0., 0.))
    with torch.no_grad():
        image_a = mod(o, d, t, wl)['image']
    out_a = mod.render_dem(o, d, t, attenuation_wavelength=193)
    assert bool((out_a['em'] < out['em']).all()) and same_bits(out_a['column'], out['column'])
    folded_a = dem.fold(out_a['dem'].double(), mod.response_table[3].double()) * factor
    u = gate_units(folded_a, image_a[:, 3].cpu())
    lit = image[:, 3] > 0
    dimmed = (image_a[:, 3][lit] / image[:, 3][lit]).min().item()
    print(f'{what}: folded render_dem vs image, attenuated at 193, {u:.3f} gate units (dimmest ray x {dimmed:.2f})')
    assert u <= 1.0 and dimmed < 0.8, (what, u, dimmed)
    with pytest.raises(ValueError, match='not a channel'):
        mod.render_dem(o, d, t, attenuation_wavelength=1600)


def test_render_dem_nerf_dt_folds_to_the_image(dem, monkeypatch):
    monkeypatch.setenv('SUNERF_FORWARD_PRECISION', 'exact')
    _identity(_nerf_dt(), dem, 'NeRF_DT d_filter 64')


def test_render_dem_simple_star_folds_to_the_image(dem):
    _identity(_star(), dem, 'SimpleStar')


def test_render_dem_custom_nodes_and_mask(dem):
    """A coarse user grid and a radius mask go through to the kernel: the result is ``dem_integral`` on the returned samples."""
    mod = _star()
    o, d, t = _observer_rays()
    nodes = torch.linspace(5.0, 7.0, 21)
    out = mod.render_dem(o, d, t, logt_nodes=nodes, r_range=(1.02, 1.2))
    assert out['dem'].shape == (o.shape[0], 21) and torch.equal(out['logt_nodes'].cpu(), nodes)
    raw = mod.fine_model.field_on_rays(o, d, out['z_vals'])
    want = dem.dem_integral(raw, out['z_vals'], nodes.cuda(), (0., 0.), None, o, d, (1.02, 1.2))
    for k in want:
        assert same_bits(out[k], want[k]), k
    full = mod.render_dem(o, d, t, logt_nodes=nodes)
    assert bool((out['em'] <= full['em']).all()) and bool((out['em'] < full['em']).any())


def test_render_dem_mhd_equals_dem_integral_of_the_sampled_cube(dem, tmp_path):
    import mhd_reference as mref
    from sunerf.model.mhd_model import MHDModel
    from sunerf.rendering.density_temperature import DensityTemperatureRadiativeTransfer
    frames = {10: mref.synthetic_frame(1), 11: mref.synthetic_frame(2), 12: mref.synthetic_frame(3)}
    root = mref.write_placeholders(tmp_path / 'run', sorted(frames))
    g = load_golden('g9_simple_star')
    mod = DensityTemperatureRadiativeTransfer(
        Rs_per_ds=1, model=MHDModel, model_config={'data_path': root, 'reader': mref.DictReader(frames)},
        sampling_config={'type': 'stratified', 'n_samples': 16, 'perturb': False},
        hierarchical_sampling_config={'type': 'hierarchical', 'n_samples': 16, 'perturb': False},
        pixel_intensity_factor=float(g['pixel_intensity_factor']),
        response_table=(g['aia_logte'].numpy(), g['aia_tresp'].numpy())).cuda()
    _set_absorption(mod, (2e-9, 3e-9, 4e-9, 5e-9, 6e-9, 7e-9, 8e-9))
    o, d, _ = _observer_rays()
    t = torch.full((o.shape[0], 1), 0.3, device='cuda')
    out = mod.render_dem(o, d, t, attenuation_wavelength=211)
    raw = mod.fine_model.field_on_rays(o, d, out['z_vals'], t)
    want = dem.dem_integral(raw, out['z_vals'], mod.response_logte[0].contiguous(), (0., 0.),
                            mod.fine_model.log_absortpion['211'].detach().reshape(1))
    assert bool((want['em'] > 0).any()) and bool((want['dem'] > 0).any())
    for k in want:
        assert same_bits(out[k], want[k]), k


def _loader(mod):
    from sunerf.evaluation.loader import ModelLoader
    grid = {'shape': (16, 16), 'cdelt': (150., 150.), 'meta': {'t_obs': '2022-01-01T00:00:00.000'}}
    return ModelLoader(rendering=mod, model=mod.fine_model, ref_map=grid)


def test_loader_dem_image_tiles_are_bit_identical(dem):
    """16 x 16 frame in ragged tiles of 100 rays against one tile: the same bits; numpy out by default."""
    loader = _loader(_star())
    tiled = loader.render_dem_image(0.1, 0.3, 0.4, batch_size=100, as_numpy=False)
    whole = loader.render_dem_image(0.1, 0.3, 0.4, as_numpy=False)
    assert tiled['dem'].shape == (16, 16, 101) and tiled['logt_nodes'].shape == (101,)
    for k in ('em', 'logt_mean', 'column'):
        assert tiled[k].shape == (16, 16), k
    for k in whole:
        assert same_bits(tiled[k], whole[k]), k
    assert bool((whole['em'] > 0).any())
    as_np = loader.render_dem_image(0.1, 0.3, 0.4, batch_size=100, length_scale=2.0)
    assert isinstance(as_np['dem'], np.ndarray) and np.array_equal(as_np['em'], (whole['em'] * 2.0).cpu().numpy())
    cut = loader.render_dem_image(0.1, 0.3, 0.4, r_range=(1.05, 1.2), as_numpy=False)
    assert bool((cut['em'] <= whole['em']).all()) and bool((cut['em'] < whole['em']).any())


def test_loader_dem_image_nerf_dt_tiles_are_bit_identical(dem, monkeypatch):
    monkeypatch.setenv('SUNERF_FORWARD_PRECISION', 'exact')
    mod = _nerf_dt()
    _set_absorption(mod, (0.,) * 7)
    loader = _loader(mod)
    tiled = loader.render_dem_image(0.1, 0.3, 0.4, batch_size=100, as_numpy=False)
    whole = loader.render_dem_image(0.1, 0.3, 0.4, as_numpy=False)
    for k in whole:
        assert same_bits(tiled[k], whole[k]), k
    assert bool((whole['em'] > 0).all())


def test_loader_dem_map_shapes_and_column(dem):
    """5 x 9 map: documented shapes; its outputs are ``dem_integral``'s on the same columns (the column's r_range as mask
    cuts none of its own samples, the two ends included)."""
    from sunerf_hip.maps import column_rays, radial_row
    mod = _star()
    loader = _loader(mod)
    S = 48
    out = loader.render_dem_map(0.4, shape=(5, 9), r_range=(1.0, 1.3), n_samples=S, batch_size=7, as_numpy=False)
    assert out['dem'].shape == (5, 9, 101) and out['logt_nodes'].shape == (101,)
    for k in ('em', 'logt_mean', 'column'):
        assert out[k].shape == (5, 9), k
    lat = torch.from_numpy(np.linspace(-np.pi / 2, np.pi / 2, 5)).cuda()
    lon = torch.from_numpy(np.linspace(-np.pi, np.pi, 9)).cuda()
    o, d = column_rays(lat, lon)
    z = radial_row((1.0, 1.3), S, 1.0).cuda()[None].expand(45, -1).contiguous()
    raw = mod.fine_model.field_on_rays(o, d, z)
    want = dem.dem_integral(raw, z, mod.response_logte[0].contiguous(), (0., 0.))
    for k in want:
        assert same_bits(out[k].reshape(want[k].shape), want[k]), k
    assert bool((want['column'] > 0).all())
    as_np = loader.render_dem_map(0.4, shape=(5, 9), n_samples=S, attenuation_wavelength=171)
    assert isinstance(as_np['column'], np.ndarray) and as_np['dem'].shape == (5, 9, 101)
    assert np.array_equal(as_np['column'], want['column'].reshape(5, 9).cpu().numpy())
