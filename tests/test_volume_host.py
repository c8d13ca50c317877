"""3-D volumes on the host: the grids' fp64 restatements, layouts and cell weights, the argument checks that run
before anything touches the device, the loader's grids and times, the file format and the statistics derived from the sums."""
import datetime
import math

import numpy as np
import pytest
import torch

import volume_reference as vref


def _emission(Rs_per_ds=1.0):
    from sunerf.rendering.emission import EmissionRadiativeTransfer
    return EmissionRadiativeTransfer(Rs_per_ds=Rs_per_ds, sampling_config={'type': 'stratified', 'n_samples': 8, 'perturb': False},
                                     hierarchical_sampling_config={'type': 'hierarchical', 'n_samples': 8},
                                     model_config={'d_filter': 64})


def _dt():
    from conftest import load_golden
    from sunerf.model.model import NeRF_DT
    from sunerf.rendering.density_temperature import DensityTemperatureRadiativeTransfer
    g = load_golden('g6_dt_e2e')
    return DensityTemperatureRadiativeTransfer(
        Rs_per_ds=1.0, sampling_config={'type': 'stratified', 'n_samples': 8, 'perturb': False},
        hierarchical_sampling_config={'type': 'hierarchical', 'n_samples': 8}, model_config={'d_filter': 64}, model=NeRF_DT,
        pixel_intensity_factor=1.0, response_table=(g['aia_logte'].numpy(), g['aia_tresp'].numpy()))


# ---- grids ------------------------------------------------------------------------------------------------------------------
def test_identity_frame_reproduces_float32_axes():
    from sunerf_hip.volume import CartesianGrid
    x = np.linspace(-1.3, 1.3, 7, dtype=np.float32)
    y = np.linspace(-0.7, 0.9, 5, dtype=np.float32)
    z = np.linspace(0.1, 2.0, 3, dtype=np.float32)
    grid = CartesianGrid(x, y, z)
    assert grid.shape == (7, 5, 3)
    p = grid.points_f64(1.0)
    assert p.dtype == torch.float64 and p.shape == (7, 5, 3, 3)
    want = np.stack(np.meshgrid(x, y, z, indexing='ij'), -1)            # plain C order (x, y, z): NOT meshgrid's default 'xy'
    assert np.array_equal(p.float().numpy(), want)
    r = grid.radius_f64()
    assert r.shape == (7, 5, 3) and (r - p.norm(dim=-1)).abs().max().item() < 1e-15
    cube = CartesianGrid.cube(1.3, 4)
    assert cube.shape == (4, 4, 4) and cube.axes[0][0] == -1.3 and cube.axes[2][-1] == 1.3


def test_c_order_layout_and_oblique_frame():
    from sunerf_hip.volume import CartesianGrid, Plane
    basis = np.array([[1., 0.2, 0.], [0., 1., 0.5], [0.3, 0., 2.]])
    origin = np.array([0.1, -0.2, 0.3])
    x, y, z = np.array([0., 1., 2.]), np.array([-1., 1.]), np.array([0.5, 0.75, 1.0, 1.25])
    grid = CartesianGrid(x, y, z, origin, basis)
    p = grid.points_f64(2.0).reshape(-1, 3)
    for i in range(3):
        for j in range(2):
            for k in range(4):
                want = (origin + x[i] * basis[0] + y[j] * basis[1] + z[k] * basis[2]) / 2.0
                assert np.array_equal(p[(i * 2 + j) * 4 + k].numpy(), want), (i, j, k)       # last axis fastest
    plane = Plane(origin, basis[0], basis[1], x, y)
    assert plane.shape == (3, 2) and plane.n_voxels == 6
    q = plane.points_f64(1.0)
    assert q.shape == (3, 2, 3)
    assert np.array_equal(q[2, 1].numpy(), origin + x[2] * basis[0] + y[1] * basis[1] + 0. * np.zeros(3))
    assert plane.radius_f64().shape == (3, 2)


def test_spherical_restatement_is_column_directions_times_r():
    from sunerf_hip.maps import column_directions, grid_columns
    from sunerf_hip.volume import SphericalGrid
    lat = torch.linspace(-math.pi / 2, math.pi / 2, 9, dtype=torch.float64)
    lon = torch.linspace(-math.pi, math.pi, 13, dtype=torch.float64)
    r = torch.linspace(1.0, 1.3, 5, dtype=torch.float64)
    grid = SphericalGrid(lat, lon, r)
    assert grid.shape == (9, 13, 5)                                        # the layout of render_heliographic_map(profiles=True)
    u = column_directions(*grid_columns(lat, lon)).reshape(9, 13, 3)
    want = u[:, :, None, :] * r[None, None, :, None] / 0.5
    assert torch.equal(grid.points_f64(0.5), want)
    assert torch.equal(grid.radius_f64(), r.expand(9, 13, 5))
    assert grid.points_f64(1.0)[0, 0, 0, 2].item() == pytest.approx(1.0)   # lat = -90 deg: u = (0, 0, +1)


def test_cell_weights_sum_to_the_volume():
    from sunerf_hip.volume import CartesianGrid, Plane, SphericalGrid, trapezoid_widths
    assert torch.equal(trapezoid_widths(torch.tensor([0., 1., 3.], dtype=torch.float64)),
                       torch.tensor([0.5, 1.5, 1.0], dtype=torch.float64))
    x, y, z = np.linspace(-1., 2., 11), np.sort(np.random.default_rng(0).uniform(0., 1., 7)), np.linspace(3., 3.5, 4)
    w = CartesianGrid(x, y, z).cell_weights()
    total = (w[0][:, None, None] * w[1][None, :, None] * w[2][None, None, :]).sum().item()
    assert total == pytest.approx(3. * (y[-1] - y[0]) * 0.5, rel=1e-13)
    basis = np.array([[1., 0.2, 0.], [0., 1., 0.5], [0.3, 0., 2.]])
    w = CartesianGrid(x, y, z, basis=basis).cell_weights()
    total = (w[0][:, None, None] * w[1][None, :, None] * w[2][None, None, :]).sum().item()
    assert total == pytest.approx(3. * (y[-1] - y[0]) * 0.5 * abs(np.linalg.det(basis)), rel=1e-13)
    w = Plane((0, 0, 0), (2., 0, 0), (0, 0, 3.), x, z).cell_weights()
    assert len(w) == 3 and w[2].tolist() == [1.0]
    assert (w[0][:, None] * w[1][None, :]).sum().item() == pytest.approx(3. * 0.5 * 6., rel=1e-13)
    # a full sphere: 4 pi / 3 (r_out^3 - r_in^3).  The trapezoid rule's own error with step h is h^2 / 12 (f'(b) - f'(a)): relative
    # pi^2 / (12 n^2) = 1.6e-6 for cos(lat) over pi (n = 720 intervals), 1.7e-7 for r^2 over [1, 1.3] (n = 256), none in longitude
    n_lat, n_r = 721, 257
    grid = SphericalGrid(np.linspace(-np.pi / 2, np.pi / 2, n_lat), np.linspace(-np.pi, np.pi, 1441), np.linspace(1.0, 1.3, n_r))
    w = grid.cell_weights()
    total = w[0].sum().item() * w[1].sum().item() * w[2].sum().item()
    exact = 4 * np.pi / 3 * (1.3 ** 3 - 1.0)
    own = np.pi ** 2 / (12 * (n_lat - 1) ** 2) + 0.3 ** 2 / (12 * (n_r - 1) ** 2) * 2 / ((1.3 ** 3 - 1.0) / 0.9)
    print(f'sphere volume: relative error {abs(total / exact - 1):.2e}, the rule\'s own {own:.2e}')
    assert abs(total / exact - 1) <= 1.5 * own


# ---- argument checks --------------------------------------------------------------------------------------------------------
def test_bad_grids_are_rejected():
    from sunerf_hip.volume import CartesianGrid, Plane, SphericalGrid
    ax = np.linspace(-1, 1, 3)
    for bad in (dict(x=[]), dict(x=[[0., 1.]]), dict(y=[0., float('nan')]), dict(origin=(0., 1.)), dict(basis=np.eye(2)),
                dict(basis=np.full((3, 3), np.inf))):
        args = dict(x=ax, y=ax, z=ax)
        args.update(bad)
        with pytest.raises(ValueError):
            CartesianGrid(**args)
    with pytest.raises(ValueError):
        CartesianGrid.cube(1.3, 0)
    with pytest.raises(ValueError):
        CartesianGrid.cube(-1.0, 4)
    with pytest.raises(ValueError):
        Plane((0, 0, 0), (1, 0), (0, 1, 0), ax, ax)
    with pytest.raises(ValueError):
        SphericalGrid(ax, ax, [-1.0, 1.0])


def test_bad_arguments_are_rejected_before_the_device():
    from sunerf_hip import SunerfHipError
    from sunerf_hip.volume import CartesianGrid, field_quantities, grid_points, sample_volume, volume_metrics
    grid = CartesianGrid.cube(1.3, 4)
    rendering = _emission()                                               # on the CPU: a check that came late would say so
    bad = [dict(r_range=(1.3, 1.0)), dict(r_range=(1.0,)), dict(r_range=(float('nan'), None)), dict(tile_points=0),
           dict(tile_points=2.5), dict(time=float('inf')), dict(time=[]), dict(quantities=('density',)),
           dict(quantities=('emission', 'nonsense')), dict(model='middle'), dict(kind='dt'), dict(kind='x-ray'),
           dict(wavelengths=[171.]), dict(Rs_per_ds=0.0)]
    for kw in bad:
        args = dict(time=0.0)
        args.update(kw)
        with pytest.raises(ValueError):
            sample_volume(rendering, grid, **args)
    with pytest.raises(TypeError):
        sample_volume(rendering, 'cube', 0.0)
    with pytest.raises(ValueError, match='rank'):
        sample_volume(rendering, grid, 0.0, rank=2, world=2)
    with pytest.raises(ValueError, match='process group'):
        sample_volume(rendering, grid, 0.0, rank=0, world=2)
    with pytest.raises(ValueError, match='kind='):
        sample_volume(rendering.fine_model, grid, 0.0)                    # a bare field module says nothing about its answer
    with pytest.raises(SunerfHipError, match='CPU'):
        sample_volume(rendering, grid, 0.0)                               # every argument fine: only now the device matters
    with pytest.raises(SunerfHipError, match='CPU'):
        sample_volume(rendering.fine_model, grid, [0.0, 0.5], kind='emission')
    dt = _dt()
    with pytest.raises(ValueError, match='wavelengths'):
        sample_volume(dt, grid, 0.0)                                      # missing, as in render_columns
    with pytest.raises(ValueError, match='wavelengths'):
        sample_volume(dt, grid, 0.0, wavelengths=[171.], quantities=('density',))     # unwanted
    with pytest.raises(ValueError, match='wavelengths'):
        sample_volume(dt, grid, 0.0, wavelengths=np.full(8, 171.))
    with pytest.raises(ValueError, match='response_table'):
        sample_volume(dt.fine_model, grid, 0.0, wavelengths=[171.], kind='dt')
    with pytest.raises(SunerfHipError, match='CPU'):
        sample_volume(dt, grid, 0.0, wavelengths=[171., 193.])
    with pytest.raises(SunerfHipError, match='CPU'):
        sample_volume(dt, grid, 0.0, quantities=('density', 'log_temperature'))
    # the wrappers
    with pytest.raises(ValueError):
        grid_points(grid, 1.0, 0.0, first=60, count=10)
    with pytest.raises(ValueError):
        grid_points(grid, -1.0)
    with pytest.raises(TypeError):
        grid_points(None)
    with pytest.raises(SunerfHipError):
        grid_points(grid, device='cpu')
    inf, rad = torch.zeros(5, 2), torch.ones(5)
    with pytest.raises(ValueError):
        field_quantities(inf, rad, 'emission', r_range=(2.0, 1.0))
    with pytest.raises(ValueError):
        field_quantities(inf, rad, 'emission', quantities=('density',))
    with pytest.raises(ValueError):
        field_quantities(inf, rad, 'dt', quantities=('emissivity',))          # no wavelengths
    with pytest.raises(ValueError):
        field_quantities(inf, rad, 'emission', wavelengths=[171.])
    with pytest.raises(SunerfHipError):
        field_quantities(inf, rad, 'emission')
    a = torch.zeros(3, 4, 5)
    with pytest.raises(ValueError):
        volume_metrics(a, torch.zeros(3, 4, 6))
    with pytest.raises(ValueError):
        volume_metrics(torch.zeros(5), torch.zeros(5))
    with pytest.raises(ValueError):
        volume_metrics(a, a, weights=(torch.ones(3), torch.ones(4)))
    with pytest.raises(ValueError):
        volume_metrics(a, a, weights=grid)                                # a 4 x 4 x 4 grid's weights on 3 x 4 x 5 volumes
    with pytest.raises(SunerfHipError):
        volume_metrics(a, a)


def test_thomson_and_hooked_renderings_name_their_kind():
    from sunerf.rendering.emission import EmissionRadiativeTransfer
    from sunerf.rendering.thompson import ThompsonScattering
    from sunerf_hip.volume import _volume_kind

    def cfg():                                                            # (the constructors pop 'type' from the dicts)
        return dict(Rs_per_ds=1.0, sampling_config={'type': 'stratified', 'n_samples': 8, 'perturb': False},
                    hierarchical_sampling_config={'type': 'hierarchical', 'n_samples': 8}, model_config={'d_filter': 64})
    th = ThompsonScattering(**cfg())
    net, kind, rendering = _volume_kind(th, None, 'coarse')
    assert kind == 'white_light' and net is th.coarse_model and rendering is th
    assert _volume_kind(_emission(), None, 'fine')[1] == 'emission' and _volume_kind(_dt(), None, 'fine')[1] == 'dt'

    class Own(EmissionRadiativeTransfer):
        def raw2outputs(self, raw, z_vals, rays_d, **kwargs):
            return super().raw2outputs(raw * 2, z_vals, rays_d, **kwargs)
    own = Own(**cfg())
    with pytest.raises(ValueError, match='kind='):
        _volume_kind(own, None, 'fine')
    assert _volume_kind(own, 'emission', 'fine')[1] == 'emission'

    class OwnRender(EmissionRadiativeTransfer):                           # the hooks of maps._kind, not raw2outputs alone
        def _render(self, model, query_points, rays_d, rays_o, z_vals):
            return super()._render(model, query_points, rays_d, rays_o, z_vals)
    with pytest.raises(ValueError, match='kind='):
        _volume_kind(OwnRender(**cfg()), None, 'fine')


def test_exported_symbols():
    import sunerf_hip
    assert {'sunerf_grid_points', 'sunerf_field_quantities', 'sunerf_volume_metrics'} <= set(sunerf_hip.symbols('core'))


# ---- loader -----------------------------------------------------------------------------------------------------------------
def test_loader_grids_and_times(monkeypatch):
    """The loader's volume / slice methods hand sample_volume the right grid, the normalised time and the channels."""
    from sunerf.evaluation import loader as L
    from sunerf_hip.volume import CartesianGrid, Plane, SphericalGrid
    seen = {}

    def fake(rendering, grid, time, wavelengths=None, quantities=None, r_range=(1.0, None), fill=float('nan'), model='fine',
             tile_points=None, **kw):
        seen.update(rendering=rendering, grid=grid, time=time, wl=wavelengths, quantities=quantities, r_range=r_range, fill=fill,
                    tile=tile_points, model=model)
        return {'emission': torch.zeros(grid.shape), 'radius': torch.ones(grid.shape), 'grid': grid, 'times': time}
    monkeypatch.setattr(L, 'sample_volume', fake)
    ld = L.SuNeRFLoader.__new__(L.SuNeRFLoader)
    ld.device, ld.rendering = torch.device('cpu'), 'the rendering'
    ld.seconds_per_dt, ld.ref_time = 86400., datetime.datetime(2022, 1, 1)
    out = ld.render_volume(datetime.datetime(2022, 1, 2, 12), half_width=1.2, shape=6)
    assert out['emission'].shape == (6, 6, 6) and isinstance(out['emission'], np.ndarray) and out['grid'] is seen['grid']
    g = seen['grid']
    assert type(g) is CartesianGrid and g.shape == (6, 6, 6) and seen['rendering'] == 'the rendering'
    assert seen['time'] == 1.5 and seen['wl'] is None and seen['tile'] is None and seen['r_range'] == (1.0, None)
    assert math.isnan(seen['fill']) and seen['model'] == 'fine'
    for a in g.axes:
        assert np.array_equal(a.numpy(), np.linspace(-1.2, 1.2, 6))
    assert torch.equal(g.basis, torch.eye(3, dtype=torch.float64)) and g.origin.tolist() == [0., 0., 0.]
    ld.render_volume(datetime.datetime(2022, 1, 1), half_width=(1.0, 1.1, 1.2), shape=(2, 3, 4), batch_size=100, r_range=(1.0, 1.3),
                     as_numpy=False)
    assert seen['grid'].shape == (2, 3, 4) and seen['grid'].axes[1][-1] == 1.1 and seen['tile'] == 100 and seen['time'] == 0.0
    assert seen['r_range'] == (1.0, 1.3)
    shell = SphericalGrid(np.linspace(-1, 1, 3), np.linspace(-2, 2, 5), np.linspace(1.0, 1.3, 4))
    ld.render_volume(datetime.datetime(2022, 1, 1), grid=shell)
    assert seen['grid'] is shell
    out = ld.render_slice(datetime.datetime(2022, 1, 1, 6), origin=(0., 0., 0.1), e_u=(0., 1., 0.), e_v=(0., 0., 1.), half_width=1.5,
                          shape=(4, 8), quantities=('emission',))
    p = seen['grid']
    assert type(p) is Plane and p.shape == (4, 8) and out['emission'].shape == (4, 8) and seen['time'] == 0.25
    assert p.origin.tolist() == [0., 0., 0.1] and p.basis[0].tolist() == [0., 1., 0.] and p.basis[1].tolist() == [0., 0., 1.]
    assert np.array_equal(p.axes[0].numpy(), np.linspace(-1.5, 1.5, 4)) and np.array_equal(p.axes[1].numpy(), np.linspace(-1.5, 1.5, 8))
    assert seen['quantities'] == ('emission',)
    ml = L.ModelLoader.__new__(L.ModelLoader)
    ml.device, ml.rendering = torch.device('cpu'), None
    ml.render_volume(0.25, shape=3, wl=np.array([171, 193]), batch_size=64)
    assert seen['time'] == 0.25 and seen['tile'] == 64 and seen['wl'].tolist() == [171., 193.] and seen['grid'].shape == (3, 3, 3)
    ml.render_slice(0.75, shape=5, wl=np.array([211]))
    assert seen['time'] == 0.75 and seen['wl'].tolist() == [211.] and seen['grid'].shape == (5, 5)


def test_ensemble_volume_mean_and_std(monkeypatch):
    from sunerf.evaluation import loader as L
    fields = [torch.tensor([[[1., 2.], [float('nan'), 4.]]]), torch.tensor([[[3., 2.], [float('nan'), 0.]]])]

    class Member:
        def __init__(self, f):
            self.f = f

        def render_volume(self, time, grid=None, **kw):
            assert kw['as_numpy'] is False
            return {'emission': self.f, 'inferences': self.f[..., None], 'radius': torch.ones(1, 2, 2), 'grid': grid, 'times': 0.5,
                    'kind': 'emission', 'wavelengths': torch.tensor([171.])}      # only the kind's quantities are averaged
    ens = L.EnsembleLoader.__new__(L.EnsembleLoader)
    ens.loaders = [Member(f) for f in fields]
    out = ens.render_volume(datetime.datetime(2022, 1, 1), shape=2)
    assert set(out) == {'emission_mean', 'emission_std', 'radius', 'grid', 'times', 'kind'}
    assert np.array_equal(out['emission_mean'], np.array([[[2., 2.], [np.nan, 2.]]], np.float32), equal_nan=True)
    assert np.array_equal(out['emission_std'], np.array([[[1., 0.], [np.nan, 2.]]], np.float32), equal_nan=True)
    assert out['grid'].shape == (2, 2, 2)


# ---- files ------------------------------------------------------------------------------------------------------------------
def test_npz_round_trip(tmp_path):
    from sunerf_hip.volume import CartesianGrid, Plane, SphericalGrid, load_volume, save_volume
    gen = torch.Generator().manual_seed(4)
    basis = np.array([[1., 0.2, 0.], [0., 1., 0.5], [0.3, 0., 2.]])
    grids = [CartesianGrid(np.linspace(-1, 1, 3), np.linspace(0, 1, 4), np.linspace(2, 3, 5), (0.1, 0.2, 0.3), basis),
             Plane((0., 0.5, 0.), (1., 0., 0.), (0., 0., 1.), np.linspace(-2, 2, 6), np.linspace(-1, 1, 3)),
             SphericalGrid(np.linspace(-1.5, 1.5, 4), np.linspace(-3, 3, 5), np.linspace(1.0, 1.3, 6))]
    for n, grid in enumerate(grids):
        em = torch.rand((2,) + grid.shape, generator=gen)
        em[0].view(-1)[0] = float('nan')
        vol = {'emission': em, 'inferences': torch.rand((2,) + grid.shape + (2,), generator=gen), 'radius': grid.radius_f64().float(),
               'grid': grid, 'times': [0.25, 0.5], 'Rs_per_ds': 1.5, 'kind': 'emission'}
        path = tmp_path / f'volume{n}.npz'
        save_volume(path, vol)
        back = load_volume(path)
        assert set(back) == set(vol)
        assert type(back['grid']) is type(grid) and back['grid'].shape == grid.shape
        assert torch.equal(back['grid'].points_f64(1.5), grid.points_f64(1.5))
        assert all(torch.equal(x, y) for x, y in zip(back['grid'].cell_weights(), grid.cell_weights()))
        assert back['times'] == [0.25, 0.5] and back['Rs_per_ds'] == 1.5 and back['kind'] == 'emission'
        for k in ('emission', 'inferences', 'radius'):
            assert isinstance(back[k], np.ndarray) and np.array_equal(back[k], vol[k].numpy(), equal_nan=True), k
    with pytest.raises(ValueError):
        save_volume(tmp_path / 'x.npz', {'emission': torch.zeros(2)})
    with pytest.raises(ValueError):
        save_volume(tmp_path / 'x.npz', {'grid': grids[0], 'axis0': torch.zeros(2)})


# ---- statistics from sums ---------------------------------------------------------------------------------------------------
def test_statistics_from_sums_equal_numpy():
    from sunerf_hip.volume import SUM_NAMES, SphericalGrid, metrics_from_sums
    rng = np.random.default_rng(5)
    a = rng.normal(2.0, 1.0, (7, 6, 5)).astype(np.float32)
    b = (0.7 * a + rng.normal(0.0, 0.5, a.shape)).astype(np.float32)
    a[1, 2, 3] = np.nan
    b[4, 0, 1] = np.inf
    grid = SphericalGrid(np.linspace(-1.2, 1.2, 7), np.linspace(-3, 3, 6), np.linspace(1.0, 1.3, 5))
    weights = [w.numpy() for w in grid.cell_weights()]
    terms, count, max_abs = vref.volume_terms(a, b, weights)
    sums = [terms[k].sum() for k in vref.TERMS] + [max_abs, count]
    assert len(sums) == len(SUM_NAMES) and vref.TERMS == SUM_NAMES[:9]
    got = metrics_from_sums(sums)
    want = vref.weighted_statistics(a, b, weights)
    assert got['count'] == want['count'] == a.size - 2 and got['max_abs'] == want['max_abs']
    for k in ('me', 'mae', 'rmse', 'pearson', 'mean_a', 'mean_b'):
        assert got[k] == pytest.approx(want[k], rel=1e-12, abs=1e-14), k
    assert got['sum_wab'] == sums[8]
    empty = metrics_from_sums([0.] * 11)
    assert empty['count'] == 0 and empty['max_abs'] == 0.0
    assert all(math.isnan(empty[k]) for k in ('me', 'mae', 'rmse', 'pearson', 'mean_a', 'mean_b'))
