"""Heliographic columns on the host: the fp64 restatement of the column direction against the observer pose,
the grid layout, the argument checks that run before anything touches the device, and the loader's axes."""
import datetime
import math

import numpy as np
import pytest
import torch

import sunerf_oracle as orc


def _pose_f64(theta, phi, radius):
    """pose_spherical (coordinate_transformation.py:36-54) composed in float64 from the same matrices as the oracle's."""
    m = lambda rows: np.array(rows, dtype=np.float64)   # noqa: E731
    c2w = m([[1, 0, 0, 0], [0, 1, 0, 0], [0, 0, 1, radius], [0, 0, 0, 1]])
    c2w = m([[1, 0, 0, 0], [0, np.cos(phi), -np.sin(phi), 0], [0, np.sin(phi), np.cos(phi), 0], [0, 0, 0, 1]]) @ c2w
    c2w = m([[np.cos(theta), 0, -np.sin(theta), 0], [0, 1, 0, 0], [np.sin(theta), 0, np.cos(theta), 0], [0, 0, 0, 1]]) @ c2w
    return m([[-1, 0, 0, 0], [0, 0, 1, 0], [0, 1, 0, 0], [0, 0, 0, 1]]) @ c2w


def test_column_direction_is_the_normalised_observer_position():
    from sunerf_hip.maps import column_directions
    gen = torch.Generator().manual_seed(11)
    lat = (torch.rand(200, generator=gen, dtype=torch.float64) - 0.5) * math.pi
    lon = (torch.rand(200, generator=gen, dtype=torch.float64) - 0.5) * 2 * math.pi
    u = column_directions(lat, lon)
    assert u.dtype == torch.float64 and u.shape == (200, 3)
    assert (u.norm(dim=1) - 1).abs().max().item() < 1e-15
    worst32 = worst64 = 0.0
    for i in range(lat.shape[0]):
        b, l = lat[i].item(), lon[i].item()
        pos = orc.pose_spherical(-l, b, 215.)[:3, 3].double()            # the oracle builds its matrices in fp32
        worst32 = max(worst32, (pos / pos.norm() - u[i]).abs().max().item())
        pos = torch.from_numpy(_pose_f64(-l, b, 215.)[:3, 3])            # the same chain in fp64
        worst64 = max(worst64, (pos / pos.norm() - u[i]).abs().max().item())
    assert worst64 < 1e-12, worst64
    assert worst32 < 1e-6, worst32


def test_grid_layout_south_first_then_longitude():
    from sunerf_hip.maps import column_directions, grid_columns
    lat = torch.linspace(-math.pi / 2, math.pi / 2, 5, dtype=torch.float64)
    lon = torch.linspace(-math.pi, math.pi, 7, dtype=torch.float64)
    plat, plon = grid_columns(lat, lon)
    assert plat.shape == plon.shape == (35,)
    for row in range(5):
        for col in range(7):
            assert plat[row * 7 + col] == lat[row] and plon[row * 7 + col] == lon[col]
    assert plat[0] == lat.min() and plon[0] == lon.min()                 # row 0: the south; column 0: the smallest longitude
    u = column_directions(plat, plon)
    assert u[0, 2].item() == pytest.approx(1.0)                           # lat = -90 deg: u = (0, 0, -sin lat) (the scripts' lat' = 90 deg)


def test_radial_row():
    from sunerf_hip.maps import radial_row
    z = radial_row((1.0, 1.3), 5, 2.0)
    assert z.dtype == torch.float32
    assert torch.equal(z, (torch.linspace(1.0, 1.3, 5, dtype=torch.float64) / 2).float())


def _emission(Rs_per_ds=1.0):
    from sunerf.rendering.emission import EmissionRadiativeTransfer
    return EmissionRadiativeTransfer(Rs_per_ds=Rs_per_ds, sampling_config={'type': 'stratified', 'n_samples': 8, 'perturb': False},
                                     hierarchical_sampling_config={'type': 'hierarchical', 'n_samples': 8},
                                     model_config={'d_filter': 64})


def test_bad_arguments_are_rejected_before_the_device():
    from sunerf_hip.maps import check_columns, render_columns
    lat = torch.linspace(-1, 1, 4, dtype=torch.float64)
    lon = torch.linspace(-2, 2, 6, dtype=torch.float64)
    assert check_columns(lat, lon, True, (1.0, 1.3), 2) == (4, 6)
    assert check_columns(lat, lat, False, (1.0, 1.3), 2) == (4, 1)
    bad = [dict(n_samples=1), dict(n_samples=0), dict(r_range=(1.3, 1.3)), dict(r_range=(1.3, 1.0)),
           dict(r_range=(1.0, float('nan')))]
    rendering = _emission()                                               # on the CPU: a check that came late would say so
    for kw in bad:
        args = dict(r_range=(1.0, 1.3), n_samples=16)
        args.update(kw)
        with pytest.raises(ValueError):
            check_columns(lat, lon, True, args['r_range'], args['n_samples'])
        with pytest.raises(ValueError):
            render_columns(rendering, lat, lon, 0.0, **args)
    with pytest.raises(ValueError, match='same length'):
        render_columns(rendering, lat, lon, 0.0, grid=False)
    with pytest.raises(ValueError, match='empty grid'):
        render_columns(rendering, lat[:0], lon, 0.0)
    with pytest.raises(ValueError, match='no columns'):
        render_columns(rendering, lat[:0], lon[:0], 0.0, grid=False)
    with pytest.raises(ValueError, match='wavelengths'):
        render_columns(rendering, lat, lon, 0.0, wavelengths=torch.tensor([171.]))
    with pytest.raises(ValueError, match='rank'):
        render_columns(rendering, lat, lon, 0.0, rank=2, world=2)
    with pytest.raises(ValueError, match='process group'):
        render_columns(rendering, lat, lon, 0.0, rank=0, world=2)


def test_thomson_is_refused():
    from sunerf.rendering.thompson import ThompsonScattering
    from sunerf_hip.maps import render_columns
    th = ThompsonScattering(Rs_per_ds=1.0, sampling_config={'type': 'stratified', 'n_samples': 8, 'perturb': False},
                            hierarchical_sampling_config={'type': 'hierarchical', 'n_samples': 8}, model_config={'d_filter': 64})
    with pytest.raises(ValueError, match='ThompsonScattering'):
        render_columns(th, torch.zeros(2, dtype=torch.float64), torch.zeros(3, dtype=torch.float64), 0.0)


def test_exported_symbols():
    import sunerf_hip
    assert {'sunerf_column_rays', 'sunerf_column_stats'} <= set(sunerf_hip.symbols('core'))


def test_loader_axes_and_time(monkeypatch):
    """The loader's map / profile methods hand render_columns the pixel-centre axes (both ends included, radians), the
    normalised time and the per-column arrays of an arc."""
    from sunerf.evaluation import loader as L
    seen = {}

    def fake(rendering, lat, lon, time, r_range, n_samples, wavelengths, tile_rays, profiles=False, grid=True):
        seen.update(lat=lat.cpu(), lon=lon.cpu(), time=time, r_range=r_range, n_samples=n_samples, wl=wavelengths,
                    tile=tile_rays, profiles=profiles, grid=grid)
        return {'image': torch.zeros(lat.shape[0], lon.shape[0] if grid else 1)}
    monkeypatch.setattr(L, 'render_columns', fake)
    ld = L.SuNeRFLoader.__new__(L.SuNeRFLoader)
    ld.device, ld.rendering = torch.device('cpu'), None
    ld.seconds_per_dt, ld.ref_time = 86400., datetime.datetime(2022, 1, 1)
    out = ld.render_heliographic_map(datetime.datetime(2022, 1, 2, 12), shape=(5, 9), n_samples=64)
    assert out['image'].shape == (5, 9) and isinstance(out['image'], np.ndarray)
    assert seen['time'] == 1.5 and seen['grid'] and not seen['profiles'] and seen['n_samples'] == 64 and seen['tile'] is None
    assert seen['lat'].dtype == torch.float64 and torch.equal(seen['lat'], torch.from_numpy(np.linspace(-np.pi / 2, np.pi / 2, 5)))
    assert seen['lon'][0] == -np.pi and seen['lon'][-1] == np.pi and seen['lon'].shape == (9,)
    ld.render_radial_profile(np.linspace(0.1, 0.3, 4), np.full(4, 0.2), datetime.datetime(2022, 1, 1), r_range=(1.0, 1.2))
    assert not seen['grid'] and seen['profiles'] and seen['time'] == 0.0 and seen['r_range'] == (1.0, 1.2)
    assert seen['lat'].shape == seen['lon'].shape == (4,)
    ml = L.ModelLoader.__new__(L.ModelLoader)
    ml.device, ml.rendering = torch.device('cpu'), None
    ml.render_heliographic_map(0.25, shape=3, wl=np.array([171, 193]), batch_size=100)
    assert seen['time'] == 0.25 and seen['tile'] == 100 and seen['wl'].tolist() == [171., 193.]
    assert seen['lat'].shape == seen['lon'].shape == (3,)
