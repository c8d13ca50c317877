"""GPU checks of the reprojection baseline: ``sunerf_synchronic_map`` / ``sunerf_map_fill`` /
``sunerf_reproject_views`` and ``sunerf_hip.reprojection`` against the numpy restatement (tests/reprojection_reference.py) --
coordinates, every value of every pixel, coverage counts, the fill, exact cases, shards, the ``ObservationSet`` methods, one
analytic scene and a randomised sweep.  The inputs' decision margins are asserted in tests/test_reprojection_host.py, which is
why nothing is left out of the fixed cases."""
import datetime

import numpy as np
import pytest
import torch

import metrics_reference
import reprojection_reference as ref

pytestmark = pytest.mark.gpu

N_RANDOM_CASES = 24
LEAVE_OUT_CAP = 1e-4


def _np(t):
    return t.detach().cpu().numpy()


def _bits(x):
    x = _np(x) if isinstance(x, torch.Tensor) else np.asarray(x)
    return np.ascontiguousarray(x, dtype=np.float32).view(np.int32)


def _device_axes(lat, lon):
    return torch.from_numpy(lat).cuda(), torch.from_numpy(lon).cuda()


def _value_bound(res, delta):
    """ulp_fp32(max |tap|) + 2 delta (max tap - min tap): fp64 interpolation of identical fp32 taps with weights ``delta`` apart,
    then one rounding on each side.  Only read where the restatement's value is finite (then every tap is)."""
    with np.errstate(invalid='ignore'):
        ulp = np.spacing(res['tap_max'].astype(np.float32)).astype(np.float64)
        return ulp + 2.0 * delta * (res['tap_hi'] - res['tap_lo'])


def _check_values(got, want, bound, what, keep=None):
    """NaN positions equal, +-Inf equal, finite values within ``bound``; ``keep``: the samples compared (default: all)."""
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    keep = np.ones(want.shape, dtype=bool) if keep is None else np.broadcast_to(keep, want.shape)
    nan = np.isnan(want)
    assert np.array_equal(np.isnan(got)[keep], nan[keep]), (what, 'NaN positions', int((np.isnan(got) != nan)[keep].sum()))
    inf = np.isinf(want) & keep
    assert np.array_equal(got[inf], want[inf]), (what, 'infinities')
    fin = np.isfinite(want) & keep
    err = np.abs(got[fin] - want[fin])
    worst = float((err / bound[fin]).max()) if fin.any() else 0.0
    print(f'{what}: {int(fin.sum())} finite values, {int((err > 0).sum())} differ, worst error / bound {worst:.3f}')
    assert worst <= 1.0, (what, worst)


def _coordinate_check(got, want, wide, n_x, n_y, what, keep=None):
    """``got`` (device fp64) against the restatement ``want``; the bound from the restatement's noise against ``wide``."""
    noise = max(ref.coordinate_noise(want[k], wide[k]) for k in (0, 1))
    bound = ref.coordinate_bound(noise, n_x, n_y)
    worst = 0.0
    for k in (0, 1):
        g, w = np.asarray(got[k]), np.asarray(want[k], dtype=np.float64)
        sel = np.ones(w.shape, dtype=bool) if keep is None else keep
        assert np.array_equal(np.isnan(g)[sel], np.isnan(w)[sel]), (what, 'NaN coordinates')
        fin = np.isfinite(w) & sel
        if fin.any():
            worst = max(worst, float(np.abs(g[fin] - w[fin]).max()))
    floor = '' if ref.LONG_DOUBLE_IS_WIDER else ' (long double is no wider than fp64 here: the floor alone applies)'
    print(f'{what}: max |device - restatement| {worst:.2e} pixels, restatement noise {noise:.2e}, bound {bound:.2e}{floor}')
    assert worst <= bound, (what, worst, bound)
    return bound


@pytest.fixture(scope='module')
def fixed():
    obs, views = ref.observation_set(ref.view_specs(), 'cuda')
    return obs, views


# ------------------------------------------------------------------------------------------------------ the map kernel
@pytest.mark.parametrize('name', list(ref.MAPS))
def test_view_coordinates_and_margin(fixed, name):
    from sunerf_hip.reprojection import map_rows
    obs, views = fixed
    lat, lon = ref.map_axes(name)
    points, wide = ref.column_points(lat, lon, 1.0), ref.column_points(lat, lon, 1.0, np.longdouble)
    for k, (ov, v) in enumerate(zip(obs.views, views)):
        image, footprint, coords = map_rows([ov], *_device_axes(lat, lon), want_coords=True)
        coords = _np(coords)
        x, y, margin = ref.view_coords(v, points, 1.0)
        xw, yw, _ = ref.view_coords(v, wide, 1.0, np.longdouble)
        _coordinate_check(coords[:2], (x, y), (xw, yw), len(v['tx']), len(v['ty']), f'map {name} view {k}')
        assert np.array_equal(coords[2] > 0, margin > 0)                       # the visibility decision, every pixel
        assert np.abs(coords[2] - margin).max() <= 1e-12 * np.abs(margin).max()


@pytest.mark.parametrize('name', list(ref.MAPS))
def test_map_values_footprint_and_fill(fixed, name):
    from sunerf_hip.reprojection import map_rows, synchronic_map
    obs, views = fixed
    lat, lon = ref.map_axes(name)
    want = ref.synchronic_map(views, lat, lon, 1.0)
    points, wide = ref.column_points(lat, lon, 1.0), ref.column_points(lat, lon, 1.0, np.longdouble)
    delta = 0.0
    for v in views:                                                             # the coordinate bound of the worst view
        c64, cw = ref.view_coords(v, points, 1.0), ref.view_coords(v, wide, 1.0, np.longdouble)
        delta = max(delta, ref.coordinate_bound(max(ref.coordinate_noise(c64[k], cw[k]) for k in (0, 1)), len(v['tx']), len(v['ty'])))
    image, footprint = map_rows(obs.views, *_device_axes(lat, lon))
    assert np.array_equal(_np(footprint), want['footprint'])                    # every pixel, every channel
    assert (want['footprint'] > 0).sum() > 0.3 * want['footprint'].size and want['footprint'].max() >= 2
    _check_values(_np(image), want['map'], _value_bound(want, delta), f'map {name}')
    # the fill: None leaves exactly the uncovered pixels NaN, 'mean' and a number fill exactly those
    m = ref.MAPS[name]
    raw = synchronic_map(obs.views, fill=None, **m)
    assert np.array_equal(_bits(raw.image), _bits(image)) and np.array_equal(_np(raw.footprint), want['footprint'])
    assert np.array_equal(np.isnan(_np(raw.image)), np.isnan(want['map']))
    _, mean, count = ref.fill(_np(image))
    assert raw.covered_fraction == count.sum() / want['map'].size
    filled = synchronic_map(obs.views, fill='mean', **m)
    assert filled.covered_fraction == raw.covered_fraction
    got_fill = _np(filled.fill_value)
    for c in range(7):
        hole = np.isnan(_np(image)[c])
        if not hole.any():                                                      # (a channel the views cover completely)
            assert np.array_equal(_bits(_np(filled.image)[c]), _bits(_np(image)[c]))
            continue
        value = _np(filled.image)[c][hole]
        assert (value == value[0]).all() or np.isnan(value).all()
        if np.isfinite(mean[c]):
            assert abs(np.float64(value[0]) - mean[c]) <= np.spacing(np.float32(abs(mean[c]))), (c, value[0], mean[c])
            assert abs(got_fill[c] - mean[c]) <= 1e-12 * abs(mean[c])
        else:
            assert value[0] == np.float32(mean[c]) or (np.isnan(value[0]) and np.isnan(mean[c]))
        assert np.array_equal(_bits(_np(filled.image)[c][~hole]), _bits(_np(image)[c][~hole]))
    assert np.isnan(_np(image)).any()
    number = synchronic_map(obs.views, fill=-2.5, **m)
    assert np.array_equal(_np(number.image) == -2.5, np.isnan(_np(image))) and number.covered_fraction == raw.covered_fraction
    print(f'map {name}: covered fraction {raw.covered_fraction:.4f}, fill values {got_fill}')


def test_fill_entry_point_modes():
    """``sunerf_map_fill`` through the C ABI: statistics only, mean, number; all-NaN and NaN-free channels."""
    from sunerf_hip import lib as _l
    from sunerf_hip.ops import _ptr, _stream
    rng = np.random.default_rng(3)
    host = rng.uniform(0.5, 1.5, size=(3, 123, 457)).astype(np.float32)
    host[0][rng.random(host[0].shape) < 0.4] = np.nan
    host[1] = np.nan
    stats_want = ref.fill(host)
    ws = torch.empty(int(_l.load().sunerf_map_fill_workspace_bytes(3)), dtype=torch.uint8, device='cuda')
    for mode, value, fill in ((0, 0.0, None), (1, 0.0, 'mean'), (2, 7.0, 7.0)):
        image = torch.from_numpy(host).cuda()
        stats = torch.empty(3, 2, dtype=torch.float64, device='cuda')
        _l.call(image.device, 'sunerf_map_fill', _ptr(image), 3, 123 * 457, mode, value, _ptr(stats), _ptr(ws), ws.numel(),
                _stream(image.device))
        want, mean, count = ref.fill(host, fill)
        got, s = _np(image), _np(stats)
        assert np.array_equal(s[:, 1], count) and np.isnan(s[1, 0]) and count[1] == 0 and count[2] == 123 * 457
        assert abs(s[0, 0] - mean[0]) <= 1e-12 * mean[0] and abs(s[2, 0] - mean[2]) <= 1e-12 * mean[2]
        assert np.array_equal(np.isnan(got), np.isnan(want))
        ok = ~np.isnan(want)
        assert (np.abs(got[ok].astype(np.float64) - want[ok]) <= np.spacing(np.abs(want[ok]))).all()
        assert np.array_equal(_bits(got[2]), _bits(host[2]))                    # a channel without NaNs is untouched
    assert stats_want[2][0] > 0


# ------------------------------------------------------------------------------------------------ the view kernel
@pytest.mark.parametrize('name', list(ref.MAPS))
def test_observer_coordinates_and_values(fixed, name):
    from sunerf_hip.reprojection import synchronic_map
    obs, views = fixed
    lat, lon = ref.map_axes(name)
    h_map = synchronic_map(obs.views, fill=None, **ref.MAPS[name])              # NaN holes stay: they must propagate
    image = _np(h_map.image)
    for oname, specs in ref.observer_specs().items():
        images, coords = h_map.reproject_many(specs, want_coords=True)
        coords = _np(coords)
        begin, delta = 0, 0.0
        for spec, got in zip(specs, images):
            o = ref.observer_dict(spec)
            n = len(o['tx']) * len(o['ty'])
            x, y, mrel, on_disk = ref.observer_coords(o, lat, lon, 1.0)
            xw, yw, _, _ = ref.observer_coords(o, lat, lon, 1.0, np.longdouble)
            mine = coords[:, begin:begin + n].reshape(3, *x.shape)
            quiet = oname == 'grid' and begin > 0
            noise = max(ref.coordinate_noise(x, xw), ref.coordinate_noise(y, yw))
            bound = ref.coordinate_bound(noise, len(lon), len(lat))
            for k, w in enumerate((x, y)):
                assert np.array_equal(np.isnan(mine[k]), np.isnan(w)), (name, oname, begin)
                fin = np.isfinite(w)
                assert not fin.any() or np.abs(mine[k][fin] - w[fin]).max() <= bound, (name, oname, begin, bound)
            if not quiet:
                _coordinate_check(mine[:2], (x, y), (xw, yw), len(lon), len(lat), f'map {name} observer {oname}')
            assert np.array_equal((mine[2] > 0), (mrel > 0))
            want = ref.reproject(image, lat, lon, 1.0, o)
            assert got.shape == want['image'].shape
            if quiet:
                _check_quietly(_np(got), want, bound)
            else:
                _check_values(_np(got), want['image'], _value_bound(want, bound), f'map {name} observer {oname}')
            assert np.isnan(_np(got)[~on_disk]).all()
            begin += n
        # off_disk= fills the pixels off the disk and nothing else; pixels outside the map's axes stay NaN
        zero = h_map.reproject_many(specs[:1], off_disk=0.0)[0]
        o = ref.observer_dict(specs[0])
        on_disk = ref.observer_coords(o, lat, lon, 1.0)[3]
        assert (_np(zero)[~on_disk] == 0).all()
        assert np.array_equal(_bits(_np(zero)[on_disk]), _bits(_np(images[0])[on_disk]))


def _check_quietly(got, want, delta):
    bound = _value_bound(want, delta)
    w = want['image'].astype(np.float64)
    assert np.array_equal(np.isnan(got), np.isnan(w))
    inf = np.isinf(w)
    assert np.array_equal(got[inf], w[inf])
    fin = np.isfinite(w)
    assert (np.abs(got[fin].astype(np.float64) - w[fin]) <= bound[fin]).all()


# ---------------------------------------------------------------------------------------------------------- exact cases
def test_constant_views_give_a_constant_map_and_views():
    from sunerf_hip.reprojection import synchronic_map
    c = np.float32(0.3712)
    specs = [dict(v, planes=np.full_like(v['planes'], c)) for v in ref.view_specs()]
    obs, _ = ref.observation_set(specs, 'cuda')
    lat, lon = ref.map_axes('full')
    h_map = synchronic_map(obs.views, fill=None, **ref.MAPS['full'])
    image, footprint = _np(h_map.image), _np(h_map.footprint)
    assert (image[footprint > 0] == c).all() and np.isnan(image[footprint == 0]).all() and (footprint > 0).mean() > 0.3
    filled = synchronic_map(obs.views, fill='mean', **ref.MAPS['full'])
    assert (_np(filled.image) == c).all()                                      # the mean of a constant is the constant
    for oname in ('square', 'odd'):
        spec = ref.observer_specs()[oname][0]
        got = _np(filled.reproject_many([spec])[0])
        on_disk = ref.observer_coords(ref.observer_dict(spec), lat, lon, 1.0)[3]
        assert (got[on_disk] == c).all() and np.isnan(got[~on_disk]).all() and on_disk.any() and (~on_disk).any()


def test_a_view_seen_from_its_own_observer(fixed):
    from sunerf_hip.reprojection import synchronic_map
    obs, views = fixed
    for k in (0, 2, 4):
        lat, lon = ref.map_axes('full')
        h_map = synchronic_map([obs.views[k]], fill=None, **ref.MAPS['full'])
        got = _np(h_map.reproject_many([obs.views[k]])[0])
        v = views[k]
        want = ref.reproject(_np(h_map.image), lat, lon, 1.0, v)
        und = ref.observer_margins(v, _np(h_map.image), lat, lon, 1.0)[0]
        assert und.sum() == 0, (k, int(und.sum()))
        assert got.shape == (len(v['ty']), len(v['tx']), 7)
        assert np.array_equal(np.isnan(got), np.isnan(want['image']))
        assert np.isfinite(got).any()


def test_reruns_batches_and_shards_are_bit_identical(fixed):
    from sunerf_hip.dist import shard_range
    from sunerf_hip.reprojection import finish_map, map_rows, synchronic_map
    obs, _ = fixed
    m = ref.MAPS['full']
    first, second = synchronic_map(obs.views, **m), synchronic_map(obs.views, **m)
    assert np.array_equal(_bits(first.image), _bits(second.image)) and torch.equal(first.footprint, second.footprint)
    assert torch.equal(first.fill_value, second.fill_value) or bool(torch.isnan(first.fill_value).any())
    specs = ref.observer_specs()
    everyone = specs['square'] + specs['odd'] + specs['single'] + specs['grid'][:40]
    batch = first.reproject_many(everyone)
    again = first.reproject_many(everyone)
    for spec, a, b in zip(everyone, batch, again):
        alone = first.reproject(spec['lat'], spec['lon'], spec['distance'], tx=spec['tx'], ty=spec['ty'], center=spec.get('center'))
        assert np.array_equal(_bits(a), _bits(b)) and np.array_equal(_bits(a), _bits(alone))
    lat, lon = _device_axes(*ref.map_axes('full'))
    for world in (1, 2, 4):
        slabs = [map_rows(obs.views, lat, lon, 1.0, b, e - b) for b, e in (shard_range(91, r, world) for r in range(world))]
        image = torch.cat([s[0] for s in slabs], 1).contiguous()
        footprint = torch.cat([s[1] for s in slabs], 1).contiguous()
        whole = finish_map(image, footprint, lat, lon, 1.0, None)
        assert np.array_equal(_bits(whole.image), _bits(first.image)) and torch.equal(whole.footprint, first.footprint), world
        assert whole.covered_fraction == first.covered_fraction


# ------------------------------------------------------------------------------------------------------ through the set
def _set_of_four():
    specs = [ref.view_specs()[k] for k in (0, 2, 3, 4)]
    obs, views = ref.observation_set(specs, 'cuda')
    obs.hold_out('reference')                                                   # 4 // 6: view 0, 37 x 53 pixels, 7 channels
    return specs, obs, views


def test_baseline_of_the_held_out_view():
    specs, obs, views = _set_of_four()
    assert obs.held_out == [0] and obs.training_views == [1, 2, 3]
    m = ref.MAPS['full']
    lat, lon = ref.map_axes('full')
    pred = obs.baseline_view(**m)
    assert pred.shape == (37, 53, 7) and pred.is_cuda
    coadd = ref.synchronic_map(views[1:], lat, lon, 1.0)
    for v in views[1:]:
        assert ref.view_margins(v, lat, lon, 1.0)[0].sum() == 0
    filled, _, _ = ref.fill(coadd['map'])
    assert ref.observer_margins(views[0], filled, lat, lon, 1.0)[0].sum() == 0
    want = ref.reproject(filled, lat, lon, 1.0, views[0])
    differ = int((_bits(pred) != _bits(want['image'])).sum())
    print(f'baseline prediction: {differ} of {want["image"].size} values differ in bits from the restatement')
    assert np.array_equal(np.isnan(_np(pred)), np.isnan(want['image']))
    # the held-out image is not part of its own baseline
    obs.views[0].image.mul_(3.0).add_(1.0)
    assert np.array_equal(_bits(obs.baseline_view(**m)), _bits(pred))
    obs.views[0].image.sub_(1.0).div_(3.0)
    # scores: image_metrics of the restatement's prediction, to the tolerances tests/test_gpu_metrics.py holds image_metrics to
    p0 = torch.from_numpy(np.nan_to_num(want['image'].transpose(2, 0, 1), nan=0.0).copy()).cuda()
    for normalize in (None, lambda t: torch.asinh(t / 5.0)):                    # (the device's asinh on both sides)
        got = {k: _np(v) for k, v in obs.baseline_metrics(data_range=2000.0, normalize=normalize, **m).items()}
        p, t = (p0, obs.views[0].image) if normalize is None else (normalize(p0), normalize(obs.views[0].image))
        exp = metrics_reference.image_metrics(_np(p).astype(np.float64), _np(t).astype(np.float64), 2000.0)
        assert set(got) == {'ssim', 'mse', 'mae', 'me', 'psnr'} and got['ssim'].shape == (7,)
        print('baseline psnr per channel', got['psnr'], 'ssim', got['ssim'])
        assert np.abs(got['ssim'] - exp['ssim']).max() <= 1e-10
        for k in ('mse', 'mae', 'psnr'):
            np.testing.assert_allclose(got[k], exp[k], rtol=1e-12, atol=0, err_msg=k)
        np.testing.assert_allclose(got['me'], exp['me'], rtol=1e-9, atol=1e-15 * 2000.0)


def test_only_the_covered_count_crosses_to_the_host(monkeypatch):
    specs, obs, views = _set_of_four()
    m = ref.MAPS['full']
    obs.synchronic_map(**m)                                                     # (the axes' monotonicity is checked once per view)
    crossed = []

    def counted(name):
        original = getattr(torch.Tensor, name)

        def wrapper(self, *args, **kwargs):
            out = original(self, *args, **kwargs)
            to_host = name != 'to' or (isinstance(out, torch.Tensor) and not out.is_cuda)
            if self.is_cuda and to_host:
                crossed.append((name, self.numel()))
            return out
        monkeypatch.setattr(torch.Tensor, name, wrapper)
    for name in ('cpu', 'numpy', 'tolist', 'to', 'item'):
        counted(name)
    h_map = obs.synchronic_map(**m)
    view = h_map.reproject(0.2, 0.4, 215.0, grid={'shape': (32, 32), 'cdelt': (75., 75.)})
    pred = obs.baseline_view(**m)
    monkeypatch.undo()
    assert h_map.image.is_cuda and view.is_cuda and pred.is_cuda
    assert all(n <= 1 for _, n in crossed) and any(name == 'item' for name, _ in crossed), crossed
    counted('cpu')                                                              # (the wrappers do see a copy: the positive control)
    view.cpu()
    monkeypatch.undo()
    assert crossed[-1] == ('cpu', 32 * 32 * 7)


# ----------------------------------------------------------------------------------------------- sanity of the science
def _disk_and_corona(rays_o, rays_d):
    b = torch.linalg.cross(rays_o, rays_d).norm(dim=-1) / rays_d.norm(dim=-1)              # impact parameter in solar radii
    return torch.where(b < 1, 0.25 * torch.sqrt((1 - b * b).clamp_min(0)) + 0.06, 0.06 * torch.exp(-(b - 1) / 0.12))


def test_baseline_of_an_analytic_disk_and_corona():
    """The analytic target of tools/mini_train.py from 8 longitudes; the baseline of the held-out view is finite on the disk.  Its
    PSNR is printed, not judged: the surface assumption is supposed to be poor off the limb."""
    from sunerf.evaluation.loader import linear_plate_scale_axes
    from sunerf_hip.observations import ObservationSet
    from sunerf_hip.rays import grid_rays, pose_spherical
    n = 64
    obs = ObservationSet(device='cuda', wavelength=193)
    grid = {'shape': (n, n), 'cdelt': (2400. / n, 2400. / n)}
    t0 = datetime.datetime(2022, 1, 1)
    for k in range(8):
        lat, lon, dist = 0.1 * (k % 3 - 1), 0.3 - 0.785 * k, 215.032
        tx, ty = linear_plate_scale_axes(grid, None, 'cuda')
        o, d = grid_rays(tx, ty, pose_spherical(-lon, lat, dist))
        obs.add_view(_disk_and_corona(o, d).reshape(n, n), lat, lon, dist, time=t0 + datetime.timedelta(hours=k), grid=grid)
    obs.hold_out('reference')
    pred = obs.baseline_view(shape=(181, 361))
    held = obs.views[obs.held_out[0]]
    o = dict(tx=_np(held.tx), ty=_np(held.ty), c2w=held.c2w[:3, :4].numpy())
    _, mrel, on_disk = ref.surface_points(o, 1.0)
    assert pred.shape == (n, n, 1) and on_disk.sum() > 1000
    assert np.isfinite(_np(pred)[..., 0][on_disk]).all() and np.isnan(_np(pred)[..., 0][~on_disk]).all()
    scores = obs.baseline_metrics(shape=(181, 361))
    inner = mrel > 0.2
    err = np.abs(_np(pred)[..., 0] - _np(held.image[0]))[inner]
    print(f'analytic scene, held-out view {obs.held_out[0]}: baseline PSNR {scores["psnr"].item():.2f} dB, SSIM {scores["ssim"].item():.4f}, '
          f'max |error| inside mu^2 > 0.2: {err.max():.4f}')
    assert torch.isfinite(scores['psnr']).all()


# -------------------------------------------------------------------------------------------------- randomised sweep
@pytest.mark.parametrize('seed', range(N_RANDOM_CASES))
def test_random_case(seed):
    from sunerf_hip.reprojection import finish_map, map_rows
    case = ref.random_case(seed)
    obs, views = ref.observation_set(case['views'], 'cuda')
    radius = 1.0 / case['Rs_per_ds']
    m = case['map']
    lat = np.linspace(m['lat_range'][0], m['lat_range'][1], m['shape'][0])
    lon = np.linspace(m['lon_range'][0], m['lon_range'][1], m['shape'][1])
    points, wide = ref.column_points(lat, lon, radius), ref.column_points(lat, lon, radius, np.longdouble)
    left_out, delta = np.zeros(m['shape'], dtype=bool), 0.0
    for ov, v in zip(obs.views, views):
        und = ref.view_margins(v, lat, lon, radius)[0]
        left_out |= und
        _, _, coords = map_rows([ov], *_device_axes(lat, lon), Rs_per_ds=case['Rs_per_ds'], want_coords=True)
        c64, cw = ref.view_coords(v, points, radius), ref.view_coords(v, wide, radius, np.longdouble)
        delta = max(delta, _coordinate_check(_np(coords)[:2], c64[:2], cw[:2], len(v['tx']), len(v['ty']), f'case {seed} view', ~und))
    assert left_out.sum() <= LEAVE_OUT_CAP * left_out.size
    want = ref.synchronic_map(views, lat, lon, radius)
    image, footprint = map_rows(obs.views, *_device_axes(lat, lon), Rs_per_ds=case['Rs_per_ds'])
    assert np.array_equal(_np(footprint)[:, ~left_out], want['footprint'][:, ~left_out])
    _check_values(_np(image), want['map'], _value_bound(want, delta), f'case {seed} map', ~left_out[None])
    h_map = finish_map(image, footprint, *_device_axes(lat, lon), case['Rs_per_ds'], None, fill=None)
    o = ref.observer_dict(case['observer'])
    und = ref.observer_margins(o, _np(image), lat, lon, radius)[0]
    assert und.sum() <= LEAVE_OUT_CAP * und.size
    (got,), coords = h_map.reproject_many([case['observer']], want_coords=True)
    x, y, _, _ = ref.observer_coords(o, lat, lon, radius)
    xw, yw, _, _ = ref.observer_coords(o, lat, lon, radius, np.longdouble)
    bound = _coordinate_check(_np(coords)[:2].reshape(2, *x.shape), (x, y), (xw, yw), len(lon), len(lat), f'case {seed} observer', ~und)
    res = ref.reproject(_np(image), lat, lon, radius, o)
    _check_values(_np(got), res['image'], _value_bound(res, bound), f'case {seed} view', ~und[..., None])
    print(f'case {seed}: left out {int(left_out.sum())} map pixels, {int(und.sum())} observer pixels')


# ------------------------------------------------------------------------------------- load_views' grid and the mirror
def test_view_grid_and_the_mirror_module(fixed):
    import sunerf.baseline.reprojection as mirror
    from sunerf_hip.reprojection import synchronic_map, view_grid_coordinates
    obs, _ = fixed
    views = [obs.views[k] for k in (0, 2, 4)]                                   # the first view has a plate-scale grid
    h_map = synchronic_map(views, **ref.MAPS['full'])
    axis = np.linspace(-5e-3, 5e-3, 9)
    pairs = list(h_map.view_grid(30, 215.0, tx=axis, ty=axis, off_disk=0.0))
    coords = view_grid_coordinates(30)
    assert len(pairs) == 7 * 13 and [p[0] for p in pairs] == [(float(b), float(l)) for b, l in coords]
    for (b, l), image in pairs[::17]:
        alone = h_map.reproject(np.deg2rad(b), np.deg2rad(l), 215.0, tx=axis, ty=axis, off_disk=0.0)
        assert image.shape == (9, 9, 7) and np.array_equal(_bits(image), _bits(alone))
    # the reference's import path: the same map (at the reference's default shape) and the same views
    m = mirror.create_heliographic_map(*views)
    assert m.shape == (1024, 2048) and 0.3 < m.covered_fraction < 1.0 and not bool(torch.isnan(m.image[0]).any())
    small = mirror.create_heliographic_map(*views, shape_out=(91, 181))
    assert np.array_equal(_bits(small.image), _bits(h_map.image))
    v = views[0]
    seen = mirror.transform(*views, lat=v.lat, lon=v.lon, distance=v.distance)          # on the first view's own grid
    assert seen.shape == (37, 53, 7) and np.array_equal(_bits(seen), _bits(m.reproject_many([v])[0]))
    got = list(mirror.load_views(*views, strides=90, resolution=(8, 12)))
    assert len(got) == 3 * 5 and got[0][0] == (-90.0, 0.0) and all(image.shape == (8, 12, 7) for _, image in got)
    assert bool(torch.isfinite(got[7][1][4, 6, 0]))                                     # (lat 0, lon 180): disk centre
