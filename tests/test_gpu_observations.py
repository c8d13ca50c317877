"""GPU checks of the training-set builder: ``sunerf_build_ray_pool`` / ``sunerf_hip.observations`` against the
reference's rays (fixture g8), against ``grid_rays`` + the numpy restatement bit for bit, across shards, epochs, files, the
state file and one short training run."""
import datetime

import numpy as np
import pytest
import torch

import observations_reference as ref
from conftest import load_golden

pytestmark = pytest.mark.gpu

WL7 = [94., 131., 171., 193., 211., 304., 335.]


def _ulp_close(a, b, what):
    """The criterion tests/test_gpu_frame.py applies to ``grid_rays``: fp32 results of fp64 sin / cos -- the device library and
    glibc may differ in the last fp64 bit, which can flip a rounding to fp32 -- at most 1 ulp, on at most 1 % of the elements;
    everything else bit-exact."""
    a, b = a.cpu(), b.cpu()
    assert a.shape == b.shape, (what, a.shape, b.shape)
    diff = (a - b).abs()
    ulp = torch.finfo(torch.float32).eps * b.abs().clamp_min(1e-30)
    assert (diff <= 2 * ulp).all(), (what, diff.max().item())
    assert (diff > 0).float().mean().item() <= 0.01, (what, (diff > 0).float().mean().item())


def _bits(x):
    x = x.detach().cpu().numpy() if isinstance(x, torch.Tensor) else np.asarray(x)
    return np.ascontiguousarray(x, dtype=np.float32).view(np.int32)


def _same_bits(got, want, what):
    g, w = _bits(got), _bits(want)
    assert g.shape == w.shape, (what, g.shape, w.shape)
    assert np.array_equal(g, w), (what, int((g != w).sum()), g.size)


@pytest.mark.parametrize('grid', ['axis', 'pix'])
def test_pool_rays_match_reference_get_rays(grid):
    from sunerf_hip.observations import ObservationSet
    g = load_golden('g8_observer_rays')
    tx, ty = g[f'tx_{grid}'].double(), g[f'ty_{grid}'].double()
    height, width = (tx.shape if tx.dim() == 2 else (ty.shape[0], tx.shape[0]))
    for name in ('a', 'b'):
        theta, phi, radius, sx, sy, sz, has_shift = [float(v) for v in g[f'pose_{name}']]
        obs = ObservationSet(device='cuda')
        obs.add_view(torch.zeros(height, width), lat=phi, lon=-theta, distance=radius, time=0.25, tx=tx, ty=ty,
                     center=(sx, sy, sz) if has_shift else None)
        pool = obs.pool(batch_size=64, seed=11)
        n = height * width
        assert pool.n_rays == n and pool.data['rays'].shape == (n, 2, 3)
        pixel = torch.from_numpy(ref.permutation(np.arange(n), n, 11, 0))       # slot -> pixel: undo the shuffle
        rays = torch.empty(n, 2, 3)
        rays[pixel] = pool.data['rays'].cpu()
        assert torch.equal(rays[:, 0], g[f'rays_o_{name}_{grid}'].reshape(-1, 3))
        _ulp_close(rays[:, 1], g[f'rays_d_{name}_{grid}'].reshape(-1, 3), (name, grid))
        assert (pool.data['time'] == 0.25).all() and 'wavelength' not in pool.data


def _record_views(device='cuda'):
    """Six views of different shapes, plate scales and channel sets: an odd size, a 1 x 1 view, a downscale-2 view, a
    3-of-7-channel view with per-pixel angles, a view with NaN / Inf pixels, a downscale-3 view with a non-finite block."""
    rng = np.random.default_rng(5)

    def planes(c, h, w):
        return (rng.uniform(0.0, 2.0, size=(c, h, w)) * 10.0 ** rng.integers(-3, 4, size=(c, h, w))).astype(np.float32)
    views = []
    views.append(dict(planes=planes(7, 37, 53), wavelengths=WL7, downscale=1, lat=0.1, lon=0.3, distance=215.0, time=0.0,
                      grid={'shape': (37, 53), 'cdelt': (60., 80.)}))
    views.append(dict(planes=planes(1, 1, 1), wavelengths=[0, 0, 171., 0, 0, 0, 0], downscale=1, lat=-0.2, lon=1.3,
                      distance=200.0, time=0.5, grid={'shape': (1, 1), 'cdelt': (2400., 2400.)}))
    views.append(dict(planes=planes(7, 24, 40), wavelengths=WL7, downscale=2, lat=0.0, lon=2.0, distance=215.0, time=1.25,
                      grid={'shape': (24, 40), 'cdelt': (100., 100.), 'crpix': (19.0, 11.5), 'crval': (30., -20.)}))
    ax, ay = np.linspace(-4e-3, 5e-3, 9), np.linspace(-6e-3, 6e-3, 16)
    tx = ax[None, :] + 1e-5 * ay[:, None] ** 2 * 1e3
    ty = ay[:, None] - 2e-2 * ax[None, :] + 0 * tx
    views.append(dict(planes=planes(3, 16, 9), wavelengths=[0, 131., 0, 193., 211., 0, 0], downscale=1, lat=0.3, lon=-0.8,
                      distance=150.0, time=-0.75, tx=np.ascontiguousarray(tx), ty=np.ascontiguousarray(ty),
                      center=(0.01, -0.02, 0.03)))
    nan_planes = planes(2, 20, 31)
    nan_planes[0, 3, 4] = np.nan
    nan_planes[1, 3, 4] = np.nan
    nan_planes[1, 19, 30] = np.nan
    nan_planes[0, 0, 0] = np.inf
    nan_planes[1, 7, 7] = -np.inf
    views.append(dict(planes=nan_planes, wavelengths=[94., 0, 0, 0, 0, 0, 335.], downscale=1, lat=-0.1, lon=3.0, distance=215.0,
                      time=2.0, grid={'shape': (20, 31), 'cdelt': (110., 110.)}))
    block = planes(7, 9, 12)
    block[2, 4, 7] = np.nan                                        # inside block (1, 2) of the 3 x 4 reduced frame
    views.append(dict(planes=block, wavelengths=WL7, downscale=3, lat=0.2, lon=-2.0, distance=215.0, time=3.0,
                      grid={'shape': (9, 12), 'cdelt': (200., 200.)}))
    return views


N_NONFINITE = 4 + 1          # the NaN / Inf pixels of view 4 (two NaNs share a pixel) + one block of view 5


def _observation_set(views, device_images=True):
    from sunerf_hip.observations import ObservationSet
    obs = ObservationSet(device='cuda')
    for v in views:
        image = torch.from_numpy(v['planes'])
        kw = {k: v[k] for k in ('grid', 'tx', 'ty', 'center') if k in v}
        obs.add_view(image.cuda() if device_images else image, v['lat'], v['lon'], v['distance'], v['time'],
                     wavelengths=v['wavelengths'], downscale=v['downscale'], **kw)
    return obs


def _with_grid_rays(obs, views):
    """The restatement's inputs: every view's rays in pixel order from ``grid_rays`` (pinned to the reference by g8)."""
    from sunerf_hip.rays import grid_rays
    out = []
    for v, ov in zip(views, obs.views):
        o, d = grid_rays(ov.tx, ov.ty, ov.c2w)
        out.append(dict(v, rays_o=o.cpu().numpy(), rays_d=d.cpu().numpy(), time=ov.time))
    return out


@pytest.mark.parametrize('drop', [True, False])
def test_every_record_equals_grid_rays_plus_restatement(drop):
    views = _record_views()
    obs = _observation_set(views)
    pool = obs.pool(batch_size=100, seed=3, drop_nonfinite=drop)
    want = ref.assemble(_with_grid_rays(obs, views), None, 3, 0, drop_nonfinite=drop)
    total = sum(v.n_pixels for v in obs.views)
    assert total == 37 * 53 + 1 + 12 * 20 + 16 * 9 + 20 * 31 + 3 * 4
    assert pool.total_rays == want['n_valid'] == (total - N_NONFINITE if drop else total)
    for key in ('rays', 'time', 'target_image', 'wavelength'):      # every record of every array: nothing is left out
        assert pool.data[key].shape[0] == pool.total_rays
        if drop:
            _same_bits(pool.data[key], want[key], key)
        else:       # NaN payloads of a block MEAN are not pinned (a copied pixel's are): compare NaN positions + all other bits
            got, exp = pool.data[key].cpu().numpy(), want[key]
            block_nan = np.isnan(exp) & (np.repeat(want['pixels'], exp[0].size).reshape(exp.shape) >= total - 12)
            assert np.array_equal(np.isnan(got), np.isnan(exp))
            _same_bits(np.where(block_nan, 0, got), np.where(block_nan, 0, exp), key)
    if drop:
        assert torch.isfinite(pool.data['target_image']).all()
        # exactly the non-finite pixels are gone, nothing else
        everything = ref.assemble(_with_grid_rays(obs, views), None, 3, 0, drop_nonfinite=False, permute=False)
        bad = ~np.isfinite(everything['target_image']).all(1)
        assert bad.sum() == N_NONFINITE
        assert np.array_equal(np.sort(want['pixels']), np.nonzero(~bad)[0])
    # host images give the same pool
    host = _observation_set(views, device_images=False).pool(batch_size=100, seed=3, drop_nonfinite=drop)
    for key in pool.data:
        assert np.array_equal(_bits(host.data[key]), _bits(pool.data[key])), key


def test_shards_epochs_and_reruns():
    views = _record_views()
    obs = _observation_set(views)
    whole = obs.pool(batch_size=128, seed=9)
    ranks = [obs.pool(batch_size=128, rank=r, world=4, seed=9) for r in range(4)]
    assert sum(p.n_rays for p in ranks) == whole.n_rays and [p.begin for p in ranks] == sorted(p.begin for p in ranks)
    for key in whole.data:
        _same_bits(torch.cat([p.data[key] for p in ranks]), whole.data[key], key)
    again = obs.pool(batch_size=128, seed=9)
    for key in whole.data:
        _same_bits(again.data[key], whole.data[key], key)
    # reshuffle='rays': epoch 1 is another order of the same records
    pool = obs.pool(batch_size=128, seed=9, reshuffle='rays')

    def rows(p):
        flat = np.concatenate([_bits(p.data[k]).reshape(p.n_rays, -1) for k in ('rays', 'time', 'target_image', 'wavelength')], 1)
        return flat, flat[np.lexsort(flat.T[::-1])]
    first = [{k: v.clone() for k, v in b.items()} for b in pool]                       # epoch 0
    assert len(first) == len(pool) == -(-pool.n_rays // 128) and pool.epoch == 1
    _same_bits(torch.cat([b['rays'] for b in first]), whole.data['rays'], 'epoch 0 = key (seed, 0)')
    flat0, sorted0 = rows(whole)
    second = list(pool)                                                               # epoch 1: rebuilt in place
    flat1, sorted1 = rows(pool)
    assert pool.built_epoch == 1 and pool.epoch == 2
    assert np.array_equal(sorted0, sorted1) and (flat0 != flat1).any(1).mean() > 0.9
    want = ref.assemble(_with_grid_rays(obs, views), None, 9, 1)
    _same_bits(torch.cat([b['target_image'] for b in second]), want['target_image'], 'epoch 1 = key (seed, 1)')
    # reshuffle='batches' keeps RayPool's semantics: fixed batches, fresh batch order
    fixed = obs.pool(batch_size=128, seed=9, reshuffle='batches')
    assert not np.array_equal(fixed.order(0), fixed.order(1)) and sorted(fixed.order(0)) == list(range(len(fixed)))
    e0 = list(fixed)
    assert torch.equal(e0[0]['rays'], fixed.batch(int(fixed.order(0)[0]))['rays'])
    with pytest.raises(ValueError):
        obs.pool(batch_size=128, reshuffle='pixels')


def test_pool_leaves_device_images_on_the_device(monkeypatch):
    """Counted, not profiled: during ``pool()`` every ``.cpu()`` / ``.numpy()`` / ``.tolist()`` / ``.to(<host>)`` of a device tensor
    is recorded through wrappers on ``torch.Tensor``; only scalars (the count of valid pixels) may cross."""
    views = _record_views()
    obs = _observation_set(views)
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
    for name in ('cpu', 'numpy', 'tolist', 'to'):
        counted(name)
    pool = obs.pool(batch_size=64, seed=1)
    list(obs.pool(batch_size=64, seed=1, reshuffle='rays'))
    monkeypatch.undo()
    assert pool.n_rays > 0 and all(n <= 1 for _, n in crossed), crossed
    assert all(v.is_cuda for v in pool.data.values())
    # (the wrappers do see a copy: the positive control)
    counted('cpu')
    pool.data['rays'].cpu()
    monkeypatch.undo()
    assert crossed[-1] == ('cpu', pool.n_rays * 6)


def test_written_files_feed_raypool_like_the_pool(tmp_path):
    from sunerf_hip.feed import RayPool
    views = _record_views()
    obs = _observation_set(views)
    obs.hold_out('reference')                      # 6 // 6: view 1 stays out of the files
    paths = obs.write_npy(str(tmp_path / 'work'), seed=4, chunk_rays=1000)       # several ragged chunks
    assert {k: p.split('/')[-1] for k, p in paths.items()} == {
        'rays': 'rays_batches.npy', 'time': 'times_batches.npy', 'target_image': 'images_batches.npy',
        'wavelength': 'wavelengths_batches.npy'}
    pool = obs.pool(batch_size=96, seed=4, reshuffle='batches')
    files = RayPool.from_files(paths, batch_size=96, seed=4, device='cuda')
    assert np.load(paths['rays']).shape == (pool.total_rays, 2, 3) and np.load(paths['time']).shape == (pool.total_rays, 1)
    assert np.load(paths['target_image']).shape == (pool.total_rays, 7) and len(files) == len(pool)
    assert pool.total_rays == sum(v.n_pixels for v in obs.views) - 1 - N_NONFINITE
    for epoch in range(2):
        assert np.array_equal(files.order(epoch), pool.order(epoch))
    for a, b in zip(files, pool):
        assert a.keys() == b.keys()
        for key in a:
            _same_bits(a[key], b[key], key)


def _disk_and_corona(rays_o, rays_d):
    b = torch.linalg.cross(rays_o, rays_d).norm(dim=-1) / rays_d.norm(dim=-1)              # impact parameter in solar radii
    return torch.where(b < 1, 0.25 * torch.sqrt((1 - b * b).clamp_min(0)) + 0.06, 0.06 * torch.exp(-(b - 1) / 0.12))


def _emission_set(resolution, n_views=7):
    """Single-channel views of an analytic target (limb-darkened disk + exponential corona) from ``n_views`` longitudes."""
    from sunerf.evaluation.loader import linear_plate_scale_axes
    from sunerf_hip.observations import ObservationSet
    from sunerf_hip.rays import grid_rays, pose_spherical
    obs = ObservationSet(Rs_per_ds=1.0, seconds_per_dt=86400.0, device='cuda', wavelength=193)
    grid = {'shape': (resolution, resolution), 'cdelt': (2400. / resolution, 2400. / resolution)}
    t0 = datetime.datetime(2022, 1, 1)
    for k in range(n_views):
        lat, lon, dist = 0.1 * (k % 3 - 1), 0.3 - 0.785 * k, 215.032
        tx, ty = linear_plate_scale_axes(grid, None, 'cuda')
        o, d = grid_rays(tx, ty, pose_spherical(-lon, lat, dist))
        obs.add_view(_disk_and_corona(o, d).reshape(resolution, resolution), lat, lon, dist,
                     time=t0 + datetime.timedelta(hours=8 * k), grid=grid)
    obs.hold_out('reference')
    return obs


def _emission_module():
    from sunerf.model.sunerf import EmissionSuNeRFModule
    torch.manual_seed(2)
    return EmissionSuNeRFModule(Rs_per_ds=1.0, seconds_per_dt=86400.0, image_scaling_config={'vmax': 1, 'a': 0.005},
                                sampling_config={'type': 'stratified', 'n_samples': 32, 'perturb': False},
                                hierarchical_sampling_config={'type': 'hierarchical', 'n_samples': 32, 'perturb': False},
                                model_config={'d_filter': 64}, lr_config={'start': 5e-4, 'end': 5e-5, 'iterations': 60}).cuda()


def test_state_file_renders_the_held_out_views_rays(tmp_path, monkeypatch):
    from sunerf.evaluation.loader import SuNeRFLoader
    from sunerf.model.sunerf import save_state
    monkeypatch.setenv('SUNERF_FORWARD_PRECISION', 'exact')
    obs = _emission_set(14)
    module = _emission_module()
    path = str(tmp_path / 'run' / 'save_state.snf')
    save_state(module, obs, path)
    loader = SuNeRFLoader(path, device='cuda')
    assert loader.ref_time == obs.ref_time and loader.wcs == obs.config['wcs'] and loader.wavelength == 193
    (val,) = obs.validation_batches(batch_size=50)
    held = obs.views[val['index']]
    assert val['index'] == 1 and val['image_shape'] == (14, 14) and len(val['batches']) == 4
    frame = loader.render_observer_image(held.lat, held.lon, held.raw_time, distance=held.distance, as_numpy=False,
                                         batch_size=77)
    outputs = [module.validation_step(batch, i) for i, batch in enumerate(val['batches'])]
    module.validation_dataset_mapping = {0: 'test_image'}
    module.validation_epoch_end(outputs)
    stored = module.validation_outputs['test_image']
    assert frame['fine_image'].shape[:2] == (14, 14)
    for key in ('fine_image', 'coarse_image', 'height_map', 'absorption_map'):
        assert torch.equal(torch.nan_to_num(frame[key].reshape(stored[key].shape)), torch.nan_to_num(stored[key])), key
    _same_bits(stored['target_image'].reshape(14, 14), held.image[0], 'held-out target in pixel order')
    scores = module.validation_metrics(val['image_shape'])
    assert set(scores) == {'validation.loss', 'validation.ssim', 'validation.psnr'} and all(torch.isfinite(v) for v in scores.values())


def test_pool_feeds_fit_steps():
    """Only that the pool feeds the step (the step itself is covered elsewhere): finite losses that go down."""
    from sunerf.model.sunerf import fit_steps
    from sunerf_hip.feed import training_batches
    obs = _emission_set(48)
    module = _emission_module()
    pool = obs.pool(batch_size=1024, seed=0, reshuffle='rays')
    assert pool.n_rays == 6 * 48 * 48
    losses = torch.stack(fit_steps(module, training_batches(pool, 60))).cpu()
    assert losses.shape == (60,) and torch.isfinite(losses).all()
    first, last = losses[:20].mean().item(), losses[-20:].mean().item()
    print(f'mean loss of steps 0-19: {first:.5f}, of steps 40-59: {last:.5f}')
    assert last < first, (first, last)
