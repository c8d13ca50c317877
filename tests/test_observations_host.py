"""CPU-only checks of the training-set builder: the numpy restatement of the keyed permutation and the record
assembly (tests/observations_reference.py), the host side of ``sunerf_hip.observations`` and the C entry point's argument
checks.  The kernel itself is compared with the restatement in tests/test_gpu_observations.py."""
import datetime
import os
import re

import numpy as np
import pytest
import torch

import observations_reference as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIZES = [1, 2, 3, 5, 64, 1000, 65537, 2 ** 20 + 1, 10 ** 6 + 3]
KEYS = [(0, 0), (1234567891011, 7)]


@pytest.fixture(scope='module')
def lib():
    import sunerf_hip
    if not os.path.exists(sunerf_hip.LIB_PATH):
        import subprocess
        subprocess.check_call(['bash', os.path.join(ROOT, '2024-hl-spi3s-sunerf_amd', 'csrc', 'build.sh')])
    return sunerf_hip.load()


@pytest.mark.parametrize('n', SIZES)
def test_permutation_is_a_bijection(n):
    for seed, epoch in KEYS:
        pi = ref.permutation(np.arange(n), n, seed, epoch)
        assert np.array_equal(np.sort(pi), np.arange(n)), (n, seed, epoch)


def test_epochs_and_seeds_give_different_permutations():
    n = 65537
    a, b, c = (ref.permutation(np.arange(n), n, s, e) for s, e in ((3, 0), (3, 1), (4, 0)))
    assert (a != b).mean() > 0.99 and (a != c).mean() > 0.99 and (b != c).mean() > 0.99
    assert np.array_equal(a, ref.permutation(np.arange(n), n, 3, 0))
    # a uniform permutation displaces an element by n / 3 on average
    assert abs(np.abs(a - np.arange(n)).mean() / n - 1 / 3) < 0.01
    # 64-bit keys: both words count
    assert not np.array_equal(ref.round_keys(1, 0), ref.round_keys(1 << 32, 0))
    assert not np.array_equal(ref.round_keys(0, 1), ref.round_keys(0, 1 << 32))


@pytest.mark.parametrize('world', [1, 2, 3, 8])
@pytest.mark.parametrize('n', [5, 1000, 65537])
def test_shards_are_disjoint_and_complete(n, world):
    from sunerf_hip.dist import shard_range
    parts = []
    for rank in range(world):
        begin, end = shard_range(n, rank, world)
        assert (begin, end) == ref.shard_range(n, rank, world)
        parts.append(ref.permutation(np.arange(begin, end), n, 5, 2))
    whole = np.concatenate(parts)
    assert whole.size == n and np.array_equal(np.sort(whole), np.arange(n))
    assert np.array_equal(whole, ref.permutation(np.arange(n), n, 5, 2))      # the shards are slices of ONE permutation


def test_pixel_decode_over_views_of_different_shapes():
    shapes = [(37, 53), (1, 1), (12, 20), (16, 9)]
    total = sum(h * w for h, w in shapes)
    view, row, col = ref.decode(np.arange(total), shapes)
    p = 0
    for k, (h, w) in enumerate(shapes):
        for r in (0, h - 1):
            for c in (0, w - 1):
                i = p + r * w + c
                assert (view[i], row[i], col[i]) == (k, r, c)
        p += h * w
    assert np.array_equal(np.bincount(view), [h * w for h, w in shapes])


def _observation_set(n_views=7):
    from sunerf_hip.observations import ObservationSet
    obs = ObservationSet(Rs_per_ds=1.0, seconds_per_dt=86400.0, device='cpu')
    t0 = datetime.datetime(2022, 3, 1)
    for k in range(n_views):
        obs.add_view(torch.zeros(4 + k, 6), lat=0.1 * k, lon=0.5 * k, distance=215.0, time=t0 + datetime.timedelta(hours=6 * k),
                     grid={'shape': (4 + k, 6), 'cdelt': (300., 300.)})
    return obs, t0


def test_descriptor_table_matches_the_decode():
    from sunerf_hip.observations import VIEW_DESC, view_descriptors
    obs, _ = _observation_set(5)
    rows, total = view_descriptors(obs.views)
    shapes = [(4 + k, 6) for k in range(5)]
    assert total == sum(h * w for h, w in shapes) and VIEW_DESC.itemsize == 232
    view, row, col = ref.decode(np.arange(total), shapes)
    for k in range(5):
        assert rows['pix_offset'][k] == np.nonzero(view == k)[0][0]
        assert (rows['height'][k], rows['width'][k], rows['downscale'][k], rows['per_pixel'][k]) == (4 + k, 6, 1, 0)
        assert rows['image'][k] == obs.views[k].image.data_ptr() and rows['tx'][k] == obs.views[k].tx.data_ptr()
        assert np.array_equal(rows['c2w'][k], obs.views[k].c2w[:3, :4].reshape(-1).numpy())
        assert rows['time'][k] == np.float32(0.25 * k) and rows['n_planes'][k] == 1
        assert rows['plane'][k][0] == 0 and (rows['plane'][k][1:] == -1).all()


def test_hold_out_is_the_references_view():
    from sunerf_hip.observations import hold_out_index
    assert [hold_out_index(n) for n in (1, 5, 6, 7, 12, 13)] == [0, 0, 1, 1, 2, 2]
    obs, _ = _observation_set(7)
    assert obs.held_out == [] and obs.training_views == list(range(7))
    obs.hold_out('reference')
    assert obs.held_out == [1] and obs.training_views == [0, 2, 3, 4, 5, 6]
    obs.add_view(torch.zeros(4, 6), 0., 0., 215., time=2.0, grid={'shape': (4, 6), 'cdelt': (300., 300.)})
    for _ in range(4):
        obs.add_view(torch.zeros(4, 6), 0., 0., 215., time=2.0, grid={'shape': (4, 6), 'cdelt': (300., 300.)})
    assert obs.held_out == [2]                      # 12 // 6: resolved when asked, not when set
    obs.hold_out([3, 0])
    assert obs.held_out == [0, 3]
    obs.hold_out(None)
    assert obs.held_out == []
    obs.hold_out(40)
    with pytest.raises(IndexError):
        obs.held_out
    with pytest.raises(ValueError):
        obs.hold_out('first')


def test_channel_map_with_absent_channels():
    from sunerf_hip.observations import MAX_CHANNELS, channel_map
    plane, wl = channel_map([0, 171, 0, 193, 211, 0, 0], 3)
    assert plane.tolist() == [-1, 0, -1, 1, 2, -1, -1] and wl.dtype == np.float32 and wl.tolist() == [0, 171, 0, 193, 211, 0, 0]
    with pytest.raises(ValueError):
        channel_map([0, 171, 0, 193], 3)
    with pytest.raises(ValueError):
        channel_map(np.ones(MAX_CHANNELS + 1), MAX_CHANNELS + 1)
    planes = np.arange(3 * 2 * 2, dtype=np.float32).reshape(3, 2, 2)
    target, wave, valid = ref.channel_fill(planes, [0, 171, 0, 193, 211, 0, 0], 1)
    assert target.shape == (4, 7) and valid.all()
    assert target[:, 1].tolist() == [0, 1, 2, 3] and target[:, 4].tolist() == [8, 9, 10, 11] and not target[:, [0, 2, 5, 6]].any()
    assert (wave == np.float32([0, 171, 0, 193, 211, 0, 0])).all()


def test_block_mean_of_a_known_array():
    a = np.arange(24, dtype=np.float32).reshape(4, 6)
    assert np.array_equal(ref.block_mean(a, 2), np.float32([[3.5, 5.5, 7.5], [15.5, 17.5, 19.5]]))
    assert ref.block_mean(a, 1).tobytes() == a.tobytes()
    # one rounding: the fp64 sum of 1 + 3 x 2^-24 is exact, an fp32 running sum would have lost every small term
    b = np.float32([[1.0, 2.0 ** -24], [2.0 ** -24, 2.0 ** -24]])
    assert ref.block_mean(b, 2)[0, 0] == np.float32((1.0 + 3 * 2.0 ** -24) / 4)
    assert ref.block_mean(b, 2)[0, 0] != np.float32(np.float32(1.0) / 4)
    c = a.copy()
    c[1, 1] = np.nan
    m = ref.block_mean(c, 2)
    assert np.isnan(m[0, 0]) and np.isfinite(m.reshape(-1)[1:]).all()


def test_non_dividing_downscale_is_refused():
    from sunerf_hip.observations import ObservationSet
    obs = ObservationSet(device='cpu')
    grid = {'shape': (9, 12), 'cdelt': (100., 100.)}
    for f in (2, 4, 0, -1):
        with pytest.raises(ValueError):
            obs.add_view(torch.zeros(9, 12), 0., 0., 215., time=0., grid=grid, downscale=f)
    assert obs.add_view(torch.zeros(9, 12), 0., 0., 215., time=0., grid=grid, downscale=3) == 0
    v = obs.views[0]
    assert (v.height, v.width) == (3, 4) and v.grid['shape'] == (3, 4) and v.grid['cdelt'] == (300., 300.)
    # the reduced grid spans the same field of view: its axes are those of the loader's resampled frame
    from sunerf.evaluation.loader import linear_plate_scale_axes
    tx, ty = linear_plate_scale_axes(grid, (3, 4), 'cpu')
    assert torch.equal(v.tx, tx) and torch.equal(v.ty, ty)
    with pytest.raises(ValueError):        # neither grid nor angles
        obs.add_view(torch.zeros(9, 12), 0., 0., 215., time=0.)
    with pytest.raises(ValueError):        # a set has one channel count
        obs.add_view(torch.zeros(2, 9, 12), 0., 0., 215., time=0., grid=grid, wavelengths=[171, 193])


def test_config_and_time_normalisation():
    from sunerf.evaluation.loader import normalize_datetime
    from sunerf_hip.observations import ObservationSet, normalize_time
    obs, t0 = _observation_set(7)
    assert obs.ref_time == t0                                   # the first datetime, as no ref_time was given
    when = t0 + datetime.timedelta(hours=18)
    assert obs.views[3].time == normalize_datetime(when, 86400.0, t0) == 0.75
    assert normalize_time(when, 3600.0, t0) == normalize_datetime(when, 3600.0, t0) and normalize_time(0.3, 1., None) == 0.3
    obs.hold_out('reference')
    config = obs.config
    assert set(config) == {'type', 'Rs_per_ds', 'seconds_per_dt', 'ref_time', 'wcs', 'resolution', 'wavelength', 'times'}
    assert config['type'] == 'emission' and config['ref_time'] == t0 and config['seconds_per_dt'] == 86400.0
    assert config['resolution'] == (5, 6) and config['wcs']['shape'] == (5, 6)        # the held-out view (index 1)
    assert config['times'][3] == when and len(config['times']) == 7
    assert (obs.Rs_per_ds, obs.seconds_per_dt, obs.ref_time) == (1.0, 86400.0, t0)     # what save_state reads
    multi = ObservationSet(ref_time=t0, device='cpu')
    multi.add_view(torch.zeros(2, 4, 4), 0., 0., 215., time=when, grid={'shape': (4, 4), 'cdelt': (1., 1.)},
                   wavelengths=[0, 171, 193])
    config = multi.config
    assert set(config) == {'type', 'Rs_per_ds', 'seconds_per_dt', 'ref_time', 'wcs', 'resolution', 'wavelengths', 'times'}
    assert config['type'] == 'D_T' and config['wavelengths'].tolist() == [0, 171, 193]


def test_pool_needs_a_device():
    from sunerf_hip.lib import SunerfHipError
    obs, _ = _observation_set(3)
    with pytest.raises(SunerfHipError):
        obs.pool(16)


def test_entry_point_is_declared_bound_and_exported(lib):
    import sunerf_hip
    header = open(os.path.join(ROOT, 'include', 'sunerf_hip.h')).read()
    for name in ('sunerf_build_ray_pool', 'sunerf_view_desc_bytes'):
        assert re.search(r'\b' + name + r'\s*\(', header) and name in sunerf_hip.symbols('core')
        assert getattr(lib, name) is not None
    assert re.search(r'#define\s+SUNERF_ABI_VERSION\s+9\b', header) and lib.sunerf_abi_version() == 9
    from sunerf_hip.observations import VIEW_DESC
    assert lib.sunerf_view_desc_bytes() == VIEW_DESC.itemsize


def test_argument_errors_without_gpu(lib):
    """Refused before anything touches a device (the pointers below are never dereferenced on the host)."""
    build = lib.sunerf_build_ray_pool
    views, out = 0x1000, 0x2000          # non-null, 16-byte aligned stand-ins

    def call(views=views, n_views=2, n_pixels=100, valid=None, n_valid=100, channels=1, begin=0, n=10, rays=out, time=out,
             target=out, wl=None):
        return build(views, n_views, n_pixels, valid, n_valid, channels, 1, 0, 0, begin, n, rays, time, target, wl, None)
    assert call(views=None) == -1 and call(n_views=0) == -1 and call(n_views=-3) == -1
    assert call(n_pixels=0, n_valid=0) == -1 and call(n_valid=0) == -1 and call(n_valid=-5) == -1      # V = 0
    assert call(n_valid=50) == -1                       # pixels dropped but no index
    assert call(n_valid=101) == -1 and call(n_pixels=2 ** 40, n_valid=2 ** 40) == -1
    assert call(channels=0) == -1 and call(channels=17) == -1
    assert call(begin=-1) == -1 and call(n=-1) == -1 and call(begin=95, n=6) == -1 and call(begin=101, n=0) == -1
    assert call(rays=None) == -1 and call(time=None) == -1
    assert call(rays=out + 4) == -1 and call(target=out + 8) == -1 and call(wl=out + 12) == -1      # 16-byte alignment
    assert call(n=0) == 0 and call(begin=100, n=0) == 0 and call(n=0, rays=None, time=None) == 0       # nothing to do
