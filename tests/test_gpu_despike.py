"""The despiking kernels (csrc/despike.hip) against the NumPy restatement tests/despike_reference.py: ``image`` by value with NaN at
the same places, ``mask`` and ``state`` exactly -- the algorithm uses + - * max and comparisons on float64 only, so there is no
tolerance.  Shapes are the smallest at which the kernel can go wrong: frames smaller than the window, single rows and columns,
33 x 65 and 9 x 33 (one pixel past the 8 x 32 tile in each axis), every radius, both modes, every flag, and planes built to take
each path: all NaN, wholly bad, hits on every edge and corner, a block too large to fill, ties, a plane that stops beside one that
does not.  Inputs hold no negative zero.  The reference of a case is computed once and shared."""
import functools

import numpy as np
import pytest
import torch

import despike_reference as dr

pytestmark = pytest.mark.gpu

TILE = (8, 32)                                    # csrc/despike.hip: DS_TH x DS_TW
A, B = 1.0e-4, 4.0e-3                             # variance = A + B signal: sigma 0.064 at signal 1


def _dev():
    assert torch.cuda.is_available(), 'GPU tests need a ROCm device'
    return torch.device('cuda', torch.cuda.current_device())


def make_planes(c, h, w, seed, hits=0.03, invalid=0.01):
    """``[c, h, w]`` float32: a smooth positive scene with noise of the (A, B) model, ``hits`` of the pixels raised by 8 .. 40 sigma
    (every third one with a weaker neighbour that only the lower threshold catches), ``invalid`` of them NaN or +-inf."""
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[:h, :w]
    out = np.empty((c, h, w), dtype=np.float32)
    for p in range(c):
        scene = 1.0 + 0.5 * np.sin(xx / 6.0 + p) * np.cos(yy / 5.0) + 0.02 * xx
        sigma = np.sqrt(A * (p + 1) + B * scene)
        x = scene + sigma * rng.standard_normal((h, w))
        n_hits = max(1, int(round(hits * h * w)))
        for k, q in enumerate(rng.choice(h * w, n_hits, replace=False)):
            y0, x0 = divmod(int(q), w)
            x[y0, x0] += rng.uniform(8, 40) * sigma[y0, x0]
            if k % 3 == 0 and x0 + 1 < w:
                x[y0, x0 + 1] += 4.0 * sigma[y0, x0 + 1]
        n_bad = int(round(invalid * h * w))
        for k, q in enumerate(rng.choice(h * w, n_bad, replace=False)):
            x.reshape(-1)[q] = (np.nan, np.inf, -np.inf)[k % 3]
        out[p] = x.astype(np.float32)
    return out


def params_of(c):
    return np.array([[A * (p + 1), B * (1 + 0.25 * p), 0.5 * np.sqrt(A * (p + 1)), 0.0] for p in range(c)])


def device_run(x, bad, params, radius, mode, flags, n_sigma, grow_sigma, min_valid, max_iterations):
    from sunerf_hip.despike import launch
    dev = _dev()
    clean, mask, state = launch(torch.from_numpy(x).to(dev), None if bad is None else torch.from_numpy(bad.astype(np.uint8)).to(dev),
                                torch.from_numpy(np.ascontiguousarray(params, dtype=np.float64)).to(dev), radius, mode, flags, n_sigma,
                                grow_sigma, min_valid, max_iterations)
    torch.cuda.synchronize(dev)
    return clean.cpu().numpy(), mask.cpu().numpy(), state.cpu().numpy()


def compare(x, bad=None, params=None, radius=2, mode=dr.MODEL, flags=0, n_sigma=5.0, grow_sigma=3.0, min_valid=3, max_iterations=4,
            what=''):
    """Runs both sides on planes ``x`` [C, H, W], prints the counts and holds the device to the restatement.  Returns the
    restatement's ``(image, mask, state)``."""
    params = params_of(x.shape[0]) if params is None else np.asarray(params, dtype=np.float64)
    kw = dict(radius=radius, mode=mode, flags=flags, n_sigma=n_sigma, grow_sigma=grow_sigma, min_valid=min_valid,
              max_iterations=max_iterations)
    want = dr.despike(x, bad=bad, params=params, **kw)
    got = device_run(x, bad, params, **kw)
    print(f'{what} {x.shape} radius {radius} mode {mode} flags {flags} passes <= {max_iterations}: state (n_spike, n_invalid, n_unfilled, '
          f'passes, converged, 0) = {want[2].tolist()}')
    assert got[1].dtype == np.uint8 and got[0].dtype == np.float32 and got[2].shape == (x.shape[0], dr.N_STATE)
    assert np.array_equal(got[2], want[2]), ('state', got[2].tolist(), want[2].tolist())
    differ = got[1] != want[1]
    assert not differ.any(), ('mask', int(differ.sum()), np.argwhere(differ)[:5].tolist())
    differ = ~((got[0] == want[0]) | (np.isnan(got[0]) & np.isnan(want[0])))
    assert not differ.any(), ('image', int(differ.sum()), np.argwhere(differ)[:5].tolist())
    assert np.array_equal(got[0], want[0], equal_nan=True)
    untouched = want[1] == 0
    assert np.array_equal(got[0][untouched].view(np.uint32), x[untouched].view(np.uint32))          # bit for bit
    return want


@functools.lru_cache(maxsize=None)
def planes(c, h, w, seed):
    return make_planes(c, h, w, seed)


# ---- shapes -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('mode', [dr.MODEL, dr.MAD], ids=['model', 'mad'])
@pytest.mark.parametrize('radius', [1, 2, 3])
@pytest.mark.parametrize('shape', [(5, 7), (1, 40), (40, 1)], ids=['5x7', '1x40', '40x1'])
def test_frames_smaller_than_the_window_and_single_rows_and_columns(shape, radius, mode):
    want = compare(planes(1, *shape, 11), radius=radius, mode=mode, min_valid=2, what='small frame')
    assert want[2][0, 1] >= 0


@pytest.mark.parametrize('mode', [dr.MODEL, dr.MAD], ids=['model', 'mad'])
@pytest.mark.parametrize('radius', [1, 2, 3])
@pytest.mark.parametrize('c,h,w', [(1, 33, 65), (3, 33, 65), (1, TILE[0] + 1, TILE[1] + 1), (3, TILE[0] + 1, TILE[1] + 1)],
                         ids=['1x33x65', '3x33x65', '1x9x33', '3x9x33'])
def test_tiles_and_their_tails_with_one_and_three_planes_of_different_parameters(c, h, w, radius, mode):
    want = compare(planes(c, h, w, 100 * c + h), radius=radius, mode=mode, what='tiles')
    assert (want[2][:, 0] > 0).all() and (want[2][:, 1] > 0).all()          # every plane has hits and invalid pixels


# ---- flags ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('mode', [dr.MODEL, dr.MAD], ids=['model', 'mad'])
def test_two_sided_flags_negative_outliers_too(mode):
    x = planes(2, 33, 65, 7).copy()
    x[:, 5::7, 3::11] -= 2.0                      # deep negative outliers (30 sigma)
    one = compare(x, mode=mode, what='one-sided')
    two = compare(x, mode=mode, flags=dr.TWO_SIDED, what='two-sided')
    low = np.zeros(x.shape, dtype=bool)
    low[:, 5::7, 3::11] = np.isfinite(x[:, 5::7, 3::11])
    assert not (one[1][low] & dr.SPIKE).any() and (two[1][low] & dr.SPIKE).mean() > 0.9


@pytest.mark.parametrize('radius', [1, 2, 3])
def test_fill_nan_drops_every_flagged_pixel_and_sets_no_unfilled_bit(radius):
    x = planes(2, 33, 65, 8)
    image, mask, state = compare(x, radius=radius, flags=dr.FILL_NAN, what='fill nan')
    assert np.array_equal(np.isnan(image), mask != 0) and not (mask & dr.UNFILLED).any() and (state[:, 2] == 0).all()
    compare(x, radius=radius, flags=dr.FILL_NAN | dr.TWO_SIDED, mode=dr.MAD, what='fill nan, two-sided, mad')


@pytest.mark.parametrize('radius', [1, 2, 3])
def test_no_iterations_is_masked_median_inpainting_of_bad_and_nan_pixels(radius):
    x = planes(2, 33, 65, 9)
    bad = np.zeros(x.shape, dtype=np.uint8)
    bad[:, ::4, ::5] = 1
    bad[1, 10:13, 20:24] = 7                      # any non-zero value
    image, mask, state = compare(x, bad=bad, radius=radius, max_iterations=0, what='inpainting')
    assert not (mask & dr.SPIKE).any() and (state[:, 3:5] == 0).all() and ((mask & dr.INVALID) != 0)[bad != 0].all()
    assert np.array_equal(state[:, 1], ((bad != 0) | ~np.isfinite(x)).sum(axis=(1, 2)))


# ---- planes built to take each path -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('mode', [dr.MODEL, dr.MAD], ids=['model', 'mad'])
def test_a_plane_of_all_nan_and_a_plane_wholly_bad_beside_an_ordinary_one(mode):
    x = planes(3, 19, 37, 10).copy()
    x[0] = np.nan
    bad = np.zeros(x.shape, dtype=np.uint8)
    bad[2] = 1
    image, mask, state = compare(x, bad=bad, mode=mode, what='all nan / wholly bad')
    for p in (0, 2):
        assert np.isnan(image[p]).all() and (mask[p] == dr.INVALID | dr.UNFILLED).all() and state[p].tolist() == [0, 19 * 37, 19 * 37, 0, 1, 0]
    assert state[1, 0] > 0 and not (mask[1] & dr.UNFILLED).any()
    compare(x, bad=bad, mode=mode, flags=dr.FILL_NAN, max_iterations=1, what='all nan / wholly bad, fill nan')


@pytest.mark.parametrize('radius', [1, 2, 3])
def test_hits_in_all_four_corners_and_on_every_edge(radius):
    h, w = 2 * TILE[0] + 3, 2 * TILE[1] + 5
    x = planes(1, h, w, 12).copy()
    x[~np.isfinite(x)] = 1.0
    spots = [(0, 0), (0, w - 1), (h - 1, 0), (h - 1, w - 1), (0, w // 2), (h - 1, w // 3), (h // 2, 0), (h // 3, w - 1),
             (0, TILE[1]), (TILE[0], 0), (TILE[0] - 1, w - 1), (h - 1, TILE[1] - 1)]
    for y, xq in spots:
        x[0, y, xq] += 5.0
    _, mask, _ = compare(x, radius=radius, what='corners and edges')
    assert all(mask[0, y, xq] == dr.SPIKE for y, xq in spots)
    compare(x, radius=radius, mode=dr.MAD, min_valid=1, what='corners and edges, mad')


def test_a_block_of_hits_larger_than_the_window_cannot_be_filled():
    x = planes(2, 21, 40, 13).copy()
    x[~np.isfinite(x)] = 1.0
    x[0, 6:15, 9:18] += 9.0                       # 9 x 9 under window 5: the block's core has no clean neighbour
    bad = np.zeros(x.shape, dtype=np.uint8)
    bad[0, 6:15, 9:18] = 1
    image, mask, state = compare(x, bad=bad, radius=2, what='9 x 9 block, bad')
    core = (slice(8, 13), slice(11, 16))
    assert (mask[0][core] == dr.INVALID | dr.UNFILLED).all() and np.isnan(image[0][core]).all() and state[0, 2] >= 25
    assert not np.isnan(image[0, 6, 9]) and state[1, 2] == 0
    compare(x, radius=2, min_valid=1, max_iterations=8, what='9 x 9 block, found')          # eaten from the rim, pass by pass


@pytest.mark.parametrize('mode', [dr.MODEL, dr.MAD], ids=['model', 'mad'])
@pytest.mark.parametrize('radius', [1, 2, 3])
def test_ties_come_out_as_the_order_statistics_define_them(radius, mode):
    """Integer-quantised planes of at most 8, 6 and 4 distinct values (4, 3 and 2 levels, and each of them under a hit): most
    neighbours are equal, which is where selection by comparison breaks."""
    rng = np.random.default_rng(14)
    x = np.stack([rng.integers(1, 5, (33, 65)), rng.integers(1, 4, (33, 65)), rng.integers(1, 3, (33, 65))]).astype(np.float32)
    x[:, ::9, ::13] += 40.0
    x[0, 3, 3] = np.nan
    params = [[0.05, 0.1, 0.2, 0.0]] * 3
    want = compare(x, params=params, radius=radius, mode=mode, n_sigma=3.0, grow_sigma=2.0, what='ties')
    assert len(np.unique(x[0][np.isfinite(x[0])])) <= 8 and (want[2][:, 0] > 0).all()
    compare(x, params=params, radius=radius, mode=mode, n_sigma=0.5, grow_sigma=0.25, flags=dr.TWO_SIDED, what='ties, low threshold')


def stopping_planes():
    """``(planes [3, 19, 70], params)``: plane 0 has no hit (its first pass flags nothing), plane 1 one hit (the second pass flags
    nothing), plane 2 a track whose pixels only the lower threshold beside a flagged pixel catches: one more per pass, nine in all."""
    h, w = 19, 70
    x = np.ones((3, h, w), dtype=np.float32)
    x += (0.001 * np.arange(w, dtype=np.float32))[None, None, :]
    x[1, 9, 40] += 2.0
    x[2, 9, 30] += 2.0                            # 20 sigma
    x[2, 9, 31:39] += 0.4                         # 4 sigma each: between grow_sigma 3 and n_sigma 5
    return x, [[0.01, 0.0, 0.1, 0.0]] * 3


def test_a_plane_stops_on_its_own_beside_one_that_uses_every_pass():
    x, params = stopping_planes()
    _, mask, state = compare(x, params=params, radius=2, max_iterations=4, what='per-plane stop')
    assert state[:, 3].tolist() == [0, 1, 4] and state[:, 4].tolist() == [1, 1, 0] and state[:, 0].tolist() == [0, 1, 4]
    assert mask[2, 9, 30:34].tolist() == [1, 1, 1, 1] and not mask[2, 9, 34:].any()
    _, _, odd = compare(x, params=params, radius=2, max_iterations=5, what='per-plane stop, odd count')
    assert odd[:, 3].tolist() == [0, 1, 5] and odd[:, 4].tolist() == [1, 1, 0]
    _, _, full = compare(x, params=params, radius=3, max_iterations=64, what='per-plane stop, every pass allowed')
    assert full[:, 3].tolist() == [0, 1, 9] and full[:, 4].tolist() == [1, 1, 1]


# ---- the call ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('mode,iterations', [(dr.MODEL, 4), (dr.MAD, 3)], ids=['model-4', 'mad-3'])
def test_reruns_give_equal_bits_whatever_the_outputs_and_the_workspace_held(mode, iterations):
    from sunerf_hip import lib
    from sunerf_hip.ops import _ptr, _stream
    dev = _dev()
    x = planes(3, 33, 65, 15)
    c, h, w = x.shape
    image = torch.from_numpy(x).to(dev)
    params = torch.from_numpy(params_of(c)).to(dev)
    nbytes = int(lib.load().sunerf_despike_workspace_bytes(c, h, w, 2))
    runs = []
    for fill in (0x00, 0xFF, 0x01, 0xFF):
        clean = torch.full((c, h, w), float('nan') if fill == 0xFF else float(fill), dtype=torch.float32, device=dev)
        mask = torch.full((c, h, w), fill, dtype=torch.uint8, device=dev)
        state = torch.full((c, dr.N_STATE), float(fill), dtype=torch.float64, device=dev)
        ws = torch.full((nbytes,), fill, dtype=torch.uint8, device=dev)
        lib.call(dev, 'sunerf_despike', _ptr(image), None, _ptr(params), c, h, w, 2, mode, 0, 5.0, 3.0, 3, iterations, _ptr(clean),
                 _ptr(mask), _ptr(state), _ptr(ws), _stream(dev))
        torch.cuda.synchronize(dev)
        runs.append((clean.view(torch.int32).cpu(), mask.cpu(), state.view(torch.int64).cpu()))
    for other in runs[1:]:
        assert all(torch.equal(a, b) for a, b in zip(runs[0], other))
    want = dr.despike(x, params=params_of(c), radius=2, mode=mode, max_iterations=iterations)
    assert np.array_equal(runs[0][1].numpy(), want[1]) and np.array_equal(runs[0][2].view(torch.float64).numpy(), want[2])
    assert torch.equal(image.cpu().view(torch.int32), torch.from_numpy(x).view(torch.int32))          # the input is read only


def test_the_wrapper_and_the_instrument_method_run_the_same_call():
    from sunerf_hip.despike import add_cosmic_rays, despike, despike_params
    from sunerf_hip.instrument import Instrument
    dev = _dev()
    inst = Instrument(unit=[100.0, 50.0], exposure=2.9, dn_per_photon=1.2, read_noise=1.2)
    rng = np.random.default_rng(16)
    truth = 1.0 + 0.3 * np.sin(np.arange(48)[None, :] / 5.0) * np.ones((2, 40, 48))
    sigma = inst.errors(torch.from_numpy(truth), channel_axis=0)
    x = torch.from_numpy(truth).float() + sigma * torch.from_numpy(rng.standard_normal(truth.shape)).float()
    x, where = add_cosmic_rays(x, 0.01, (15.0, 50.0), sigma=sigma, seed=2)
    x[1, 3, 4] = float('nan')
    p = despike_params(inst, 2)
    for kw in (dict(), dict(window=7, fill='nan'), dict(mode='mad', window=5, two_sided=True, iterations=2), dict(window=3, min_valid=1)):
        got = inst.despike(x.to(dev), **kw)
        same = despike(x.to(dev), a=p[:, 0], b=p[:, 1], floor=p[:, 2], **kw)
        flags = (dr.TWO_SIDED if kw.get('two_sided') else 0) | (dr.FILL_NAN if kw.get('fill') == 'nan' else 0)
        want = dr.despike(x.numpy(), params=p, radius=kw.get('window', 5) // 2, mode=dr.MAD if kw.get('mode') == 'mad' else dr.MODEL,
                          flags=flags, min_valid=kw.get('min_valid', 3), max_iterations=kw.get('iterations', 4))
        for k in ('image', 'mask', 'n_spike', 'n_invalid', 'n_unfilled', 'passes', 'converged'):
            assert torch.equal(got[k].cpu(), same[k].cpu()) or k == 'image'
        assert np.array_equal(got['image'].cpu().numpy(), same['image'].cpu().numpy(), equal_nan=True)
        assert np.array_equal(got['image'].cpu().numpy(), want[0], equal_nan=True) and np.array_equal(got['mask'].cpu().numpy(), want[1])
        state = torch.stack([got['n_spike'], got['n_invalid'], got['n_unfilled'], got['passes'], got['converged'].long()], dim=1)
        assert np.array_equal(state.cpu().numpy(), want[2][:, :5].astype(np.int64))
        found = float(((got['mask'].cpu() & dr.SPIKE) != 0)[where].float().mean())
        print(kw, 'hits flagged:', found, 'state', want[2].tolist())
        assert found > 0.9 and got['n_invalid'].tolist() == [0, 1] and got['converged'].dtype == torch.bool
    one = inst_single = Instrument(unit=100.0, exposure=2.9, dn_per_photon=1.2, read_noise=1.2).despike(x[0].to(dev))
    assert one['image'].shape == (1, 40, 48) and inst_single['mask'].dtype == torch.uint8
    empty = despike(torch.zeros(0, 5, 7, device=dev), a=1.0, b=1.0)
    assert empty['image'].shape == (0, 5, 7) and empty['n_spike'].shape == (0,)
