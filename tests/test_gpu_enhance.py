"""The enhancement filters on the device against their NumPy restatement (tests/enhance_reference.py).

MGN: ``lo``, ``hi``, the state and the NaN positions exactly; values within the bound the restatement derives from its own
quantities (the fp32 tap sums of G[x] and G[r^2] carried through r / s and the derivative of atan, plus the ulps of atan, pow and
sqrt; the floor keeps it finite).  Shapes: one pixel, an image far smaller than the window, one row, one column, one pixel past the
row tile (4 x 512) and past the column tile (128 x 32), three planes of 150 x 300 under the default six scales, a radius of 0, eight
scales; variants with invalid pixels, given ``lo`` / ``hi``, ``floor = 0`` and a pedestal.

Ring statistics and NRGF (cases: tests/test_enhance_host.py ``RADIAL_CASES``): ``count``, ``min``, ``max``, ring membership and the
state exactly, segment membership exactly apart from undecidable pixels (none in these cases), ``mean`` and ``std`` within the
derived fp64 bound, NRGF values within 2^-23 |want| plus the propagated bound.

Reruns: every entry point twice through the raw call, on outputs (and a workspace) that first hold NaN and then a sentinel: equal bits.
The worst error over its bound is printed for every case."""
import ctypes
import functools

import numpy as np
import pytest
import torch

import enhance_reference as er
from test_enhance_host import RADIAL_CASES, radial_case

pytestmark = pytest.mark.gpu

SENTINEL = -12345.0


def _dev():
    assert torch.cuda.is_available(), 'GPU tests need a ROCm device'
    return torch.device('cuda', torch.cuda.current_device())


def _structure(shape, seed, pedestal=0.0, scale=1.0):
    """Positive data with structure at every pixel and a trend; the planes differ in range."""
    rng = np.random.default_rng(seed)
    c, h, w = shape
    y, x = np.meshgrid(np.arange(h), np.arange(w), indexing='ij')
    planes = [pedestal + scale * (p + 1.0) ** 2 * (np.exp(0.6 * rng.standard_normal((h, w))) + 0.02 * x + 0.5 * np.sin(0.3 * y + p)) for p in range(c)]
    return np.stack(planes).astype(np.float32)


def _holes(planes, whole_plane=None):
    """NaN and flagged pixels at a corner, in a run longer than the widest window here (2 x 30 + 1), an inf, and a whole plane."""
    planes = planes.copy()
    bad = np.zeros(planes.shape, dtype=np.uint8)
    planes[:, 0, 0] = np.nan
    bad[:, -1, -1] = 1
    planes[0, 7, 5:80] = np.nan
    bad[0, 20:24, 10:85] = 1
    planes[0, 30, 40] = np.inf
    if whole_plane is not None:
        planes[whole_plane] = np.nan
    return planes, bad


# name -> (planes, keyword arguments)
@functools.lru_cache(maxsize=None)
def mgn_case(name):
    if name == 'one_pixel':
        return np.full((1, 1, 1), 3.0, dtype=np.float32), {}
    if name == 'smaller_than_the_window':
        return _structure((1, 5, 7), 1), dict(sigma=(40.0,))
    if name == 'one_row':
        return _structure((1, 1, 300), 2), {}
    if name == 'one_column':
        return _structure((1, 300, 1), 3), {}
    if name == 'past_the_row_tile':
        return _structure((1, 5, 513), 4), dict(sigma=(2.5, 20.0))
    if name == 'past_the_column_tile':
        return _structure((1, 129, 33), 5), dict(sigma=(2.5, 20.0))
    if name == 'default_scales':
        return _structure((3, 150, 300), 6), {}
    if name == 'radius_0':
        return _structure((2, 20, 30), 7), dict(sigma=(0.1,))
    if name == 'eight_scales':
        return _structure((2, 40, 70), 8), dict(sigma=(1.0, 1.5, 2.0, 3.0, 4.0, 6.0, 8.0, 12.0), weights=(1.0, 0.5, 2.0, 1.0, -1.0, 0.25, 1.5, 1.0), k=1.3, gamma=2.2, h=0.4,
                                                truncate=2.5)
    if name == 'invalid':
        planes, bad = _holes(_structure((3, 60, 90), 9), whole_plane=2)
        return planes, dict(sigma=(1.25, 5.0, 10.0), bad=bad)
    if name == 'given_range':
        planes = _structure((2, 60, 90), 10)
        return planes, dict(sigma=(1.25, 5.0, 10.0), lo=(2.0, 6.0), hi=float(np.percentile(planes[0], 90)))
    if name == 'given_range_invalid':
        planes, bad = _holes(_structure((2, 60, 90), 11))
        return planes, dict(sigma=(1.25, 10.0), bad=bad, lo=1.5, hi=(4.0, 30.0), floor=(0.01, 0.5))
    if name == 'floor_0':
        return _structure((1, 60, 90), 12), dict(sigma=(1.25, 5.0, 10.0), floor=0.0)
    if name == 'pedestal':
        return _structure((1, 60, 90), 13, pedestal=1e3, scale=0.25), dict(sigma=(1.25, 5.0, 10.0))
    raise KeyError(name)


MGN_CASES = ('one_pixel', 'smaller_than_the_window', 'one_row', 'one_column', 'past_the_row_tile', 'past_the_column_tile', 'default_scales',
             'radius_0', 'eight_scales', 'invalid', 'given_range', 'given_range_invalid', 'floor_0', 'pedestal')


@functools.lru_cache(maxsize=None)
def mgn_reference(name):
    planes, kw = mgn_case(name)
    return er.mgn(planes, **kw)


def _gpu(array, dev):
    return None if array is None else torch.from_numpy(np.ascontiguousarray(array)).to(dev)


@pytest.mark.parametrize('name', MGN_CASES)
def test_mgn_matches_the_restatement(name):
    from sunerf_hip.enhance import mgn
    dev = _dev()
    planes, kw = mgn_case(name)
    want, lo, hi, state, detail = mgn_reference(name)
    call = dict(kw)
    if 'bad' in call:
        call['bad'] = _gpu(call['bad'], dev)
    got = mgn(_gpu(planes, dev), **call)
    torch.cuda.synchronize(dev)
    image = got['image'].cpu().numpy().astype(np.float64)
    assert np.array_equal(got['lo'].cpu().numpy().view(np.uint32), lo.view(np.uint32)), (got['lo'].tolist(), lo.tolist())
    assert np.array_equal(got['hi'].cpu().numpy().view(np.uint32), hi.view(np.uint32)), (got['hi'].tolist(), hi.tolist())
    assert got['counts'].cpu().tolist() == state.tolist()
    nan = np.isnan(want)
    assert np.array_equal(np.isnan(image), nan) and nan.sum() == state[:, 0].sum()
    err, bound = np.abs(image - want)[~nan], detail['bound'][~nan]
    ratio = float((err / bound).max()) if err.size else 0.0
    print(f'mgn {name}: worst error {err.max() if err.size else 0.0:.3e}, worst bound {bound.max() if err.size else 0.0:.3e}, worst error / bound {ratio:.3e}, '
          f'pixels where the bound gives up {(bound >= 0.3 * np.pi / max(1, len(kw.get("sigma", er.DEFAULT_SIGMA)))).sum()} of {bound.size}')
    assert bool((err <= bound).all())
    if name in ('given_range', 'given_range_invalid'):
        assert state[:, 1].min() > 0 and state[:, 2].min() > 0
    if name == 'invalid':
        assert state[2, 0] == 60 * 90 and np.isnan(lo[2]) and state[0, 0] > 300
    if name not in ('floor_0', 'one_pixel'):          # the bound means something: far below the range of the result
        assert np.isfinite(bound).all() and bound.max() < 0.2
    # an image without a plane axis is its one plane
    if planes.shape[0] == 1 and 'bad' not in kw:
        flat = mgn(_gpu(planes[0], dev), **call)
        assert flat['image'].dim() == 2 and torch.equal(flat['image'], got['image'][0]) and torch.equal(flat['counts'], got['counts'])


def test_a_plane_with_an_invalid_pixel_does_not_change_its_neighbours_path():
    """The mask sums are decided per plane on the device: a clean plane beside one with a NaN gives the bits it gives alone."""
    from sunerf_hip.enhance import mgn
    dev = _dev()
    planes = _structure((2, 40, 50), 21)
    alone = mgn(_gpu(planes[:1], dev), sigma=(2.5, 10.0))['image']
    planes[1, 3, 4] = np.nan
    both = mgn(_gpu(planes, dev), sigma=(2.5, 10.0))
    assert torch.equal(both['image'][0], alone[0]) and both['counts'][:, 0].tolist() == [0, 1]


# ---- rings ------------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def radial_reference(name):
    planes, bad, center, edges, n_segments = radial_case(name)
    return er.radial_statistics(planes, center, edges, n_segments, bad)


@pytest.mark.parametrize('name', list(RADIAL_CASES))
def test_radial_statistics_match_the_restatement(name):
    from sunerf_hip.enhance import radial_statistics
    dev = _dev()
    planes, bad, center, edges, n_segments = radial_case(name)
    count, mean, std, mn, mx, detail = radial_reference(name)
    assert not detail['undecidable'].any()          # else count, min and max of the two bins such a pixel may fall in could not be exact
    got = {k: v.cpu().numpy() for k, v in radial_statistics(_gpu(planes, dev), center, edges, n_segments, bad=_gpu(bad, dev)).items()}
    assert np.array_equal(got['count'], count), f'{(got["count"] != count).sum()} of {count.size} bins differ in count'
    empty = count == 0
    for key, want in (('min', mn), ('max', mx)):
        assert np.array_equal(got[key], want, equal_nan=True), key
    for key in ('mean', 'std'):
        assert np.array_equal(np.isnan(got[key]), empty), key
    ratios = {}
    for key, want, bound in (('mean', mean, detail['mean_bound']), ('std', std, detail['std_bound'])):
        err = np.abs(got[key] - want)[~empty]
        assert bool((err <= bound[~empty]).all()), (key, float((err / bound[~empty]).max()))
        ratios[key] = float((err / np.maximum(bound[~empty], 1e-300)).max()) if err.size else 0.0
    print(f'radial_statistics {name}: {count.size} bins, {int(empty.sum())} empty, {int(count.sum())} pixels; worst error / bound: mean {ratios["mean"]:.3e}, std {ratios["std"]:.3e}')
    assert count.sum() > 0 and (name != 'thin_rings' or empty.sum() > 0)


NRGF_CASES = [(name, outside) for name in RADIAL_CASES if RADIAL_CASES[name][3] == 1 for outside in ('keep', 'missing')]


@pytest.mark.parametrize('name,outside', NRGF_CASES, ids=[f'{n}-{o}' for n, o in NRGF_CASES])
def test_nrgf_matches_the_restatement(name, outside):
    from sunerf_hip.enhance import nrgf
    dev = _dev()
    planes, bad, center, edges, _ = radial_case(name)
    mode = er.KEEP if outside == 'keep' else er.MISSING
    want, state, stats, detail = er.nrgf(planes, center, edges, outside=mode, missing=-2.5, bad=bad)
    got = nrgf(_gpu(planes, dev), center, edges, outside=outside, missing=-2.5, bad=_gpu(bad, dev))
    image = got['image'].cpu().numpy().astype(np.float64)
    assert got['counts'].cpu().tolist() == state.tolist()
    nan = np.isnan(want)
    assert np.array_equal(np.isnan(image), nan)
    err = np.abs(image - want)[~nan]
    assert bool((err <= detail['bound'][~nan]).all())
    copied = ~nan & (detail['bound'] == 0)
    assert np.array_equal(image[copied], want[copied])          # kept, missing and degenerate pixels: exact
    ratio = float((err / np.maximum(detail['bound'][~nan], 1e-300))[detail['bound'][~nan] > 0].max()) if (detail['bound'][~nan] > 0).any() else 0.0
    print(f'nrgf {name} {outside}: state {state.tolist()}, worst error / bound {ratio:.3e}')
    count, mean, std, mn, mx, sdetail = radial_reference(name)
    table = {k: v.cpu().numpy() for k, v in got['statistics'].items()}
    assert np.array_equal(table['count'], count[..., 0]) and np.array_equal(table['min'], mn[..., 0], equal_nan=True) and np.array_equal(table['max'], mx[..., 0], equal_nan=True)
    # the caller's own statistics: the table the call computed gives the same bits; a table of its own gives what the restatement gives
    again = nrgf(_gpu(planes, dev), center, edges, outside=outside, missing=-2.5, bad=_gpu(bad, dev),
                 statistics={k: got['statistics'][k] for k in ('count', 'mean', 'std')})
    assert torch.equal(again['image'].view(torch.int32), got['image'].view(torch.int32)) and torch.equal(again['counts'], got['counts'])
    assert set(again['statistics']) == {'count', 'mean', 'std'}
    own = (np.full(count[..., 0].shape, 5, dtype=np.int64), np.full(mean[..., 0].shape, 1.5), np.full(std[..., 0].shape, 0.25))
    own[0][:, ::3], own[2][:, 1::3] = 1, 0.0          # degenerate rings by count and by spread
    want2, state2, _, detail2 = er.nrgf(planes, center, edges, outside=mode, missing=-2.5, bad=bad, statistics=own)
    got2 = nrgf(_gpu(planes, dev), center, edges, outside=outside, missing=-2.5, bad=_gpu(bad, dev),
                statistics=dict(zip(('count', 'mean', 'std'), (_gpu(v, dev) for v in own))))
    image2 = got2['image'].cpu().numpy().astype(np.float64)
    assert got2['counts'].cpu().tolist() == state2.tolist() and np.array_equal(np.isnan(image2), np.isnan(want2))
    assert bool((np.abs(image2 - want2)[~nan] <= detail2['bound'][~nan]).all())


# ---- reruns -----------------------------------------------------------------------------------------------------------------------------
def _filled(shape, dtype, dev, fill):
    t = torch.empty(shape, dtype=dtype, device=dev)
    if dtype == torch.int64:
        t.fill_(-12345 if fill == SENTINEL else -1)
    else:
        t.fill_(fill)
    return t


def raw_mgn(name, fill):
    from sunerf_hip import lib, ops
    dev = _dev()
    planes, kw = mgn_case(name)
    c, h, w = planes.shape
    x, bad = _gpu(planes, dev), _gpu(kw.get('bad'), dev)
    sigma = np.asarray(kw.get('sigma', er.DEFAULT_SIGMA), dtype=np.float64)
    per_plane = lambda v: None if v is None else _gpu(np.broadcast_to(np.asarray(v, dtype=np.float32), (c,)).copy(), dev)          # noqa: E731
    lo, hi, floor = per_plane(kw.get('lo')), per_plane(kw.get('hi')), per_plane(kw.get('floor'))
    out, lo_out, hi_out = _filled((c, h, w), torch.float32, dev, fill), _filled((c,), torch.float32, dev, fill), _filled((c,), torch.float32, dev, fill)
    state = _filled((c, 3), torch.int64, dev, fill)
    nbytes = int(lib.load().sunerf_enhance_mgn_workspace_bytes(c, h, w))
    ws = _filled((nbytes // 4 + 64,), torch.float32, dev, fill)
    ws_ptr = ws.data_ptr() + (-ws.data_ptr()) % 256
    lib.call(dev, 'sunerf_enhance_mgn', ops._ptr(x), ops._ptr(bad), c, h, w, sigma.ctypes.data_as(ctypes.c_void_p), None, len(sigma), 3.0, 0.7, 3.2, 0.7,
             ops._ptr(lo), ops._ptr(hi), ops._ptr(floor), ops._ptr(out), ops._ptr(lo_out), ops._ptr(hi_out), ops._ptr(state), ctypes.c_void_p(ws_ptr), nbytes,
             ops._stream(dev))
    torch.cuda.synchronize(dev)
    return [t.cpu().numpy() for t in (out, lo_out, hi_out, state)]


@pytest.mark.parametrize('name', ('invalid', 'given_range_invalid', 'past_the_column_tile'))
def test_mgn_reruns_are_bit_identical(name):
    first, second = raw_mgn(name, float('nan')), raw_mgn(name, SENTINEL)
    for a, b in zip(first, second):
        assert np.array_equal(a.view(np.uint8), b.view(np.uint8))
    assert not (second[0] == SENTINEL).any() and (second[3] >= 0).all()


def raw_rings(name, fill, apply):
    from sunerf_hip import lib, ops
    dev = _dev()
    planes, bad, center, edges, n_segments = radial_case(name)
    c, h, w = planes.shape
    x, flagged, e = _gpu(planes, dev), _gpu(bad, dev), _gpu(edges, dev)
    shape = (c, len(edges) - 1, 1 if apply else n_segments)
    count = _filled(shape, torch.int64, dev, fill)
    mean, std, mn, mx = (_filled(shape, torch.float64, dev, fill) for _ in range(4))
    outputs = [count, mean, std, mn, mx]
    if apply:
        out, state = _filled((c, h, w), torch.float32, dev, fill), _filled((c, 3), torch.int64, dev, fill)
        outputs += [out, state]
        lib.call(dev, 'sunerf_enhance_nrgf', ops._ptr(x), ops._ptr(flagged), c, h, w, center[0], center[1], ops._ptr(e), shape[1], 1, -2.5, 1, ops._ptr(count),
                 ops._ptr(mean), ops._ptr(std), ops._ptr(mn), ops._ptr(mx), ops._ptr(out), ops._ptr(state), ops._stream(dev))
    else:
        lib.call(dev, 'sunerf_enhance_radial_statistics', ops._ptr(x), ops._ptr(flagged), c, h, w, center[0], center[1], ops._ptr(e), shape[1], shape[2],
                 ops._ptr(count), ops._ptr(mean), ops._ptr(std), ops._ptr(mn), ops._ptr(mx), ops._stream(dev))
    torch.cuda.synchronize(dev)
    return [t.cpu().numpy() for t in outputs]


@pytest.mark.parametrize('name,apply', [('invalid', False), ('invalid_segments', False), ('thin_rings', False), ('invalid', True), ('thin_rings', True)])
def test_ring_reruns_are_bit_identical(name, apply):
    first, second = raw_rings(name, float('nan'), apply), raw_rings(name, SENTINEL, apply)
    for a, b in zip(first, second):
        assert np.array_equal(a.view(np.uint8), b.view(np.uint8))
        assert not (b == SENTINEL).any() and not (b == -12345).any()
