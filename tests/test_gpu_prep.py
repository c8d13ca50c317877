"""The image preparation on the device (``sunerf_hip/prep.py``, ``csrc/prep.hip``) against the fp64
restatement of tests/prep_reference.py (scipy.ndimage.affine_transform, np.sort, np.percentile).

The gate of every resample: ``|got - want| <= 2^-23 |want| + 1e-9 scale`` with ``scale`` = max |image| carried through the epilogue's
linear map (``|factor| / (vmax - vmin)``).  The first term is the one rounding to fp32; the second covers fp64 coordinate and
prefilter noise: a 1e-13 relative perturbation of scipy's own matrix moves its output by <= 5.3e-11 of the maximum, the truncated
horizon by <= 2.3e-14, and the host-side restatement of the kernels' arithmetic stays within 3.3e-13 of scipy's coefficients.  No
output pixel is left out: tests/test_prep_host.py shows that every case keeps clear of the borders where a 1e-13 change of the
coordinate would change the pixel.  Every test prints what it measured before it asserts."""
import functools

import numpy as np
import pytest
import torch

import prep_reference as pr
from sunerf_hip import prep

pytestmark = pytest.mark.gpu

CASES = pr.geometry_cases(prep.SEGMENT, prep.HORIZON)
MISSING = -3.5
PLAIN = dict(missing=MISSING, clip_negative=False, clip_to_input_range=False)


def _bits(a):
    return np.ascontiguousarray(np.asarray(a, dtype=np.float32)).view(np.uint32)


def _gpu(a):
    return torch.from_numpy(np.array(a)).cuda()


def _run(case, img, order, **kw):
    out, grid = prep.prepare_image(_gpu(img), case['wcs'], target_scale=case['s'], out_shape=case['out_shape'], order=order, **kw)
    assert out.is_cuda and out.dtype == torch.float32 and tuple(out.shape) == (img.shape[0],) + tuple(case['out_shape'])
    return out.cpu().numpy(), grid


@functools.lru_cache(maxsize=None)
def _want(name, order, n_planes):
    case = next(c for c in CASES if c['name'] == name)
    _, (matrix, offset) = pr.case_matrix(case)
    return pr.prepare(pr.case_image(case['wcs']['shape'], n_planes), matrix, offset, case['out_shape'], order, **PLAIN)[0]


# ---- the resample against scipy ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('n_planes', [1, 3])
@pytest.mark.parametrize('order', range(6))
@pytest.mark.parametrize('case', CASES, ids=[c['name'] for c in CASES])
def test_resample_matches_scipy(case, order, n_planes):
    img = pr.case_image(case['wcs']['shape'], n_planes)
    got, grid = _run(case, img, order, **PLAIN)
    want_grid, _ = pr.case_matrix(case)
    assert grid == want_grid
    want = _want(case['name'], order, n_planes)
    ratio = pr.gate(got, want, float(np.abs(img).max()))
    inside = int((want != MISSING).sum())
    print(f"{case['name']} order {order} C {n_planes}: |got - want| / bound = {ratio:.4f}, {inside} of {want.size} pixels inside the frame")
    assert ratio <= 1.0
    if case['name'] == 'strip':
        assert np.all(got[:, 0] == MISSING) and np.all(got[:, 2] == MISSING) and not np.any(got[:, 1] == MISSING)


@pytest.mark.parametrize('order', range(6))
def test_identity_returns_the_input(order):
    shape = (37, 53)
    img = pr.case_image(shape, 3)
    wcs = {'shape': shape, 'cdelt': (.6, .6), 'crpix': (27.0, 19.0), 'crval': (1.0, 2.0), 'crota': 0.0}
    out, grid = prep.prepare_image(_gpu(img), wcs, order=order, **PLAIN)
    got = out.cpu().numpy()
    assert grid['shape'] == shape
    ratio = pr.gate(got, img.astype(np.float64), float(np.abs(img).max()))
    differ = int((_bits(got) != _bits(img)).sum())
    print(f'identity order {order}: ratio {ratio:.4f}, {differ} of {img.size} values differ in bits')
    assert ratio <= 1.0
    if order <= 1:
        assert differ == 0


@pytest.mark.parametrize('order', range(6))
@pytest.mark.parametrize('turn', [1, -1])
def test_quarter_turn_returns_the_permuted_input(turn, order):
    n = 33
    img = pr.case_image((n, n), 3)
    wcs = {'shape': (n, n), 'cdelt': (1.3, 1.3), 'crota': turn * np.pi / 2}
    out, grid = prep.prepare_image(_gpu(img), wcs, order=order, **PLAIN)
    got = out.cpu().numpy()
    matrix, offset = prep.affine_matrix(wcs, grid)
    y, x = pr.source_coordinates(matrix, offset, (n, n))           # integers, a permutation (tests/test_prep_host.py)
    moved = img[:, y.astype(int), x.astype(int)]
    assert not np.array_equal(moved, img)
    ratio = pr.gate(got, moved.astype(np.float64), float(np.abs(img).max()))
    differ = int((_bits(got) != _bits(moved)).sum())
    print(f'quarter turn {turn} order {order}: ratio {ratio:.4f}, {differ} of {img.size} values differ in bits')
    assert ratio <= 1.0
    if order <= 1:
        assert differ == 0


# ---- epilogue and policies --------------------------------------------------------------------------------------------------------
FACTOR = [0.5, -2.0, 1.25]
NORM = ([10.0, 0.0, 400.0], [900.0, -999.0, 430.0])
OPTIONS = {
    'range': dict(clip_to_input_range=True),
    'factor': dict(factor=FACTOR),
    'scalar_factor': dict(factor=3.0),
    'norm': dict(norm=NORM),
    'norm_clip': dict(norm=NORM + (True,)),
    'negative': dict(clip_negative=True),
    'propagate': dict(nan_policy='propagate'),
    'all': dict(clip_to_input_range=True, factor=FACTOR, norm=NORM + (True,), clip_negative=True, nan_policy='propagate'),
    'all_zero': dict(clip_to_input_range=True, factor=FACTOR, norm=NORM, clip_negative=True, nan_policy='zero'),
}


def _holed(shape):
    img = np.array(pr.case_image(shape, 3))
    img[0, 3, 4] = np.nan
    img[0, shape[0] - 1, shape[1] - 1] = np.inf
    img[1, shape[0] // 2, 1 + shape[1] // 3] = -np.inf
    img[2, 0, 0] = np.nan
    img[2, 10:12, 20:23] = np.nan
    return img


@pytest.mark.parametrize('order', [0, 1, 3, 4])
@pytest.mark.parametrize('option', list(OPTIONS))
def test_epilogue_matches_the_restatement(option, order):
    case = CASES[0]
    img = _holed(case['wcs']['shape'])
    kw = {**PLAIN, **OPTIONS[option]}
    got, _ = _run(case, img, order, **kw)
    _, (matrix, offset) = pr.case_matrix(case)
    want, want32 = pr.prepare(img, matrix, offset, case['out_shape'], order, **kw)
    scale = np.full((3, 1, 1), float(np.abs(img[np.isfinite(img)]).max()))
    scale = scale * np.abs(np.broadcast_to(np.asarray(kw.get('factor', 1.0), dtype=np.float64), (3,))).reshape(3, 1, 1)
    if 'norm' in kw:
        scale = scale / np.abs(np.asarray(kw['norm'][1]) - np.asarray(kw['norm'][0])).reshape(3, 1, 1)
    ratio = pr.gate(got, want, np.broadcast_to(scale, want.shape)[~np.isnan(want)])
    n_nan = int(np.isnan(got).sum())
    print(f'{option} order {order}: ratio {ratio:.4f}, {n_nan} NaN pixels, {int((_bits(got) != _bits(want32)).sum())} values differ in bits')
    assert ratio <= 1.0
    if kw.get('nan_policy', 'zero') == 'zero':
        assert np.isfinite(got).all()
    else:
        assert n_nan > 0 and np.array_equal(np.isnan(got), pr.nan_footprint(img, matrix, offset, case['out_shape'], order))
    if kw.get('clip_negative'):
        assert not (got < 0).any()
    if option == 'range':          # the spike plane rings: without the clip it leaves the input's range
        plain, _ = _run(case, img, order, **PLAIN)
        assert got[1].min() >= MISSING and got[1].max() <= 999.0
        assert order < 2 or plain[1].min() < MISSING


def test_non_finite_results_become_zero():
    case = CASES[2]
    img = pr.case_image(case['wcs']['shape'], 3)
    got, _ = _run(case, img, 3, **{**PLAIN, 'factor': [float('inf'), 1e38, 1.0], 'norm': ([0.0, 0.0, 5.0], [1.0, 1e-3, 5.0])})
    assert np.isfinite(got).all() and not got[0].any() and not got[2].any()


@pytest.mark.parametrize('option', ['all', 'all_zero'])
def test_reruns_and_batches_give_the_same_bits(option):
    case = next(c for c in CASES if c['name'] == f'x{2 * prep.SEGMENT + 1}')
    img = _holed(case['wcs']['shape'])
    kw = {**PLAIN, **OPTIONS[option], 'percentile_clip': 2.0}
    for order in (1, 3, 5):
        a, _ = _run(case, img, order, **kw)
        b, _ = _run(case, img, order, **kw)
        assert np.array_equal(_bits(a), _bits(b))
        for k in range(3):
            one = {**kw, 'factor': FACTOR[k], 'norm': tuple(v[k] if isinstance(v, list) else v for v in kw['norm'])}
            alone, _ = _run(case, img[k:k + 1], order, **one)
            assert np.array_equal(_bits(alone[0]), _bits(a[k])), (order, k)


# ---- order statistics and percentiles ---------------------------------------------------------------------------------------------
def _values(n, seed):
    rng = np.random.default_rng(seed)
    x = (rng.standard_normal(n) * 50).astype(np.float32)
    if n >= 255:
        x[rng.integers(0, n, n // 5)] = np.float32(7.25)                     # ties
        x[5:9] = [0.0, -0.0, 0.0, -0.0]
        x[9:13] = np.array([1e-45, -1e-45, 3e-39, -3e-39], dtype=np.float32)   # denormals
        x[13] = -np.inf
        x[20:20 + 3 + seed] = np.nan
        x[40] = np.array([0xFFC00000], dtype=np.uint32).view(np.float32)[0]      # a negative NaN
        if n > 60000:
            x[14] = np.inf
    return x


def _same_value(a, b):
    return np.array_equal(_bits(a), _bits(b)) or (np.all(np.asarray(a) == 0) and np.all(np.asarray(b) == 0))


@pytest.mark.parametrize('n', [1, 2, 255, 256, 257, 65537])
def test_plane_quantiles(n):
    x = np.stack([_values(n, 0), _values(n, 1)])
    if n == 2:
        x[1, 0] = np.nan
    dev = _gpu(x)
    ranks, srt = [], []
    for p in x:
        v, n_nan = pr.sorted_valid(p)
        pos = (v.size - 1) * (99.75 / 100)
        ranks.append([0, v.size - 1, int(np.floor(pos)), min(int(np.floor(pos)) + 1, v.size - 1)])
        srt.append((v, n_nan))
    got, nan_count = prep.order_statistics(dev, torch.tensor(ranks))
    got, nan_count = got.cpu().numpy(), nan_count.cpu().numpy()
    for p in range(2):
        v, n_nan = srt[p]
        print(f'n {n} plane {p}: {n_nan} NaNs, ranks {ranks[p]} -> {got[p].tolist()}')
        assert nan_count[p] == n_nan
        for k, r in enumerate(ranks[p]):
            assert _same_value(got[p, k], v[r]), (p, r, got[p, k], v[r])
    # a rank outside the valid ones answers NaN
    out, _ = prep.order_statistics(dev, torch.tensor([[-1, n], [srt[1][0].size, 0]]))
    out = out.cpu().numpy()
    assert np.isnan(out[0]).all() and np.isnan(out[1, 0]) and _same_value(out[1, 1], srt[1][0][0])
    # the percentile: within one fp32 ulp of np.percentile's value cast to fp32
    for q in (99.75, 50.0, 0.0, 100.0, 12.5):
        thr = prep.plane_quantiles(dev, q).cpu().numpy()
        assert thr.shape == (2, 1)
        for p in range(2):
            want = pr.percentile(x[p], q)
            ulps = abs(int(_bits(thr[p, 0])[0]) - int(_bits(want)[0])) if np.isfinite(want) else 0
            print(f'n {n} plane {p} q {q}: {thr[p, 0]!r} against {want!r}: {ulps} ulp')
            if np.isfinite(want):
                assert np.isfinite(thr[p, 0]) and (ulps <= 1 or (thr[p, 0] == 0 and want == 0))
            else:
                assert _same_value(thr[p, 0], want) or (np.isnan(thr[p, 0]) and np.isnan(want))


def test_percentile_clip_of_a_prepared_image():
    case = CASES[1]
    img = _holed(case['wcs']['shape'])
    for policy in ('zero', 'propagate'):
        kw = {**PLAIN, 'nan_policy': policy}
        plain, _ = _run(case, img, 3, **kw)
        got, _ = _run(case, img, 3, **kw, percentile_clip=0.25)
        for k in range(3):
            thr = pr.percentile(plain[k], 99.75)
            got_thr = np.nanmax(got[k])
            ulps = abs(int(_bits(got_thr)[0]) - int(_bits(thr)[0]))
            print(f'{policy} plane {k}: clipped at {got_thr!r}, np.percentile {thr!r}: {ulps} ulp')
            assert ulps <= 1
            want = np.where(plain[k] > got_thr, got_thr, plain[k])
            assert np.array_equal(_bits(got[k]), _bits(want))


# ---- round trip -------------------------------------------------------------------------------------------------------------------
def _scene(tx, ty):
    """A limb-darkened disk of 960 arcsec and three Gaussian blobs, in helioprojective angles [arcsec]."""
    r2 = (tx ** 2 + ty ** 2) / 960.0 ** 2
    mu = np.sqrt(np.clip(1.0 - r2, 0.0, None))
    v = np.where(r2 < 1.0, 0.4 + 0.6 * mu, 0.0) * 0.5 / (1.0 + np.exp((np.sqrt(r2) - 1.0) * 40.0)) * 2.0
    for bx, by, sig, amp in ((300.0, 200.0, 90.0, 0.8), (-500.0, -100.0, 140.0, 0.5), (100.0, -650.0, 70.0, 0.6)):
        v = v + amp * np.exp(-((tx - bx) ** 2 + (ty - by) ** 2) / (2 * sig ** 2))
    return v


def _detector(n=96, cdelt=25.0, crota=0.4, crpix=(44.3, 51.8)):
    wcs = {'shape': (n, n), 'cdelt': (cdelt, cdelt), 'crpix': crpix, 'crval': (0.0, 0.0), 'crota': crota}
    x, y = np.meshgrid(np.arange(1, n + 1) - crpix[0], np.arange(1, n + 1) - crpix[1])
    pc = pr.pc_matrix(wcs)
    tx = cdelt * (pc[0, 0] * x + pc[0, 1] * y)
    ty = cdelt * (pc[1, 0] * x + pc[1, 1] * y)
    return wcs, _scene(tx, ty).astype(np.float32)


def test_round_trip_through_the_observation_set():
    from sunerf_hip.observations import ObservationSet
    wcs, image = _detector()
    kw = dict(target_scale=30.0, out_shape=(72, 72), order=3, norm=(0.0, 2.0))
    prepared, grid = prep.prepare_image(_gpu(image), wcs, **kw)
    assert grid == {'shape': (72, 72), 'cdelt': (30.0, 30.0), 'crpix': (36.5, 36.5), 'crval': (0.0, 0.0)}
    ax = 30.0 * (np.arange(1, 73) - 36.5)
    direct = _scene(*np.meshgrid(ax, ax)) / 2.0
    got = prepared[0].cpu().numpy().astype(np.float64)
    inside = pr.resample(np.ones((1, 96, 96)), *pr.scipy_matrix(wcs, grid), (72, 72), 0, missing=0.0)[0] > 0
    mse = ((got - direct)[inside] ** 2).mean()
    print(f'round trip: PSNR {10 * np.log10(direct.max() ** 2 / mse):.2f} dB against the scene sampled on the output grid '
          f'({int(inside.sum())} of {inside.size} pixels inside the detector)')

    sets = []
    for prepared_first in (True, False):
        obs = ObservationSet(device='cuda')
        for k in range(4):
            lat, lon = 0.05 * k, 0.6 * k
            w, img = _detector(crota=0.4 - 0.3 * k, crpix=(44.3 + k, 51.8 - k))
            if prepared_first:
                obs.add_prepared_view(img, w, lat, lon, time=float(k), **kw)
            else:
                p, g = prep.prepare_image(_gpu(img), w, **kw)
                obs.add_view(p, lat, lon, time=float(k), grid=g)
        sets.append(obs)
    pools = [s.pool(batch_size=512, seed=3) for s in sets]
    assert pools[0].data.keys() == pools[1].data.keys() and len(sets[0].views) == 4
    for k in pools[0].data:
        assert torch.equal(pools[0].data[k].view(torch.int32), pools[1].data[k].view(torch.int32)), k
    assert sets[0].views[0].grid == sets[1].views[0].grid
    sets[0].hold_out('reference')
    pred = sets[0].baseline_view(shape=(91, 181))
    assert pred.shape == (72, 72, 1) and pred.is_cuda and bool(torch.isfinite(pred).any())
