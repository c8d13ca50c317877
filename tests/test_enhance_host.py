"""CPU-only checks of the enhancement filters (no GPU): the sixteenth entry-point table (declared, bound, versioned,
its argument checks in their documented order), the wrapper's refusals, the geometry helpers, and the NumPy restatement
tests/enhance_reference.py against what it has to be: scipy's ``gaussian_filter(mode='nearest')`` on a mask-free plane, a brute-force
two-dimensional loop on a plane with NaNs, the rules of the header one by one, and a closed radial scene (a rho^-3 fall-off times
1 + 0.2 cos 3 phi) whose ring means span decades before NRGF and are 0 with unit spread and one modulation amplitude after it.  The
radial cases of tests/test_gpu_enhance.py live here (``RADIAL_CASES``); none of them may leave a pixel undecidable.  Every figure
is printed."""
import ctypes
import os

import numpy as np
import pytest
import torch

import enhance_reference as er

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope='session')
def lib():
    import sunerf_hip
    if not os.path.exists(sunerf_hip.LIB_PATH):
        import subprocess
        subprocess.check_call(['bash', os.path.join(ROOT, '2024-hl-spi3s-sunerf_amd', 'csrc', 'build.sh')])
    return sunerf_hip.load()


# ---- the radial cases of the GPU tests ---------------------------------------------------------------------------------------------
def _scene(shape, center, seed):
    """A fall-off around ``center`` with structure: positive, spanning decades, float32."""
    rng = np.random.default_rng(seed)
    d2, dy, dx = er.squared_distance(shape[1:], center)
    rho = np.sqrt(d2) + 1.0
    planes = np.stack([(p + 1.0) * 1e3 * rho ** -2.5 * (1.0 + 0.2 * np.cos(3.0 * np.arctan2(dy, dx) + p)) for p in range(shape[0])])
    return (planes * (1.0 + 0.05 * rng.standard_normal(shape))).astype(np.float32)


def _flag(planes, seed):
    """NaN, an inf and flagged pixels: returns (planes, bad)."""
    rng = np.random.default_rng(seed)
    planes = planes.copy()
    planes[rng.random(planes.shape) < 0.04] = np.nan
    planes.reshape(-1)[5] = np.inf
    planes[:, 3:6, 2:30] = np.nan
    bad = (rng.random(planes.shape) < 0.05).astype(np.uint8)
    return planes, bad


# name -> (shape [C, H, W], centre, edges, n_segments, with invalid pixels).  Fractional centres whose sum and difference are no
# whole numbers either: no pixel sits on a segment boundary (0, 45, 90 ... degrees are the only rational directions that can).
RADIAL_CASES = {
    'one_ring': ((2, 37, 41), (17.3, 20.6), [3.0, 15.0], 1, False),
    'thin_rings': ((1, 33, 35), (16.3, 17.6), np.linspace(2.0, 14.0, 1201), 1, False),          # 0.01 pixel: most bins are empty
    'centre_outside': ((2, 40, 30), (-25.7, 60.4), np.linspace(30.0, 90.0, 13), 1, False),
    'segments_7': ((1, 45, 50), (22.3, 24.6), [2.0, 8.0, 14.0, 20.0], 7, False),
    'segments_360': ((1, 64, 64), (10.3, 12.6), [5.0, 30.0, 70.0], 360, False),
    'rings_4096': ((1, 64, 64), (31.3, 32.6), np.linspace(0.0, 48.0, 4097), 1, False),
    'bins_65536': ((1, 64, 64), (31.3, 32.6), np.linspace(0.0, 48.0, 4097), 16, False),
    'invalid': ((2, 50, 47), (24.3, 21.6), np.linspace(1.5, 30.0, 9), 1, True),
    'invalid_segments': ((2, 50, 47), (24.3, 21.6), np.linspace(1.5, 30.0, 9), 7, True),
    'long_rows': ((1, 9, 700), (4.3, 350.6), [0.0, 100.0, 340.0, 360.0], 3, False),          # a row interval longer than one staging of 256 pixels
}


def radial_case(name):
    shape, center, edges, n_segments, invalid = RADIAL_CASES[name]
    planes = _scene(shape, center, len(name))
    bad = None
    if invalid:
        planes, bad = _flag(planes, len(name) + 1)
    return planes, bad, center, np.asarray(edges, dtype=np.float64), n_segments


# ---- the sixteenth table ---------------------------------------------------------------------------------------------------------
def test_entry_points_are_declared_and_bound(lib):
    """(The table itself -- declared, bound, frozen, versioned, built: tests/test_abi_tables_host.py.)"""
    from sunerf_hip import enhance as wrapper
    header = open(os.path.join(ROOT, 'include', 'sunerf_hip_enhance.h')).read()
    assert lib.sunerf_enhance_abi_version() == 1
    for define in ('SUNERF_ENHANCE_ABI_VERSION 1', 'SUNERF_ENHANCE_MAX_SCALES 8', 'SUNERF_ENHANCE_MAX_RADIUS 128', 'SUNERF_ENHANCE_MGN_STATE 3',
                   'SUNERF_ENHANCE_NRGF_STATE 3', 'SUNERF_ENHANCE_MAX_RINGS 4096', 'SUNERF_ENHANCE_MAX_SEGMENTS 360',
                   'SUNERF_ENHANCE_MAX_BINS 65536', 'SUNERF_ENHANCE_ROW_TILE_Y 4', 'SUNERF_ENHANCE_ROW_TILE_X 512',
                   'SUNERF_ENHANCE_COL_TILE_Y 128', 'SUNERF_ENHANCE_COL_TILE_X 32', 'SUNERF_ENHANCE_OUTSIDE_KEEP 0',
                   'SUNERF_ENHANCE_OUTSIDE_MISSING 1'):
        assert f'#define {define}' in header, define
    assert (wrapper.MAX_SCALES, wrapper.MAX_RADIUS, wrapper.MAX_RINGS, wrapper.MAX_SEGMENTS, wrapper.MAX_BINS) == (8, 128, 4096, 360, 65536)
    assert wrapper.ROW_TILE == (4, 512) and wrapper.COL_TILE == (128, 32) and wrapper.OUTSIDE_MODES == {'keep': er.KEEP, 'missing': er.MISSING}
    assert wrapper.DEFAULT_SIGMA == er.DEFAULT_SIGMA == (1.25, 2.5, 5.0, 10.0, 20.0, 40.0)
    # the workspace: 32 bytes per plane and four fp32 planes, each part rounded up to 256 bytes
    assert lib.sunerf_enhance_mgn_workspace_bytes(3, 150, 300) == 256 + 4 * 540160 and lib.sunerf_enhance_mgn_workspace_bytes(1, 1, 1) == 5 * 256
    assert lib.sunerf_enhance_mgn_workspace_bytes(0, 5, 5) == 0 and lib.sunerf_enhance_mgn_workspace_bytes(2, -1, 5) == 0


def check_argument_order(lib):
    """Each entry point refuses in the order its header gives, before anything touches a device, so this runs without one.  ``Q``
    stands for any non-null pointer aligned to 256 bytes: no call here reaches a launch."""
    Q = lambda i: ctypes.c_void_p((1 << 20) * (i + 1))          # noqa: E731
    nan, inf = float('nan'), float('inf')

    # ---- sunerf_enhance_mgn
    names = ('image', 'out', 'lo_out', 'hi_out', 'state', 'workspace')
    P = {k: Q(i) for i, k in enumerate(names)}
    none = {k: None for k in names}

    def mgn(c=2, h=9, w=11, sigma=(1.25, 40.0), weights=None, n=None, truncate=3.0, k=0.7, gamma=3.2, hh=0.7, lo=None, hi=None, floor=None,
            bad=None, ws_bytes=0, **ptrs):
        p = dict(P)
        p.update(ptrs)
        sig = None if sigma is None else (ctypes.c_double * len(sigma))(*sigma)
        wts = None if weights is None else (ctypes.c_float * len(weights))(*weights)
        return lib.sunerf_enhance_mgn(p['image'], bad, c, h, w, sig, wts, len(sigma) if n is None else n, truncate, k, gamma, hh, lo, hi, floor,
                                      p['out'], p['lo_out'], p['hi_out'], p['state'], p['workspace'], ws_bytes, None)
    for count in (0, -1, 9):
        assert mgn(n=count, **none) == -2 and mgn(n=count, c=-1, sigma=None, **none) == -2, count          # the number of scales comes first
    assert mgn(sigma=None, n=2, **none) == -1 and mgn(sigma=None, n=2, c=0, **none) == -1
    for wrong in (dict(sigma=(1.0, nan)), dict(sigma=(inf,)), dict(sigma=(-1.0,)), dict(truncate=nan), dict(truncate=inf), dict(truncate=-0.5)):
        assert mgn(**wrong, **none) == -1 and mgn(**wrong, c=0, **none) == -1, wrong
    for wide in (dict(sigma=(43.0,)), dict(sigma=(1.0, 1e300)), dict(sigma=(10.0,), truncate=13.0)):          # radius 129, huge, 130
        assert mgn(**wide, **none) == -2 and mgn(**wide, h=0, **none) == -2, wide
    assert mgn(sigma=(42.83,), ws_bytes=0) == -3 and mgn(sigma=(0.0,), ws_bytes=0) == -3                      # radius 128 and 0 pass
    for empty in (dict(c=0), dict(h=0), dict(w=0), dict(c=0, h=0, w=0)):
        assert mgn(**empty, **none) == 0 and mgn(**empty, k=nan, gamma=-1.0, **none) == 0, empty                # the empty call, before k and gamma
    assert mgn(c=-1) == -1 and mgn(h=-1) == -1 and mgn(w=-1) == -1 and mgn(c=-1, h=0) == -1
    assert mgn(c=65536) == -1 and mgn(h=4 * 65535 + 1) == -1
    for wrong in (dict(k=nan), dict(k=inf), dict(hh=nan), dict(gamma=0.0), dict(gamma=-1.0), dict(gamma=nan), dict(gamma=inf),
                  dict(weights=(1.0, inf)), dict(weights=(nan, 1.0))):
        assert mgn(**wrong) == -1, wrong
    for k in names:
        assert mgn(**{k: None}) == -1, k
        assert mgn(**{k: ctypes.c_void_p(P[k].value + 2)}) == -1, k
    assert mgn(state=ctypes.c_void_p(P['state'].value + 4)) == -1 and mgn(workspace=ctypes.c_void_p(P['workspace'].value + 128)) == -1
    for k in ('lo', 'hi', 'floor'):
        assert mgn(**{k: ctypes.c_void_p((1 << 26) + 2)}) == -1, k
    need = lib.sunerf_enhance_mgn_workspace_bytes(2, 9, 11)
    assert need == 256 + 4 * 1024 and mgn(ws_bytes=need - 1) == -3 and mgn(ws_bytes=0, bad=Q(9), lo=Q(10), hi=Q(11), floor=Q(12)) == -3
    assert all(mgn(c=c, h=h, w=w, sigma=s, truncate=t, k=k, **none) == -1
               for c, h, w, s, t, k in ((1, 1, 1, (0.0,), 0.0, 0.0), (65535, 4 * 65535, 7, (32.0,) * 8, 4.0, -3.0), (3, 150, 300, er.DEFAULT_SIGMA, 3.0, 0.7)))

    # ---- sunerf_enhance_radial_statistics
    names = ('image', 'edges', 'count', 'mean', 'std', 'min', 'max')
    P = {k: Q(i) for i, k in enumerate(names)}
    none = {k: None for k in names}

    def stats(c=2, h=9, w=11, cy=4.3, cx=5.6, rings=5, segments=1, bad=None, **ptrs):
        p = dict(P)
        p.update(ptrs)
        return lib.sunerf_enhance_radial_statistics(p['image'], bad, c, h, w, cy, cx, p['edges'], rings, segments, p['count'], p['mean'], p['std'],
                                                    p['min'], p['max'], None)
    for limit in (dict(rings=0), dict(rings=-1), dict(rings=4097), dict(segments=0), dict(segments=361), dict(rings=4096, segments=17),
                  dict(rings=183, segments=360)):
        assert stats(**limit, **none) == -2 and stats(**limit, c=0, **none) == -2 and stats(**limit, h=-1, **none) == -2, limit
    for empty in (dict(c=0), dict(h=0), dict(w=0)):
        assert stats(**empty, **none) == 0 and stats(**empty, cy=nan, **none) == 0, empty
    assert stats(c=-1) == -1 and stats(h=-1) == -1 and stats(w=-1, c=0) == -1 and stats(c=65536) == -1
    for wrong in (dict(cy=nan), dict(cx=inf), dict(cy=-2.0 ** 31), dict(cx=2.0 ** 30 + 1)):
        assert stats(**wrong) == -1, wrong
    for k in names:
        assert stats(**{k: None}) == -1, k
        assert stats(**{k: ctypes.c_void_p(P[k].value + (2 if k == 'image' else 4))}) == -1, k
    assert all(stats(rings=r, segments=s, cy=cy, **none) == -1 for r, s, cy in ((1, 1, 0.0), (4096, 16, -2.0 ** 30), (182, 360, 2.0 ** 30)))

    # ---- sunerf_enhance_nrgf
    names = ('image', 'edges', 'count', 'mean', 'std', 'min', 'max', 'out', 'state')
    P = {k: Q(i) for i, k in enumerate(names)}
    none = {k: None for k in names}

    def nrgf(c=2, h=9, w=11, cy=4.3, cx=5.6, rings=5, outside=0, missing=0.0, compute=1, bad=None, **ptrs):
        p = dict(P)
        p.update(ptrs)
        return lib.sunerf_enhance_nrgf(p['image'], bad, c, h, w, cy, cx, p['edges'], rings, outside, missing, compute, p['count'], p['mean'],
                                       p['std'], p['min'], p['max'], p['out'], p['state'], None)
    for limit in (dict(rings=0), dict(rings=4097), dict(outside=2), dict(outside=-1)):
        assert nrgf(**limit, **none) == -2 and nrgf(**limit, c=0, **none) == -2 and nrgf(**limit, w=-1, **none) == -2, limit
    for empty in (dict(c=0), dict(h=0), dict(w=0)):
        assert nrgf(**empty, **none) == 0 and nrgf(**empty, cx=nan, missing=nan, **none) == 0, empty
    assert nrgf(c=-1) == -1 and nrgf(h=-1) == -1 and nrgf(w=-1) == -1 and nrgf(c=65536) == -1
    assert nrgf(cy=nan) == -1 and nrgf(cx=-inf) == -1
    for k in names:
        assert nrgf(**{k: None}) == -1, k
        assert nrgf(**{k: ctypes.c_void_p(P[k].value + (2 if k in ('image', 'out') else 4))}) == -1, k
    for k in ('image', 'edges', 'count', 'mean', 'std', 'out', 'state'):          # the caller's statistics: min and max may be NULL, the rest not
        assert nrgf(compute=0, **{**{'min': None, 'max': None}, k: None}) == -1, k
    assert all(nrgf(rings=r, outside=o, compute=cp, missing=nan, **none) == -1 for r, o, cp in ((1, 0, 0), (4096, 1, 1)))


def test_argument_checks_come_in_the_documented_order(lib):
    check_argument_order(lib)


# ---- the wrapper -------------------------------------------------------------------------------------------------------------------
def test_the_wrapper_refuses_before_any_device_work():
    """Every refusal is a ValueError or TypeError that names the argument, raised on CPU tensors: nothing here needs a device."""
    from sunerf_hip import SunerfHipError
    from sunerf_hip import enhance as en
    image = torch.zeros((2, 9, 11))
    for fn, call in (('mgn', lambda im, **kw: en.mgn(im, **kw)), ('radial_statistics', lambda im, **kw: en.radial_statistics(im, (4.3, 5.6), [1.0, 3.0], **kw)),
                     ('nrgf', lambda im, **kw: en.nrgf(im, (4.3, 5.6), [1.0, 3.0], **kw))):
        with pytest.raises(TypeError, match='image'):
            call(np.zeros((2, 9, 11), dtype=np.float32))
        for wrong in (image.double(), image[None], image[0, 0], torch.zeros((0, 9, 11)), torch.zeros((2, 9, 0))):
            with pytest.raises(ValueError, match='image'):
                call(wrong)
        with pytest.raises(TypeError, match='bad'):
            call(image, bad=np.zeros((2, 9, 11), dtype=bool))
        for wrong in (torch.zeros((2, 9, 11)), torch.zeros((2, 9, 10), dtype=torch.bool), torch.zeros((9, 11), dtype=torch.uint8)):
            with pytest.raises(ValueError, match='bad'):
                call(image, bad=wrong)
        with pytest.raises(SunerfHipError, match=fn):          # all arguments fine: only now the device is looked at
            call(image)
    for kw, err, word in ((dict(sigma=()), ValueError, 'sigma'), (dict(sigma=(1.0,) * 9), ValueError, 'sigma'), (dict(sigma=(1.0, -2.0)), ValueError, 'sigma'),
                          (dict(sigma=(float('nan'),)), ValueError, 'sigma'), (dict(sigma='wide'), TypeError, 'sigma'), (dict(sigma=(43.0,)), ValueError, 'radius'),
                          (dict(truncate=-1.0), ValueError, 'truncate'), (dict(truncate='3'), TypeError, 'truncate'), (dict(truncate=50.0), ValueError, 'radius'),
                          (dict(weights=(1.0,)), ValueError, 'weights'), (dict(weights=(1.0,) * 5 + (float('inf'),)), ValueError, 'weights'),
                          (dict(k=float('nan')), ValueError, 'k'), (dict(k=None), TypeError, 'k'), (dict(h=float('inf')), ValueError, 'h'),
                          (dict(gamma=0.0), ValueError, 'gamma'), (dict(gamma=-2.0), ValueError, 'gamma'), (dict(gamma=True), TypeError, 'gamma'),
                          (dict(lo=(1.0, 2.0, 3.0)), ValueError, 'lo'), (dict(hi=float('nan')), ValueError, 'hi'), (dict(floor=-1.0), ValueError, 'floor'),
                          (dict(floor=(0.0, float('inf'))), ValueError, 'floor')):
        with pytest.raises(err, match=word):
            en.mgn(image, **kw)
    for fn in (en.radial_statistics, en.nrgf):
        for center, edges, err, word in (((4.3,), [1.0, 3.0], TypeError, 'center'), (4.3, [1.0, 3.0], TypeError, 'center'), ((float('nan'), 1.0), [1.0, 3.0], ValueError, 'center'),
                                         ((1.0, 2.0 ** 31), [1.0, 3.0], ValueError, 'center'), ((4.3, 5.6), [1.0], ValueError, 'edges'),
                                         ((4.3, 5.6), [[1.0, 3.0]], ValueError, 'edges'), ((4.3, 5.6), [-1.0, 3.0], ValueError, 'edges'),
                                         ((4.3, 5.6), [1.0, 3.0, 3.0], ValueError, 'edges'), ((4.3, 5.6), [1.0, float('inf')], ValueError, 'edges'),
                                         ((4.3, 5.6), np.arange(4098.0), ValueError, 'edges')):
            with pytest.raises(err, match=word):
                fn(image, center, edges)
    for segments, err in ((0, ValueError), (361, ValueError), (2.0, TypeError), (True, TypeError)):
        with pytest.raises(err, match='n_segments'):
            en.radial_statistics(image, (4.3, 5.6), [1.0, 3.0], n_segments=segments)
    with pytest.raises(ValueError, match='n_segments'):
        en.radial_statistics(image, (4.3, 5.6), np.arange(4097.0), n_segments=17)
    with pytest.raises(ValueError, match='outside'):
        en.nrgf(image, (4.3, 5.6), [1.0, 3.0], outside='nan')
    with pytest.raises(TypeError, match='missing'):
        en.nrgf(image, (4.3, 5.6), [1.0, 3.0], missing='nan')
    table = {'count': torch.zeros((2, 1), dtype=torch.int64), 'mean': torch.zeros((2, 1), dtype=torch.float64), 'std': torch.ones((2, 1), dtype=torch.float64)}
    for wrong, err in (((1, 2), TypeError), ({'count': table['count']}, TypeError), ({**table, 'mean': table['mean'].float()}, TypeError),
                       ({**table, 'std': torch.ones((2, 2), dtype=torch.float64)}, ValueError), ({**table, 'count': torch.zeros((1, 2), dtype=torch.int64)}, ValueError)):
        with pytest.raises(err, match='statistics'):
            en.nrgf(image, (4.3, 5.6), [1.0, 3.0], statistics=wrong)
    with pytest.raises(SunerfHipError, match='nrgf'):
        en.nrgf(image, (4.3, 5.6), [1.0, 3.0], statistics=table)


def test_sun_geometry_and_radial_edges():
    from sunerf_hip import enhance as en
    from sunerf_hip.reprojection import Observer
    pitch, distance = 2.5e-5, 215.0
    tx = (np.arange(64) - 30.25) * pitch
    ty = -(np.arange(48) - 20.5) * pitch                    # a descending axis
    center, per_radius = en.sun_geometry(Observer(0.1, 0.2, distance, tx=tx, ty=ty))
    print(f'sun_geometry: centre {center}, {per_radius:.6f} pixels per radius')
    assert abs(center[0] - 20.5) < 1e-9 and abs(center[1] - 30.25) < 1e-9
    assert abs(per_radius - np.arcsin(1.0 / distance) / pitch) < 1e-9 * per_radius
    assert abs(en.sun_geometry(Observer(0.1, 0.2, distance, tx=tx, ty=ty), Rs_per_ds=0.5)[1] - np.arcsin(2.0 / distance) / pitch) < 1e-9 * per_radius
    bent = tx.copy()
    bent[40:] += 0.01 * pitch
    with pytest.raises(ValueError, match='tx'):
        en.sun_geometry(Observer(0.0, 0.0, distance, tx=bent, ty=ty))
    with pytest.raises(ValueError, match='ty'):
        en.sun_geometry(Observer(0.0, 0.0, distance, tx=tx, ty=ty[:1]))
    with pytest.raises(ValueError, match='pitches'):
        en.sun_geometry(Observer(0.0, 0.0, distance, tx=tx, ty=ty * (1.0 + 1e-8)))
    en.sun_geometry(Observer(0.0, 0.0, distance, tx=tx, ty=ty * (1.0 + 1e-10)))
    with pytest.raises(ValueError, match='inside'):
        en.sun_geometry(Observer(0.0, 0.0, 0.9, tx=tx, ty=ty))
    edges = en.radial_edges(1.5, 6.0, 9, per_radius)
    assert edges.shape == (10,) and abs(edges[0] - 1.5 * per_radius) < 1e-9 and abs(edges[-1] - 6.0 * per_radius) < 1e-9
    assert np.allclose(np.diff(edges), 0.5 * per_radius)
    for args, err in (((2.0, 1.0, 4, 10.0), ValueError), ((-1.0, 1.0, 4, 10.0), ValueError), ((1.0, 2.0, 0, 10.0), ValueError), ((1.0, 2.0, 4097, 10.0), ValueError),
                      ((1.0, 2.0, 4.0, 10.0), TypeError), ((1.0, 2.0, 4, 0.0), ValueError), ((1.0, float('nan'), 4, 10.0), ValueError)):
        with pytest.raises(err):
            en.radial_edges(*args)


# ---- the restatement: MGN ----------------------------------------------------------------------------------------------------------
def test_the_window_is_scipys_gaussian_filter():
    """Exact fp64 weights, no mask: G equals ``scipy.ndimage.gaussian_filter(mode='nearest', truncate=...)`` to 1e-12 relative."""
    from scipy.ndimage import gaussian_filter
    rng = np.random.default_rng(11)
    plane = 3.0 + rng.standard_normal((23, 31))
    worst = 0.0
    for sigma, truncate in ((1.25, 3.0), (2.5, 3.0), (5.0, 4.0), (40.0, 3.0), (0.7, 2.0), (3.3, 1.7)):
        w = er.taps(sigma, truncate, exact=True)
        assert w.shape[0] == 2 * int(truncate * sigma + 0.5) + 1
        got = er.gaussian(plane, np.ones(plane.shape), w)
        want = gaussian_filter(plane, sigma, mode='nearest', truncate=truncate)
        worst = max(worst, float((np.abs(got - want) / np.abs(want)).max()))
    print(f'G against scipy.ndimage.gaussian_filter: worst relative difference {worst:.2e}')
    assert worst <= 1e-12
    rounded = er.taps(5.0, 3.0)
    assert np.array_equal(rounded, rounded.astype(np.float32).astype(np.float64)) and rounded[15] == 1.0 and np.array_equal(rounded, rounded[::-1])


def test_the_normalised_window_is_the_brute_force_loop():
    rng = np.random.default_rng(12)
    plane = rng.standard_normal((13, 17))
    plane[0, 0] = plane[12, 16] = plane[5, 3:12] = np.nan
    plane[7:11, 8] = np.inf
    bad = np.zeros(plane.shape, dtype=np.uint8)
    bad[2, 2] = 1
    mask = er.validity(plane, bad).astype(np.float64)
    w = er.taps(1.25, 3.0)
    r = (w.shape[0] - 1) // 2
    got = er.gaussian(plane, mask, w)
    hgt, wid = plane.shape
    want = np.zeros(plane.shape)
    for y in range(hgt):
        for x in range(wid):
            num = den = 0.0
            for j in range(-r, r + 1):
                for i in range(-r, r + 1):
                    yy, xx = min(max(y + j, 0), hgt - 1), min(max(x + i, 0), wid - 1)          # a replicated tap is as valid as its pixel
                    if mask[yy, xx]:
                        num += w[j + r] * w[i + r] * plane[yy, xx]
                        den += w[j + r] * w[i + r]
            want[y, x] = num / den
    err = float(np.abs(got - want).max())
    print(f'normalised window against the 2-D loop: {err:.2e}')
    assert np.isfinite(got).all() and err <= 1e-13


def test_the_rules_of_mgn_one_by_one():
    rng = np.random.default_rng(13)
    planes = (10.0 + rng.standard_normal((1, 12, 14))).astype(np.float32)
    # R = 0: the window is the pixel, r = 0 and every t_i = 0: the result is the gamma term alone
    out, lo, hi, state, detail = er.mgn(planes, sigma=(0.0, 0.1), truncate=3.0)
    assert er.radius_of(0.1, 3.0) == 0 and not detail['t'].any()
    g = ((planes.astype(np.float64) - float(lo[0])) / (float(hi[0]) - float(lo[0]))) ** float(np.float32(1.0 / np.float32(3.2)))
    assert np.allclose(out, float(np.float32(0.7)) * g, rtol=0, atol=1e-15) and state.tolist() == [[0, 0, 0]]
    assert lo[0] == planes.min() and hi[0] == planes.max()
    # a constant plane blurs to itself up to rounding; hi == lo: no gamma term
    out, lo, hi, state, detail = er.mgn(np.full((1, 9, 40), 5.0, dtype=np.float32))
    print(f'constant plane: max |out| {np.abs(out).max():.2e}')
    assert lo[0] == hi[0] == 5.0 and np.abs(out).max() < 1e-9 and state.tolist() == [[0, 0, 0]]
    # an all-zero plane: floor 0, s = 0, t = 0 by the rule, not 0 / 0
    out, lo, hi, state, detail = er.mgn(np.zeros((1, 6, 7), dtype=np.float32))
    assert not out.any() and np.isfinite(out).all() and lo[0] == hi[0] == 0.0 and not np.signbit(lo[0])
    out, lo, hi, _, _ = er.mgn(np.full((1, 6, 7), -0.0, dtype=np.float32))
    assert not np.signbit(lo[0]) and not np.signbit(hi[0]) and not out.any()
    # a plane without a valid pixel is NaN throughout, and so are its lo and hi -- beside a plane that has some
    both = np.concatenate([np.full((1, 12, 14), np.nan, dtype=np.float32), planes])
    both[1, 3, 4] = np.inf
    out, lo, hi, state, detail = er.mgn(both, lo=1.0)
    assert np.isnan(out[0]).all() and np.isnan(lo[0]) and np.isnan(hi[0]) and state[0].tolist() == [168, 0, 0]
    assert np.isnan(out[1]).sum() == 1 and np.isnan(out[1, 3, 4]) and lo[1] == 1.0 and state[1].tolist() == [1, 0, 0]
    # hi <= lo: g = 0, the result is the normalised part alone; every valid pixel is below lo or above hi or neither
    out, lo, hi, state, detail = er.mgn(planes, sigma=(1.25, 2.5), lo=11.0, hi=9.0)
    want = float(np.float32((1.0 - float(np.float32(0.7))) / 2))
    assert np.allclose(out, want * detail['t'].sum(0), rtol=0, atol=1e-15)
    assert state[0].tolist() == [0, int((planes < 11.0).sum()), int((planes > 9.0).sum())]
    # bad flags a pixel like a NaN does
    bad = np.zeros(planes.shape, dtype=np.uint8)
    bad[0, 5, 5] = 1
    holed = planes.copy()
    holed[0, 5, 5] = np.nan
    a, b = er.mgn(planes, bad=bad, lo=8.0, hi=12.0), er.mgn(holed, lo=8.0, hi=12.0)
    assert np.array_equal(a[0], b[0], equal_nan=True) and np.isnan(a[0][0, 5, 5]) and a[3].tolist() == b[3].tolist() and a[3][0, 0] == 1
    # the bound is finite above the floor and gives up (pi per scale) only below it
    out, _, _, _, detail = er.mgn(planes)
    assert np.isfinite(detail['bound']).all() and detail['bound'].max() < 1e-3


# ---- the restatement: rings ----------------------------------------------------------------------------------------------------------
def test_membership_and_statistics_are_the_plain_loop():
    planes, bad, center, edges, n_segments = radial_case('invalid_segments')
    count, mean, std, mn, mx, detail = er.radial_statistics(planes, center, edges, n_segments, bad)
    c, hgt, wid = planes.shape
    values = [[[[] for _ in range(n_segments)] for _ in range(len(edges) - 1)] for _ in range(c)]
    for y in range(hgt):
        for x in range(wid):
            d2 = (y - center[0]) ** 2 + (x - center[1]) ** 2
            ring = [i for i in range(len(edges) - 1) if edges[i] ** 2 <= d2 < edges[i + 1] ** 2]
            assert (ring[0] if ring else -1) == detail['ring'][y, x]
            if not ring:
                continue
            seg = min(int(np.floor((np.arctan2(y - center[0], x - center[1]) + np.pi) / (2 * np.pi) * n_segments)), n_segments - 1)
            assert seg == detail['segment'][y, x]
            for p in range(c):
                if np.isfinite(planes[p, y, x]) and not bad[p, y, x]:
                    values[p][ring[0]][seg].append(float(planes[p, y, x]))
    assert (detail['ring'] >= 0).sum() > 1000 and (detail['ring'] < 0).sum() > 50
    for p in range(c):
        for i in range(len(edges) - 1):
            for s in range(n_segments):
                v = np.asarray(values[p][i][s])
                assert count[p, i, s] == v.size
                if v.size:
                    assert mn[p, i, s] == v.min() and mx[p, i, s] == v.max()
                    assert abs(mean[p, i, s] - v.mean()) <= detail['mean_bound'][p, i, s] and abs(std[p, i, s] - v.std()) <= detail['std_bound'][p, i, s]
                else:
                    assert np.isnan([mean[p, i, s], std[p, i, s], mn[p, i, s], mx[p, i, s]]).all()
    assert count.sum() == (er.validity(planes, bad) & (detail['ring'] >= 0)).sum()


def test_closed_radial_scene():
    """rho^-3 (1 + 0.2 cos 3 phi) in rings half a pixel wide between 30 and 75 pixels: before the filter the ring means span more
    than a decade; after it every ring has mean 0 and spread 1 to rounding, and a fit of cos 3 phi finds one amplitude -- sqrt 2
    up to the ring's own radial spread -- in every ring."""
    shape, center = (160, 160), (79.3, 80.6)
    d2, dy, dx = er.squared_distance(shape, center)
    phi = np.arctan2(dy, dx)
    planes = (1e6 * np.maximum(d2, 1.0) ** -1.5 * (1.0 + 0.2 * np.cos(3.0 * phi))).astype(np.float32)[None]
    edges = np.linspace(30.0, 75.0, 91)
    out, state, (count, mean, std, mn, mx), detail = er.nrgf(planes, center, edges)
    ring = detail['ring']
    assert mean[0, 0] / mean[0, -1] > 10.0 and count.min() > 80 and state[0].tolist() == [0, int((ring < 0).sum()), 0]
    assert np.array_equal(out[0][ring < 0], planes[0][ring < 0].astype(np.float64))
    amplitude, worst_mean, worst_std = [], 0.0, 0.0
    for i in range(len(edges) - 1):
        v, basis = out[0][ring == i], np.cos(3.0 * phi[ring == i])
        worst_mean, worst_std = max(worst_mean, abs(v.mean())), max(worst_std, abs(v.std() - 1.0))
        amplitude.append(float((v * basis).sum() / (basis * basis).sum()))
    amplitude = np.asarray(amplitude)
    print(f'closed scene: ring means {mean[0, 0]:.3g} .. {mean[0, -1]:.3g}; after NRGF worst |mean| {worst_mean:.2e}, worst |std - 1| {worst_std:.2e}, '
          f'amplitude {amplitude.min():.4f} .. {amplitude.max():.4f}')
    assert worst_mean <= 1e-6 and worst_std <= 1e-6          # fp32 outputs of about 100 pixels: 2^-24 each
    assert np.abs(amplitude - np.sqrt(2.0)).max() <= 0.03 * np.sqrt(2.0)
    # the caller's statistics and outside='missing'
    again, state2, _, _ = er.nrgf(planes, center, edges, outside=er.MISSING, missing=-1.0, statistics=(count, mean, std))
    assert np.array_equal(again[0][ring >= 0], out[0][ring >= 0]) and (again[0][ring < 0] == -1.0).all() and state2.tolist() == state.tolist()


def test_no_radial_case_leaves_a_pixel_undecidable():
    """A pixel whose angle lies within 8 ulp of a segment boundary cannot be held to one segment; at most 2 % of a case may be such,
    and with the fractional centres chosen none is."""
    for name in RADIAL_CASES:
        planes, bad, center, edges, n_segments = radial_case(name)
        ring = er.membership(planes.shape[1:], center, edges)
        if n_segments > 1:
            seg, undecidable = er.segments(planes.shape[1:], center, n_segments)
            share = float(undecidable[ring >= 0].mean())
            print(f'{name}: {int(undecidable.sum())} undecidable pixels, {share:.2%} of those in a ring; segments used {np.unique(seg[ring >= 0]).size} of {n_segments}')
            assert share <= 0.02 and not undecidable.any()
        assert (ring >= 0).any()
    # the rule does find a pixel on a boundary: a whole-number centre puts a row and a column on 0, 90, 180 degrees
    _, undecidable = er.segments((9, 9), (4.0, 4.0), 4)
    assert undecidable[4, 5:].all() and undecidable[:4, 4].all() and not undecidable[1, 2]
