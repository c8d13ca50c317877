"""CPU-only checks of the co-alignment step (no GPU): the twelfth entry-point table (declared, bound, versioned, its
workspace query and its argument checks in their documented order), the wrapper's refusals, the NumPy restatement
tests/coalign_reference.py against ``scipy.signal.correlate2d``, the fp64 torch functions behind the kernel (``scores_from_sums``,
``peak``, ``shifted_grid``) against the restatement, every status bit, and the sub-pixel recovery on an analytic scene.  Every
figure is printed."""
import ctypes
import os

import numpy as np
import pytest
import torch

import coalign_reference as cr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MAX_RUNS = 256          # include/sunerf_hip_coalign.h


@pytest.fixture(scope='session')
def lib():
    import sunerf_hip
    if not os.path.exists(sunerf_hip.LIB_PATH):
        import subprocess
        subprocess.check_call(['bash', os.path.join(ROOT, '2024-hl-spi3s-sunerf_amd', 'csrc', 'build.sh')])
    return sunerf_hip.load()


# ---- the twelfth table ------------------------------------------------------------------------------------------------------------
def test_entry_points_are_declared_and_bound(lib):
    """(The table itself -- declared, bound, frozen, versioned, built: tests/test_abi_tables_host.py.)"""
    header = open(os.path.join(ROOT, 'include', 'sunerf_hip_coalign.h')).read()
    assert lib.sunerf_coalign_abi_version() == 1
    for define in ('SUNERF_COALIGN_MAX_SHIFT 32', 'SUNERF_COALIGN_SUMS 6', 'SUNERF_COALIGN_TILE 32', 'SUNERF_COALIGN_CHUNK 1024',
                   f'SUNERF_COALIGN_MAX_RUNS {MAX_RUNS}'):
        assert f'#define {define}' in header, define
    from sunerf_hip import coalign as wrapper
    assert (wrapper.NO_PEAK, wrapper.EDGE, wrapper.FLAT) == (cr.NO_PEAK, cr.EDGE, cr.FLAT) == (1, 2, 4)
    assert wrapper.MAX_SHIFT == cr.MAX_SHIFT == 32 and wrapper.N_SUMS == 6


def workspace_bytes(n_planes, h, w, my, mx):
    """The header's formula."""
    tiles = -(-h // 32) * -(-w // 32)
    return n_planes * min(tiles, max(1, MAX_RUNS // n_planes)) * (2 * my + 1) * (2 * mx + 1) * 6 * 8


def test_workspace_query(lib):
    q = lib.sunerf_coalign_workspace_bytes
    valid = [(1, 1, 1, 0, 0), (1, 1, 1, 2, 3), (1, 5, 7, 8, 8), (2, 33, 65, 2, 5), (3, 64, 64, 1, 1), (1, 40, 70, 32, 32),
             (16, 96, 192, 2, 2), (7, 1024, 1024, 8, 8), (1, 4096, 4096, 32, 32), (300, 40, 40, 1, 0), (1, 46341, 46341, 0, 0)]
    assert [q(*a) for a in valid] == [workspace_bytes(*a) for a in valid]
    assert q(1, 1, 1, 0, 0) == 48 and q(7, 1024, 1024, 8, 8) == 7 * 36 * 289 * 48 and q(1, 4096, 4096, 32, 32) == 256 * 4225 * 48
    assert q(300, 40, 40, 1, 0) == 300 * 3 * 48          # more planes than runs: one run per plane
    invalid = [(0, 5, 7, 1, 1), (-1, 5, 7, 1, 1), (1, 0, 7, 1, 1), (1, 5, 0, 1, 1), (1, 5, 7, -1, 1), (1, 5, 7, 1, -1), (1, 5, 7, 33, 1),
               (1, 5, 7, 1, 33), (1, -5, 7, 2, 2)]
    assert [q(*a) for a in invalid] == [0] * len(invalid)


def check_argument_order(lib):
    """Limits (-2) first, then the empty call (0), then counts, null pointers, alignment and the overlap of sums with an input
    (-1): all before anything touches a device, so this runs without one.  ``Q`` stands for any non-null aligned pointer: no call
    here reaches a launch."""
    fn = lib.sunerf_coalign_shift_sums
    names = ('image', 'templ', 'sums', 'workspace')
    Q = {k: ctypes.c_void_p(4096 + (1 << 20) * i) for i, k in enumerate(names)}

    def call(n_planes=2, h=9, w=11, my=2, mx=3, bad_image=None, bad_template=None, **ptrs):
        p = dict(Q)
        p.update(ptrs)
        return fn(p['image'], p['templ'], bad_image, bad_template, n_planes, h, w, my, mx, p['sums'], p['workspace'], None)
    none = {k: None for k in names}
    assert call(my=33, **none) == -2 and call(mx=33, **none) == -2
    assert call(my=33, n_planes=0, **none) == -2 and call(mx=33, n_planes=-1, **none) == -2          # the limits come first
    for empty in (dict(n_planes=0), dict(h=0), dict(w=0), dict(h=0, w=0), dict(n_planes=0, my=32, mx=0)):
        assert call(**empty, **none) == 0, empty                                                     # then the empty call
    assert call(n_planes=-1) == -1 and call(h=-1) == -1 and call(w=-1) == -1 and call(n_planes=-1, h=0) == -1
    assert call(my=-1) == -1 and call(mx=-1) == -1 and call(my=-1, n_planes=0) == -1
    for k in names:
        assert call(**{k: None}) == -1, k
    for k in ('sums', 'workspace'):
        assert call(**{k: ctypes.c_void_p(Q[k].value + 4)}) == -1, k
    # sums may not overlap an input: 2 x 9 x 11 floats are 792 bytes (198 bytes of a mask); sums are 2 x 5 x 7 x 48 = 3360 bytes
    for k in ('image', 'templ'):
        assert call(sums=Q[k]) == -1 and call(sums=ctypes.c_void_p(Q[k].value + 784)) == -1, k
        assert call(sums=ctypes.c_void_p(Q[k].value - 3352)) == -1, k
    far = ctypes.c_void_p(Q['sums'].value + (1 << 19))
    for k in ('bad_image', 'bad_template'):
        assert call(**{k: Q['sums']}) == -1 and call(**{k: ctypes.c_void_p(Q['sums'].value + 3359)}) == -1, k
        assert call(**{k: ctypes.c_void_p(Q['sums'].value - 197)}) == -1, k
        assert call(**{k: far}, **none) == -1          # a mask alone changes nothing about the refusals that follow
    # with every pointer null the next refusal is the pointers': all the scalar checks before them pass at the limits
    assert all(call(my=a, mx=b, **none) == -1 for a, b in ((0, 0), (32, 32), (0, 32), (9, 11), (20, 1)))


def test_argument_checks_come_in_the_documented_order(lib):
    check_argument_order(lib)


# ---- the wrapper ------------------------------------------------------------------------------------------------------------------
def test_the_wrapper_refuses_what_it_cannot_run():
    from sunerf_hip import SunerfHipError
    from sunerf_hip.coalign import coalign, peak, scores_from_sums, shift_sums
    x = torch.zeros(2, 9, 11)
    for max_shift in (-1, 33, (1, 33), (1,), (1, 2, 3), 2.5, (1.0, 2), True):
        with pytest.raises(ValueError, match='max_shift'):
            shift_sums(x, x, max_shift)
        print('refused: max_shift', max_shift)
    with pytest.raises(ValueError, match='float32'):
        shift_sums(x.double(), x, 2)
    with pytest.raises(ValueError, match='float32'):
        shift_sums(x, x.double(), 2)
    with pytest.raises(ValueError, match='float32'):
        shift_sums(torch.zeros(2, 2, 9, 11), torch.zeros(2, 2, 9, 11), 2)
    with pytest.raises(ValueError, match="image's shape"):
        shift_sums(x, torch.zeros(2, 9, 10), 2)
    with pytest.raises(ValueError, match='bad_image'):
        shift_sums(x, x, 2, bad_image=torch.zeros(2, 9, 10))
    with pytest.raises(ValueError, match='bad_template'):
        shift_sums(x, x, 2, bad_template=torch.zeros(1, 9, 11))
    with pytest.raises(TypeError):
        shift_sums(x.numpy(), x, 2)
    with pytest.raises(SunerfHipError, match='no CPU path'):          # every argument is in order: only the device is missing
        shift_sums(x, x, (2, 0), bad_image=torch.zeros(2, 9, 11, dtype=torch.bool))
    with pytest.raises(SunerfHipError, match='no CPU path'):
        coalign(x[0], x[0], 3)
    for kw in (dict(measure='ncc'), dict(combine='mean')):
        with pytest.raises(ValueError):
            coalign(x, x, 2, **kw)
    sums = torch.zeros(2, 5, 7, 6, dtype=torch.float64)
    for bad in (dict(measure='ncc'), dict(min_overlap=1.5), dict(min_overlap=-0.1)):
        with pytest.raises(ValueError):
            scores_from_sums(sums, **bad)
    with pytest.raises(ValueError):
        scores_from_sums(sums[..., :5])
    with pytest.raises(ValueError):
        peak(torch.zeros(2, 4, 7))
    with pytest.raises(ValueError):
        peak(torch.zeros(2, 5, 7), combine='mean')


def test_the_observation_set_refuses_views_whose_pointing_it_cannot_move():
    """Per-pixel angles and non-uniform axes, the way ``patch_pool`` refuses them -- before anything is computed."""
    from sunerf_hip.observations import ObservationSet
    obs = ObservationSet(device='cpu')
    img = torch.zeros(6, 8)
    tx, ty = torch.linspace(-1, 1, 8, dtype=torch.float64), torch.linspace(-1, 1, 6, dtype=torch.float64)
    obs.add_view(img, 0.0, 0.0, tx=tx[None, :].expand(6, 8).contiguous(), ty=ty[:, None].expand(6, 8).contiguous())
    bent = tx.clone()
    bent[3] += 0.01
    obs.add_view(img, 0.0, 0.5, tx=bent, ty=ty)
    obs.add_view(img, 0.0, 1.0, tx=tx, ty=ty)
    with pytest.raises(ValueError, match='per-pixel angles are not supported'):
        obs.coalign_view(0, reference=img[None])
    with pytest.raises(ValueError, match='uniform pixel axis'):
        obs.coalign_view(1, reference=img[None])
    with pytest.raises(ValueError, match="combine='shared'"):
        obs.coalign_view(2, reference=img[None], combine='planes')
    with pytest.raises(ValueError, match='reference must be'):
        obs.coalign_view(2, reference=torch.zeros(1, 6, 7), apply=False)
    with pytest.raises(ValueError, match="'baseline'"):
        obs.coalign_view(2, reference='model', apply=False)
    with pytest.raises(IndexError):
        obs.coalign_view(3)
    with pytest.raises(ValueError):
        obs.coalign_views(apply=True)


# ---- the restatement ----------------------------------------------------------------------------------------------------------------
def test_the_restatements_cross_term_is_scipys_cross_correlation():
    """Without masks ``Sab[dy, dx] = sum_{r, c} image[r + dy, c + dx] templ[r, c]`` is the full cross-correlation
    ``correlate2d(image, templ)`` at lag (dy, dx), which scipy stores at index (dy + H - 1, dx + W - 1).  Small integers: every sum
    is exact, the comparison is by equality."""
    from scipy.signal import correlate2d
    rng = np.random.default_rng(1)
    for h, w, my, mx in ((9, 11, 3, 4), (5, 7, 8, 8), (1, 12, 0, 5)):
        image = rng.integers(-8, 9, (1, h, w)).astype(np.float32)
        templ = rng.integers(-8, 9, (1, h, w)).astype(np.float32)
        sums = cr.shift_sums(image, templ, my, mx)
        full = correlate2d(image[0].astype(np.float64), templ[0].astype(np.float64), mode='full')
        padded = np.zeros((2 * my + 1, 2 * mx + 1))
        for i, dy in enumerate(range(-my, my + 1)):
            for j, dx in enumerate(range(-mx, mx + 1)):
                if abs(dy) < h and abs(dx) < w:
                    padded[i, j] = full[dy + h - 1, dx + w - 1]
        assert np.array_equal(sums[0, ..., 5], padded), (h, w, my, mx)
        n = np.array([[max(0, h - abs(dy)) * max(0, w - abs(dx)) for dx in range(-mx, mx + 1)] for dy in range(-my, my + 1)])
        assert np.array_equal(sums[0, ..., 0], n)
        # the two exact modes of the restatement agree with the plain one on exact data
        assert np.array_equal(cr.shift_sums(image, templ, my, mx, exact='fsum'), sums)
        assert np.array_equal(cr.shift_sums(image, templ, my, mx, exact='longdouble'), sums)


def test_the_restatement_follows_the_pair_set_on_planes_small_enough_to_check_by_hand():
    image = np.array([[[1.0, 2.0, np.inf], [4.0, np.nan, 6.0]]], dtype=np.float32)
    templ = np.array([[[1.0, -np.inf, 3.0], [2.0, 5.0, 7.0]]], dtype=np.float32)
    bad_t = np.array([[[0, 0, 0], [9, 0, 0]]], dtype=np.uint8)
    sums = cr.shift_sums(image, templ, 1, 1, bad_template=bad_t)
    # shift (0, 0): pairs (1, 1), (6, 7); (2, -inf), (inf, 3), (4, bad), (nan, 5) drop out
    assert sums[0, 1, 1].tolist() == [2.0, 7.0, 8.0, 37.0, 50.0, 43.0]
    # shift (1, -1): a = image[r + 1, c - 1], r = 0, c = 1, 2: (4, -inf) drops, (nan, 3) drops
    assert sums[0, 2, 0].tolist() == [0.0] * 6
    # shift (0, 1): a = image[r, c + 1], c = 0, 1: (2, 1), (inf, -inf), (nan, bad), (6, 5)
    assert sums[0, 1, 2].tolist() == [2.0, 8.0, 6.0, 40.0, 26.0, 32.0]
    assert np.array_equal(cr.shift_sums(image, templ, 3, 0)[0, [0, 6]], np.zeros((2, 1, 6)))          # |dy| >= H: no overlap


def _random_sums(seed, c=3, h=24, w=30, my=4, mx=5):
    """Inputs whose standard deviation is at least a tenth of their mean: n Saa - Sa^2 cancels at most two digits."""
    rng = np.random.default_rng(seed)
    base = rng.uniform(0.5, 1.5, (h + 2 * my, w + 2 * mx)).astype(np.float32)
    image = np.stack([base[my + 1:my + 1 + h, mx - 2:mx - 2 + w] * (1 + 0.1 * p) + 0.05 * rng.standard_normal((h, w)) for p in range(c)])
    templ = np.stack([base[my:my + h, mx:mx + w] + 0.05 * rng.standard_normal((h, w)) for _ in range(c)])
    image, templ = image.astype(np.float32), templ.astype(np.float32)
    assert image.std() >= 0.1 * image.mean() and templ.std() >= 0.1 * templ.mean()
    templ[:, :3, :4] = np.nan
    return cr.shift_sums(image, templ, my, mx)


@pytest.mark.parametrize('measure', ['zncc', 'ssd'])
def test_scores_and_peak_on_cpu_torch_match_the_restatement(measure):
    """The same sums through ``scores_from_sums`` / ``peak`` (torch, fp64, CPU) and through the restatement: about ten fp64
    operations each, on scores in [-1, 1] (zncc) or of order 0.1 (ssd) -- gated at 1e-12."""
    from sunerf_hip.coalign import peak, scores_from_sums
    worst = 0.0
    for seed in range(4):
        sums = _random_sums(seed)
        if seed == 3:
            sums[1] = 0.0          # an absent channel
        for min_overlap in (0.0, 0.5, 0.9):
            want = cr.scores_from_sums(sums, measure, min_overlap)
            got = scores_from_sums(torch.from_numpy(sums), measure, min_overlap).numpy()
            assert np.array_equal(np.isnan(got), np.isnan(want)) and np.isfinite(want).any()
            worst = max(worst, float(np.nanmax(np.abs(got - want))))
            if measure == 'zncc':
                assert np.nanmax(np.abs(want)) <= 1.0 + 1e-12
            for combine in ('shared', 'planes'):
                a, b = peak(torch.from_numpy(got), combine), cr.peak(got, combine)
                assert np.array_equal(a['integer'].numpy(), b['integer']) and np.array_equal(a['status'].numpy(), b['status'])
                assert a['shift'].dtype == torch.float64 and a['integer'].dtype == torch.int64 and a['status'].dtype == torch.int64
                assert a['shift'].shape == ((2,) if combine == 'shared' else (3, 2))
                np.testing.assert_allclose(a['shift'].numpy(), b['shift'], rtol=0, atol=1e-9)
                np.testing.assert_allclose(a['score'].numpy(), b['score'], rtol=0, atol=1e-12, equal_nan=True)
        shared = cr.peak(cr.scores_from_sums(sums, measure, 0.5))
        assert shared['integer'].tolist() == [-1, 2] and shared['status'] == 0, (seed, shared)
    print(f'{measure}: largest |torch - restatement| over the scores: {worst:.3e} (gate 1e-12)')
    assert worst <= 1e-12


def test_overlap_rule_and_degenerate_variances():
    from sunerf_hip.coalign import scores_from_sums
    sums = np.zeros((1, 1, 3, 6))
    sums[0, 0, 0] = [10, 10, 20, 10, 40, 20]          # a constant: va = 0 -> NaN
    sums[0, 0, 1] = [10, 5, 7, 9, 11, 8]
    sums[0, 0, 2] = [4, 2, 3, 5, 6, 4]                # n below half of the largest
    for f in (lambda s, **k: scores_from_sums(torch.from_numpy(s), **k).numpy(), cr.scores_from_sums):
        z = f(sums, measure='zncc', min_overlap=0.5)
        assert np.isnan(z[0, 0, 0]) and np.isnan(z[0, 0, 2]) and z[0, 0, 1] == (80 - 35) / np.sqrt((90 - 25) * (110 - 49))
        s = f(sums, measure='ssd', min_overlap=0.5)
        assert s[0, 0, 0] == -1.0 and s[0, 0, 1] == -0.4 and np.isnan(s[0, 0, 2])
        assert f(sums, measure='ssd', min_overlap=0.4)[0, 0, 2] == -0.75


def test_every_status_bit_is_reached():
    from sunerf_hip.coalign import EDGE, FLAT, NO_PEAK, peak
    nan = float('nan')

    def both(scores, combine='shared'):
        a, b = peak(torch.tensor(scores, dtype=torch.float64), combine), cr.peak(np.array(scores), combine)
        assert np.array_equal(a['status'].numpy(), b['status']) and np.array_equal(a['integer'].numpy(), b['integer'])
        np.testing.assert_allclose(a['shift'].numpy(), b['shift'], rtol=0, atol=1e-15)
        np.testing.assert_array_equal(a['score'].numpy(), b['score'])
        return a
    bowl = [[0.1, 0.2, 0.1], [0.3, 0.9, 0.5], [0.1, 0.2, 0.1]]
    out = both([bowl])
    assert out['status'].item() == 0 and out['integer'].tolist() == [0, 0] and out['score'].item() == 0.9
    assert out['shift'].tolist() == [0.0, 0.5 * (0.3 - 0.5) / (0.3 - 1.8 + 0.5)]
    out = both([[[nan] * 3] * 3])
    assert out['status'].item() == NO_PEAK and out['shift'].tolist() == [0.0, 0.0] and np.isnan(out['score'].item())
    out = both([[[0.1, 0.2, 0.9], [0.3, 0.4, 0.5], [0.1, 0.2, 0.1]]])
    assert out['status'].item() == EDGE and out['integer'].tolist() == [-1, 1] and out['shift'].tolist() == [-1.0, 1.0]
    out = both([[[0.1, 0.2, 0.1], [0.3, 0.4, 0.9], [0.1, 0.2, 0.3]]])          # on the border in x only: y is refined
    assert out['status'].item() == EDGE and out['integer'].tolist() == [0, 1] and out['shift'][1].item() == 1.0
    assert out['shift'][0].item() == 0.5 * (0.1 - 0.3) / (0.1 - 1.8 + 0.3)
    out = both([[[0.1, nan, 0.1], [0.3, 0.9, 0.5], [0.1, 0.2, 0.1]]])          # a NaN neighbour in y
    assert out['status'].item() == FLAT and out['shift'][0].item() == 0.0 and out['shift'][1].item() != 0.0
    out = both([[[0.1, 0.9, nan], [0.9, 0.9, 0.9], [0.1, 0.9, 0.1]]])          # the first of equal maxima: on the border in y, NaN beside it in x
    assert out['status'].item() == EDGE | FLAT and out['integer'].tolist() == [-1, 0]
    out = both([[[0.2, 0.9, 0.4]]])                                              # max_dy = 0: that axis sets no bit
    assert out['status'].item() == 0 and out['shift'][0].item() == 0.0 and out['shift'][1].item() != 0.0
    out = both([[[0.9]]])
    assert out['status'].item() == 0 and out['shift'].tolist() == [0.0, 0.0]
    # two nearly equal neighbours: the offset never leaves half a pixel
    out = both([[[0.0, 0.0, 0.0], [0.0, 1.0, 0.999999], [0.0, 0.0, 0.0]]])
    assert out['status'].item() == 0 and abs(out['shift'][1].item()) <= 0.5
    # a score at the measure's bound is an exact copy: the whole-pixel shift, no refinement and no bit -- only with the bound given
    copy = [[[0.1, 0.2, 0.1], [0.3, 1.0, 0.5], [0.1, nan, 0.1]]]
    assert both(copy)['status'].item() == FLAT and both(copy)['shift'][1].item() != 0.0
    for f in (lambda s, **k: peak(torch.tensor(s, dtype=torch.float64), **k), lambda s, **k: cr.peak(np.array(s), **k)):
        out = f(copy, bound=1.0)
        assert int(out['status']) == 0 and np.asarray(out['shift']).tolist() == [0.0, 0.0] and float(out['score']) == 1.0
        assert int(f(copy, bound=0.0)['status']) == FLAT
        out = f([[[0.1, 0.2, 1.0], [0.3, 0.4, 0.5], [0.1, 0.2, 0.1]]], bound=1.0)          # on the border, but exact
        assert int(out['status']) == 0 and np.asarray(out['shift']).tolist() == [-1.0, 1.0]
    # shared: an absent plane is left out, a NaN of a present one refuses the shift; planes: one peak each
    planes = [bowl, [[nan] * 3] * 3, [[0.1, 0.2, 0.1], [0.3, 0.5, nan], [0.1, 0.2, 0.1]]]
    out = both(planes)
    assert out['status'].item() == FLAT and out['score'].item() == 0.5 * (0.9 + 0.5)
    out = both(planes, 'planes')
    assert out['status'].tolist() == [0, NO_PEAK, FLAT] and out['shift'].shape == (3, 2)


def test_shifted_grid_moves_crpix_so_that_the_shifted_pixel_keeps_its_angles():
    """``new_tx[c + dx] == old_tx[c]`` and ``new_ty[r + dy] == old_ty[r]`` to 1e-12 |cdelt|: by index for whole shifts, through
    the linear formula for fractional ones -- with the axes of ``linear_plate_scale_axes`` itself, so the sign is not a guess."""
    from sunerf.evaluation.loader import ARCSEC, linear_plate_scale_axes
    from sunerf_hip.coalign import shifted_grid
    grids = [{'shape': (37, 53), 'cdelt': (2.4, 2.4)}, {'shape': (20, 31), 'cdelt': (-0.6, 1.2), 'crpix': (14.25, 9.5), 'crval': (30., -12.)},
             {'shape': (16, 16), 'cdelt': (75., -75.), 'crval': (1., 2.), 'extra': 'kept'}]
    for grid in grids:
        old_tx, old_ty = (t.numpy() for t in linear_plate_scale_axes(grid, None, 'cpu'))
        cdx, cdy = (abs(c) * ARCSEC for c in grid['cdelt'])
        for dy, dx in ((3, -5), (0, 0), (-2, 7), (2.3, -1.6), (-4.5, 0.5), (0.25, 6.75)):
            new = shifted_grid(grid, dy, dx)
            want = cr.shifted_grid(grid, dy, dx)
            assert new == want and {k: v for k, v in new.items() if k != 'crpix'} == {k: v for k, v in grid.items() if k != 'crpix'}
            new_tx, new_ty = (t.numpy() for t in linear_plate_scale_axes(new, None, 'cpu'))
            if float(dy).is_integer() and float(dx).is_integer():
                dy, dx = int(dy), int(dx)
                c = np.arange(max(0, -dx), min(len(old_tx), len(old_tx) - dx))
                r = np.arange(max(0, -dy), min(len(old_ty), len(old_ty) - dy))
                assert np.abs(new_tx[c + dx] - old_tx[c]).max() <= 1e-12 * cdx and np.abs(new_ty[r + dy] - old_ty[r]).max() <= 1e-12 * cdy
            # the axis is linear in the pixel index: the new grid's formula at the (fractional) index c + dx, r + dy
            (cpx, cpy), (cvx, cvy) = new['crpix'], new.get('crval', (0., 0.))
            at_x = ((np.arange(1, len(old_tx) + 1) + dx - cpx) * new['cdelt'][0] + cvx) * ARCSEC
            at_y = ((np.arange(1, len(old_ty) + 1) + dy - cpy) * new['cdelt'][1] + cvy) * ARCSEC
            assert np.abs(at_x - old_tx).max() <= 1e-12 * cdx and np.abs(at_y - old_ty).max() <= 1e-12 * cdy


# ---- sub-pixel recovery ---------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def recovered():
    return [(t, cr.coalign(*cr.scene_pair(*t)[:2], 8, bad_template=cr.scene_pair(*t)[2])) for t in cr.SCENE_SHIFTS]


def test_sub_pixel_recovery_on_the_analytic_scene(recovered):
    """40 Gaussians (sigma 2 .. 6 px) on 96 x 80 evaluated at shifted coordinates, the template NaN outside radius 44 and with a
    lattice of bad pixels, ``max_shift`` 8: the integer peak of the whole-pixel case is exact, every estimate lies within 0.5 px
    of the truth, and for a fractional truth the estimate is nearer than the integer peak.  Errors of this scene (restatement):
    0, 0.0220, 0.0290 and 0.0105 px against 0, 0.50, 0.71 and 0.35 px for the integer peak.  The whole-pixel case is an exact
    copy and scores exactly 1, the measure's bound, so it is not refined; its parabola alone would give 0.0019 px."""
    for truth, out in recovered:
        err = float(np.hypot(*(out['shift'] - np.array(truth))))
        err_int = float(np.hypot(*(out['integer'] - np.array(truth))))
        print(f'true shift {truth}: estimate ({out["shift"][0]:+.4f}, {out["shift"][1]:+.4f}), error {err:.4f} px; integer peak '
              f'{out["integer"].tolist()}, error {err_int:.4f} px; score {out["score"]:.6f}, status {out["status"]}')
        assert out['status'] == 0 and err <= 0.5
        if all(float(t).is_integer() for t in truth):
            assert out['integer'].tolist() == [int(t) for t in truth]
        else:
            assert err < err_int


def test_scores_of_the_scene_through_torch_give_the_same_peak(recovered):
    from sunerf_hip.coalign import peak, scores_from_sums
    for truth, out in recovered:
        got = peak(scores_from_sums(torch.from_numpy(out['sums'])), bound=1.0)
        assert got['integer'].tolist() == out['integer'].tolist() and got['status'].item() == out['status']
        np.testing.assert_allclose(got['shift'].numpy(), out['shift'], rtol=0, atol=1e-9)
