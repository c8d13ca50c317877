"""CPU-only checks of the despiking step (no GPU): the eleventh entry-point table (declared, bound, versioned, its
workspace query and its argument checks in their documented order), the wrapper's refusals, the instrument's variance parameters
against ``Instrument.errors``, and the algorithm itself -- the NumPy restatement tests/despike_reference.py -- against
``scipy.ndimage.median_filter`` where the two medians coincide and on a fixed scene with known hits.  Every figure is printed."""
import ctypes
import os

import numpy as np
import pytest
import torch

import despike_reference as dr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N_COUNTERS = 64 + 2          # per plane, 4 bytes each: include/sunerf_hip_despike.h


@pytest.fixture(scope='session')
def lib():
    import sunerf_hip
    if not os.path.exists(sunerf_hip.LIB_PATH):
        import subprocess
        subprocess.check_call(['bash', os.path.join(ROOT, '2024-hl-spi3s-sunerf_amd', 'csrc', 'build.sh')])
    return sunerf_hip.load()


# ---- the eleventh table -----------------------------------------------------------------------------------------------------------
def test_entry_points_are_declared_and_bound(lib):
    """(The table itself -- declared, bound, frozen, versioned, built: tests/test_abi_tables_host.py.)"""
    header = open(os.path.join(ROOT, 'include', 'sunerf_hip_despike.h')).read()
    assert lib.sunerf_despike_abi_version() == 1
    for define in ('SUNERF_DESPIKE_MAX_RADIUS 3', 'SUNERF_DESPIKE_MAX_ITERATIONS 64', 'SUNERF_DESPIKE_MAX_MIN_VALID 48',
                   'SUNERF_DESPIKE_SPIKE 1', 'SUNERF_DESPIKE_INVALID 2', 'SUNERF_DESPIKE_UNFILLED 4'):
        assert f'#define {define}' in header, define
    from sunerf_hip import despike as wrapper
    assert (wrapper.SPIKE, wrapper.INVALID, wrapper.UNFILLED) == (dr.SPIKE, dr.INVALID, dr.UNFILLED) == (1, 2, 4)
    assert wrapper.MODES == {'model': dr.MODEL, 'mad': dr.MAD} and (wrapper.TWO_SIDED, wrapper.FILL_NAN) == (dr.TWO_SIDED, dr.FILL_NAN)


def test_workspace_query(lib):
    """The second mask buffer, one byte per pixel rounded up to 8, and 66 counters of 4 bytes per plane; the radius does not change
    the size but a radius outside 1 .. 3 has none."""
    q = lib.sunerf_despike_workspace_bytes
    valid = [((1, 5, 7, 3), 40 + 264), ((1, 1, 1, 1), 8 + 264), ((3, 33, 65, 2), 6440 + 3 * 264), ((1, 40, 1, 1), 40 + 264),
             ((7, 1024, 1024, 3), 7 * 1024 * 1024 + 7 * 264), ((2, 46341, 46341, 1), (2 * 46341 * 46341 + 7) // 8 * 8 + 2 * 264)]
    assert [q(*a) for a, _ in valid] == [b for _, b in valid]
    assert N_COUNTERS * 4 == 264
    invalid = [(0, 5, 7, 1), (-1, 5, 7, 1), (1, 0, 7, 1), (1, 5, 0, 1), (1, 5, 7, 0), (1, 5, 7, 4), (1, 5, 7, -1), (1, -5, 7, 2)]
    assert [q(*a) for a in invalid] == [0] * len(invalid)


def check_argument_order(lib):
    """Limits (-2) first, then the empty call (0), then counts, thresholds, null pointers, alignment and the overlap of clean with
    image (-1): all before anything touches a device, so this runs without one.  ``Q`` stands for any non-null aligned pointer: no
    call here reaches a launch."""
    fn = lib.sunerf_despike
    names = ('image', 'params', 'clean', 'mask', 'state', 'workspace')
    Q = {k: ctypes.c_void_p(4096 + 65536 * i) for i, k in enumerate(names)}

    def call(n_planes=2, h=9, w=11, radius=2, mode=0, flags=0, n_sigma=5.0, grow_sigma=3.0, min_valid=3, iterations=4, bad=None, **ptrs):
        p = dict(Q)
        p.update(ptrs)
        return fn(p['image'], bad, p['params'], n_planes, h, w, radius, mode, flags, n_sigma, grow_sigma, min_valid, iterations,
                  p['clean'], p['mask'], p['state'], p['workspace'], None)
    none = {k: None for k in names}
    assert call(radius=4, **none) == -2 and call(iterations=65, **none) == -2 and call(min_valid=49, **none) == -2
    assert call(mode=2, **none) == -2 and call(mode=-1, **none) == -2 and call(flags=4, **none) == -2 and call(flags=-1, **none) == -2
    assert call(radius=4, n_planes=0, **none) == -2 and call(iterations=65, n_planes=-1, **none) == -2          # the limits come first
    for empty in (dict(n_planes=0), dict(h=0), dict(w=0), dict(h=0, w=0)):
        assert call(min_valid=0, n_sigma=-1.0, **empty, **none) == 0, empty                                       # then the empty call
    assert call(n_planes=-1) == -1 and call(h=-1) == -1 and call(w=-1) == -1 and call(n_planes=-1, h=0) == -1
    assert call(radius=0) == -1 and call(radius=-1) == -1 and call(radius=0, n_planes=0) == -1
    assert call(min_valid=0) == -1 and call(iterations=-1) == -1
    for bad_sigma in (0.0, -1.0, float('nan'), float('inf')):
        assert call(n_sigma=bad_sigma) == -1 and call(grow_sigma=bad_sigma) == -1, bad_sigma
    for k in names:
        assert call(**{k: None}) == -1, k
    for k in ('params', 'state', 'workspace'):
        assert call(**{k: ctypes.c_void_p(Q[k].value + 4)}) == -1, k
    # clean may not overlap image: 2 x 9 x 11 floats are 792 bytes
    assert call(clean=Q['image']) == -1 and call(clean=ctypes.c_void_p(Q['image'].value + 788)) == -1
    assert call(clean=ctypes.c_void_p(Q['image'].value - 788)) == -1
    # with every pointer null the next refusal is the pointers': all the scalar checks before them pass at the limits
    assert all(call(radius=r, iterations=i, min_valid=m, mode=mode, flags=f, **none) == -1
               for r, i, m, mode, f in ((1, 0, 1, 0, 0), (3, 64, 48, 1, 3), (2, 4, 3, 0, 1)))


def test_argument_checks_come_in_the_documented_order(lib):
    check_argument_order(lib)


# ---- the wrapper ------------------------------------------------------------------------------------------------------------------
def test_the_wrapper_refuses_what_it_cannot_run():
    from sunerf_hip import SunerfHipError
    from sunerf_hip.despike import add_cosmic_rays, despike
    x = torch.zeros(2, 9, 11)
    ok = dict(a=0.01, b=0.02)
    with pytest.raises(ValueError, match="mode='mad' needs window 5 or 7"):
        despike(x, mode='mad', window=3)
    for kw in (dict(mode='median'), dict(window=4), dict(window=9), dict(window=1), dict(fill='mean'), dict(n_sigma=0.0),
               dict(n_sigma=float('nan')), dict(grow_sigma=-1.0), dict(min_valid=0), dict(min_valid=25), dict(min_valid=2.5),
               dict(iterations=-1), dict(iterations=65), dict(iterations=1.5), dict(a=-1.0), dict(b=float('inf')), dict(a=[1.0, 2.0, 3.0]),
               dict(floor=-1.0), dict(bad=torch.zeros(2, 9, 10)), dict(min_valid=9, window=3)):
        with pytest.raises(ValueError):
            despike(x, **{**ok, **kw})
        print('refused:', kw)
    with pytest.raises(ValueError, match='needs the variance parameters'):
        despike(x)
    with pytest.raises(ValueError, match='needs the variance parameters'):
        despike(x, a=1.0)
    with pytest.raises(ValueError, match='float32'):
        despike(x.double(), **ok)
    with pytest.raises(ValueError, match='float32'):
        despike(torch.zeros(2, 2, 9, 11), **ok)
    with pytest.raises(TypeError):
        despike(x.numpy(), **ok)
    with pytest.raises(SunerfHipError, match='no CPU path'):          # every argument is in order: only the device is missing
        despike(x, **ok)
    with pytest.raises(SunerfHipError, match='no CPU path'):
        despike(x[0], mode='mad', floor=[0.1], min_valid=24, window=5, bad=torch.zeros(9, 11, dtype=torch.bool))
    with pytest.raises(ValueError):
        add_cosmic_rays(x, 1.5, 10.0)
    with pytest.raises(ValueError):
        add_cosmic_rays(x, 0.01, 10.0, length=(0, 2))
    with pytest.raises(ValueError):
        add_cosmic_rays(x, 0.01, 10.0, sigma=torch.ones(9, 11))


def test_add_cosmic_rays_is_seeded_and_hits_the_asked_fraction():
    from sunerf_hip.despike import add_cosmic_rays
    x = torch.ones(3, 64, 80)
    sigma = torch.full_like(x, 0.5)
    out, truth = add_cosmic_rays(x, 0.01, (10.0, 50.0), sigma=sigma, seed=3)
    again, truth2 = add_cosmic_rays(x, 0.01, (10.0, 50.0), sigma=sigma, seed=3)
    other, _ = add_cosmic_rays(x, 0.01, (10.0, 50.0), sigma=sigma, seed=4)
    assert torch.equal(out, again) and torch.equal(truth, truth2) and not torch.equal(out, other)
    assert out.dtype == x.dtype and truth.dtype == torch.bool and out.shape == x.shape == truth.shape
    assert torch.equal(out[~truth], x[~truth])
    gain = (out - x)[truth]
    assert float(gain.min()) >= 10.0 * 0.5 - 1e-5          # overlapping tracks add up: no upper bound
    fraction = truth.float().mean(dim=(1, 2))
    print('fraction of pixels hit per plane:', fraction.tolist())
    # tracks are cut at the edge and may overlap: a little below the asked 1 %, never above
    assert bool((fraction <= 0.01 + 1e-9).all()) and bool((fraction >= 0.008).all())
    single, t1 = add_cosmic_rays(x[0], 0.02, 7.0, length=(1, 1), seed=1)
    assert single.shape == (64, 80) and set((single - x[0])[t1].tolist()) <= {7.0, 14.0, 21.0}
    same, none = add_cosmic_rays(x, 0.0, 7.0)
    assert torch.equal(same, x) and not bool(none.any())


def test_despike_params_are_the_squared_errors_of_the_instrument():
    """``Instrument.errors(x) ** 2 == a + b max(x, 0)``: errors is rounded to float32 once (2^-24 relative), squaring doubles
    that and the float64 operations of both sides add a few 2^-53 -- 2^-22 is the bound."""
    from sunerf_hip.despike import despike_params
    from sunerf_hip.instrument import Instrument
    rng = np.random.default_rng(5)
    worst = 0.0
    for quantise in (False, True):
        inst = Instrument(unit=[100.0, 40.0, 7.5], exposure=[2.9, 1.0, 12.0], dn_per_photon=[1.2, 0.8, 3.0], read_noise=[1.2, 0.0, 5.0],
                          quantise=quantise)
        p = despike_params(inst, 3)
        assert p.shape == (3, 4) and p.dtype == np.float64 and np.array_equal(p[:, 3], np.zeros(3))
        np.testing.assert_allclose(p[:, 2], np.sqrt(p[:, 0]), rtol=1e-15)
        x = np.concatenate([rng.uniform(-0.5, 20.0, (3, 40)), np.zeros((3, 1))], axis=1)
        got = inst.errors(torch.from_numpy(x)[..., None], channel_axis=0).double().numpy()[..., 0] ** 2
        want = p[:, :1] + p[:, 1:2] * np.maximum(x, 0.0)
        if not quantise:                          # a channel without read noise has no variance at zero signal
            assert want[1, -1] == 0.0 and got[1, -1] == 0.0
        rel = np.abs(got - want) / np.where(want > 0, want, 1.0)
        worst = max(worst, float(rel.max()))
    print(f'largest relative difference between errors^2 and a + b max(x, 0): {worst:.3e} (bound {2.0 ** -22:.3e})')
    assert worst <= 2.0 ** -22
    scalar = despike_params(Instrument(unit=100.0, exposure=2.9, dn_per_photon=1.2, read_noise=1.2), 4)
    assert scalar.shape == (4, 4) and np.ptp(scalar, axis=0).max() == 0.0
    _, a, b = dr.scene()
    np.testing.assert_allclose(scalar[0, :2], [a, b], rtol=1e-15)


# ---- the restatement ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('r', [1, 2, 3])
def test_the_unmasked_median_is_scipys_where_the_definitions_coincide(r):
    """The restatement's median leaves the centre out: n = (2r+1)^2 - 1 is even and the result the mean of two middle values.
    With the centre put back n is odd, the ranks (n - 1) // 2 and n // 2 are the same one, and the rule is
    ``scipy.ndimage.median_filter(size=2r+1)`` -- at the interior pixels, where scipy pads nothing."""
    from scipy.ndimage import median_filter
    rng = np.random.default_rng(r)
    x = rng.integers(0, 12, (23, 31)).astype(np.float32) + rng.integers(0, 2, (23, 31)).astype(np.float32) * 0.5          # many ties
    v = np.concatenate([dr.neighbours(x, np.zeros(x.shape, dtype=np.uint8), r), x.astype(np.float64)[..., None]], axis=-1)
    med, n = dr.masked_median(v)
    want = median_filter(x.astype(np.float64), size=2 * r + 1, mode='constant')
    inner = (slice(r, -r), slice(r, -r))
    assert np.array_equal(n[inner], np.full_like(n[inner], (2 * r + 1) ** 2)) and np.array_equal(med[inner], want[inner])
    # the frame's corner has (r + 1)^2 - 1 neighbours without the centre
    _, n_out = dr.masked_median(dr.neighbours(x, np.zeros(x.shape, dtype=np.uint8), r))
    assert n_out[0, 0] == (r + 1) ** 2 - 1 and n_out[r, r] == (2 * r + 1) ** 2 - 1 and n_out[0, r] == (r + 1) * (2 * r + 1) - 1


def test_the_restatement_follows_the_rules_on_a_plane_small_enough_to_check_by_hand():
    x = np.full((5, 5), 2.0, dtype=np.float32)
    x[2, 2] = 9.0                                 # a hit
    x[0, 0] = np.nan                              # invalid, filled from its 3 neighbours
    x[4, 4] = 1.0                                 # a negative outlier
    out, mask, state = dr.despike(x, params=[[0.0, 0.5, 0.0, 0.0]], radius=1, n_sigma=3.0, grow_sigma=3.0, min_valid=3, max_iterations=4)
    want_mask = np.zeros((5, 5), dtype=np.uint8)
    want_mask[2, 2], want_mask[0, 0] = dr.SPIKE, dr.INVALID
    assert np.array_equal(mask, want_mask) and out[2, 2] == 2.0 and out[0, 0] == 2.0 and out[4, 4] == 1.0
    assert state.tolist() == [[1.0, 1.0, 0.0, 1.0, 1.0, 0.0]]
    _, mask2, state2 = dr.despike(x, params=[[0.0, 0.5, 0.0, 0.0]], radius=1, n_sigma=0.5, grow_sigma=0.5, min_valid=3, max_iterations=4,
                                  flags=dr.TWO_SIDED)
    assert mask2[4, 4] == dr.SPIKE and state2[0, 0] == 2.0          # (1 - 2)^2 = 1 > 0.25 * (0.5 * 2)
    out3, mask3, state3 = dr.despike(x, params=[[0.0, 0.5, 0.0, 0.0]], radius=1, min_valid=4, max_iterations=0)
    assert mask3[0, 0] == dr.INVALID | dr.UNFILLED and np.isnan(out3[0, 0]) and out3[2, 2] == 9.0
    assert state3.tolist() == [[0.0, 1.0, 1.0, 0.0, 0.0, 0.0]]
    out4, mask4, _ = dr.despike(x, params=[[0.0, 0.5, 0.0, 0.0]], radius=1, n_sigma=3.0, min_valid=4, flags=dr.FILL_NAN)
    assert np.isnan(out4[0, 0]) and np.isnan(out4[2, 2]) and mask4[0, 0] == dr.INVALID and mask4[2, 2] == dr.SPIKE


@pytest.fixture(scope='module')
def fixed_scene():
    rng = np.random.default_rng(0)
    truth, a, b = dr.scene()
    obs = dr.observed_scene(rng, truth)
    hit, where = dr.add_hits(rng, obs, np.sqrt(a + b * truth))
    return obs.astype(np.float32), hit.astype(np.float32), where, a, b


CONDITIONS = {dr.MODEL: (0.97, 2e-3), dr.MAD: (0.95, 2e-3)}


@pytest.mark.parametrize('mode,window', [(dr.MODEL, 3), (dr.MODEL, 5), (dr.MODEL, 7), (dr.MAD, 5), (dr.MAD, 7)],
                         ids=['model-3', 'model-5', 'model-7', 'mad-5', 'mad-7'])
def test_hits_are_found_and_clean_pixels_left_alone_on_the_fixed_scene(fixed_scene, mode, window):
    """96 x 96, a structured disc inside a falling corona seen through unit=100, exposure=2.9, dn_per_photon=1.2,
    read_noise=1.2 (``default_rng(0)``); 1 % of the pixels hit, every fourth hit a 3-pixel track, 10 .. 50 sigma.  With the
    defaults (n_sigma 5, grow_sigma 3, 4 passes, min_valid 3, floor sqrt(a)): at least 97 % ('model') / 95 % ('mad') of the hit
    pixels flagged, at most 2e-3 of the clean pixels flagged on the frame with hits and on the frame without."""
    obs, hit, where, a, b = fixed_scene
    kw = dict(params=[[a, b, np.sqrt(a), 0.0]], radius=window // 2, mode=mode)
    _, mask_clean, state_clean = dr.despike(obs, **kw)
    out, mask, state = dr.despike(hit, **kw)
    found = float((mask[where] != 0).mean())
    false_hit = float((mask[~where] != 0).mean())
    false_clean = float((mask_clean != 0).mean())
    residual = np.abs(out - obs)[where & (mask != 0)] / np.sqrt(a + b * np.maximum(obs[where & (mask != 0)], 0))
    print(f"{('model', 'mad')[mode]} window {window}: {where.sum()} hit pixels, {100 * found:.2f} % flagged; clean pixels flagged "
          f'{false_hit:.2e} (frame with hits), {false_clean:.2e} (frame without); passes {int(state[0, 3])} / {int(state_clean[0, 3])}, '
          f'converged {int(state[0, 4])}; filled pixels lie {np.median(residual):.2f} sigma (median) from the frame without hits')
    least, most = CONDITIONS[mode]
    assert found >= least and false_hit <= most and false_clean <= most
    assert state[0, 0] == (mask & dr.SPIKE != 0).sum() and state[0, 1] == 0 and not np.isnan(out).any()
