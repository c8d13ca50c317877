"""Richardson-Lucy deconvolution on the device (include/sunerf_hip_deconvolve.h) against the fp64 restatement
tests/deconvolve_reference.py: the iterates by bits, the deviance to 1e-12 of the size of its terms, masking, determinism,
independence of the planes of a batch (their stops included), the call without an update, one update against the adjoint entry
by bits, and ``Instrument.deconvolve``.

One reference run of five updates per (case, boundary) serves every test: pass k of it describes the iterate after k updates, so it
holds the iterate and the state of every shorter call.  Gates: ``u`` is made of +, * and / in a pinned order -- bits.  The deviance
is a sum in another order than the restatement's and over the device's ``log``: |D_gpu - D_ref| <= 1e-12 * sum(|L| + |N| +
|N log(N / L)|), a thousand-fold margin over a few fp64 ulps per term, absolute on that scale because L - N cancels near the fit."""
import functools

import numpy as np
import pytest
import torch

import deconvolve_reference as dr

pytestmark = pytest.mark.gpu

DEV = 'cuda'
N_MAX = 5
_IDS = lambda c: '-'.join(str(v) for v in c[:6])          # noqa: E731


def _scale(case):
    return 1.0 / (case[5] * case[5])


def _device_norm(d, bad, K, case, boundary):
    from sunerf_hip.instrument import BOUNDARY, correlate_bin_adjoint
    taps = torch.tensor(K, dtype=torch.float64).to(DEV)
    valid = torch.tensor(dr.valid_mask(d, bad).astype(np.float32)).to(DEV)
    return correlate_bin_adjoint(valid, case[1], case[2], taps, K.shape[0], K.shape[1], K.shape[2], case[5], case[6][0], case[6][1],
                                 _scale(case), BOUNDARY[boundary])


def _rl(u0, d, bad, norm, K, c, v, case, boundary, n, stop=0.0):
    """The ABI call through ``sunerf_hip.deconvolve.launch``: (u, state, ratio) as NumPy arrays."""
    from sunerf_hip.deconvolve import launch
    from sunerf_hip.instrument import BOUNDARY
    u = torch.tensor(u0).to(DEV)          # (torch.tensor copies: the shared reference arrays are read-only)
    taps = torch.tensor(K, dtype=torch.float64).to(DEV)
    params = torch.from_numpy(np.stack([np.asarray(c, dtype=np.float64), np.asarray(v, dtype=np.float64)], axis=1)).to(DEV)
    mask = None if bad is None else torch.tensor(bad).to(DEV)
    norm = norm if isinstance(norm, torch.Tensor) else torch.tensor(norm).to(DEV)
    state, ratio = launch(u, torch.tensor(d).to(DEV), mask, norm, params, taps, K.shape[0], K.shape[1], K.shape[2],
                          case[5], case[6][0], case[6][1], _scale(case), BOUNDARY[boundary], n, stop)
    torch.cuda.synchronize()
    return u.cpu().numpy(), state.cpu().numpy(), ratio.cpu().numpy()


@functools.lru_cache(maxsize=None)
def _reference(case, boundary):
    """Inputs, the restatement's norm, and per plane the (deviance, n_valid, scale) and the iterate of passes 0 .. N_MAX."""
    K, u0, d, bad, c, v = dr.case_data(case)
    norm = dr.norm_of(d, bad, K, case[1], case[2], case[5], case[6], _scale(case), boundary)
    history, iterates = [], []
    dr.richardson_lucy(u0, d, bad, norm, K, case[5], case[6], _scale(case), boundary, c, v, N_MAX, 0.0, history, iterates)
    for a in (K, u0, d, bad, c, v, norm):
        a.setflags(write=False)
    return (K, u0, d, bad, c, v), norm, history, iterates


@functools.lru_cache(maxsize=None)
def _device(case, boundary, n):
    (K, u0, d, bad, c, v), norm, _, _ = _reference(case, boundary)
    got_norm = _device_norm(d, bad, K, case, boundary)
    assert np.array_equal(got_norm.cpu().numpy().view(np.uint32), norm.view(np.uint32)), 'norm differs from the restatement by bits'
    return _rl(u0, d, bad, got_norm, K, c, v, case, boundary, n)


def _same_bits(got, want, what):
    assert got.shape == want.shape and got.dtype == want.dtype == np.float32
    assert not np.isnan(want).any(), f'{what}: the restatement holds NaN'
    differ = got.view(np.uint32) != want.view(np.uint32)
    assert not differ.any(), f'{what}: {int(differ.sum())} of {got.size} elements differ by bits, first at {tuple(np.argwhere(differ)[0])}: ' \
                             f'{got[differ][0]!r} != {want[differ][0]!r}'


# ---- 1. against the restatement ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('n', (1, 2, 5))
@pytest.mark.parametrize('boundary', dr.BOUNDARIES)
@pytest.mark.parametrize('case', dr.CASES, ids=_IDS)
def test_iterates_equal_the_restatement_by_bits(case, boundary, n):
    _, _, _, iterates = _reference(case, boundary)
    u, _, _ = _device(case, boundary, n)
    for p in range(case[0]):
        _same_bits(u[p], iterates[p][n], f'{case} {boundary} plane {p} after {n} updates')


@pytest.mark.parametrize('n', (0, 1, 2, 5))
@pytest.mark.parametrize('boundary', dr.BOUNDARIES)
@pytest.mark.parametrize('case', dr.CASES, ids=_IDS)
def test_state_describes_the_last_iterate(case, boundary, n):
    """deviance to 1e-12 of the size of its terms; n_valid, iterations_applied and stopped exactly."""
    (_, _, d, bad, _, _), _, history, _ = _reference(case, boundary)
    _, state, _ = _device(case, boundary, n)
    assert state.shape == (case[0], 4)
    for p in range(case[0]):
        dev, n_valid, size = history[p][n]
        assert n_valid == dr.valid_mask(d, bad)[p].sum() and n_valid < d[p].size
        print(f'{case} {boundary} plane {p} after {n}: deviance {state[p, 0]!r}, restatement {dev!r}, |difference| {abs(state[p, 0] - dev):.3e}, '
              f'bound {1e-12 * size:.3e}')
        assert abs(state[p, 0] - dev) <= 1e-12 * size
        assert state[p, 1] == n_valid and state[p, 2] == n and state[p, 3] == 0.0


# ---- 2. masking -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('boundary', dr.BOUNDARIES)
@pytest.mark.parametrize('case', [dr.CASES[2], dr.CASES[3], dr.CASES[7]], ids=_IDS)
def test_masked_pixels_take_no_part(case, boundary):
    """The value under a ``bad`` pixel, and whether an invalid pixel is a NaN or a flagged number, change no bit of u, ratio or
    state.  Where norm is 0 -- trailing rows and columns that fill no detector pixel and that no tap of a valid pixel reads -- u keeps
    its initial bits."""
    (K, u0, d, bad, c, v), norm, _, _ = _reference(case, boundary)
    u, state, ratio = _device(case, boundary, 2)
    other = d.copy()
    other[bad != 0] = 1234.5                                  # another value under the flag
    flagged = bad.copy()
    flagged[np.isnan(d)] = 1                                  # the NaN becomes a flagged number
    other[np.isnan(d)] = -7.0
    u2, state2, ratio2 = _rl(u0, other, flagged, norm, K, c, v, case, boundary, 2)
    assert np.array_equal(u.view(np.uint32), u2.view(np.uint32)) and np.array_equal(ratio.view(np.uint32), ratio2.view(np.uint32))
    assert np.array_equal(state.view(np.uint64), state2.view(np.uint64))
    assert (ratio[(bad != 0) | np.isnan(d)] == 0).all()
    dead = norm == 0
    assert dead.any() and not dead.all(), 'the case must have pixels that no valid detector pixel reads'
    assert np.array_equal(u[dead].view(np.uint32), u0[dead].view(np.uint32))
    assert (u[~dead] != u0[~dead]).mean() > 0.5


# ---- 3. determinism, independence, the stop -----------------------------------------------------------------------------------------
@pytest.mark.parametrize('boundary', dr.BOUNDARIES)
@pytest.mark.parametrize('case', [dr.CASES[1], dr.CASES[3], dr.CASES[7]], ids=_IDS)
def test_reruns_agree_and_a_plane_alone_gives_its_bits_of_the_batch(case, boundary):
    (K, u0, d, bad, c, v), norm, _, _ = _reference(case, boundary)
    u, state, ratio = _device(case, boundary, 2)
    again = _rl(u0, d, bad, norm, K, c, v, case, boundary, 2)
    for a, b in zip((u, state, ratio), again):
        assert np.array_equal(a.view(np.uint8), b.view(np.uint8))
    for p in range(case[0]):
        sl = slice(p, p + 1)
        alone = _rl(u0[sl], d[sl], bad[sl], norm[sl], K[sl] if case[7] else K, c[sl], v[sl], (1,) + case[1:], boundary, 2)
        for a, b in zip((u, state, ratio), alone):
            assert np.array_equal(a[sl].view(np.uint8), b.view(np.uint8)), f'plane {p}'


STOP_UNITS = (3000.0, 1000.0, 300.0)          # photons per second and image unit of the three planes: the stop falls later for more signal
STOP_CASE = (3, 48, 48, 17, 17, 1, (8, 8), False)


@functools.lru_cache(maxsize=None)
def _stop_reference():
    """Three planes of the host tests' 48 x 48 case at three exposure levels, chosen on the restatement: their discrepancy stops
    fall at least two updates apart and no iterate lies within 1e-6 relative of the threshold."""
    cases = [dr.host_case(1, 'nearest', unit=unit) for unit in STOP_UNITS]
    d = np.concatenate([hc['d'] for hc in cases])
    c = np.array([hc['c'] for hc in cases])
    v = np.array([hc['v'] for hc in cases])
    K, anchor = cases[0]['K'], cases[0]['anchor']
    assert K.shape[1:] == STOP_CASE[3:5] and anchor == STOP_CASE[6]
    u0 = dr.initial_image(d, None, 1)
    norm = dr.norm_of(d, None, K, 48, 48, 1, anchor, 1.0, 'nearest')
    history, iterates = [], []
    u, state, _ = dr.richardson_lucy(u0, d, None, norm, K, 1, anchor, 1.0, 'nearest', c, v, 12, 1.0, history, iterates)
    free = []
    dr.richardson_lucy(u0, d, None, norm, K, 1, anchor, 1.0, 'nearest', c, v, 12, 0.0, free)
    return (K, u0, d, c, v, norm), u, state, history, free


def test_planes_of_a_batch_stop_on_their_own():
    (K, u0, d, c, v, norm), want_u, want_state, history, free = _stop_reference()
    counts = [int(s[2]) for s in want_state]
    print('the restatement stops after', counts, 'updates; deviance per valid pixel', [round(s[0] / s[1], 4) for s in want_state])
    assert all(s[3] == 1 for s in want_state) and all(a - b >= 2 for a, b in zip(counts, counts[1:])) and counts[-1] >= 1
    for trace in free:
        assert all(abs(dev / n - 1.0) > 1e-6 for dev, n, _ in trace)          # no decision hangs on the last bits of a log
    u, state, _ = _rl(u0, d, None, norm, K, c, v, STOP_CASE, 'nearest', 12, stop=1.0)
    for p in range(3):
        _same_bits(u[p], want_u[p], f'plane {p}, stopped after {counts[p]} updates')
        assert state[p, 1] == 48 * 48 and state[p, 2] == counts[p] and state[p, 3] == 1.0
        assert abs(state[p, 0] - want_state[p, 0]) <= 1e-12 * history[p][-1][2]
        assert state[p, 0] <= state[p, 1]
        alone = _rl(u0[p:p + 1], d[p:p + 1], None, norm[p:p + 1], K, c[p:p + 1], v[p:p + 1], (1,) + STOP_CASE[1:], 'nearest', 12, stop=1.0)
        assert np.array_equal(alone[0].view(np.uint32), u[p:p + 1].view(np.uint32))
        assert np.array_equal(alone[1].view(np.uint64), state[p:p + 1].view(np.uint64))
    # a count that runs out first: the middle plane has stopped, the first has not
    u, state, _ = _rl(u0, d, None, norm, K, c, v, STOP_CASE, 'nearest', counts[1] + 1, stop=1.0)
    assert state[:, 2].tolist() == [counts[1] + 1, counts[1], counts[2]] and state[:, 3].tolist() == [0.0, 1.0, 1.0]
    _same_bits(u[1], want_u[1], 'the stopped plane of a shorter call')


@pytest.mark.parametrize('boundary', dr.BOUNDARIES)
@pytest.mark.parametrize('case', [dr.CASES[3], dr.CASES[5]], ids=_IDS)
def test_no_iterations_leaves_u_untouched_and_fills_the_state(case, boundary):
    (_, u0, _, _, _, _), _, history, _ = _reference(case, boundary)
    u, state, ratio = _device(case, boundary, 0)
    assert np.array_equal(u.view(np.uint32), u0.view(np.uint32))
    assert np.isfinite(state).all() and np.isfinite(ratio).all() and (ratio >= 0).all() and ratio.any()
    assert state[:, 2].tolist() == [0.0] * case[0] and state[:, 1].tolist() == [h[0][1] for h in history]


@pytest.mark.parametrize('boundary', dr.BOUNDARIES)
@pytest.mark.parametrize('case', [dr.CASES[1], dr.CASES[3], dr.CASES[4], dr.CASES[7]], ids=_IDS)
def test_one_update_from_ones_is_the_adjoint_entry_on_the_ratio_by_bits(case, boundary):
    """The update kernel and ``sunerf_patch_correlate_bin_adjoint`` share their sums (csrc/corr_bin.h): tied together directly, not
    through the restatement.  With u0 = 1, a caller's norm = 1 and no stop, the call without an update returns the ratio of the
    start, and one update from the same start is u = (float)((1.0 * (scale acc)) / 1.0) = (float)(scale acc) -- products and
    quotients by 1.0 are exact in fp64 -- which is what the adjoint entry stores for the same ratio.  Per-plane kernels, bin 3, a
    plane in which every tap clamps, partial last tiles of both tilings; the data's NaN and ``bad`` pixel put zeros into the ratio."""
    from sunerf_hip.instrument import BOUNDARY, correlate_bin_adjoint
    (K, _, d, bad, c, v), _, _, _ = _reference(case, boundary)
    ones = np.ones((case[0], case[1], case[2]), dtype=np.float32)
    u, state, ratio = _rl(ones, d, bad, ones, K, c, v, case, boundary, 0)
    assert np.array_equal(u.view(np.uint32), ones.view(np.uint32)) and state[:, 2].tolist() == [0.0] * case[0]
    assert (ratio == 0).any() and (ratio > 0).any() and np.isfinite(ratio).all()
    u, state, _ = _rl(ones, d, bad, ones, K, c, v, case, boundary, 1)
    assert state[:, 2].tolist() == [1.0] * case[0] and state[:, 3].tolist() == [0.0] * case[0]
    taps = torch.tensor(K, dtype=torch.float64).to(DEV)
    want = correlate_bin_adjoint(torch.tensor(ratio).to(DEV), case[1], case[2], taps, K.shape[0], K.shape[1], K.shape[2], case[5],
                                 case[6][0], case[6][1], _scale(case), BOUNDARY[boundary])
    _same_bits(u, want.cpu().numpy(), f'{case} {boundary}: one update from ones against the adjoint of the ratio')
    assert (u != ones).any()


# ---- 4. the Python level ----------------------------------------------------------------------------------------------------------
def _observed(inst, channels, h, w, seed):
    rng = np.random.default_rng(seed)
    truth = torch.from_numpy(rng.uniform(0.2, 2.0, size=(channels, h * inst.bin, w * inst.bin)).astype(np.float32)).to(DEV)
    return truth, inst.observe(truth, seed=seed)['image']


@pytest.mark.parametrize('bin_mode', ('mean', 'sum'))
@pytest.mark.parametrize('per_channel', (False, True))
def test_instrument_deconvolve_is_the_abi_call(bin_mode, per_channel):
    from sunerf_hip.deconvolve import initial_image, launch, photon_params
    from sunerf_hip.instrument import BOUNDARY, Instrument, correlate_bin_adjoint, gaussian_psf
    psf = np.stack([gaussian_psf(2.0, 3), gaussian_psf(3.0, 3)]) if per_channel else gaussian_psf(2.5, 3)
    inst = Instrument(psf=psf, bin=2, bin_mode=bin_mode, boundary='zero', unit=[400.0, 900.0], exposure=2.9, dn_per_photon=1.2, read_noise=1.2)
    _, image = _observed(inst, 2, 19, 23, seed=4)
    image[0, 3, 4] = float('nan')
    bad = torch.zeros(image.shape, dtype=torch.bool, device=DEV)
    bad[1, 7, 7] = True
    K, (ay, ax) = inst.effective_kernel()
    call = (inst._taps(K, image.device), K.shape[0], K.shape[1], K.shape[2], 2, ay, ax, inst.scale, BOUNDARY['zero'])
    valid = torch.isfinite(image) & ~bad
    norm = correlate_bin_adjoint(valid.to(torch.float32), 38, 46, *call)
    params = torch.from_numpy(photon_params(inst, 2)).to(DEV)
    starts = {'image': initial_image(image, valid, inst, 'image'), 'flat': initial_image(image, valid, inst, 'flat')}
    starts['tensor'] = (starts['image'] * 0.5 + 0.1).contiguous()
    assert (starts['flat'][0] == starts['flat'][0, 0, 0]).all() and not torch.equal(starts['image'], starts['flat'])
    for name, start in starts.items():
        for iterations, stop, threshold in ((4, None, 0.0), (25, 'discrepancy', 1.0), (25, 1.5, 1.5)):
            u = start.clone()
            state, _ = launch(u, image, bad.to(torch.uint8), norm, params, *call, iterations, threshold)
            out = inst.deconvolve(image, iterations=iterations, stop=stop, bad=bad, init=start if name == 'tensor' else name)
            assert out['image'].shape == (2, 38, 46) and out['image'].dtype == torch.float32
            assert torch.equal(out['image'].view(torch.int32), u.view(torch.int32)), (name, iterations, stop)
            assert torch.equal(out['norm'].view(torch.int32), norm.view(torch.int32))
            assert torch.equal(out['deviance'], state[:, 0] / state[:, 1]) and out['deviance'].dtype == torch.float64
            assert torch.equal(out['iterations'], state[:, 2].long()) and torch.equal(out['stopped'], state[:, 3] != 0)
            if stop is None:
                assert out['iterations'].tolist() == [4, 4] and not out['stopped'].any()
            else:
                assert bool((out['deviance'][out['stopped']] <= threshold).all())
    assert not torch.equal(starts['tensor'], inst.deconvolve(image, iterations=1, init=starts['tensor'])['image'])          # copied, not updated in place


@pytest.mark.parametrize('b,boundary', [(1, 'nearest'), (2, 'nearest'), (2, 'zero')])
def test_truth_is_a_fixed_point_of_a_noise_free_frame_on_the_device(b, boundary):
    """The host bound on the device: d = expected(truth), read noise 0, init = truth; after n = 5 updates |u - truth| <= 4 n 2^-24
    truth (tests/test_deconvolve_host.py)."""
    from sunerf_hip.instrument import Instrument
    inst = Instrument(psf=dr.gaussian_psf(dr.HOST_FWHM, dr.HOST_RADIUS), bin=b, boundary=boundary, read_noise=0.0,
                      **{k: v for k, v in dr.HOST_DETECTOR.items() if k != 'read_noise'})
    truth = torch.from_numpy(dr.host_truth(48)).to(DEV)
    n = 5
    out = inst.deconvolve(inst.expected(truth)[0], iterations=n, init=truth)          # a frame [h, w] is one plane
    assert out['image'].shape == (1, 48, 48)
    err = ((out['image'].double() - truth.double()).abs() / truth.double()).max().item()
    print(f'bin {b} {boundary}: largest |u - truth| / truth after {n} updates {err * 2 ** 24:.2f} x 2^-24; deviance per pixel '
          f'{out["deviance"].item():.3e}')
    assert err <= 4 * n * 2.0 ** -24 and out['iterations'].tolist() == [n]


def test_rejections():
    from sunerf_hip.instrument import Instrument
    from sunerf_hip.lib import SunerfHipError
    image = torch.rand(2, 8, 8, device=DEV)
    psf = np.full((3, 3), 0.125)
    psf[1, 1] = -0.0001
    with pytest.raises(ValueError, match='negative'):
        Instrument(psf=psf).deconvolve(image)
    with pytest.raises(ValueError, match='channels'):
        Instrument(psf=np.full((3, 3, 3), 1.0 / 9.0)).deconvolve(image)
    with pytest.raises(ValueError, match='values'):
        Instrument(unit=[1.0, 2.0, 3.0]).deconvolve(image)
    with pytest.raises(SunerfHipError):
        Instrument().deconvolve(image.cpu())
    for kw in (dict(stop='chi2'), dict(stop=-1.0), dict(iterations=-1), dict(iterations=10001), dict(init='zeros'),
               dict(init=torch.rand(2, 8, 9, device=DEV)), dict(bad=torch.zeros(2, 8, 9, device=DEV))):
        with pytest.raises(ValueError):
            Instrument().deconvolve(image, **kw)
