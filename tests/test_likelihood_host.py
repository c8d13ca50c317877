"""CPU-only checks of the noise-weighted likelihood (no GPU): the restatement tests/likelihood_reference.py against
central finite differences, against ``Instrument.errors`` and against two closed forms; the seventh entry-point table (declared,
bound, kept out of the other six, its argument checks in their documented order); ``NoiseLikelihood``'s validation.

Gate of the finite differences: 1e-7 of the magnitude of the derivative's own terms (for a derivative without cancellation, of
the derivative).  With a step of 1e-6 the central difference carries a truncation error of h^2 f''' / 6 -- at most
(slope / s2)^2 h^2 = 4e-10 of the derivative, as every prediction and target stays 1e-3 or more from the clamp -- and a rounding
error of 2^-53 / h = 1e-10 of the slot's own share of the loss, which is |m - t| / 2 <= 2 times its derivative (the shares are
differenced slot by slot: differenced as one sum of 1e4, their rounding alone would be 1e-6), and where m and t nearly cancel
a further 2^-53 m / (2 h |m - t|), 5e-8 at the closest pair of the case (|m - t| = m / 1000): all inside the gate, while a
wrong sign, a missing factor or a missing d s2 / d m term is an error of order one."""
import ctypes
import os

import numpy as np
import pytest

import likelihood_reference as lr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FD_GATE, FD_STEP = 1e-7, 1e-6


@pytest.fixture(scope='session')
def lib():
    import sunerf_hip
    if not os.path.exists(sunerf_hip.LIB_PATH):
        import subprocess
        subprocess.check_call(['bash', os.path.join(ROOT, '2024-hl-spi3s-sunerf_amd', 'csrc', 'build.sh')])
    return sunerf_hip.load()


# ---- 1. the restatement -----------------------------------------------------------------------------------------------------------
def _fd_case():
    """16 rays x 3 columns, 3 rows: predictions and targets of both signs, each 0.05 or more (far more than 1e-3) from 0; a few
    masked slots of every kind."""
    rng = np.random.default_rng(8)
    n, w, m = 16, 3, 3
    row_codes = np.array([94, 171, 10171], dtype=np.float32)
    noise = np.array([[40.0, 2.9, 1.2, 1.5, 1.0 / 12.0, 0.0, 0, 0], [12.0, 1.0, 0.8, 2.0, 0.0, 0.01, 0, 0],
                      [5.0, 0.7, 1.0, 0.0, 0.0, 0.05, 0, 0]])
    sign = lambda: np.where(rng.random((n, w)) < 0.25, -1.0, 1.0)          # noqa: E731
    truth = rng.uniform(0.05, 2.0, (n, w))
    coarse = (truth * rng.uniform(0.6, 1.5, (n, w)) * sign()).astype(np.float32)
    fine = (truth * rng.uniform(0.8, 1.25, (n, w)) * sign()).astype(np.float32)
    target = (truth * rng.uniform(0.7, 1.3, (n, w)) * sign()).astype(np.float32)
    codes = row_codes[rng.integers(0, m, (n, w))]
    codes[0, 0], codes[3, 1], target[5, 2] = 0.0, 777.0, np.nan
    log_gain = np.array([0.2, -0.3, 0.1], dtype=np.float32)
    reg = rng.uniform(0.0, 1.0, 20).astype(np.float32)
    assert min(np.abs(coarse).min(), np.abs(fine).min(), np.nanmin(np.abs(target))) >= 1e-3
    return dict(coarse=coarse, fine=fine, target=target, codes=codes, row_codes=row_codes, noise=noise, log_gain=log_gain, reg=reg)


@pytest.mark.parametrize('mode', [lr.OBSERVED, lr.MODEL], ids=['observed', 'model'])
def test_restatement_gradients_equal_central_differences(mode):
    c = _fd_case()
    lam, lam_r = 0.75, 0.5
    out = lr.evaluate(c['coarse'], c['fine'], c['target'], c['codes'], c['row_codes'], c['noise'], c['log_gain'], mode, c['reg'],
                      lam, lam_r)
    base = {k: np.asarray(c[k], dtype=np.float64) for k in ('coarse', 'fine', 'log_gain', 'reg')}

    def parts(**changed):
        v = {**base, **changed}
        return lr.loss_parts_fp64(v['coarse'], v['fine'], c['target'], c['codes'], c['row_codes'], c['noise'], v['log_gain'], mode,
                                  v['reg'], lam, lam_r)
    slots, reg_term = parts()
    assert abs(slots.sum() + reg_term - out['loss']) <= 1e-14 * abs(out['loss'])
    # both branches of both clamps take part
    rows = lr.rows_of(c['codes'], c['row_codes'], c['fine'].shape)[0]
    m_fine = np.exp(np.float64(c['log_gain']))[rows] * c['fine']
    assert (m_fine[out['valid']] <= 0).any() and (m_fine[out['valid']] > 0).any()
    assert (c['target'][out['valid']] <= 0).any() and (c['target'][out['valid']] > 0).any()
    two_h = 2 * FD_STEP
    fd = {}
    # a prediction belongs to one slot: every slot is stepped at once and differenced on its own
    for name in ('coarse', 'fine'):
        fd[name] = (parts(**{name: base[name] + FD_STEP})[0] - parts(**{name: base[name] - FD_STEP})[0]) / two_h
    # a gain belongs to the slots of its row: their differences are added, not their sums differenced
    fd['log_gain'] = np.zeros(3)
    for k in range(3):
        step = np.zeros(3)
        step[k] = FD_STEP
        fd['log_gain'][k] = (parts(log_gain=base['log_gain'] + step)[0] - parts(log_gain=base['log_gain'] - step)[0]).sum() / two_h
    fd['reg'] = np.zeros(base['reg'].shape)
    for k in range(base['reg'].size):
        step = np.zeros(base['reg'].shape)
        step[k] = FD_STEP
        fd['reg'][k] = (parts(reg=base['reg'] + step)[1] - parts(reg=base['reg'] - step)[1]) / two_h
    scales = {'coarse': out['m_coarse'], 'fine': out['m_fine'], 'log_gain': lam / out['stats'][6] * out['magnitude'][:, 4],
              'reg': np.abs(out['d_reg'])}
    for name, grad in (('coarse', out['d_coarse']), ('fine', out['d_fine']), ('log_gain', out['d_log_gain']), ('reg', out['d_reg'])):
        scale = scales[name]
        err = np.abs(fd[name] - grad)
        masked = scale == 0
        assert not np.any(grad[masked]) and not np.any(fd[name][masked])
        rel = float((err[~masked] / scale[~masked]).max())
        print(f'mode {mode}, d loss / d {name}: largest |fd - analytic| = {rel:.3g} of the terms\' magnitudes (gate {FD_GATE})')
        assert rel <= FD_GATE
    assert int(masked.sum()) == 0 and int((scales['coarse'] == 0).sum()) == 3
    assert int(out['stats'][6]) == 16 * 3 - 3 and int(out['stats'][7]) == 1 and int(out['stats'][5]) == 0


def test_variance_is_the_square_of_instrument_errors():
    import torch
    from sunerf_hip.instrument import Instrument
    from sunerf_hip.likelihood import noise_table
    rng = np.random.default_rng(3)
    for quantise in (False, True):
        inst = Instrument(unit=[40.0, 12.0, 5.5], exposure=[2.9, 1.0, 0.7], dn_per_photon=[1.2, 0.8, 1.0], read_noise=[1.5, 2.0, 0.3],
                          quantise=quantise)
        table = noise_table(inst, (94, 171, 193))
        assert np.array_equal(table[:, 4], np.full(3, 1.0 / 12.0 if quantise else 0.0))
        image = (rng.uniform(-0.5, 2.0, (50, 3)) * 10.0 ** rng.integers(-3, 3, (50, 3))).astype(np.float32)
        want = inst.errors(torch.from_numpy(image)).numpy()
        got = np.sqrt(lr.variance(image.astype(np.float64), table[None])).astype(np.float32)
        ulp = np.spacing(want)
        worst = float((np.abs(got.astype(np.float64) - want.astype(np.float64)) / ulp).max())
        print(f'quantise {quantise}: sqrt(var(t)) against Instrument.errors, largest difference {worst:.3g} fp32 ulp')
        assert worst <= 1.0


def test_observed_mode_with_constant_sigma_is_the_mse_over_sigma_squared():
    rng = np.random.default_rng(4)
    coarse, fine, target = (rng.uniform(-1.0, 3.0, (37, 1)).astype(np.float32) for _ in range(3))
    s = 0.37
    noise = np.array([[1.0, 1.0, 1e-300, s, 0.0, 0.0, 0, 0]])
    out = lr.evaluate(coarse, fine, target, None, np.array([1.0], dtype=np.float32), noise, np.zeros(1, dtype=np.float32), lr.OBSERVED,
                      None, 1.0, 1.0)
    mse = lambda a: float(((a.astype(np.float64) - target.astype(np.float64)) ** 2).mean())          # noqa: E731
    want = (mse(coarse) + mse(fine)) / s ** 2
    assert abs(out['loss'] - want) <= 1e-12 * want
    assert abs(out['stats'][1] - mse(coarse) / s ** 2) <= 1e-12 * out['stats'][1]
    assert abs(out['stats'][4] + 10 * np.log10(mse(fine))) <= 1e-12 * abs(out['stats'][4])


@pytest.mark.parametrize('mode', [lr.OBSERVED, lr.MODEL], ids=['observed', 'model'])
def test_all_slots_masked_leaves_the_regularization_term(mode):
    c = lr.make_case(9, 3, 3, 0)
    codes = np.zeros_like(c['codes'])
    codes[::2] = 2500.0
    out = lr.evaluate(c['coarse'], c['fine'], c['target'], codes, c['row_codes'], c['noise'], c['log_gain'], mode, c['reg'], 1.0, 0.25)
    assert out['loss'] == 0.25 * np.float64(c['reg'].astype(np.float64).sum() / c['reg'].size)
    for k in ('g_coarse', 'g_fine', 'g_log_gain', 'channel_stats', 'd_coarse', 'd_fine', 'd_log_gain'):
        assert not np.any(out[k]), k
    assert np.isfinite(out['stats']).all() and out['stats'][6] == 0 and out['stats'][7] == 5 * 3


def test_the_parity_cases_mask_at_most_a_quarter_and_cross_both_clamps():
    for n, w, m in ((63, 3, 7), (257, 7, 64), (1, 1, 1)):
        c = lr.make_case(n, w, m, 0)
        out = lr.evaluate(c['coarse'], c['fine'], c['target'], c['codes'], c['row_codes'], c['noise'], c['log_gain'], lr.MODEL, c['reg'])
        assert out['stats'][6] >= n * w - (n * w) // 4
        if n > 1:
            assert out['stats'][7] > 0 and (c['coarse'] <= 0).any() and (c['fine'] < 0).any() and (c['target'][out['valid']] <= 0).any()
            assert len({tuple(r) for r in c['codes']}) > 1          # the rays' codes rows differ


# ---- 2. the seventh table ---------------------------------------------------------------------------------------------------------
def test_entry_points_are_declared_bound_and_kept_out_of_the_other_tables(lib):
    """(The table itself -- declared, bound, frozen, versioned, built, its symbols in no other table or older header:
    tests/test_abi_tables_host.py.)"""
    header = open(os.path.join(ROOT, 'include', 'sunerf_hip_likelihood.h')).read()
    assert lib.sunerf_abi_version() == 9 and lib.sunerf_ext_abi_version() == 1 and lib.sunerf_response_abi_version() == 1
    assert lib.sunerf_prep_abi_version() == 1 and lib.sunerf_instrument_abi_version() == 1 and lib.sunerf_patch_abi_version() == 1
    assert lib.sunerf_likelihood_abi_version() == 1
    assert '#define SUNERF_LIKELIHOOD_MAX_ROWS 64' in header
    assert 'sunerf/model/sunerf.py:105-125' in header and 'sunerf/model/sunerf.py:187-191' in header
    # the workspace query: a ticket line and 128 partials of 5 rows + 3 words; nothing outside 1 .. 64 rows
    assert [lib.sunerf_likelihood_workspace_bytes(m) for m in (0, 1, 64, 65, -1)] == [0, 64 + 128 * 8 * 8, 64 + 128 * 323 * 8, 0, 0]


def check_argument_order(lib):
    """Unsupported (-2) first, then the empty call (0), then bad counts and null pointers (-1), then the workspace (-3): all
    before anything touches a device, so this runs without one.  ``P`` stands for any non-null pointer: no call here reaches a
    launch."""
    P = ctypes.c_void_p(4096)
    fn = lib.sunerf_likelihood_loss
    big = 1 << 20

    def call(n_rays=4, n_columns=3, n_rows=2, mode=0, n_reg=0, n_fc=0, ptrs=None, codes=P, reg=None, fc=(None, None), ws_bytes=big):
        p = [P] * 12 if ptrs is None else ptrs
        return fn(p[0], p[1], p[2], codes, n_rays, n_columns, p[3], p[4], p[5], n_rows, mode, reg, n_reg, fc[0], fc[1], n_fc, 1.0, 1.0,
                  p[6], p[7], p[8], p[9], p[10], p[11], ws_bytes, None)
    none = [None] * 12
    assert call(n_rows=65, ptrs=none) == -2 and call(mode=2, ptrs=none) == -2 and call(mode=-1, ptrs=none) == -2
    assert call(n_fc=9, ptrs=none) == -2
    assert call(n_rays=-1, n_rows=65, ptrs=none) == -2 and call(n_rays=0, mode=3, ptrs=none) == -2      # unsupported comes first
    assert call(n_rays=0, ptrs=none, codes=None, ws_bytes=0) == 0 and call(n_columns=0, ptrs=none, codes=None, ws_bytes=0) == 0
    assert call(n_rays=0, n_columns=0, n_rows=64, mode=1, ptrs=none) == 0
    assert call(n_rays=-1) == -1 and call(n_columns=-1) == -1 and call(n_rays=0, n_columns=-1) == -1
    assert call(n_rows=0) == -1 and call(n_rays=0, n_rows=0) == -1                                       # no rows is no empty call
    assert call(n_reg=-1) == -1 and call(n_rays=0, n_reg=-1) == -1 and call(n_fc=-1) == -1
    assert call(n_rays=1 << 62, n_columns=4) == -1
    for k in range(12):
        ptrs = [P] * 12
        ptrs[k] = None
        assert call(ptrs=ptrs) == -1, k
    assert call(codes=None, ws_bytes=0) == -3                                         # NULL codes are legal: only the workspace check is left
    assert call(n_reg=5, reg=None) == -1 and call(n_reg=5, reg=P, ws_bytes=0) == -3
    assert call(n_fc=1) == -1                                                         # a count of tensors without their lists
    for k in (4, 8, 9, 11):                                                           # noise, g_log_gain, channel_stats, workspace
        ptrs = [P] * 12
        ptrs[k] = ctypes.c_void_p(4100)
        assert call(ptrs=ptrs) == -1, k
    one_short = lib.sunerf_likelihood_workspace_bytes(2) - 1
    assert call(ws_bytes=one_short) == -3 and call(ws_bytes=0) == -3


def test_argument_checks_come_in_the_documented_order(lib):
    check_argument_order(lib)


# ---- 3. NoiseLikelihood -----------------------------------------------------------------------------------------------------------
def test_noise_likelihood_lays_instruments_onto_rows_and_validates():
    import torch
    from sunerf_hip.instrument import Instrument
    from sunerf_hip.likelihood import NoiseLikelihood
    a = Instrument(unit=40.0, exposure=2.9, dn_per_photon=1.2, read_noise=[1.5, 2.5], quantise=True)
    b = Instrument(unit=10.0, read_noise=0.5)
    like = NoiseLikelihood({94: a, 10171: b, 171: a}, codes=(94, 10171, 171), mode='model', free=(10171,), gain_rate=25.0, floor=0.01)
    want = np.array([[40.0, 2.9, 1.2, 1.5, 1 / 12, 0.01, 0, 0], [10.0, 1.0, 1.0, 0.5, 0.0, 0.01, 0, 0],
                     [40.0, 2.9, 1.2, 2.5, 1 / 12, 0.01, 0, 0]])
    assert np.array_equal(like.noise.numpy(), want) and like.noise.dtype == torch.float64
    assert like.free.tolist() == [False, True, False] and like.row_codes.tolist() == [94.0, 10171.0, 171.0]
    assert like.log_gain.shape == (3,) and like.log_gain.requires_grad and float(like.log_gain.detach().abs().max()) == 0.0
    assert [n for n, _ in like.named_parameters()] == ['log_gain'] and 'log_gain' in like.state_dict()
    with torch.no_grad():
        like.log_gain[1] = 0.01
    assert torch.allclose(like.gains(), torch.tensor([1.0, np.exp(0.25), 1.0], dtype=torch.float64), rtol=1e-6)
    stats = torch.tensor([[4.0, 1.0, 6.0, 0.0], [2.0, 1.0, 3.0, 0.0], [1.0, 0.0, 0.5, 0.0]], dtype=torch.float64)
    assert like.reduced_chi2(stats).tolist() == [1.5, 1.5, 0.5]
    frozen = NoiseLikelihood(b)
    assert frozen.n_rows == 1 and frozen.single_row and not any(p.requires_grad for p in frozen.parameters())
    assert NoiseLikelihood(b, free='all').log_gain.requires_grad
    with pytest.raises(ValueError, match='sigma is 0'):
        NoiseLikelihood(Instrument(unit=40.0))                                        # no read noise, no quantisation, no floor
    assert NoiseLikelihood(Instrument(unit=40.0), floor=1e-3).n_rows == 1 and NoiseLikelihood(Instrument(quantise=True)).n_rows == 1
    with pytest.raises(ValueError, match='no row'):
        NoiseLikelihood(b, codes=(94, 171), free=(193,))
    with pytest.raises(ValueError):
        NoiseLikelihood(b, codes=tuple(range(1, 66)))                                 # 65 rows
    assert NoiseLikelihood(b, codes=tuple(range(1, 65))).n_rows == 64
    with pytest.raises(ValueError, match='read_noise has 2 values'):
        NoiseLikelihood(a, codes=(94, 171, 193))                                      # two values onto three rows
    with pytest.raises(ValueError, match='no instrument'):
        NoiseLikelihood({94: b}, codes=(94, 171))
    with pytest.raises(ValueError):
        NoiseLikelihood(b, mode='poisson')


def test_lightning_modules_take_a_likelihood_and_hand_its_gains_to_the_optimiser_list():
    from sunerf.model.sunerf import EmissionSuNeRFModule
    from sunerf_hip.instrument import Instrument
    from sunerf_hip.likelihood import NoiseLikelihood
    config = lambda: dict(Rs_per_ds=1.0, seconds_per_dt=1.0, image_scaling_config={'vmax': 1, 'a': 0.005},          # noqa: E731
                          sampling_config={'type': 'stratified', 'n_samples': 8, 'perturb': False},
                          hierarchical_sampling_config={'type': 'hierarchical', 'n_samples': 8}, model_config={'d_filter': 64})
    plain = EmissionSuNeRFModule(**config())
    assert plain.likelihood is None and not any('likelihood' in k for k in plain.state_dict())
    like = NoiseLikelihood(Instrument(read_noise=1.0), free='all')
    mod = EmissionSuNeRFModule(likelihood=like, **config())
    assert 'likelihood.log_gain' in mod.state_dict()
    assert any(p is like.log_gain for p in mod._trainable_parameters())
    frozen = EmissionSuNeRFModule(likelihood=NoiseLikelihood(Instrument(read_noise=1.0)), **config())
    assert not any(p is frozen.likelihood.log_gain for p in frozen._trainable_parameters())
