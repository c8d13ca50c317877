"""CPU-only checks of the trainable PSF (no GPU): the tenth entry-point table (declared, bound, its argument checks in
their documented order, the workspace query), the stamps of TrainablePSF against gaussian_psf / moffat_psf, the host chain rule
(stamp -> flip -> box) against the transpose of tests/psf_grad_reference.py, the modules' ``psf_models`` and the restatement's own
calibration fit.  Bounds are reasoned in each test's docstring; every figure is printed."""
import ctypes
import io
import os

import numpy as np
import pytest
import torch

import psf_grad_reference as pr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

@pytest.fixture(scope='session')
def lib():
    import sunerf_hip
    if not os.path.exists(sunerf_hip.LIB_PATH):
        import subprocess
        subprocess.check_call(['bash', os.path.join(ROOT, '2024-hl-spi3s-sunerf_amd', 'csrc', 'build.sh')])
    return sunerf_hip.load()


# ---- the tenth table --------------------------------------------------------------------------------------------------------------
def test_entry_points_are_declared_and_bound(lib):
    """(The table itself -- declared, bound, frozen, versioned, built: tests/test_abi_tables_host.py.)"""
    assert lib.sunerf_psf_grad_abi_version() == 1


def test_workspace_query(lib):
    """8 bytes per tap, kernel index and run; runs = min(items, max(1, 512 / n_kernels)) with items the (plane, tile) pairs of one
    kernel index, T = min(32, (127 - k) / bin + 1).  The cap holds at 4096^2 under 33 x 33: 512 runs, 4.5 MB."""
    q = lib.sunerf_psf_grad_workspace_bytes
    valid = [((1, 5, 7, 1, 1, 1, 1), 1 * 1 * 8), ((2, 33, 65, 1, 3, 3, 1), 2 * 2 * 3 * 9 * 8), ((2, 33, 65, 2, 3, 3, 1), 2 * 6 * 9 * 8),
             ((21, 48, 48, 7, 18, 18, 2), 7 * 3 * 324 * 8), ((1, 40, 40, 1, 96, 96, 8), 4 * 9216 * 8),
             ((1, 4096, 4096, 1, 33, 33, 1), 512 * 1089 * 8), ((1024, 8, 8, 1024, 3, 3, 1), 1024 * 9 * 8)]
    assert [q(*a) for a, _ in valid] == [b for _, b in valid]
    invalid = [(0, 5, 7, 1, 1, 1, 1), (-1, 5, 7, 1, 1, 1, 1), (1, 5, 7, 1, 97, 1, 1), (1, 5, 7, 1, 1, 1, 9), (1, 5, 7, 1, 0, 1, 1),
               (1, 1, 7, 1, 1, 1, 2), (4, 5, 7, 3, 1, 1, 1), (4, 5, 7, 0, 1, 1, 1), (1, 0, 7, 1, 1, 1, 1)]
    assert [q(*a) for a in invalid] == [0] * len(invalid)


def check_argument_order(lib):
    """Limits (-2) first, then the empty call (0), then counts, n_kernels, anchors, null pointers and alignment (-1): all before
    anything touches a device, so this runs without one.  ``Q`` stands for any non-null aligned pointer: no call here reaches a
    launch."""
    Q = ctypes.c_void_p(4096)
    fn = lib.sunerf_psf_grad_taps
    names = ('inp', 'g_out', 'g_K', 'workspace')

    def call(n_planes=6, h=9, w=11, n_kernels=1, kh=3, kw=5, b=1, ay=1, ax=2, scale=1.0, boundary=1, **ptrs):
        p = {k: Q for k in names}
        p.update(ptrs)
        return fn(p['inp'], p['g_out'], n_planes, h, w, n_kernels, kh, kw, b, ay, ax, scale, boundary, p['g_K'], p['workspace'], None)
    none = {k: None for k in names}
    assert call(kh=97, **none) == -2 and call(kw=97, **none) == -2 and call(b=9, **none) == -2
    assert call(boundary=2, **none) == -2 and call(boundary=-1, **none) == -2
    assert call(kh=97, n_planes=0, **none) == -2 and call(b=9, n_planes=-1, **none) == -2          # the limits come first
    for empty in (dict(n_planes=0), dict(h=0), dict(w=0), dict(h=1, b=2), dict(w=3, b=4)):
        assert call(n_kernels=7, ay=-1, **empty, **none) == 0, empty                               # then the empty call
    assert call(n_planes=-1) == -1 and call(h=-1) == -1 and call(kh=0) == -1 and call(b=0) == -1 and call(n_planes=-1, h=0) == -1
    assert call(n_kernels=4) == -1 and call(n_kernels=0) == -1 and call(n_kernels=-1) == -1 and call(n_kernels=12) == -1
    assert call(ay=3) == -1 and call(ax=-1) == -1 and call(ax=5) == -1
    for k in names:
        assert call(**{k: None}) == -1, k
    for k in ('g_K', 'workspace'):
        assert call(**{k: ctypes.c_void_p(4100)}) == -1, k
    # every divisor of n_planes passes the checks: with all pointers null the next refusal is the pointers', not n_kernels'
    assert all(call(n_kernels=d, **none) == -1 for d in (1, 2, 3, 6))


def test_argument_checks_come_in_the_documented_order(lib):
    check_argument_order(lib)


# ---- stamps -----------------------------------------------------------------------------------------------------------------------
def _ulps(got, want):
    return float((np.abs(got - want) / np.spacing(np.abs(want))).max())


def test_gaussian_and_moffat_stamps_are_the_formulas_of_the_instrument():
    """Same operations in the same order as gaussian_psf / moffat_psf; exp, pow and the sum of the stamp may differ between torch
    and NumPy by an ulp each, the division rounds once: 4 ulp of fp64, shared and per channel.  The reference takes the model's own
    ``fwhm`` (exp of the float32 parameter), so the parameter's rounding is not part of the comparison."""
    from sunerf_hip.instrument import gaussian_psf, moffat_psf
    from sunerf_hip.psf_fit import TrainablePSF
    worst = 0.0
    for fwhm in (2.5, (1.7, 3.0, 4.4)):
        for rate in (1.0, 0.1):
            g = TrainablePSF.gaussian(fwhm, 6, rate=rate)
            m = TrainablePSF.moffat(fwhm, 2.5 if np.isscalar(fwhm) else (2.5, 3.5, 4.7), 7, rate=rate, train_beta=True)
            gs, ms = g.stamp().detach().numpy(), m.stamp().detach().numpy()
            assert gs.dtype == np.float64 and gs.shape == (g.n, 13, 13) and ms.shape == (m.n, 15, 15)
            assert g.n == m.n == (1 if np.isscalar(fwhm) else 3)
            np.testing.assert_allclose(g.fwhm.numpy(), np.atleast_1d(fwhm), rtol=1e-6)
            for c in range(g.n):
                worst = max(worst, _ulps(gs[c], gaussian_psf(float(g.fwhm[c]), 6)))
                worst = max(worst, _ulps(ms[c], moffat_psf(float(m.fwhm[c]), float(m.beta[c]), 7)))
            assert g.numpy().shape == ((13, 13) if g.n == 1 else (3, 13, 13))
    print(f'largest difference between a TrainablePSF stamp and the instrument formula: {worst:.2f} ulp')
    assert worst <= 4.0
    per_channel = TrainablePSF.gaussian(2.0, 3, channels=4)
    assert per_channel.n == 4 and per_channel.log_fwhm.dtype == torch.float32
    assert not TrainablePSF.moffat(2.0, 3.0, 3).log_beta.requires_grad and TrainablePSF.moffat(2.0, 3.0, 3, train_beta=True).log_beta.requires_grad


def test_free_stamp_is_non_negative_and_sums_to_one():
    from sunerf_hip.psf_fit import TrainablePSF
    rng = np.random.default_rng(5)
    start = rng.uniform(0.0, 1.0, size=(2, 5, 7))
    start[0, 2, 3] = 0.0
    psf = TrainablePSF.free(start, rate=0.5)
    s = psf.stamp().detach().numpy()
    assert s.shape == (2, 5, 7) and (s >= 0).all() and psf.fwhm is None
    np.testing.assert_allclose(s.sum(axis=(1, 2)), 1.0, rtol=0, atol=4 * 2.0 ** -52)
    np.testing.assert_allclose(s, start / start.sum(axis=(1, 2), keepdims=True), rtol=1e-6, atol=1e-29)      # float32 logits
    with torch.no_grad():
        psf.logits.add_(torch.randn(psf.logits.shape) * 3.0)
    s = psf.stamp().detach().numpy()
    assert (s >= 0).all()
    np.testing.assert_allclose(s.sum(axis=(1, 2)), 1.0, rtol=0, atol=4 * 2.0 ** -52)
    np.testing.assert_allclose(s[1], pr.free_stamp(0.5 * psf.logits[1].detach().double().numpy()), rtol=1e-14)


# ---- the host chain rule ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('b', [1, 2, 3])
def test_flip_and_box_autograd_is_the_transpose(b):
    """``<A psf, Y> == <psf, A^T Y>`` with A = effective_kernel_of (torch, its autograd giving A^T Y) and A^T the restatement's
    flip_box_transpose: sums of 15 x 12 products of O(1) values in fp64, 1e-14 relative to sum |psf| |A^T |Y||."""
    from sunerf_hip.psf_fit import effective_kernel_of
    rng = np.random.default_rng(b)
    psf = torch.tensor(rng.standard_normal((2, 5, 4)), requires_grad=True)
    Y = rng.standard_normal((2, 5 + b - 1, 4 + b - 1))
    K = effective_kernel_of(psf, b)
    for c in range(2):
        assert np.array_equal(K[c].detach().numpy(), pr.flip_box(psf[c].detach().numpy(), b))
    (K * torch.tensor(Y)).sum().backward()
    for c in range(2):
        want = pr.flip_box_transpose(Y[c], b)
        lhs, rhs = float((K[c].detach().numpy() * Y[c]).sum()), float((psf[c].detach().numpy() * want).sum())
        mass = float((np.abs(psf[c].detach().numpy()) * pr.flip_box_transpose(np.abs(Y[c]), b)).sum())
        print(f'bin {b} channel {c}: <A psf, Y> {lhs:.15g}, <psf, A^T Y> {rhs:.15g}, difference {abs(lhs - rhs):.2e}')
        assert abs(lhs - rhs) <= 1e-14 * mass
        assert np.abs(psf.grad[c].numpy() - want).max() <= 1e-14 * np.abs(Y[c]).sum()


def test_stamp_derivatives_of_the_restatement_match_autograd():
    """The restatement's analytic derivatives (what the GPU test carries the tap gradient through) against torch's autograd of
    TrainablePSF.stamp: both fp64, a handful of operations per tap: 1e-10 relative to the largest derivative (the float32
    parameter is the same on both sides: the restatement is given the model's own fwhm and beta)."""
    from sunerf_hip.psf_fit import TrainablePSF
    rng = np.random.default_rng(2)
    g = rng.standard_normal((9, 9))
    gauss = TrainablePSF.gaussian(2.3, 4, rate=0.5)
    (gauss.stamp()[0] * torch.tensor(g)).sum().backward()
    want = 0.5 * float((pr.gaussian_stamp(float(gauss.fwhm[0]), 4)[1] * g).sum())
    assert abs(float(gauss.log_fwhm.grad[0]) - want) <= 1e-6 * abs(want)          # the gradient is stored in float32
    mof = TrainablePSF.moffat(2.3, 2.8, 4, train_beta=True)
    (mof.stamp()[0] * torch.tensor(g)).sum().backward()
    _, df, db = pr.moffat_stamp(float(mof.fwhm[0]), float(mof.beta[0]), 4)
    assert abs(float(mof.log_fwhm.grad[0]) - float((df * g).sum())) <= 1e-6 * abs(float((df * g).sum()))
    assert abs(float(mof.log_beta.grad[0]) - float((db * g).sum())) <= 1e-6 * abs(float((db * g).sum()))
    free = TrainablePSF.free(rng.uniform(0.1, 1.0, size=(9, 9)), rate=2.0)
    (free.stamp()[0] * torch.tensor(g)).sum().backward()
    want = 2.0 * pr.free_stamp_vjp(free.stamp()[0].detach().numpy(), g)
    np.testing.assert_allclose(free.logits.grad[0].numpy(), want, rtol=1e-6, atol=1e-9)


def test_fitted_instrument_has_the_effective_kernel_of_its_stamp():
    from sunerf_hip.instrument import Instrument
    from sunerf_hip.psf_fit import FittedInstrument, TrainablePSF, effective_kernel_of
    for psf in (TrainablePSF.gaussian(2.5, 4), TrainablePSF.moffat((2.0, 3.0), 3.0, 5), TrainablePSF.free(np.ones((3, 5)))):
        for b in (1, 2, 3):
            fitted = FittedInstrument(psf, bin=b, unit=40.0, read_noise=1.2, boundary='zero', bin_mode='sum')
            plain = Instrument(psf=fitted.psf, bin=b)
            K, anchor = fitted.effective_kernel()
            K0, anchor0 = plain.effective_kernel()
            assert anchor == anchor0 and np.array_equal(K.view(np.uint64), K0.view(np.uint64))
            assert np.array_equal(effective_kernel_of(psf.stamp().detach(), b).numpy().view(np.uint64), K0.view(np.uint64))
            assert fitted.window_shape(4) == plain.window_shape(4)
            frozen = fitted.freeze()
            assert type(frozen) is Instrument and np.array_equal(frozen.psf, fitted.psf)
            assert (frozen.bin, frozen.bin_mode, frozen.boundary, float(frozen.unit), float(frozen.read_noise)) == (b, 'sum', 'zero', 40.0, 1.2)
    moving = FittedInstrument(TrainablePSF.gaussian(2.0, 4))
    before = moving.psf.copy()
    with torch.no_grad():
        moving.psf_model.log_fwhm.add_(0.2)
    assert not np.array_equal(before, moving.psf) and moving.psf.shape == before.shape          # psf is the current stamp
    with pytest.raises(ValueError):
        FittedInstrument(TrainablePSF.gaussian(2.0, 46), bin=8)                                 # 93 + 7 taps
    with pytest.raises(TypeError):
        FittedInstrument(np.ones((3, 3)))


# ---- modules ------------------------------------------------------------------------------------------------------------------------
def _config():
    return dict(Rs_per_ds=1.0, seconds_per_dt=1.0, image_scaling_config={'vmax': 1, 'a': 0.005},
                sampling_config={'type': 'stratified', 'n_samples': 8, 'perturb': False},
                hierarchical_sampling_config={'type': 'hierarchical', 'n_samples': 8}, model_config={'d_filter': 64})


def test_modules_take_psf_models_and_hand_their_parameters_to_the_optimiser_list():
    from sunerf.model.sunerf import EmissionSuNeRFModule
    from sunerf_hip.psf_fit import TrainablePSF
    plain = EmissionSuNeRFModule(**_config())
    assert plain.psf_models is None and not any('psf' in k for k in plain.state_dict())
    assert set(plain.state_dict()) == ({'rendering.' + k for k in plain.rendering.state_dict()}
                                       | {'image_scaling.' + k for k in plain.image_scaling.state_dict()})
    today = plain._trainable_parameters()
    assert len(today) == len(list(plain.rendering.parameters())) and all(a is b for a, b in zip(today, plain.rendering.parameters()))
    psf = TrainablePSF.moffat(2.0, 3.0, 4)                                 # log_beta is frozen
    mod = EmissionSuNeRFModule(psf_models=psf, **_config())
    assert {'psf_models.0.log_fwhm', 'psf_models.0.log_beta'} <= set(mod.state_dict())
    assert set(mod.state_dict()) - set(plain.state_dict()) == {'psf_models.0.log_fwhm', 'psf_models.0.log_beta'}
    params = mod._trainable_parameters()
    assert any(p is psf.log_fwhm for p in params) and not any(p is psf.log_beta for p in params)
    assert len(params) == len(today) + 1
    two = EmissionSuNeRFModule(psf_models=[TrainablePSF.gaussian(2.0, 3), TrainablePSF.free(np.ones((3, 3)))], **_config())
    assert {'psf_models.0.log_fwhm', 'psf_models.1.logits'} <= set(two.state_dict())
    assert len(two._trainable_parameters()) == len(today) + 2
    # a checkpoint round trip restores log_fwhm
    with torch.no_grad():
        psf.log_fwhm.fill_(0.321)
    buffer = io.BytesIO()
    torch.save(mod.state_dict(), buffer)
    buffer.seek(0)
    back = EmissionSuNeRFModule(psf_models=TrainablePSF.moffat(5.0, 2.0, 4), **_config())
    back.load_state_dict(torch.load(buffer))
    assert back.psf_models[0].log_fwhm.detach()[0].item() == psf.log_fwhm.detach()[0].item() == float(np.float32(0.321))
    assert back.psf_models[0].log_beta.detach()[0].item() == psf.log_beta.detach()[0].item()


# ---- the restatement's own fit --------------------------------------------------------------------------------------------------------
def test_the_restatement_fits_the_hidden_fwhm():
    """The calibration problem of the GPU test on the restatement alone: observed with a hidden FWHM of 3.0, Adam from 2.0 at
    lr = 0.05 for 200 steps on the mean square.  Noise-free data and one parameter: the minimum is the hidden value, and the
    torch-CPU fp64 equivalent of this loop reached 5.4e-6 relative; required 1e-4."""
    scene = pr.fit_scene()
    assert scene.shape == (2, 48, 48) and scene.dtype == np.float32
    observed = pr.observe(scene, pr.FIT['hidden'])
    fwhm, losses = pr.fit_gaussian(scene, observed, pr.FIT['start'], pr.FIT['steps'], pr.FIT['lr'])
    print(f'fitted FWHM {fwhm:.9f} (hidden {pr.FIT["hidden"]}), relative error {abs(fwhm - 3.0) / 3.0:.3e}; loss {losses[0]:.3e} -> {losses[-1]:.3e}')
    assert abs(fwhm - pr.FIT['hidden']) <= 1e-4 * pr.FIT['hidden']
    assert losses[-1] < 1e-6 * losses[0]


def test_the_restatement_is_the_derivative_of_its_own_correlation():
    """tap_gradient against central differences of correlate_bin on a 3 x 4 kernel (bin 2, both boundaries, two kernel indices
    over four planes): the correlation is linear in K, so the difference quotient is exact up to rounding: 1e-9 relative."""
    rng = np.random.default_rng(4)
    planes, g = rng.standard_normal((4, 9, 10)).astype(np.float32), rng.standard_normal((4, 4, 5)).astype(np.float32)
    for boundary in (pr.ZERO, pr.NEAREST):
        got = pr.tap_gradient(planes, g, 2, 3, 4, 2, 2, 0, 0.25, boundary)
        K = rng.standard_normal((2, 3, 4))
        for k, i, j in ((0, 0, 0), (1, 2, 3), (0, 1, 2)):
            dK = np.zeros_like(K)
            dK[k, i, j] = 1.0
            quotient = ((pr.correlate_bin(planes, K + dK, 2, 2, 0, 0.25, boundary) - pr.correlate_bin(planes, K - dK, 2, 2, 0, 0.25, boundary)) * g).sum() / 2
            assert abs(got[k, i, j] - quotient) <= 1e-9 * np.abs(got).max()
