"""The tap gradient of the PSF-and-bin correlation on the device (include/sunerf_hip_psf_grad.h, csrc/psf_grad.hip)
against the fp64 restatement tests/psf_grad_reference.py, and the trainable PSF of sunerf_hip/psf_fit.py end to end.

Gate of the kernel.  Every addition rounds once and the products of two fp32 values are exact in fp64, so for a tap that sums N
terms, whatever the order of the additions,

    |g_K - ref| <= 2 (N + 2) 2^-53 scale sum |g_out| |in_b|

(N - 1 additions and the final ``* scale``, each (1 + 2^-53); the factor 2 covers the restatement's own rounding).  The right-hand
side is ``psf_grad_reference.tap_gradient_bound``: derived, not measured.  Every figure is printed before it is asserted."""
import functools

import numpy as np
import pytest
import torch

import psf_grad_reference as pr

pytestmark = pytest.mark.gpu
DEV = 'cuda'
ZERO, NEAREST = pr.ZERO, pr.NEAREST

# name: (planes, height, width, n_kernels, kh, kw, bin, anchor_y, anchor_x, boundary)
CASES = {
    '1-dot-product': (1, 5, 7, 1, 1, 1, 1, 0, 0, NEAREST),                  # 1 x 1 at bin 1: the plain dot product
    '2-anchor': (2, 9, 11, 1, 3, 5, 1, 2, 0, NEAREST),                      # a non-central anchor, kh != kw
    '3-trailing': (1, 10, 11, 1, 4, 4, 3, 1, 2, ZERO),                      # trailing rows and columns fill no detector pixel
    '4-clamped-nearest': (1, 5, 7, 1, 9, 9, 1, 4, 4, NEAREST),              # every tap is clamped somewhere
    '4-clamped-zero': (1, 5, 7, 1, 9, 9, 1, 4, 4, ZERO),
    '5-seams': (1, 33, 65, 1, 3, 3, 1, 1, 1, NEAREST),                      # tile seams on both axes, fewer taps than threads
    '6-largest': (1, 40, 40, 1, 96, 96, 8, 47, 50, NEAREST),                # the tile shrinks to 4; nine chunks of taps
    '7-odd-taps': (1, 6, 5, 1, 95, 96, 1, 10, 90, ZERO),                    # more taps than threads, an odd count
    '8-patch-shared': (7, 48, 48, 1, 18, 18, 2, 0, 0, ZERO),                # the patch shape
    '8-patch-per-plane': (7, 48, 48, 7, 18, 18, 2, 0, 0, ZERO),
    '8-patch-per-channel': (21, 48, 48, 7, 18, 18, 2, 0, 0, ZERO),          # planes laid out [3, 7]
    '9-long-runs': (1040, 4, 4, 1, 2, 2, 1, 0, 1, NEAREST),                 # 1040 items in 512 runs of 2 or 3: a run spans planes
    '9-one-run-each': (1040, 4, 4, 260, 2, 2, 1, 0, 1, ZERO),               # more kernel indices than runs: one run of 4 planes each
    # taps per thread: 1 in cases 1, 2, 5 and the first two here, 2 in the cases 9, 3 in the last one here, 4 in the others
    '10-one-pair': (2, 19, 27, 1, 1, 1, 8, 0, 0, ZERO),                     # T = 16: 16 x 4 slices (rows x column segments) of one tap
    '10-two-pairs': (2, 19, 27, 2, 1, 2, 8, 0, 1, NEAREST),                 # 64 slices of two taps, a kernel per plane
    '10-three-pairs': (1, 6, 5, 1, 33, 33, 1, 16, 16, NEAREST),             # 1089 taps: two chunks of 545, three per thread
}
SCALE = 0.25


@functools.lru_cache(maxsize=None)
def _inputs(name):
    n, h, w, nk, kh, kw, b, ay, ax, boundary = CASES[name]
    rng = np.random.default_rng(sum(map(ord, name)))
    planes = rng.standard_normal((n, h, w)).astype(np.float32)
    g = rng.standard_normal((n, h // b, w // b)).astype(np.float32)
    if name.startswith('8-'):
        g[:, 16:, :] = 0.0
        g[:, :, 16:] = 0.0
    return planes, g


@functools.lru_cache(maxsize=None)
def _reference(name):
    """(ref, bound) of a case, computed once and never written to."""
    n, h, w, nk, kh, kw, b, ay, ax, boundary = CASES[name]
    planes, g = _inputs(name)
    ref = pr.tap_gradient(planes, g, nk, kh, kw, b, ay, ax, SCALE, boundary)
    bound = pr.tap_gradient_bound(planes, g, nk, kh, kw, b, ay, ax, SCALE, boundary)
    ref.setflags(write=False)
    bound.setflags(write=False)
    return ref, bound


def _device(name, planes=None, g=None):
    from sunerf_hip.psf_fit import tap_gradient
    n, h, w, nk, kh, kw, b, ay, ax, boundary = CASES[name]
    p0, g0 = _inputs(name)
    planes = torch.from_numpy(p0 if planes is None else planes).to(DEV)
    g = torch.from_numpy(g0 if g is None else g).to(DEV)
    return tap_gradient(planes, g, nk, kh, kw, b, ay, ax, SCALE, boundary)


@pytest.mark.parametrize('name', list(CASES))
def test_tap_gradient_matches_the_definition(name):
    ref, bound = _reference(name)
    got = _device(name).cpu().numpy()
    assert got.shape == ref.shape and got.dtype == np.float64
    err = np.abs(got - ref)
    used = float((err / np.maximum(bound, 1e-300)).max())
    print(f'{name}: largest |g_K - ref| {err.max():.3e}, largest bound {bound.max():.3e}, {used:.3f} of the bound used at most')
    assert np.isfinite(got).all() and (err <= bound).all()


def test_dot_product_case_is_the_plain_dot_product():
    planes, g = _inputs('1-dot-product')
    got = float(_device('1-dot-product').cpu()[0, 0, 0])
    want = SCALE * float((planes.astype(np.float64) * g.astype(np.float64)).sum())
    assert abs(got - want) <= 2 * 37 * 2.0 ** -53 * SCALE * float(np.abs(planes.astype(np.float64) * g.astype(np.float64)).sum())


@pytest.mark.parametrize('name', ['5-seams', '8-patch-per-channel', '6-largest'])
def test_zero_cotangent_gives_positive_zero(name):
    _, g = _inputs(name)
    got = _device(name, g=np.zeros_like(g))
    assert torch.equal(got.view(torch.int64), torch.zeros_like(got, dtype=torch.int64))          # the bits of +0.0


def test_nan_reaches_exactly_the_taps_of_its_kernel_index():
    """The definition sums every detector pixel of every plane of a kernel index into every tap of that index (under ``zero`` the
    product with the 0 outside the frame is formed all the same): a NaN in g_out[p] reaches all taps of index p % n_kernels and
    no tap of another index."""
    name = '8-patch-per-channel'
    _, g = _inputs(name)
    g = g.copy()
    g[10, 3, 5] = np.nan                                                    # plane 10 of [3, 7]: kernel index 3
    got = _device(name, g=g).cpu().numpy()
    ref, bound = _reference(name)
    assert np.isnan(got[3]).all()
    others = [k for k in range(7) if k != 3]
    assert (np.abs(got[others] - ref[others]) <= bound[others]).all()
    shared = _device('5-seams', g=np.where(np.arange(33 * 65).reshape(1, 33, 65) == 1234, np.nan, _inputs('5-seams')[1]).astype(np.float32))
    assert bool(torch.isnan(shared).all())


@pytest.mark.parametrize('name', ['5-seams', '8-patch-per-channel', '9-long-runs', '7-odd-taps'])
def test_reruns_are_bit_identical(name):
    first = _device(name).clone()
    second = _device(name).clone()
    assert torch.equal(first.view(torch.int64), second.view(torch.int64))
    # an unrelated launch on the same stream in between: another shape through the same workspace, and a torch kernel
    _device('3-trailing')
    torch.full((1 << 16,), float('nan'), device=DEV).sum()
    third = _device(name)
    assert torch.equal(first.view(torch.int64), third.view(torch.int64))


def test_wrapper_checks_its_arguments():
    from sunerf_hip.lib import SunerfHipError
    from sunerf_hip.psf_fit import tap_gradient
    planes, g = torch.zeros(4, 6, 6, device=DEV), torch.zeros(4, 3, 3, device=DEV)
    assert torch.equal(tap_gradient(planes[:, :1], g[:, :0], 2, 3, 3, 2, 1, 1, 1.0, 0), torch.zeros(2, 3, 3, dtype=torch.float64, device=DEV))
    with pytest.raises(SunerfHipError):
        tap_gradient(planes.cpu(), g.cpu(), 1, 3, 3, 2, 1, 1, 1.0, 0)
    with pytest.raises(ValueError):
        tap_gradient(planes, g, 3, 3, 3, 2, 1, 1, 1.0, 0)                   # 3 does not divide 4
    with pytest.raises(ValueError):
        tap_gradient(planes.double(), g, 1, 3, 3, 2, 1, 1, 1.0, 0)
    with pytest.raises(ValueError):
        tap_gradient(planes, g[:, :2], 1, 3, 3, 2, 1, 1, 1.0, 0)
    with pytest.raises(ValueError):
        tap_gradient(planes, g, 1, 97, 3, 2, 1, 1, 1.0, 0)                  # the library's UNSUPPORTED


# ---- end to end ---------------------------------------------------------------------------------------------------------------------
def _models():
    from sunerf_hip.psf_fit import TrainablePSF
    rng = np.random.default_rng(8)
    return {
        'gaussian-shared': lambda: TrainablePSF.gaussian(2.2, 3, rate=0.5),
        'gaussian-per-channel': lambda: TrainablePSF.gaussian((1.8, 2.9), 3),
        'moffat-shared': lambda: TrainablePSF.moffat(2.4, 2.8, 3, train_beta=True),
        'moffat-per-channel': lambda: TrainablePSF.moffat((2.0, 3.1), (2.5, 3.5), 3, rate=2.0, train_beta=True),
        'free-shared': lambda: TrainablePSF.free(rng.uniform(0.1, 1.0, size=(5, 7))),
        'free-per-channel': lambda: TrainablePSF.free(rng.uniform(0.1, 1.0, size=(2, 5, 7)), rate=0.5),
    }


def _chain_reference(model, g_K, bound_K, b):
    """{parameter: (gradient, gate)} by the restatement: A^T of the tap gradient, then the stamp's derivative.  The gate is the
    kernel's bound carried through the same (linear) chain with absolute values, plus 1e-12 of the chain's mass for the host's
    fp64 (the device's exp / pow against NumPy's, a handful of roundings per tap)."""
    out = {}
    rate = model.rate
    for c in range(model.n):
        g_psf = pr.flip_box_transpose(g_K[c], b)
        bound_psf = pr.flip_box_transpose(bound_K[c], b)
        mass_psf = pr.flip_box_transpose(np.abs(g_K[c]), b)
        if model.kind == 'free':
            p = model.stamp()[c].detach().cpu().numpy()
            grad = rate * pr.free_stamp_vjp(p, g_psf)
            # |d/dlogit_t| <= p_t (|g_t| + sum |g| p): the same form with absolute values
            gate = rate * p * (bound_psf + (bound_psf * p).sum()) + 1e-12 * rate * p * (mass_psf + (mass_psf * p).sum())
            out.setdefault('logits', []).append((grad, gate))
            continue
        if model.kind == 'gaussian':
            derivs = {'log_fwhm': pr.gaussian_stamp(float(model.fwhm[c]), model.radius)[1]}
        else:
            _, df, db = pr.moffat_stamp(float(model.fwhm[c]), float(model.beta[c]), model.radius)
            derivs = {'log_fwhm': df, 'log_beta': db}
        for key, dp in derivs.items():
            grad = rate * float((g_psf * dp).sum())
            gate = rate * float((bound_psf * np.abs(dp)).sum()) + 1e-12 * rate * float((mass_psf * np.abs(dp)).sum())
            out.setdefault(key, []).append((grad, gate))
    return out


def _check_parameters(label, model, reference):
    for key, rows in reference.items():
        got = getattr(model, key).grad.detach().cpu().numpy()
        assert got.dtype == np.float64
        for c, (want, gate) in enumerate(rows):
            err = np.abs(got[c] - want)
            print(f'{label} {key}[{c}]: largest |gradient| {np.abs(want).max():.6e}, largest error {err.max():.3e}, '
                  f'{float((err / np.maximum(gate, 1e-300)).max()):.3f} of the gate used at most')
            assert np.isfinite(got[c]).all() and (err <= gate).all()
            assert np.abs(want).max() > 0


@pytest.mark.parametrize('kind', list(_models()))
@pytest.mark.parametrize('b,boundary', [(1, 'nearest'), (2, 'zero')])
def test_expected_gradients(kind, b, boundary):
    """``FittedInstrument.expected`` under a random fp64 cotangent: the PSF parameters' gradients against the restatement's chain
    (the model is taken to fp64 with ``.double()`` so that the gradient is not rounded to the float32 of the stored parameter),
    the planes' gradient by bits against ``Instrument.expected`` with the same stamp, the frozen forward by bits."""
    from sunerf_hip.instrument import BOUNDARY, Instrument
    from sunerf_hip.psf_fit import FittedInstrument
    model = _models()[kind]().double().to(DEV)
    fitted = FittedInstrument(model, bin=b, boundary=boundary)
    plain = Instrument(psf=fitted.psf, bin=b, boundary=boundary)
    rng = np.random.default_rng(3 + b)
    planes_np = rng.standard_normal((2, 13, 15)).astype(np.float32)
    cot = rng.standard_normal((2, 13 // b, 15 // b))
    planes = torch.from_numpy(planes_np).to(DEV).requires_grad_(True)
    out = fitted.expected(planes)
    (out.double() * torch.from_numpy(cot).to(DEV)).sum().backward()
    K, (ay, ax) = plain.effective_kernel()
    g32 = cot.astype(np.float32)
    call = (model.n, K.shape[1], K.shape[2], b, ay, ax, plain.scale, BOUNDARY[boundary])
    reference = _chain_reference(model, pr.tap_gradient(planes_np, g32, *call), pr.tap_gradient_bound(planes_np, g32, *call), b)
    _check_parameters(f'{kind} bin {b} {boundary}', model, reference)
    # the planes' gradient and the forward: the bits of the plain instrument with the same stamp
    again = torch.from_numpy(planes_np).to(DEV).requires_grad_(True)
    want = plain.expected(again)
    (want.double() * torch.from_numpy(cot).to(DEV)).sum().backward()
    assert torch.equal(out.detach().view(torch.int32), want.detach().view(torch.int32))
    assert torch.equal(planes.grad.view(torch.int32), again.grad.view(torch.int32))
    for p in model.parameters():
        p.requires_grad_(False)
    assert torch.equal(fitted.expected(planes.detach()).view(torch.int32), want.detach().view(torch.int32))
    frozen_planes = torch.from_numpy(planes_np).to(DEV).requires_grad_(True)          # only the planes need a gradient now
    (fitted.expected(frozen_planes).double() * torch.from_numpy(cot).to(DEV)).sum().backward()
    assert torch.equal(frozen_planes.grad.view(torch.int32), again.grad.view(torch.int32))


@pytest.mark.parametrize('kind', list(_models()))
def test_expected_windows_gradients(kind):
    """``expected_windows`` on 3 x 2 windows of a 4 x 4 patch at bin 2: the tap gradient takes the [n, C] layout as it is
    (``n_kernels = C``); the cropped rows and columns take no gradient, so the restatement sees a cotangent that is zero there."""
    from sunerf_hip.instrument import Instrument
    from sunerf_hip.psf_fit import FittedInstrument
    b, patch = 2, 4
    model = _models()[kind]().double().to(DEV)
    fitted = FittedInstrument(model, bin=b)
    plain = Instrument(psf=fitted.psf, bin=b)
    hw, ww = fitted.window_shape(patch)
    assert (hw, ww) == plain.window_shape(patch)
    rng = np.random.default_rng(17)
    windows_np = rng.standard_normal((3, 2, hw, ww)).astype(np.float32)
    cot = rng.standard_normal((3, 2, patch, patch))
    windows = torch.from_numpy(windows_np).to(DEV).requires_grad_(True)
    out = fitted.expected_windows(windows)
    assert out.shape == (3, 2, patch, patch)
    (out.double() * torch.from_numpy(cot).to(DEV)).sum().backward()
    K, _ = plain.effective_kernel()
    g_full = np.zeros((6, hw // b, ww // b), dtype=np.float32)
    g_full[:, :patch, :patch] = cot.astype(np.float32).reshape(6, patch, patch)
    call = (model.n, K.shape[1], K.shape[2], b, 0, 0, plain.scale, ZERO)
    planes_np = windows_np.reshape(6, hw, ww)
    reference = _chain_reference(model, pr.tap_gradient(planes_np, g_full, *call), pr.tap_gradient_bound(planes_np, g_full, *call), b)
    _check_parameters(f'{kind} windows', model, reference)
    again = torch.from_numpy(windows_np).to(DEV).requires_grad_(True)
    want = plain.expected_windows(again)
    (want.double() * torch.from_numpy(cot).to(DEV)).sum().backward()
    assert torch.equal(out.detach().view(torch.int32), want.detach().view(torch.int32))
    assert torch.equal(windows.grad.view(torch.int32), again.grad.view(torch.int32))
    for p in model.parameters():
        p.requires_grad_(False)
    assert torch.equal(fitted.expected_windows(windows.detach()).view(torch.int32), want.detach().view(torch.int32))


def test_fitted_instrument_never_serves_stale_taps():
    """The PSF moves between two calls on one stream: the second call sees the new stamp (the per-stream tap cache of
    ``Instrument`` would not), for ``expected`` and for ``deconvolve``'s taps alike."""
    from sunerf_hip.instrument import Instrument
    from sunerf_hip.psf_fit import FittedInstrument, TrainablePSF
    model = TrainablePSF.gaussian(2.0, 4).to(DEV)
    fitted = FittedInstrument(model, bin=2)
    planes = torch.rand(1, 20, 20, device=DEV)
    first = fitted.expected(planes)
    with torch.no_grad():
        model.log_fwhm.add_(0.3)
    second = fitted.expected(planes)
    assert not torch.equal(first, second)
    assert torch.equal(second, Instrument(psf=fitted.psf, bin=2).expected(planes))
    assert torch.equal(fitted.freeze().expected(planes), second)
    K, _ = fitted.effective_kernel()
    assert torch.equal(fitted._taps(K, planes.device).cpu(), torch.from_numpy(K))


def test_fit_psf_recovers_the_hidden_fwhm():
    """The host test's problem on the device: observed through ``Instrument(gaussian_psf(3.0, 6), bin=2).expected``, Adam from 2.0
    at lr = 0.05 for 200 steps.  Gate: within 1e-3 relative of 3.0 -- the restatement reaches 3e-6 and the device differs from it
    by the one fp32 rounding of ``expected`` (and the float32 parameter); a fit that does not work stays near 2.0, 0.33 off."""
    from sunerf_hip.instrument import Instrument, gaussian_psf
    from sunerf_hip.psf_fit import FittedInstrument, TrainablePSF, fit_psf
    f = pr.FIT
    scene = torch.from_numpy(pr.fit_scene()).to(DEV)
    observed = Instrument(psf=gaussian_psf(f['hidden'], f['radius']), bin=f['bin'], boundary='nearest').expected(scene)
    fitted = FittedInstrument(TrainablePSF.gaussian(f['start'], f['radius']).to(DEV), bin=f['bin'], boundary='nearest')
    result = fit_psf(fitted, scene, observed, steps=f['steps'], lr=f['lr'])
    fwhm = float(result['fwhm'][0])
    loss = result['loss']
    print(f'fit_psf on the device: FWHM {fwhm:.9f} (hidden {f["hidden"]}), relative error {abs(fwhm - f["hidden"]) / f["hidden"]:.3e}; '
          f'loss {float(loss[0]):.3e} -> {float(loss[-1]):.3e}')
    assert loss.shape == (f['steps'],) and result['stamp'].shape == (13, 13)
    assert abs(fwhm - f['hidden']) <= 1e-3 * f['hidden']
    weighted = FittedInstrument(TrainablePSF.gaussian(f['start'], f['radius']).to(DEV), bin=f['bin'], boundary='nearest')
    chi = fit_psf(weighted, scene, observed, steps=3, lr=f['lr'], sigma=0.5)
    np.testing.assert_allclose(float(chi['loss'][0]), 4.0 * float(loss[0]), rtol=1e-12)          # residual / sigma, squared


def test_module_step_moves_the_psf():
    """One patch batch of 2 patches of 4 x 4 through a FittedInstrument: the training step leaves a finite, non-zero gradient on
    ``log_fwhm``, and ``ClipAdam.step`` moves the parameter."""
    from sunerf.model.sunerf import EmissionSuNeRFModule
    from sunerf_hip.psf_fit import FittedInstrument, TrainablePSF
    from test_gpu_patch import _observations
    torch.manual_seed(0)
    psf = TrainablePSF.gaussian(1.6, 2)
    mod = EmissionSuNeRFModule(Rs_per_ds=1.0, seconds_per_dt=1.0, image_scaling_config={'vmax': 1, 'a': 0.005},
                               sampling_config={'type': 'stratified', 'n_samples': 8, 'perturb': False},
                               hierarchical_sampling_config={'type': 'hierarchical', 'n_samples': 8},
                               model_config={'d_filter': 64}, psf_models=psf).cuda()
    inst = FittedInstrument(psf, bin=2)
    tracing = _observations(1).patch_pool(inst, patch=4).batch([0, 13])
    (optimiser,), _ = mod.configure_optimizers()
    assert any(p is psf.log_fwhm for p in optimiser._params)
    before = psf.log_fwhm.detach().clone()
    loss = mod.training_step({'tracing': tracing}, 0)
    loss.backward()
    grad = psf.log_fwhm.grad.detach().clone()
    print(f'module step: loss {loss.item():.6g}, d loss / d log_fwhm {grad.item():.6e}')
    assert bool(torch.isfinite(grad).all()) and float(grad.abs().max()) > 0
    optimiser.step()
    torch.cuda.synchronize()
    assert bool(torch.isfinite(psf.log_fwhm).all()) and not torch.equal(psf.log_fwhm.detach(), before)
