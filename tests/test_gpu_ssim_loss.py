"""The structural loss on the device (include/sunerf_hip_ssim_loss.h) against the fp64 restatement
tests/ssim_loss_reference.py: every output of the kernel at the seams of its launch (one window, one more pixel than a window,
patches whose planes are kept in LDS for all channels at once, for a group of channels, and patches so large that a workgroup
takes one channel; 1, 3 and 65 patches; 1, 3 and 7 channels; with and without the asinh stretch), identical images, invalid
planes, determinism, the autograd node, and one patch ``training_step`` of each Lightning module.

Counts.  A plane is one channel of one patch of ONE of the two images together with the target's: stats[2] and stats[3] count
valid and invalid planes over the 2 n C planes of both images.  A channel whose fine values hold a NaN while its coarse and
target values are finite is one valid (coarse) and one invalid (fine) plane; a non-finite target makes two invalid planes.

Bounds.  The kernel's arithmetic is fp64; an SSIM lies within 1e-12 of the restatement (the two order their sums differently:
a few ulp of a sum of at most 121 terms, divided by B2 >= 9e-4).  A gradient is rounded to fp32 once (twice behind the autograd
node): |g - ref| <= 2^-23 |ref| + 1e-12 max|ref|, the second term for elements in which the three box sums cancel."""
import functools

import numpy as np
import pytest
import torch

import ssim_loss_reference as sr

pytestmark = pytest.mark.gpu

DEV = 'cuda'
ASINH = (1.0, 0.005)
# (7, 48) is added to the issue's list: at 7 channels its planes no longer fit LDS together and a workgroup takes a group of two
WINDOWS = [(3, 3), (7, 7), (7, 8), (7, 16), (7, 33), (7, 48), (11, 64)]
CASES = [(n, C, w, P) for n in (1, 3, 65) for C in (1, 3, 7) for w, P in WINDOWS if (P != 48 or (C == 7 and n == 3))]


def _bits(t):
    return t.detach().contiguous().cpu().numpy().reshape(-1).view(np.uint8)


@functools.lru_cache(maxsize=None)
def _case(n, P, C, seed=0):
    return sr.make_case(n, P, C, seed)


@functools.lru_cache(maxsize=4)
def _reference(n, P, C, w, stretched, seed=0):
    return sr.evaluate(*_case(n, P, C, seed), n, P, w, 1.0, ASINH if stretched else None)


def _device(arrays):
    return [torch.from_numpy(np.ascontiguousarray(v)).to(DEV) for v in arrays]


def _launch(tensors, n, P, w, scaling, data_range=1.0):
    from sunerf_hip.ssim_loss import launch
    out = launch(*tensors, n, P, data_range, w, scaling)
    torch.cuda.synchronize()
    return dict(zip(('g_coarse', 'g_fine', 'plane_ssim', 'stats'), out))


def _check_gradient(got, ref, what, scale=1.0):
    got, ref = np.asarray(got, dtype=np.float64), np.asarray(ref, dtype=np.float64) * scale
    bound = 2.0 ** -23 * np.abs(ref) + 1e-12 * np.abs(ref).max()
    err = np.abs(got - ref)
    worst = float((err[bound > 0] / bound[bound > 0]).max()) if (bound > 0).any() else 0.0
    print(f'{what}: largest error {worst:.3g} of its bound')
    assert np.isfinite(got).all() and np.array_equal(got[bound == 0], ref[bound == 0]) and worst <= 1.0, (what, worst)
    return worst


def _compare(got, ref, tag):
    ps = got['plane_ssim'].cpu().numpy()
    assert np.array_equal(np.isnan(ps), np.isnan(ref['plane_ssim'])), tag
    keep = ~np.isnan(ps)
    err = float(np.abs(ps[keep] - ref['plane_ssim'][keep]).max()) if keep.any() else 0.0
    print(f'{tag} plane_ssim: largest error {err:.3g} (bound 1e-12)')
    assert err <= 1e-12, (tag, err)
    worst = max(_check_gradient(got[k].cpu().numpy(), ref[k], f'{tag} {k}') for k in ('g_coarse', 'g_fine'))
    stats = got['stats'].cpu().numpy()
    assert np.abs(stats[:2] - ref['stats'][:2]).max() <= 1e-12, (tag, stats, ref['stats'])
    assert np.array_equal(stats[2:], ref['stats'][2:]), (tag, stats, ref['stats'])
    return worst


# ---- 1. parity at the seams -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('n,C,w,P', CASES, ids=[f'{n}x{P}x{C}-w{w}' for n, C, w, P in CASES])
def test_every_output_equals_the_restatement(n, C, w, P):
    from sunerf_hip.metrics import image_metrics
    tensors = _device(_case(n, P, C))
    for stretched in (False, True):
        ref = _reference(n, P, C, w, stretched)
        got = _launch(tensors, n, P, w, ASINH if stretched else None)
        worst = _compare(got, ref, f'{n} x {P}^2 x {C} w {w}{" asinh" if stretched else ""}')
        print(f'gradient error as a fraction of its bound: {worst:.3g}')
        assert ref['stats'][3] == 0 and 0.0 < ref['stats'][0] < 1.0
    if w == 7:          # the existing score kernel takes fp32 images: the unstretched planes, permuted to [n, C, P, P]
        planes = [t.reshape(n, P, P, C).permute(0, 3, 1, 2).contiguous() for t in tensors]
        plain = _launch(tensors, n, P, w, None)['plane_ssim']
        for k in range(2):
            score = image_metrics(planes[k], planes[2], 1.0)['ssim']
            err = float((plain[k] - score).abs().max())
            print(f'plane_ssim[{k}] against sunerf_image_metrics: largest difference {err:.3g} (bound 1e-10)')
            assert err <= 1e-10


def test_patch_ssim_is_the_coarse_row_of_the_loss():
    from sunerf_hip.ssim_loss import patch_ssim
    n, P, C = 3, 16, 3
    tensors = _device(_case(n, P, C))
    ref = _reference(n, P, C, 7, True)
    got = patch_ssim(tensors[1], tensors[2], n, P, 1.0, asinh_scaling=ASINH)
    assert got.shape == (n, C) and got.dtype == torch.float64 and not got.requires_grad
    assert float(np.abs(got.cpu().numpy() - ref['plane_ssim'][1]).max()) <= 1e-12


# ---- 2. identical images, invalid planes ------------------------------------------------------------------------------------------
@pytest.mark.parametrize('w,P', [(3, 3), (7, 16), (7, 48), (11, 64)])
@pytest.mark.parametrize('stretched', [False, True], ids=['plain', 'asinh'])
def test_identical_images_score_one_exactly(w, P, stretched):
    n, C = 3, 7
    target = _device(_case(n, P, C))[2]
    got = _launch([target, target.clone(), target], n, P, w, ASINH if stretched else None)
    assert bool((got['plane_ssim'] == 1.0).all()) and got['stats'].tolist() == [0.0, 0.0, 2.0 * n * C, 0.0]
    worst = max(float(got[k].abs().max()) for k in ('g_coarse', 'g_fine'))
    print(f'identical images, {P}^2 w {w}: largest |g| {worst:.3g} (bound 1e-10)')
    assert worst <= 1e-10


@pytest.mark.parametrize('w,P', [(7, 8), (7, 48), (11, 64)])
def test_invalid_planes_are_left_out_and_counted(w, P):
    n, C = 4, 3
    coarse, fine, target = (v.copy().reshape(n, P, P, C) for v in _case(n, P, C, 1))
    ways = []
    for index in range(0, n * C, 4):          # one channel plane in four, in three ways in turn
        k, c = divmod(index, C)
        way = (index // 4) % 3
        ways.append((k, c, way))
        if way == 0:
            coarse[k, P - 1, 0, c] = np.nan
        elif way == 1:
            target[k, 0, P - 1, c] = np.inf
        else:
            fine[k, P // 2, P // 2, c] = np.nan
    assert {way for _, _, way in ways} == {0, 1, 2}
    arrays = [v.reshape(n * P * P, C) for v in (coarse, fine, target)]
    ref = sr.evaluate(*arrays, n, P, w, 1.0, ASINH)
    got = _launch(_device(arrays), n, P, w, ASINH)
    _compare(got, ref, f'invalid planes {P}^2 w {w}')
    g = [got[k].cpu().numpy().reshape(n, P, P, C) for k in ('g_coarse', 'g_fine')]
    ps = got['plane_ssim'].cpu().numpy()
    assert np.isfinite(g[0]).all() and np.isfinite(g[1]).all()
    invalid = 0
    for k, c, way in ways:
        bad = {0: (True, False), 1: (True, True), 2: (False, True)}[way]
        for image in range(2):
            assert bool(np.isnan(ps[image, k, c])) == bad[image], (k, c, way, image)
            assert bool(g[image][k, :, :, c].any()) != bad[image], (k, c, way, image)          # exactly 0 where invalid, alive elsewhere
            invalid += bad[image]
    stats = got['stats'].cpu().numpy()
    assert stats[3] == invalid == int(np.isnan(ps).sum()) and stats[2] == 2 * n * C - invalid
    # no valid plane at all: the term and every gradient are 0
    arrays[2][:] = np.nan
    none = _launch(_device(arrays), n, P, w, ASINH)
    assert none['stats'].tolist() == [0.0, 0.0, 0.0, 2.0 * n * C]
    assert not bool(none['g_coarse'].any()) and not bool(none['g_fine'].any()) and bool(torch.isnan(none['plane_ssim']).all())


# ---- 3. determinism ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('w,P', [(7, 16), (7, 48), (11, 64)])
def test_reruns_streams_and_a_plane_alone_give_the_same_bits(w, P):
    from sunerf_hip.ssim_loss import _workspace
    n, C = 5, 7
    arrays = _case(n, P, C, 2)
    tensors = _device(arrays)
    first = _launch(tensors, n, P, w, ASINH)
    again = _launch(tensors, n, P, w, ASINH)
    for k in first:
        assert np.array_equal(_bits(first[k]), _bits(again[k])), k
    streams = [torch.cuda.Stream(), torch.cuda.Stream()]
    torch.cuda.synchronize()
    results = []
    for s in streams:
        with torch.cuda.stream(s):
            ws = _workspace(torch.device(DEV, torch.cuda.current_device()), n, C)
            results.append((ws.data_ptr(), _launch(tensors, n, P, w, ASINH)))
    assert results[0][0] != results[1][0]          # a workspace per stream
    for _, got in results:
        for k in first:
            assert np.array_equal(_bits(first[k]), _bits(got[k])), k
    # a plane alone: patch 3, channel 5 as a batch of one patch with one channel
    k, c = 3, 5
    alone = _device([v.reshape(n, P * P, C)[k, :, c:c + 1] for v in arrays])
    single = _launch(alone, 1, P, w, ASINH)
    assert np.array_equal(_bits(single['plane_ssim']), _bits(first['plane_ssim'][:, k, c]))
    for name in ('g_coarse', 'g_fine'):
        assert np.array_equal(_bits(single[name]), _bits(first[name].reshape(n, P * P, C)[k, :, c]))


# ---- 4. autograd ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('stretched', [False, True], ids=['plain', 'asinh'])
def test_backward_gives_the_restatements_gradients_and_a_descent_direction(stretched):
    from sunerf_hip.ssim_loss import ssim_loss
    n, P, C, w = 3, 16, 3, 7
    scaling = ASINH if stretched else None
    arrays = [v.copy() for v in _case(n, P, C, 3)]
    arrays[1].reshape(n, P, P, C)[2, 1, 1, 0] = np.nan          # a fine plane drops out: the two images have different counts
    ref = sr.evaluate(*arrays, n, P, w, 1.0, scaling)
    assert ref['counts'].tolist() == [n * C, n * C - 1]
    coarse, fine, target = _device(arrays)
    coarse.requires_grad_(True)
    fine.requires_grad_(True)
    loss, stats, plane_ssim = ssim_loss(coarse, fine, target, n, P, 1.0, window=w, asinh_scaling=scaling)
    assert loss.dim() == 0 and loss.dtype == torch.float64 and not stats.requires_grad and not plane_ssim.requires_grad
    assert abs(loss.item() - ref['loss']) <= 1e-12
    (2.5 * loss).backward()
    _check_gradient(coarse.grad.cpu().numpy(), ref['d_coarse'], 'coarse.grad', scale=2.5)
    _check_gradient(fine.grad.cpu().numpy(), ref['d_fine'], 'fine.grad', scale=2.5)
    assert not bool(fine.grad.reshape(n, P, P, C)[2, :, :, 0].any())
    with torch.no_grad():
        g = coarse.grad
        moved, _, _ = ssim_loss(coarse - 1e-3 * g / g.abs().max(), fine, target, n, P, 1.0, window=w, asinh_scaling=scaling)
    print(f'loss {loss.item():.12f}, after a step of 1e-3 down the gradient {moved.item():.12f}')
    assert moved.item() < loss.item()
    with pytest.raises(ValueError):
        ssim_loss(coarse, fine, target, n, P, 1.0, window=4)
    with pytest.raises(ValueError):
        ssim_loss(coarse, fine, target, n, 6, 1.0)
    with pytest.raises(Exception):
        ssim_loss(coarse.cpu(), fine.cpu(), target.cpu(), n, P, 1.0)          # no CPU path


# ---- 5. the Lightning modules -----------------------------------------------------------------------------------------------------
def torch_dssim(pred, target, n, P, w, data_range, scaling=None):
    """``dssim`` of images [n P P, C] as a composition of torch operations in fp64 (``avg_pool2d``), with autograd."""
    def planes(v):
        v = v.double()
        if scaling is not None:
            v = torch.asinh(v / scaling[0] / scaling[1]) / float(np.arcsinh(1.0 / scaling[1]))
        return v.reshape(n, P, P, -1).permute(0, 3, 1, 2)
    pool = lambda v: torch.nn.functional.avg_pool2d(v, w, stride=1)          # noqa: E731
    x, y = planes(pred), planes(target)
    norm = w * w / (w * w - 1.0)
    mu_x, mu_y = pool(x), pool(y)
    var_x, var_y, cov = norm * (pool(x * x) - mu_x * mu_x), norm * (pool(y * y) - mu_y * mu_y), norm * (pool(x * y) - mu_x * mu_y)
    c1, c2 = (0.01 * data_range) ** 2, (0.03 * data_range) ** 2
    s = (2 * mu_x * mu_y + c1) * (2 * cov + c2) / ((mu_x * mu_x + mu_y * mu_y + c1) * (var_x + var_y + c2))
    return 1.0 - s.mean(dim=(2, 3)).mean()


def _emission(**kwargs):
    from sunerf.model.sunerf import EmissionSuNeRFModule
    torch.manual_seed(0)
    return EmissionSuNeRFModule(Rs_per_ds=1.0, seconds_per_dt=1.0, image_scaling_config={'vmax': 1, 'a': 0.005},
                                sampling_config={'type': 'stratified', 'n_samples': 8, 'perturb': False},
                                hierarchical_sampling_config={'type': 'hierarchical', 'n_samples': 8},
                                model_config={'d_filter': 64}, **kwargs).cuda()


def _emission_batch():
    from sunerf_hip.instrument import Instrument
    from test_gpu_patch import _observations
    inst = Instrument(psf=np.random.default_rng(21).uniform(0.1, 1.0, size=(3, 5)), bin=2)
    return _observations(1).patch_pool(inst, patch=4).batch([0, 4, 13])


def _by_hand(mod, tracing, pixel_loss, data_range, scaling, wavelength=False):
    """The step's chain composed by hand on the step's own images: the pixel loss the module would take, plus lambda_ssim times
    the torch composition of D-SSIM, both on ``_observed_windows`` of a second (bit-identical) pass through the render."""
    from sunerf.model.sunerf import _observed_windows
    rays = tracing['rays'].reshape(-1, 2, 3)
    args = (rays[:, 0].contiguous(), rays[:, 1].contiguous(), tracing['time']) + ((tracing['wavelength'],) if wavelength else ())
    out = mod.rendering(*args)
    coarse, fine, target = _observed_windows(tracing, out)
    spec = tracing['patch']
    term = sum(torch_dssim(v, target, spec['n'], spec['P'], mod.ssim_window, data_range, scaling) for v in (coarse, fine))
    return pixel_loss(coarse, fine, target, out), term


def _check_step(mod, tracing, pixel_loss, data_range, scaling, tag, wavelength=False):
    from test_gpu_patch import _compare_gradients, _gradients_of
    loss = mod.training_step({'tracing': tracing}, 0)
    stats = mod.last_ssim
    got = _gradients_of(mod, loss)          # (before the second forward: one pass through the render at a time)
    pixel, term = _by_hand(mod, tracing, pixel_loss, data_range, scaling, wavelength)
    want = pixel.double() + mod.lambda_ssim * term
    rel = abs(loss.item() - want.item()) / abs(want.item())
    print(f'{tag}: loss {loss.item():.9g}, by hand {want.item():.9g} (relative difference {rel:.2e}, bound 1e-6); '
          f'structural term {term.item():.6f} of it')
    assert rel <= 1e-6 and term.item() > 1e-3
    assert stats is not None and abs(float(stats[0] + stats[1]) - term.item()) <= 1e-9
    logged = getattr(mod, 'logged', None)          # (the stand-in base of sunerf/model/sunerf.py keeps what was logged)
    if logged is not None:
        assert set(logged['train_ssim']) == {'coarse', 'fine'} and set(logged['train']) == {'coarse', 'fine', 'regularization', 'psnr'}
    _compare_gradients(mod, got, want)


def test_emission_patch_step_with_the_structural_term():
    from sunerf.model.sunerf import _other_outputs
    from sunerf_hip.train import training_loss
    tracing = _emission_batch()
    mod = _emission(lambda_ssim=0.5, ssim_window=3)
    scaling = mod._asinh_constants()

    def mse(coarse, fine, target, out):
        return training_loss(coarse, fine, target, out['regularization'], mod.lambda_image, mod.lambda_regularization,
                             asinh_scaling=scaling, finite_check=_other_outputs(out))[0]
    _check_step(mod, tracing, mse, 1.0, scaling, 'emission, asinh MSE')


def test_emission_patch_step_with_a_frozen_gain_likelihood_and_the_structural_term():
    from sunerf.model.sunerf import _other_outputs
    from sunerf_hip.instrument import Instrument
    from sunerf_hip.likelihood import NoiseLikelihood, likelihood_loss
    tracing = _emission_batch()
    like = NoiseLikelihood(Instrument(unit=30.0, read_noise=1.0))
    mod = _emission(lambda_ssim=0.5, ssim_window=3, likelihood=like)

    def nll(coarse, fine, target, out):
        return likelihood_loss(coarse, fine, target, out['regularization'], like, lambda_image=mod.lambda_image,
                               lambda_regularization=mod.lambda_regularization, finite_check=_other_outputs(out))[0]
    _check_step(mod, tracing, nll, 1.0, mod._asinh_constants(), 'emission, likelihood')
    assert mod.last_channel_stats is not None


def _dt_module(**kwargs):
    from conftest import load_golden
    from sunerf.model.model import NeRF_DT
    from sunerf.model.sunerf import DensityTemperatureSuNeRFModule
    g = load_golden('g6_dt_e2e')
    mod = DensityTemperatureSuNeRFModule(
        Rs_per_ds=1.0, seconds_per_dt=1.0, image_scaling_config={}, model=NeRF_DT,
        sampling_config={'type': 'stratified', 'n_samples': 16, 'perturb': False},
        hierarchical_sampling_config={'type': 'hierarchical', 'n_samples': 16}, model_config={'d_filter': 64},
        pixel_intensity_factor=float(g['pixel_intensity_factor']),
        response_table=(g['aia_logte'].numpy(), g['aia_tresp'].numpy()), **kwargs)
    mod.rendering.load_state_dict({k[4:].replace('__', '.'): v for k, v in g.items() if k.startswith('sd__')}, strict=True)
    return mod.cuda()


def _dt_batch(mod):
    from sunerf_hip.instrument import Instrument
    from test_gpu_patch import _observations
    inst = Instrument(psf=np.random.default_rng(22).uniform(0.1, 1.0, size=(2, 3, 3)), bin=2)
    tracing = _observations(2, full=True).patch_pool(inst, patch=4).batch([2, 4, 13])
    with torch.no_grad():          # targets of the size of the render, so that neither term of (render - target) is lost
        rays = tracing['rays'].reshape(-1, 2, 3)
        scale = mod.rendering(rays[:, 0].contiguous(), rays[:, 1].contiguous(), tracing['time'], tracing['wavelength'])['fine_image'].mean().item()
    tracing['target_image'] = tracing['target_image'] * scale
    return tracing, scale


def test_density_temperature_patch_step_with_the_structural_term():
    from sunerf.model.sunerf import _other_outputs
    from sunerf_hip.train import training_loss
    tracing, scale = _dt_batch(_dt_module())
    mod = _dt_module(lambda_ssim=0.5, ssim_window=3, ssim_data_range=scale)          # the targets lie in (0.05, 1) x scale

    def mse(coarse, fine, target, out):
        return training_loss(coarse, fine, target, out['regularization'], mod.lambda_image, mod.lambda_regularization,
                             asinh_scaling=None, finite_check=_other_outputs(out))[0]
    _check_step(mod, tracing, mse, scale, None, 'density-temperature, MSE', wavelength=True)


def test_density_temperature_patch_step_with_a_frozen_gain_likelihood_and_the_structural_term():
    from sunerf.model.sunerf import _other_outputs, _patch_codes
    from sunerf_hip.likelihood import NoiseLikelihood, likelihood_loss
    tracing, scale = _dt_batch(_dt_module())
    inst = tracing['patch']['instrument']
    like = NoiseLikelihood(inst, codes=(171, 193), mode='observed', floor=0.05 * scale)          # (this instrument has no read noise)
    mod = _dt_module(lambda_ssim=0.5, ssim_window=3, ssim_data_range=scale, likelihood=like)
    codes = _patch_codes(tracing)

    def chi2(coarse, fine, target, out):
        return likelihood_loss(coarse, fine, target, out['regularization'], like, codes=codes, lambda_image=mod.lambda_image,
                               lambda_regularization=mod.lambda_regularization, finite_check=_other_outputs(out))[0]
    _check_step(mod, tracing, chi2, scale, None, 'density-temperature, likelihood', wavelength=True)
    assert mod.last_channel_stats is not None and not any(p.requires_grad for p in like.parameters())


def test_the_term_switched_off_and_ray_batches_keep_the_old_loss_bits():
    from conftest import load_golden
    from sunerf.model.sunerf import _observed_windows, _other_outputs
    from sunerf_hip.train import training_loss
    # lambda_ssim = 0 on a patch batch
    tracing = _emission_batch()
    for kwargs in ({}, {'lambda_ssim': 0.0, 'ssim_window': 3}):
        mod = _emission(**kwargs)
        loss = mod.training_step({'tracing': tracing}, 0)
        rays = tracing['rays'].reshape(-1, 2, 3)
        out = mod.rendering(rays[:, 0].contiguous(), rays[:, 1].contiguous(), tracing['time'])
        coarse, fine, target = _observed_windows(tracing, out)
        want, _ = training_loss(coarse, fine, target, out['regularization'], mod.lambda_image, mod.lambda_regularization,
                                asinh_scaling=mod._asinh_constants(), finite_check=_other_outputs(out))
        assert np.array_equal(_bits(loss), _bits(want)) and loss.dtype == torch.float32
        assert mod.last_ssim is None and 'train_ssim' not in getattr(mod, 'logged', {})
    # lambda_ssim > 0 on a ray batch
    g = load_golden('g5_emission_e2e')
    mod = _emission(lambda_ssim=0.5)
    rays = torch.stack([g['rays_o'], g['rays_d']], 1)[:64].cuda()
    tracing = {'rays': rays, 'time': g['times'][:64].cuda(), 'target_image': g['target'][:64].cuda()}
    loss = mod.training_step({'tracing': tracing}, 0)
    out = mod.rendering(rays[:, 0].contiguous(), rays[:, 1].contiguous(), tracing['time'])
    want, _ = training_loss(out['coarse_image'], out['fine_image'], tracing['target_image'].reshape(-1, 1), out['regularization'],
                            mod.lambda_image, mod.lambda_regularization, asinh_scaling=mod._asinh_constants(),
                            finite_check=_other_outputs(out))
    assert np.array_equal(_bits(loss), _bits(want)) and mod.last_ssim is None and 'train_ssim' not in getattr(mod, 'logged', {})
