"""The noise-weighted likelihood on the device (include/sunerf_hip_likelihood.h) against the fp64 restatement
tests/likelihood_reference.py: every output of the kernel at the seams of its launch (one slot, one wave less / exactly / more
than one, several workgroups, more slots than the launch has threads; 1, 7 and 64 table rows; both modes; with and without
codes), the masked and empty cases, determinism, the autograd node, a gain fitted without a network, and one ``training_step`` of
each Lightning module on rays and on patches.

Bounds.  The kernel's arithmetic is fp64 and every fp32 output is rounded once, so an fp32 output lies within 2^-23 |ref| (+ 1e-30
for fp32's subnormals) of the restatement; sums taken in another order than numpy's differ by at most a few 2^-53 of the sum of
their terms' magnitudes per addition, which 1e-12 of that sum covers at these sizes (at most 32900 terms); counts are exact.  A
gradient that leaves the autograd node has been rounded twice (the kernel's store, the node's product): 2 (2^-24 / (1 + 2^-24))
+ 2^-48 < 2^-23, the same bound."""
import numpy as np
import pytest
import torch

import likelihood_reference as lr
from conftest import load_golden

pytestmark = pytest.mark.gpu

DEV = 'cuda'
F32_REL, F32_ABS, F64_REL = 2.0 ** -23, 1e-30, 1e-12
SHAPES = [(n, w) for n in (1, 63, 64, 65, 257) for w in (1, 3, 7)] + [(4700, 7)]
ROWS = (1, 7, 64)
MODES = (('observed', lr.OBSERVED), ('model', lr.MODEL))


def _bits(t):
    return t.detach().contiguous().cpu().numpy().reshape(-1).view(np.uint8)


def _close32(got, ref, what, extra=0.0):
    got, ref = np.asarray(got, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    err = np.abs(got - ref)
    bound = F32_REL * np.abs(ref) + F32_ABS + extra
    worst = float((err / bound).max()) if err.size else 0.0
    print(f'{what}: largest error {worst:.3g} of its bound')
    assert np.isfinite(got).all() and worst <= 1.0, (what, worst)


def _close64(got, ref, magnitude, what):
    got, ref = np.asarray(got, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    err = np.abs(got - ref)
    bound = F64_REL * np.asarray(magnitude, dtype=np.float64)
    assert np.array_equal(err[bound == 0], np.zeros(int((bound == 0).sum()))), what
    worst = float((err[bound > 0] / bound[bound > 0]).max()) if (bound > 0).any() else 0.0
    print(f'{what}: largest error {worst:.3g} of its bound')
    assert np.isfinite(got).all() and worst <= 1.0, (what, worst)


def _device(case):
    return {k: (None if v is None else torch.from_numpy(np.ascontiguousarray(v)).to(DEV)) for k, v in case.items()}


def _launch(d, mode, lam=0.75, lam_r=0.5, with_codes=True, extras=()):
    from sunerf_hip.likelihood import launch
    out = launch(d['coarse'], d['fine'], d['target'], d['codes'] if with_codes else None, d['row_codes'], d['noise'], d['log_gain'], mode,
                 d['reg'], list(extras), lam, lam_r)
    torch.cuda.synchronize()
    return dict(zip(('g_coarse', 'g_fine', 'g_log_gain', 'channel_stats', 'stats'), out))


def _compare(got, ref, tag):
    for k in ('g_coarse', 'g_fine'):
        _close32(got[k].cpu().numpy(), ref[k], f'{tag} {k}')
    _close32(got['stats'][:5].cpu().numpy(), ref['stats'][:5], f'{tag} stats[0:5]')
    assert np.array_equal(got['stats'][5:].cpu().numpy().astype(np.float64), ref['stats'][5:]), (tag, got['stats'], ref['stats'])
    cs = got['channel_stats'].cpu().numpy()
    assert np.array_equal(cs[:, 0], ref['channel_stats'][:, 0]), f'{tag}: valid counts per row'
    _close64(cs[:, 1:], ref['channel_stats'][:, 1:], ref['magnitude'][:, 1:4], f'{tag} channel_stats')
    _close64(got['g_log_gain'].cpu().numpy(), ref['g_log_gain'], ref['magnitude'][:, 4], f'{tag} g_log_gain')


# ---- 1. parity at the seams -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('m', ROWS)
@pytest.mark.parametrize('n,w', SHAPES, ids=[f'{n}x{w}' for n, w in SHAPES])
def test_every_output_equals_the_restatement(n, w, m):
    case = lr.make_case(n, w, m, 0)
    d = _device(case)
    variants = [True] + ([False] if m == 1 else [])
    for with_codes in variants:
        for name, mode in MODES:
            ref = lr.evaluate(case['coarse'], case['fine'], case['target'], case['codes'] if with_codes else None, case['row_codes'],
                              case['noise'], case['log_gain'], mode, case['reg'], 0.75, 0.5)
            got = _launch(d, mode, with_codes=with_codes)
            _compare(got, ref, f'{n}x{w} rows {m} {name}{"" if with_codes else " no codes"}')
            assert ref['stats'][6] >= n * w - (n * w) // 4          # masking cannot hide a failure
    if n * w > 128 * 256:
        assert n * w > 32768          # more slots than the launch has threads: the stride loop runs twice for some threads


def test_finite_check_tensors_and_non_finite_predictions_are_counted():
    case = lr.make_case(65, 3, 7, 1)
    case['coarse'][2, 1] = np.inf          # at a valid slot
    case['reg'][5] = np.nan
    valid = lr.evaluate(case['coarse'], case['fine'], case['target'], case['codes'], case['row_codes'], case['noise'], case['log_gain'],
                        lr.OBSERVED, case['reg'])['valid']
    assert valid[2, 1]
    extras = [torch.tensor([1.0, float('nan'), float('inf')], device=DEV), torch.zeros(300, device=DEV)]
    got = _launch(_device(case), lr.OBSERVED, extras=extras)
    assert float(got['stats'][5]) == 1 + 1 + 2


# ---- 2. masked, deterministic -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name,mode', MODES)
def test_all_slots_masked_gives_zeros_and_no_nan(name, mode):
    case = lr.make_case(65, 3, 7, 2)
    case['codes'][:] = 0.0
    case['codes'][::2] = 2500.0
    got = _launch(_device(case), mode, lam_r=0.25)
    want = 0.25 * case['reg'].astype(np.float64).mean()
    for k in ('g_coarse', 'g_fine', 'g_log_gain', 'channel_stats'):
        assert not bool(got[k].any()) and bool(torch.isfinite(got[k]).all()), k
    stats = got['stats'].cpu().numpy()
    assert np.isfinite(stats).all()
    _close32(stats[0], want, f'{name} loss of the regularization alone')
    _close32(stats[3], want / 0.25, f'{name} regularization mean')
    assert stats[1] == 0 and stats[2] == 0 and stats[4] == 0 and stats[6] == 0 and stats[7] == 33 * 3


def test_reruns_and_streams_with_their_own_workspaces_are_bit_identical():
    case = lr.make_case(4700, 7, 64, 3)
    d = _device(case)
    first = _launch(d, lr.MODEL)
    again = _launch(d, lr.MODEL)
    for k in first:
        assert np.array_equal(_bits(first[k]), _bits(again[k])), k
    streams = [torch.cuda.Stream(), torch.cuda.Stream()]
    torch.cuda.synchronize()
    results = []
    for s in streams:
        with torch.cuda.stream(s):
            from sunerf_hip.likelihood import _workspace
            ws = _workspace(torch.device(DEV, torch.cuda.current_device()), 64)
            results.append((ws.data_ptr(), _launch(d, lr.MODEL)))
    assert results[0][0] != results[1][0]          # a workspace per stream
    for _, got in results:
        for k in first:
            assert np.array_equal(_bits(first[k]), _bits(got[k])), k


# ---- 3. autograd ------------------------------------------------------------------------------------------------------------------
def _likelihood(case, mode, free, gain_rate=1.0):
    """A NoiseLikelihood holding the case's table: one Instrument per row, the case's floor shared."""
    from sunerf_hip.instrument import Instrument
    from sunerf_hip.likelihood import NoiseLikelihood
    codes = [int(c) for c in case['row_codes']]
    noise = case['noise'].copy()
    noise[:, 5] = noise[0, 5]
    insts = {c: Instrument(unit=noise[i, 0], exposure=noise[i, 1], dn_per_photon=noise[i, 2], read_noise=noise[i, 3],
                           quantise=bool(noise[i, 4] > 0)) for i, c in enumerate(codes)}
    like = NoiseLikelihood(insts, codes=codes, mode=mode, free=free, gain_rate=gain_rate, floor=float(noise[0, 5])).to(DEV)
    assert np.array_equal(like.noise.cpu().numpy(), noise)
    with torch.no_grad():
        like.log_gain.copy_(torch.from_numpy(case['log_gain'] / np.float32(gain_rate)))
    return like, noise


@pytest.mark.parametrize('name,mode', MODES)
def test_backward_gives_the_restatements_gradients(name, mode):
    from sunerf_hip.likelihood import likelihood_loss
    case = lr.make_case(257, 7, 7, 4)
    codes = [int(c) for c in case['row_codes']]
    free = codes[:3] + codes[5:]
    like, noise = _likelihood(case, name, free)
    d = _device(case)
    coarse, fine, reg = (d[k].clone().requires_grad_(True) for k in ('coarse', 'fine', 'reg'))
    loss, stats, channel_stats = likelihood_loss(coarse, fine, d['target'], reg, like, codes=d['codes'], lambda_image=0.75,
                                                 lambda_regularization=0.5)
    loss.backward()
    ref = lr.evaluate(case['coarse'], case['fine'], case['target'], case['codes'], case['row_codes'], noise,
                      like.effective_log_gain().cpu().numpy(), mode, case['reg'], 0.75, 0.5)
    _close32(loss.item(), ref['loss'], f'{name} loss')
    assert not stats.requires_grad and not channel_stats.requires_grad and loss.dim() == 0
    _close32(coarse.grad.cpu().numpy(), ref['d_coarse'], f'{name} coarse.grad')
    _close32(fine.grad.cpu().numpy(), ref['d_fine'], f'{name} fine.grad')
    _close32(reg.grad.cpu().numpy(), ref['d_reg'], f'{name} reg.grad')
    frozen = np.array([c not in free for c in codes])
    want = np.where(frozen, 0.0, ref['d_log_gain'])
    scale = 0.75 / ref['stats'][6]
    _close32(like.log_gain.grad.cpu().numpy(), want, f'{name} log_gain.grad', extra=F64_REL * scale * ref['magnitude'][:, 4])
    assert frozen.sum() == 2 and not bool(like.log_gain.grad[torch.from_numpy(frozen).to(DEV)].any())
    assert np.abs(ref['d_log_gain'][frozen]).min() > 0          # the restatement's own gradient of a frozen row is not 0

    # gain_rate: the same effective gains from a stored parameter 8 times smaller give 8 times the gradient, exactly (a power of two)
    fast, _ = _likelihood(case, name, free, gain_rate=8.0)
    assert np.array_equal(_bits(fast.effective_log_gain()), _bits(like.effective_log_gain()))
    loss8, _, _ = likelihood_loss(d['coarse'], d['fine'], d['target'], d['reg'], fast, codes=d['codes'], lambda_image=0.75,
                                  lambda_regularization=0.5)
    loss8.backward()
    assert np.array_equal(_bits(loss8), _bits(loss))
    assert np.array_equal(_bits(fast.log_gain.grad), _bits(like.log_gain.grad * 8.0))
    # a likelihood without a free gain takes no gradient at all
    none, _ = _likelihood(case, name, ())
    loss0, _, _ = likelihood_loss(coarse, fine, d['target'], reg, none, codes=d['codes'])
    loss0.backward()
    assert none.log_gain.grad is None and not none.log_gain.requires_grad


def test_a_free_gain_reaches_the_closed_form_optimum():
    """Fixed predictions, targets 1.3 times as bright plus noise, one free row, ClipAdam on log_gain alone: 'observed' mode is a
    weighted least-squares fit of the gain, whose optimum is sum(p t / s2) / sum(p^2 / s2)."""
    from sunerf_hip.instrument import Instrument
    from sunerf_hip.likelihood import NoiseLikelihood, likelihood_loss
    from sunerf_hip.train import ClipAdam
    rng = np.random.default_rng(12)
    inst = Instrument(unit=40.0, exposure=2.9, dn_per_photon=1.2, read_noise=1.5)
    like = NoiseLikelihood(inst, free='all', gain_rate=1.0).to(DEV)
    p = rng.uniform(0.05, 2.0, (64, 3)).astype(np.float32)
    sigma = like.sigma(torch.from_numpy(1.3 * p.astype(np.float64))).numpy()
    t = (1.3 * p + rng.normal(0.0, 1.0, p.shape) * sigma).astype(np.float32)
    s2 = like.sigma(torch.from_numpy(t)).numpy() ** 2          # the weights of 'observed' mode: from the targets
    p64, t64 = p.astype(np.float64), t.astype(np.float64)
    optimum = np.log((p64 * t64 / s2).sum() / (p64 * p64 / s2).sum())
    assert abs(optimum - np.log(1.3)) < 0.05
    pred, target = torch.from_numpy(p.reshape(-1, 1)).to(DEV), torch.from_numpy(t.reshape(-1, 1)).to(DEV)
    opt = ClipAdam(like.parameters(), lr=0.02)
    for step in range(400):
        opt.param_groups[0]['lr'] = 0.02 * 0.98 ** step
        opt.zero_grad()
        loss, stats, channel_stats = likelihood_loss(pred, pred, target, None, like)
        loss.backward()
        opt.step()
    got = float(like.log_gain.detach().cpu()[0])
    print(f'fitted log gain {got:.6f}, closed form {optimum:.6f}, difference {abs(got - optimum):.2e} (bound 1e-3); '
          f'reduced chi2 {float(like.reduced_chi2(channel_stats)[0]):.3f}')
    assert abs(got - optimum) <= 1e-3
    assert abs(float(like.gains()[0]) - np.exp(got)) < 1e-6


# ---- 4. the Lightning modules -------------------------------------------------------------------------------------------------------
def _emission_module(likelihood=None):
    from sunerf.model.sunerf import EmissionSuNeRFModule
    g = load_golden('g5_emission_e2e')
    mod = EmissionSuNeRFModule(Rs_per_ds=1.0, seconds_per_dt=1.0, image_scaling_config={'vmax': 1, 'a': 0.005},
                               sampling_config={'type': 'stratified', 'n_samples': 32, 'perturb': False},
                               hierarchical_sampling_config={'type': 'hierarchical', 'n_samples': 32}, model_config={'d_filter': 64},
                               likelihood=likelihood)
    mod.rendering.load_state_dict({k[4:].replace('__', '.'): v for k, v in g.items() if k.startswith('sd__')}, strict=True)
    rays = torch.stack([g['rays_o'], g['rays_d']], 1)[:64].cuda()
    return mod.cuda(), {'rays': rays, 'time': g['times'][:64].cuda(), 'target_image': g['target'][:64].cuda()}


def _dt_module(likelihood=None):
    from sunerf.model.model import NeRF_DT
    from sunerf.model.sunerf import DensityTemperatureSuNeRFModule
    g = load_golden('g6_dt_e2e')
    mod = DensityTemperatureSuNeRFModule(
        Rs_per_ds=1.0, seconds_per_dt=1.0, image_scaling_config={}, model=NeRF_DT,
        sampling_config={'type': 'stratified', 'n_samples': 16, 'perturb': False},
        hierarchical_sampling_config={'type': 'hierarchical', 'n_samples': 16}, model_config={'d_filter': 64},
        pixel_intensity_factor=float(g['pixel_intensity_factor']),
        response_table=(g['aia_logte'].numpy(), g['aia_tresp'].numpy()), likelihood=likelihood)
    mod.rendering.load_state_dict({k[4:].replace('__', '.'): v for k, v in g.items() if k.startswith('sd__')}, strict=True)
    rays = torch.stack([g['rays_o'], g['rays_d']], 1)[:64].cuda()
    return mod.cuda(), {'rays': rays, 'time': g['times'][:64].cuda(), 'target_image': g['target'][:64].cuda(),
                        'wavelength': g['wavelengths'][:64].cuda()}


def _check_step(mod, like, loss, coarse, fine, target, codes, reg, tag):
    """The loss, ``last_channel_stats`` and ``log_gain.grad`` of a step that has been run AND differentiated already, against the
    restatement on the images the same rays render."""
    ref = lr.evaluate(coarse.cpu().numpy(), fine.cpu().numpy(), target.cpu().numpy(), None if codes is None else codes.cpu().numpy(),
                      like.row_codes.cpu().numpy(), like.noise.cpu().numpy(), like.effective_log_gain().cpu().numpy(),
                      lr.MODEL if like.mode == 'model' else lr.OBSERVED, reg.detach().cpu().numpy(), mod.lambda_image,
                      mod.lambda_regularization)
    assert ref['stats'][6] > 0
    _close32(loss.item(), ref['loss'], f'{tag} loss')
    cs = mod.last_channel_stats.cpu().numpy()
    assert cs.shape == (like.n_rows, 4) and np.array_equal(cs[:, 0], ref['channel_stats'][:, 0])
    _close64(cs[:, 1:], ref['channel_stats'][:, 1:], ref['magnitude'][:, 1:4], f'{tag} last_channel_stats')
    scale = np.float64(np.float32(mod.lambda_image)) / ref['stats'][6]
    want = np.where(like.free.cpu().numpy(), ref['d_log_gain'] * like.gain_rate, 0.0)
    _close32(like.log_gain.grad.cpu().numpy(), want, f'{tag} log_gain.grad', extra=F64_REL * scale * like.gain_rate * ref['magnitude'][:, 4])
    assert float(mod.last_stats[6]) == ref['stats'][6] and float(mod.last_stats[5]) == 0
    return ref


def test_emission_training_step_under_a_likelihood():
    from sunerf.model.sunerf import _other_outputs
    from sunerf_hip.instrument import Instrument
    from sunerf_hip.likelihood import NoiseLikelihood
    from sunerf_hip.train import training_loss
    like = NoiseLikelihood(Instrument(unit=200.0, exposure=2.0, dn_per_photon=1.5, read_noise=2.0, quantise=True), mode='model',
                           free='all', gain_rate=10.0)
    mod, tracing = _emission_module(like)
    with torch.no_grad():
        like.log_gain.fill_(0.01)
    loss = mod.training_step({'tracing': tracing}, 0)
    loss.backward()          # (before the second forward: one pass through the render at a time)
    rays = tracing['rays']
    out = mod.rendering(rays[:, 0].contiguous(), rays[:, 1].contiguous(), tracing['time'])
    _check_step(mod, like, loss, out['coarse_image'].detach(), out['fine_image'].detach(), tracing['target_image'].reshape(-1, 1), None,
                out['regularization'], 'emission')
    (optimizer,), _ = mod.configure_optimizers()
    assert any(p is like.log_gain for p in optimizer._params)
    # likelihood=None: the bits of the parent's step
    plain, tracing = _emission_module()
    loss = plain.training_step({'tracing': tracing}, 0)
    out = plain.rendering(rays[:, 0].contiguous(), rays[:, 1].contiguous(), tracing['time'])
    want, _ = training_loss(out['coarse_image'], out['fine_image'], tracing['target_image'].reshape(-1, 1), out['regularization'],
                            plain.lambda_image, plain.lambda_regularization, asinh_scaling=plain._asinh_constants(),
                            finite_check=_other_outputs(out))
    assert np.array_equal(_bits(loss), _bits(want)) and plain.last_channel_stats is None
    (optimizer,), _ = plain.configure_optimizers()
    assert optimizer.n_params == sum(p.numel() for p in plain.rendering.parameters())


def _dt_likelihood(tracing, free_codes=None, mode='observed'):
    from sunerf_hip.instrument import Instrument
    from sunerf_hip.likelihood import NoiseLikelihood
    codes = sorted({int(c) for c in tracing['wavelength'].cpu().reshape(-1).tolist() if c > 0})
    inst = Instrument(unit=50.0, exposure=2.9, dn_per_photon=1.2, read_noise=1.2)
    free = codes[1:3] if free_codes is None else free_codes
    return NoiseLikelihood(inst, codes=codes, mode=mode, free=free), codes


def test_density_temperature_training_step_under_a_likelihood():
    from sunerf.model.sunerf import _other_outputs
    from sunerf_hip.train import training_loss
    _, tracing = _dt_module()
    like, codes = _dt_likelihood(tracing)
    assert len(codes) >= 2
    mod, tracing = _dt_module(like)
    with torch.no_grad():          # targets of the size of the render, so that neither term of (render - target) is lost
        rays = tracing['rays']
        out = mod.rendering.forward(rays[:, 0].contiguous(), rays[:, 1].contiguous(), tracing['time'], tracing['wavelength'])
        tracing['target_image'] = tracing['target_image'] * (out['fine_image'].mean() / tracing['target_image'].mean())
    loss = mod.training_step({'tracing': tracing}, 0)
    loss.backward()          # (before the second forward: one pass through the render at a time)
    out = mod.rendering.forward(rays[:, 0].contiguous(), rays[:, 1].contiguous(), tracing['time'], tracing['wavelength'])
    ref = _check_step(mod, like, loss, out['coarse_image'].detach(), out['fine_image'].detach(), tracing['target_image'],
                      tracing['wavelength'], out['regularization'], 'density-temperature')
    assert (ref['channel_stats'][:, 0] > 0).sum() >= 2          # more than one row took part
    plain, tracing = _dt_module()
    loss = plain.training_step({'tracing': tracing}, 0)
    out = plain.rendering.forward(rays[:, 0].contiguous(), rays[:, 1].contiguous(), tracing['time'], tracing['wavelength'])
    want, _ = training_loss(out['coarse_image'], out['fine_image'], tracing['target_image'], out['regularization'],
                            plain.lambda_image, plain.lambda_regularization, asinh_scaling=None, finite_check=_other_outputs(out))
    assert np.array_equal(_bits(loss), _bits(want)) and plain.last_channel_stats is None


def test_a_patch_batch_sends_its_views_codes_to_every_detector_pixel():
    from sunerf.model.sunerf import _observed_windows, _patch_codes
    from sunerf_hip.instrument import Instrument
    from sunerf_hip.likelihood import NoiseLikelihood
    from test_gpu_patch import _observations
    rng = np.random.default_rng(23)
    inst = Instrument(psf=rng.uniform(0.1, 1.0, size=(3, 3)), bin=2, unit=30.0, read_noise=[1.0, 2.0])
    pool = _observations(2).patch_pool(inst, patch=4)          # the first view lacks the second channel: codes (171, 0) and (171, 193)
    picks = [2, 4, 13]
    tracing = pool.batch(picks)
    codes = _patch_codes(tracing)
    assert codes.shape == (3 * 16, 2)
    views = [int(pool.triples[k][0]) for k in picks]
    assert set(views) == {0, 1}
    want = np.repeat(np.array([[171.0, 0.0] if v == 0 else [171.0, 193.0] for v in views], dtype=np.float32), 16, axis=0)
    assert np.array_equal(codes.cpu().numpy(), want)

    like = NoiseLikelihood(inst, codes=(171, 193), mode='observed', free=(193,))
    mod, _ = _dt_module(like)
    rays = tracing['rays'].reshape(-1, 2, 3)
    with torch.no_grad():
        scale = mod.rendering(rays[:, 0].contiguous(), rays[:, 1].contiguous(), tracing['time'], tracing['wavelength'])['fine_image'].mean().item()
    tracing['target_image'] = tracing['target_image'] * scale
    loss = mod.training_step({'tracing': tracing}, 0)
    loss.backward()          # (before the second forward: one pass through the render at a time)
    out = mod.rendering(rays[:, 0].contiguous(), rays[:, 1].contiguous(), tracing['time'], tracing['wavelength'])
    coarse, fine, target = _observed_windows(tracing, out)
    ref = _check_step(mod, like, loss, coarse.detach(), fine.detach(), target, codes, out['regularization'], 'patch')
    n0, n1 = views.count(0), views.count(1)
    assert ref['channel_stats'][:, 0].tolist() == [16.0 * (n0 + n1), 16.0 * n1]          # the absent channel of view 0 is masked

    # the emission module on patches: one row, no codes
    from sunerf.model.sunerf import EmissionSuNeRFModule
    single = NoiseLikelihood(Instrument(unit=30.0, read_noise=1.0), free='all')
    emission = EmissionSuNeRFModule(Rs_per_ds=1.0, seconds_per_dt=1.0, image_scaling_config={'vmax': 1, 'a': 0.005},
                                    sampling_config={'type': 'stratified', 'n_samples': 8, 'perturb': False},
                                    hierarchical_sampling_config={'type': 'hierarchical', 'n_samples': 8},
                                    model_config={'d_filter': 64}, likelihood=single).cuda()
    inst1 = Instrument(psf=rng.uniform(0.1, 1.0, size=(3, 5)), bin=2)
    tracing = _observations(1).patch_pool(inst1, patch=4).batch([0, 13])
    torch.manual_seed(0)
    loss = emission.training_step({'tracing': tracing}, 0)
    loss.backward()
    rays = tracing['rays'].reshape(-1, 2, 3)
    out = emission.rendering(rays[:, 0].contiguous(), rays[:, 1].contiguous(), tracing['time'])
    coarse, fine, target = _observed_windows(tracing, out)
    _check_step(emission, single, loss, coarse.detach(), fine.detach(), target, None, out['regularization'], 'emission patch')
