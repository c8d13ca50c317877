"""Training through the instrument on the device (include/sunerf_hip_patch.h): the adjoint of the PSF-and-bin
correlation against the restatement tests/patch_reference.py by bits, the differentiable ``Instrument.expected`` and
``expected_windows``, the records of ``sunerf_patch_records``, and the patch branch of the two modules' ``training_step`` against
the same chain composed by hand.

End-to-end gates: the parameter gradients of the patch ``training_step`` against those of the hand-made chain -- the same rays
through ``module.rendering``, fp64 ``conv2d`` on the device, the loss in torch operations -- at the project's own 1e-3 relative L2
per tensor (tests/test_gpu_backward.py).  Both chains run the same render kernels, so the gate only has to catch a
wrong reshape, channel order or halo offset, and those are errors of order one."""
import functools

import numpy as np
import pytest
import torch

import patch_reference as pr
from conftest import load_golden

pytestmark = pytest.mark.gpu

DEV = 'cuda'


def _bits(t):
    return t.detach().contiguous().cpu().numpy().view(np.uint32)


def _adjoint(g, K, h, w, b, anchor, scale, boundary):
    from sunerf_hip.instrument import BOUNDARY, correlate_bin_adjoint
    taps = torch.as_tensor(np.ascontiguousarray(K), dtype=torch.float64).to(DEV)
    g = torch.as_tensor(g).to(DEV)
    out = correlate_bin_adjoint(g, h, w, taps, K.shape[0], K.shape[1], K.shape[2], b, anchor[0], anchor[1], scale, BOUNDARY[boundary])
    torch.cuda.synchronize()
    return out.cpu().numpy()


@functools.lru_cache(maxsize=None)
def _reference(case, boundary, poisoned):
    K, _, g = pr.case_data(case)
    if poisoned:
        g = g.copy()
        g.reshape(-1)[1] = np.nan
        g.reshape(-1)[g.size // 2] = np.inf
    scale = 1.0 / (case[5] * case[5])
    want, _ = pr.correlate_bin_adjoint(g, K, case[1], case[2], case[5], case[6], scale, boundary)
    return K, g, scale, want


def _same_bits(got, want, what):
    nan_g, nan_w = np.isnan(got), np.isnan(want)
    assert np.array_equal(nan_g, nan_w), f'{what}: NaNs at different positions'
    differ = (got.view(np.uint32) != want.view(np.uint32)) & ~nan_w
    assert not differ.any(), f'{what}: {int(differ.sum())} of {got.size} elements differ by bits, first at {tuple(np.argwhere(differ)[0])}: ' \
                             f'{got[differ][0]!r} != {want[differ][0]!r}'


_IDS = lambda c: '-'.join(str(v) for v in c[:6])          # noqa: E731


# ---- 1. the adjoint ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('boundary', pr.BOUNDARIES)
@pytest.mark.parametrize('case', pr.ADJOINT_CASES + pr.SEAM_CASES, ids=_IDS)
def test_adjoint_equals_the_restatement_by_bits(case, boundary):
    K, g, scale, want = _reference(case, boundary, False)
    got = _adjoint(g, K, case[1], case[2], case[5], case[6], scale, boundary)
    assert got.shape == want.shape and got.dtype == np.float32
    assert not np.isnan(want).any()
    _same_bits(got, want, f'{case} {boundary}')


@pytest.mark.parametrize('boundary', pr.BOUNDARIES)
@pytest.mark.parametrize('case', [pr.ADJOINT_CASES[1], pr.ADJOINT_CASES[6], pr.SEAM_CASES[1]], ids=_IDS)
def test_adjoint_propagates_non_finite_gradients_like_the_restatement(case, boundary):
    K, g, scale, want = _reference(case, boundary, True)
    got = _adjoint(g, K, case[1], case[2], case[5], case[6], scale, boundary)
    assert np.isnan(want).any() and not np.isnan(want).all()
    _same_bits(got, want, f'{case} {boundary} with NaN and inf')


@pytest.mark.parametrize('boundary', pr.BOUNDARIES)
@pytest.mark.parametrize('case', [pr.ADJOINT_CASES[4], pr.ADJOINT_CASES[8], pr.SEAM_CASES[1]], ids=_IDS)
def test_adjoint_is_deterministic_and_a_plane_alone_gives_its_bits_of_the_batch(case, boundary):
    planes, h, w, _, _, b, anchor, per_plane = case
    K, g, scale, _ = _reference(case, boundary, False)
    batch = _adjoint(g, K, h, w, b, anchor, scale, boundary)
    again = _adjoint(g, K, h, w, b, anchor, scale, boundary)
    assert np.array_equal(batch.view(np.uint32), again.view(np.uint32))
    for p in range(planes):
        alone = _adjoint(g[p:p + 1], K[p:p + 1] if per_plane else K, h, w, b, anchor, scale, boundary)
        assert np.array_equal(alone[0].view(np.uint32), batch[p].view(np.uint32)), f'plane {p}'


# ---- 2. Instrument.expected -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('boundary', pr.BOUNDARIES)
def test_expected_is_differentiable_and_keeps_its_bits(boundary):
    from sunerf_hip import lib as binding
    from sunerf_hip.instrument import BOUNDARY, Instrument
    from sunerf_hip.ops import _ptr, _stream
    rng = np.random.default_rng(11)
    psf = rng.uniform(0.0, 1.0, size=(2, 3, 5))
    inst = Instrument(psf=psf, bin=2, boundary=boundary)
    x = torch.from_numpy(rng.uniform(-1.0, 1.0, size=(2, 9, 11)).astype(np.float32)).to(DEV)
    g = torch.from_numpy(rng.uniform(-1.0, 1.0, size=(2, 4, 5)).astype(np.float32)).to(DEV)
    K, (ay, ax) = inst.effective_kernel()
    # the parent's path: the forward entry point, called as Instrument.expected called it
    taps = torch.as_tensor(K, dtype=torch.float64).contiguous().to(DEV)
    parent = torch.empty(2, 4, 5, dtype=torch.float32, device=DEV)
    dev = torch.device(DEV, torch.cuda.current_device())
    binding.call(dev, 'sunerf_instrument_correlate_bin', _ptr(x), 2, 9, 11, _ptr(taps), 2, K.shape[1], K.shape[2], 2, ay, ax,
                 inst.scale, BOUNDARY[boundary], _ptr(parent), _stream(dev))
    plain = inst.expected(x)
    assert plain.grad_fn is None and not plain.requires_grad
    assert np.array_equal(_bits(plain), _bits(parent))
    leaf = x.clone().requires_grad_()
    out = inst.expected(leaf)
    assert out.grad_fn is not None, 'Instrument.expected(x.requires_grad_()) has no grad_fn'
    assert np.array_equal(_bits(out), _bits(parent))
    out.backward(g)
    want, _ = pr.correlate_bin_adjoint(g.cpu().numpy(), K, 9, 11, 2, (ay, ax), inst.scale, boundary)
    _same_bits(leaf.grad.cpu().numpy(), want, 'x.grad')
    with torch.no_grad():
        assert inst.expected(leaf).grad_fn is None


# ---- 3. expected_windows ----------------------------------------------------------------------------------------------------------
def _ulp32(x64):
    a = x64.abs().to(torch.float32)
    return (torch.nextafter(a, torch.full_like(a, float('inf'))) - a).double()


@pytest.mark.parametrize('patch,b,psf_shape,channels', [(4, 2, (3, 3), 1), (3, 3, (4, 2), 1), (4, 2, (2, 3, 3), 2)],
                         ids=['P4-bin2-3x3', 'P3-bin3-4x2', 'per-channel'])
def test_expected_windows_against_fp64_conv2d(patch, b, psf_shape, channels):
    """Forward and ``windows.grad`` within 1 fp32 ulp of fp64 ``conv2d(stride=bin)`` on the device.  Windows, PSF and the incoming
    gradient are positive, so no sum cancels and the fp64 orders of summation differ by 1e-16 of the result: what is compared is
    the one rounding to fp32."""
    from sunerf_hip.instrument import Instrument
    rng = np.random.default_rng(patch * 100 + b)
    psf = rng.uniform(0.1, 1.0, size=psf_shape)
    inst = Instrument(psf=psf, bin=b)
    K, _ = inst.effective_kernel()
    hw, ww = inst.window_shape(patch)
    assert (hw, ww) == ((patch - 1) * b + K.shape[1], (patch - 1) * b + K.shape[2])
    n = 3
    windows = torch.from_numpy(rng.uniform(0.1, 2.0, size=(n, channels, hw, ww)).astype(np.float32)).to(DEV).requires_grad_()
    g = torch.from_numpy(rng.uniform(0.1, 2.0, size=(n, channels, patch, patch)).astype(np.float32)).to(DEV)
    out = inst.expected_windows(windows)
    assert out.shape == (n, channels, patch, patch) and out.dtype == torch.float32
    out.backward(g)
    w64 = windows.detach().double().requires_grad_()
    weight = torch.as_tensor(K, dtype=torch.float64, device=DEV)
    if K.shape[0] == 1:
        ref = torch.nn.functional.conv2d(w64.reshape(n * channels, 1, hw, ww), weight[None], stride=b).reshape(n, channels, patch, patch)
    else:
        ref = torch.nn.functional.conv2d(w64, weight[:, None], stride=b, groups=channels)
    ref = ref * inst.scale
    ref.backward(g.double())
    for what, got, want in (('forward', out.detach(), ref.detach()), ('windows.grad', windows.grad, w64.grad)):
        err = (got.double() - want).abs() / _ulp32(want)
        print(f'expected_windows {what}: largest error {err.max().item():.3f} fp32 ulp of the fp64 result')
        assert err.max().item() <= 1.0, what
    with torch.no_grad():
        assert np.array_equal(_bits(inst.expected_windows(windows)), _bits(out))


# ---- 4. records -------------------------------------------------------------------------------------------------------------------
def _grid(h, w):
    return {'shape': (h, w), 'cdelt': (2.2 * 960. / w, 2.2 * 960. / h)}


def _observations(channels, poison=False, seed=3, full=False):
    """Two views of 12 x 10 and 9 x 9 detector pixels; with two channels the first view lacks the second one unless ``full``."""
    from sunerf_hip.observations import ObservationSet
    rng = np.random.default_rng(seed)
    obs = ObservationSet(device=DEV)
    shapes = ((12, 10), (9, 9))
    for k, (h, w) in enumerate(shapes):
        if channels == 1:
            image, wl = rng.uniform(0.05, 1.0, size=(1, h, w)), None
        elif k == 0 and not full:
            image, wl = rng.uniform(0.05, 1.0, size=(1, h, w)), [171., 0.]
        else:
            image, wl = rng.uniform(0.05, 1.0, size=(2, h, w)), [171., 193.]
        image = torch.from_numpy(image.astype(np.float32))
        if poison and k == 1:
            image[-1, 0, 0] = float('nan')
        obs.add_view(image, 0.1 - 0.2 * k, 0.3 + 0.9 * k, time=0.25 * k, grid=_grid(h, w), wavelengths=wl)
    return obs


def test_patch_records():
    from sunerf_hip.instrument import Instrument
    from sunerf_hip.rays import grid_rays
    rng = np.random.default_rng(5)
    inst = Instrument(psf=rng.uniform(0.1, 1.0, size=(3, 3)), bin=2)
    obs = _observations(2)
    pool = obs.patch_pool(inst, patch=4)
    assert pool.dropped == 0 and pool.n_patches == 18 and (pool.hw, pool.ww) == (10, 10)
    triples = [tuple(int(v) for v in t) for t in pool.triples]
    # all four corners, the shifted last lattice positions and the interior of both views
    for want in [(0, 0, 0), (0, 0, 6), (0, 8, 0), (0, 8, 6), (0, 4, 4), (1, 0, 0), (1, 0, 5), (1, 5, 0), (1, 5, 5), (1, 4, 4)]:
        assert want in triples, want
    batch = pool.batch(np.arange(pool.n_patches))
    torch.cuda.synchronize()
    spec = batch['patch']
    assert (spec['n'], spec['C'], spec['P'], spec['hw'], spec['ww']) == (18, 2, 4, 10, 10) and spec['instrument'] is inst
    assert batch['rays'].shape == (18, 10, 10, 2, 3) and batch['time'].shape == (1800, 1)
    assert batch['target_image'].shape == (18, 2, 4, 4) and batch['wavelength'].shape == (1800, 2)
    time, wl = batch['time'].view(18, 100), batch['wavelength'].view(18, 100, 2)
    for k, (v, r0, c0) in enumerate(triples):
        view, (tx, ty) = pool.views[v], pool.axes[v]
        assert tx.shape[0] == (view.width - 1) * 2 + 4 and ty.shape[0] == (view.height - 1) * 2 + 4
        o, d = grid_rays(tx[c0 * 2:c0 * 2 + 10].contiguous(), ty[r0 * 2:r0 * 2 + 10].contiguous(), view.c2w)
        assert torch.equal(batch['rays'][k, :, :, 0], o.view(10, 10, 3)) and torch.equal(batch['rays'][k, :, :, 1], d.view(10, 10, 3)), (v, r0, c0)
        want = torch.zeros(2, 4, 4, device=DEV)
        for c in range(2):
            if view.plane[c] >= 0:
                want[c] = view.image[int(view.plane[c]), r0:r0 + 4, c0:c0 + 4]
        assert torch.equal(batch['target_image'][k], want), (v, r0, c0)
        assert bool((time[k] == np.float32(view.time)).all())
        assert torch.equal(wl[k], torch.as_tensor(view.wavelength, device=DEV).expand(100, 2))
    # a NaN pixel drops its patch and only that patch
    poisoned = _observations(2, poison=True).patch_pool(inst, patch=4)
    assert poisoned.dropped == 1 and poisoned.n_patches == 17
    assert [tuple(int(v) for v in t) for t in poisoned.triples] == [t for t in triples if t != (1, 0, 0)]
    # epochs: one permutation, rank r takes [r::world]
    shards = [obs.patch_pool(inst, patch=4, rank=r, world=4, seed=9).order(2) for r in range(4)]
    whole = np.random.default_rng([9, 2]).permutation(18)
    assert all(np.array_equal(s, whole[r::4]) for r, s in enumerate(shards))
    assert pool.patches_per_batch == 82 and len(pool) == 1          # 8192 / 100 rays


def test_patch_pool_rejections():
    from sunerf_hip.instrument import Instrument
    from sunerf_hip.observations import ObservationSet
    inst = Instrument(psf=np.ones((3, 3)) / 9, bin=2)
    with pytest.raises(ValueError):
        _observations(1).patch_pool(inst, patch=10)          # the 9 x 9 view is smaller than the patch
    obs = ObservationSet(device=DEV)
    obs.add_view(torch.ones(8, 8), 0.0, 0.0, grid=_grid(8, 8), downscale=2)
    with pytest.raises(ValueError):
        obs.patch_pool(inst, patch=4)
    obs = ObservationSet(device=DEV)
    obs.add_view(torch.ones(8, 8), 0.0, 0.0, tx=torch.zeros(8, 8, dtype=torch.float64), ty=torch.zeros(8, 8, dtype=torch.float64))
    with pytest.raises(ValueError):
        obs.patch_pool(inst, patch=4)


# ---- 5. end to end ----------------------------------------------------------------------------------------------------------------
def _detector_fp64(image, spec, K, scale):
    """[n hw ww, C] rendered window rays -> [n P P, C] detector pixels: fp64 conv2d on the device."""
    n, hw, ww, b = spec['n'], spec['hw'], spec['ww'], spec['instrument'].bin
    windows = image.reshape(n, hw, ww, -1).permute(0, 3, 1, 2).double()
    c = windows.shape[1]
    weight = torch.as_tensor(K, dtype=torch.float64, device=image.device)
    if K.shape[0] == 1:
        det = torch.nn.functional.conv2d(windows.reshape(n * c, 1, hw, ww), weight[None], stride=b).reshape(n, c, spec['P'], spec['P'])
    else:
        det = torch.nn.functional.conv2d(windows, weight[:, None], stride=b, groups=c)
    return (det * scale).permute(0, 2, 3, 1).reshape(-1, c)


def _gradients_of(module, loss):
    """``loss.backward()`` on cleared gradients: {name: gradient or None}, the module's gradients cleared again."""
    params = dict(module.rendering.named_parameters())
    for p in params.values():
        p.grad = None
    loss.backward()
    got = {k: (None if p.grad is None else p.grad.detach().clone()) for k, p in params.items()}
    for p in params.values():
        p.grad = None
    return got


def _compare_gradients(module, got, reference_loss):
    """Per-tensor relative L2 of the gradients ``got`` against those of ``reference_loss``, gated at 1e-3."""
    params = dict(module.rendering.named_parameters())
    reference_loss.backward()
    worst = 0.0
    compared = 0
    for name, p in params.items():
        ref = p.grad
        if ref is None or float(ref.abs().max()) == 0.0:
            assert got[name] is None or float(got[name].abs().max()) == 0.0, name
            continue
        err = ((got[name].double() - ref.double()).norm() / ref.double().norm()).item()
        worst = max(worst, err)
        compared += 1
        assert err < 1e-3, (name, err)
    print(f'patch training step: {compared} gradient tensors, worst relative L2 {worst:.2e} (bound 1e-3)')
    assert compared >= 16


def test_patch_training_step_emission():
    from sunerf.model.sunerf import EmissionSuNeRFModule
    from sunerf_hip.instrument import Instrument
    torch.manual_seed(0)
    rng = np.random.default_rng(21)
    inst = Instrument(psf=rng.uniform(0.1, 1.0, size=(3, 5)), bin=2)
    pool = _observations(1).patch_pool(inst, patch=4)
    tracing = pool.batch([0, 4, 13])          # a corner and the interior of the first view, the interior of the second
    mod = EmissionSuNeRFModule(Rs_per_ds=1.0, seconds_per_dt=1.0, image_scaling_config={'vmax': 1, 'a': 0.005},
                               sampling_config={'type': 'stratified', 'n_samples': 8, 'perturb': False},
                               hierarchical_sampling_config={'type': 'hierarchical', 'n_samples': 8},
                               model_config={'d_filter': 64}).cuda()
    loss = mod.training_step({'tracing': tracing}, 0)
    got = _gradients_of(mod, loss)          # (before the second forward: one pass through the render at a time)
    spec = tracing['patch']
    K, _ = inst.effective_kernel()
    rays = tracing['rays'].reshape(-1, 2, 3)
    out = mod.rendering(rays[:, 0].contiguous(), rays[:, 1].contiguous(), tracing['time'])
    target = tracing['target_image'].permute(0, 2, 3, 1).reshape(-1, 1).double()
    s = lambda x: torch.asinh(x / 1.0 / 0.005) / float(np.arcsinh(1 / 0.005))          # noqa: E731
    mse = lambda a, b: ((a - b) ** 2).mean()                                             # noqa: E731
    coarse, fine = (_detector_fp64(out[k], spec, K, inst.scale) for k in ('coarse_image', 'fine_image'))
    assert coarse.shape == target.shape == (3 * 16, 1)
    reference = mod.lambda_image * (mse(s(coarse), s(target)) + mse(s(fine), s(target))) \
        + mod.lambda_regularization * out['regularization'].double().mean()
    print(f'patch training step (emission): loss {loss.item():.8g}, by hand {reference.item():.8g}')
    assert abs(loss.item() - reference.item()) < 2e-4 * abs(reference.item())
    _compare_gradients(mod, got, reference)


def test_patch_training_step_density_temperature():
    from sunerf.model.model import NeRF_DT
    from sunerf.model.sunerf import DensityTemperatureSuNeRFModule
    from sunerf_hip.instrument import Instrument
    g = load_golden('g6_dt_e2e')
    rng = np.random.default_rng(22)
    inst = Instrument(psf=rng.uniform(0.1, 1.0, size=(2, 3, 3)), bin=2)          # a different PSF per channel
    pool = _observations(2, full=True).patch_pool(inst, patch=4)
    tracing = pool.batch([2, 4, 13])
    mod = DensityTemperatureSuNeRFModule(
        Rs_per_ds=1.0, seconds_per_dt=1.0, image_scaling_config={}, model=NeRF_DT,
        sampling_config={'type': 'stratified', 'n_samples': 16, 'perturb': False},
        hierarchical_sampling_config={'type': 'hierarchical', 'n_samples': 16}, model_config={'d_filter': 64},
        pixel_intensity_factor=float(g['pixel_intensity_factor']),
        response_table=(g['aia_logte'].numpy(), g['aia_tresp'].numpy()))
    mod.rendering.load_state_dict({k[4:].replace('__', '.'): v for k, v in g.items() if k.startswith('sd__')}, strict=True)
    mod = mod.cuda()
    with torch.no_grad():          # targets of the size of the render, so that neither term of (render - target) is lost
        rays = tracing['rays'].reshape(-1, 2, 3)
        scale = mod.rendering(rays[:, 0].contiguous(), rays[:, 1].contiguous(), tracing['time'], tracing['wavelength'])['fine_image'].mean().item()
    tracing['target_image'] = tracing['target_image'] * scale
    loss = mod.training_step({'tracing': tracing}, 0)
    got = _gradients_of(mod, loss)
    spec = tracing['patch']
    K, _ = inst.effective_kernel()
    assert K.shape[0] == 2 and not np.array_equal(K[0], K[1])
    out = mod.rendering(rays[:, 0].contiguous(), rays[:, 1].contiguous(), tracing['time'], tracing['wavelength'])
    target = tracing['target_image'].permute(0, 2, 3, 1).reshape(-1, 2).double()
    mse = lambda a, b: ((a - b) ** 2).mean()          # noqa: E731
    coarse, fine = (_detector_fp64(out[k], spec, K, inst.scale) for k in ('coarse_image', 'fine_image'))
    assert coarse.shape == target.shape == (3 * 16, 2)
    reference = mod.lambda_image * (mse(coarse, target) + mse(fine, target)) + mod.lambda_regularization * out['regularization'].double().mean()
    print(f'patch training step (density-temperature): loss {loss.item():.8g}, by hand {reference.item():.8g}')
    assert abs(loss.item() - reference.item()) < 2e-4 * abs(reference.item())
    _compare_gradients(mod, got, reference)


# ---- 6. regression ----------------------------------------------------------------------------------------------------------------
def test_a_batch_without_patch_takes_the_parents_lines():
    """The loss bits of ``training_step`` on a ray batch are those of the parent commit's lines, restated here."""
    from sunerf.model.model import NeRF_DT
    from sunerf.model.sunerf import DensityTemperatureSuNeRFModule, EmissionSuNeRFModule, _other_outputs
    from sunerf_hip.train import training_loss
    g = load_golden('g5_emission_e2e')
    mod = EmissionSuNeRFModule(Rs_per_ds=1.0, seconds_per_dt=1.0, image_scaling_config={'vmax': 1, 'a': 0.005},
                               sampling_config={'type': 'stratified', 'n_samples': 32, 'perturb': False},
                               hierarchical_sampling_config={'type': 'hierarchical', 'n_samples': 32}, model_config={'d_filter': 64})
    mod.rendering.load_state_dict({k[4:].replace('__', '.'): v for k, v in g.items() if k.startswith('sd__')}, strict=True)
    mod = mod.cuda()
    rays = torch.stack([g['rays_o'], g['rays_d']], 1).cuda()
    tracing = {'rays': rays, 'time': g['times'].cuda(), 'target_image': g['target'].cuda()}
    loss = mod.training_step({'tracing': tracing}, 0)
    out = mod.rendering(rays[:, 0].contiguous(), rays[:, 1].contiguous(), tracing['time'])
    want, _ = training_loss(out['coarse_image'], out['fine_image'], tracing['target_image'].reshape(-1, 1), out['regularization'],
                            mod.lambda_image, mod.lambda_regularization, asinh_scaling=mod._asinh_constants(),
                            finite_check=_other_outputs(out))
    assert np.array_equal(_bits(loss), _bits(want))

    g = load_golden('g6_dt_e2e')
    mod = DensityTemperatureSuNeRFModule(
        Rs_per_ds=1.0, seconds_per_dt=1.0, image_scaling_config={}, model=NeRF_DT,
        sampling_config={'type': 'stratified', 'n_samples': 16, 'perturb': False},
        hierarchical_sampling_config={'type': 'hierarchical', 'n_samples': 16}, model_config={'d_filter': 64},
        pixel_intensity_factor=float(g['pixel_intensity_factor']),
        response_table=(g['aia_logte'].numpy(), g['aia_tresp'].numpy()))
    mod.rendering.load_state_dict({k[4:].replace('__', '.'): v for k, v in g.items() if k.startswith('sd__')}, strict=True)
    mod = mod.cuda()
    rays = torch.stack([g['rays_o'], g['rays_d']], 1).cuda()
    tracing = {'rays': rays, 'time': g['times'].cuda(), 'target_image': g['target'].cuda(), 'wavelength': g['wavelengths'].cuda()}
    loss = mod.training_step({'tracing': tracing}, 0)
    out = mod.rendering.forward(rays[:, 0].contiguous(), rays[:, 1].contiguous(), tracing['time'], tracing['wavelength'])
    want, _ = training_loss(out['coarse_image'], out['fine_image'], tracing['target_image'], out['regularization'],
                            mod.lambda_image, mod.lambda_regularization, asinh_scaling=None, finite_check=_other_outputs(out))
    assert np.array_equal(_bits(loss), _bits(want))
    assert abs(loss.item() - g['loss'].item()) < 2e-4 * abs(g['loss'].item())
