"""Image scores on MI355X: sunerf_image_metrics against scikit-image's own SSIM (g14) and against the fp64
restatement tests/metrics_reference.py at edge and frame shapes, its determinism, batch invariance and NaN isolation; the
module's validation_metrics against the reference callbacks restated in fp64; the loaders' ``strides``; EnsembleLoader; and
the error / uncertainty correlation against numpy and scipy."""
import datetime
import os

import numpy as np
import pytest
import torch

import metrics_reference as mr
from conftest import GOLDEN

pytestmark = pytest.mark.gpu


def _scores(pred, target, r):
    from sunerf_hip.metrics import image_metrics
    out = image_metrics(torch.from_numpy(np.ascontiguousarray(pred)).cuda(),
                        torch.from_numpy(np.ascontiguousarray(target)).cuda(), r)
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in out.items()}


# ---- 1. against scikit-image ------------------------------------------------------------------------------------------------
def test_kernel_matches_skimage_golden():
    with np.load(os.path.join(GOLDEN, 'skimage', 'g14_ssim_skimage.npz')) as z:
        g = {k: z[k] for k in z.files}
    for name in (str(n) for n in g['names']):
        target, pred = g[f'{name}__target'], g[f'{name}__pred']
        d = pred.astype(np.float64) - target
        axes = (-2, -1)
        for r in (1, 255):
            got = _scores(pred, target, r)
            want = g[f'{name}__ssim_r{r}']
            assert got['ssim'].shape == want.shape, name
            assert np.abs(got['ssim'] - want).max() <= 1e-12, (name, r, np.abs(got['ssim'] - want).max())
            np.testing.assert_allclose(got['mse'], (d * d).mean(axes), rtol=1e-12, atol=0, err_msg=name)
            np.testing.assert_allclose(got['mae'], np.abs(d).mean(axes), rtol=1e-12, atol=0, err_msg=name)
            np.testing.assert_allclose(got['me'], d.mean(axes), rtol=1e-12, atol=1e-300, err_msg=name)
            with np.errstate(divide='ignore'):
                np.testing.assert_allclose(got['psnr'], 10 * np.log10(r * r / (d * d).mean(axes)), rtol=1e-12, err_msg=name)


# ---- 2. against the fp64 restatement ---------------------------------------------------------------------------------------
def _inputs(kind, shape, r, seed):
    rng = np.random.default_rng(seed)
    n, h, w = shape
    yy, xx = np.meshgrid(np.linspace(-1, 1, h), np.linspace(-1, 1, w), indexing='ij')
    if kind == 'noise':
        target = rng.random(shape) * r
        pred = np.clip(target + 0.1 * r * rng.standard_normal(shape), 0, 3 * r)
    elif kind == 'smooth':          # low variance on a large mean: uxx - ux^2 cancels
        field = 2 * r + 1e-3 * r * np.sin(7 * xx + 2 * yy) * np.cos(3 * yy)
        target = np.broadcast_to(field, shape) + 1e-4 * r * rng.standard_normal(shape)
        pred = target + 2e-4 * r * rng.standard_normal(shape)
    else:                           # a limb-darkened disc on a dark background, the shape of a solar frame
        rad = np.sqrt(xx ** 2 + yy ** 2) / 0.8
        disc = np.where(rad < 1, r * (0.4 + 0.6 * np.sqrt(np.clip(1 - rad ** 2, 0, 1))), 0.01 * r)
        target = np.broadcast_to(disc, shape) * (1 + 0.05 * rng.standard_normal(shape))
        pred = np.clip(target * (1 + 0.1 * rng.standard_normal(shape)), 0, 3 * r)
    return np.clip(pred, 0, 3 * r).astype(np.float32), np.clip(target, 0, 3 * r).astype(np.float32)


@pytest.mark.parametrize('shape,kind', [((1, 7, 7), 'noise'), ((1, 7, 4099), 'smooth'), ((1, 4099, 7), 'disc'),
                                        ((3, 1031, 2053), 'noise'), ((7, 256, 256), 'smooth'), ((7, 256, 256), 'disc'),
                                        ((1, 4096, 4096), 'disc')])
def test_kernel_matches_restatement(shape, kind):
    for r in (1, 255):
        pred, target = _inputs(kind, shape, r, seed=sum(shape) + r)
        got = _scores(pred, target, r)
        want = mr.image_metrics(pred, target, r)
        assert got['ssim'].shape == (shape[0],)
        assert np.abs(got['ssim'] - want['ssim']).max() <= 1e-10, (shape, kind, r, np.abs(got['ssim'] - want['ssim']).max())
        for k in ('mse', 'mae'):
            np.testing.assert_allclose(got[k], want[k], rtol=1e-12, atol=0, err_msg=k)
        np.testing.assert_allclose(got['me'], want['me'], rtol=1e-9, atol=1e-15 * r)


# ---- 3. identical images ----------------------------------------------------------------------------------------------------
def test_identical_images():
    pred, _ = _inputs('disc', (3, 45, 77), 1, seed=5)
    for r in (1, 255):
        got = _scores(pred, pred.copy(), r)
        assert np.abs(1 - got['ssim']).max() <= 1e-15
        assert (got['mse'] == 0).all() and (got['mae'] == 0).all() and (got['me'] == 0).all()
        assert np.isinf(got['psnr']).all()


# ---- 4. determinism and batch invariance ------------------------------------------------------------------------------------
def test_bitwise_batch_invariance_and_reruns():
    from sunerf_hip.metrics import image_metrics
    pred, target = _inputs('noise', (5, 67, 131), 1, seed=9)
    p, t = torch.from_numpy(pred).cuda(), torch.from_numpy(target).cuda()
    batch = torch.stack([image_metrics(p, t, 1.0)[k] for k in ('ssim', 'mse', 'mae', 'me')], -1)
    again = torch.stack([image_metrics(p, t, 1.0)[k] for k in ('ssim', 'mse', 'mae', 'me')], -1)
    assert torch.equal(batch, again)
    rev = torch.stack([image_metrics(p.flip(0), t.flip(0), 1.0)[k] for k in ('ssim', 'mse', 'mae', 'me')], -1)
    assert torch.equal(rev.flip(0), batch)
    for i in range(5):
        alone = torch.stack([image_metrics(p[i], t[i], 1.0)[k] for k in ('ssim', 'mse', 'mae', 'me')], -1)
        assert alone.shape == (4,)
        assert torch.equal(alone, batch[i]), i


# ---- 5. NaN ----------------------------------------------------------------------------------------------------------------
def test_nan_stays_in_its_image():
    pred, target = _inputs('disc', (4, 40, 70), 1, seed=11)
    clean = _scores(pred, target, 1.0)
    pred[2, 0, 69] = np.nan                     # a corner pixel: inside one crop window only
    dirty = _scores(pred, target, 1.0)
    for k in ('ssim', 'mse', 'mae', 'me', 'psnr'):
        assert np.isnan(dirty[k][2]), k
        keep = [0, 1, 3]
        assert np.array_equal(dirty[k][keep], clean[k][keep]), k


def test_argument_errors_from_python():
    from sunerf_hip.metrics import image_metrics
    a = torch.zeros(6, 9, device='cuda')
    with pytest.raises(ValueError, match='7 x 7'):
        image_metrics(a, a, 1.0)
    b = torch.zeros(2, 9, 9, device='cuda')
    with pytest.raises(ValueError, match='data_range'):
        image_metrics(b, b, 0.0)
    out = image_metrics(torch.zeros(0, 9, 9, device='cuda'), torch.zeros(0, 9, 9, device='cuda'), 1.0)
    assert out['ssim'].shape == (0,)
    # float64 / non-contiguous inputs are taken as contiguous fp32
    x, y = torch.rand(2, 20, 30, device='cuda', dtype=torch.float64), torch.rand(2, 20, 30, device='cuda', dtype=torch.float64)
    got = image_metrics(x.transpose(1, 2), y.transpose(1, 2), 1.0)
    want = image_metrics(x.float().transpose(1, 2).contiguous(), y.float().transpose(1, 2).contiguous(), 1.0)
    assert all(torch.equal(got[k], want[k]) for k in got)


# ---- 6. validation_metrics -------------------------------------------------------------------------------------------------
def _check_scores(got, want):
    assert set(got) == {'validation.loss', 'validation.ssim', 'validation.psnr'}
    for k, v in got.items():
        assert v.dim() == 0 and v.dtype == torch.float64 and v.is_cuda, k
        assert abs(v.item() - want[k]) <= 1e-10 * max(1.0, abs(want[k])), (k, v.item(), want[k])


def test_validation_metrics_emission():
    from sunerf.model.sunerf import EmissionSuNeRFModule
    from sunerf_hip.rays import observer_rays
    torch.manual_seed(4)
    lm = EmissionSuNeRFModule(Rs_per_ds=1.0, seconds_per_dt=1.0, image_scaling_config={'vmax': 1.0, 'a': 0.005},
                              sampling_config={'type': 'stratified', 'n_samples': 32, 'perturb': False},
                              hierarchical_sampling_config={'type': 'hierarchical', 'n_samples': 32},
                              model_config={'d_filter': 64}, validation_dataset_mapping={0: 'test', 1: 'other'}).cuda()
    h, w = 10, 11
    o, d = observer_rays(11, 0, 10, device='cuda')
    rays = torch.stack([o, d], 1)
    time = torch.full((h * w, 1), 0.25, device='cuda')
    target = torch.rand(h * w, 1, device='cuda') * 1.2 - 0.1          # beyond [0, 1]: the clip takes part
    batches = [lm.validation_step({'rays': rays[s], 'time': time[s], 'target_image': target[s]}, i)
               for i, s in enumerate((slice(0, 60), slice(60, None)))]
    assert lm.validation_step({'rays': rays, 'time': time, 'target_image': target}, 0, dataloader_idx=1) is None
    other = [{'fine_image': torch.zeros(49, 1, device='cuda'), 'target_image': torch.ones(49, 1, device='cuda')}]
    lm.validation_epoch_end([batches, other])
    stored = lm.validation_outputs['test']
    want = mr.callback_scores(stored['fine_image'].cpu().numpy(), stored['target_image'].cpu().numpy(), (h, w), normalize=True)
    _check_scores(lm.validation_metrics((h, w)), want)               # default: the first set
    _check_scores(lm.validation_metrics((h, w), name='test'), want)
    assert lm.validation_metrics((7, 7), name='other')['validation.loss'].item() == 1.0
    with pytest.raises(ValueError):
        lm.validation_metrics((w, w))


def test_validation_metrics_density_temperature():
    from conftest import load_golden
    from sunerf.model.model import NeRF_DT
    from sunerf.model.sunerf import DensityTemperatureSuNeRFModule
    from sunerf_hip.rays import observer_rays
    g = load_golden('g6_dt_e2e')
    torch.manual_seed(6)
    lm = DensityTemperatureSuNeRFModule(
        Rs_per_ds=1.0, seconds_per_dt=1.0, image_scaling_config={}, model=NeRF_DT,
        sampling_config={'type': 'stratified', 'n_samples': 16, 'perturb': False},
        hierarchical_sampling_config={'type': 'hierarchical', 'n_samples': 16}, model_config={'d_filter': 64},
        pixel_intensity_factor=float(g['pixel_intensity_factor']),
        response_table=(g['aia_logte'].numpy(), g['aia_tresp'].numpy()), validation_dataset_mapping={0: 'test'})
    sd = {k[4:].replace('__', '.'): v for k, v in g.items() if k.startswith('sd__')}
    lm.rendering.load_state_dict(sd, strict=True)
    lm = lm.cuda()
    h, w = 9, 9
    o, d = observer_rays(9, device='cuda')
    rays = torch.stack([o, d], 1)
    wl = g['wavelengths'][0:1].expand(h * w, -1).contiguous().cuda()
    out = lm.validation_step({'rays': rays, 'time': torch.zeros(h * w, 1, device='cuda'),
                              'target_image': torch.zeros(h * w, wl.shape[1], device='cuda'), 'wavelength': wl}, 0)
    scale = out['fine_image'].abs().max().clamp_min(1e-30)
    target = out['fine_image'] + 0.1 * scale * torch.randn_like(out['fine_image'])
    out['target_image'] = target
    lm.validation_epoch_end([out])
    want = mr.callback_scores(out['fine_image'].cpu().numpy(), target.cpu().numpy(), (h, w), normalize=False)
    _check_scores(lm.validation_metrics((h, w)), want)
    with pytest.raises(ValueError):
        lm.validation_metrics((8, 10))


# ---- 7. strides -------------------------------------------------------------------------------------------------------------
class _Module:
    pass


def _data(shape=(37, 53), ref_time=datetime.datetime(2022, 1, 1)):
    class _Data:
        config = {'wavelength': 193, 'times': [datetime.datetime(2022, 1, 1), datetime.datetime(2022, 1, 3)],
                  'resolution': shape, 'wcs': {'shape': shape, 'cdelt': (90., 70.)}}
        seconds_per_dt, Rs_per_ds = 86400., 1.0
    _Data.ref_time = ref_time
    return _Data()


def _state(tmp_path, name, seed, **kw):
    from sunerf.model.sunerf import save_state
    from sunerf.rendering.emission import EmissionRadiativeTransfer
    torch.manual_seed(seed)
    mod = _Module()
    mod.rendering = EmissionRadiativeTransfer(Rs_per_ds=1.0,
                                              sampling_config={'type': 'stratified', 'n_samples': 32, 'perturb': False},
                                              hierarchical_sampling_config={'type': 'hierarchical', 'n_samples': 32},
                                              model_config={'d_filter': 64})
    path = str(tmp_path / name / 'save_state.snf')
    save_state(mod, _data(**kw), path)
    return path


@pytest.mark.parametrize('mode', ['exact', 'fast'])
def test_strides_slice_the_full_frame(tmp_path, monkeypatch, mode):
    monkeypatch.setenv('SUNERF_FORWARD_PRECISION', mode)
    from sunerf.evaluation.loader import ModelLoader, SuNeRFLoader
    loader = SuNeRFLoader(_state(tmp_path, 'a', 3), device='cuda')
    when = datetime.datetime(2022, 1, 2, 6)
    full = loader.render_observer_image(0.2, -0.4, when, distance=200.)
    assert full['image'].shape == (37, 53, 1)
    model_loader = ModelLoader(loader.rendering, loader.model, ref_map=loader.ref_map)
    full_m = model_loader.render_observer_image(0.2, -0.4, 1.25, distance=200.)
    for s in (2, 3):
        part = loader.render_observer_image(0.2, -0.4, when, distance=200., strides=s)
        part_m = model_loader.render_observer_image(0.2, -0.4, 1.25, distance=200., strides=s, as_numpy=False)
        assert set(part) == set(full)
        for k in full:
            assert np.array_equal(part[k], full[k][::s, ::s]), (s, k)
            assert np.array_equal(part_m[k].cpu().numpy(), full_m[k][::s, ::s]), (s, k)
    with pytest.raises(ValueError):
        loader.render_observer_image(0.2, -0.4, when, strides=0)


def test_strides_on_per_pixel_angles(monkeypatch):
    monkeypatch.setenv('SUNERF_FORWARD_PRECISION', 'exact')
    from sunerf.evaluation.loader import ModelLoader, linear_plate_scale_axes
    from sunerf.rendering.emission import EmissionRadiativeTransfer
    torch.manual_seed(8)
    rendering = EmissionRadiativeTransfer(Rs_per_ds=1.0,
                                          sampling_config={'type': 'stratified', 'n_samples': 32, 'perturb': False},
                                          hierarchical_sampling_config={'type': 'hierarchical', 'n_samples': 32},
                                          model_config={'d_filter': 64})

    class _PerPixel(ModelLoader):          # a real WCS gives per-pixel (H, W) angles (all_coordinates_from_map)
        def _pixel_angles(self, resolution):
            tx, ty = linear_plate_scale_axes({'shape': (23, 31), 'cdelt': (120., 100.)}, resolution, self.device)
            return (tx[None, :].expand(23, -1) + 1e-5 * ty[:, None]).contiguous(), ty[:, None].expand(-1, 31).contiguous()
    loader = _PerPixel(rendering, rendering.fine_model, ref_map={'meta': {}})
    full = loader.render_observer_image(0.1, 0.3, 0.5, distance=150.)
    part = loader.render_observer_image(0.1, 0.3, 0.5, distance=150., strides=3)
    for k in full:
        assert np.array_equal(part[k], full[k][::3, ::3]), k


# ---- 8. EnsembleLoader ------------------------------------------------------------------------------------------------------
def test_ensemble_loader(tmp_path, monkeypatch):
    monkeypatch.setenv('SUNERF_FORWARD_PRECISION', 'exact')
    from sunerf.evaluation.loader import EnsembleLoader, SuNeRFLoader
    a, b = _state(tmp_path, 'a', 3), _state(tmp_path, 'b', 4)
    when = datetime.datetime(2022, 1, 2)
    ens = EnsembleLoader([a, b, a], device='cuda')
    out = ens.render_observer_image(-0.1, 0.5, when, distance=180., strides=2)
    single = SuNeRFLoader(a, device='cuda').render_observer_image(-0.1, 0.5, when, distance=180., strides=2)
    for k, v in single.items():
        assert np.array_equal(out[k], v), k
    members = [SuNeRFLoader(p, device='cuda').render_observer_image(-0.1, 0.5, when, distance=180., strides=2)['image']
               for p in (a, b, a)]
    stack = np.stack(members).astype(np.float64)
    assert out['ensemble_mean'].dtype == np.float32 and out['ensemble_mean'].shape == single['image'].shape
    eps = 2. ** -23
    assert (np.abs(out['ensemble_mean'] - stack.mean(0)) <= eps * np.abs(stack.mean(0))).all()
    assert (np.abs(out['ensemble_std'] - stack.std(0)) <= eps * np.abs(stack.std(0))).all()
    assert out['ensemble_std'].max() > 0
    same = EnsembleLoader([a, a], device='cuda').render_observer_image(-0.1, 0.5, when, distance=180., as_numpy=False)
    assert bool((same['ensemble_std'] == 0).all())
    assert torch.equal(same['ensemble_mean'], same['image'])
    other = _state(tmp_path, 'c', 5, ref_time=datetime.datetime(2022, 1, 2))
    with pytest.raises(ValueError, match='ref_time') as err:
        EnsembleLoader([a, other], device='cuda')
    assert other in str(err.value)


# ---- 9. correlation ---------------------------------------------------------------------------------------------------------
def test_error_uncertainty_correlation():
    stats = pytest.importorskip('scipy.stats')
    from sunerf_hip.metrics import error_uncertainty_correlation
    rng = np.random.default_rng(12)
    n = 1_000_000
    unc = np.round(rng.random(n) * 50) / 50                      # 51 distinct values: many ties
    unc[: n // 10] = 0                                           # identical members: uncertainty 0
    err = np.round(np.abs(unc * 2 + 0.3 * rng.standard_normal(n)) * 200) / 200
    err, unc = err.astype(np.float32), unc.astype(np.float32)
    out = error_uncertainty_correlation(torch.from_numpy(err).cuda().reshape(1000, 1000),
                                        torch.from_numpy(unc).cuda().reshape(1000, 1000))
    assert out['pearson'].is_cuda and out['pearson'].dtype == torch.float64 and out['pearson'].dim() == 0
    want_p = np.corrcoef(err.astype(np.float64), unc.astype(np.float64))[0, 1]
    want_s = stats.spearmanr(err, unc).correlation
    assert abs(out['pearson'].item() - want_p) <= 1e-9
    assert abs(out['spearman'].item() - want_s) <= 1e-9
