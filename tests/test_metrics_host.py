"""Image scores without a GPU: the fp64 restatement tests/metrics_reference.py against scikit-image's own
SSIM (tests/golden/skimage/g14_ssim_skimage.npz), the argument errors and workspace size of the two C entry points, and the
restatement of the emission callback's asinh normalisation."""
import ctypes
import math
import os

import numpy as np
import pytest
import torch

import metrics_reference as mr
from conftest import GOLDEN

BADARG, WORKSPACE = -1, -3


def _g14():
    with np.load(os.path.join(GOLDEN, 'skimage', 'g14_ssim_skimage.npz')) as z:
        return {k: z[k] for k in z.files}


def test_restatement_reproduces_skimage():
    g = _g14()
    assert str(g['skimage_version']) == '0.18.3'
    names = [str(n) for n in g['names']]
    assert {'r7x7', 'r7x40', 'r40x7', 'r13x29', 'r64x64', 'r97x131', 'stack3x37x53', 'constant', 'identical',
            'three_r'} <= set(names)
    for name in names:
        target, pred = g[f'{name}__target'], g[f'{name}__pred']
        assert target.dtype == np.float32 and pred.dtype == np.float32
        for r in (1, 255):
            want = g[f'{name}__ssim_r{r}']
            got = mr.image_metrics(pred, target, r)['ssim']
            assert got.shape == want.shape, name
            assert np.abs(got - want).max() <= 1e-12, (name, r, np.abs(got - want).max())
    assert float(g['identical__ssim_r1']) == 1.0
    assert float(g['three_r__target'].max()) > 2.0            # values beyond the data range


def test_restatement_of_the_pixel_means():
    rng = np.random.default_rng(1)
    t = rng.random((2, 9, 11)).astype(np.float32)
    p = rng.random((2, 9, 11)).astype(np.float32)
    out = mr.image_metrics(p, t, 1.0)
    d = p.astype(np.float64) - t
    assert out['ssim'].shape == (2,)
    np.testing.assert_allclose(out['mse'], (d ** 2).reshape(2, -1).mean(1), rtol=1e-15)
    np.testing.assert_allclose(out['mae'], np.abs(d).reshape(2, -1).mean(1), rtol=1e-15)
    np.testing.assert_allclose(out['me'], d.reshape(2, -1).mean(1), rtol=1e-15)
    np.testing.assert_allclose(out['psnr'], -10 * np.log10(out['mse']), rtol=1e-15)
    with pytest.raises(ValueError, match='win_size'):
        mr.ssim(t[0, :6], p[0, :6], 1.0)


def _lib():
    import sunerf_hip
    return sunerf_hip.load()


def test_entry_points_are_bound():
    from sunerf_hip.lib import symbols
    assert 'sunerf_image_metrics' in symbols('core') and 'sunerf_image_metrics_workspace_bytes' in symbols('core')
    header = open(os.path.join(os.path.dirname(GOLDEN), '..', 'include', 'sunerf_hip.h')).read()
    assert '#define SUNERF_ABI_VERSION 9' in header


def test_workspace_size():
    lib = _lib()
    # one fp64 quadruple per 64 x 16 tile of every image
    assert lib.sunerf_image_metrics_workspace_bytes(1, 7, 7) == 32
    assert lib.sunerf_image_metrics_workspace_bytes(3, 16, 64) == 3 * 32
    assert lib.sunerf_image_metrics_workspace_bytes(7, 4096, 4096) == 7 * 256 * 64 * 32
    assert lib.sunerf_image_metrics_workspace_bytes(2, 17, 65) == 2 * 4 * 32
    assert lib.sunerf_image_metrics_workspace_bytes(0, 64, 64) == 0
    assert lib.sunerf_image_metrics_workspace_bytes(1, 6, 64) == 0
    assert lib.sunerf_image_metrics_workspace_bytes(1, 64, 6) == 0


def test_argument_errors_need_no_gpu():
    """Every check runs before a launch, so these return without a device (fake non-null addresses are never touched)."""
    lib = _lib()
    f = lib.sunerf_image_metrics
    fake = ctypes.c_void_p(4096)
    ws = lib.sunerf_image_metrics_workspace_bytes(2, 32, 40)

    def call(pred=fake, target=fake, n=2, h=32, w=40, r=1.0, out=fake, work=fake, nbytes=ws):
        return f(pred, target, n, h, w, r, out, work, nbytes, None)
    assert call(n=0) == 0
    assert call(n=0, pred=None, target=None, out=None, work=None) == 0
    for kw in ({'pred': None}, {'target': None}, {'out': None}, {'work': None}, {'h': 6}, {'w': 6}, {'h': 0}, {'n': -1},
               {'r': 0.0}, {'r': -1.0}, {'r': math.inf}, {'r': math.nan}, {'out': ctypes.c_void_p(4100)}):
        assert call(**kw) == BADARG, kw
    assert call(nbytes=ws - 1) == WORKSPACE
    assert call(nbytes=0) == WORKSPACE


def test_python_wrapper_refuses_without_launching():
    from sunerf_hip.lib import SunerfHipError
    from sunerf_hip.metrics import image_metrics
    a = torch.zeros(8, 8)
    with pytest.raises(ValueError, match='shape'):
        image_metrics(a, torch.zeros(8, 9), 1.0)
    with pytest.raises(SunerfHipError, match='ROCm'):
        image_metrics(a, a, 1.0)


def test_asinh_normalisation_restatement():
    x = np.array([-1., 0., 1e-4, 0.005, 0.1, 0.5, 1., 2., np.nan])
    got = mr.asinh_normalize(x)
    a = 0.005
    want = [np.arcsinh(min(max(v, 0.), 1.) / a) / np.arcsinh(1 / a) for v in x[:-1]]
    np.testing.assert_allclose(got[:-1], want, rtol=1e-15, atol=0)
    assert got[0] == 0 and got[1] == 0 and got[6] == 1 and got[7] == 1 and np.isnan(got[-1])
    # the module applies the same map in torch (fp64)
    from sunerf.model.sunerf import EmissionSuNeRFModule
    t = torch.tensor(x)
    fine, target = EmissionSuNeRFModule._validation_images(None, t, t)
    assert fine.dtype == torch.float64
    np.testing.assert_allclose(fine.numpy()[:-1], got[:-1], rtol=1e-15, atol=0)
    assert torch.isnan(fine[-1])


def test_callback_restatement_is_the_callbacks_formula():
    rng = np.random.default_rng(2)
    fine = rng.random((63, 2)).astype(np.float32)
    target = rng.random((63, 2)).astype(np.float32)
    dt = mr.callback_scores(fine, target, (7, 9), normalize=False)
    d = fine.astype(np.float64) - target
    assert dt['validation.loss'] == pytest.approx((d ** 2).mean(), rel=1e-15)
    assert dt['validation.psnr'] == pytest.approx(-10 * np.log10((d ** 2).mean()), rel=1e-15)
    assert dt['validation.ssim'] == mr.ssim(target.reshape(7, 9, 2)[..., 0], fine.reshape(7, 9, 2)[..., 0], 1.0)


def test_validation_metrics_without_outputs_is_none():
    from sunerf.model.sunerf import EmissionSuNeRFModule
    mod = EmissionSuNeRFModule(Rs_per_ds=1.0, seconds_per_dt=1.0, image_scaling_config={'vmax': 1.0, 'a': 0.005},
                               sampling_config={'type': 'stratified', 'n_samples': 8, 'perturb': False},
                               hierarchical_sampling_config={'type': 'hierarchical', 'n_samples': 8},
                               model_config={'d_filter': 64}, validation_dataset_mapping={0: 'test'})
    assert mod.validation_metrics((4, 4)) is None
    assert mod.validation_metrics((4, 4), name='test') is None
    mod.validation_epoch_end([{'fine_image': torch.zeros(16, 1), 'target_image': torch.zeros(16, 1)}])
    assert mod.validation_metrics((4, 4), name='other') is None
    with pytest.raises(ValueError, match='image_shape'):
        mod.validation_metrics((4, 5))


def test_correlation_on_host_tensors():
    from sunerf_hip.metrics import error_uncertainty_correlation
    x = torch.tensor([1., 2., 2., 3., 5.])
    y = torch.tensor([0., 0., 1., 1., 1.])
    out = error_uncertainty_correlation(x, y)
    assert out['pearson'].dtype == torch.float64
    np.testing.assert_allclose(out['pearson'].item(), np.corrcoef(x.numpy(), y.numpy())[0, 1], rtol=1e-14)
    # ranks with ties: x -> 1, 2.5, 2.5, 4, 5;  y -> 1.5, 1.5, 4, 4, 4
    rx, ry = np.array([1, 2.5, 2.5, 4, 5]), np.array([1.5, 1.5, 4, 4, 4])
    np.testing.assert_allclose(out['spearman'].item(), np.corrcoef(rx, ry)[0, 1], rtol=1e-14)
