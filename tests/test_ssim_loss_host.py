"""CPU-only checks of the structural loss (no GPU): the restatement tests/ssim_loss_reference.py against
tests/metrics_reference.py (which tests/test_metrics_host.py ties to scikit-image's own output) and against central finite
differences; invalid planes; the eighth entry-point table (declared, bound, kept out of the other seven, its argument checks in
their documented order); the validation of both Lightning modules.

Gate of the finite differences: 1e-6 of the plane's largest gradient element, at a step of 1e-6.  The differences are taken of an
extended-precision evaluation of the same definition (``_ssim_extended``: numpy's longdouble, 64 bits of mantissa on x86), so
what is left is the truncation error h^2 f''' / 6, far inside the gate for planes whose values stay 0.02 or more from 0 (the
stretch's third derivative grows like 1 / v^3), while a wrong coefficient is an error of order one."""
import ctypes
import os

import numpy as np
import pytest

import metrics_reference as mr
import ssim_loss_reference as sr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FD_GATE, FD_STEP = 1e-6, 1e-6
ASINH = (1.0, 0.005)


@pytest.fixture(scope='session')
def lib():
    import sunerf_hip
    if not os.path.exists(sunerf_hip.LIB_PATH):
        import subprocess
        subprocess.check_call(['bash', os.path.join(ROOT, '2024-hl-spi3s-sunerf_amd', 'csrc', 'build.sh')])
    return sunerf_hip.load()


def _pair(P, kind, seed):
    rng = np.random.default_rng([seed, P])
    target = sr.make_plane(P, kind, rng).astype(np.float64)
    pred = target * rng.uniform(0.8, 1.2) + 0.05 * rng.uniform(-1, 1, target.shape) * target
    return pred, target


def _ssim_extended(pred, target, w, data_range, scaling):
    """The SSIM of one plane from the definitions in extended precision (numpy's longdouble), with centred second moments: what
    the central differences are taken of.  In fp64 the raw-moment form of the variance leaves 1e-14 of rounding in the value of a
    smooth stretched plane, which a step of 1e-6 turns into 1e-8 of noise in the difference -- more than the gate at P = w."""
    ld = np.longdouble
    x, y = np.asarray(pred, dtype=ld), np.asarray(target, dtype=ld)
    if scaling is not None:
        vmax, a = ld(scaling[0]), ld(scaling[1])
        x, y = np.arcsinh(x / vmax / a) / np.arcsinh(1 / a), np.arcsinh(y / vmax / a) / np.arcsinh(1 / a)
    c1, c2 = (ld(0.01) * ld(data_range)) ** 2, (ld(0.03) * ld(data_range)) ** 2
    n = x.shape[0] - w + 1
    total = ld(0)
    for i in range(n):
        for j in range(n):
            u, v = x[i:i + w, j:j + w], y[i:i + w, j:j + w]
            mu, mv = u.mean(), v.mean()
            du, dv = u - mu, v - mv
            var_u, var_v, cov = (du * du).sum() / (w * w - 1), (dv * dv).sum() / (w * w - 1), (du * dv).sum() / (w * w - 1)
            total += (2 * mu * mv + c1) * (2 * cov + c2) / ((mu * mu + mv * mv + c1) * (var_u + var_v + c2))
    return total / (n * n)


# ---- 1. the restatement -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('kind', sr.KINDS)
@pytest.mark.parametrize('P', [7, 8, 16])
def test_restatement_equals_the_metrics_reference_at_window_7(P, kind):
    pred, target = _pair(P, kind, 1)
    for data_range in (1.0, 2.5):
        got, want = sr.ssim(pred, target, 7, data_range), mr.ssim(target, pred, data_range)
        print(f'P {P} {kind} R {data_range}: ssim {got:.15f}, metrics_reference {want:.15f}, difference {abs(got - want):.2e} (bound 1e-13)')
        assert abs(got - want) <= 1e-13
        assert abs(got) < 1.0
    assert sr.ssim(target, target, 7, 1.0) == 1.0


@pytest.mark.parametrize('stretched', [False, True], ids=['plain', 'asinh'])
@pytest.mark.parametrize('w', [3, 7, 11])
def test_restatement_gradient_equals_central_differences(w, stretched):
    scaling = ASINH if stretched else None
    worst = 0.0
    for P in (w, w + 1, w + 5):          # one window, four windows, 36 windows
        for kind in sr.KINDS:
            pred, target = _pair(P, kind, 2)
            value, grad = sr.ssim_and_gradient(pred, target, w, 1.0, scaling)
            assert abs(value - sr.ssim(pred, target, w, 1.0, scaling)) == 0.0
            assert abs(value - float(_ssim_extended(pred, target, w, 1.0, scaling))) <= 1e-12
            fd = np.zeros_like(grad)
            for r in range(P):
                for q in range(P):
                    step = np.zeros_like(pred)
                    step[r, q] = FD_STEP
                    fd[r, q] = float(_ssim_extended(pred + step, target, w, 1.0, scaling)
                                     - _ssim_extended(pred - step, target, w, 1.0, scaling)) / (2 * FD_STEP)
            rel = float(np.abs(fd - grad).max() / np.abs(grad).max())
            worst = max(worst, rel)
            assert np.abs(grad).max() > 0 and rel <= FD_GATE, (P, kind, rel)
    print(f'window {w}, {"asinh" if stretched else "no"} stretch: largest |fd - closed form| = {worst:.3g} of max|g| (gate {FD_GATE})')


def test_an_invalid_plane_contributes_nothing_and_no_valid_plane_gives_zero():
    n, P, C = 3, 8, 2
    coarse, fine, target = sr.make_case(n, P, C, 5)
    whole = sr.evaluate(coarse, fine, target, n, P)
    assert whole['stats'][2] == 2 * n * C and whole['stats'][3] == 0
    poisoned = [v.copy() for v in (coarse, fine, target)]
    poisoned[0].reshape(n, P, P, C)[1, 3, 4, 0] = np.nan          # coarse plane (1, 0) only
    poisoned[2].reshape(n, P, P, C)[2, 0, 0, 1] = np.inf          # target plane (2, 1): coarse and fine
    out = sr.evaluate(*poisoned, n, P)
    assert out['stats'][2] == 2 * n * C - 3 and out['stats'][3] == 3 and out['counts'].tolist() == [n * C - 2, n * C - 1]
    keep = np.ones((2, n, C), dtype=bool)
    keep[0, 1, 0] = keep[0, 2, 1] = keep[1, 2, 1] = False
    assert np.array_equal(np.isfinite(out['plane_ssim']), keep)
    assert np.array_equal(out['plane_ssim'][keep], whole['plane_ssim'][keep])
    for i in range(2):
        assert out['stats'][i] == 1.0 - whole['plane_ssim'][i][keep[i]].sum() / keep[i].sum()
    g = out['g_coarse'].reshape(n, P, P, C)
    assert not g[1, :, :, 0].any() and not g[2, :, :, 1].any() and np.isfinite(g).all() and g[0].any()
    assert not out['g_fine'].reshape(n, P, P, C)[2, :, :, 1].any() and out['g_fine'].reshape(n, P, P, C)[1, :, :, 0].any()
    poisoned[2][:] = np.nan
    none = sr.evaluate(*poisoned, n, P)
    assert none['loss'] == 0.0 and none['stats'].tolist() == [0.0, 0.0, 0.0, float(2 * n * C)]
    assert not none['g_coarse'].any() and not none['d_coarse'].any() and not none['d_fine'].any()


# ---- 2. the eighth table ----------------------------------------------------------------------------------------------------------
def test_entry_points_are_declared_bound_and_kept_out_of_the_other_tables(lib):
    """(The table itself -- declared, bound, frozen, versioned, built, its symbols in no other table or older header:
    tests/test_abi_tables_host.py.)"""
    import sunerf_hip
    header = open(os.path.join(ROOT, 'include', 'sunerf_hip_ssim_loss.h')).read()
    assert lib.sunerf_abi_version() == 9 and lib.sunerf_ext_abi_version() == 1 and lib.sunerf_response_abi_version() == 1
    assert lib.sunerf_prep_abi_version() == 1 and lib.sunerf_instrument_abi_version() == 1 and lib.sunerf_patch_abi_version() == 1
    assert lib.sunerf_likelihood_abi_version() == 1
    assert lib.sunerf_ssim_loss_abi_version() == 1
    assert '#define SUNERF_SSIM_LOSS_MAX_PATCH 64' in header
    assert callable(sunerf_hip.ssim_loss) and callable(sunerf_hip.patch_ssim)
    # the workspace query: a ticket line and 4 words per patch and channel; nothing for no patch or outside 1 .. 64 channels
    assert [lib.sunerf_ssim_loss_workspace_bytes(n, c) for n, c in ((0, 1), (1, 1), (65, 7), (4, 64), (4, 65), (4, 0), (-1, 1))] \
        == [0, 64 + 32, 64 + 65 * 7 * 32, 64 + 4 * 64 * 32, 0, 0, 0]


def check_argument_order(lib):
    """Limits (-2) first, then the empty call (0), then a negative count and null pointers (-1), then the workspace (-3): all
    before anything touches a device, so this runs without one.  ``Q`` stands for any non-null pointer: no call here reaches a
    launch."""
    Q = ctypes.c_void_p(4096)
    fn = lib.sunerf_ssim_loss

    def call(n=4, P=16, C=3, w=7, R=1.0, vmax=1.0, a=0.005, use_asinh=0, ptrs=None, ws_bytes=1 << 20):
        p = [Q] * 8 if ptrs is None else ptrs
        return fn(p[0], p[1], p[2], n, P, C, w, R, vmax, a, use_asinh, p[3], p[4], p[5], p[6], p[7], ws_bytes, None)
    none = [None] * 8
    for w in (1, 2, 4, 6, 8, 10, 12, 13, 0, -7):
        assert call(w=w, P=16, ptrs=none) == -2, w
    assert call(P=6, ptrs=none) == -2 and call(P=65, ptrs=none) == -2 and call(w=11, P=10, ptrs=none) == -2
    assert call(C=0, ptrs=none) == -2 and call(C=65, ptrs=none) == -2
    for R in (0.0, -1.0, float('inf'), float('nan')):
        assert call(R=R, ptrs=none) == -2, R
    assert call(use_asinh=1, a=0.0, ptrs=none) == -2 and call(use_asinh=1, vmax=float('nan'), ptrs=none) == -2
    assert call(use_asinh=0, a=0.0, vmax=-1.0, ws_bytes=0) == -3          # the stretch constants are not looked at when it is off
    assert call(n=0, w=4, ptrs=none) == -2 and call(n=-1, P=65, ptrs=none) == -2          # the limits come first
    assert call(n=0, ptrs=none, ws_bytes=0) == 0 and call(n=0, P=64, C=64, w=11, ptrs=none, ws_bytes=0) == 0
    assert call(n=-1) == -1 and call(n=1 << 40, C=64) == -1
    for k in range(8):
        ptrs = [Q] * 8
        ptrs[k] = None
        assert call(ptrs=ptrs) == -1 and call(ptrs=ptrs, ws_bytes=0) == -1, k          # a null pointer before the workspace
    for k in (5, 6, 7):                                                                # plane_ssim, stats, workspace
        ptrs = [Q] * 8
        ptrs[k] = ctypes.c_void_p(4100)
        assert call(ptrs=ptrs) == -1, k
    assert call(P=3, w=3, C=1, n=1, ws_bytes=64 + 32 - 1) == -3 and call(ws_bytes=0) == -3
    assert call(ws_bytes=lib.sunerf_ssim_loss_workspace_bytes(4, 3) - 1) == -3


def test_argument_checks_come_in_the_documented_order(lib):
    check_argument_order(lib)


# ---- 3. the Lightning modules -----------------------------------------------------------------------------------------------------
def _emission(**kwargs):
    from sunerf.model.sunerf import EmissionSuNeRFModule
    return EmissionSuNeRFModule(Rs_per_ds=1.0, seconds_per_dt=1.0, image_scaling_config={'vmax': 1, 'a': 0.005},
                                sampling_config={'type': 'stratified', 'n_samples': 8, 'perturb': False},
                                hierarchical_sampling_config={'type': 'hierarchical', 'n_samples': 8}, model_config={'d_filter': 64},
                                **kwargs)


def _density_temperature(**kwargs):
    from conftest import load_golden
    from sunerf.model.model import NeRF_DT
    from sunerf.model.sunerf import DensityTemperatureSuNeRFModule
    g = load_golden('g6_dt_e2e')
    return DensityTemperatureSuNeRFModule(
        Rs_per_ds=1.0, seconds_per_dt=1.0, image_scaling_config={}, model=NeRF_DT,
        sampling_config={'type': 'stratified', 'n_samples': 16, 'perturb': False},
        hierarchical_sampling_config={'type': 'hierarchical', 'n_samples': 16}, model_config={'d_filter': 64},
        pixel_intensity_factor=float(g['pixel_intensity_factor']),
        response_table=(g['aia_logte'].numpy(), g['aia_tresp'].numpy()), **kwargs)


def test_lightning_modules_validate_the_structural_term():
    import torch
    from sunerf_hip.instrument import Instrument
    from sunerf_hip.likelihood import NoiseLikelihood
    plain = _emission()
    assert plain.lambda_ssim == 0.0 and plain.ssim_window == 7 and plain.last_ssim is None
    mod = _emission(lambda_ssim=0.5, ssim_window=5)
    assert mod._ssim_scaling() == (1.0, (1.0, float(np.float32(0.005))))          # the scaling's buffers are fp32
    dt = _density_temperature()
    assert dt.lambda_ssim == 0.0 and dt.ssim_window == 7 and dt.ssim_data_range is None
    assert _density_temperature(lambda_ssim=0.5, ssim_data_range=3.0)._ssim_scaling() == (3.0, None)
    with pytest.raises(ValueError, match='ssim_data_range'):
        _density_temperature(lambda_ssim=0.5)
    for window in (4, 13, 1):
        with pytest.raises(ValueError, match='window'):
            _emission(ssim_window=window)
    with pytest.raises(ValueError, match='lambda_ssim'):
        _emission(lambda_ssim=-1.0)
    free = NoiseLikelihood(Instrument(read_noise=1.0), free='all')
    with pytest.raises(ValueError, match='free gains'):
        _emission(lambda_ssim=0.5, likelihood=free)
    assert _emission(lambda_ssim=0.0, likelihood=free).likelihood is free                                  # the term is off: allowed
    assert _emission(lambda_ssim=0.5, likelihood=NoiseLikelihood(Instrument(read_noise=1.0))).lambda_ssim == 0.5      # frozen gains
    # patches smaller than the window: refused before anything is rendered (so it shows without a device)
    tracing = {'rays': torch.zeros(1, 6, 6, 2, 3), 'time': torch.zeros(36, 1), 'target_image': torch.zeros(1, 1, 4, 4),
               'patch': {'n': 1, 'C': 1, 'P': 4, 'hw': 6, 'ww': 6, 'instrument': None}}
    with pytest.raises(ValueError, match='smaller than ssim_window'):
        _emission(lambda_ssim=0.5).training_step({'tracing': tracing}, 0)
    tracing['wavelength'] = torch.zeros(36, 1)
    with pytest.raises(ValueError, match='smaller than ssim_window'):
        _density_temperature(lambda_ssim=0.5, ssim_data_range=1.0).training_step({'tracing': tracing}, 0)
