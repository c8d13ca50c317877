"""CPU-only checks of the per-pixel DEM inversion (no GPU): the dual fixed point the device iterates on holds
for the ``nnls`` solution; a numpy restatement of the device's Newton iteration reaches ``nnls``; chi2(lam) is monotone;
the host helpers; the entry point is declared, bound and exported; its argument errors; CPU tensors and renderings without a
temperature are refused.

``test_newton_restatement_on_the_gpu_cases`` prints the worst agreement of the restatement with ``nnls`` on the very cases of
tests/test_gpu_dem_inversion.py: that figure x 16 (another summation order on the device), floored at 2^-22 (fp32 outputs),
is the GPU test's bound.  Measured here: 2.1e-11 of the pixel's largest node at worst (lam = 1e-4, K = 128, M = 8), at most 26
Newton steps.
"""
import os
import re

import numpy as np
import pytest
import torch

import dem_inversion_reference as ref
from conftest import load_golden

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope='session')
def lib():
    import sunerf_hip
    if not os.path.exists(sunerf_hip.LIB_PATH):
        import subprocess
        subprocess.check_call(['bash', os.path.join(ROOT, '2024-hl-spi3s-sunerf_amd', 'csrc', 'build.sh')])
    return sunerf_hip.load()


@pytest.fixture(scope='module')
def golden():
    return load_golden('g6_dt_e2e')


@pytest.fixture(scope='module')
def cases(golden):
    """64 generated pixels on the table's own grid, all seven channels."""
    return ref.make_cases(golden, 64, 7, 101, seed=7)


GRID = (1e-4, 1e-2, 1.0, 1e2, 1e4)


def test_nnls_solution_is_the_dual_fixed_point(cases):
    """x = max(0, P^2 G^T u / lam) with u = (y - G x) / sigma^2 holds for the nnls solution to 1e-9 of the pixel's largest node for
    lam >= 1 (measured: 3.0e-11 at lam = 1, 1.2e-13 above).  The map magnifies the rounding of x itself by |P^2 Gs^T Gs|_2 / lam --
    1e8 at lam = 1, 1e12 at lam = 1e-4 on these cases -- so below lam = 1 nnls, whose x carries its own solver's rounding, cannot
    be held to 1e-9: it gives 4.1e-9 at lam = 1e-2 and 5.6e-9 at 1e-4, and is held to 2e-8 there (four times its own figure: the
    reference's error, not the device's)."""
    c = cases
    for lam in GRID:
        worst, gain = 0.0, 0.0
        for i in range(0, 64, 4):
            x = ref.invert_reference(c['y'][i], c['sigma'][i], c['G'], c['prior'], lam)
            u = (c['y'][i] - c['G'] @ x) / c['sigma'][i] ** 2
            back = np.maximum(0.0, c['prior'] ** 2 * (c['G'].T @ u) / lam)
            worst = max(worst, np.abs(back - x).max() / x.max())
            gs = c['G'] / c['sigma'][i][:, None]
            gain = max(gain, np.linalg.norm((c['prior'] ** 2 / lam)[:, None] * (gs.T @ gs), 2))
        print(f'lam={lam:g}: dual fixed point of the nnls solution {worst:.2e} (gain of the map {gain:.1e})')
        assert worst <= (1e-9 if lam >= 1 else 2e-8)


def test_newton_restatement_reaches_nnls_and_chi2_is_monotone(cases):
    """The recommended iteration, restated in numpy, on 64 pixels for lam in {1e-4, 1e-2, 1, 1e2, 1e4}: within 1e-9 of the
    pixel's largest node, never at max_iter = 64; chi2(lam) non-decreasing over the grid for every pixel."""
    c = cases
    worst, most = 0.0, 0
    chi2 = np.zeros((len(GRID), 64))
    for j, lam in enumerate(GRID):
        for i in range(64):
            want = ref.invert_reference(c['y'][i], c['sigma'][i], c['G'], c['prior'], lam)
            x, _, it, ok = ref.newton_reference(c['y'][i], c['sigma'][i], c['G'], c['prior'], lam, tol=1e-10, max_iter=64)
            assert ok and it < 64, (lam, i, it)
            worst, most = max(worst, np.abs(x - want).max() / want.max()), max(most, it)
            chi2[j, i] = ref.chi2_of(want, c['y'][i], c['sigma'][i], c['G'])
    print(f'newton restatement vs nnls: {worst:.2e} of the largest node, at most {most} steps')
    assert worst <= 1e-9
    assert (np.diff(chi2, axis=0) >= -1e-9 * chi2[1:]).all()
    assert (chi2[-1] > chi2[0]).all()


@pytest.mark.parametrize('k,m', ref.CONFIGS)
def test_newton_restatement_on_the_gpu_cases(golden, k, m):
    """The same on the pools of the GPU test (every configuration, lam in {1e-4, 1, 1e4}): the figure its bound derives from."""
    c = ref.pool(golden, k, m)
    worst, most = 0.0, 0
    for lam in ref.LAMS:
        for i in range(ref.POOL):
            want = c['ref'][lam]['dem'][i]
            x, _, it, ok = ref.newton_reference(c['y'][i], c['sigma'][i], c['G'], c['prior'], lam, tol=1e-10, max_iter=64)
            assert ok and it < 64, (lam, i, it)
            assert want.max() > 0
            worst, most = max(worst, np.abs(x - want).max() / want.max()), max(most, it)
    print(f'K={k} M={m}: newton restatement vs nnls {worst:.2e} of the largest node, at most {most} steps')
    assert worst <= ref.HOST_WORST
    assert 16 * ref.HOST_WORST < 2.0 ** -22          # so the GPU test's bound is its floor, 2^-22


def test_left_out_channels_equal_the_smaller_problem(cases):
    """A NaN value and a zero error leave their channels out: the restatement (which keeps M and zeroes 1 / sigma, as the device
    does) equals nnls on the remaining channels."""
    c = cases
    y, s = c['y'][3].copy(), c['sigma'][3].copy()
    y[2], s[5] = np.nan, 0.0
    keep = [0, 1, 3, 4, 6]
    want = ref.invert_reference(c['y'][3][keep], c['sigma'][3][keep], c['G'][keep], c['prior'], 1.0)
    assert np.array_equal(ref.invert_reference(y, s, c['G'], c['prior'], 1.0), want)
    x, v, _, ok = ref.newton_reference(y, s, c['G'], c['prior'], 1.0)
    assert ok and v[2] == 0 and v[5] == 0 and np.abs(x - want).max() <= 1e-9 * want.max()
    assert ref.invert_reference(np.full(7, np.nan), s, c['G'], c['prior'], 1.0).max() == 0


def test_response_on_nodes(golden):
    from sunerf_hip.dem_inversion import response_on_nodes
    lt = golden['aia_logte']
    resp = (golden['aia_tresp'] * float(golden['aia_exp_time'])).float()
    same = response_on_nodes(lt, resp, lt[0])
    assert same.dtype == torch.float64 and same.shape == (7, 101)
    assert torch.equal(same, resp.double())                                  # the rows' bits on the table's own grid
    assert torch.equal(response_on_nodes(lt[0], resp, lt[0]), resp.double())  # one grid for all rows
    nodes = np.concatenate([[3.0, 3.99], np.linspace(4.0, 9.0, 37), [9.01, 12.0]])
    got = response_on_nodes(lt, resp, torch.from_numpy(nodes)).numpy()
    x = lt[0].double().numpy()
    want = np.stack([np.interp(nodes, x, r, left=0.0, right=0.0) for r in resp.double().numpy()])
    assert np.allclose(got, want, rtol=1e-12, atol=0)
    assert (got[:, :2] == 0).all() and (got[:, -2:] == 0).all() and (got[:, 2:-2] > 0).any()
    with pytest.raises(ValueError):
        response_on_nodes(lt[:, :50], resp, lt[0])


def test_default_errors_and_flat_prior():
    from sunerf_hip.dem_inversion import default_errors, flat_prior
    y = torch.tensor([[[1.0, -4.0], [3.0, float('nan')]], [[float('inf'), 2.0], [0.0, 1.0]]])
    s = default_errors(y)
    assert s.shape == y.shape
    top = torch.tensor([3.0, 2.0])
    want = 0.05 * y.abs() + 1e-3 * top
    assert torch.equal(s[0, 0], want[0, 0]) and torch.equal(s[1, 1], want[1, 1]) and s[0, 1, 0] == want[0, 1, 0]
    assert torch.isnan(s[0, 1, 1]) and torch.isinf(s[1, 0, 0])
    s2 = default_errors(y, relative=0.1, floor_fraction=0.5)
    assert s2[1, 1, 0] == 0.5 * 3.0 and s2[1, 1, 1] == pytest.approx(0.1 + 0.5 * 2.0)
    assert 'ONLY' in default_errors.__doc__
    G = torch.tensor([[1.0, 1.0, 2.0], [0.5, 0.25, 0.25]], dtype=torch.float64)
    p = flat_prior(y, G)
    ratios = np.array([1 / 4, -4.0, 3 / 4, 2.0, 0.0, 1.0])      # the finite y_w / sum_k G[w, k]
    assert p.shape == (3,) and p.dtype == torch.float64 and float(p[0]) == np.sort(ratios)[2]    # torch's lower median
    assert float(flat_prior(-y.abs(), G)[0]) == 1.0


def test_entry_point_is_declared_bound_and_exported(lib):
    import sunerf_hip
    header = open(os.path.join(ROOT, 'include', 'sunerf_hip.h')).read()
    declared = set(re.findall(r'\b(sunerf_\w+)\s*\(', header))
    assert 'sunerf_dem_invert' in declared
    assert 'sunerf_dem_invert' in sunerf_hip.symbols('core')
    assert getattr(lib, 'sunerf_dem_invert') is not None
    assert 'DESIGN.md 8k' in header and 'density_temperature.py:237-265' in header
    assert lib.sunerf_abi_version() == 9
    build = open(os.path.join(ROOT, '2024-hl-spi3s-sunerf_amd', 'csrc', 'build.sh')).read()
    assert 'dem_inversion' in build


def test_argument_errors_without_gpu(lib):
    """Sizes first (n_nodes < 2, n_channels < 1, n_bisect < 0, max_iter < 1: -1; n_nodes > 128, n_channels > 8: -2), then the
    empty batch (0), then values and null pointers (-1); all before anything touches a device."""
    def call(n_nodes=101, n_channels=7, n=4, n_bisect=20, max_iter=64, discrepancy=1, lam_min=1e-4, lam_max=1e4, tol=1e-10):
        return lib.sunerf_dem_invert(None, None, None, None, None, None, 0, discrepancy, -1.0, lam_min, lam_max, n_bisect, tol,
                                     max_iter, n, n_channels, n_nodes, None, None, None, None, None, None, None)
    assert call() == -1 and call(discrepancy=0) == -1                     # null pointers
    assert call(n_nodes=1) == -1 and call(n_nodes=1, n=0) == -1
    assert call(n_channels=0) == -1 and call(n_channels=0, n=0) == -1
    assert call(n_bisect=-1) == -1 and call(n_bisect=-1, n=0) == -1
    assert call(max_iter=0) == -1 and call(max_iter=0, n=0) == -1
    assert call(n_nodes=129) == -2 and call(n_nodes=129, n=0) == -2
    assert call(n_channels=9) == -2 and call(n_channels=9, n=0) == -2
    assert call(n_nodes=1, n_channels=9) == -1                            # -1 sizes before -2
    assert call(n_nodes=128, n_channels=8) == -1 and call(n_nodes=2, n_channels=1) == -1     # supported: the null pointers
    assert call(n=0) == 0 and call(n=0, n_nodes=2, n_channels=1, n_bisect=0, max_iter=1) == 0
    assert call(n=-1) == -1
    # values come after the empty batch, with the null pointers (tests/test_gpu_dem_inversion.py gives them real pointers)
    assert call(n=0, lam_min=0.0) == 0 and call(n=0, lam_min=2.0, lam_max=1.0) == 0 and call(n=0, tol=-1.0) == 0


def test_python_op_refuses_cpu_tensors_and_bad_arguments():
    from sunerf_hip import SunerfHipError
    from sunerf_hip.dem_inversion import invert_dem
    y, G, nodes = torch.ones(4, 5, 7), torch.ones(7, 11, dtype=torch.float64), torch.linspace(5, 7, 11)
    with pytest.raises(SunerfHipError):
        invert_dem(y, G, nodes)
    with pytest.raises(SunerfHipError):
        invert_dem(y, G, nodes, lam=1.0)
    with pytest.raises(ValueError, match='unknown outputs'):
        invert_dem(y, G, nodes, want=('dem', 'temperature'))
    with pytest.raises(ValueError, match='1-d'):
        invert_dem(y, G, nodes[None])
    with pytest.raises(ValueError, match='tile_pixels'):
        invert_dem(y, G, nodes, tile_pixels=0)


def _emission_module():
    from sunerf.rendering.emission import EmissionRadiativeTransfer
    return EmissionRadiativeTransfer(Rs_per_ds=1.0, sampling_config={'type': 'stratified', 'n_samples': 8, 'perturb': False},
                                     hierarchical_sampling_config={'type': 'hierarchical', 'n_samples': 8},
                                     model_config={'d_filter': 64})


def test_loaders_refuse_a_rendering_without_a_temperature():
    import datetime
    from sunerf.evaluation.loader import ModelLoader, SuNeRFLoader
    mod = _emission_module()
    loader = ModelLoader(rendering=mod, model=mod.fine_model, device='cpu',
                         ref_map={'shape': (4, 4), 'cdelt': (600., 600.), 'meta': {'t_obs': '2022-01-01T00:00:00.000'}})
    frame = np.ones((4, 4, 7), dtype=np.float32)
    with pytest.raises(TypeError, match='density-temperature'):
        loader.invert_dem_image(frame)
    snf = SuNeRFLoader.__new__(SuNeRFLoader)
    snf.rendering, snf.device, snf.seconds_per_dt, snf.ref_time = mod, torch.device('cpu'), 86400., datetime.datetime(2022, 1, 1)
    with pytest.raises(TypeError, match='density-temperature'):
        snf.invert_dem_image(torch.ones(4, 4, 7))


def test_model_method_builds_the_response_and_refuses_unknown_channels(golden):
    from sunerf.model.model import NeRF_DT
    from sunerf.rendering.density_temperature import DensityTemperatureRadiativeTransfer
    from sunerf_hip import SunerfHipError
    g = golden
    mod = DensityTemperatureRadiativeTransfer(
        Rs_per_ds=1.0, sampling_config={'type': 'stratified', 'n_samples': 8, 'perturb': False},
        hierarchical_sampling_config={'type': 'hierarchical', 'n_samples': 8}, model_config={'d_filter': 64}, model=NeRF_DT,
        device=torch.device('cpu'), pixel_intensity_factor=1e17, response_table=(g['aia_logte'].numpy(), g['aia_tresp'].numpy()))
    with torch.no_grad():
        mod.fine_model.volumetric_constant.fill_(0.5)
    G = mod.inversion_response()
    assert G.shape == (7, 101) and G.dtype == torch.float64
    assert torch.equal(G, mod.response_table.double() * (torch.tensor(0.5, dtype=torch.float64) * 1e17))
    G2 = mod.inversion_response(wavelengths=(193, 94), logt_nodes=torch.linspace(5.5, 7.5, 21))
    assert G2.shape == (2, 21) and bool((G2 > 0).all())
    assert mod.channel_indices((193, 94)) == [3, 0] and mod.channel_indices() == list(range(7))
    for bad in (1600, 171.5, 'hot'):
        with pytest.raises(ValueError, match='not a channel'):
            mod.invert_dem(torch.ones(4, 1), wavelengths=(bad,))
    with pytest.raises(ValueError, match='one value per channel'):
        mod.invert_dem(torch.ones(4, 6))
    with pytest.raises(SunerfHipError):
        mod.invert_dem(torch.ones(4, 7))
    assert 'OPTICALLY THIN' in mod.invert_dem.__doc__
