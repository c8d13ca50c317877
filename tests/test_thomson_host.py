"""White-light Thomson scattering without a GPU: the mirror of thompson.py (constructor, buffers, state dict, pickling,
refusals), the argument errors of the two C entry points, and the physics of the fp64 restatement the GPU tests check the
kernels against (tests/thomson_reference.py)."""
import ctypes
import io
import math
import os
import pickle

import pytest
import torch

import thomson_reference as tr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _module(**kw):
    from sunerf.rendering.thompson import ThompsonScattering
    args = dict(Rs_per_ds=0.25, sampling_config={'type': 'stratified', 'n_samples': 8, 'perturb': False},
                hierarchical_sampling_config={'type': 'hierarchical', 'n_samples': 8}, model_config={'d_filter': 64})
    args.update(kw)
    return ThompsonScattering(**args)


def test_thompson_scattering_is_importable():
    from sunerf.rendering.thompson import ThompsonScattering
    from sunerf.rendering.base_tracing import SuNeRFRendering
    assert issubclass(ThompsonScattering, SuNeRFRendering)


def test_constructor_passes_rs_per_ds_and_pops_type():
    sampling = {'type': 'stratified', 'n_samples': 8, 'perturb': False}
    hier = {'type': 'hierarchical', 'n_samples': 8}
    mod = _module(Rs_per_ds=0.25, sampling_config=sampling, hierarchical_sampling_config=hier)
    assert mod.Rs_per_ds == 0.25
    assert 'type' not in sampling and 'type' not in hier          # popped from the caller's dicts, as the reference does
    assert mod.sampler.solar_R.item() == 4.0                       # the sampler got it too
    assert mod.coarse_model.out_layer.weight.shape[1] == 64
    assert mod.limb_darkening_coeff.dtype == torch.float32 and mod.limb_darkening_coeff.item() == pytest.approx(0.63)
    assert mod.C_0.item() == 1.0 and mod.C_0.dtype == torch.float32
    assert mod.solar_radius.item() == float(torch.tensor(4.0))     # 1 / Rs_per_ds in fp32
    assert mod.solar_radius.shape == () and mod.limb_darkening_coeff.shape == () and mod.C_0.shape == ()


def test_state_dict_accepts_the_references_keys():
    mod = _module()
    sd = mod.state_dict()
    for k in ('limb_darkening_coeff', 'C_0', 'solar_radius'):
        assert k in sd
    ref_keys = {k: v.clone() for k, v in sd.items()}
    ref_keys['solar_radius'] = torch.tensor(0.5)
    other = _module()
    other.load_state_dict(ref_keys, strict=True)
    assert other.solar_radius.item() == 0.5


def test_wavelengths_are_refused():
    mod = _module()
    o, d = torch.zeros(2, 3), torch.ones(2, 3)
    with pytest.raises(ValueError, match='wavelengths'):
        mod(o, d, torch.zeros(2, 1), wavelengths=torch.ones(2, 1))


def test_module_pickles_with_its_buffers():
    mod = _module()
    with torch.no_grad():
        mod.limb_darkening_coeff.fill_(0.5)
    buf = io.BytesIO()
    torch.save(mod, buf)
    buf.seek(0)
    back = torch.load(buf, weights_only=False)
    assert type(back).__name__ == 'ThompsonScattering'
    assert back.limb_darkening_coeff.item() == 0.5 and back.solar_radius.item() == 4.0
    assert all(not t.is_cuda for t in back.state_dict().values())
    assert pickle.loads(pickle.dumps(mod)).Rs_per_ds == 0.25


def test_field_modules_take_natural_log_density():
    from sunerf.model.stellar_model import SimpleStar
    from sunerf.rendering.functional import LN10
    assert _module()._kappa() == LN10
    assert _module(model=SimpleStar, model_config={})._kappa() == 1.0


@pytest.fixture(scope='module')
def lib():
    import sunerf_hip
    if not os.path.exists(sunerf_hip.LIB_PATH):
        import subprocess
        subprocess.check_call(['bash', os.path.join(ROOT, '2024-hl-spi3s-sunerf_amd', 'csrc', 'build.sh')])
    return sunerf_hip.load()


def test_entry_points_return_argument_errors_without_gpu(lib):
    import sunerf_hip
    assert 'sunerf_thomson_integral_fwd' in sunerf_hip.symbols('core')
    assert 'sunerf_thomson_integral_bwd' in sunerf_hip.symbols('core')
    assert lib.sunerf_abi_version() == 9
    fake = ctypes.c_void_p(16)            # never dereferenced: every call below fails its argument check first
    fwd, bwd = lib.sunerf_thomson_integral_fwd, lib.sunerf_thomson_integral_bwd
    ins = [fake, 2, 1.0, fake, fake, fake, fake, fake, fake]
    outs = [fake] * 5
    # null inputs / outputs
    assert fwd(None, 2, 1.0, fake, fake, fake, fake, fake, fake, 4, 8, *outs, None) == -1
    assert fwd(*ins[:6], None, fake, fake, 4, 8, *outs, None) == -1
    assert fwd(*ins, 4, 8, fake, fake, None, fake, fake, None) == -1
    # sample count, ray count, channel count
    assert fwd(*ins, 4, 0, *outs, None) == -1
    assert fwd(*ins, -1, 8, *outs, None) == -1
    assert fwd(fake, 3, 1.0, *ins[3:], 4, 8, *outs, None) == -1
    assert fwd(fake, 0, 1.0, *ins[3:], 4, 8, *outs, None) == -1
    # the backward: no g_raw, bad shapes
    assert bwd(*ins, 4, 8, None, None, None, None, None, None, None, None) == -1
    assert bwd(*ins, 4, 0, None, None, None, None, None, fake, None, None) == -1
    assert bwd(None, 2, 1.0, *ins[3:], 4, 8, None, None, None, None, None, fake, None, None) == -1
    # an empty batch is not an error (nothing is launched, nothing to clear)
    assert fwd(None, 2, 1.0, None, None, None, fake, fake, fake, 0, 8, None, None, None, None, None, None) == 0


# ---- the fp64 restatement: limits of the geometry --------------------------------------------------------------------------
def test_geometry_at_the_limb():
    s = torch.tensor([1 - 1e-12], dtype=torch.float64)
    A, B, C, D = tr.geometry_factors(s)
    assert abs(A.item()) < 1e-5
    assert B.item() == pytest.approx(0.25, abs=1e-5)
    assert C.item() == pytest.approx(4 / 3, abs=1e-5)
    assert D.item() == pytest.approx(0.75, abs=1e-5)


def test_geometry_far_from_the_sun_is_the_point_source_law():
    s = torch.tensor([1e-2, 3e-3, 1 / 215.], dtype=torch.float64)
    A, B, C, D = tr.geometry_factors(s)
    s2 = s * s
    for got, want in ((A / s2, 1.), (C / s2, 1.), (B / s2, 2 / 3), (D / s2, 2 / 3)):
        assert torch.allclose(got, torch.full_like(got, want), rtol=2e-4), (got, want)


def test_point_source_brightness_without_limb_darkening():
    """u = 0 far out: tB per electron ~ (R/r)^2 (1 + cos^2 chi), pB ~ (R/r)^2 sin^2 chi (Thomson's dipole law)."""
    r = torch.tensor([[100.]], dtype=torch.float64)
    # ray o = (100, -b... ): a sample at r = 100 with impact parameter p = 60 -> sin chi = 0.6
    o = torch.tensor([[60., -200., 0.]])
    d = torch.tensor([[0., 1., 0.]])
    z = torch.tensor([[200. - 80., 200. - 80. + 1e-3]])
    raw = torch.zeros(1, 2, 1)
    out = tr.thomson_integral(raw, z, o, d, 1.0, limb=0.0)
    s2 = 1 / r.item() ** 2
    ds = 1e-3
    sin2 = 0.36
    tb, pb = out['pixel_B'][0, 0].item(), out['pixel_B'][0, 1].item()
    assert tb / (2 * ds) == pytest.approx(s2 * (1 + (1 - sin2)), rel=1e-3)
    assert pb / (2 * ds) == pytest.approx(s2 * sin2, rel=1e-3)


def test_literal_fp32_drifts_where_the_fp64_form_does_not():
    n, s = 4, 64
    o = torch.tensor([[215., 0., 0.]]).repeat(n, 1)
    d = torch.tensor([[-1., 0.3, 0.], [-1., 0.1, 0.], [-1., 0.5, 0.2], [-1., 0.9, 0.1]])
    d = d / d.norm(dim=-1, keepdim=True)
    z = torch.linspace(0., 160., s).repeat(n, 1)
    raw = torch.randn(n, s, 2, generator=torch.Generator().manual_seed(0))
    ref = tr.thomson_integral(raw, z, o, d, math.log(10.))['pixel_B']
    lit = tr.thomson_literal_fp32(raw, z, o, d).double()
    assert ((lit - ref).abs() / ref.abs()).max() > 1e-3        # far above the 1e-4 gate
