"""Host side of tests/test_gpu_emission_integral.py: the float64 yardstick of the emission integral
(sunerf_oracle.emission_outputs) and the case generator, both without a GPU."""
import pytest
import torch

import sunerf_oracle as orc
import test_gpu_emission_integral as emi


def test_emission_outputs_fp32_is_the_oracle():
    """In fp32 emission_outputs is emission_integral plus the epilogue expressions of render_emission, bit for bit."""
    c = emi.make_case(9, 70, seed=1)
    raw, z, o, d = c['raw'], c['z'], c['o'], c['d']
    got = orc.emission_outputs(raw, z, o, d, 1.2)
    want = orc.emission_integral(raw, z, d)
    pts = orc.points_on_rays(o, d, z)
    dist_pts = pts.pow(2).sum(-1).pow(0.5)
    absorption = want['regularizing_quantity']
    want.update(points=pts, height_map=(want['weights'] * dist_pts).sum(-1), absorption_map=(1 - absorption).sum(-1),
                regularization=torch.relu(dist_pts - 1.2) * (1 - absorption))
    assert set(got) == set(want)
    for k in want:
        assert got[k].dtype == torch.float32, k
        assert torch.equal(got[k], want[k]), k


def test_emission_outputs_fp64_differentiates_raw():
    """float64 raw: every output in float64 (points formed in fp32, then promoted) and differentiable w.r.t. raw."""
    c = emi.make_case(7, 33, seed=2)
    raw = c['raw'].double().requires_grad_(True)
    out = orc.emission_outputs(raw, c['z'], c['o'], c['d'], 1.0)
    assert all(v.dtype == torch.float64 for v in out.values())
    assert torch.equal(out['points'], orc.points_on_rays(c['o'], c['d'], c['z']).double())
    (out['image'].sum() + out['regularization'].sum()).backward()
    assert raw.grad is not None and bool(torch.isfinite(raw.grad).all())


CASES = [(n, s) for s in emi.S_VALUES for n in (1, 7, 8, 9)]


@pytest.mark.parametrize('n, s', CASES)
def test_emission_cases_contain_their_regimes(n, s):
    """Every case of the GPU test contains each regime it claims: exact +-0 r1, duplicate z, tau >= 104 (across the chunk seam
    at 32 for S > 32), a transmittance that reaches 0 in fp32, sum em < 1e-10, tau ~ 23, ..."""
    c = emi.make_case(n, s, seed=s * 10 + n)
    want = emi.claims(c)
    assert want <= emi.regimes_found(c), sorted(want - emi.regimes_found(c))


def test_emission_cases_are_deterministic():
    a, b = emi.make_case(9, 65, seed=3), emi.make_case(9, 65, seed=3)
    for k in ('raw', 'z', 'o', 'd'):
        assert torch.equal(a[k], b[k]), k
    assert bool((a['d'].norm(dim=-1) >= 0.25 * (1 - 1e-6)).all()) and bool((a['d'].norm(dim=-1) <= 4 * (1 + 1e-6)).all())
    assert bool((a['z'] >= 213.7).all()) and bool((a['z'] <= 216.3).all())
