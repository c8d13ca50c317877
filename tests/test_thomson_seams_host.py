"""The seam cases of the white-light Thomson integral without a GPU (tests/thomson_reference.py): that the constructions put
their sample on the limb by bits or on the intended side of it, that the fp64 restatement masks them as intended and stays
finite on degenerate rays, and how much of the parity gate the restatement's own rounding takes at the limb, measured against
a cancellation-free evaluation in long double."""
import numpy as np
import pytest
import torch

import thomson_reference as tr

RADII = [1.0, 4.0, 0.5, float(np.float32(1 / 0.7))]
LIMBS = [0.0, 0.63, 1.0]
LIMB32 = [float(np.float32(u)) for u in LIMBS]          # the values the fp32 buffer holds


@pytest.mark.parametrize('R', RADII)
def test_seam_samples_sit_where_they_are_meant_to(R):
    raw, z, o, d, info = tr.seam_cases(R)
    assert len(info) == 18 and z.shape == (18, 2) and raw.shape == (18, 2, 1)
    _, _, gap64 = tr.intensities_fp64(z, o, d, R, 0.63)
    _, _, gap_ld = tr.intensities_longdouble(z, o, d, R, 0.63)
    for i, case in enumerate(info):
        g64, gld = gap64[i, 0].item(), float(gap_ld[i, 0])
        if case['side'] == 0:
            assert g64 == 0.0 and gld == 0.0, (case, g64, gld)              # r == R by bits
        else:
            assert np.sign(g64) == np.sign(gld) == case['side'], (case, g64, gld)
            assert abs(g64) < 1e-6 * R, (case, g64)                          # one step beside, not far away
    # the line element carries |d|: D_0 = D_1 = (z_1 - z_0) |d| is the same length for every scale of a ray
    dl = (z[:, 1] - z[:, 0]).double() * d.double().norm(dim=-1)
    for i, case in enumerate(info):
        assert dl[i].item() == pytest.approx(4 * R - R if case['radial'] else 8.0, rel=1e-6)


@pytest.mark.parametrize('u', LIMB32)
@pytest.mark.parametrize('R', RADII)
def test_reference_masks_the_limb_as_inside(R, u):
    raw, z, o, d, info = tr.seam_cases(R)
    i_tot, i_p, _ = tr.intensities_fp64(z, o, d, R, u)
    out = tr.thomson_integral(raw, z, o, d, 1.0, solar_radius=R, limb=u)
    for i, case in enumerate(info):
        live = case['side'] > 0
        assert (i_tot[i, 0].item() > 0) == live, (case, i_tot[i, 0].item())
        assert (out['pixel_B'][i, 0].item() > 0) == live
        if case['radial'] or not live:
            assert i_p[i, 0].item() == 0.0 and out['pixel_B'][i, 1].item() == 0.0, case
        else:
            assert i_p[i, 0].item() > 0, case
        # the masked sample still counts everywhere else
        assert out['pixel_density'][i].item() > 0 and out['weights'][i, 0].item() == pytest.approx(1.0, abs=1e-9)
        r0 = (o[i].double() + d[i].double() * z[i, 0].double()).norm().item()
        assert out['distance_from_sun'][i].item() == pytest.approx(r0, rel=1e-9)
        assert out['distance_from_obs'][i].item() == pytest.approx(R if case['radial'] else 8.0, rel=1e-6)
        assert out['weights'][i, 1].item() == 0.0


def test_restatement_noise_at_the_limb_is_negligible_beside_the_gate():
    """|fp64 restatement - long double, cancellation-free| / value on every live seam sample: at most 1e-6 (1 % of the 1e-4
    gate).  Measured with an 80-bit long double: 4.7e-14 on I_tot, 1.2e-7 on I_P at u = 0 (= cos Omega there; that is the long
    double's own rounding of r in (r - R)(r + R) at r - R = 8e-14).  With cos^2 taken as 1 - (R / r)^2 the restatement missed
    this bound: 7.6e-4 on that I_P and 2.9e-10 on I_tot, see thomson_reference._geometry."""
    worst = {'I_tot': (0.0, None), 'I_P': (0.0, None)}
    for R in RADII:
        raw, z, o, d, info = tr.seam_cases(R)
        for u in LIMB32:
            t64, p64, _ = tr.intensities_fp64(z, o, d, R, u)
            tld, pld, _ = tr.intensities_longdouble(z, o, d, R, u)
            for i, case in enumerate(info):
                if case['side'] <= 0:
                    assert float(tld[i, 0]) == 0.0 and float(pld[i, 0]) == 0.0 and t64[i, 0].item() == 0.0
                    continue
                for name, a, b in (('I_tot', t64[i, 0].item(), tld[i, 0]), ('I_P', p64[i, 0].item(), pld[i, 0])):
                    if float(b) == 0.0:
                        assert a == 0.0, (case, name)
                        continue
                    err = abs(float((np.longdouble(a) - b) / b))
                    if err > worst[name][0]:
                        worst[name] = (err, (R, u, case['name'], case['scale']))
    wider = '' if tr.LONG_DOUBLE_IS_WIDER else ' (long double is no wider than fp64 here: only the forms differ)'
    for name, (err, where) in worst.items():
        print(f'limb: worst |fp64 - long double| / value of {name} = {err:.2e} at (R, u, case, |d|) = {where}{wider}')
        assert err <= 1e-6, (name, err, where)


def test_restatement_agrees_with_long_double_away_from_the_limb():
    """r - R > 1e-3 R, r <= 9: the fp64 differences 4/3 - c - c^3/3 etc. cancel to ~1e-16 / s^2 < 1e-13 here."""
    gen = torch.Generator().manual_seed(0)
    o = torch.tensor([[0., -8., 1.0], [0., -8., 4.0], [0., -8., 0.5], [0., -8., 1.5]])      # r <= 9: s >= 1 / 18
    d = torch.tensor([[0., 1., 0.]]).repeat(4, 1)
    z = (torch.rand(4, 64, generator=gen) * 16).sort(dim=1).values
    for R in (1.0, 0.5):
        t64, p64, gap = tr.intensities_fp64(z, o, d, R, 0.63)
        tld, pld, _ = tr.intensities_longdouble(z, o, d, R, 0.63)
        sel = (gap > 1e-3 * R).numpy()
        assert sel.any()
        for a, b in ((t64.numpy(), tld), (p64.numpy(), pld)):
            err = np.abs((a.astype(np.longdouble) - b)[sel] / b[sel]).max()
            assert float(err) < 1e-12, float(err)


@pytest.mark.parametrize('R', RADII)
def test_closed_forms_at_the_limb(R):
    """s -> 1: A -> 0, B -> 1/4, C -> 4/3, D -> 3/4 and sin^2 chi = 1 on the tangent ray: I_P -> u / 4,
    I_tot -> 2 ((1 - u) 4/3 + u 3/4) - u / 4; on the radial ray I_P = 0."""
    raw, z, o, d, info = tr.seam_cases(R)
    for u, want_tot, want_p in ((1.0, 1.25, 0.25), (0.0, 8 / 3, 0.0), (LIMB32[1], None, None)):
        if want_tot is None:
            want_p = u / 4
            want_tot = 2 * ((1 - u) * 4 / 3 + u * 0.75) - want_p
        i_tot, i_p, _ = tr.intensities_fp64(z, o, d, R, u)
        for i, case in enumerate(info):
            if case['side'] <= 0:
                continue
            if case['radial']:
                assert i_p[i, 0].item() == 0.0
                assert i_tot[i, 0].item() == pytest.approx(want_tot + want_p, abs=2e-3)   # c ~ 5e-4 one fp32 step outside
            else:
                assert i_tot[i, 0].item() == pytest.approx(want_tot, abs=1e-5)            # c ~ 1e-6
                assert i_p[i, 0].item() == pytest.approx(want_p, abs=1e-5)


@pytest.mark.parametrize('c', [1, 2])
def test_muted_samples_get_a_zero_gradient_not_nan(c):
    """raw0 = -inf: rho = 0, and fp64 autograd through the restatement gives exactly 0 there for every output."""
    raw, z, o, d, info = tr.seam_cases(4.0, c=c)
    gen = torch.Generator().manual_seed(1)
    for keys in [(k,) for k in tr.KEYS] + [tr.KEYS]:
        leaf = raw.double().requires_grad_(True)
        out = tr.thomson_integral(leaf, z, o, d, tr.LN10 if c == 2 else 1.0, solar_radius=4.0, limb=0.37, c0=2.5)
        loss = sum((out[k] * torch.randn(out[k].shape, generator=gen, dtype=torch.float64)).sum() for k in keys)
        g = torch.autograd.grad(loss, leaf)[0]
        assert bool(torch.isfinite(g).all()), keys
        assert bool((g[:, 1] == 0).all()), keys
        if c == 2:
            assert bool((g[..., 1] == 0).all())
        if keys == ('pixel_B',):
            for i, case in enumerate(info):
                assert (g[i, 0, 0].item() != 0) == (case['side'] > 0), case          # on the limb: exactly 0


@pytest.mark.parametrize('R', [1.0, 4.0])
def test_degenerate_rays_have_finite_reference_outputs(R):
    raw, z, o, d, names = tr.degenerate_rays(R, 40)
    leaf = raw.double().requires_grad_(True)
    out = tr.thomson_integral(leaf, z, o, d, 1.0, solar_radius=R, limb=0.63, c0=2.5)
    for k in tr.KEYS:
        assert bool(torch.isfinite(out[k]).all()), k
    g = torch.autograd.grad(sum(out[k].sum() for k in tr.KEYS), leaf)[0]
    assert bool(torch.isfinite(g).all())
    i = {n: j for j, n in enumerate(names)}
    # a ray through the centre: no polarised brightness, some total brightness (it has samples outside the Sun)
    assert out['pixel_B'][i['centre'], 1].item() == 0.0 and out['pixel_B'][i['centre'], 0].item() > 0
    # d = 0: no line element, the observer's own radius
    j = i['null-d']
    assert out['pixel_B'][j].abs().sum().item() == 0.0 and out['pixel_density'][j].item() == 0.0
    assert out['distance_from_obs'][j].item() == 0.0
    assert out['distance_from_sun'][j].item() == pytest.approx(o[j].double().norm().item(), rel=1e-9)
    assert out['weights'][j].sum().item() == pytest.approx(1.0, abs=1e-9)
    # the origin sample is inside; its neighbours outside still shine
    i_tot, i_p, gap = tr.intensities_fp64(z, o, d, R, 0.63)
    at = int((z[i['origin']] == np.float32(2 * R)).nonzero()[0])
    assert gap[i['origin'], at].item() == -R and i_tot[i['origin'], at].item() == 0.0
    assert out['pixel_B'][i['origin'], 1].item() == 0.0 and out['pixel_B'][i['origin'], 0].item() > 0
    # repeated z: zero line elements inside a run, positive ones between runs
    dz = z[i['repeats'], 1:] - z[i['repeats'], :-1]
    assert bool((dz == 0).any()) and bool((dz > 0).any()) and out['pixel_B'][i['repeats'], 0].item() > 0
