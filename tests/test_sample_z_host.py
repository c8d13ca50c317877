"""CPU checks of the sample-placement restatement (tests/sample_z_reference.py) that the GPU test compares the kernel with:

* with torch's CPU square root handed in, it IS the oracle (``sunerf_oracle.stratified_z`` / ``spherical_z``), bit for bit and
  NaN for NaN, at every shape, constant pair and jitter setting of the GPU test (measured: 0 of 1,604,808 elements differ);
* with the IEEE square root it reproduces the four arrays of fixture ``g1_sampler`` bit for bit (measured: 0 differ);
* the share of elements on which the IEEE variant and the oracle differ is printed, not asserted: it is a property of the
  host's torch build, whose fp32 ``sqrt`` / ``pow(0.5)`` is one ulp off the correctly rounded value for 0.65 % of inputs
  (measured: 6,461 of 1e6 uniform values in (0, 6e4); 5,860 of 1,604,808 z values; numpy's: 0 of 1e6 against fp64-then-round)."""
import numpy as np
import pytest
import torch

import sample_z_reference as sz
import sunerf_oracle as orc
from conftest import load_golden

ORACLE = {sz.STRATIFIED: orc.stratified_z, sz.SPHERICAL: orc.spherical_z}
CONSTANTS = {sz.STRATIFIED: sz.STRATIFIED_CONSTANTS, sz.SPHERICAL: sz.SPHERICAL_CONSTANTS}


def _oracle(kind, o, d, t_vals, t_rand, distance, solar_R):
    f32 = torch.float32
    return ORACLE[kind](torch.from_numpy(o), torch.from_numpy(d), torch.from_numpy(t_vals)[None],
                        torch.tensor(distance, dtype=f32), torch.tensor(solar_R, dtype=f32),
                        None if t_rand is None else torch.from_numpy(t_rand)).numpy()


def test_numpy_sqrt_and_divide_are_correctly_rounded():
    """The restatement's claim to be the IEEE evaluation rests on numpy's fp32 sqrt and divide."""
    rng = np.random.default_rng(0)
    x = rng.uniform(0., 6e4, 1_000_000).astype(np.float32)
    y = rng.uniform(0.1, 3., x.size).astype(np.float32)
    assert np.array_equal(np.sqrt(x), np.sqrt(x.astype(np.float64)).astype(np.float32))
    assert np.array_equal(x / y, (x.astype(np.float64) / y.astype(np.float64)).astype(np.float32))
    off = int((torch.sqrt(torch.from_numpy(x)).numpy() != np.sqrt(x)).sum())
    off_pow = int((torch.from_numpy(x).pow(0.5).numpy() != np.sqrt(x)).sum())
    print(f'torch CPU fp32 sqrt differs from the correctly rounded value on {off} of {x.size} inputs, pow(0.5) on {off_pow}')


@pytest.mark.parametrize('n,s', sz.SHAPES)
def test_restatement_with_torch_sqrt_is_the_oracle(n, s):
    cases = [sz.make_case(n, s, 1000 * n + s)]
    if (n, s) == (513, 128):
        cases.append(sz.make_case(n, s, 7, monotone=False))
    total = differ_torch = differ_ieee = 0
    for o, d, limb, t_vals, t_rand in cases:
        if n >= 255:
            sz.assert_population(sz.population_facts(o, d, limb))
        for kind in (sz.STRATIFIED, sz.SPHERICAL):
            for distance, solar_R in CONSTANTS[kind]:
                for jitter in (None, t_rand):
                    want = _oracle(kind, o, d, t_vals, jitter, distance, solar_R)
                    got = sz.sample_z(kind, o, d, t_vals, jitter, distance, solar_R, sqrt=sz.torch_sqrt)
                    assert np.array_equal(np.isnan(got), np.isnan(want))
                    differ_torch += int(sz.bits_differ(got, want).sum())
                    differ_ieee += int(sz.bits_differ(sz.sample_z(kind, o, d, t_vals, jitter, distance, solar_R), want).sum())
                    total += want.size
    print(f'({n}, {s}): restatement with torch.sqrt differs from the oracle on {differ_torch} of {total} elements; '
          f'with the IEEE sqrt on {differ_ieee} ({100. * differ_ieee / total:.2f} %, not asserted)')
    assert differ_torch == 0


def test_ieee_restatement_reproduces_the_sampler_fixture():
    g = {k: v.numpy() for k, v in load_golden('g1_sampler').items()}
    t, t_rs = g['t_vals'].reshape(-1), g['t_vals_rs'].reshape(-1)
    rs_distance = float(np.float32(1.3 / 0.5))
    got = {'z_vals': sz.sample_z(sz.STRATIFIED, g['rays_o'], g['rays_d'], t, None, 1.3, 1.0),
           'z_vals_perturb': sz.sample_z(sz.STRATIFIED, g['rays_o'], g['rays_d'], t, g['t_rand'], 1.3, 1.0),
           'z_vals_sph': sz.sample_z(sz.SPHERICAL, g['rays_o_sph'], g['rays_d_sph'], t, None, 2.0, 1.0),
           'z_vals_rs': sz.sample_z(sz.STRATIFIED, g['rays_o_rs'], g['rays_d'], t_rs, None, rs_distance, 2.0)}
    for k, v in got.items():
        differ = int(sz.bits_differ(v, g[k]).sum())
        print(f'g1_sampler {k}: {differ} of {v.size} elements differ')
        assert differ == 0, k


def test_helpers():
    a = np.array([1., -0., np.nan, 1., np.nan], dtype=np.float32)
    b = np.array([np.nextafter(np.float32(1.), np.float32(2.)), 0., -np.nan, 1., 1.], dtype=np.float32)
    assert sz.bits_differ(a, b).tolist() == [True, True, False, False, True]
    assert sz.ulp_distance(a, b).tolist() == [1, 0, 0, 0, 2 ** 31 - 1]
    # the special rows of a batch are what the docstring says, and an origin inside the sun / the sampling sphere is sampled
    o, d, _ = sz.make_rays(7, 3)
    assert (d[3] == 0).all() and (o[4] == 0).all() and np.isnan(o[5, 1]) and np.isinf(d[6, 2])
    z = sz.sample_z(sz.STRATIFIED, o, d, [0., 0.5, 1.], None, 1.3, 1.0)
    # d = 0: 0 / 0 = NaN for dist_inner, so the far end is |o| + distance; o = 0: near = -distance, far = -1 / |d|
    # (an Inf in d: inf - inf = NaN under the root, the same far end)
    assert np.isfinite(z[3]).all() and np.isfinite(z[4]).all() and np.isnan(z[5]).all() and np.isfinite(z[6]).all()
    assert z[4, 0] == np.float32(-1.3) and z[4, 2] < 0
    assert np.isnan(sz.sample_z(sz.SPHERICAL, o, d, [0., 0.5, 1.], None, 2.0, 1.0)[[3, 5, 6]]).all()
    inside = np.array([[0.5, 0., 0.], [1.2, 0., 0.]], dtype=np.float32)
    z = sz.sample_z(sz.STRATIFIED, inside, np.array([[1., 0., 0.]] * 2, dtype=np.float32), [0., 1.], None, 1.3, 1.0)
    assert z[0].tolist() == [np.float32(0.5) - np.float32(1.3), -1.5]       # the far end is the NEGATIVE-side root -b - sqrt
    assert z[1, 0] == np.float32(1.2) - np.float32(1.3) and z[1, 1] == np.float32(-2.2)
