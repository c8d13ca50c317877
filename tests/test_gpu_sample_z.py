"""Sample placement on MI355X (csrc/sampler.hip: ``sample_z_kernel``) against the IEEE evaluation of the reference's operation
order (tests/sample_z_reference.py, tied to the oracle and to fixture g1_sampler by tests/test_sample_z_host.py).

The contract is the kernel's own: the same bits, or NaN in both (NaN sign and payload are not compared) -- no tolerance.
Shapes put 255, 256 and 257 elements around one 256-thread block, leave ragged last blocks and divide by S that are odd,
prime-ish and larger than a block; origins lie in every direction at 0.5 ... 250 radii (inside the sun, inside the sampling
sphere, 1 AU), a quarter of the rays graze the limb where the discriminant changes sign, 5 % miss the spherical sampler's
sphere (all-NaN rows), and the last rows of a batch are degenerate (d = 0, o = 0, NaN, Inf).

Measured on MI355X: bit-equal -- 0 of 1,604,808 elements differ (0 ulp) over the nine shapes, both samplers, all constant
pairs, with and without jitter, and the arbitrary ``t_vals`` case; 0 of 666 with origins inside the sun / the sampling sphere.
The device's ``sqrtf`` and divide under the project's flags are correctly rounded: 0 of 200,000 roots, 0 of 200,000 quotients
and 0 of 200,000 ``(-b - sqrt(D)) / (2 a)`` differ from fp64-then-round.  A scratch build that sums ``b`` in another order fails
19 of the cases here."""
import numpy as np
import pytest
import torch

import sample_z_reference as sz

pytestmark = pytest.mark.gpu

CONSTANTS = {sz.STRATIFIED: sz.STRATIFIED_CONSTANTS, sz.SPHERICAL: sz.SPHERICAL_CONSTANTS}
_CASES = {}


@pytest.fixture(scope='module')
def ops():
    assert torch.cuda.is_available(), 'GPU tests need a ROCm device'
    from sunerf_hip import ops as _ops
    assert (_ops.SAMPLER_STRATIFIED, _ops.SAMPLER_SPHERICAL) == (sz.STRATIFIED, sz.SPHERICAL)
    return _ops


def _case(n, s, seed, monotone=True):
    """One seeded case and its references, computed once and shared (read-only)."""
    key = (n, s, seed, monotone)
    if key not in _CASES:
        o, d, limb, t_vals, t_rand = sz.make_case(n, s, seed, monotone)
        want = {(kind, c, jitter): sz.sample_z(kind, o, d, t_vals, t_rand if jitter else None, *c)
                for kind in (sz.STRATIFIED, sz.SPHERICAL) for c in CONSTANTS[kind] for jitter in (False, True)}
        for v in want.values():
            v.setflags(write=False)
        _CASES[key] = (o, d, limb, t_vals, t_rand, want)
    return _CASES[key]


def _kernel(ops, kind, o, d, t_vals, t_rand, distance, solar_R):
    z = ops.sample_z(kind, torch.from_numpy(o).cuda(), torch.from_numpy(d).cuda(), torch.from_numpy(t_vals).cuda(), distance,
                     solar_R, t_rand=None if t_rand is None else torch.from_numpy(t_rand).cuda())
    return z.cpu().numpy()


def _assert_same_bits(got, want, what):
    assert got.shape == want.shape and got.dtype == np.float32, what
    differ = sz.bits_differ(got, want)
    nan_rows = int(np.isnan(want).all(1).sum())
    ulps = sz.ulp_distance(got, want)
    print(f'{what}: {int(differ.sum())} of {want.size} elements differ, max {int(ulps.max()) if ulps.size else 0} ulp; '
          f'{nan_rows} of {want.shape[0]} rows all NaN')
    assert np.array_equal(np.isnan(got), np.isnan(want)), what
    assert not differ.any(), (what, int(differ.sum()), np.argwhere(differ)[:5].tolist())


@pytest.mark.parametrize('jitter', [False, True], ids=['plain', 'jitter'])
@pytest.mark.parametrize('kind', [sz.STRATIFIED, sz.SPHERICAL], ids=['stratified', 'spherical'])
@pytest.mark.parametrize('n,s', sz.SHAPES)
def test_sample_z_is_the_ieee_evaluation(ops, n, s, kind, jitter):
    o, d, limb, t_vals, t_rand, want = _case(n, s, 1000 * n + s)
    if n >= 255:      # the population has what the case is about: asserted on the restatement alone
        facts = sz.population_facts(o, d, limb)
        sz.assert_population(facts)
        if kind == sz.SPHERICAL:
            share = np.isnan(want[(kind, CONSTANTS[kind][0], jitter)]).all(1).mean()
            assert 0.02 <= share <= 0.2, share
    for c in CONSTANTS[kind]:
        got = _kernel(ops, kind, o, d, t_vals, t_rand if jitter else None, *c)
        _assert_same_bits(got, want[(kind, c, jitter)], f'({n}, {s}) kind {kind} distance {c[0]:.2f} solar_R {c[1]} jitter {jitter}')


@pytest.mark.parametrize('kind', [sz.STRATIFIED, sz.SPHERICAL], ids=['stratified', 'spherical'])
def test_arbitrary_t_vals(ops, kind):
    """``t_vals`` in no order and beyond [0, 1]: the kernel takes them as they come (mid points of neighbours in the jitter)."""
    n, s = 513, 128
    o, d, limb, t_vals, t_rand, want = _case(n, s, 7, monotone=False)
    assert (np.diff(t_vals) < 0).any() and t_vals.min() < 0 and t_vals.max() > 1
    for jitter in (False, True):
        for c in CONSTANTS[kind]:
            got = _kernel(ops, kind, o, d, t_vals, t_rand if jitter else None, *c)
            _assert_same_bits(got, want[(kind, c, jitter)], f'arbitrary t_vals, kind {kind} {c} jitter {jitter}')


def test_origins_inside_the_sun_and_inside_the_sampling_sphere(ops):
    """Stratified sampler: |o| < solar_R (the far end is the root behind the origin) and solar_R < |o| < distance (the
    near end is behind the origin)."""
    rng = np.random.default_rng(5)
    n, s = 37, 9
    u = rng.standard_normal((n, 3))
    u /= np.linalg.norm(u, axis=1, keepdims=True)
    radius = np.where(np.arange(n) % 2 == 0, rng.uniform(0.05, 0.999, n), rng.uniform(1.001, 1.299, n))
    o = (u * radius[:, None]).astype(np.float32)
    d = rng.standard_normal((n, 3))
    d = (d / np.linalg.norm(d, axis=1, keepdims=True) * rng.uniform(0.5, 1.5, (n, 1))).astype(np.float32)
    t_vals = np.linspace(0., 1., s).astype(np.float32)
    t_rand = rng.uniform(0., 1., (n, s)).astype(np.float32)
    want = sz.sample_z(sz.STRATIFIED, o, d, t_vals, None, 1.3, 1.0)
    inside = radius < 1.
    assert (want[inside, -1] < 0).all() and (want[:, 0] < 0).all() and not np.isnan(want[inside]).any()
    assert (sz.ray_terms(o[~inside], d[~inside], 1.0)[3] < 0).any()     # some of the others miss the sun
    for jitter in (None, t_rand):
        got = _kernel(ops, sz.STRATIFIED, o, d, t_vals, jitter, 1.3, 1.0)
        _assert_same_bits(got, sz.sample_z(sz.STRATIFIED, o, d, t_vals, jitter, 1.3, 1.0),
                          f'origins inside, jitter {jitter is not None}')


def test_device_sqrt_and_divide_are_correctly_rounded(ops):
    """The kernel's three building blocks, isolated through inputs that leave one of them alone in the result, against the
    correctly rounded values (fp64, then rounded once; numpy's fp32 operations are asserted equal to that).

    * ``dist_o``: t = 0 and distance = 0 give z = sqrt(oo) * 1 + far * 0 = sqrtf(oo), with oo = fl(x^2) for o = (x, 0, 0);
    * the quotient: o = 0, d = (dx, 0, 0), t = 1 give z = -2 |dx| / (2 fl(dx^2)), the root being exact;
    * both behind a rounded discriminant: o = (ox, 0, 0), d = (dx, 0, 0), t = 1 give z = (-b - sqrt(D)) / (2 a)."""
    rng = np.random.default_rng(1)
    m = 200_000
    zero = np.zeros(m, dtype=np.float32)
    # 1. sqrt alone
    x = (0.5 * 500. ** rng.uniform(0., 1., m)).astype(np.float32)
    o = np.stack([x, zero, zero], 1)
    d = np.stack([-np.ones(m, dtype=np.float32), zero, zero], 1)
    oo = x * x
    want = np.sqrt(oo.astype(np.float64)).astype(np.float32)
    assert np.array_equal(want, np.sqrt(oo))
    got = _kernel(ops, sz.STRATIFIED, o, d, np.zeros(1, dtype=np.float32), None, 0.0, 1.0)[:, 0]
    off = sz.ulp_distance(got, want)
    print(f'device sqrtf: {int((off != 0).sum())} of {m} differ from the correctly rounded root, max {int(off.max())} ulp')
    assert not (off != 0).any()
    # 2. the divide alone: o = 0 gives b = 0 and D = (4 a) (1) = 4 fl(dx^2), whose correctly rounded root is 2 |dx| exactly
    # (step 1 has just checked the device's roots of numbers of this very form), so z = (-0 - 2 |dx|) / (2 fl(dx^2))
    dx = rng.uniform(0.5, 1.5, m).astype(np.float32)
    o, d = np.zeros((m, 3), dtype=np.float32), np.stack([dx, zero, zero], 1)
    oo, a, b, disc = sz.ray_terms(o, d, 1.0)
    assert np.array_equal(np.sqrt(disc), np.float32(2.) * dx) and not b.any()
    num, den = -b - np.sqrt(disc), np.float32(2.) * a
    want = (num.astype(np.float64) / den.astype(np.float64)).astype(np.float32)
    assert np.array_equal(want, num / den)
    assert (want.astype(np.float64) * den.astype(np.float64) != num.astype(np.float64)).mean() > 0.5      # the divide does round
    got = _kernel(ops, sz.STRATIFIED, o, d, np.ones(1, dtype=np.float32), None, 1.3, 1.0)[:, 0]
    off = sz.ulp_distance(got, want)
    print(f'device divide: {int((off != 0).sum())} of {m} differ from the correctly rounded quotient, max {int(off.max())} ulp')
    assert not (off != 0).any()
    # 3. root of a rounded discriminant, then the divide
    ox = -(1.01 + 249. * rng.uniform(0., 1., m)).astype(np.float32)
    dx = rng.uniform(0.5, 1.5, m).astype(np.float32)
    o, d = np.stack([ox, zero, zero], 1), np.stack([dx, zero, zero], 1)
    want = sz.sample_z(sz.STRATIFIED, o, d, np.ones(1, dtype=np.float32), None, 1.3, 1.0)[:, 0]
    assert np.isfinite(want).all()
    got = _kernel(ops, sz.STRATIFIED, o, d, np.ones(1, dtype=np.float32), None, 1.3, 1.0)[:, 0]
    off = sz.ulp_distance(got, want)
    print(f'device (-b - sqrt(D)) / (2 a): {int((off != 0).sum())} of {m} differ, max {int(off.max())} ulp')
    assert not (off != 0).any()


@pytest.mark.parametrize('n,s', [(1, 1), (3, 85), (1, 257), (7, 33)])
def test_nothing_is_written_beyond_the_last_sample(ops, n, s):
    """The ragged last block: the launch rounds n * S up to whole 256-thread blocks, and the surplus threads must leave.  The
    entry point is called on an output that sits inside a larger buffer of sentinels; every input carries as much slack as
    the surplus threads of a kernel without the guard would reach (256 more rays, 512 more elements), so that even such a
    kernel stays inside these buffers and shows as overwritten sentinels, not as a fault."""
    from sunerf_hip import lib
    o, d, limb, t_vals, t_rand, want = _case(n, s, 1000 * n + s)
    front, back, sentinel = 256, 512, -12345.0
    total = n * s
    assert (-total) % 256 != 0 and 256 - total % 256 < back         # there are surplus threads, and the slack holds them all
    dev = torch.device('cuda', torch.cuda.current_device())
    pad_rows = lambda a: torch.cat([torch.from_numpy(a), torch.ones(256, 3)]).to(dev).contiguous()      # noqa: E731
    o_buf, d_buf = pad_rows(o), pad_rows(d)
    t_dev = torch.from_numpy(t_vals).to(dev)
    r_buf = torch.cat([torch.from_numpy(t_rand).reshape(-1), torch.full((back,), 0.5)]).to(dev).contiguous()
    for kind in (sz.STRATIFIED, sz.SPHERICAL):
        c = CONSTANTS[kind][0]
        for jitter in (False, True):
            buf = torch.full((front + total + back,), sentinel, dtype=torch.float32, device=dev)
            z = buf[front:front + total]
            lib.call(dev, 'sunerf_sample_z', kind, ops._ptr(o_buf), ops._ptr(d_buf), ops._ptr(t_dev), ops._ptr(r_buf) if jitter else None,
                     n, s, float(c[0]), float(c[1]), ops._ptr(z), ops._stream(dev))
            out = buf.cpu().numpy()
            _assert_same_bits(out[front:front + total].reshape(n, s), want[(kind, c, jitter)], f'({n}, {s}) inside sentinels, kind {kind}')
            touched = int((out[:front] != sentinel).sum() + (out[front + total:] != sentinel).sum())
            assert touched == 0, f'{touched} elements outside the {total} of the output were written'
