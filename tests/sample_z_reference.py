"""Host restatement of sample placement (csrc/sampler.hip: ``sample_z_kernel``; sunerf/train/sampling.py:16-49, :68-98) in
numpy float32, and the seeded ray population the sample-placement tests run on.

Every product, sum, quotient and square root is one float32 numpy operation, i.e. rounded separately and correctly (numpy's
fp32 ``sqrt`` and ``/`` are the IEEE ones), in the order in which ``sunerf_oracle.stratified_z`` / ``spherical_z`` /
``_jitter`` restate sampling.py: ``(x^2 + y^2) + z^2``, ``((2 o) d)`` summed left to right, ``(4 a) c``, ``2 a``,
``near (1 - t) + far t`` and the mid-point jitter.  This -- the IEEE evaluation of the reference's operation order -- is
the kernel's contract.  ``sqrt`` is an argument because torch's CPU fp32 square root is not the IEEE one in every build
(tests/test_sample_z_host.py measures the share): handing ``torch.sqrt`` in ties this very code to the oracle bit for bit.
"""
import numpy as np

STRATIFIED, SPHERICAL = 0, 1          # include/sunerf_hip.h: SUNERF_SAMPLER_*, sunerf_hip.ops.SAMPLER_*

F32 = np.float32

# (n_rays, S) of the tests: 255 / 256 / 257 elements around one 256-thread block, ragged last blocks, S odd, prime-ish and
# larger than a block, idx / S for S that is no power of two
SHAPES = ((1, 1), (1, 2), (3, 85), (1, 256), (1, 257), (7, 33), (4099, 33), (255, 257), (513, 128))
# (distance, solar_R): the default buffers of sampling.py:62-63, and those of Rs_per_ds = 0.5
STRATIFIED_CONSTANTS = ((1.3, 1.0), (float(np.float32(1.3 / 0.5)), 2.0))
SPHERICAL_CONSTANTS = ((2.0, 1.0),)


def _sum3(v):
    return (v[:, 0] + v[:, 1]) + v[:, 2]


def ray_terms(rays_o, rays_d, radius):
    """(oo, a, b, b^2 - (4 a) c) of the ray-sphere quadratic for a sphere of ``radius``, fp32, each operation rounded."""
    o, d = np.asarray(rays_o, dtype=F32), np.asarray(rays_d, dtype=F32)
    with np.errstate(all='ignore'):
        oo = _sum3(o * o)                                  # rays_o.pow(2).sum(-1)
        a = _sum3(d * d)                                   # rays_d.pow(2).sum(-1)
        b = _sum3((F32(2.) * o) * d)                       # (2 * rays_o * rays_d).sum(-1)
        c = oo - F32(radius) * F32(radius)
        return oo, a, b, b * b - (F32(4.) * a) * c


def sample_z(kind, rays_o, rays_d, t_vals, t_rand, distance, solar_R, sqrt=np.sqrt):
    """``StratifiedSampler.forward`` (``kind`` = STRATIFIED) or ``SphericalSampler.forward`` (SPHERICAL) -> (N, S) fp32.
    ``t_rand``: None, or the (N, S) uniform numbers of the in-bin jitter.  ``sqrt``: float32 array -> float32 array."""
    t = np.asarray(t_vals, dtype=F32).reshape(1, -1)
    with np.errstate(all='ignore'):
        oo, a, b, disc = ray_terms(rays_o, rays_d, solar_R)
        dist_inner = (-b - sqrt(disc)) / (F32(2.) * a)
        if kind == STRATIFIED:
            dist_o = sqrt(oo)
            dist_near, dist_far = dist_o - F32(distance), dist_o + F32(distance)
        elif kind == SPHERICAL:
            root = sqrt(ray_terms(rays_o, rays_d, distance)[3])
            dist_near, dist_far = (-b - root) / (F32(2.) * a), (-b + root) / (F32(2.) * a)
        else:
            raise ValueError(kind)
        dist_far = np.where(np.isnan(dist_inner), dist_far, dist_inner)      # stop at the solar surface
        z = dist_near[:, None] * (F32(1.) - t) + dist_far[:, None] * t
        if t_rand is not None:                                               # sampling.py:93-98
            mids = F32(.5) * (z[:, 1:] + z[:, :-1])
            upper = np.concatenate([mids, z[:, -1:]], 1)
            lower = np.concatenate([z[:, :1], mids], 1)
            z = lower + (upper - lower) * np.asarray(t_rand, dtype=F32)
    assert z.dtype == F32
    return z


def torch_sqrt(a):
    """``sqrt=`` that takes the square roots with torch's CPU kernel, like the oracle."""
    import torch
    return torch.sqrt(torch.from_numpy(np.ascontiguousarray(a))).numpy()


def bits_differ(a, b):
    """Elementwise: not the same bits, and not NaN in both (NaN sign and payload are not compared)."""
    a, b = np.ascontiguousarray(a, dtype=F32), np.ascontiguousarray(b, dtype=F32)
    return (a.view(np.int32) != b.view(np.int32)) & ~(np.isnan(a) & np.isnan(b))


def ulp_distance(a, b):
    """Distance in fp32 ulps between finite ``a`` and ``b`` (0 where both are NaN, 2^31 - 1 where one is)."""
    def ordered(v):
        i = np.ascontiguousarray(v, dtype=F32).view(np.int32).astype(np.int64)
        return np.where(i < 0, -(i & 0x7fffffff), i)
    d = np.abs(ordered(a) - ordered(b))
    nan_a, nan_b = np.isnan(a), np.isnan(b)
    return np.where(nan_a & nan_b, 0, np.where(nan_a | nan_b, 2 ** 31 - 1, d))


# ---- the ray population -----------------------------------------------------------------------------------------------
N_SPECIAL = 4          # the last rows of a batch of n >= 7 rays: d = 0, o = 0, a NaN component in o, an Inf component in d
LIMB_HALF_WIDTH = 4e-6


def _unit(rng, n):
    v = rng.standard_normal((n, 3))
    return v / np.linalg.norm(v, axis=1, keepdims=True)


def make_rays(n, seed):
    """``(rays_o, rays_d, limb)``: fp32 (n, 3) origins and directions, and the mask of the limb rays.

    Origins in every direction at radii 0.5 ... 250 (log-uniform: inside the sun, inside the sampling sphere, 1 AU);
    directions towards targets within 2.5 radii of the centre, |d| in 0.5 ... 1.5.  Every fourth ray (with its origin outside
    the sun) is aimed at the point of its own closest approach, placed at a radius within 4e-6 of 1: its discriminant
    4 |d|^2 (1 - p^2) is below the rounding of b^2, so its sign -- hit or miss -- is decided by the last bits.  For
    n >= 7 the last four rows are the degenerate ones (``N_SPECIAL``)."""
    rng = np.random.default_rng(seed)
    radius = 0.5 * 500. ** rng.uniform(0., 1., (n, 1))
    o = _unit(rng, n) * radius
    target = _unit(rng, n) * (2.5 * rng.uniform(0., 1., (n, 1)))
    limb = (np.arange(n) % 4 == 1) & (radius[:, 0] > 1.001)
    # closest-approach point at radius rho for an origin at radius R > rho: p = (rho^2 / R^2) o + rho sqrt(1 - rho^2 / R^2) u,
    # u a unit vector perpendicular to o, so that p . (p - o) = 0
    rho = 1. + rng.uniform(-LIMB_HALF_WIDTH, LIMB_HALF_WIDTH, (n, 1))
    u = np.cross(o, _unit(rng, n))
    u = u / np.linalg.norm(u, axis=1, keepdims=True)
    q = np.minimum(rho / radius, 1.)
    tangent = q * q * o + rho * np.sqrt(1. - q * q) * u
    target = np.where(limb[:, None], tangent, target)
    d = target - o
    d = d / np.linalg.norm(d, axis=1, keepdims=True) * rng.uniform(0.5, 1.5, (n, 1))
    o, d = o.astype(F32), d.astype(F32)
    if n >= 7:
        d[n - 4] = 0.
        o[n - 3] = 0.
        o[n - 2, 1] = np.nan
        d[n - 1, 2] = np.inf
        limb[n - 4:] = False
    return o, d, limb


def make_case(n, s, seed, monotone=True):
    """``(rays_o, rays_d, limb, t_vals (S,), t_rand (n, S))`` of one shape: ``t_vals`` are torch.linspace's own fp32 values
    (sampling.py:65-66), or for ``monotone=False`` arbitrary numbers in (-0.2, 1.2) in no order."""
    import sunerf_oracle as orc
    o, d, limb = make_rays(n, seed)
    rng = np.random.default_rng(seed + 1000)
    t_rand = rng.uniform(0., 1., (n, s)).astype(F32)
    t_vals = orc.linspace_t_vals(s).numpy().reshape(-1) if monotone else rng.uniform(-0.2, 1.2, s).astype(F32)
    return o, d, limb, t_vals, t_rand


def population_facts(rays_o, rays_d, limb):
    """What the tests assert about a large batch before any kernel is looked at, from the restatement alone."""
    body = slice(0, rays_o.shape[0] - (N_SPECIAL if rays_o.shape[0] >= 7 else 0))
    o, d, limb = rays_o[body], rays_d[body], limb[body]
    norm_o = np.linalg.norm(o.astype(np.float64), axis=1)
    norm_d = np.linalg.norm(d.astype(np.float64), axis=1)
    disc = ray_terms(o, d, 1.0)[3]
    miss_sphere = np.isnan(sample_z(SPHERICAL, o, d, [0., 1.], None, 2.0, 1.0)).all(1)
    p = np.linalg.norm(np.cross(o.astype(np.float64), d.astype(np.float64)), axis=1) / norm_d      # impact parameter
    return {'n': o.shape[0], 'distinct_dist_o': np.unique(np.sqrt(ray_terms(o, d, 1.0)[0])).size,
            'min_o': norm_o.min(), 'max_o': norm_o.max(), 'min_d': norm_d.min(), 'max_d': norm_d.max(),
            'octants': np.unique((o > 0) @ np.array([1, 2, 4])).size,
            'inside_sun': int((norm_o < 1.).sum()), 'inside_sampling_sphere': int(((norm_o > 1.) & (norm_o < 1.3)).sum()),
            'limb_share': limb.mean(), 'limb_max_offset': np.abs(p[limb] - 1.).max() if limb.any() else 0.,
            'limb_hits': int((disc[limb] >= 0).sum()), 'limb_misses': int((disc[limb] < 0).sum()),
            'hit_share': (disc >= 0).mean(), 'sphere_miss_share': miss_sphere.mean()}


def assert_population(facts):
    n = facts['n']
    assert facts['distinct_dist_o'] > 0.9 * n and facts['octants'] == 8, facts
    assert 0.5 <= facts['min_o'] < 0.6 and 150. < facts['max_o'] <= 250.001, facts
    assert 0.499 <= facts['min_d'] < 0.6 and 1.4 < facts['max_d'] <= 1.501, facts
    assert facts['inside_sun'] > 0 and facts['inside_sampling_sphere'] > 0, facts
    assert 0.2 <= facts['limb_share'] <= 0.25 and facts['limb_max_offset'] <= 1e-4, facts      # 4e-6 and the fp32 rounding of o (|o| <= 250) and d
    assert facts['limb_hits'] > 0 and facts['limb_misses'] > 0, facts
    assert 0.1 <= facts['hit_share'] <= 0.9, facts
    assert 0.02 <= facts['sphere_miss_share'] <= 0.2, facts
