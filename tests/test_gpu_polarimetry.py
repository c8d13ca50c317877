"""White-light polarimetry on the device (include/sunerf_hip_polarimetry.h) against its fp64 restatement
tests/polarimetry_reference.py.

* ``stokes``: everything built from ``+ - * /`` is equal by value, status, counts and NaN positions exactly, the two standard
  deviations (one sqrt each) within one fp32 ulp, reruns by bits -- at shapes below, at and above the workgroup of 256 pixels, with
  and without ``bad``, NaN / inf samples, the noise model and the optional outputs, the Sun's centre on a pixel, between pixels and
  outside the frame.
* ``ratio_depth``: the round trip through the existing render kernel.  ``sunerf_thomson_integral_fwd`` with two samples of which
  the first carries nothing puts all the brightness on one sample; pB / tB of its ``pixel_b`` is then that sample's ``f``, and the
  inversion must give back the sample's distance from the closest-approach point, to the bound written out at
  :func:`depth_bound`.
* End to end: a ``SimpleStar`` render, polarised and solved, is the render again; ``add_polarised_view`` feeds the pool.
"""
import numpy as np
import pytest
import torch

import polarimetry_reference as pr

pytestmark = pytest.mark.gpu

STOKES_SHAPES = [(3, 1, 1, 1), (3, 1, 1, 257), (4, 2, 3, 85), (8, 1, 16, 16), (5, 3, 7, 37)]
ANGLES = {3: np.radians([0.0, 60.0, 120.0]), 4: np.radians([0.0, 45.0, 90.0, 135.0]), 5: np.radians([3.0, 41.0, 77.0, 112.0, 158.0]),
          8: np.radians([0.0, 22.5, 45.0, 67.5, 90.0, 112.5, 135.0, 157.5])}
VALUE_KEYS = ('stokes', 'tb', 'pb', 'pb_cross', 'chi2')


def make_frames(n, c, h, w, seed=0, spoil=True):
    """``(frames [n, c, h, w] float32, bad uint8, design, a, b)``: the exposures of a smooth positive (tB, pB) scene with a cross
    term and noise on it; with ``spoil`` and more than two pixels in a plane some samples are NaN, +-inf, flagged or negative (not
    valid under the noise model of plane 0, whose ``a`` is 0), and the first pixel has one valid sample only."""
    rng = np.random.default_rng(1000 * n + 100 * c + 10 * h + w + seed)
    cos2, sin2, thr, eff = pr.design(ANGLES[n], 1.0 + 0.05 * np.arange(n), 0.98 - 0.01 * np.arange(n))
    g = pr.rows(cos2, sin2, thr, eff)
    i = rng.uniform(5.0, 20.0, (c, h, w))
    q, u = rng.uniform(-0.4, 0.4, (2, c, h, w)) * i
    frames = np.stack([g[k, 0] * i + g[k, 1] * q + g[k, 2] * u for k in range(n)])
    frames = (frames + rng.normal(0.0, 0.05, frames.shape)).astype(np.float32)
    bad = np.zeros(frames.shape, dtype=np.uint8)
    if spoil and h * w > 2:
        kind = rng.integers(0, 24, frames.shape)
        frames[kind == 0] = np.nan
        frames[kind == 1] = np.inf
        frames[kind == 2] = -np.inf
        bad[kind == 3] = 1
        frames[kind == 4] = -1.0
        frames[1:, 0, 0, 0] = np.nan
    a, b = 0.002 * np.arange(c), 0.01 / (1.0 + np.arange(c))
    return frames, bad, (cos2, sin2, thr, eff), a, b


def centres(h, w):
    """On a pixel, between pixels, outside the frame."""
    return [(float(h // 2), float(w // 2)), (0.5 * (h - 1) + 0.25, 0.5 * (w - 1) - 0.125), (-3.5, w + 10.0)]


def launch_stokes(frames, bad, design, a, b, centre, outputs=None):
    from sunerf_hip import polarimetry as pl
    t = lambda x: None if x is None else torch.from_numpy(np.ascontiguousarray(x)).cuda()          # noqa: E731
    kw = {} if outputs is None else {'outputs': outputs}
    out = pl.stokes_launch(t(frames), t(bad), *design, t(None if a is None else a.astype(np.float64)),
                           t(None if b is None else b.astype(np.float64)), *centre, **kw)
    torch.cuda.synchronize()
    return out


def ulps(got, want):
    """|got - want| in units of the fp32 spacing at want, where both are finite."""
    fin = np.isfinite(want)
    return np.abs(got[fin].astype(np.float64) - want[fin].astype(np.float64)) / np.spacing(np.abs(want[fin]))


@pytest.mark.parametrize('shape', STOKES_SHAPES, ids=['x'.join(map(str, s)) for s in STOKES_SHAPES])
def test_stokes_equals_the_restatement(shape):
    n, c, h, w = shape
    frames, bad, design, a, b = make_frames(*shape)
    seen = np.zeros(3, dtype=np.int64)
    for centre in centres(h, w):
        for with_bad in (False, True):
            for model in (False, True):
                kw = dict(bad=bad if with_bad else None, a=a if model else None, b=b if model else None)
                got = launch_stokes(frames, kw['bad'], design, kw['a'], kw['b'], centre)
                want = pr.stokes(frames, *design, *centre, **kw)
                what = (shape, centre, with_bad, model)
                for k in VALUE_KEYS:
                    g = got[k].cpu().numpy()
                    assert g.dtype == np.float32 and np.array_equal(g, want[k], equal_nan=True), (k, what)
                assert np.array_equal(got['status'].cpu().numpy(), want['status']), what
                assert np.array_equal(got['counts'].cpu().numpy(), want['counts']), what
                for k in ('sigma_tb', 'sigma_pb'):
                    g = got[k].cpu().numpy()
                    assert np.array_equal(np.isnan(g), np.isnan(want[k])), (k, what)
                    if model:
                        worst = ulps(g, want[k])
                        assert worst.size == 0 or worst.max() <= 1.0, (k, what, worst.max())
                    else:
                        assert np.isnan(g).all(), (k, what)
                again = launch_stokes(frames, kw['bad'], design, kw['a'], kw['b'], centre)
                for k in got:
                    assert torch.equal(got[k].view(torch.uint8), again[k].view(torch.uint8)), (k, what, 'rerun')
                lean = launch_stokes(frames, kw['bad'], design, kw['a'], kw['b'], centre, outputs=('tb', 'pb'))
                assert set(lean) == {'tb', 'pb'} and all(torch.equal(lean[k].view(torch.uint8), got[k].view(torch.uint8)) for k in lean), what
                seen += np.bincount(want['status'].reshape(-1), minlength=3)
    print(f'{shape}: pixels DETERMINED, UNDETERMINED, CENTRE over the variants: {seen.tolist()}')
    assert seen[0] > 0 and seen[2] > 0 and (h * w <= 2 or seen[1] > 0)


def test_stokes_duplicate_angles_and_one_missing_sample():
    """Two equal angles among three: UNDETERMINED everywhere.  One NaN among four: solved from the other three, by value."""
    frames, _, _, _, _ = make_frames(4, 1, 5, 9, spoil=False)
    dup = pr.design(np.radians([10.0, 10.0, 100.0]))
    got = launch_stokes(frames[:3], None, dup, None, None, (2.0, 4.0))
    assert (got['status'] == pr.UNDETERMINED).all() and torch.isnan(got['tb']).all() and got['counts'].tolist() == [[0, 45, 0, 0]]
    design = pr.design(ANGLES[4])
    frames[2, 0, 1, 3] = np.nan
    got = launch_stokes(frames, None, design, None, None, (2.0, 4.0))
    three = launch_stokes(np.delete(frames, 2, axis=0), None, tuple(np.delete(v, 2) for v in design), None, None, (2.0, 4.0))
    assert got['status'][0, 1, 3] == pr.DETERMINED and got['counts'].tolist() == [[44, 0, 1, 1]]
    for k in ('tb', 'pb', 'pb_cross'):
        assert got[k][0, 1, 3].item() == three[k][0, 1, 3].item(), k


# ---- ratio_depth ---------------------------------------------------------------------------------------------------------------------
def lattice_rays(R, seed=0):
    """The rays and samples of the lattice for the solar radius ``R``: per (b / R, x / b, |d|, side) an observer 215 R away in a
    direction that is no axis, a ray with that impact parameter, and the fp32 ``z`` of the sample x before or behind its
    closest-approach point.  Returns ``(rays_o, rays_d, z)`` float32."""
    rng = np.random.default_rng(seed)
    o, d, z = [], [], []
    for b in pr.LATTICE_B:
        for xb in pr.LATTICE_X:
            for l in pr.LATTICE_L:
                for side in (-1.0, 1.0):
                    e2 = rng.normal(size=3); e2 /= np.linalg.norm(e2)
                    e1 = np.cross(e2, rng.normal(size=3)); e1 /= np.linalg.norm(e1)
                    oo = (b * R * e1 - 215.0 * R * e2).astype(np.float32)
                    dd = (l * e2).astype(np.float32)
                    _, ll, z0, _, bb = (v[0] for v in pr.ray_geometry(oo[None], dd[None]))
                    o.append(oo); d.append(dd); z.append(np.float32(z0 + side * xb * bb / ll))
    return np.stack(o), np.stack(d), np.array(z, dtype=np.float32)


def render_one_sample(rays_o, rays_d, z, R, u):
    """``pixel_b`` [n, 2] of sunerf_thomson_integral_fwd with S = 2, raw = (-80, 0): the first sample, one unit of z before the
    second, carries 10^-80 = 0 in fp32, and the second all the brightness."""
    from sunerf_hip import ops
    n = z.shape[0]
    z_vals = np.stack([z - np.float32(1.0), z], axis=1).astype(np.float32)
    raw = np.zeros((n, 2, 1), dtype=np.float32)
    raw[:, 0] = -80.0
    consts = [torch.tensor([v], dtype=torch.float32).cuda() for v in (R, u, 1.0)]
    out = ops.thomson_integral_fwd(*(torch.from_numpy(v).cuda() for v in (raw, z_vals, rays_o, rays_d)), consts, float(np.log(10.0)))
    return out['pixel_B']


def depth_bound(x_ref, slope_ref, q, x_max):
    """|x_dev - x_ref| <= E_f / |slope| + 2^-23 |x_ref| + x_max 2^-63 + 6 x 2^-24 |q| / |slope|, none of it fitted:

    * E_f = 4 E_F: the restatement's own error in f against longdouble over this lattice (polarimetry_reference.E_F, measured on the
      CPU), times 4 for a device log1p, divide and sqrt that differ from the host's by a few ulp; an error in f moves the root by
      that over the slope;
    * 2^-23 |x_ref|: the fp32 rounding of the depth that comes out (2^-24), and as much again for the fp64 geometry of either side
      (the sample's r^2 from o + d z against b^2 + x^2: 1e-14 relative);
    * x_max 2^-63: what 64 halvings leave of the bracket (half the last interval);
    * the fp32 rounding of the ratio that went in: tB and pB of ``pixel_b`` are each a product rho |I| dl formed in fp32 from three
      factors -- the conversion of |I| and two multiplications round, 3 x 2^-24 relative each -- so pB / tB is off by up to
      6 x 2^-24 |q|, carried through 1 / |slope|."""
    return (4.0 * pr.E_F + 6.0 * 2.0 ** -24 * np.abs(q)) / np.abs(slope_ref) + 2.0 ** -23 * np.abs(x_ref) + x_max * 2.0 ** -63


@pytest.fixture(scope='module')
def lattice():
    """The rays of both solar radii, shared by the tests below and left as they are."""
    return {R: lattice_rays(R, seed=int(100 * R)) for R in pr.LATTICE_R}


@pytest.mark.parametrize('R', pr.LATTICE_R)
@pytest.mark.parametrize('u', pr.LATTICE_U)
def test_ratio_depth_returns_the_sample_the_render_kernel_lit(lattice, R, u):
    from sunerf_hip import polarimetry as pl
    rays_o, rays_d, z = lattice[R]
    n = z.shape[0]
    assert n == len(pr.LATTICE_B) * len(pr.LATTICE_X) * len(pr.LATTICE_L) * 2
    pixel_b = render_one_sample(rays_o, rays_d, z, R, u)
    tb, pb = pixel_b[:, 0].contiguous(), pixel_b[:, 1].contiguous()
    o_t, d_t = torch.from_numpy(rays_o).cuda(), torch.from_numpy(rays_d).cuda()
    out = pl.ratio_depth(tb, pb, o_t, d_t, (R, u))
    torch.cuda.synchronize()
    got = {k: v.cpu().numpy() for k, v in out.items()}
    assert (got['status'] == pr.OK).all(), got['status']
    # the truth: the sample's own distance from the closest-approach point, in longdouble from the fp32 rays and z
    ld = np.longdouble
    _, l, z0, b2, b = pr.ray_geometry(rays_o, rays_d, ld)
    x_ref = np.abs(z.astype(ld) - z0) * l
    h = b / 4096
    slope_ref = ((pr.ratio(x_ref + h, b2, ld(np.float32(R)), ld(np.float32(u))) - pr.ratio(x_ref - h, b2, ld(np.float32(R)), ld(np.float32(u))))
                 / (2 * h)).astype(np.float64)
    q = pb.double().cpu().numpy() / tb.double().cpu().numpy()
    x_ref, l, z0 = x_ref.astype(np.float64), l.astype(np.float64), z0.astype(np.float64)
    bound = depth_bound(x_ref, slope_ref, q, 64.0 * b.astype(np.float64))
    err = np.abs(got['depth'].astype(np.float64) - x_ref)
    worst = int(np.argmax(err / bound))
    print(f'R = {R}, u = {u}: worst depth error / bound {err[worst] / bound[worst]:.3f} at b / R = {float(b[worst]) / R:.3g}, '
          f'x / b = {x_ref[worst] / float(b[worst]):.3g} (error {err[worst]:.3e}, relative {err[worst] / x_ref[worst]:.1e})')
    assert (err <= bound).all(), (err[worst], bound[worst])
    # front or back: the sample before the closest-approach point is z_front, the one behind it z_back -- to the depth bound in
    # units of z and the fp32 rounding of the ray parameter that comes out (z is near 215 R / |d|, its ulp far above the depth's)
    before = z.astype(np.float64) < z0
    hit = np.where(before, got['z_front'], got['z_back']).astype(np.float64)
    z_err = np.abs(hit - z.astype(np.float64))
    z_bound = bound / l + 2.0 ** -24 * np.abs(z.astype(np.float64))
    assert before.sum() == n // 2 and (z_err <= z_bound).all(), float((z_err / z_bound).max())
    other = np.where(before, got['z_back'], got['z_front']).astype(np.float64)
    assert (np.abs(other - (2.0 * z0 - z)) <= z_bound).all()
    # radius and slope against the restatement at the device's own inputs; the restatement's depth within the same bound
    want = pr.ratio_depth(tb.cpu().numpy(), pb.cpu().numpy(), rays_o, rays_d, R, u)
    assert np.array_equal(want['status'], got['status'])
    assert (np.abs(want['depth'].astype(np.float64) - x_ref) <= bound).all()
    assert (np.abs(got['radius'].astype(np.float64) - np.sqrt(b2.astype(np.float64) + x_ref ** 2)) <= bound + 2.0 ** -23 * got['radius']).all()
    # the slope: two values of f, each within 4 E_F of the restatement's, over 2 h, and the fp32 rounding of what comes out
    slope_bound = 2.0 * 4.0 * pr.E_F / (2.0 * h.astype(np.float64)) + 2.0 ** -23 * np.abs(want['slope'])
    assert (np.abs(got['slope'].astype(np.float64) - want['slope']) <= slope_bound).all() and (got['slope'] < 0).all()


def test_ratio_depth_batch_sizes_and_status_cases(lattice):
    """1, 255, 256 and 257 rays give the bits the rays give in the full batch; the status cases sit between ordinary rays, which
    keep their bits."""
    from sunerf_hip import polarimetry as pl
    R, u = 1.0, 0.63
    rays_o, rays_d, z = (np.concatenate([v] * 3)[:257] for v in lattice[R])
    pixel_b = render_one_sample(rays_o, rays_d, z, R, u)
    tb, pb = pixel_b[:, 0].contiguous(), pixel_b[:, 1].contiguous()
    o_t, d_t = torch.from_numpy(rays_o).cuda(), torch.from_numpy(rays_d).cuda()
    full = pl.ratio_depth(tb, pb, o_t, d_t, (R, u))
    assert (full['status'] == pr.OK).all()
    for n in (1, 255, 256):
        part = pl.ratio_depth(tb[:n].contiguous(), pb[:n].contiguous(), o_t[:n].contiguous(), d_t[:n].contiguous(), (R, u))
        again = pl.ratio_depth(tb[:n].contiguous(), pb[:n].contiguous(), o_t[:n].contiguous(), d_t[:n].contiguous(), (R, u))
        for k in pl.DEPTH_OUTPUTS:
            assert torch.equal(part[k].view(torch.uint8), full[k][:n].view(torch.uint8)), (n, k)
            assert torch.equal(part[k].view(torch.uint8), again[k].view(torch.uint8)), (n, k, 'rerun')
    # the status cases, at odd positions between ordinary rays
    tb2, pb2, o2, d2 = tb[:16].clone(), pb[:16].clone(), o_t[:16].clone(), d_t[:16].clone()
    e = torch.tensor([0.0, 0.0, 1.0]).cuda()
    o2[1], d2[1] = torch.tensor([1.2, 0.0, -215.0]).cuda(), e           # b = 1.2 R: CLOSE
    o2[3], d2[3] = torch.tensor([0.3, 0.2, -215.0]).cuda(), e           # a disc ray: CLOSE
    d2[5] = 0.0                                                         # d = 0: DEGENERATE
    tb2[7] = float('nan')                                               # INVALID
    tb2[9] = 0.0                                                        # tb <= 0: INVALID
    pb2[11] = -pb2[11]                                                  # pb < 0: BELOW, x the far end
    o2[13], d2[13] = torch.tensor([2.0, 0.0, -215.0]).cuda(), e        # a ratio 1 % above f(0): ABOVE, x = 0
    f0 = float(pr.ratio(np.float64(0.0), np.float64(4.0), np.float64(R), np.float64(np.float32(u))))
    tb2[13], pb2[13] = 1.0, 1.01 * f0
    pb2[15] = float('inf')                                              # INVALID
    got = pl.ratio_depth(tb2, pb2, o2, d2, (R, u))
    torch.cuda.synchronize()
    status = got['status'].cpu().tolist()
    assert [status[i] for i in (1, 3, 5, 7, 9, 11, 13, 15)] == [pr.CLOSE, pr.CLOSE, pr.DEGENERATE, pr.INVALID, pr.INVALID, pr.BELOW,
                                                              pr.ABOVE, pr.INVALID], status
    for i in (1, 3, 5, 7, 9, 15):
        assert all(torch.isnan(got[k][i]) for k in ('depth', 'z_front', 'z_back', 'radius', 'slope')), i
    _, l, z0, _, b = pr.ray_geometry(o2.cpu().numpy(), d2.cpu().numpy())
    assert got['depth'][13].item() == 0.0 and got['z_front'][13].item() == got['z_back'][13].item() == np.float32(z0[13])
    assert got['radius'][13].item() == 2.0
    assert got['depth'][11].item() == np.float32(64.0 * b[11]) and got['z_back'][11].item() == np.float32(z0[11] + 64.0 * b[11] / l[11])
    want = pr.ratio_depth(tb2.cpu().numpy(), pb2.cpu().numpy(), o2.cpu().numpy(), d2.cpu().numpy(), R, u)
    assert want['status'].tolist() == status
    for i in range(0, 16, 2):
        for k in pl.DEPTH_OUTPUTS:
            assert torch.equal(got[k][i:i + 1].view(torch.uint8), full[k][i:i + 1].view(torch.uint8)), (i, k)
    # depth_sigma of the wrapper
    sigma = torch.full((16,), 1e-3).cuda()
    with_sigma = pl.ratio_depth(tb2, pb2, o2, d2, (R, u), ratio_sigma=sigma)
    assert torch.equal(with_sigma['depth_sigma'][::2], (sigma / got['slope'].abs())[::2])


# ---- end to end ----------------------------------------------------------------------------------------------------------------------
def test_a_render_polarised_and_solved_is_the_render_and_feeds_the_pool():
    """A SimpleStar through ThompsonScattering on a 24 x 24 view from 1 AU, ``polarise`` at 0 / 60 / 120 degrees, ``stokes`` without
    noise: tB and pB come back to the fp32 rounding of the three frames.  The bound is the restatement's: a frame value carries
    2^-24 relative, the solve is linear, and its rows are I = 2/3 sum y_k and, rotated, pB = -4/3 sum y_k cos(2 theta_k - 2 phi)
    (the cross term with the sine): the absolute row sums are 2 and at most 4/3 (1 + 1/2 + 1/2) = 8/3 for angles 60 degrees
    apart, so 3 x 2^-24 of the largest frame value of the pixel covers each, with the fp32 rounding of the plane that comes out
    on top (the fp64 roundings of either side are 1e-16)."""
    from sunerf.model.stellar_model import SimpleStar
    from sunerf.rendering.thompson import ThompsonScattering
    from sunerf_hip import polarimetry as pl
    from sunerf_hip.enhance import sun_geometry
    from sunerf_hip.observations import POLARISED_PLANES, ObservationSet
    from sunerf_hip.rays import grid_rays, render_frame
    from sunerf_hip.reprojection import Observer
    torch.manual_seed(3)
    mod = ThompsonScattering(Rs_per_ds=1.0, model=SimpleStar, model_config={},
                             sampling_config={'type': 'stratified', 'n_samples': 24, 'perturb': False},
                             hierarchical_sampling_config={'type': 'hierarchical', 'n_samples': 24}).cuda()
    res, lat, lon, dist = 24, 0.1, 0.4, 215.032
    axis = torch.linspace(-0.02, 0.02, res, dtype=torch.float64, device='cuda')          # +-4.3 solar radii from 1 AU
    observer = Observer(lat, lon, dist, tx=axis, ty=axis)
    frame = render_frame(mod, axis, axis, observer.c2w, 0.0, keys=('pixel_B',))['pixel_B']
    tb, pb = frame[..., 0].contiguous(), frame[..., 1].contiguous()
    centre, per_radius = sun_geometry(observer)
    assert max(abs(centre[0] - 11.5), abs(centre[1] - 11.5)) < 1e-9 and (tb > 0).all()
    angles = np.radians([0.0, 60.0, 120.0])
    frames = pl.polarise(tb, pb, angles, center=centre)
    assert frames.dtype == torch.float32 and frames.shape == (3, res, res)
    got = pl.stokes(frames, angles, center=centre)
    assert got['tb'].shape == (res, res) and (got['status'] == pl.DETERMINED).all() and got['counts'].tolist() == [[res * res, 0, 0, 0]]
    biggest = frames.abs().amax(0).double()
    for k, plane in (('tb', tb), ('pb', pb)):
        err = (got[k].double() - plane.double()).abs()
        bound = 3.0 * 2.0 ** -24 * biggest + 2.0 ** -24 * plane.double().abs()
        print(f'{k}: worst error / bound {float((err / bound).max()):.3f}')
        assert bool((err <= bound).all()), k
    assert bool((got['pb_cross'].double().abs() <= 3.0 * 2.0 ** -24 * biggest).all())
    # the observation set: the same frames in, the (tB, pB) planes out as the pool's targets
    obs = ObservationSet(Rs_per_ds=1.0, device='cuda')
    spoiled = frames.clone()
    spoiled[1:, 5, 7] = float('nan')          # one valid sample: UNDETERMINED, dropped from the pool
    out = obs.add_polarised_view(spoiled, angles, lat, lon, dist, tx=axis, ty=axis)
    view = obs.views[out['index']]
    assert view.image.shape == (2, res, res) and out['status'][5, 7] == pl.UNDETERMINED and torch.isnan(view.image[:, 5, 7]).all()
    keep = torch.ones(res, res, dtype=torch.bool, device='cuda')
    keep[5, 7] = False
    assert torch.equal(view.image[0][keep], got['tb'][keep]) and torch.equal(view.image[1][keep], got['pb'][keep])
    obs.hold_out(None)
    pool = obs.pool(batch_size=128, seed=0)
    assert pool.n_rays == res * res - 1
    from sunerf_hip.feed import training_batches
    batch = next(iter(training_batches(pool, 1)))['tracing']
    assert batch['target_image'].shape == (128, 2) and torch.isfinite(batch['target_image']).all()
    assert batch['wavelength'].shape == (128, 2) and batch['wavelength'][0].tolist() == list(POLARISED_PLANES)
    # every target row is a (tB, pB) pair of the view
    pairs = torch.stack([view.image[0][keep], view.image[1][keep]], 1)
    assert all(bool((pairs == row).all(1).any()) for row in batch['target_image'][:16])
    # ... and the depth maps of the view: the wrapper over the launch, rays from the view's own grid
    depth = pl.view_ratio_depth(got['tb'], got['pb'], view, mod)
    assert depth['depth'].shape == (res, res) and depth['points_front'].shape == (res, res, 3)
    flat = pl.ratio_depth(got['tb'].reshape(-1), got['pb'].reshape(-1), *grid_rays(axis, axis, view.c2w), (mod.solar_radius, mod.limb_darkening_coeff))
    assert torch.equal(depth['depth'].reshape(-1).view(torch.uint8), flat['depth'].view(torch.uint8))
    ok = depth['status'] == pl.OK
    assert int(ok.sum()) > 100 and int((depth['status'] == pl.CLOSE).sum()) > 20
    r_front = depth['points_front'][ok].norm(dim=-1)
    assert torch.allclose(r_front, depth['radius'][ok], rtol=1e-4) and torch.allclose(depth['points_back'][ok].norm(dim=-1), depth['radius'][ok], rtol=1e-4)
