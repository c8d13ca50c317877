"""The co-alignment kernels (include/sunerf_hip_coalign.h, csrc/coalign.hip) against the NumPy restatement
tests/coalign_reference.py: by bits on dyadic inputs, where no addition can round in any order; to the bound of any summation
order on general inputs; and, through ``coalign`` and ``ObservationSet.coalign_view``, the recovery of a known pointing error.

The shapes are the smallest at which the kernel can go wrong, with the two seams at the constants the kernel chose: a run holds
several tiles only when a plane has more tiles than ``max(1, 256 / n_planes)`` runs, so that case is 16 planes of 96 x 192 (18
tiles, 16 runs; one plane of 288 x 256 would have 72 tiles and 72 runs), and 33 x 33 = 1089 shifts are two chunks of 545."""
import datetime
import math

import numpy as np
import pytest
import torch

import coalign_reference as cr

pytestmark = pytest.mark.gpu

# (planes, H, W, max_dy, max_dx)
SHAPES = [(1, 1, 1, 0, 0), (1, 1, 1, 2, 3), (1, 1, 40, 0, 3), (1, 40, 1, 3, 0), (1, 5, 7, 8, 8), (2, 33, 65, 2, 5), (3, 64, 64, 1, 1),
          (2, 65, 97, 16, 16), (1, 40, 70, 32, 32), (16, 96, 192, 2, 2), (7, 19, 70, 3, 3)]
FSUM_PAIRS = 1_000_000          # math.fsum on the cases with at most this many (pixel, shift) pairs; np.longdouble above
IDS = ['x'.join(map(str, s)) for s in SHAPES]


def _bits(x):
    return np.ascontiguousarray(x, dtype=np.float64).view(np.int64)


def _dev(x):
    return torch.from_numpy(np.ascontiguousarray(x)).cuda()


def _masks(rng, shape):
    bad_i = (rng.random(shape) < 0.1).astype(np.uint8) * rng.integers(1, 256, shape).astype(np.uint8)          # not 0 is bad
    bad_t = (rng.random(shape) < 0.1).astype(np.uint8)
    return bad_i, bad_t


def _spoil(image, templ, bad_t):
    """The 7-plane case: one image plane all NaN, one template plane all bad, +-inf and NaN sprinkled in the others."""
    rng = np.random.default_rng(70)
    image[2] = np.nan
    bad_t[4] = 1
    for x in (image, templ):
        for value in (np.inf, -np.inf, np.nan):
            x[rng.random(x.shape) < 0.02] = value
    image[2] = np.nan


def dyadic_case(shape, masks):
    c, h, w, my, mx = shape
    rng = np.random.default_rng(1000 * h + w + my)
    image = (rng.integers(0, 4096, (c, h, w)) / 1024.0).astype(np.float32)
    templ = (rng.integers(0, 4096, (c, h, w)) / 1024.0).astype(np.float32)
    bad_i, bad_t = _masks(rng, (c, h, w)) if masks else (None, None)
    if c == 7:
        bad_t = np.zeros((c, h, w), dtype=np.uint8) if bad_t is None else bad_t
        _spoil(image, templ, bad_t)
    return image, templ, bad_i, bad_t


def general_case(shape, masks):
    c, h, w, my, mx = shape
    rng = np.random.default_rng(2000 * h + w + mx)
    scale = 10.0 ** rng.integers(-3, 4, (c, h, w))
    image = (rng.standard_normal((c, h, w)) * scale).astype(np.float32)
    templ = (rng.standard_normal((c, h, w)) * 10.0 ** rng.integers(-3, 4, (c, h, w))).astype(np.float32)
    bad_i, bad_t = _masks(rng, (c, h, w)) if masks else (None, None)
    if c == 7:
        bad_t = np.zeros((c, h, w), dtype=np.uint8) if bad_t is None else bad_t
        _spoil(image, templ, bad_t)
    return image, templ, bad_i, bad_t


def device_sums(image, templ, bad_i, bad_t, my, mx):
    from sunerf_hip.coalign import shift_sums
    return shift_sums(_dev(image), _dev(templ), (my, mx), None if bad_i is None else _dev(bad_i), None if bad_t is None else _dev(bad_t))


@pytest.mark.parametrize('masks', [False, True], ids=['plain', 'masked'])
@pytest.mark.parametrize('shape', SHAPES, ids=IDS)
def test_dyadic_inputs_give_the_restatements_bits(shape, masks):
    """Values k / 1024, 0 <= k < 4096: every term is a multiple of 2^-20 below 2^4, every partial sum of at most 96 x 192 of them
    stays below 2^33 -- far inside 2^53 2^-20 -- so no addition rounds, in the kernel's order or in NumPy's."""
    c, h, w, my, mx = shape
    image, templ, bad_i, bad_t = dyadic_case(shape, masks)
    got = device_sums(image, templ, bad_i, bad_t, my, mx)
    assert got.shape == (c, 2 * my + 1, 2 * mx + 1, 6) and got.dtype == torch.float64 and got.is_cuda
    want = cr.shift_sums(image, templ, my, mx, bad_i, bad_t)
    differ = int((_bits(got.cpu().numpy()) != _bits(want)).sum())
    print(f'{shape} masks={masks}: {differ} of {want.size} sums differ in bits; pairs per shift {int(want[..., 0].min())} .. {int(want[..., 0].max())}')
    assert differ == 0
    if c == 7:
        assert not want[2].any() and not want[4].any() and want[0, ..., 0].max() > 0
    if (h, w) == (1, 1) and my:
        assert int((want[..., 0] > 0).sum()) == 1          # only the zero shift overlaps


@pytest.mark.parametrize('masks', [False, True], ids=['plain', 'masked'])
@pytest.mark.parametrize('shape', SHAPES, ids=IDS)
def test_general_inputs_stay_inside_the_bound_of_any_summation_order(shape, masks):
    """Random fp32 of mixed sign over seven decades: n is exact, and each of the five real sums lies within N 2^-53 sum |term| of
    an exact reference, N the shift's pair count -- the bound of ANY order of fp64 additions of exact terms.  The reference is
    ``math.fsum`` on the small cases and ``np.longdouble`` (64 mantissa bits or more) on the larger ones."""
    c, h, w, my, mx = shape
    image, templ, bad_i, bad_t = general_case(shape, masks)
    n_pairs = c * h * w * (2 * my + 1) * (2 * mx + 1)
    if n_pairs <= FSUM_PAIRS:
        exact = 'fsum'
    elif np.finfo(np.longdouble).nmant >= 63:
        exact = 'longdouble'
    else:
        print(f'{shape}: np.longdouble has {np.finfo(np.longdouble).nmant} mantissa bits: this case is checked in its dyadic form only')
        return
    got = device_sums(image, templ, bad_i, bad_t, my, mx).cpu().numpy()
    want = cr.shift_sums(image, templ, my, mx, bad_i, bad_t, exact=exact)
    bound = cr.sum_bounds(image, templ, my, mx, bad_i, bad_t)
    assert np.array_equal(got[..., 0], want[..., 0])
    err = np.abs(got - want)
    ratio = np.where(bound > 0, err / np.where(bound > 0, bound, 1.0), np.where(err > 0, np.inf, 0.0))
    print(f'{shape} masks={masks} ({exact}): largest error / bound per sum {ratio.reshape(-1, 6).max(0)[1:]}, largest N {int(want[..., 0].max())}')
    assert np.isfinite(got).all() and bool((err <= bound).all())


def test_reruns_streams_and_stale_buffers_do_not_change_a_bit():
    from sunerf_hip import coalign as wrapper
    from sunerf_hip import lib
    from sunerf_hip.ops import _ptr, _stream
    shape = (2, 65, 97, 16, 16)
    image, templ, bad_i, bad_t = general_case(shape, True)
    args = (_dev(image), _dev(templ), _dev(bad_i), _dev(bad_t), 16, 16)
    first = wrapper.launch(*args).clone()
    assert torch.equal(wrapper.launch(*args), first)
    # sums and a workspace of exactly the stated size, both full of NaN
    dev = first.device
    nbytes = int(lib.load().sunerf_coalign_workspace_bytes(*shape))
    for fill in (float('nan'), -1.0):
        sums = torch.full(first.shape, fill, dtype=torch.float64, device=dev)
        ws = torch.full((nbytes // 8,), fill, dtype=torch.float64, device=dev)
        lib.call(dev, 'sunerf_coalign_shift_sums', *(_ptr(t) for t in args[:4]), *shape, _ptr(sums), _ptr(ws), _stream(dev))
        assert torch.equal(sums, first)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        other = wrapper.launch(*args)
    side.synchronize()
    assert torch.equal(other, first)
    assert len({key for key in wrapper._WORKSPACES if key[0] == dev}) >= 2          # one workspace per stream


def test_the_cross_term_agrees_with_the_tap_gradient_kernel():
    """An independent witness on the device: with finite inputs and no masks, Sab is ``sunerf_psf_grad_taps(in=image,
    g_out=template, bin=1, anchor=(max_dy, max_dx), scale=1, BOUNDARY_ZERO)`` with one kernel per plane -- another kernel, another
    order of additions.  The two agree within the sum of their derived bounds: N 2^-53 sum |term| here, (N' + 2) 2^-53 sum |term|
    there (N' = H W: that kernel adds the products with the zeros outside the frame too)."""
    import psf_grad_reference as pr
    from sunerf_hip.psf_fit import tap_gradient
    for shape in ((2, 33, 65, 2, 5), (1, 40, 70, 32, 32), (3, 19, 70, 3, 3)):
        c, h, w, my, mx = shape
        image, templ, _, _ = general_case(shape, False)
        image, templ = np.nan_to_num(image, nan=1.0, posinf=2.0, neginf=-2.0), np.nan_to_num(templ, nan=1.0, posinf=2.0, neginf=-2.0)
        got = device_sums(image, templ, None, None, my, mx)[..., 5].cpu().numpy()
        call = (c, 2 * my + 1, 2 * mx + 1, 1, my, mx, 1.0, pr.ZERO)
        witness = tap_gradient(_dev(image), _dev(templ), *call).cpu().numpy()
        bound = cr.sum_bounds(image, templ, my, mx)[..., 5] + 0.5 * pr.tap_gradient_bound(image, templ, *call)
        err = np.abs(got - witness)
        print(f'{shape}: largest |Sab - tap gradient| / bound {float((err / bound).max()):.3e}')
        assert bool((err <= bound).all())


def test_coalign_on_the_device_finds_the_restatements_peak():
    """The analytic scene of tests/test_coalign_host.py: the integer peak exactly, ``shift`` to 1e-9, and nothing crosses to the
    host on the way."""
    from sunerf_hip.coalign import coalign
    for truth in cr.SCENE_SHIFTS:
        image, templ, bad = cr.scene_pair(*truth)
        want = cr.coalign(image, templ, 8, bad_template=bad)
        got = coalign(_dev(image), _dev(templ), 8, bad_template=_dev(bad))
        assert all(got[k].is_cuda for k in ('shift', 'integer', 'score', 'status', 'scores', 'sums'))
        assert got['integer'].tolist() == want['integer'].tolist() and got['status'].item() == want['status'] == 0
        err = np.abs(got['shift'].cpu().numpy() - want['shift']).max()
        print(f'true shift {truth}: device {got["shift"].tolist()}, restatement {want["shift"].tolist()}, difference {err:.2e}')
        assert err <= 1e-9 and abs(got['score'].item() - want['score']) <= 1e-12
        planes = coalign(_dev(np.concatenate([image, image])), _dev(np.concatenate([templ, templ])), (8, 8), combine='planes',
                         bad_template=_dev(np.concatenate([bad, bad])), measure='ssd')
        ssd = cr.coalign(image, templ, 8, bad_template=bad, measure='ssd')
        assert planes['integer'].tolist() == [ssd['integer'].tolist()] * 2
        assert np.abs(planes['shift'].cpu().numpy() - ssd['shift']).max() <= 1e-9


# ---- through the observation set ------------------------------------------------------------------------------------------------------
N_VIEWS, N_PX = 8, 64
GRID = {'shape': (N_PX, N_PX), 'cdelt': (2400. / N_PX, 2400. / N_PX)}
SPOTS = [(0.3, 0.2, 0.15, 0.8), (-0.2, -0.5, 0.1, 1.2), (0.1, -1.1, 0.2, 0.6), (-0.4, 0.9, 0.12, 1.0), (0.5, -0.3, 0.08, 1.5),
         (0.0, 0.5, 0.1, 0.9)]          # latitude, longitude, width [rad] and amplitude of the bright regions


def _surface_and_corona(rays_o, rays_d):
    """The scene of tests/test_gpu_reprojection.py::_disk_and_corona with the disk made a SURFACE: 0.25 (1 + bright regions fixed
    in latitude and longitude) where the ray meets the sphere, the same falling corona off it.  The reprojection baseline assumes
    emission from the surface; the limb darkening of the original scene depends on the viewing angle, and on the fp64
    restatement the baseline of eight such views missed a 3-pixel displacement by up to 1.3 px (scores near 0.5)."""
    d = rays_d / rays_d.norm(dim=-1, keepdim=True)
    od = (rays_o * d).sum(-1)
    b2 = (rays_o * rays_o).sum(-1) - od * od          # squared impact parameter in solar radii
    b = b2.clamp_min(0).sqrt()
    p = rays_o + d * (-od - (1 - b2).clamp_min(0).sqrt())[..., None]
    lat, lon = torch.atan2(-p[..., 2], torch.hypot(p[..., 0], p[..., 1])), torch.atan2(-p[..., 0], p[..., 1])
    spots = torch.zeros_like(b)
    for bl, ll, sg, amp in SPOTS:
        cosd = torch.sin(lat) * math.sin(bl) + torch.cos(lat) * math.cos(bl) * torch.cos(lon - ll)
        spots = spots + amp * torch.exp(-torch.acos(cosd.clamp(-1, 1)) ** 2 / (2 * sg * sg))
    return torch.where(b < 1, 0.25 * (1 + spots), 0.06 * torch.exp(-(b - 1) / 0.12)).float()


def _render(grid, lat, lon, dist):
    from sunerf.evaluation.loader import linear_plate_scale_axes
    from sunerf_hip.rays import grid_rays, pose_spherical
    tx, ty = linear_plate_scale_axes(grid, None, 'cuda')
    o, d = grid_rays(tx, ty, pose_spherical(-lon, lat, dist))
    return _surface_and_corona(o.double(), d.double()).reshape(grid['shape'])


def _set_of_eight(displaced, ey, ex, with_grid=True):
    """Eight views all around the Sun, as ``_set_of_four`` / ``test_baseline_of_an_analytic_disk_and_corona`` build theirs; view
    ``displaced`` is added with its crpix off by (ex, ey) pixels -- the image is what the TRUE grid sees."""
    from sunerf.evaluation.loader import linear_plate_scale_axes
    from sunerf_hip.observations import ObservationSet
    obs = ObservationSet(device='cuda', wavelength=193)
    t0 = datetime.datetime(2022, 1, 1)
    poses = [(0.1 * (k % 3 - 1), 0.3 - (2 * math.pi / N_VIEWS) * k, 215.032) for k in range(N_VIEWS)]
    wrong = dict(GRID, crpix=((N_PX + 1) / 2 + ex, (N_PX + 1) / 2 + ey))
    for k, pose in enumerate(poses):
        grid = wrong if k == displaced else GRID
        kw = dict(grid=grid) if with_grid else dict(zip(('tx', 'ty'), linear_plate_scale_axes(grid, None, 'cuda')))
        obs.add_view(_render(GRID, *pose), *pose, time=t0 + datetime.timedelta(hours=k), **kw)
    return obs, poses, wrong


@pytest.mark.parametrize('with_grid', [True, False], ids=['grid', 'axes'])
def test_a_displaced_view_is_put_back_exactly_against_its_own_render(with_grid):
    """``reference``: what the scene looks like on the view's (wrong) grid -- the render a perfect model would give.  It is the
    view's image moved by whole pixels, bit for bit, so the score is exactly 1, the shift exactly minus the displacement, and
    ``tx`` / ``ty`` come back to 1e-12 of a pixel."""
    from sunerf.evaluation.loader import ARCSEC, linear_plate_scale_axes
    ey, ex, i = -2, 3, 2
    obs, poses, wrong = _set_of_eight(i, ey, ex, with_grid)
    true_tx, true_ty = linear_plate_scale_axes(GRID, None, 'cuda')
    view = obs.views[i]
    assert (view.tx - true_tx).abs().max() > 2.9 * GRID['cdelt'][0] * ARCSEC
    obs.pool(batch_size=64)
    assert obs._tables
    dry = obs.coalign_view(i, reference=_render(wrong, *poses[i])[None], apply=False)
    assert not dry['applied'] and dry['shift'].tolist() == [-ey, -ex] and (view.tx - true_tx).abs().max() > 0 and obs._tables
    out = obs.coalign_view(i, reference=_render(wrong, *poses[i])[None])
    print(f'displacement (ey, ex) = ({ey}, {ex}): shift {out["shift"].tolist()}, score {out["score"].item()!r}, status {out["status"].item()}')
    assert out['applied'] and out['shift'].tolist() == [-ey, -ex] == out['integer'].tolist() and out['status'].item() == 0
    tol = 1e-12 * GRID['cdelt'][0] * ARCSEC
    err_x, err_y = (view.tx - true_tx).abs().max().item(), (view.ty - true_ty).abs().max().item()
    print(f'restored axes: largest |tx - true| {err_x:.2e} rad, |ty - true| {err_y:.2e} rad (gate {tol:.2e})')
    assert err_x <= tol and err_y <= tol and not obs._tables
    if with_grid:
        assert view.grid['crpix'] == ((N_PX + 1) / 2, (N_PX + 1) / 2) and view.grid['cdelt'] == GRID['cdelt']
    else:
        assert view.grid is None


def test_the_baseline_recovers_a_displacement_to_half_a_pixel():
    """``reference='baseline'``: the synchronic map of the seven other views seen from the displaced view's pose on its (wrong)
    grid, NaN off the disk.  Within 0.5 px of the truth; on the fp64 restatement of the reprojection this scene gave 0.11 px
    (score 0.85) for this view and 0.09 to 0.11 px for two others."""
    from sunerf.evaluation.loader import ARCSEC, linear_plate_scale_axes
    ey, ex, i = -2, 3, 2
    obs, poses, wrong = _set_of_eight(i, ey, ex)
    out = obs.coalign_view(i, reference='baseline', shape=(181, 361))
    dy, dx = out['shift'].tolist()
    err = math.hypot(dy + ey, dx + ex)
    print(f'baseline of 7 views: shift ({dy:+.4f}, {dx:+.4f}) for a displacement (ey, ex) = ({ey}, {ex}): error {err:.4f} px; score '
          f'{out["score"].item():.4f}, status {out["status"].item()}')
    assert out['applied'] and out['status'].item() == 0 and err <= 0.5
    true_tx, true_ty = linear_plate_scale_axes(GRID, None, 'cuda')
    px = GRID['cdelt'][0] * ARCSEC
    assert (obs.views[i].tx - true_tx).abs().max().item() <= 0.5 * px and (obs.views[i].ty - true_ty).abs().max().item() <= 0.5 * px


def test_coalign_views_moves_every_view_but_the_anchor_towards_the_truth():
    """Two passes with view 0 as the anchor and view 7 held out.  A view that looks at the bland far side of the scene has nothing
    to correlate: its peak lies on the border of the window (EDGE) and it is left where it is.  Every view that is moved ends
    within the 0.5 px of the baseline test of its true pointing."""
    from sunerf_hip.coalign import EDGE, NO_PEAK
    ey, ex, i = -2, 3, 2
    obs, poses, wrong = _set_of_eight(i, ey, ex)
    obs.hold_out([7])
    history = obs.coalign_views(anchor=0, passes=2, shape=(181, 361))
    assert len(history) == 2 and sorted(history[0]) == sorted(history[1]) == [1, 2, 3, 4, 5, 6]
    for k, result in enumerate(history):
        for j, r in result.items():
            print(f"pass {k + 1}, view {j}: shift ({r['shift'][0]:+.3f}, {r['shift'][1]:+.3f}), status {r['status']}, score {r['score']:.4f}, "
                  f"applied {r['applied']}")
            assert r['applied'] == (not r['status'] & (NO_PEAK | EDGE))
    assert history[0][i]['applied'] and history[0][1]['applied'] and history[0][3]['applied']
    centre = ((N_PX + 1) / 2, (N_PX + 1) / 2)
    assert obs.views[0].grid['crpix'] == centre and obs.views[7].grid['crpix'] == centre          # the anchor and the held-out view stay
    worst = 0.0
    for j in history[0]:
        moved = [sum(h[j]['shift'][k] for h in history if h[j]['applied']) for k in (0, 1)]
        cpx, cpy = obs.views[j].grid['crpix']
        start = wrong['crpix'] if j == i else centre
        assert abs(cpx - (start[0] + moved[1])) <= 1e-12 and abs(cpy - (start[1] + moved[0])) <= 1e-12          # crpix moved by (dx, dy)
        if any(h[j]['applied'] for h in history):
            worst = max(worst, math.hypot(cpx - centre[0], cpy - centre[1]))
        else:
            assert (cpx, cpy) == start
    print(f'largest residual pointing error of the views that were moved: {worst:.4f} px')
    assert worst <= 0.5
