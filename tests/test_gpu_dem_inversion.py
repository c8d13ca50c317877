"""Per-pixel DEM inversion on MI355X (csrc/dem_inversion.hip: sunerf_dem_invert) against ``scipy.optimize.nnls``
on the stacked system (tests/dem_inversion_reference.py), which shares nothing with the device's algorithm.

Cases: (K, M) in {(2, 1), (21, 2), (101, 7), (128, 8), (101, 6)} -- the kernel is compiled per M and walks K nodes in stores of 32 --
each with N in {1, 63, 64, 65, 257} (a lone lane, both sides of a wave, a second workgroup with one lane), and (101, 7) also with
4099 (17 workgroups, a partial last wave).  Every configuration has a pool of 65 generated pixels with their nnls solutions; a batch
takes pixel i from pool entry i % 65, so the reference is computed once (nnls costs 10 - 20 ms per pixel).

Bound: ``B = max(16 x HOST_WORST, 2^-22)`` with ``dem_inversion_reference.HOST_WORST`` = 2.5e-11 the ceiling tests/test_dem_inversion_host.py asserts for the
float64 restatement of the device's algorithm against nnls on these very pools (measured 2.1e-11), x 16 for another summation
order on the device; 2^-22 because the outputs are fp32 (2^-24) and em adds up to 128 of them.  So B = 2^-22 = 2.4e-7:
  dem        |dem - ref| <= B max_k ref per pixel                                   measured on an MI355X: 5.9e-8
  em         |em - ref| <= B ref;  logt_mean |lm - ref| <= B |ref|                  measured: 6.0e-8, 4.2e-8
  chi2       ``chi2_tolerance``: the residual moves by at most dr = 16 HOST_WORST max x |Gs 1|, chi2 by 2 sqrt(chi2) dr + dr^2 + B chi2
                                                                                    measured: 0.22 of that bound
No pixel of these cases may stop before it met tol (status bit 0); the host test shows the restatement does not (the device took at
most 26 Newton steps per solve, 94 over the 23 solves of a discrepancy pixel).  What is measured is the fp32 rounding of the
outputs (2^-24 = 6.0e-8): the fp64 iterate itself is far below it.
"""
import numpy as np
import pytest
import torch

import dem_inversion_reference as ref
from conftest import load_golden

pytestmark = pytest.mark.gpu

X_REL = 16 * ref.HOST_WORST
B = max(X_REL, 2.0 ** -22)
AIA = (94, 131, 171, 193, 211, 304, 335)
WORST = {}


@pytest.fixture(scope='module')
def inv():
    assert torch.cuda.is_available(), 'GPU tests need a ROCm device'
    from sunerf_hip import dem_inversion
    return dem_inversion


@pytest.fixture(scope='module')
def golden():
    return load_golden('g6_dt_e2e')


def cu(a, dtype=torch.float32):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dtype).cuda()


def same_bits(a, b):
    """Bit-for-bit equality (NaN == NaN)."""
    if a.dtype == torch.float64:
        return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int64), b.contiguous().view(torch.int64))
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def run(inv, c, idx, y=None, sigma=None, **kw):
    """``invert_dem`` on the pool pixels ``idx`` of ``c`` (or on the given y / sigma rows)."""
    y = c['y'][idx] if y is None else y
    sigma = c['sigma'][idx] if sigma is None else sigma
    return inv.invert_dem(cu(y), cu(c['G'], torch.float64), cu(c['nodes']), errors=cu(sigma), prior=cu(c['prior'], torch.float64), **kw)


def compare(got, want, idx, y, sigma, G, what):
    """Device outputs against the reference rows ``want[...][idx]``; updates WORST; returns nothing, asserts."""
    dem, r_dem = got['dem'].double().cpu().numpy(), want['dem'][idx]
    top = r_dem.max(axis=1)
    m = {'dem': (np.abs(dem - r_dem).max(axis=1) / top).max(),
         'em': (np.abs(got['em'].double().cpu().numpy() - want['em'][idx]) / want['em'][idx]).max(),
         'logt_mean': (np.abs(got['logt_mean'].double().cpu().numpy() - want['logt_mean'][idx]) / np.abs(want['logt_mean'][idx])).max()}
    sub = {k: v[idx] for k, v in want.items()}
    tol = ref.chi2_tolerance(sub, y, sigma, G, X_REL, B)
    m['chi2'] = (np.abs(got['chi2'].double().cpu().numpy() - sub['chi2']) / tol).max()
    status = got['status'].cpu().numpy()
    print(f'{what}: ' + ' '.join(f'{k} {v:.2e}' for k, v in m.items()) + f' (chi2 in units of its bound); most steps {(status >> 8).max()}')
    for k, v in m.items():
        WORST[k] = max(WORST.get(k, 0.0), float(v))
    assert (status & 1 == 0).all(), f'{what}: {(status & 1 != 0).sum()} pixels stopped before they met tol'
    assert (status & 0xff == 0).all(), what
    assert m['dem'] <= B and m['em'] <= B and m['logt_mean'] <= B and m['chi2'] <= 1.0, (what, m, B)


@pytest.mark.parametrize('k,m', ref.CONFIGS)
def test_fixed_lam_against_nnls(inv, golden, k, m):
    """lam in {1e-4, 1, 1e4} as one number, then per pixel (pixel i: LAMS[i % 3])."""
    c = ref.pool(golden, k, m)
    sizes = (1, 63, 64, 65, 257) + ((4099,) if (k, m) == (101, 7) else ())
    for n in sizes:
        idx = np.arange(n) % ref.POOL
        for lam in ref.LAMS:
            got = run(inv, c, idx, lam=lam)
            assert got['dem'].shape == (n, k) and got['em'].shape == (n,) and got['status'].dtype == torch.int32
            assert bool((got['lam'] == np.float32(lam)).all())
            compare(got, c['ref'][lam], idx, c['y'][idx], c['sigma'][idx], c['G'], f'K={k} M={m} N={n} lam={lam:g}')
    n = 257 if (k, m) != (101, 7) else 4099
    idx = np.arange(n) % ref.POOL
    which = np.arange(n) % 3
    lam = np.array(ref.LAMS, dtype=np.float32)[which]
    got = run(inv, c, idx, lam=cu(lam))
    assert torch.equal(got['lam'].cpu(), torch.from_numpy(lam))
    for j, one in enumerate(ref.LAMS):
        rows = np.nonzero(which == j)[0]
        part = {key: v[rows] for key, v in got.items() if key in ('dem', 'em', 'logt_mean', 'chi2', 'status')}
        compare(part, c['ref'][one], idx[rows], c['y'][idx[rows]], c['sigma'][idx[rows]], c['G'], f'K={k} M={m} N={n} per-pixel lam={one:g}')
    print('worst so far', WORST, 'bound', B)


def test_fixed_lam_keeps_the_leading_shape_and_the_default_prior(inv, golden):
    """(5, 13, M) in, (5, 13, ...) out; without errors / prior the defaults are used and returned."""
    c = ref.pool(golden, 101, 7)
    y = cu(c['y'][:65]).reshape(5, 13, 7)
    out = inv.invert_dem(y, cu(c['G'], torch.float64), cu(c['nodes']), lam=1.0)
    assert out['dem'].shape == (5, 13, 101) and out['em'].shape == (5, 13) and out['status'].shape == (5, 13)
    assert out['prior'].shape == (101,) and out['prior'].dtype == torch.float64 and out['logt_nodes'].shape == (101,)
    want_prior = inv.flat_prior(y, cu(c['G'], torch.float64))
    assert same_bits(out['prior'], want_prior) and float(want_prior[0]) > 0
    flat = inv.invert_dem(y.reshape(65, 7), cu(c['G'], torch.float64), cu(c['nodes']), errors=inv.default_errors(y).reshape(65, 7),
                          prior=want_prior, lam=torch.full((65,), 1.0).cuda(), want=('dem', 'status'))
    assert set(flat) == {'dem', 'status', 'prior', 'logt_nodes'} and same_bits(flat['dem'], out['dem'].reshape(65, 101))
    with pytest.raises(ValueError, match='unsupported'):
        inv.invert_dem(y, torch.ones(7, 129).cuda(), torch.linspace(5, 7, 129).cuda(), lam=1.0)
    with pytest.raises(ValueError, match='positive'):
        inv.invert_dem(y, cu(c['G'], torch.float64), cu(c['nodes']), lam=0.0)
    for bad in (dict(prior=torch.zeros(101).cuda()), dict(prior=torch.full((101,), float('nan')).cuda())):
        with pytest.raises(ValueError, match='finite'):
            inv.invert_dem(y, cu(c['G'], torch.float64), cu(c['nodes']), lam=1.0, **bad)
    nan_G = cu(c['G'], torch.float64)
    nan_G[3, 50] = float('nan')
    with pytest.raises(ValueError, match='finite'):
        inv.invert_dem(y, nan_G, cu(c['nodes']), lam=1.0)
    empty = inv.invert_dem(y[:0], cu(c['G'], torch.float64), cu(c['nodes']), lam=1.0, prior=want_prior)
    assert empty['dem'].shape == (0, 13, 101) and empty['em'].shape == (0, 13)


def test_value_errors_of_the_entry_point(golden):
    """tol < 0 and a bad [lam_min, lam_max] come after the empty batch, with the null pointers: -1 with every pointer given, and
    nothing is launched (the outputs keep their fill)."""
    import ctypes
    import sunerf_hip
    lib = sunerf_hip.load()
    c = ref.pool(golden, 101, 7)
    y, s, G, p, nodes = cu(c['y'][:4]), cu(c['sigma'][:4]), cu(c['G'], torch.float64), cu(c['prior'], torch.float64), cu(c['nodes'])
    em, status = torch.full((4,), -5.0).cuda(), torch.full((4,), -5, dtype=torch.int32).cuda()
    ptr = lambda t: ctypes.c_void_p(t.data_ptr())      # noqa: E731

    def call(lam_min=1e-4, lam_max=1e4, tol=1e-10, discrepancy=1, n=4):
        return lib.sunerf_dem_invert(ptr(y), ptr(s), ptr(G), ptr(p), ptr(nodes), None, 0, discrepancy, -1.0, lam_min, lam_max, 20, tol,
                                     64, n, 7, 101, None, ptr(em), None, None, None, ptr(status), None)
    assert call(tol=-1.0) == -1 and call(tol=float('nan')) == -1
    assert call(lam_min=0.0) == -1 and call(lam_min=2.0, lam_max=1.0) == -1 and call(lam_max=float('inf')) == -1
    assert call(discrepancy=0) == -1                        # a given lam needs its pointer
    assert call(tol=-1.0, n=0) == 0
    torch.cuda.synchronize()
    assert bool((em == -5.0).all()) and bool((status == -5).all())


def test_exact_cases(inv, golden):
    """y = 0: dem exactly 0 in 0 steps; every y < 0: dem exactly 0; every channel NaN: status 2, dem = 0, logt_mean = NaN; channels
    2 and 5 left out (a NaN y, a zero sigma): the reference on the remaining channels."""
    c = ref.pool(golden, 101, 7)
    y, s = c['y'][:4].copy(), c['sigma'][:4].copy()
    y[0] = 0.0
    y[1] = -y[1]
    y[2] = np.nan
    y[3, 2], s[3, 5] = np.nan, 0.0
    for mode in ('fixed', 'per pixel', 'discrepancy'):
        kw = {'fixed': dict(lam=1.0), 'per pixel': dict(lam=torch.ones(4).cuda()), 'discrepancy': {}}[mode]
        got = run(inv, c, None, y=y, sigma=s, **kw)
        dem, status = got['dem'].cpu(), got['status'].cpu()
        assert bool((dem[0] == 0).all()) and int(status[0]) >> 8 == 0 and got['em'][0].item() == 0, mode
        assert bool((dem[1] == 0).all()) and got['em'][1].item() == 0 and np.isnan(got['logt_mean'][1].item()), mode
        assert int(status[2]) == 2 and bool((dem[2] == 0).all()) and got['em'][2].item() == 0, mode
        assert np.isnan(got['logt_mean'][2].item()) and np.isnan(got['lam'][2].item()) and got['chi2'][2].item() == 0, mode
        assert int(status[3]) & 3 == 0, mode
        lam3 = float(got['lam'][3])
        want = ref.solve_all(y[3:4], s[3:4], c['G'], c['prior'], c['nodes'], np.array([lam3]))
        keep = [0, 1, 3, 4, 6]
        small = ref.invert_reference(y[3, keep], s[3, keep], c['G'][keep], c['prior'], lam3)
        assert np.array_equal(want['dem'][0], small)
        part = {k: v[3:4] for k, v in got.items() if k not in ('prior', 'logt_nodes')}
        part['status'] = part['status'] & ~0xfc          # (discrepancy mode may end at either end of the range)
        compare(part, want, np.arange(1), y[3:4], s[3:4], c['G'], f'channels 2 and 5 left out, {mode}')
    # a lam that is not positive, per pixel: bit 16 and the outputs of an empty pixel; its neighbours are untouched
    lam = torch.tensor([1.0, 0.0, float('nan'), 1.0]).cuda()
    got = run(inv, c, np.arange(4), lam=lam)
    whole = run(inv, c, np.arange(4), lam=1.0)
    assert got['status'][1].item() == 16 and got['status'][2].item() == 16 and bool((got['dem'][1:3] == 0).all())
    assert same_bits(got['dem'][[0, 3]], whole['dem'][[0, 3]])


def _discrepancy_batch(c):
    """257 pixels from 65 unique ones: 63 of the pool, one whose channels no non-negative DEM fits (every other channel x 5, the
    rest x 0.2), one whose errors are 100 x too large."""
    y, s = c['y'][:65].copy(), c['sigma'][:65].copy()
    y[63] = c['y'][0] * np.where(np.arange(7) % 2 == 0, 5.0, 0.2)
    y[63] = y[63].astype(np.float32).astype(np.float64)
    s[63] = c['sigma'][0]
    y[64], s[64] = c['y'][1], (c['sigma'][1] * 100).astype(np.float32).astype(np.float64)
    idx = np.arange(257) % 65
    return y, s, idx


def test_discrepancy_mode(inv, golden):
    """K = 101, M = 7, N = 257, lam_range (1e-4, 1e4), 20 halvings, target = the channels used: dem equals the reference at the
    RETURNED lam; for interior pixels the reference's chi2 at lam x 10^-w is <= target (1 + 1e-9) and at lam x 10^+w >= target
    (1 - 1e-9), w = 2 x 8 / 2^20 dex; the two end cases carry their bit and their end."""
    c = ref.pool(golden, 101, 7)
    y, s, idx = _discrepancy_batch(c)
    got = run(inv, c, None, y=y[idx], sigma=s[idx])
    status, lam = got['status'].cpu().numpy(), got['lam'].double().cpu().numpy()
    assert (status & 3 == 0).all()
    for u in range(65):                       # the copies of one pixel agree in every bit
        rows = np.nonzero(idx == u)[0]
        for k in ('dem', 'em', 'logt_mean', 'chi2', 'lam', 'status'):
            assert same_bits(got[k][rows[1:]], got[k][rows[:1]].expand_as(got[k][rows[1:]])), (u, k)
    first = np.arange(65)
    lam_u, status_u = lam[first], status[first] & 0xff
    assert (lam_u >= np.float32(1e-4)).all() and (lam_u <= np.float32(1e4)).all()
    assert status_u[63] == 4 and lam_u[63] == np.float32(1e-4)
    assert status_u[64] == 8 and lam_u[64] == np.float32(1e4)
    interior = np.nonzero(status_u == 0)[0]
    assert len(interior) >= 48 and set(status_u) == {0, 4, 8}
    want = ref.solve_all(y, s, c['G'], c['prior'], c['nodes'], lam_u)
    part = {k: v[:65] for k, v in got.items() if k not in ('prior', 'logt_nodes')}
    part['status'] = part['status'] & ~0xfc          # the bracket bits are checked above
    compare(part, want, first, y, s, c['G'], 'discrepancy, at the returned lam')
    w = 2 * 8.0 / 2 ** 20
    target = 7.0
    below = ref.solve_all(y[interior], s[interior], c['G'], c['prior'], c['nodes'], lam_u[interior] * 10.0 ** -w)['chi2']
    above = ref.solve_all(y[interior], s[interior], c['G'], c['prior'], c['nodes'], lam_u[interior] * 10.0 ** w)['chi2']
    print(f'interior {len(interior)}: chi2 / target at lam 10^-w in [{below.min() / target:.8f}, {below.max() / target:.8f}], '
          f'at lam 10^+w in [{above.min() / target:.8f}, {above.max() / target:.8f}]; most steps over all solves {(status >> 8).max()}')
    assert (below <= target * (1 + 1e-9)).all() and (above >= target * (1 - 1e-9)).all()
    ends = ref.solve_all(y[63:65], s[63:65], c['G'], c['prior'], c['nodes'], np.array([1e-4, 1e4], dtype=np.float32).astype(np.float64))
    assert ends['chi2'][0] > target and ends['chi2'][1] < target       # the reference agrees about the ends
    # a target of one's own, and no halvings: the middle of the range
    loose = run(inv, c, np.arange(8), chi2_target=70.0)
    assert bool((loose['lam'][:8] > got['lam'][:8]).all())
    mid = run(inv, c, np.arange(8), n_bisect=0)
    assert bool((mid['lam'] == 1.0).all()) and bool((mid['status'] & 0xff == 0).all())


def test_determinism_batches_and_tiles(inv, golden):
    """Two runs give identical bits in every output; pixels 0, 64 and 4098 of the 4099 batch have the bits of the same pixels
    solved alone; ``tile_pixels = 100`` gives the bits of one call -- with a given lam and in discrepancy mode."""
    c = ref.pool(golden, 101, 7)
    y, s, idx65 = _discrepancy_batch(c)
    idx = np.arange(4099) % 65
    for kw in (dict(lam=1e-2), {}):
        a = run(inv, c, None, y=y[idx], sigma=s[idx], **kw)
        b = run(inv, c, None, y=y[idx], sigma=s[idx], **kw)
        tiled = run(inv, c, None, y=y[idx], sigma=s[idx], tile_pixels=100, **kw)
        keys = ('dem', 'em', 'logt_mean', 'chi2', 'lam', 'status')
        for k in keys:
            assert same_bits(a[k], b[k]), k
            assert same_bits(a[k], tiled[k]), k
        for p in (0, 64, 4098):
            alone = run(inv, c, None, y=y[idx[p:p + 1]], sigma=s[idx[p:p + 1]], **kw)
            for k in keys:
                assert same_bits(alone[k], a[k][p:p + 1]), (k, p)


# ---- through the model ------------------------------------------------------------------------------------------------------
def _star(n_samples=24):
    from sunerf.model.stellar_model import SimpleStar
    from sunerf.rendering.density_temperature import DensityTemperatureRadiativeTransfer
    g = load_golden('g9_simple_star')
    mod = DensityTemperatureRadiativeTransfer(
        Rs_per_ds=1, model=SimpleStar, model_config={},
        sampling_config={'type': 'stratified', 'n_samples': n_samples, 'perturb': False},
        hierarchical_sampling_config={'type': 'hierarchical', 'n_samples': n_samples, 'perturb': False},
        pixel_intensity_factor=float(g['pixel_intensity_factor']),
        response_table=(g['aia_logte'].numpy(), g['aia_tresp'].numpy())).cuda()
    with torch.no_grad():
        for m in (mod.coarse_model, mod.fine_model):
            for w in AIA:
                m.log_absortpion[str(w)].fill_(0.0)          # optically thin
    return mod


def _pearson(a, b):
    a, b = a - a.mean(), b - b.mean()
    return float((a @ b) / np.sqrt((a @ a) * (b @ b)))


def test_through_the_model(inv):
    """A SimpleStar DT rendering, 33 x 33 rays, optically thin, default nodes: ``invert_dem`` of ``forward``'s image (default
    errors, discrepancy mode), folded back, reproduces the image within the solver's chi2; its em and logt_mean are scored against
    ``render_dem`` of the same rays, and so is the float64 reference inversion of the same image at the same lam (every 9th
    pixel: 121 nnls solves): the device reproduces the reference's scores.

    chi2: a returned interior lam is the middle of a bracket [lo, hi] of 8 / 2^20 dex with chi2(lo) <= target, and
    d ln chi2 / d ln lam <= 2 (each residual component scales like lam / (lam + a), a >= 0), so chi2 <= target 10^(8 / 2^20)
    = target (1 + 1.8e-5); 2e-5 + B with the fp32 output.
    Scores: em within B relative moves log10 em by B / ln 10, the Pearson coefficient by at most 2 |delta| / |centred log em|;
    logt_mean within B relative moves the MAE by at most B max |logt_mean|.
    Measured on an MI355X: device and reference both Pearson 0.990280 and MAE 0.098623 dex on the 121 pixels (dem within 5.6e-8); 1077
    of the 1089 pixels interior, 12 at lam_max, chi2 / target up to 1.0000101.  The thresholds on the scores themselves are set a
    little beyond those figures: they guard the comparison, the equality with the reference is the check."""
    from sunerf_hip import dem as demlib
    from sunerf_hip.rays import observer_rays
    mod = _star()
    o, d = observer_rays(33, device='cuda')
    t = torch.full((o.shape[0], 1), 0.4, device='cuda')
    n = o.shape[0]
    assert n == 33 * 33
    wl = torch.tensor(AIA, dtype=torch.float32, device='cuda').expand(n, 7).contiguous()
    with torch.no_grad():
        image = mod(o, d, t, wl)['image']
    model = mod.render_dem(o, d, t)
    out = mod.invert_dem(image)
    assert out['dem'].shape == (n, 101) and torch.equal(out['logt_nodes'], mod.response_logte[0])
    status = out['status'].cpu().numpy()
    assert (status & 1 == 0).all()
    lit = (image > 0).all(dim=1).cpu().numpy()
    interior = (status & 0xff) == 0
    print(f'pixels: {n}, lit {lit.sum()}, interior {interior.sum()}, at lam_min {(status & 4 != 0).sum()}, at lam_max '
          f'{(status & 8 != 0).sum()}, no channel {(status & 2 != 0).sum()}')
    assert interior.sum() >= n // 2
    # folded back: the image within the solver's chi2
    G = mod.inversion_response()
    sigma = inv.default_errors(image).double()
    folded = demlib.fold(out['dem'].double(), G)
    chi2_fold = (((folded - image.double()) / sigma) ** 2).sum(dim=1).cpu().numpy()
    chi2 = out['chi2'].double().cpu().numpy()
    print(f'interior chi2 / target: solver up to {chi2[interior].max() / 7:.8f}, folded back up to {chi2_fold[interior].max() / 7:.8f}')
    assert (chi2[interior] <= 7 * (1 + 2e-5 + B)).all()
    # folding the fp32 dem back: each node within 2^-24, the whitened residual within 2^-24 |Gs x| <= 2^-24 sum_w y / sigma
    dr = 2.0 ** -24 * np.linalg.norm((image.double() / sigma).cpu().numpy(), axis=1)
    assert (np.abs(chi2_fold - chi2) <= 2 * np.sqrt(chi2) * dr + dr * dr + B * chi2)[interior].all()
    # scores against the model's own line-of-sight DEM, device and reference on every 9th pixel
    sub = np.arange(0, n, 9)
    sub = sub[(status[sub] & 2) == 0]
    y64, s64 = image.double().cpu().numpy()[sub], sigma.cpu().numpy()[sub]
    lam = out['lam'].double().cpu().numpy()[sub]
    G64, prior, nodes = G.cpu().numpy(), out['prior'].cpu().numpy(), out['logt_nodes'].double().cpu().numpy()
    want = ref.solve_all(y64, s64, G64, prior, nodes, lam)
    got = {k: out[k].double().cpu().numpy()[sub] for k in ('dem', 'em', 'logt_mean')}
    top = want['dem'].max(axis=1)
    ok = top > 0
    worst = (np.abs(got['dem'] - want['dem']).max(axis=1)[ok] / top[ok]).max()
    print(f'device vs reference inversion on {ok.sum()} pixels: dem {worst:.2e} of the largest node (bound {B:.2e})')
    assert worst <= B
    em_model, lt_model = model['em'].double().cpu().numpy()[sub], model['logt_mean'].double().cpu().numpy()[sub]
    both = ok & (got['em'] > 0) & (em_model > 0)
    assert both.sum() >= 60
    scores = {}
    for name, r in (('device', got), ('reference', want)):
        scores[name] = (_pearson(np.log10(r['em'][both]), np.log10(em_model[both])), float(np.abs(r['logt_mean'][both] - lt_model[both]).mean()))
        print(f'{name}: Pearson of log10 em {scores[name][0]:.6f}, MAE of logt_mean {scores[name][1]:.6f} dex ({both.sum()} pixels)')
    centred = np.log10(want['em'][both]) - np.log10(want['em'][both]).mean()
    d_pearson = 2 * (B / np.log(10)) * np.sqrt(both.sum()) / np.linalg.norm(centred)
    assert abs(scores['device'][0] - scores['reference'][0]) <= d_pearson
    assert abs(scores['device'][1] - scores['reference'][1]) <= B * np.abs(want['logt_mean'][both]).max()
    assert scores['device'][0] >= PEARSON_MIN and scores['device'][1] <= MAE_MAX


# thresholds of the comparison with the model's own DEM, stated after measuring them on an MI355X (see the docstring's figures)
PEARSON_MIN, MAE_MAX = 0.985, 0.11


def test_loader_inverts_a_frame(inv):
    """``ModelLoader.invert_dem_image`` on its own rendered frame: the leading shape is kept, numpy out by default, the device
    result is ``invert_dem``'s."""
    from sunerf.evaluation.loader import ModelLoader
    mod = _star()
    loader = ModelLoader(rendering=mod, model=mod.fine_model,
                         ref_map={'shape': (16, 16), 'cdelt': (150., 150.), 'meta': {'t_obs': '2022-01-01T00:00:00.000'}})
    frame = loader.render_observer_image(0.1, 0.3, 0.4, wl=np.array(AIA), as_numpy=False)['image']
    assert frame.shape == (16, 16, 7)
    out = loader.invert_dem_image(frame, as_numpy=False)
    direct = mod.invert_dem(frame)
    for k in direct:
        assert same_bits(out[k], direct[k]), k
    assert out['dem'].shape == (16, 16, 101) and out['em'].shape == (16, 16)
    as_np = loader.invert_dem_image(frame.cpu().numpy()[..., 2:5], wl=np.array([171, 193, 211]), lam=1.0, logt_nodes=np.linspace(5.5, 7.0, 21))
    assert isinstance(as_np['dem'], np.ndarray) and as_np['dem'].shape == (16, 16, 21) and as_np['lam'].shape == (16, 16)
    with pytest.raises(ValueError, match='one value per channel'):
        loader.invert_dem_image(frame, wl=np.array([171, 193]))
