"""The instrument kernels on the device (include/sunerf_hip_instrument.h) against scipy and against the fp64
restatement tests/instrument_reference.py.  Every test prints what it measured before it asserts.

Tiles (csrc/instrument.hip): the correlation works on T x T output pixels per workgroup, T = min(32, (127 - max(kh, kw)) / bin + 1)
-- 32 for the small kernels here, 7 for the 72-tap and 4 for the 96-tap kernel with bin 8; the noise and Philox kernels take 256
elements per workgroup, so 4099 counters are sixteen workgroups plus three."""
import numpy as np
import pytest
import torch

import instrument_reference as ir

pytestmark = pytest.mark.gpu

KNOWN_ANSWERS = [
    ((0, 0, 0, 0), (0, 0), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
    ((0xffffffff,) * 4, (0xffffffff,) * 2, (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
    ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0), (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1)),
]


def _bits(t):
    return t.detach().cpu().contiguous().view(torch.int32)


def _u32(t):
    return t.cpu().numpy().view(np.uint32)


# ---- 7. Philox ------------------------------------------------------------------------------------------------------------------
def test_philox_on_the_device():
    from sunerf_hip.instrument import philox
    for ctr, key, want in KNOWN_ANSWERS:
        got = _u32(philox(torch.from_numpy(np.array([ctr], dtype=np.uint32).view(np.int32)).cuda(), key[0], key[1]))[0]
        print(' '.join(f'{int(v):08x}' for v in got))
        assert tuple(int(v) for v in got) == want
    rng = np.random.default_rng(5)
    ctr = rng.integers(0, 2 ** 32, (4099, 4), dtype=np.uint64).astype(np.uint32)
    got = _u32(philox(torch.from_numpy(ctr.view(np.int32)).cuda(), 0xDEADBEEF, 0x0BADF00D))
    want = ir.philox(ctr, 0xDEADBEEF, 0x0BADF00D)
    print(f'4099 counters: {int((got != want).any(1).sum())} differ')
    assert np.array_equal(got, want)


# ---- 8. the correlation ---------------------------------------------------------------------------------------------------------
def _block_mean(x, b):
    h, w = x.shape[0] // b * b, x.shape[1] // b * b
    return x[:h, :w].reshape(h // b, b, w // b, b).mean((1, 3))


def _scipy(img, psf, b, boundary):
    """convolve2d(mode='same') / ndimage.convolve(mode='nearest') of every plane in fp64, then the b x b block mean."""
    from scipy import ndimage, signal
    out = []
    for p in range(img.shape[0]):
        k = psf if psf.ndim == 2 else psf[p]
        x = img[p].astype(np.float64)
        if boundary == 'zero':
            full = signal.convolve2d(x, k, mode='same', boundary='fill', fillvalue=0.0)
        else:
            full = ndimage.convolve(x, k, mode='nearest', origin=tuple(-1 if n % 2 == 0 else 0 for n in k.shape))
        out.append(_block_mean(full, b))
    return np.stack(out)


# (planes, H, W, psf shape, bin, per-plane kernels)
CORRELATE_CASES = [
    (1, 5, 7, (9, 9), 1, False),                 # kernel larger than the image
    (1, 1, 1, (3, 3), 1, False),                 # one pixel
    (1, 32, 64, (5, 5), 1, False),               # whole tiles
    (1, 33, 65, (5, 5), 1, False),               # tile + 1
    (3, 34, 67, (5, 5), 1, True),                # ragged, per-plane kernels
    (1, 20, 33, (3, 11), 1, False),
    (1, 33, 20, (11, 3), 1, False),
    (1, 72, 80, (65, 65), 8, False),             # effective 72: tiles of 7
    (1, 40, 48, (89, 89), 8, False),             # effective 96, the limit: tiles of 4
    (1, 37, 53, (7, 5), 1, False),
    (3, 37, 53, (7, 5), 2, False),               # H % b != 0, shared kernel over 3 planes
    (3, 37, 53, (7, 5), 3, True),
    (1, 37, 53, (4, 6), 4, False),               # even PSF
    (3, 70, 99, (9, 9), 2, True),                # several tiles on both axes
]


def _case(c, h, w, shape, per_plane, seed):
    rng = np.random.default_rng(seed)
    img = (rng.random((c, h, w)) * 2000.0 - 300.0).astype(np.float32)
    psf = rng.random(((c,) if per_plane else ()) + shape) - 0.15
    return img, psf / np.abs(psf).sum()


@pytest.mark.parametrize('boundary', ['zero', 'nearest'])
@pytest.mark.parametrize('case', CORRELATE_CASES, ids=lambda c: f'{c[0]}x{c[1]}x{c[2]}-psf{c[3][0]}x{c[3][1]}-b{c[4]}-{"per" if c[5] else "shared"}')
def test_correlation_against_scipy(case, boundary):
    """|got - want| <= 2^-23 |want| + 1e-11 sum|K| max|img| on every output pixel: one rounding to fp32, and an fp64 sum of at
    most 96^2 terms taken in another order (9216 x 2^-53 ~ 1e-12, times ten)."""
    from sunerf_hip.instrument import Instrument
    c, h, w, shape, b, per_plane = case
    img, psf = _case(c, h, w, shape, per_plane, 1000 * h + w + b)
    inst = Instrument(psf=psf, bin=b, boundary=boundary)
    K, _ = inst.effective_kernel()
    x = torch.from_numpy(img).cuda()
    got = inst.expected(x)
    want = _scipy(img, psf, b, boundary)
    assert got.shape == want.shape == (c, h // b, w // b) and got.dtype == torch.float32
    ksum = np.abs(K).sum((1, 2)).max() * inst.scale
    bound = 2.0 ** -23 * np.abs(want) + 1e-11 * ksum * np.abs(img).max()
    err = np.abs(got.cpu().numpy().astype(np.float64) - want)
    print(f'{case} {boundary}: worst |diff| / bound {np.max(err / bound):.3f} over {err.size} pixels')
    assert np.all(err <= bound)
    again = inst.expected(x)
    assert torch.equal(_bits(got), _bits(again))                                        # a rerun gives the same bits
    if c > 1:                                                                           # a plane alone gives the bits of the batch
        alone = Instrument(psf=psf[1] if per_plane else psf, bin=b, boundary=boundary).expected(x[1:2])
        assert torch.equal(_bits(alone[0]), _bits(got[1]))
    ref = ir.correlate_bin(img, K, b, inst.effective_kernel()[1], inst.scale, boundary)[0]
    same = np.array_equal(ref.view(np.int32), got.cpu().numpy().view(np.int32))
    print(f'  the restatement in the header\'s tap order {"agrees" if same else "differs"} by bits')
    assert same


def test_identity_kernel_returns_the_input_by_bits():
    from sunerf_hip.instrument import Instrument
    rng = np.random.default_rng(11)
    img = (rng.standard_normal((2, 33, 65)) * 1e3).astype(np.float32)
    img[0, 0, :4] = [0.0, -0.0, np.inf, 1e-42]
    x = torch.from_numpy(img).cuda()
    for boundary in ('zero', 'nearest'):
        got = Instrument(psf=np.ones((1, 1)), bin=1, boundary=boundary).expected(x)
        print(f'{boundary}: {int((_bits(got) != _bits(x)).sum())} words differ')
        assert torch.equal(_bits(got), _bits(x))
    assert torch.equal(_bits(Instrument().expected(x)), _bits(x))                       # no PSF at all


@pytest.mark.parametrize('boundary,b,pixel', [('zero', 1, (17, 40)), ('zero', 3, (17, 40)), ('nearest', 2, (17, 40)),
                                              ('nearest', 1, (0, 0)), ('zero', 1, (36, 52))])
def test_a_nan_spreads_over_exactly_the_kernels_footprint(boundary, b, pixel):
    """One NaN pixel under a kernel with zero taps: the NaN outputs are exactly those with a tap on the pixel (0 * NaN is NaN)."""
    from sunerf_hip.instrument import Instrument
    rng = np.random.default_rng(2)
    img = rng.random((1, 37, 53)).astype(np.float32)
    img[0][pixel] = np.nan
    psf = rng.random((5, 7))
    psf[1, 2] = psf[4, 6] = psf[0, 0] = 0.0
    inst = Instrument(psf=psf, bin=b, boundary=boundary)
    K, (ay, ax) = inst.effective_kernel()
    got = torch.isnan(inst.expected(torch.from_numpy(img).cuda())).cpu().numpy()[0]
    want = np.zeros_like(got)
    for r in range(got.shape[0]):
        for c in range(got.shape[1]):
            ys, xs = r * b - ay + np.arange(K.shape[1]), c * b - ax + np.arange(K.shape[2])
            if boundary == 'nearest':
                ys, xs = np.clip(ys, 0, 36), np.clip(xs, 0, 52)
            want[r, c] = (ys == pixel[0]).any() and (xs == pixel[1]).any()
    print(f'{boundary} bin {b} NaN at {pixel}: {int(got.sum())} NaN outputs, footprint {int(want.sum())}')
    assert want.sum() > 0 and np.array_equal(got, want)


# ---- 9. the noise against the restatement ----------------------------------------------------------------------------------------
NOISE_SEED, NOISE_OFFSET = 2024, 3 * 2 ** 32 + 11
NOISE_FLAGS = tuple(range(16))           # every combination of POISSON, READ, QUANTISE, SATURATE


def noise_case():
    """3 x 64 x 80, lam from 0 to 1e5 (log-uniform over seven decades) with the special values in plane 0, whose unit, exposure
    and gain are 1; the planes differ in every parameter."""
    rng = np.random.default_rng(77)
    params = np.array([[1.0, 1.0, 1.0, 1.5, 100.0, 3.0e4, 0.0, 0.0],
                       [2.5, 2.9, 1.2, 1.2, 50.0, 5.0e3, 0.0, 0.0],
                       [0.5, 1.0, 2.0, 3.0, 0.0, 1.0e4, 0.0, 0.0]])
    lam = 10.0 ** rng.uniform(-2.0, 5.0, (3, 64, 80))
    x = (lam * (params[:, 2] / (params[:, 0] * params[:, 1]))[:, None, None]).astype(np.float32)
    x[0, 0, :9] = [0.0, -3.0, np.nextafter(np.float32(10.0), np.float32(0.0)), 10.0, np.nan, np.inf, 1e16, 1e5, -np.inf]
    x[1, 0, 0] = x[2, 0, 0] = 0.0
    return x, params


@pytest.fixture(scope='module')
def noise_inputs():
    x, params = noise_case()
    return x, params, torch.from_numpy(x).cuda(), torch.from_numpy(params).cuda()


def _run_noise(x_dev, params_dev, seed, offset, flags, sigma=True, saturated=True):
    from sunerf_hip import lib
    from sunerf_hip.ops import _ptr, _stream
    c, h, w = x_dev.shape
    dev = x_dev.device
    image = torch.empty_like(x_dev)
    sig = torch.empty_like(x_dev) if sigma else None
    sat = torch.empty(x_dev.shape, dtype=torch.uint8, device=dev) if saturated else None
    lib.call(dev, 'sunerf_instrument_noise', _ptr(x_dev), c, h, w, _ptr(params_dev), seed, offset, flags, _ptr(image), _ptr(sig),
             _ptr(sat), _stream(dev))
    return image, sig, sat


@pytest.mark.parametrize('flags', NOISE_FLAGS)
def test_noise_against_the_restatement(noise_inputs, flags):
    """saturated by bytes; image and sigma within 2^-23 |want| + 1e-12 (n g + |pedestal| + read_noise |z|) / (exposure unit); no
    element is left out (tests/test_instrument_host.py checks the same count on the host)."""
    x, params, x_dev, params_dev = noise_inputs
    ref = ir.noise(x, params, NOISE_SEED, NOISE_OFFSET, flags)
    left_out = int((ref['margin'] < ir.MARGIN).sum())
    print(f'flags {flags}: smallest decision margin {ref["margin"].min():.3e}, {left_out} elements left out')
    assert left_out == 0
    image, sigma, sat = _run_noise(x_dev, params_dev, NOISE_SEED, NOISE_OFFSET, flags)
    image, sigma, sat = image.cpu().numpy(), sigma.cpu().numpy(), sat.cpu().numpy()
    valid = ref['valid']
    assert np.array_equal(np.isnan(image), ~valid) and np.array_equal(np.isnan(sigma), ~valid) and not sat[~valid].any()
    print(f'  saturated: {int(sat.sum())} on the device, {int(ref["saturated"].sum())} in the restatement')
    assert np.array_equal(sat, ref['saturated'])
    unit, exposure, g, rn, ped = (params[:, k][:, None, None] for k in range(5))
    with np.errstate(invalid='ignore'):
        slack = 1e-12 * (np.abs(ref['n']) * g + np.abs(ped) + rn * np.abs(ref['z'])) / (exposure * unit)
    for name, got in (('image', image), ('sigma', sigma)):
        want = ref[name].astype(np.float64)
        err = np.abs(got.astype(np.float64) - want)[valid]
        bound = (2.0 ** -23 * np.abs(want) + slack)[valid]
        ratio = np.divide(err, bound, out=np.where(err > 0, np.inf, 0.0), where=bound > 0)
        print(f'  {name}: worst |diff| / bound {ratio.max():.3f}; {int((got.view(np.int32) != ref[name].view(np.int32))[valid].sum())} '
              f'of {int(valid.sum())} differ by bits')
        assert np.all(err <= bound)
    if flags & (ir.POISSON | ir.READ) == 0 and flags & (ir.QUANTISE | ir.SATURATE) == 0:
        want = np.where(x < 0, 0.0, x.astype(np.float64))[valid]          # the unit round trip of the expectation
        rel = np.abs(image.astype(np.float64)[valid] - want) / np.where(want == 0, 1.0, want)
        print(f'  noise-free image against expected: worst relative difference {rel.max():.3e}')
        assert rel.max() <= 2.0 ** -23


def test_sampled_counts_equal_the_restatement(noise_inputs):
    """READ off, unit = exposure = dn_per_photon = 1, no pedestal: the image IS the sampled n, exactly (n < 2^24)."""
    x, _, x_dev, _ = noise_inputs
    params = np.tile(np.array([1.0, 1.0, 1.0, 0.0, 0.0, np.inf, 0.0, 0.0]), (3, 1))
    ref = ir.noise(x, params, NOISE_SEED, NOISE_OFFSET, ir.POISSON)
    left_out = int((ref['margin'] < ir.MARGIN).sum())
    image, _, _ = _run_noise(x_dev, torch.from_numpy(params).cuda(), NOISE_SEED, NOISE_OFFSET, ir.POISSON, False, False)
    got = image.cpu().numpy().astype(np.float64)
    valid = ref['valid']
    differ = int((got[valid] != ref['n'][valid]).sum())
    print(f'{int(valid.sum())} counts up to {ref["n"][valid].max():.0f}: {differ} differ, {left_out} left out, '
          f'smallest margin {ref["margin"].min():.3e}')
    assert left_out == 0 and differ == 0 and ref['n'][valid].max() < 2 ** 24


# ---- 10. distributions on the device, against scipy alone ------------------------------------------------------------------------
def _constant_frame(lam):
    return torch.full((1, 512, 512), lam, dtype=torch.float32, device='cuda')


@pytest.mark.parametrize('lam', ir.DIST_LAMS)
def test_poisson_on_the_device_against_scipy(lam):
    from sunerf_hip.instrument import Instrument
    assert 512 * 512 == ir.DIST_N
    image, _, _ = Instrument().noise(_constant_frame(lam), ir.DIST_SEED, ir.DIST_E0, poisson=True, read=False)
    n = image.cpu().numpy().astype(np.float64).reshape(-1)
    assert np.array_equal(n, np.round(n)) and n.min() >= 0
    unit = float(np.float32(lam))          # the fp32 frame holds lam rounded: that is the rate sampled
    p, bins = ir.chi_square_poisson(n, unit)
    print(f'lam {lam}: chi-square p = {p:.4f} over {bins} bins, mean {n.mean():.4f}')
    assert p >= ir.DIST_GATE


def test_read_noise_on_the_device_against_scipy():
    from scipy import stats
    from sunerf_hip.instrument import Instrument
    image, _, _ = Instrument(read_noise=1.0).noise(_constant_frame(0.0), ir.DIST_SEED, ir.DIST_E0, poisson=False, read=True)
    z = image.cpu().numpy().astype(np.float64).reshape(-1)
    p = stats.kstest(z, 'norm').pvalue
    print(f'KS p = {p:.4f}, mean {z.mean():.4f}, std {z.std():.4f}')
    assert p >= ir.DIST_GATE


# ---- 11. addressing --------------------------------------------------------------------------------------------------------------
def test_addressing():
    from sunerf_hip.instrument import Instrument
    inst = Instrument(read_noise=2.0, pedestal=10.0, dn_per_photon=1.3, quantise=True, saturation=400.0)
    rng = np.random.default_rng(4)
    frame = torch.from_numpy((10.0 ** rng.uniform(-1, 2.7, (1, 64, 80))).astype(np.float32)).cuda()
    whole = inst.noise(frame, seed=99, index_offset=1000)
    rows = inst.noise(frame[:, 17:41].contiguous(), seed=99, index_offset=1000 + 17 * 80)
    for name, a, b in zip(('image', 'sigma', 'saturated'), whole, rows):
        same = torch.equal(a[:, 17:41].cpu(), b.cpu()) if a.dtype == torch.uint8 else torch.equal(_bits(a[:, 17:41]), _bits(b))
        print(f'rows [17, 41) alone against the whole frame, {name}: {"equal" if same else "DIFFERENT"}')
        assert same
    again = inst.noise(frame, seed=99, index_offset=1000)
    other = inst.noise(frame, seed=100, index_offset=1000)
    assert all(torch.equal(a.cpu(), b.cpu()) or torch.equal(_bits(a), _bits(b)) for a, b in zip(whole[:2], again[:2]))
    changed = float((whole[0] != other[0]).float().mean())
    print(f'another seed changes {changed:.3f} of the pixels')
    assert changed > 0.5
    # the photon and the read-noise streams of one element are independent draws
    flat = torch.full((1, 256, 256), 50.0, dtype=torch.float32, device='cuda')
    n = Instrument().noise(flat, seed=5, poisson=True, read=False)[0].cpu().numpy().reshape(-1).astype(np.float64)
    z = Instrument(read_noise=1.0).noise(torch.zeros_like(flat), seed=5, poisson=False, read=True)[0].cpu().numpy().reshape(-1).astype(np.float64)
    r = float(np.corrcoef(n, z)[0, 1])
    print(f'Pearson of n against z over 2^16 pixels: {r:.5f} (bound {4.4 / 256:.5f})')
    assert abs(r) <= 4.4 / np.sqrt(2 ** 16)


# ---- 12. the loaders -------------------------------------------------------------------------------------------------------------
def test_model_loader_observes_a_frame():
    from sunerf.evaluation.loader import ModelLoader
    from sunerf_hip.instrument import Instrument, gaussian_psf
    from sunerf_hip.observations import resampled_grid
    from test_gpu_dem_inversion import AIA, _star
    mod = _star()
    ref_map = {'shape': (32, 32), 'cdelt': (75., 75.), 'meta': {'t_obs': '2022-01-01T00:00:00.000'}}
    loader = ModelLoader(rendering=mod, model=mod.fine_model, ref_map=ref_map)
    fine = loader.render_observer_image(0.1, 0.3, 0.4, wl=np.array(AIA), resolution=64, as_numpy=False)['image']
    assert fine.shape == (64, 64, 7)
    peak = float(fine.max())
    inst = Instrument(psf=gaussian_psf(2.0, 2), bin=2, unit=200.0 / peak, exposure=2.9, dn_per_photon=1.2, read_noise=1.2,
                      quantise=True)
    out = loader.observe_image(0.1, 0.3, 0.4, inst, seed=3, wl=np.array(AIA), as_numpy=False)
    want = inst.expected(fine.permute(2, 0, 1).contiguous()).permute(1, 2, 0).contiguous()
    print(f'expected {tuple(out["expected"].shape)}: {int((_bits(out["expected"]) != _bits(want)).sum())} words differ')
    assert out['expected'].shape == (32, 32, 7) and torch.equal(_bits(out['expected']), _bits(want))
    assert out['image'].shape == out['sigma'].shape == out['saturated'].shape == (32, 32, 7)
    assert out['grid'] == inst.detector_grid(resampled_grid(ref_map, (64, 64)))
    assert out['grid']['shape'] == (32, 32) and out['grid']['cdelt'] == (75., 75.) and out['grid']['crpix'] == (16.5, 16.5)
    assert not torch.equal(out['image'], out['expected']) and not bool(out['saturated'].any())
    as_np = loader.observe_image(0.1, 0.3, 0.4, inst, seed=3, wl=np.array(AIA))
    assert isinstance(as_np['image'], np.ndarray) and np.array_equal(as_np['image'], out['image'].cpu().numpy())
    errors = inst.errors(out['image'])
    assert errors.shape == (32, 32, 7) and bool(torch.isfinite(errors).all()) and bool((errors > 0).all())
    dem = loader.invert_dem_image(out['image'], errors=errors, as_numpy=False)
    chi2 = dem['chi2']
    print(f'invert_dem_image of the observed frame: chi2 from {float(chi2.min()):.3g} to {float(chi2.max()):.3g}')
    assert chi2.shape == (32, 32) and bool(torch.isfinite(chi2).all())
