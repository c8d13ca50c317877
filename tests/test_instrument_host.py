"""CPU-only checks of the instrument model (no GPU): the restatement tests/instrument_reference.py against the
Random123 known answers, scipy's distributions and scipy's convolutions; the fifth entry-point table (declared, bound, kept out
of the other four, its argument checks in their documented order); ``Instrument.errors`` and ``detector_grid``; and the
conditions the cases of tests/test_gpu_instrument.py must meet so that they compare every element."""
import ctypes
import os
import re

import numpy as np
import pytest

import instrument_reference as ir

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KNOWN_ANSWERS = [          # Random123 kat_vectors, philox4x32 10: counter, key, output
    ((0, 0, 0, 0), (0, 0), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
    ((0xffffffff,) * 4, (0xffffffff,) * 2, (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
    ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0), (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1)),
]


@pytest.fixture(scope='session')
def lib():
    import sunerf_hip
    if not os.path.exists(sunerf_hip.LIB_PATH):
        import subprocess
        subprocess.check_call(['bash', os.path.join(ROOT, '2024-hl-spi3s-sunerf_amd', 'csrc', 'build.sh')])
    return sunerf_hip.load()


# ---- 1. the generator -----------------------------------------------------------------------------------------------------------
def test_philox_known_answers():
    for ctr, key, want in KNOWN_ANSWERS:
        got = ir.philox(np.array([ctr], dtype=np.uint32), key[0], key[1])[0]
        print(' '.join(f'{int(v):08x}' for v in got))
        assert tuple(int(v) for v in got) == want
    ua, ub = ir.uniforms(np.arange(4096, dtype=np.uint64), 0, 0, 7)
    assert ua.min() > 0.0 and ua.max() <= 1.0 and ub.min() > 0.0 and ub.max() <= 1.0
    assert np.array_equal(ua * 2.0 ** 53, np.round(ua * 2.0 ** 53))          # exact multiples of 2^-53


# ---- 2. distributions -----------------------------------------------------------------------------------------------------------
def _dist_elements():
    return np.uint64(ir.DIST_E0) + np.arange(ir.DIST_N, dtype=np.uint64)


# the p-values the header's stream gives (seed 2024, e = 5 2^18 + arange(2^18)), to three digits: a restatement that follows the
# header reproduces them (to two digits 0.27, 0.35, 0.44, 0.56, 0.78, 0.97; the normal's KS test 0.37)
P_VALUES = {0.05: 0.265, 3.0: 0.345, 9.99: 0.437, 10.0: 0.555, 37.5: 0.783, 1e4: 0.969}


@pytest.mark.parametrize('lam', ir.DIST_LAMS)
def test_poisson_restatement_against_scipy(lam):
    n, margin, rounds = ir.poisson(np.full(ir.DIST_N, lam), _dist_elements(), ir.DIST_SEED)
    p, bins = ir.chi_square_poisson(n, lam)
    print(f'lam {lam}: chi-square p = {p:.4f} over {bins} bins, mean {n.mean():.4f}, PTRS rounds at most {rounds.max()}, '
          f'smallest margin {margin.min():.2e}')
    assert p >= ir.DIST_GATE
    assert abs(p - P_VALUES[lam]) < 5e-4
    assert rounds.max() <= 10 and (rounds.max() == 0) == (lam < 10.0)
    assert np.array_equal(n, np.round(n)) and n.min() >= 0


def test_normal_restatement_against_scipy():
    from scipy import stats
    z = ir.normal(_dist_elements(), ir.DIST_SEED)
    p = stats.kstest(z, 'norm').pvalue
    print(f'KS p = {p:.4f}, mean {z.mean():.4f}, std {z.std():.4f}')
    assert p >= ir.DIST_GATE and abs(p - 0.368) < 5e-4


# ---- 3. the correlation ---------------------------------------------------------------------------------------------------------
def _block_mean(x, b):
    h, w = x.shape[0] // b * b, x.shape[1] // b * b
    return x[:h, :w].reshape(h // b, b, w // b, b).mean((1, 3))


@pytest.mark.parametrize('b', [1, 2, 3, 4])
@pytest.mark.parametrize('psf_shape', [(5, 5), (3, 7), (4, 6), (1, 1), (6, 3)])
@pytest.mark.parametrize('boundary', ['zero', 'nearest'])
def test_effective_kernel_against_scipy(b, psf_shape, boundary):
    """flip(psf) * box_b with the header's strided correlation is convolve2d(mode='same', boundary='fill') -- or, for 'nearest',
    ndimage.convolve(mode='nearest') with the PSF's centre at (k - 1) // 2 -- followed by the b x b block mean."""
    from scipy import ndimage, signal
    from sunerf_hip.instrument import Instrument
    rng = np.random.default_rng(10 * b + psf_shape[0])
    psf = rng.random(psf_shape) - 0.2
    img = (rng.random((23, 31)) * 100.0).astype(np.float32)
    inst = Instrument(psf=psf, bin=b, boundary=boundary)
    K, anchor = inst.effective_kernel()
    assert K.shape == (1, psf_shape[0] + b - 1, psf_shape[1] + b - 1) and K.dtype == np.float64
    assert abs(K.sum() - psf.sum() * b * b) <= 1e-12 * np.abs(K).sum()
    got = ir.correlate_bin(img[None], K, b, anchor, inst.scale, boundary)[1][0] * inst.scale
    x = img.astype(np.float64)
    if boundary == 'zero':
        full = signal.convolve2d(x, psf, mode='same', boundary='fill', fillvalue=0.0)
    else:          # ndimage centres an even kernel at k // 2: origin -1 moves it to (k - 1) // 2
        full = ndimage.convolve(x, psf, mode='nearest', origin=tuple(-1 if k % 2 == 0 else 0 for k in psf_shape))
    want = _block_mean(full, b)
    bound = 1e-12 * np.abs(K).sum() * np.abs(x).max()
    err = np.abs(got - want).max()
    print(f'psf {psf_shape} bin {b} {boundary}: effective {K.shape[1:]}, max |diff| {err:.3e}, bound {bound:.3e}')
    assert got.shape == want.shape == (23 // b, 31 // b) and err <= bound


def test_psf_builders():
    from sunerf_hip.instrument import Instrument, gaussian_psf, moffat_psf
    for k in (gaussian_psf(2.5, 4), moffat_psf(3.0, 2.5, 6)):
        n = k.shape[0]
        assert k.dtype == np.float64 and k.shape == (n, n) and abs(k.sum() - 1.0) < 1e-15
        assert np.array_equal(k, k[::-1, ::-1]) and np.array_equal(k, k.T) and k.argmax() == (n * n) // 2
    g = gaussian_psf(4.0, 12)
    row = g[12] / g[12, 12]
    assert abs(row[14] - 0.5) < 1e-12                                   # half maximum two pixels from the centre
    m = moffat_psf(4.0, 3.0, 12)
    assert abs(m[12, 14] / m[12, 12] - 0.5) < 1e-12
    with pytest.raises(ValueError):
        Instrument(psf=np.ones((96, 96)), bin=2)
    with pytest.raises(ValueError):
        Instrument(bin=9)
    with pytest.raises(ValueError):
        Instrument(boundary='wrap')
    inst = Instrument.from_spec('fwhm=2.5,bin=2,exposure=2.9,dn_per_photon=1.2,read_noise=1.2,unit=40,quantise=1')
    assert inst.bin == 2 and inst.psf.shape == (17, 17) and float(inst.exposure) == 2.9 and inst.quantise
    assert np.array_equal(inst.params(2)[1], [40.0, 2.9, 1.2, 1.2, 0.0, np.inf, 0.0, 0.0])
    with pytest.raises(ValueError):
        Instrument.from_spec('gain=2')


# ---- 4. the fifth table ---------------------------------------------------------------------------------------------------------
def test_entry_points_are_declared_bound_and_kept_out_of_the_other_tables(lib):
    """(The table itself -- declared, bound, frozen, versioned, built, its symbols in no other table or older header:
    tests/test_abi_tables_host.py.)"""
    from sunerf_hip import instrument
    header = open(os.path.join(ROOT, 'include', 'sunerf_hip_instrument.h')).read()
    assert lib.sunerf_abi_version() == 9 and lib.sunerf_ext_abi_version() == 1 and lib.sunerf_response_abi_version() == 1
    assert lib.sunerf_prep_abi_version() == 1
    assert lib.sunerf_instrument_abi_version() == 1
    assert f'#define SUNERF_INSTRUMENT_MAX_KERNEL {instrument.MAX_KERNEL}' in header
    assert f'#define SUNERF_INSTRUMENT_MAX_BIN {instrument.MAX_BIN}' in header
    assert f'#define SUNERF_INSTRUMENT_MAX_ROUNDS {ir.MAX_ROUNDS}' in header
    for name, bit in (('POISSON', ir.POISSON), ('READ', ir.READ), ('QUANTISE', ir.QUANTISE), ('SATURATE', ir.SATURATE)):
        assert re.search(rf'#define SUNERF_INSTRUMENT_{name} {bit}\b', header) and getattr(instrument, name) == bit


# ---- 5. argument checks ---------------------------------------------------------------------------------------------------------
def test_argument_checks_come_in_the_documented_order(lib):
    """Unsupported (-2) first, then the empty call (0), then bad counts and null pointers (-1): all before anything touches a
    device, so this runs without one.  ``P`` stands for any non-null pointer: no call here reaches a launch."""
    P = ctypes.c_void_p(4096)
    cb = lib.sunerf_instrument_correlate_bin
    #            in n  h  w  K nk kh kw b ay ax scale bd out stream
    assert cb(None, 0, 4, 4, None, 1, 97, 3, 1, 0, 0, 1.0, 0, None, None) == -2
    assert cb(None, 0, 4, 4, None, 1, 3, 97, 1, 0, 0, 1.0, 0, None, None) == -2
    assert cb(None, 0, 4, 4, None, 1, 3, 3, 9, 0, 0, 1.0, 0, None, None) == -2
    assert cb(None, 0, 4, 4, None, 1, 3, 3, 1, 0, 0, 1.0, 2, None, None) == -2
    assert cb(None, -1, 4, 4, None, 1, 97, 3, 1, 0, 0, 1.0, 0, None, None) == -2          # unsupported comes before bad counts
    assert cb(None, 0, 4, 4, None, 1, 3, 3, 1, 0, 0, 1.0, 0, None, None) == 0
    assert cb(None, 2, 3, 8, None, 1, 3, 3, 4, 0, 0, 1.0, 1, None, None) == 0              # 3 // 4 rows
    assert cb(None, 2, 8, 0, None, 1, 96, 96, 8, 0, 0, 1.0, 1, None, None) == 0
    assert cb(P, -1, 4, 4, P, 1, 3, 3, 1, 0, 0, 1.0, 0, P, None) == -1
    assert cb(P, 0, 4, 4, P, 1, 0, 3, 1, 0, 0, 1.0, 0, P, None) == -1                      # kh < 1 is no empty call
    assert cb(P, 1, 4, 4, P, 1, 3, 3, 0, 0, 0, 1.0, 0, P, None) == -1
    assert cb(P, 3, 4, 4, P, 2, 3, 3, 1, 0, 0, 1.0, 0, P, None) == -1                      # 2 kernels for 3 planes
    assert cb(P, 1, 4, 4, P, 1, 3, 3, 1, 3, 0, 1.0, 0, P, None) == -1 and cb(P, 1, 4, 4, P, 1, 3, 3, 1, 0, -1, 1.0, 0, P, None) == -1
    for k in range(3):
        ptrs = [P] * 3
        ptrs[k] = None
        assert cb(ptrs[0], 1, 4, 4, ptrs[1], 1, 3, 3, 1, 1, 1, 1.0, 0, ptrs[2], None) == -1

    ph = lib.sunerf_instrument_philox
    assert ph(None, 0, 1, 2, None, None) == 0
    assert ph(P, -1, 1, 2, P, None) == -1 and ph(None, 5, 1, 2, P, None) == -1 and ph(P, 5, 1, 2, None, None) == -1

    nz = lib.sunerf_instrument_noise
    #            exp n  h  w par seed off flags img sig sat stream
    assert nz(None, 0, 4, 4, None, 1, 0, 16, None, None, None, None) == -2
    assert nz(P, -1, 4, 4, P, 1, 0, 31, P, None, None, None) == -2
    assert nz(None, 0, 4, 4, None, 1, 0, 15, None, None, None, None) == 0
    assert nz(None, 2, 0, 4, None, 1, 0, 3, None, None, None, None) == 0
    assert nz(P, -1, 4, 4, P, 1, 0, 3, P, None, None, None) == -1
    assert nz(P, 1, 4, 4, P, 1, -1, 3, P, None, None, None) == -1
    for k in range(3):
        ptrs = [P] * 3
        ptrs[k] = None
        assert nz(ptrs[0], 1, 4, 4, ptrs[1], 1, 0, 3, ptrs[2], None, None, None) == -1


def test_host_side_rejections():
    import torch
    from sunerf_hip import SunerfHipError
    from sunerf_hip.instrument import Instrument, philox
    inst = Instrument(psf=np.ones((3, 3)) / 9)
    with pytest.raises(SunerfHipError):
        inst.expected(torch.zeros(1, 4, 4))                       # no CPU path
    with pytest.raises(SunerfHipError):
        inst.observe(torch.zeros(1, 4, 4), seed=1)
    with pytest.raises(SunerfHipError):
        philox(torch.zeros(3, 4, dtype=torch.int32), 0, 0)
    with pytest.raises(ValueError):
        Instrument(unit=[1.0, 2.0]).params(3)


# ---- 6. errors and the detector grid --------------------------------------------------------------------------------------------
@pytest.mark.parametrize('quantise', [False, True])
def test_errors_is_the_sigma_formula_on_the_observed_image(quantise):
    import torch
    from sunerf_hip.instrument import Instrument
    rng = np.random.default_rng(3)
    img = (rng.random((6, 5, 3)) * 50.0 - 2.0).astype(np.float32)          # (H, W, C), some negative
    unit, exposure, g, rn, ped = np.array([2.0, 0.5, 7.0]), 2.9, np.array([1.2, 0.8, 1.0]), 1.7, 100.0
    inst = Instrument(unit=unit, exposure=exposure, dn_per_photon=g, read_noise=rn, pedestal=ped, quantise=quantise)
    got = inst.errors(torch.from_numpy(img))
    assert got.shape == img.shape and got.dtype == torch.float32 and got.device.type == 'cpu'
    x = img.astype(np.float64)
    dn = x * unit * exposure + ped
    lam = np.maximum(dn - ped, 0.0) / g
    want = np.sqrt(lam * g * g + rn * rn + (1.0 / 12.0 if quantise else 0.0)) / exposure / unit
    err = np.abs(got.numpy().astype(np.float64) - want) / want
    print(f'errors: max relative difference {err.max():.3e} (bound 2^-23 + 1e-12)')
    assert err.max() <= 2.0 ** -23 + 1e-12
    planes = inst.errors(torch.from_numpy(img).permute(2, 0, 1), channel_axis=0)
    assert torch.equal(planes.permute(1, 2, 0), got)
    # where the image is the expectation, errors is the sigma of the restatement
    ref = ir.noise(np.ascontiguousarray(np.maximum(img, 0).transpose(2, 0, 1)), inst.params(3), seed=1, flags=0)
    ref['sigma'] = np.sqrt(ref['sigma'].astype(np.float64) ** 2 + (1.0 / 12.0 if quantise else 0.0) / (exposure * unit[:, None, None]) ** 2)
    assert np.allclose(inst.errors(torch.from_numpy(ref['image']), channel_axis=0).numpy(), ref['sigma'], rtol=1e-5, atol=0)


@pytest.mark.parametrize('b', [1, 2, 3])
def test_detector_grid_shares_the_field_of_view(b):
    from sunerf.evaluation.loader import linear_plate_scale_axes
    from sunerf_hip.observations import resampled_grid
    from sunerf_hip.instrument import Instrument
    ref = {'shape': (32, 40), 'cdelt': (150., 140.), 'crpix': (19.25, 15.5), 'crval': (10., -20.), 'meta': {'t_obs': 'x'}}
    inst = Instrument(bin=b)
    fine = resampled_grid(ref, (32 * b, 40 * b))
    for a, c in zip(linear_plate_scale_axes(fine, None, 'cpu'), linear_plate_scale_axes(ref, (32 * b, 40 * b), 'cpu')):
        assert np.allclose(a.numpy(), c.numpy(), rtol=0, atol=1e-15)
    det = inst.detector_grid(fine)
    assert det['shape'] == (32, 40) and det['meta'] == ref['meta'] and det['crval'] == ref['crval']
    for a, c in zip(linear_plate_scale_axes(det, None, 'cpu'), linear_plate_scale_axes(ref, None, 'cpu')):
        print(f'bin {b}: axis differs by {np.abs(a.numpy() - c.numpy()).max():.3e} rad')
        assert np.allclose(a.numpy(), c.numpy(), rtol=0, atol=1e-15)
    # a detector pixel's centre is the mean of its b x b sub-pixel centres
    tx, ty = linear_plate_scale_axes(fine, None, 'cpu')
    dx, dy = linear_plate_scale_axes(det, None, 'cpu')
    assert np.allclose(tx.numpy().reshape(-1, b).mean(1), dx.numpy(), rtol=0, atol=1e-15)
    assert np.allclose(ty.numpy().reshape(-1, b).mean(1), dy.numpy(), rtol=0, atol=1e-15)
    ragged = inst.detector_grid({'shape': (7, 11), 'cdelt': (1., 1.)})
    assert ragged['shape'] == (7 // b, 11 // b)


# ---- the cases of the GPU tests -------------------------------------------------------------------------------------------------
def test_the_noise_case_leaves_no_element_out():
    """tests/test_gpu_instrument.py compares every element of its 3 x 64 x 80 frame: under every flag combination it runs, no
    element of the restatement decides a comparison by less than ``MARGIN``."""
    import test_gpu_instrument as gi
    x, params = gi.noise_case()
    lam = ir.noise(x, params, gi.NOISE_SEED, 0, 0)['lam']
    finite = lam[np.isfinite(lam)]
    assert x.shape == (3, 64, 80) and (x == 0).any() and (x < 0).any() and np.isnan(x).any() and np.isposinf(x).any()
    assert (finite > ir.TWO52).any() and finite[finite <= ir.TWO52].max() >= 1e5 and (finite == 0).any()
    below, above = finite[finite < 10.0].max(), finite[finite >= 10.0].min()
    assert below == float(np.nextafter(np.float32(10.0), np.float32(0.0))) and above == 10.0          # both sides of the branch
    for flags in gi.NOISE_FLAGS:
        ref = ir.noise(x, params, gi.NOISE_SEED, gi.NOISE_OFFSET, flags)
        left_out = int((ref['margin'] < ir.MARGIN).sum())
        print(f'flags {flags:2d}: smallest margin {ref["margin"].min():.3e}, {left_out} elements below {ir.MARGIN}')
        assert left_out == 0
        if flags & ir.SATURATE:
            assert 0 < int(ref['saturated'].sum()) < ref['saturated'].size


def test_abi_cases_cover_the_launching_entry_points(lib):
    """The cases of tests/test_gpu_instrument_abi.py: one table entry per launching entry point, every argument of the signature."""
    import test_gpu_instrument_abi as abi
    from sunerf_hip import lib as binding
    for name, (builder, shapes) in abi.INSTRUMENT_CASES.items():
        for shape in shapes:
            case = builder(shape, 'cpu')
            assert case.name == name and len(case.args) == len(binding.signature(name)[1])
            assert case.empty and case.ws_index is None
