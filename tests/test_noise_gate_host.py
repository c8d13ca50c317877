"""CPU-only checks of noise gating (no GPU): the fourteenth entry-point table (declared, bound, versioned, its
argument checks in their documented order), the wrapper's refusals, the NumPy restatement tests/noise_gate_reference.py against the
properties it has to have (windows that sum to 1.5, the symmetric fold, identity without noise, only DC at a huge threshold, the
rules for invalid samples on a sequence small enough to check by hand), the statistics of the gate on white noise, the closed scene
of DESIGN.md 8z, and that no case of tests/test_gpu_noise_gate.py excludes more than 5 % of its samples.  Every figure is printed."""
import ctypes
import functools
import os

import numpy as np
import pytest
import torch

import noise_gate_reference as nr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

@pytest.fixture(scope='session')
def lib():
    import sunerf_hip
    if not os.path.exists(sunerf_hip.LIB_PATH):
        import subprocess
        subprocess.check_call(['bash', os.path.join(ROOT, '2024-hl-spi3s-sunerf_amd', 'csrc', 'build.sh')])
    return sunerf_hip.load()


# ---- the fourteenth table ---------------------------------------------------------------------------------------------------------
def test_entry_points_are_declared_and_bound(lib):
    """(The table itself -- declared, bound, frozen, versioned, built: tests/test_abi_tables_host.py.)"""
    header = open(os.path.join(ROOT, 'include', 'sunerf_hip_noise_gate.h')).read()
    assert lib.sunerf_noise_gate_abi_version() == 1
    for define in ('SUNERF_NOISE_GATE_BLOCK 16', 'SUNERF_NOISE_GATE_STATE 4', 'SUNERF_NOISE_GATE_MODE_GATE 0',
                   'SUNERF_NOISE_GATE_MODE_WIENER 1', 'SUNERF_NOISE_GATE_FILL_INVALID 1'):
        assert f'#define {define}' in header, define
    from sunerf_hip import noise_gate as wrapper
    assert wrapper.MODES == {'gate': nr.GATE, 'wiener': nr.WIENER} and wrapper.FILL_INVALID == nr.FILL_INVALID == 1
    assert wrapper.BLOCK_T == nr.BLOCK_T == (1, 4, 8, 16) and wrapper.BLOCK == nr.BLOCK == 16 and wrapper.N_STATE == 4
    assert wrapper.DEFAULT_N_SIGMA == {'gate': 3.0, 'wiener': 1.0}


def check_argument_order(lib):
    """The block, the mode and the flags (-2) first, then the empty call (0), then counts, gamma, null pointers, alignment and the
    overlap of out with an input (-1): all before anything touches a device, so this runs without one.  ``Q`` stands for any
    non-null aligned pointer: no call here reaches a launch."""
    fn = lib.sunerf_noise_gate
    names = ('frames', 'params', 'out', 'state')
    Q = {k: ctypes.c_void_p((1 << 20) * (i + 1)) for i, k in enumerate(names)}

    def call(t=8, c=2, h=9, w=11, bt=8, mode=0, flags=0, gamma=3.0, bad=None, spectrum=None, **ptrs):
        p = dict(Q)
        p.update(ptrs)
        return fn(p['frames'], bad, p['params'], spectrum, t, c, h, w, bt, mode, flags, gamma, p['out'], p['state'], None)
    none = {k: None for k in names}
    for limit in (dict(bt=0), dict(bt=2), dict(bt=3), dict(bt=32), dict(bt=-1), dict(mode=2), dict(mode=-1), dict(flags=2), dict(flags=-1)):
        assert call(**limit, **none) == -2, limit
        assert call(**limit, c=0, **none) == -2 and call(**limit, h=-1, **none) == -2, limit          # the limits come first
    for empty in (dict(t=0), dict(c=0), dict(h=0), dict(w=0), dict(h=0, w=0), dict(c=0, bt=16, mode=1, flags=1)):
        assert call(**empty, **none) == 0, empty                                                       # then the empty call
    assert call(c=0, gamma=float('nan'), **none) == 0                                                  # ... before gamma
    assert call(t=-1) == -1 and call(c=-1) == -1 and call(h=-1) == -1 and call(w=-1) == -1 and call(c=-1, h=0) == -1
    for bad_gamma in (0.0, -1.0, float('nan'), float('inf')):
        assert call(gamma=bad_gamma) == -1, bad_gamma
    for k in names:
        assert call(**{k: None}) == -1, k
    for k in ('params', 'state'):
        assert call(**{k: ctypes.c_void_p(Q[k].value + 4)}) == -1, k
    far = ctypes.c_void_p(Q['state'].value + (1 << 20))
    for k in ('frames', 'out'):
        assert call(**{k: ctypes.c_void_p(Q[k].value + 2)}) == -1, k
    assert call(spectrum=ctypes.c_void_p(far.value + 2)) == -1
    # out may not overlap frames (8 x 2 x 9 x 11 floats are 6336 bytes), bad (1584), params (64) or spectrum (2 x 8 x 256 floats)
    assert call(out=Q['frames']) == -1 and call(out=ctypes.c_void_p(Q['frames'].value + 6332)) == -1
    assert call(out=ctypes.c_void_p(Q['frames'].value - 6332)) == -1
    assert call(out=ctypes.c_void_p(Q['params'].value + 60)) == -1 and call(out=ctypes.c_void_p(Q['params'].value - 6332)) == -1
    assert call(bad=far, out=far) == -1 and call(bad=far, out=ctypes.c_void_p(far.value + 1580)) == -1
    assert call(spectrum=far, out=far) == -1 and call(spectrum=far, out=ctypes.c_void_p(far.value + 16380)) == -1
    # with every pointer null the next refusal is the pointers': all the checks before them pass
    assert all(call(t=t, bt=bt, mode=m, flags=f, gamma=g, **none) == -1
               for t, bt, m, f, g in ((1, 1, 0, 0, 1e-3), (1, 16, 1, 1, 1e30), (64, 4, 0, 1, 3.0), (7, 8, 1, 0, 1.0)))


def test_argument_checks_come_in_the_documented_order(lib):
    check_argument_order(lib)


# ---- the wrapper ------------------------------------------------------------------------------------------------------------------
def test_the_wrapper_refuses_what_it_cannot_run():
    from sunerf_hip import SunerfHipError
    from sunerf_hip.noise_gate import noise_gate
    x = torch.zeros(8, 2, 9, 11)
    for kw in (dict(mode='median'), dict(block_t=2), dict(block_t=32), dict(block_t=True), dict(n_sigma=0), dict(n_sigma=float('inf')),
               dict(n_sigma=float('nan')), dict(a=-1.0), dict(b=float('nan')), dict(a=[1.0] * 3), dict(block_t=16),
               dict(spectrum=torch.ones(8, 16, 15)), dict(spectrum=torch.ones(3, 8, 16, 16)), dict(spectrum=torch.ones(8, 16, 16).double()),
               dict(spectrum=np.ones((8, 16, 16), dtype=np.float32)), dict(block_t=4, spectrum=torch.ones(8, 16, 16))):
        with pytest.raises(ValueError):
            noise_gate(x, **{'a': 1.0, 'b': 0.5, **kw})
        print('refused:', sorted(kw))
    with pytest.raises(TypeError):
        noise_gate(x, b=0.5)          # a and b have no default: the noise model is the point
    for t, fits in ((7, 4), (3, 1), (15, 8)):
        with pytest.raises(ValueError, match=f'use a smaller block \\({fits} fits\\)'):
            noise_gate(torch.zeros(t, 1, 3, 5), a=1.0, b=0.0, block_t=16 if t == 15 else 8 if t == 7 else 4)
    with pytest.raises(ValueError, match='float32'):
        noise_gate(x.double(), a=1.0, b=0.0)
    with pytest.raises(ValueError, match='float32'):
        noise_gate(x[0, 0], a=1.0, b=0.0)
    with pytest.raises(ValueError, match='bad must have'):
        noise_gate(x, a=1.0, b=0.0, bad=torch.zeros(8, 2, 9, 10))
    with pytest.raises(TypeError):
        noise_gate(x.numpy(), a=1.0, b=0.0)
    # every argument is in order: only the device is missing
    for kw in (dict(), dict(block_t=1, mode='wiener'), dict(block_t=4, n_sigma=2.5, fill_invalid=True, bad=torch.zeros(8, 2, 9, 11, dtype=torch.bool)),
               dict(a=[1.0, 2.0], b=[0.0, 0.5], spectrum=torch.ones(8, 16, 16)), dict(spectrum=torch.ones(2, 8, 16, 16))):
        with pytest.raises(SunerfHipError, match='no CPU path'):
            noise_gate(x, **{'a': 1.0, 'b': 0.5, **kw})
    with pytest.raises(SunerfHipError, match='no CPU path'):
        noise_gate(x[:, 0], a=1.0, b=0.5)


def test_instrument_noise_gate_passes_the_noise_model(monkeypatch):
    from sunerf_hip import noise_gate as module
    from sunerf_hip.despike import despike_params
    from sunerf_hip.instrument import Instrument
    seen = []
    monkeypatch.setattr(module, 'noise_gate', lambda frames, **kw: seen.append((frames, kw)) or 'result')
    inst = Instrument(unit=[100.0, 40.0, 7.5], exposure=[2.9, 1.0, 12.0], dn_per_photon=[1.2, 0.8, 3.0], read_noise=[1.2, 0.0, 5.0])
    frames = torch.zeros(8, 3, 4, 6)
    assert inst.noise_gate(frames, block_t=4, mode='wiener') == 'result'
    got, kw = seen[-1]
    p = despike_params(inst, 3)
    assert got is frames and set(kw) == {'block_t', 'mode', 'a', 'b'}
    assert np.array_equal(kw['a'], p[:, 0]) and np.array_equal(kw['b'], p[:, 1])
    single = Instrument(unit=100.0, exposure=2.9, dn_per_photon=1.2, read_noise=1.2)
    single.noise_gate(frames[:, 0], a=7.0)
    kw = seen[-1][1]
    assert kw['a'] == 7.0 and np.array_equal(kw['b'], despike_params(single, 1)[:, 1])
    with pytest.raises(ValueError):
        inst.noise_gate(frames[0, 0])


# ---- the restatement --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('n', [4, 8, 16])
def test_four_blocks_cover_every_sample_and_their_squared_windows_sum_to_one_and_a_half(n):
    w = nr.window(n)
    assert np.array_equal(w, w) and np.allclose(w, w[::-1], atol=1e-15) and nr.stride(n) == n // 4
    for size in range(1, 41):
        cover, total = np.zeros(size, dtype=int), np.zeros(size)
        for o in nr.origins(size, n):
            assert o < size and o + n > 0
            inside = (o + np.arange(n) >= 0) & (o + np.arange(n) < size)
            cover[(o + np.arange(n))[inside]] += 1
            total[(o + np.arange(n))[inside]] += w[inside] ** 2
        assert (cover == 4).all() and np.abs(total - 1.5).max() < 1e-15, (n, size)
    assert nr.origins(7, 1) == list(range(7)) and nr.window(1).tolist() == [1.0]


def test_the_fold_is_numpys_symmetric_padding():
    for n in range(1, 41):
        line = np.arange(n)
        padded = np.pad(line, (48, 48), mode='symmetric')
        assert np.array_equal(nr.fold(np.arange(-48, n + 48), n), padded), n


def test_the_canonical_coefficient_is_shared_by_k_and_minus_k():
    for bt in nr.BLOCK_T:
        canon = nr.canonical(bt).reshape(bt, 16, 16)
        kt, ky, kx = np.meshgrid(np.arange(bt), np.arange(16), np.arange(16), indexing='ij')
        assert np.array_equal(canon, canon[(-kt) % bt, (-ky) % 16, (-kx) % 16])
        assert (canon % 16 <= 8).all() and canon[0, 0, 0] == 0
        own = (kt * 16 + ky) * 16 + kx
        assert np.array_equal(canon[:, :, 1:8], own[:, :, 1:8])


SMALL = [((1, 1, 1, 1), 1), ((1, 1, 5, 7), 1), ((4, 2, 3, 9), 4), ((8, 1, 17, 5), 8), ((16, 1, 4, 18), 16), ((19, 1, 2, 3), 16), ((9, 1, 20, 33), 4)]


@pytest.mark.parametrize('shape,bt', SMALL, ids=[f'{"x".join(map(str, s))}-{b}' for s, b in SMALL])
def test_without_noise_the_sequence_comes_back_and_at_a_huge_threshold_only_dc_survives(shape, bt):
    rng = np.random.default_rng(sum(shape) + bt)
    x = rng.normal(5.0, 2.0, shape).astype(np.float32)
    for mode in (nr.GATE, nr.WIENER):
        out, state = nr.noise_gate(x, bt=bt, mode=mode)          # a = b = 0: every factor is 1
        err = float(np.abs(out - x).max())
        print(f'{shape} bt {bt} mode {mode}: identity to {err:.1e}')
        assert err < 1e-13 and (state[:, 0] == 0).all()
        assert np.array_equal(state[:, 2], state[:, 3]) if mode == nr.GATE else (state[:, 2] <= state[:, 3]).all()          # wiener: 0 where F = 0
        assert (state[:, 3] == state[:, 1] * (bt * 256 - 1)).all()
        n_blocks = len(nr.origins(shape[0], bt)) * len(nr.origins(shape[2], 16)) * len(nr.origins(shape[3], 16))
        assert (state[:, 1] == n_blocks).all()
        out, state = nr.noise_gate(x, params=np.tile([1.0, 0.0, 0.0, 0.0], (shape[1], 1)), bt=bt, mode=mode, gamma=1e12)
        assert (state[:, 2] == 0).all() and (state[:, 3] > 0).all()

def test_invalid_samples_follow_the_rules_on_a_sequence_small_enough_to_check_by_hand():
    # one plane of 1 x 2 x 2 at bt = 1: every block folds to copies of the four samples, so its mean is the mean of the valid ones
    x = np.array([[[[1.0, 3.0], [np.nan, 8.0]]]], dtype=np.float32)
    out, state = nr.noise_gate(x, bt=1)          # no noise: valid samples come back, the invalid one is NaN
    assert np.isnan(out[0, 0, 1, 0]) and np.allclose(out[0, 0][[0, 0, 1], [0, 1, 1]], [1.0, 3.0, 8.0], atol=1e-13)
    n_blocks = len(nr.origins(2, 16)) ** 2
    assert n_blocks == 16 and state[0].tolist() == [1, 16, 16 * 255, 16 * 255]
    filled, _ = nr.noise_gate(x, bt=1, flags=nr.FILL_INVALID)
    assert abs(filled[0, 0, 1, 0] - 4.0) < 1e-13 and np.array_equal(filled[~np.isnan(out)], out[~np.isnan(out)])
    # flagged and infinite samples are invalid too, and a plane without a valid sample has no block and no output
    x = np.stack([x[:, 0], np.full((1, 2, 2), np.inf, dtype=np.float32)], axis=1)
    bad = np.zeros(x.shape, dtype=np.uint8)
    bad[0, 0, 0, 0] = 7
    out, state = nr.noise_gate(x, bad, bt=1, flags=nr.FILL_INVALID)
    assert state.tolist() == [[2, 16, 16 * 255, 16 * 255], [4, 0, 0, 0]] and (out[:, 1] == 0).all()
    assert abs(out[0, 0, 0, 0] - 5.5) < 1e-13 and abs(out[0, 0, 1, 0] - 5.5) < 1e-13
    assert np.isnan(nr.noise_gate(x, bad, bt=1)[0][:, 1]).all()
    # invalid samples carry no noise: with b = 0 the noise power of a block is a sum W^2 over its valid samples
    x = np.zeros((1, 1, 16, 16), dtype=np.float32)
    x[0, 0, 3, 5] = np.nan
    out, state = nr.noise_gate(x, params=[[1.0, 0.0, 0.0, 0.0]], bt=1)
    assert state[0, 2] == 0 and np.nansum(np.abs(out)) == 0.0          # all zero: |F|^2 = 0 < 9 P


def test_white_noise_passes_the_gate_as_often_as_exp_minus_gamma_squared():
    """White Gaussian noise of variance ``a``: a coefficient with k != -k is complex Gaussian with E|F|^2 = a sum W^2 = P, so
    |F|^2 / P is exponential and passes gamma^2 with probability exp(-gamma^2).  The blocks overlap, so their coefficients are not
    independent: the margin is 5 standard deviations of a binomial over the coefficients of every 64th block (the ones that share
    no sample), which is 8 times that over all of them."""
    rng = np.random.default_rng(5)
    gamma, a = 1.5, 4.0
    x = rng.normal(0.0, np.sqrt(a), (16, 1, 64, 64)).astype(np.float32)
    out, state, detail = nr.noise_gate(x, params=[[a, 0.0, 0.0, 0.0]], bt=8, gamma=gamma, detail=True)
    # 8 coefficients of a block have k = -k and are real; the other 2040 are the ones to count, in the blocks that read no folded
    # sample (a folded block is partly its own mirror image, and the coefficients of a symmetric block are not complex Gaussian)
    blocks, kept = detail['interior_blocks'], detail['interior_kept']
    from math import exp, sqrt
    p = exp(-gamma ** 2)
    expected = blocks * 2040 * p
    sigma = 8.0 * sqrt(blocks * 2040 * p * (1.0 - p))
    print(f'white noise, gamma {gamma}: kept {kept} of {blocks * 2040} coefficients in {blocks} interior blocks, expected {expected:.0f} '
          f'+- {5 * sigma:.0f} (5 sigma); all blocks: {state[0].tolist()}')
    assert blocks == 5 * 13 * 13 and abs(kept - expected) < 5.0 * sigma and sigma < 0.02 * expected


def closed_scene(seed=1):
    """The closed scene of DESIGN.md 8z: a drifting Gaussian blob plus a travelling sine over 16 x 40 x 48 samples, shot noise ``b = 0.5``."""
    rng = np.random.default_rng(seed)
    t, y, x = np.meshgrid(np.arange(16), np.arange(40), np.arange(48), indexing='ij')
    truth = 20.0 + 60.0 * np.exp(-((y - 14 - 0.5 * t) ** 2 + (x - 12 - 1.5 * t) ** 2) / 18.0) + 8.0 * np.sin(0.45 * x + 0.2 * y - 0.6 * t)
    noisy = truth + np.sqrt(0.5 * truth) * rng.standard_normal(truth.shape)
    return noisy.astype(np.float32)[:, None], truth[:, None], np.array([[0.0, 0.5, 0.0, 0.0]])


@functools.lru_cache(maxsize=None)
def scene_result(bt, mode, gamma):
    frames, truth, params = closed_scene()
    out, state = nr.noise_gate(frames, params=params, bt=bt, mode=mode, gamma=gamma)
    return float(np.sqrt(np.mean((out - truth) ** 2))), state


def test_the_closed_scene_loses_most_of_its_noise():
    frames, truth, _ = closed_scene()
    before = float(np.sqrt(np.mean((frames - truth) ** 2)))
    print(f'closed scene 16 x 40 x 48: RMS error before {before:.2f}')
    table = {}
    for bt in (1, 8, 16):
        table[bt] = (scene_result(bt, nr.GATE, 3.0)[0], scene_result(bt, nr.WIENER, 1.5)[0])
        print(f'  block of {bt:2d} frames: gate, gamma 3: {table[bt][0]:.2f}   wiener, gamma 1.5: {table[bt][1]:.2f}')
    assert before > 1.5 and all(v < 0.5 * before for pair in table.values() for v in pair)
    assert table[16][0] < table[8][0] < table[1][0] and table[16][1] < table[8][1] < table[1][1]          # longer blocks gate better


# ---- the cases of tests/test_gpu_noise_gate.py ------------------------------------------------------------------------------------
SHAPES = [(1, 1, 1, 1, 1), (1, 1, 16, 16, 1), (1, 2, 17, 19, 1), (4, 1, 5, 33, 4), (8, 2, 20, 24, 8), (16, 1, 16, 16, 16), (17, 1, 9, 21, 16),
          (9, 3, 3, 67, 8)]
# (mode, gamma or None for the default, invalid samples, a spectrum, FILL_INVALID)
VARIANTS = {'gate': (nr.GATE, None, False, False, False), 'gate-invalid': (nr.GATE, 3.5, True, False, False),
            'gate-spectrum-fill': (nr.GATE, None, True, True, True), 'wiener': (nr.WIENER, None, False, False, False),
            'wiener-invalid': (nr.WIENER, 1.5, True, False, False), 'wiener-spectrum-fill': (nr.WIENER, 1.5, True, True, True)}
# (shape, variant) -> seed where seed 0 leaves undecidable coefficients in too many blocks; the first keeps four of them in blocks
# that hold exactly 5 % of its samples, so that the exclusion is exercised
SEEDS = {((8, 2, 20, 24, 8), 'gate-spectrum-fill'): 1, ((16, 1, 16, 16, 16), 'gate-invalid'): 1, ((17, 1, 9, 21, 16), 'gate-invalid'): 1,
         ((9, 3, 3, 67, 8), 'gate'): 1}
MAX_EXCLUDED = 0.05


def case_params(c):
    p = np.zeros((c, 4))
    p[:, 0], p[:, 1] = 1.0 + 0.5 * np.arange(c), 0.75 / (1 + np.arange(c))
    return p


def case_spectrum(c, bt):
    """Symmetric under k -> -k, rising from 1 at DC to 3.5 at the highest frequencies, different on every plane."""
    kt, ky, kx = np.meshgrid(np.arange(bt), np.arange(16), np.arange(16), indexing='ij')
    d = np.minimum(kt, bt - kt) + np.minimum(ky, 16 - ky) + np.minimum(kx, 16 - kx)
    s = np.stack([(1.0 + 0.25 * p) * (1.0 + 0.125 * d) for p in range(c)])
    return s.astype(np.float32)


@functools.lru_cache(maxsize=None)
def make_case(shape, variant):
    """``(frames, bad, params, spectrum)`` of one case: a level of 1 with a drifting blob and a travelling sine, noise of the
    plane's own model on top (a standard deviation of 1 to 2 per sample, so that values below 0 occur).  With invalid samples: every 17th NaN, every 29th
    +inf, every 31st -inf, every 13th flagged; a single sample is NaN; the second plane of a case loses its columns 0 .. 15, which
    leaves blocks without a valid sample."""
    t, c, h, w, bt = shape
    mode, gamma, invalid, with_spectrum, fill = VARIANTS[variant]
    rng = np.random.default_rng(1000 * SEEDS.get((shape, variant), 0) + 10 * w + t)
    tt, cc, yy, xx = np.meshgrid(np.arange(t), np.arange(c), np.arange(h), np.arange(w), indexing='ij')
    truth = 1.0 + 6.0 * np.exp(-((yy - 5 - 0.5 * tt) ** 2 + (xx - 8 - tt) ** 2) / 12.0) + 2.0 * np.sin(0.5 * xx + 0.3 * yy - 0.7 * tt + cc)
    params = case_params(c)
    sigma = np.sqrt(params[None, :, 0, None, None] + params[None, :, 1, None, None] * truth)
    frames = (truth + sigma * rng.standard_normal(truth.shape)).astype(np.float32)
    bad = None
    if invalid:
        flat = frames.reshape(-1)
        flat[::17], flat[5::29], flat[7::31] = np.nan, np.inf, -np.inf
        bad = np.zeros(frames.shape, dtype=np.uint8)
        bad.reshape(-1)[::13] = 3
        if c > 1:
            frames[:, 1, :, :16] = np.nan
    frames.setflags(write=False)
    return frames, bad, params, case_spectrum(c, bt) if with_spectrum else None


@functools.lru_cache(maxsize=None)
def case_reference(shape, variant):
    frames, bad, params, spectrum = make_case(shape, variant)
    mode, gamma, invalid, with_spectrum, fill = VARIANTS[variant]
    return nr.noise_gate(frames, bad, params, spectrum, bt=shape[4], mode=mode, gamma=gamma, flags=nr.FILL_INVALID if fill else 0, detail=True)


CASES = [(s, v) for s in SHAPES for v in VARIANTS]
CASE_IDS = [f'{"x".join(map(str, s[:4]))}-bt{s[4]}-{v}' for s, v in CASES]


@pytest.mark.parametrize('shape,variant', CASES, ids=CASE_IDS)
def test_no_case_of_the_gpu_test_excludes_more_than_five_percent_of_its_samples(shape, variant):
    out, state, detail = case_reference(shape, variant)
    frames, bad, params, spectrum = make_case(shape, variant)
    excluded = float(detail['excluded'].mean()) if VARIANTS[variant][0] == nr.GATE else 0.0
    print(f'{shape} {variant}: {detail["blocks"]} blocks, state {state.tolist()}, {detail["undecidable"].tolist()} undecidable coefficients, '
          f'smallest clearance {detail["min_clearance"]:.2f} of the allowed error, {100 * excluded:.1f} % of the samples excluded, '
          f'largest bound {detail["bound"].max():.1e}')
    assert excluded <= MAX_EXCLUDED
    invalid = ~np.isfinite(frames) if bad is None else ~np.isfinite(frames) | (bad != 0)
    assert np.array_equal(state[:, 0], invalid.sum(axis=(0, 2, 3)))
    assert np.array_equal(np.isnan(out), invalid & (not VARIANTS[variant][4]))
    if np.prod(shape[:4]) > 1:
        assert (state[:, 2] > 0).all() and (state[:, 2] < state[:, 3]).all(), 'the case keeps and drops something on every plane'
