"""The stacking kernel (include/sunerf_hip_stack.h, csrc/stack.hip) against the NumPy restatement
tests/stack_reference.py: ``image`` by value with NaN at the same places, ``count``, ``mask`` and the per-plane counts exactly,
without a tolerance -- for every method, both modes, one- and two-sided, on both sides of every padded frame count the kernel is
instantiated on (4, 8, 16, 32, 64), on shapes with a partial wave, a pixel past a workgroup of 256 and several planes with
different parameters, on samples quantised to small integers so that ties are everywhere."""
import functools

import numpy as np
import pytest
import torch

import stack_reference as sr
from test_stack_host import scene_result  # noqa: F401  (the session fixture: the restatement of the closed scene, computed once)

pytestmark = pytest.mark.gpu

FRAMES = (1, 2, 3, 4, 5, 8, 9, 16, 17, 32, 33, 63, 64)          # both sides of every instantiation
SHAPES = ((1, 1, 1), (2, 5, 67), (1, 3, 257), (3, 2, 64))       # one pixel; a partial wave; one past a workgroup; three planes
CLIP_MIN, MIN_VALID = 3, 2
METHOD_NAMES = {sr.MEAN: 'mean', sr.MEDIAN: 'median', sr.PERCENTILE: 'percentile', sr.RANK: 'rank'}


def params_of(c):
    """a, b, floor per plane, different on every plane."""
    p = np.zeros((c, 4))
    p[:, 0], p[:, 1], p[:, 2] = 0.5 + 0.25 * np.arange(c), 0.25 / (1 + np.arange(c)), 0.5 + 0.5 * np.arange(c)
    return p


@functools.lru_cache(maxsize=None)
def make_stack(t, shape, seed=0, full=False):
    """Small integers around 10 with a tail of outliers on both sides.  ``full``: every sample valid and no flags -- the burst
    of a healthy detector, and the only way to finite values in the top sorted registers of an instantiation -- and no outliers
    in the first row, whose pixels keep all their samples through any clipping.  Otherwise every 11th sample NaN, every 13th
    +inf, every 7th flagged; pixel 0 without a valid sample, pixel 1 with one (below MIN_VALID), pixel 2 (from 5 frames on) with 10, 10, 1000, 100000 and
    nothing else: the first pass leaves two survivors, below CLIP_MIN, in the middle of the passes."""
    c, h, w = shape
    rng = np.random.default_rng(1000 * t + 10 * w + seed)
    frames = rng.integers(8, 13, (t, c, h, w)).astype(np.float32)
    tail = rng.random(frames.shape)
    frames[tail < 0.08] += rng.integers(5, 60, int((tail < 0.08).sum())).astype(np.float32)
    frames[tail > 0.95] -= rng.integers(5, 60, int((tail > 0.95).sum())).astype(np.float32)
    if full:
        frames[:, :, 0] = np.clip(frames[:, :, 0], 8.0, 12.0)
        frames.setflags(write=False)
        return frames, None
    frames.reshape(-1)[::11] = np.nan
    frames.reshape(-1)[::13] = np.inf
    bad = np.zeros(frames.shape, dtype=np.uint8)
    bad.reshape(-1)[::7] = 3
    px = frames.reshape(t, -1)
    flags = bad.reshape(t, -1)
    px[:, 0] = np.nan
    if px.shape[1] > 1:
        px[:, 1], flags[:, 1] = -np.inf, 0
        px[t // 2, 1] = 7.0
    if px.shape[1] > 2 and t >= 5:
        px[:, 2], flags[:, 2] = np.nan, 0
        px[:4, 2] = [100000.0, 10.0, 1000.0, 10.0]
    frames.setflags(write=False)
    bad.setflags(write=False)
    return frames, bad


@functools.lru_cache(maxsize=None)
def reference(t, shape, method, q, rank, mode, two_sided, iterations, n_sigma=2.0, full=False):
    frames, bad = make_stack(t, shape, full=full)
    return sr.combine(frames, bad, params_of(shape[0]), method=method, q=q, rank=rank, mode=mode, n_sigma=n_sigma,
                      iterations=iterations, clip_min=CLIP_MIN, min_valid=MIN_VALID, two_sided=two_sided)


def device(t, shape, method, q, rank, mode, two_sided, iterations, n_sigma=2.0, return_mask=True, full=False):
    from sunerf_hip.stack import combine
    frames, bad = make_stack(t, shape, full=full)
    p = params_of(shape[0])
    return combine(torch.tensor(frames).cuda(), method=METHOD_NAMES[method], q=q if method == sr.PERCENTILE else None,
                   rank=rank if method == sr.RANK else None, a=p[:, 0], b=p[:, 1], floor=p[:, 2], mode=('model', 'mad')[mode],
                   n_sigma=n_sigma, iterations=iterations, clip_min=CLIP_MIN, min_valid=MIN_VALID, two_sided=two_sided,
                   bad=None if bad is None else torch.tensor(bad).cuda(), return_mask=return_mask)


def bits(x):
    """For ``torch.equal`` on images that hold NaN."""
    return x.view(torch.int32) if x.dtype == torch.float32 else x


def check(got, want, what):
    image, count, mask, state = want
    g = {k: v.cpu().numpy() for k, v in got.items()}
    assert g['image'].dtype == np.float32 and g['count'].dtype == np.uint8 and g['n_rejected'].dtype == np.int64
    nan = np.isnan(image)
    assert np.array_equal(np.isnan(g['image']), nan), f'{what}: NaN at other places'
    differ = g['image'][~nan] != image[~nan]
    assert not differ.any(), f'{what}: {int(differ.sum())} of {differ.size} pixels differ by value, first {g["image"][~nan][differ][0]!r} ' \
                             f'for {image[~nan][differ][0]!r}'
    assert np.array_equal(g['count'], count), f'{what}: count'
    if 'mask' in g:
        assert g['mask'].dtype == np.uint8 and np.array_equal(g['mask'], mask), f'{what}: {int((g["mask"] != mask).sum())} mask bytes differ'
    assert [g[k].tolist() for k in ('n_rejected', 'n_invalid', 'n_empty', 'passes')] == state.T.tolist(), f'{what}: state'


METHODS = ([(sr.MEAN, 0.0, 0), (sr.MEDIAN, 0.0, 0)] + [(sr.PERCENTILE, q, 0) for q in (0.0, 5.0, 50.0, 99.9, 100.0)]
           + [(sr.RANK, 0.0, k) for k in (0, 1, -1, 70)])


@pytest.mark.parametrize('method,q,rank', METHODS, ids=[f'{METHOD_NAMES[m]}-{q:g}-{k}' for m, q, k in METHODS])
def test_every_method_equals_the_restatement(method, q, rank):
    for t, iterations in ((9, 0), (9, 2), (33, 2)):
        key = (t, (2, 5, 67), method, q, rank, sr.MODEL, False, iterations)
        check(device(*key), reference(*key), f'T = {t}, {iterations} passes')


def test_min_and_max_are_the_ranks_0_and_minus_1():
    from sunerf_hip.stack import combine
    frames, bad = make_stack(9, (2, 5, 67))
    x, flags = torch.tensor(frames).cuda(), torch.tensor(bad).cuda()
    for name, rank in (('min', 0), ('max', -1)):
        got = combine(x, method=name, bad=flags, min_valid=MIN_VALID)
        want = reference(9, (2, 5, 67), sr.RANK, 0.0, rank, sr.MODEL, False, 0)
        check(got, want, name)


@pytest.mark.parametrize('iterations', [0, 1, 4])
@pytest.mark.parametrize('two_sided', [False, True])
@pytest.mark.parametrize('mode', [sr.MODEL, sr.MAD])
def test_both_modes_and_sides_equal_the_restatement(mode, two_sided, iterations):
    for t in (8, 17):
        key = (t, (2, 5, 67), sr.MEAN, 0.0, 0, mode, two_sided, iterations)
        want = reference(*key)
        check(device(*key), want, f'T = {t}')
        if iterations:
            assert want[3][:, 0].min() > 0, 'the case rejects nothing'
    if iterations == 4 and mode == sr.MODEL and not two_sided:          # the pixel that stops under clip_min, not at a pass that rejects nothing
        image, count, mask, state = reference(17, (2, 5, 67), sr.MEAN, 0.0, 0, mode, two_sided, iterations)
        assert count[0, 0, 2] == 2 and mask[:4, 0, 0, 2].tolist() == [1, 0, 1, 0] and image[0, 0, 2] == 10.0
        assert np.isnan(image[0, 0, 0]) and count[0, 0, 0] == 0 and np.isnan(image[0, 0, 1]) and count[0, 0, 1] == 1 and state[0, 2] >= 2


@pytest.mark.parametrize('shape', SHAPES, ids=['x'.join(map(str, s)) for s in SHAPES])
@pytest.mark.parametrize('t', FRAMES)
def test_every_frame_count_and_shape_equals_the_restatement(t, shape):
    key = (t, shape, sr.MEDIAN, 0.0, 0, sr.MODEL, False, 2)
    check(device(*key), reference(*key), 'model')
    if t >= 8:
        key = (t, shape, sr.PERCENTILE, 30.0, 0, sr.MAD, True, 3)
        check(device(*key), reference(*key), 'mad')


FULL = [(sr.MEDIAN, 0.0, 0, 0), (sr.PERCENTILE, 100.0, 0, 0), (sr.PERCENTILE, 99.9, 0, 0), (sr.RANK, 0.0, -1, 0), (sr.MEAN, 0.0, 0, 0),
        (sr.MEAN, 0.0, 0, 2), (sr.MEDIAN, 0.0, 0, 4), (sr.RANK, 0.0, -1, 2)]


@pytest.mark.parametrize('t', [4, 8, 16, 32, 33, 63, 64])
def test_a_stack_without_an_invalid_sample_equals_the_restatement(t):
    """Every sample valid: n = T at every pixel, so the picks, the percentile's upper neighbour, rank -1 and the mask's upper
    boundary are taken from the top sorted registers of the instantiation -- 4, 8, 16, 32 and 64 filled to the last one, and 33 and
    63 frames in the 64-frame one.  Median, percentile 100 and 99.9, the maximum, the mean, and the clipped mean, median and maximum
    with the mask, one- and two-sided, in both modes from 8 frames on."""
    shape = (2, 5, 67)
    for method, q, rank, iterations in FULL:
        for mode, two_sided in ((sr.MODEL, False), (sr.MODEL, True), (sr.MAD, False), (sr.MAD, True)):
            if mode == sr.MAD and (iterations == 0 or t < 8) or two_sided and iterations == 0:
                continue
            key = (t, shape, method, q, rank, mode, two_sided, iterations)
            want = reference(*key, full=True)
            check(device(*key, full=True), want, f'T = {t}, method {method}, q {q}, rank {rank}, mode {mode}, two-sided {two_sided}, {iterations} passes')
            image, count, mask, state = want
            assert not (mask == sr.INVALID).any() and state[:, 1].tolist() == [0, 0]
            if iterations == 0:
                assert (count == t).all() and not mask.any(), 'a pixel of the full stack has fewer than T survivors'
            else:
                assert state[:, 0].min() > 0 and (count == t).any(), 'the clipped case must reject something and leave full pixels'


def test_without_the_mask_the_result_is_the_same_and_reruns_agree_by_bits():
    for t, mode in ((5, sr.MODEL), (33, sr.MAD), (64, sr.MODEL)):
        key = (t, (1, 3, 257), sr.MEAN, 0.0, 0, mode, True, 3)
        first, again, bare = device(*key), device(*key), device(*key, return_mask=False)
        assert 'mask' not in bare and set(first) - set(bare) == {'mask'}
        for k in first:
            assert torch.equal(bits(first[k]), bits(again[k])), f'{k}: a rerun differs by bits'
        for k in bare:
            assert torch.equal(bits(bare[k]), bits(first[k])), f'{k}: differs without the mask'


def test_a_non_contiguous_stack_gives_the_result_of_its_contiguous_copy():
    from sunerf_hip.stack import combine
    frames, bad = make_stack(9, (2, 5, 67))
    wide = torch.from_numpy(np.ascontiguousarray(np.moveaxis(frames, 0, -1))).cuda()          # [C, H, W, T]
    view = wide.permute(3, 0, 1, 2)
    flags = torch.from_numpy(np.ascontiguousarray(np.moveaxis(bad, 0, -1))).cuda().permute(3, 0, 1, 2)
    assert not view.is_contiguous() and not flags.is_contiguous()
    kw = dict(method='mean', a=1.0, b=0.5, n_sigma=2.0, iterations=2, return_mask=True)
    got, want = combine(view, bad=flags, **kw), combine(view.contiguous(), bad=flags.contiguous(), **kw)
    for k in want:
        assert torch.equal(bits(got[k]), bits(want[k])), k
    single = combine(view[:, 0], bad=flags[:, 0], **kw)          # [T, H, W]: one plane
    assert single['image'].shape == (1, 5, 67) and torch.equal(single['mask'], want['mask'][:, :1])


def test_the_closed_scene_runs_on_the_device(scene_result):
    """The scene of tests/test_stack_host.py: the device finds what the restatement finds there."""
    from sunerf_hip.stack import combine
    from test_stack_host import SCENE_CALL
    frames, hit, want = scene_result
    assert SCENE_CALL == dict(method=sr.MEAN, mode=sr.MODEL, n_sigma=5.0, iterations=4)
    got = combine(torch.from_numpy(frames).cuda(), method='mean', a=9.0, b=1.0, n_sigma=5.0, iterations=4, return_mask=True)
    check(got, want, 'closed scene')
    mask = got['mask'].cpu().numpy()
    assert int(np.sum(hit & (mask != sr.REJECTED))) == 0 and int(np.sum(~hit & (mask == sr.REJECTED))) <= 1e-4 * int(np.sum(~hit))


def test_the_background_of_a_sequence_whose_moving_term_leaves_every_pixel_is_the_static_term():
    from sunerf_hip.stack import background
    from test_stack_host import moving_sequence
    frames, static = moving_sequence()
    got = background(torch.from_numpy(frames).cuda(), q=0.0)
    assert np.array_equal(got['image'].cpu().numpy(), static) and got['n_empty'].tolist() == [0]
    k_corona = torch.from_numpy(frames).cuda() - got['image']
    assert float(k_corona.min()) == 0.0 and bool(((k_corona == 0).sum(0) >= 2).all())          # what is left is the moving term


def test_instrument_combine_runs_with_the_instruments_noise_model():
    from sunerf_hip.despike import despike_params
    from sunerf_hip.instrument import Instrument
    from sunerf_hip.stack import combine
    inst = Instrument(unit=[100.0, 40.0], exposure=[2.9, 1.0], dn_per_photon=[1.2, 0.8], read_noise=[1.2, 0.5])
    frames, bad = make_stack(9, (2, 5, 67))
    x = torch.tensor(frames).cuda()
    p = despike_params(inst, 2)
    got = inst.combine(x, method='mean', iterations=2, n_sigma=3.0, return_mask=True)
    want = combine(x, method='mean', iterations=2, n_sigma=3.0, return_mask=True, a=p[:, 0], b=p[:, 1], floor=p[:, 2])
    assert all(torch.equal(bits(got[k]), bits(want[k])) for k in want)
    assert int(got['n_rejected'].min()) > 0
