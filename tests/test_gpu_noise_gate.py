"""The noise-gating kernel (include/sunerf_hip_noise_gate.h, csrc/noise_gate.hip) against the NumPy fp64 restatement
tests/noise_gate_reference.py, on the cases of tests/test_noise_gate_host.py: a single sample, one block, one past a block on
every axis, axes shorter than a block, every block length, several planes with different noise models; both modes, with and without
NaN, infinities and flagged samples, with a spectrum, with FILL_INVALID.

``state[:, 0]``, ``state[:, 1]``, ``state[:, 3]`` and the NaN positions are compared exactly.  Values are compared within the bound
the restatement derives for the fp32 transform chain.  A coefficient whose fp64 clearance from its threshold is
below the error the forward chain can make there is undecidable: the count of kept coefficients may differ by the number of those,
and in gate mode the samples of the blocks that hold one are left out of the value comparison -- never more than 5 % of a case,
which tests/test_noise_gate_host.py asserts from the restatement alone.  Every test prints its worst error / bound."""
import numpy as np
import pytest
import torch

import noise_gate_reference as nr
from test_noise_gate_host import CASE_IDS, CASES, MAX_EXCLUDED, VARIANTS, case_reference, make_case

pytestmark = pytest.mark.gpu
KEYS = ('n_invalid', 'n_blocks', 'n_kept', 'n_coefficients')


def device(shape, variant, **over):
    from sunerf_hip.noise_gate import noise_gate
    frames, bad, params, spectrum = make_case(shape, variant)
    mode, gamma, invalid, with_spectrum, fill = VARIANTS[variant]
    kw = dict(a=params[:, 0], b=params[:, 1], block_t=shape[4], mode=('gate', 'wiener')[mode], n_sigma=gamma,
              spectrum=None if spectrum is None else torch.from_numpy(spectrum).cuda(),
              bad=None if bad is None else torch.from_numpy(bad).cuda(), fill_invalid=fill)
    kw.update(over)
    return noise_gate(torch.tensor(frames).cuda(), **kw)


def bits(x):
    """For ``torch.equal`` on images that hold NaN."""
    return x.view(torch.int32) if x.dtype == torch.float32 else x


def check(got, want, mode, what):
    out, state, detail = want
    image = got['image'].cpu().numpy()
    counts = np.stack([got[k].cpu().numpy() for k in KEYS], axis=1)
    assert image.dtype == np.float32 and counts.dtype == np.int64 and image.shape == out.shape
    nan = np.isnan(out)
    assert np.array_equal(np.isnan(image), nan), f'{what}: NaN at other places'
    assert np.array_equal(counts[:, [0, 1, 3]], state[:, [0, 1, 3]]), f'{what}: state {counts.tolist()} for {state.tolist()}'
    off = np.abs(counts[:, 2] - state[:, 2])
    assert (off <= detail['undecidable']).all(), f'{what}: kept {counts[:, 2].tolist()} for {state[:, 2].tolist()}, undecidable {detail["undecidable"].tolist()}'
    compared = ~nan & ~detail['excluded'] if mode == nr.GATE else ~nan
    assert (~compared & ~nan).sum() <= MAX_EXCLUDED * nan.size
    err, bound = np.abs(image.astype(np.float64) - out)[compared], detail['bound'][compared]
    worst = float((err / np.maximum(bound, 1e-300)).max()) if err.size else 0.0
    print(f'{what}: worst error / bound {worst:.3f} (largest error {err.max() if err.size else 0.0:.2e}, largest bound '
          f'{bound.max() if err.size else 0.0:.2e}), {int((~compared & ~nan).sum())} of {int((~nan).sum())} samples excluded, '
          f'kept off by {off.tolist()} with {detail["undecidable"].tolist()} undecidable')
    assert (err <= bound).all(), f'{what}: {int((err > bound).sum())} of {err.size} samples beyond the bound, worst {worst:.2f}'


@pytest.mark.parametrize('shape,variant', CASES, ids=CASE_IDS)
def test_every_case_equals_the_restatement_within_the_derived_bound(shape, variant):
    check(device(shape, variant), case_reference(shape, variant), VARIANTS[variant][0], f'{shape} {variant}')


RERUN = [((8, 2, 20, 24, 8), 'gate-invalid'), ((17, 1, 9, 21, 16), 'wiener-spectrum-fill'), ((1, 2, 17, 19, 1), 'gate-spectrum-fill'),
         ((4, 1, 5, 33, 4), 'wiener-invalid')]


def entry_point(shape, variant, fill):
    """The C entry point on buffers of the test's own: ``out`` and ``state`` hold ``fill`` before the call."""
    from sunerf_hip import lib
    from sunerf_hip.ops import _ptr, _stream
    frames, bad, params, spectrum = make_case(shape, variant)
    mode, gamma, invalid, with_spectrum, flag = VARIANTS[variant]
    gamma = (3.0, 1.0)[mode] if gamma is None else gamma
    x = torch.tensor(frames).cuda()
    flags = None if bad is None else torch.from_numpy(bad).cuda()
    shaping = None if spectrum is None else torch.from_numpy(spectrum).cuda()
    p = torch.from_numpy(np.ascontiguousarray(params)).cuda()
    out = torch.full(x.shape, fill, dtype=torch.float32, device=x.device)
    state = torch.full((shape[1], 4), -7, dtype=torch.int64, device=x.device)
    lib.call(x.device, 'sunerf_noise_gate', _ptr(x), _ptr(flags), _ptr(p), _ptr(shaping), *shape[:4], shape[4], mode, int(flag), gamma,
             _ptr(out), _ptr(state), _stream(x.device))
    return out, state


@pytest.mark.parametrize('shape,variant', RERUN, ids=[CASE_IDS[CASES.index(c)] for c in RERUN])
def test_reruns_agree_by_bits_whatever_out_held(shape, variant):
    first, again = device(shape, variant), device(shape, variant)
    for k in first:
        assert torch.equal(bits(first[k]), bits(again[k])), f'{k}: a rerun differs by bits'
    for fill in (float('nan'), 12345.0):
        out, state = entry_point(shape, variant, fill)
        assert torch.equal(bits(out), bits(first['image'])), f'out depends on what it held ({fill})'
        assert torch.equal(state, torch.stack([first[k] for k in KEYS], dim=1)), f'state depends on what it held ({fill})'


def test_a_non_contiguous_sequence_and_a_single_plane_give_the_result_of_the_contiguous_copy():
    from sunerf_hip.noise_gate import noise_gate
    shape, variant = (8, 2, 20, 24, 8), 'gate-invalid'
    frames, bad, params, _ = make_case(shape, variant)
    wide = torch.from_numpy(np.ascontiguousarray(np.moveaxis(frames, 0, -1))).cuda()          # [C, H, W, T]
    view = wide.permute(3, 0, 1, 2)
    flags = torch.from_numpy(np.ascontiguousarray(np.moveaxis(bad, 0, -1))).cuda().permute(3, 0, 1, 2)
    assert not view.is_contiguous() and not flags.is_contiguous()
    kw = dict(a=params[:, 0], b=params[:, 1], n_sigma=3.5)
    got, want = noise_gate(view, bad=flags, **kw), device(shape, variant)
    for k in want:
        assert torch.equal(bits(got[k]), bits(want[k])), k
    single = noise_gate(view[:, 0], bad=flags[:, 0], a=params[0, 0], b=params[0, 1], n_sigma=3.5)          # [T, H, W]: one plane
    assert single['image'].shape == (8, 20, 24) and torch.equal(bits(single['image']), bits(want['image'][:, 0]))
    assert [int(single[k][0]) for k in KEYS] == [int(want[k][0]) for k in KEYS]


def test_a_second_stream_gives_the_same_bits():
    shape, variant = (9, 3, 3, 67, 8), 'wiener-invalid'
    want = device(shape, variant)
    torch.cuda.synchronize()
    stream = torch.cuda.Stream()
    with torch.cuda.stream(stream):
        got = device(shape, variant)
    stream.synchronize()
    for k in want:
        assert torch.equal(bits(got[k]), bits(want[k])), k


def test_the_empty_call_returns_empty_results():
    from sunerf_hip.noise_gate import launch, noise_gate
    got = noise_gate(torch.zeros(4, 2, 0, 5).cuda(), a=1.0, b=0.5, block_t=4)
    assert got['image'].shape == (4, 2, 0, 5) and all(got[k].tolist() == [0, 0] for k in KEYS)
    out, state = launch(torch.zeros(0, 1, 3, 5).cuda(), None, torch.zeros(1, 4, dtype=torch.float64).cuda(), None, 1, 0, 0, 3.0)
    assert out.shape == (0, 1, 3, 5) and state.tolist() == [[0, 0, 0, 0]]


def test_without_noise_the_device_returns_its_input_to_fp32_rounding():
    from sunerf_hip.noise_gate import noise_gate
    frames = make_case((17, 1, 9, 21, 16), 'gate')[0]
    for bt in (1, 4, 8, 16):
        got = noise_gate(torch.tensor(frames).cuda(), a=0.0, b=0.0, block_t=bt)
        err = float((got['image'].cpu() - torch.tensor(frames)).abs().max())
        print(f'block of {bt} frames, a = b = 0: identity to {err:.1e}')
        assert err < 1e-4 and int(got['n_kept'][0]) == int(got['n_coefficients'][0]) > 0


def test_instrument_noise_gate_runs_with_the_instruments_noise_model():
    from sunerf_hip.despike import despike_params
    from sunerf_hip.instrument import Instrument
    from sunerf_hip.noise_gate import noise_gate
    inst = Instrument(unit=[100.0, 40.0], exposure=[2.9, 1.0], dn_per_photon=[1.2, 0.8], read_noise=[1.2, 0.5])
    x = torch.tensor(make_case((8, 2, 20, 24, 8), 'gate')[0]).cuda()
    p = despike_params(inst, 2)
    got = inst.noise_gate(x, block_t=4, mode='wiener')
    want = noise_gate(x, block_t=4, mode='wiener', a=p[:, 0], b=p[:, 1])
    assert all(torch.equal(bits(got[k]), bits(want[k])) for k in want) and int(got['n_kept'].min()) > 0
