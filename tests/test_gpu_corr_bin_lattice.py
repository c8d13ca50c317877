"""The four entry points that stand on csrc/corr_bin.h -- the forward correlation, its gather-form adjoint, the tap gradient and
Richardson-Lucy -- over the lattice of kernel, bin and anchor of tests/corr_bin_lattice.py, whose classifier names the path of
the header a geometry takes (tests/test_corr_bin_lattice_host.py asserts that the lattice reaches them all, and that the three
restatements used here agree with each other on every case).

Gates.  The forward against ``instrument_reference.correlate_bin`` and the adjoint against ``patch_reference.correlate_bin_adjoint``:
bits, the project's contract.  The tap gradient against ``psf_grad_reference.tap_gradient``: ``tap_gradient_bound``, derived there,
and finite.  One Richardson-Lucy update from u = 1: bits against ``deconvolve_reference``.  A wrong loop bound or slice drops or
double-counts a few terms at a tile's edge; it shows as a bit mismatch on the geometries that carry the path's tag, so a test
collects ALL its mismatches and reports them with their tags.

Measured on one MI355X: no mismatch on any geometry; the tap gradient uses at most 0.109 of its bound (1 x 96 taps at bin 6,
nearest).  Against a scratch build whose ``b_max`` lacks the ``j0 < a.kw`` guard, 25 of the 52 tests fail and every one of the 913
mismatching geometries carries ``bin>kw``."""
import functools

import numpy as np
import pytest
import torch

import corr_bin_lattice as cl
import deconvolve_reference as dr
import patch_reference as pr

pytestmark = pytest.mark.gpu
DEV = 'cuda'


def _forward(x, K, case, boundary):
    """``sunerf_instrument_correlate_bin`` as ``Instrument.expected`` calls it; the binding raises on a status other than 0."""
    from sunerf_hip import lib as binding
    from sunerf_hip._ffi import _ptr, _stream
    _, h, w, kh, kw, b, (ay, ax), _ = case
    planes = x.shape[0]
    dev = torch.device(DEV, torch.cuda.current_device())
    taps = torch.tensor(K, dtype=torch.float64).to(DEV)          # (torch.tensor copies: the shared reference arrays are read-only)
    xd = torch.tensor(x).to(DEV)
    out = torch.empty((planes, h // b, w // b), dtype=torch.float32, device=DEV)
    binding.call(dev, 'sunerf_instrument_correlate_bin', _ptr(xd), planes, h, w, _ptr(taps), K.shape[0], kh, kw, b, ay, ax, cl.SCALE,
                 cl.BOUNDARY_CODE[boundary], _ptr(out), _stream(dev))
    torch.cuda.synchronize()
    return out.cpu().numpy()


def _adjoint(g, K, case, boundary):
    """``sunerf_patch_correlate_bin_adjoint`` as ``test_gpu_patch._adjoint`` calls it."""
    from sunerf_hip.instrument import correlate_bin_adjoint
    taps = torch.tensor(K, dtype=torch.float64).to(DEV)
    out = correlate_bin_adjoint(torch.tensor(g).to(DEV), case[1], case[2], taps, K.shape[0], K.shape[1], K.shape[2], case[5], case[6][0],
                                case[6][1], cl.SCALE, cl.BOUNDARY_CODE[boundary])
    torch.cuda.synchronize()
    return out.cpu().numpy()


def _taps(x, g, n_kernels, case, boundary):
    from sunerf_hip.psf_fit import tap_gradient
    _, _, _, kh, kw, b, (ay, ax), _ = case
    out = tap_gradient(torch.tensor(x).to(DEV), torch.tensor(g).to(DEV), n_kernels, kh, kw, b, ay, ax, cl.SCALE, cl.BOUNDARY_CODE[boundary])
    return out.cpu().numpy()


def _differ(got, want):
    """How many elements differ by bits (neither side holds a NaN in these tests), and where the first one is."""
    assert got.shape == want.shape and got.dtype == want.dtype == np.float32, (got.shape, want.shape, got.dtype)
    differ = got.view(np.uint32) != want.view(np.uint32)
    if not differ.any():
        return None
    at = tuple(int(v) for v in np.argwhere(differ)[0])
    return f'{int(differ.sum())} of {got.size} differ by bits, first at {at}: {got[at]!r} != {want[at]!r}'


def _check(case, boundary, ref):
    """The three checks of one geometry: ([mismatch], the tap gradient's largest error over its bound)."""
    bad = []
    assert not np.isnan(ref['forward']).any() and not np.isnan(ref['adjoint']).any()
    for what, got, want in (('forward', _forward(ref['x'], ref['K'], case, boundary), ref['forward']),
                            ('adjoint', _adjoint(ref['g'], ref['K'], case, boundary), ref['adjoint'])):
        msg = _differ(got, want)
        if msg:
            bad.append(f'{what}: {msg}')
    got = _taps(ref['x'], ref['g'], cl.n_kernels_of(case), case, boundary)
    assert got.shape == ref['taps'].shape and got.dtype == np.float64
    with np.errstate(invalid='ignore'):
        used = np.abs(got - ref['taps']) / np.maximum(ref['taps_bound'], 1e-300)
    if not np.isfinite(got).all():
        bad.append(f'tap gradient: {int((~np.isfinite(got)).sum())} of {got.size} taps are not finite')
    elif not (np.abs(got - ref['taps']) <= ref['taps_bound']).all():
        at = tuple(int(v) for v in np.unravel_index(np.argmax(used), used.shape))
        bad.append(f'tap gradient: {int((used > 1).sum())} of {got.size} taps outside the bound, worst at {at}: {got[at]!r} != '
                   f'{ref["taps"][at]!r}, {used[at]:.3e} of the bound')
    return bad, float(np.nanmax(used))


# ---- SMALL ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('boundary', cl.BOUNDARIES)
@pytest.mark.parametrize('b', cl.SMALL_BINS)
def test_small_lattice(b, boundary):
    """Every kernel shape up to 5 x 5 and four anchors at one bin, on 37 x 41: 2 x 2 adjoint tiles, both last ones partial."""
    cases = cl.small_cases(b)
    failures, worst = [], 0.0
    for case in cases:
        bad, used = _check(case, boundary, cl.references(case, boundary))
        worst = max(worst, used)
        failures += [f'{cl.describe(case)} {boundary}: {msg}' for msg in bad]
    print(f'bin {b} {boundary}: {len(cases)} geometries, tap gradient at most {worst:.3f} of its bound, {len(failures)} mismatches')
    assert not failures, f'{len(failures)} mismatches:\n' + '\n'.join(failures)


# ---- LARGE ----------------------------------------------------------------------------------------------------------------------------
def _rl(u0, d, bad, norm, K, c, v, case, boundary, n):
    """test_gpu_deconvolve._rl at this module's scale: (u, state, ratio) after ``n`` updates."""
    from sunerf_hip.deconvolve import launch
    taps = torch.tensor(K, dtype=torch.float64).to(DEV)
    u = torch.tensor(u0).to(DEV)
    params = torch.from_numpy(np.stack([np.asarray(c, dtype=np.float64), np.asarray(v, dtype=np.float64)], axis=1)).to(DEV)
    state, ratio = launch(u, torch.tensor(d).to(DEV), torch.tensor(bad).to(DEV), torch.tensor(norm).to(DEV), params, taps, K.shape[0],
                          K.shape[1], K.shape[2], case[5], case[6][0], case[6][1], cl.SCALE, cl.BOUNDARY_CODE[boundary], n, 0.0)
    torch.cuda.synchronize()
    return u.cpu().numpy(), state.cpu().numpy(), ratio.cpu().numpy()


@functools.lru_cache(maxsize=None)
def _rl_reference(case, boundary):
    """``deconvolve_reference``'s data of the case, the ratio of the start u = 1 and one update from it under norm = 1."""
    K, _, d, bad, c, v = dr.case_data(case)
    ones = np.ones((case[0], case[1], case[2]), dtype=np.float32)
    ratio = dr.ratio_pass(ones, d, bad, K, case[5], case[6], cl.SCALE, boundary, c, v)[0]
    u = dr.update(ones, ratio, ones, K, case[5], case[6], cl.SCALE, boundary)
    for a in (K, d, bad, c, v, ones, ratio, u):
        a.setflags(write=False)
    return (K, d, bad, c, v, ones), ratio, u


@pytest.mark.parametrize('boundary', cl.BOUNDARIES)
@pytest.mark.parametrize('case', cl.LARGE, ids=cl.large_id)
def test_large_case(case, boundary):
    """The three checks of the lattice; one Richardson-Lucy update from u = 1 by bits against the restatement, and against the
    adjoint entry on the device's own ratio (u = (float)(scale acc): products and quotients by 1.0 are exact); plane 1 alone gives
    its bits of the batch; a rerun gives the same bits.  Every wrapper raises on a status other than 0, so a case that returns
    from all of them has seen status 0 from every entry point -- on the two ``lds-max`` cases with 139,520 B of dynamic LDS, for
    which each kernel instantiation needs its own opt-in."""
    tags = cl.tags(case)
    ref = cl.large_references(case, boundary)
    bad, used = _check(case, boundary, ref)
    print(f'{cl.describe(case)} {boundary}: tap gradient at most {used:.3f} of its bound')
    K, x, g = ref['K'], ref['x'], ref['g']
    first = (_forward(x, K, case, boundary), _adjoint(g, K, case, boundary), _taps(x, g, cl.n_kernels_of(case), case, boundary))
    # Richardson-Lucy: the ratio of the start (no update), then one update
    (Kd, d, flagged, c, v, ones), want_ratio, want_u = _rl_reference(case, boundary)
    u0, state0, ratio = _rl(ones, d, flagged, ones, Kd, c, v, case, boundary, 0)
    u1, state1, ratio1 = _rl(ones, d, flagged, ones, Kd, c, v, case, boundary, 1)
    assert np.array_equal(u0.view(np.uint32), ones.view(np.uint32)) and state0[:, 2].tolist() == [0.0] * case[0]
    assert state1[:, 2].tolist() == [1.0] * case[0] and state1[:, 3].tolist() == [0.0] * case[0]
    assert np.isfinite(ratio).all() and not np.isnan(want_u).any() and not np.isnan(want_ratio).any()
    assert (want_ratio > 0).any() or want_ratio.size <= 2          # (a plane of one detector pixel may hold one negative datum)
    for what, got, want in (('ratio of the start', ratio, want_ratio), ('one update from ones', u1, want_u),
                            ('one update from ones against the adjoint entry on the ratio', u1, _adjoint(ratio, Kd, case, boundary))):
        msg = _differ(got, want)
        if msg:
            bad.append(f'{what}: {msg}')
    # a rerun
    again = (_forward(x, K, case, boundary), _adjoint(g, K, case, boundary), _taps(x, g, cl.n_kernels_of(case), case, boundary))
    for what, a, b in zip(('forward', 'adjoint', 'tap gradient'), first, again):
        if not np.array_equal(a.view(np.uint8), b.view(np.uint8)):
            bad.append(f'{what}: a rerun gives other bits')
    u2, state2, ratio2 = _rl(ones, d, flagged, ones, Kd, c, v, case, boundary, 1)
    if not all(np.array_equal(a.view(np.uint8), b.view(np.uint8)) for a, b in zip((u1, state1, ratio1), (u2, state2, ratio2))):
        bad.append('Richardson-Lucy: a rerun gives other bits')
    # plane 1 alone, with its kernel.  (The tap gradient's order depends on the arguments alone and is the same for kernel index 1
    # of the batch and for the plane alone as long as its items are fewer than the runs of either call.)
    assert case[0] == 2 and case[7]
    one = (1,) + case[1:]
    plan = cl.psf_grad_plan(*case[:3], 2, *case[3:6])
    assert plan['items'] <= cl.GRAD_MAX_RUNS // 2
    alone = (_forward(x[1:], K[1:], one, boundary), _adjoint(g[1:], K[1:], one, boundary), _taps(x[1:], g[1:], 1, one, boundary))
    for what, a, b in zip(('forward', 'adjoint', 'tap gradient'), first, alone):
        if not np.array_equal(a[1:].view(np.uint8), b.view(np.uint8)):
            bad.append(f'{what}: plane 1 alone gives other bits than in the batch')
    ua, sa, ra = _rl(ones[1:], d[1:], flagged[1:], ones[1:], Kd[1:], c[1:], v[1:], one, boundary, 1)
    if not all(np.array_equal(a[1:].view(np.uint8), b.view(np.uint8)) for a, b in zip((u1, state1, ratio1), (ua, sa, ra))):
        bad.append('Richardson-Lucy: plane 1 alone gives other bits than in the batch')
    if 'lds-max' in tags:
        assert cl.adjoint_lds_bytes(*case[3:6]) == cl.LDS_MAX
    assert not bad, f'{cl.describe(case)} {boundary}:\n' + '\n'.join(bad)


# ---- positive data ------------------------------------------------------------------------------------------------------------------
def _reached(case, boundary):
    """bool [H, W]: the input pixels that some tap of some detector pixel reads (under 'nearest': after the clamp)."""
    _, h, w, kh, kw, b, (ay, ax), _ = case
    ys = (np.arange(h // b) * b - ay)[:, None] + np.arange(kh)[None, :]
    xs = (np.arange(w // b) * b - ax)[:, None] + np.arange(kw)[None, :]
    if boundary == 'nearest':
        ys, xs = np.clip(ys, 0, h - 1), np.clip(xs, 0, w - 1)
    rows, cols = np.zeros(h, dtype=bool), np.zeros(w, dtype=bool)
    rows[ys[(ys >= 0) & (ys < h)]] = True
    cols[xs[(xs >= 0) & (xs < w)]] = True
    return rows[:, None] & cols[None, :]


EMPTY_TILE_CASES = [c for c in cl.LARGE if 'empty-tile' in cl.tags(c)] + [c for b in (5, 8) for c in cl.small_cases(b)[::17]
                                                                           if 'empty-tile' in cl.tags(c)]


@pytest.mark.parametrize('boundary', cl.BOUNDARIES)
def test_unreachable_tiles_hold_positive_zero_under_positive_data(boundary):
    """With |K| and |g| of the case data (every value above 0) a pixel that a tap reaches is a sum of positive terms: not 0.  A
    pixel of an unreachable tile must hold the bits of +0.0 -- it is written, and not with rubbish that the signed data's
    reference could equal by accident.  A pixel outside those tiles that no tap reaches (bin > kh leaves such rows in every tile)
    is +0.0 as well; every other pixel is non-zero, under either boundary.  ("Every pixel outside the unreachable tiles is
    non-zero" does not hold as it stands: 3 x 3 taps at bin 8 read three rows of every eight.  ``_reached`` marks the pixels
    that are read from the geometry alone, and both sides of it are asserted.)"""
    failures = []
    assert len(EMPTY_TILE_CASES) >= 8 and {c[5] for c in EMPTY_TILE_CASES} >= {2, 3, 4, 5, 8}
    for case in EMPTY_TILE_CASES:
        K, _, g = pr.case_data(case)
        K, g = np.abs(K), np.abs(g)
        assert (K > 0).all() and (g > 0).all()
        got = _adjoint(g, K, case, boundary)
        reached = _reached(case, boundary)
        empty = np.zeros(case[1:3], dtype=bool)
        for y0, x0 in cl.unreachable_tiles(*case[1:6], *case[6]):
            empty[y0:y0 + cl.TILE, x0:x0 + cl.TILE] = True
        assert empty.any() and not (empty & reached).any() and reached.any()
        want, _ = pr.correlate_bin_adjoint(g, K, case[1], case[2], case[5], case[6], cl.SCALE, boundary)
        for p in range(case[0]):
            bits = got[p].view(np.uint32)
            msgs = []
            if (bits[empty] != 0).any():
                msgs.append(f'{int((bits[empty] != 0).sum())} of {int(empty.sum())} pixels of unreachable tiles are not +0.0')
            if (bits[~reached & ~empty] != 0).any():
                msgs.append(f'{int((bits[~reached & ~empty] != 0).sum())} unreached pixels of reachable tiles are not +0.0')
            if not (got[p][reached] > 0).all():
                msgs.append(f'{int((~(got[p][reached] > 0)).sum())} of {int(reached.sum())} reached pixels are not positive')
            msg = _differ(got[p], want[p])
            if msg:
                msgs.append(msg)
            failures += [f'{cl.describe(case)} {boundary} plane {p}: {m}' for m in msgs]
    print(f'{len(EMPTY_TILE_CASES)} geometries with an unreachable tile under {boundary}: {len(failures)} mismatches')
    assert not failures, '\n'.join(failures)
