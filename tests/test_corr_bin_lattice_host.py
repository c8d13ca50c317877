"""The lattice of tests/corr_bin_lattice.py on a CPU: its cases reach every path of csrc/corr_bin.h that the classifier names, the
restated LDS footprint of the adjoint stays inside the device's, and the three NumPy restatements the GPU tests compare the
kernels with -- ``instrument_reference.correlate_bin``, ``patch_reference.correlate_bin_adjoint`` and
``psf_grad_reference.tap_gradient``, written independently of each other -- agree on every case through the adjoint identity

    sum(A x . g) == sum(x . A^T g) == sum(K . dK) / scale

with fp64 accumulators, before any rounding to fp32, within a derived bound (``corr_bin_lattice.identity_check``).  No kernel
takes part.  Every figure is printed before it is asserted."""
import collections

import numpy as np
import pytest

import corr_bin_lattice as cl

ISSUE_LARGE = [(34, 33, 96, 96, 1, (47, 48)), (34, 33, 96, 96, 1, (0, 95)), (40, 45, 96, 96, 5, (95, 0)), (36, 43, 96, 96, 7, (48, 48)),
               (70, 7, 96, 1, 3, (95, 0)), (7, 70, 1, 96, 6, (0, 10)), (66, 41, 65, 33, 4, (32, 16)), (71, 70, 3, 3, 8, (2, 2)),
               (71, 70, 1, 1, 8, (0, 0)), (8, 8, 2, 3, 8, (1, 2)), (2, 64, 5, 5, 2, (2, 2)), (65, 3, 7, 7, 3, (3, 3)),
               (1, 1, 3, 3, 1, (1, 1)), (1, 40, 9, 9, 1, (4, 4)), (40, 1, 9, 9, 1, (4, 4))]


def _limits():
    return [(kh, kw, b) for kh in range(1, cl.MAX_KERNEL + 1) for kw in range(1, cl.MAX_KERNEL + 1) for b in range(1, cl.MAX_BIN + 1)]


# ---- the cases ------------------------------------------------------------------------------------------------------------------------
def test_lattice_holds_the_cases_it_was_given():
    assert len(cl.SMALL) == 688 and all(len(cl.small_cases(b)) == 86 for b in cl.SMALL_BINS)
    assert len(set(cl.SMALL)) == 688 and len(set(cl.LARGE)) == len(cl.LARGE)
    assert all(c[:3] == (1, 37, 41) and not c[7] and 1 <= c[3] <= 5 and 1 <= c[4] <= 5 for c in cl.SMALL)
    assert {c[5] for c in cl.SMALL} == set(range(1, 9))
    for kh in range(1, 6):
        for kw in range(1, 6):
            want = {(0, 0), (kh - 1, kw - 1), (kh // 2, kw // 2), (0, kw - 1)}
            assert {c[6] for c in cl.small_cases(3) if c[3:5] == (kh, kw)} == want
    for geometry in ISSUE_LARGE:                                  # the list may grow; it does not shrink
        assert (2,) + geometry + (True,) in cl.LARGE, geometry
    for c in cl.SMALL + cl.LARGE:                                 # every case is a legal call with at least one detector pixel
        planes, h, w, kh, kw, b, (ay, ax), _ = c
        assert kh <= cl.MAX_KERNEL and kw <= cl.MAX_KERNEL and b <= cl.MAX_BIN and 0 <= ay < kh and 0 <= ax < kw
        assert h // b >= 1 and w // b >= 1 and h <= 71 and w <= 71


def test_tags_cover_every_path():
    count = collections.Counter(t for c in cl.SMALL + cl.LARGE for t in cl.tags(c))
    print('tag coverage over', len(cl.SMALL), 'small and', len(cl.LARGE), 'large geometries (each under both boundaries):')
    numbered = lambda s: s.split('=')[0] in ('T', 'NM', 'NT', 'slices')          # noqa: E731
    for t in sorted(count, key=lambda s: (s.split('=')[0], int(s.split('=')[1])) if numbered(s) else (s, 0)):
        print(f'  {t}: {count[t]}')
    tiles = {int(t[2:]) for t in count if t.startswith('T=')}
    assert {f'NM={n}' for n in range(1, 5)} <= set(count)
    assert len(tiles) >= 8 and (4 in tiles or 5 in tiles) and {16, 32} <= tiles
    # every NT the plan can return inside the limits, for a frame of the lattice's size
    possible = {cl.psf_grad_plan(2, 70, 70, 2, kh, kw, b)['nt'] for kh, kw, b in _limits()}
    print('NT the plan can return:', sorted(possible))
    assert possible == {1, 2, 3, 4} and {f'NT={n}' for n in possible} <= set(count)
    assert any(t.startswith('slices=') for t in count) and 'slices=1' in count
    for t in cl.FLAG_TAGS:
        assert count[t] > 0, t
    # the large cases that the issue names by their path
    by_geometry = {c[1:7]: cl.tags(c) for c in cl.LARGE}
    for g in ISSUE_LARGE[:2]:
        assert {'lds-max', 'lds>64K', 'T=32', 'NM=4'} <= by_geometry[g]
    assert 'T=7' in by_geometry[ISSUE_LARGE[2]] and 'T=5' in by_geometry[ISSUE_LARGE[3]] and 'T=16' in by_geometry[ISSUE_LARGE[6]]
    for g in ISSUE_LARGE[7:9]:
        assert 'empty-tile' in by_geometry[g] and len(cl.unreachable_tiles(*g[:5], *g[5])) == 5
    assert 'H==bin' in by_geometry[ISSUE_LARGE[9]]
    assert {'one-high', 'one-wide'} <= by_geometry[ISSUE_LARGE[12]]
    assert 'one-high' in by_geometry[ISSUE_LARGE[13]] and 'one-wide' in by_geometry[ISSUE_LARGE[14]]
    # a clamped path needs its own cases: thin planes, corner anchors with bin > 1, a plane as high as one bin
    assert any('corner-anchor' in cl.tags(c) and c[5] > 1 and c[3] == 96 for c in cl.LARGE)


def test_every_bin_meets_an_unreachable_tile_and_a_kernel_narrower_than_the_bin():
    """``empty-tile`` and ``bin>kw`` at every bin at which they exist: 2 .. 8.  At bin 1 neither does -- bin > kw needs bin >= 2,
    and with out_h = H the last detector row's last tap row, H - 1 + (kh - 1 - ay), lies in the last tile -- which the scan below
    shows on the classifier instead of taking it on trust."""
    seen = collections.defaultdict(set)
    for c in cl.SMALL + cl.LARGE:
        for t in cl.tags(c) & {'empty-tile', 'bin>kw', 'bin>kh'}:
            seen[t].add(c[5])
    print({t: sorted(b) for t, b in seen.items()})
    assert seen['empty-tile'] == set(range(2, 9)) and seen['bin>kw'] == set(range(2, 9)) and seen['bin>kh'] == set(range(2, 9))
    for n in range(1, 71):
        for k in range(1, 9):
            for a in range(k):
                assert not cl.unreachable_tiles(n, n, k, k, 1, a, a), (n, k, a)
    # the issue's count on the square lattice of kernels and anchors: which of SMALL's geometries have such a tile
    per_bin = {b: sum('empty-tile' in cl.tags(c) for c in cl.small_cases(b)) for b in cl.SMALL_BINS}
    print('geometries of SMALL with an unreachable tile, per bin:', per_bin)
    assert per_bin[8] == 86 and per_bin[1] == 0


def test_adjoint_lds_stays_inside_the_device_and_peaks_at_96_96_1():
    sizes = {k: cl.adjoint_lds_bytes(*k) for k in _limits()}
    worst = max(sizes, key=sizes.get)
    above = sum(v > cl.LDS_OPT_IN for v in sizes.values())
    print(f'adjoint_lds_bytes over {len(sizes)} (kh, kw, bin): largest {sizes[worst]} B at {worst}; {above} above 64 KiB')
    assert len(sizes) == 73728 and max(sizes.values()) <= cl.LDS_LIMIT == 163840
    assert worst == (96, 96, 1) and sizes[worst] == cl.LDS_MAX == 139520
    assert [k for k, v in sizes.items() if v == cl.LDS_MAX] == [(96, 96, 1)]
    assert above == 3610
    # the forward's tile: at most 127 x 127 words, no opt-in
    assert max(((cl.corr_tile(*k) - 1) * k[2] + k[0]) * ((cl.corr_tile(*k) - 1) * k[2] + k[1]) for k in sizes) == 127 * 127
    assert min(cl.corr_tile(*k) for k in sizes) == 4 and 127 * 127 * 4 <= cl.LDS_OPT_IN


def test_classifier_against_worked_examples():
    """The restated host arithmetic on values worked out by hand from corr_bin.h and the header of the tap gradient."""
    assert cl.corr_tile(96, 96, 8) == 4 and cl.corr_tile(65, 65, 8) == 8 and cl.corr_tile(5, 5, 1) == 32 and cl.corr_tile(3, 3, 8) == 16
    assert cl.corr_outputs_per_thread(5, 5, 1) == 4 and cl.corr_outputs_per_thread(3, 3, 8) == 1 and cl.corr_outputs_per_thread(5, 5, 5) == 3
    assert cl.adjoint_lds_bytes(96, 96, 8) == (96 * 8 * 12 + 12) * 8 + (16 * 16 + 16) * 4          # about 75 KB: the one case tested before
    assert cl.ceil_div(-3, 2) == -1 and cl.floor_div(-3, 2) == -2 and cl.ceil_div(3, 2) == 2 and cl.ceil_div(-4, 2) == -2
    # 71 rows at bin 8, 3 x 3 taps anchored at their end: the last detector row is 7, its taps end at row 56: rows 64 .. 70 see none
    assert cl.adjoint_slice(71, 70, 3, 3, 8, 2, 2, 64, 0)[:2] == (8, 7)
    assert cl.unreachable_tiles(71, 70, 3, 3, 8, 2, 2) == [(0, 64), (32, 64), (64, 0), (64, 32), (64, 64)]
    assert cl.unreachable_tiles(70, 67, 9, 9, 2, 4, 4) == []
    # the header's examples: 3 x 3 taps keep 252 threads busy, 18 x 18 taps 243; 33 x 33 taps are two chunks of 545, three a thread
    assert cl.psf_grad_plan(1, 33, 65, 1, 3, 3, 1)['group'] * cl.psf_grad_plan(1, 33, 65, 1, 3, 3, 1)['slices'] == 252
    assert cl.psf_grad_plan(7, 48, 48, 1, 18, 18, 2)['group'] * cl.psf_grad_plan(7, 48, 48, 1, 18, 18, 2)['slices'] == 243
    plan = cl.psf_grad_plan(1, 6, 5, 1, 33, 33, 1)
    assert (plan['chunks'], plan['chunk_taps'], plan['nt']) == (2, 545, 3)
    assert cl.psf_grad_plan(1040, 4, 4, 1, 2, 2, 1)['n_runs'] == 512 and cl.psf_grad_plan(1040, 4, 4, 260, 2, 2, 1)['n_runs'] == 1


# ---- the restatements agree with each other ---------------------------------------------------------------------------------------
def _check_identity(cases, boundary, references):
    worst_used, worst_ratio, worst_case = 0.0, 0.0, None
    failures = []
    for case in cases:
        ref = references(case, boundary)
        values, bound, mass = cl.identity_check(case, boundary, ref)
        spread = max(values) - min(values)
        assert np.isfinite(values).all() and mass > 0 and np.isfinite(ref['taps']).all()
        scale_of_terms = float((np.abs(ref['forward_acc']) * np.abs(ref['g'].astype(np.float64))).sum())          # sum |A x| |g|
        if spread / bound > worst_used:
            worst_used, worst_case = spread / bound, case
        worst_ratio = max(worst_ratio, spread / scale_of_terms)
        if not spread <= bound:
            failures.append(f'{cl.describe(case)} {boundary}: {values!r} spread {spread:.3e} > bound {bound:.3e}')
    print(f'{len(cases)} geometries under {boundary}: largest spread of the three sums {worst_used:.3f} of its bound '
          f'(at {cl.describe(worst_case) if worst_case else "-"}), {worst_ratio:.2e} of sum |A x| |g| at most')
    assert not failures, '\n'.join(failures)


@pytest.mark.parametrize('boundary', cl.BOUNDARIES)
def test_restatements_agree_on_the_small_lattice(boundary):
    _check_identity(cl.SMALL, boundary, cl.references)


@pytest.mark.parametrize('boundary', cl.BOUNDARIES)
@pytest.mark.parametrize('case', cl.LARGE, ids=cl.large_id)
def test_restatements_agree_on_the_large_cases(case, boundary):
    _check_identity([case], boundary, cl.large_references)
