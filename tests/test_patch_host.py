"""CPU-only checks of training through the instrument (no GPU): the restatement tests/patch_reference.py of the
adjoint against the committed restatement of the forward (tests/instrument_reference.py, imported unchanged) -- the inner-product
identity in fp64 and, for small planes, the dense transpose built from unit impulses; the patch lattice, the rank shards and the
extended sub-pixel axes of sunerf_hip/patch.py; and the sixth entry-point table (declared, bound, kept out of the other five, its
argument checks in their documented order).

Gate of the fp64 comparisons: 1e-13 relative.  Both sides of either comparison add the same products K * x * g in different orders;
with at most 96 * 96 * 25 terms of mixed sign per sum the difference stays some 1e-15 of the sum of their magnitudes (the largest
figures are printed), two orders of magnitude inside the gate, while a tap assigned to a wrong pixel is an error of order one."""
import ctypes
import os
import re

import numpy as np
import pytest

import instrument_reference as ir
import patch_reference as pr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GATE = 1e-13


@pytest.fixture(scope='session')
def lib():
    import sunerf_hip
    if not os.path.exists(sunerf_hip.LIB_PATH):
        import subprocess
        subprocess.check_call(['bash', os.path.join(ROOT, '2024-hl-spi3s-sunerf_amd', 'csrc', 'build.sh')])
    return sunerf_hip.load()


# ---- 1. the adjoint restatement ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('boundary', pr.BOUNDARIES)
@pytest.mark.parametrize('case', pr.ADJOINT_CASES + pr.SEAM_CASES, ids=lambda c: '-'.join(str(v) for v in c[:6]))
def test_adjoint_restatement_is_the_transpose_of_the_forward(case, boundary):
    planes, h, w, kh, kw, b, anchor, per_plane = case
    K, x, g = pr.case_data(case)
    _, ax = ir.correlate_bin(x, K, b, anchor, 1.0, boundary)                          # A x, fp64
    _, atg = pr.correlate_bin_adjoint(g, K, h, w, b, anchor, 1.0, boundary)          # A^T g, fp64
    g64, x64 = g.astype(np.float64), x.astype(np.float64)
    lhs, rhs = float((ax * g64).sum()), float((x64 * atg).sum())
    magnitude = float((np.abs(ax) * np.abs(g64)).sum())
    rel, rel_mag = abs(lhs - rhs) / max(abs(lhs), abs(rhs)), abs(lhs - rhs) / magnitude
    print(f'<A x, g> = {lhs:.17g}, <x, A^T g> = {rhs:.17g}: relative {rel:.3g}, of the terms\' magnitudes {rel_mag:.3g}')
    assert rel <= GATE
    if h * w <= 150:
        for p in range(planes):
            Kp = K[p if per_plane else 0]
            dense = np.empty((h // b * (w // b), h * w))
            for k in range(h * w):
                impulse = np.zeros((1, h, w), dtype=np.float32)
                impulse.reshape(-1)[k] = 1.0
                dense[:, k] = ir.correlate_bin(impulse, Kp, b, anchor, 1.0, boundary)[1].reshape(-1)
            want = dense.T @ g64[p].reshape(-1)
            bound = GATE * (np.abs(dense).T @ np.abs(g64[p]).reshape(-1))
            err = np.abs(want - atg[p].reshape(-1))
            worst = float((err / np.maximum(bound / GATE, 1e-300)).max())
            print(f'plane {p}: dense transpose, largest error {worst:.3g} of the terms\' magnitudes, absolute {float(err.max()):.3g}')
            assert bool((err <= bound).all())


def test_adjoint_restatement_scales_and_rounds_once():
    case = pr.ADJOINT_CASES[8]
    K, _, g = pr.case_data(case)
    out, acc = pr.correlate_bin_adjoint(g, K, case[1], case[2], case[5], case[6], 0.25, 'zero')
    assert out.dtype == np.float32 and np.array_equal(out, (0.25 * acc).astype(np.float32))
    # the trailing row and column of the 67 x 35 frame under bin 2 fill no detector pixel but are read by taps
    assert np.abs(acc[0, 66]).max() > 0 and np.abs(acc[0, :, 34]).max() > 0


# ---- 2. lattice, shards, axes -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('n,patch', [(16, 16), (17, 16), (31, 16), (32, 16), (12, 4), (10, 4), (9, 4), (4, 4), (5, 1)])
def test_lattice_covers_every_pixel_and_ends_at_the_edge(n, patch):
    from sunerf_hip.patch import lattice
    starts = lattice(n, patch)
    assert starts == pr.lattice(n, patch)
    covered = np.zeros(n, dtype=np.int64)
    for s in starts:
        assert 0 <= s and s + patch <= n
        covered[s:s + patch] += 1
    assert covered.min() >= 1 and starts[-1] + patch == n
    assert starts[:-1] == [k * patch for k in range(len(starts) - 1)]
    assert int((covered > 1).sum()) == ((patch - n % patch) if n % patch else 0)


def test_a_view_smaller_than_the_patch_raises():
    from sunerf_hip.patch import lattice
    with pytest.raises(ValueError):
        lattice(3, 4)


def test_four_ranks_shards_are_disjoint_and_their_union_is_one_permutation():
    from sunerf_hip.patch import epoch_order
    n = 37
    for epoch in (0, 1):
        shards = [epoch_order(n, 5, epoch, r, 4) for r in range(4)]
        whole = np.random.default_rng([5, epoch]).permutation(n)
        for r, s in enumerate(shards):
            assert np.array_equal(s, whole[r::4])
        union = np.concatenate(shards)
        assert union.size == n and np.array_equal(np.sort(union), np.arange(n))
    assert not np.array_equal(epoch_order(n, 5, 0), epoch_order(n, 5, 1))


@pytest.mark.parametrize('b,k_eff,anchor', [(1, 1, 0), (2, 4, 1), (2, 10, 4), (3, 7, 3), (8, 96, 48)])
def test_extended_axis_is_the_fine_frames_axis_inside_the_frame(b, k_eff, anchor):
    from sunerf.evaluation.loader import linear_plate_scale_axes
    from sunerf_hip.observations import resampled_grid
    from sunerf_hip.patch import extended_axis
    h, w = 9, 12
    grid = {'shape': (h, w), 'cdelt': (4.8, 5.1), 'crpix': (6.25, 4.5), 'crval': (12.0, -30.0)}
    tx, ty = (a.numpy() for a in linear_plate_scale_axes(grid, None, 'cpu'))
    fx, fy = (a.numpy() for a in linear_plate_scale_axes(resampled_grid(grid, (h * b, w * b)), None, 'cpu'))
    for axis, fine, n in ((tx, fx, w), (ty, fy, h)):
        ext = extended_axis(axis, b, k_eff, anchor)
        assert ext.dtype == np.float64 and ext.shape == ((n - 1) * b + k_eff,)
        assert np.array_equal(ext.astype(np.float32), pr.extended_axis(axis, b, k_eff, anchor))
        assert np.array_equal(ext, ext.astype(np.float32).astype(np.float64))          # rounded to fp32 once
        inside = ext[anchor:anchor + min(n * b, ext.shape[0] - anchor)]
        want = fine[:inside.shape[0]]
        diff = np.abs(inside - want)
        ulp = np.spacing(np.abs(want).astype(np.float32)).astype(np.float64)
        print(f'bin {b}: extended axis against the resampled grid, largest difference {float(diff.max()):.3g} rad = '
              f'{float((diff / ulp).max()):.3g} fp32 ulp')
        # fp32 rounding (half an ulp) and the two fp64 evaluations of the same angle (1e-16 of it)
        assert bool((diff <= 0.5 * ulp + 1e-15 * np.abs(want) + 1e-22).all())
        # past the edge the axis goes on at the same step
        step = np.diff(ext)
        assert np.allclose(step, (axis[-1] - axis[0]) / (n - 1) / b, rtol=1e-4)


def test_extended_axis_rejections():
    from sunerf_hip.patch import extended_axis
    with pytest.raises(ValueError):
        extended_axis(np.zeros((3, 3)), 2, 3, 1)
    with pytest.raises(ValueError):
        extended_axis(np.array([0.0, 1.0, 3.0]), 2, 3, 1)
    with pytest.raises(ValueError):
        extended_axis(np.array([1.0]), 2, 3, 1)


# ---- 3. the sixth table -----------------------------------------------------------------------------------------------------------
def test_entry_points_are_declared_bound_and_kept_out_of_the_other_tables(lib):
    """(The table itself -- declared, bound, frozen, versioned, built, its symbols in no other table or older header:
    tests/test_abi_tables_host.py.)"""
    from sunerf_hip import lib as binding, patch
    header = open(os.path.join(ROOT, 'include', 'sunerf_hip_patch.h')).read()
    # the adjoint takes the forward's arguments, position by position
    assert binding.signature('sunerf_patch_correlate_bin_adjoint') == binding.signature('sunerf_instrument_correlate_bin')
    assert lib.sunerf_abi_version() == 9 and lib.sunerf_ext_abi_version() == 1 and lib.sunerf_response_abi_version() == 1
    assert lib.sunerf_prep_abi_version() == 1 and lib.sunerf_instrument_abi_version() == 1
    assert lib.sunerf_patch_abi_version() == 1
    assert '#define SUNERF_PATCH_TILE 32' in header
    assert f'#define SUNERF_PATCH_VIEW_DESC_BYTES {patch.PATCH_VIEW_DESC.itemsize}' in header


def test_view_descriptor_layout_follows_the_header():
    from sunerf_hip.patch import PATCH_VIEW_DESC
    header = open(os.path.join(ROOT, 'include', 'sunerf_hip_patch.h')).read()
    body = header[header.index('typedef struct SunerfPatchViewDesc {'):header.index('} SunerfPatchViewDesc;')]
    fields = re.findall(r'^\s*(?:const\s+)?(\w+)\*?\s+\*?([\w, \[\]]+);', body, flags=re.M)
    names = []
    for ctype, decl in fields:
        names += [n.strip().split('[')[0] for n in decl.split(',')]
    assert tuple(names) == PATCH_VIEW_DESC.names, names
    sizes = {'tx': 8, 'ty': 8, 'image': 8, 'height': 4, 'width': 4, 'c2w': 48, 'time': 4, 'n_planes': 4, 'plane': 64, 'wavelength': 64}
    offset = 0
    for name in PATCH_VIEW_DESC.names:
        assert PATCH_VIEW_DESC.fields[name][1] == offset and PATCH_VIEW_DESC.fields[name][0].itemsize == sizes[name], name
        offset += sizes[name]
    assert offset == PATCH_VIEW_DESC.itemsize == 216


def check_argument_order(lib):
    """Unsupported (-2) first, then the empty call (0), then bad counts and null pointers (-1): all before anything touches a
    device, so this runs without one.  ``P`` stands for any non-null pointer: no call here reaches a launch."""
    P = ctypes.c_void_p(4096)
    adj = lib.sunerf_patch_correlate_bin_adjoint
    #          g_out n  h  w  K nk kh kw b ay ax scale bd g_in stream -- the forward's checks, call for call
    assert adj(None, 0, 4, 4, None, 1, 97, 3, 1, 0, 0, 1.0, 0, None, None) == -2
    assert adj(None, 0, 4, 4, None, 1, 3, 97, 1, 0, 0, 1.0, 0, None, None) == -2
    assert adj(None, 0, 4, 4, None, 1, 3, 3, 9, 0, 0, 1.0, 0, None, None) == -2
    assert adj(None, 0, 4, 4, None, 1, 3, 3, 1, 0, 0, 1.0, 2, None, None) == -2
    assert adj(None, -1, 4, 4, None, 1, 97, 3, 1, 0, 0, 1.0, 0, None, None) == -2          # unsupported comes before bad counts
    assert adj(None, 0, 4, 4, None, 1, 3, 3, 1, 0, 0, 1.0, 0, None, None) == 0
    assert adj(None, 2, 3, 8, None, 1, 3, 3, 4, 0, 0, 1.0, 1, None, None) == 0              # 3 // 4 rows
    assert adj(None, 2, 8, 0, None, 1, 96, 96, 8, 0, 0, 1.0, 1, None, None) == 0
    assert adj(P, -1, 4, 4, P, 1, 3, 3, 1, 0, 0, 1.0, 0, P, None) == -1
    assert adj(P, 0, 4, 4, P, 1, 0, 3, 1, 0, 0, 1.0, 0, P, None) == -1                      # kh < 1 is no empty call
    assert adj(P, 1, 4, 4, P, 1, 3, 3, 0, 0, 0, 1.0, 0, P, None) == -1
    assert adj(P, 3, 4, 4, P, 2, 3, 3, 1, 0, 0, 1.0, 0, P, None) == -1                      # 2 kernels for 3 planes
    assert adj(P, 1, 4, 4, P, 1, 3, 3, 1, 3, 0, 1.0, 0, P, None) == -1 and adj(P, 1, 4, 4, P, 1, 3, 3, 1, 0, -1, 1.0, 0, P, None) == -1
    for k in range(3):
        ptrs = [P] * 3
        ptrs[k] = None
        assert adj(ptrs[0], 1, 4, 4, ptrs[1], 1, 3, 3, 1, 1, 1, 1.0, 0, ptrs[2], None) == -1
    assert adj(P, 1, 4, 4, ctypes.c_void_p(4100), 1, 3, 3, 1, 1, 1, 1.0, 0, P, None) == -1          # K not aligned to 8 bytes

    rec = lib.sunerf_patch_records
    #          views nv patches n  C  P  b kh kw rays time target wl stream
    assert rec(None, 0, None, 0, 1, 4, 1, 97, 3, None, None, None, None, None) == -2
    assert rec(None, 0, None, 0, 1, 4, 1, 3, 97, None, None, None, None, None) == -2
    assert rec(None, 0, None, -1, 1, 4, 9, 3, 3, None, None, None, None, None) == -2       # unsupported comes before bad counts
    assert rec(None, 0, None, 0, 0, 4, 2, 3, 3, None, None, None, None, None) == 0          # no patch: nothing else is looked at
    assert rec(P, 1, P, -1, 1, 4, 2, 3, 3, P, P, P, None, None) == -1
    assert rec(P, 1, P, 0, 1, 0, 2, 3, 3, P, P, P, None, None) == -1                        # P < 1 is no empty call
    assert rec(P, 1, P, 0, 1, 4, 0, 3, 3, P, P, P, None, None) == -1
    assert rec(P, 1, P, 0, 1, 4, 2, 0, 3, P, P, P, None, None) == -1
    assert rec(P, 0, P, 2, 1, 4, 2, 3, 3, P, P, P, None, None) == -1
    assert rec(P, 1, P, 2, 0, 4, 2, 3, 3, P, P, P, None, None) == -1 and rec(P, 1, P, 2, 17, 4, 2, 3, 3, P, P, P, None, None) == -1
    assert rec(P, 1, P, 2 ** 20, 1, 64, 8, 96, 96, P, P, P, None, None) == -1                # 2^20 windows of 600 x 600 rays
    for k in range(5):
        ptrs = [P] * 5
        ptrs[k] = None
        assert rec(ptrs[0], 1, ptrs[1], 2, 1, 4, 2, 3, 3, ptrs[2], ptrs[3], ptrs[4], None, None) == -1


def test_argument_checks_come_in_the_documented_order(lib):
    check_argument_order(lib)


def test_expected_windows_host_side_rejections():
    import torch
    from sunerf_hip import SunerfHipError
    from sunerf_hip.instrument import Instrument
    inst = Instrument(psf=np.ones((3, 3)) / 9, bin=2)
    assert inst.window_shape(4) == (10, 10)
    with pytest.raises(SunerfHipError):
        inst.expected_windows(torch.zeros(1, 1, 10, 10))
    with pytest.raises(TypeError):
        inst.expected_windows(np.zeros((1, 1, 10, 10), dtype=np.float32))
