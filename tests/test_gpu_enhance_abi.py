"""The launching entry points of include/sunerf_hip_enhance.h check their arguments in the documented order and stay inside their
buffers: the checks of tests/test_gpu_abi_extents.py (runs A and B with sentinel and NaN fills, guards, inputs untouched, outputs
equal to the wrapper's launch functions by bits and independent of what they and the workspace held, the workspace bound, the empty
call, the header's rejections) on cases built with ``abi_cases.Ctx`` / ``Case`` and the guarded arena of tests/abi_arena.py, with the
extents the header states: MGN's ``out`` at the size of the image, ``lo_out`` / ``hi_out`` at one float and ``state`` at 3 int64 per
plane, the workspace at ``sunerf_enhance_mgn_workspace_bytes``; the ring tables at ``n_planes n_rings n_segments``; NRGF's ``out`` at
the size of the image and ``state`` at 3 int64 per plane.

The cases live in this file's own table ``ENHANCE_CASES`` (tests/test_abi_tables_host.py holds it to the table's symbols)."""
import ctypes

import numpy as np
import pytest
import torch

import abi_cases as ac
from abi_arena import IN, OUT
from abi_cases import F32, F64, I64, STREAM, Case, Ctx, HostValue

pytestmark = pytest.mark.gpu

# (planes, height, width, sigma, with bad, with lo / hi / floor): one pixel, an image smaller than the window, one row, one column,
# one below, at and above the row tile (4 x 512) and the column tile (128 x 32), several planes with the widest window
MGN_SHAPES = [(1, 1, 1, (1.25,), 0, 0), (1, 5, 7, (40.0,), 1, 0), (1, 1, 300, (2.5, 10.0), 0, 1), (1, 300, 1, (2.5, 10.0), 1, 1),
              (1, 3, 511, (5.0,), 1, 0), (2, 4, 512, (0.1, 1.25), 0, 0), (1, 5, 513, (5.0,), 1, 1), (1, 127, 31, (5.0,), 1, 0),
              (1, 128, 32, (1.25,), 0, 1), (1, 129, 33, (5.0,), 1, 0), (3, 37, 45, (1.25, 42.6), 1, 1)]
# (planes, height, width, rings, segments, with bad)
RING_SHAPES = [(1, 1, 1, 1, 1, 0), (2, 9, 11, 3, 1, 1), (1, 5, 300, 4, 1, 0), (1, 300, 5, 4, 7, 1), (1, 7, 530, 2, 360, 0), (2, 33, 31, 4096, 1, 1),
               (1, 33, 31, 182, 360, 0)]
# (planes, height, width, rings, outside, compute, with bad)
NRGF_SHAPES = [(1, 1, 1, 1, 0, 1, 0), (2, 9, 11, 3, 1, 1, 1), (1, 16, 16, 5, 0, 0, 0), (1, 15, 17, 5, 1, 0, 1), (3, 5, 257, 4096, 0, 1, 1), (1, 300, 3, 40, 1, 1, 0)]


def _planes(c_, h, w, flagged):
    rng = np.random.default_rng(c_ + 10 * h + 100 * w)
    planes = (5.0 + rng.standard_normal((c_, h, w))).astype(np.float32)
    bad = np.zeros(planes.shape, dtype=np.uint8)
    if flagged and planes.size > 1:
        planes.reshape(-1)[::7] = np.nan
        planes.reshape(-1)[3::11] = np.inf
        bad.reshape(-1)[::5] = 1
    return planes, bad


def mgn(shape, device):
    from sunerf_hip.enhance import mgn_launch
    c_, h, w, sigma, with_bad, with_range = shape
    c = Ctx(device)
    planes, flagged = _planes(c_, h, w, with_bad)
    image = c.IN('image', torch.from_numpy(planes))
    bad = c.IN('bad', torch.from_numpy(flagged)) if with_bad else c.NULL('bad', IN)
    given = {k: (c.IN(k, torch.full((c_,), v, dtype=torch.float32)) if with_range else c.NULL(k, IN)) for k, v in (('lo', 4.5), ('hi', 6.0), ('floor', 0.125))}
    sig = np.asarray(sigma, dtype=np.float64)
    wts = np.linspace(0.5, 1.5, len(sigma)).astype(np.float32)
    out, lo_out, hi_out, state = c.OUT('out', F32, c_ * h * w), c.OUT('lo_out', F32, c_), c.OUT('hi_out', F32, c_), c.OUT('state', I64, 3 * c_)
    nbytes = int(ac._lib().sunerf_enhance_mgn_workspace_bytes(c_, h, w))
    ws = c.WS('workspace', nbytes)
    call = (3.0, 0.9, 2.4, 0.6)          # truncate, k, gamma, h

    def expected():
        image_out, lo_, hi_, st = mgn_launch(image.t.view(c_, h, w), bad.t.view(c_, h, w) if with_bad else None, sig, wts, *call,
                                             *(given[k].t if with_range else None for k in ('lo', 'hi', 'floor')))
        return {'out': image_out, 'lo_out': lo_, 'hi_out': hi_, 'state': st}
    host = lambda a: HostValue(a.ctypes.data_as(ctypes.c_void_p), keep=a)          # noqa: E731
    args = [image, bad, c_, h, w, host(sig), host(wts), len(sigma), *call, given['lo'], given['hi'], given['floor'], out, lo_out, hi_out, state, ws, nbytes,
            STREAM]
    wide = np.asarray([43.0] * len(sigma))
    return Case('sunerf_enhance_mgn', shape, c.arena, args, expected, ws_index=20, empty={2: 0},
                rejections=[({7: 0}, -2), ({7: 9}, -2), ({5: host(wide)}, -2), ({5: host(wide), 2: 0}, -2), ({5: None}, -1), ({8: -1.0}, -1), ({8: float('nan')}, -1),
                            ({2: -1}, -1), ({3: -1}, -1), ({4: -1}, -1), ({2: 65536}, -1), ({9: float('nan')}, -1), ({10: 0.0}, -1), ({11: float('inf')}, -1),
                            ({0: None}, -1), ({15: None}, -1), ({16: None}, -1), ({17: None}, -1), ({18: None}, -1), ({19: None}, -1)])


def _edges(h, w, rings):
    return np.linspace(0.5, 0.75 * max(h, w), rings + 1)


def statistics(shape, device):
    from sunerf_hip.enhance import statistics_launch
    c_, h, w, rings, segments, with_bad = shape
    c = Ctx(device)
    planes, flagged = _planes(c_, h, w, with_bad)
    image = c.IN('image', torch.from_numpy(planes))
    bad = c.IN('bad', torch.from_numpy(flagged)) if with_bad else c.NULL('bad', IN)
    edges = c.IN('edges', torch.from_numpy(_edges(h, w, rings)))
    bins = c_ * rings * segments
    count = c.OUT('count', I64, bins)
    mean, std, mn, mx = (c.OUT(k, F64, bins) for k in ('mean', 'std', 'min', 'max'))
    center = (0.4 * h + 0.3, 0.5 * w - 0.4)

    def expected():
        got = statistics_launch(image.t.view(c_, h, w), bad.t.view(c_, h, w) if with_bad else None, *center, edges.t, segments)
        return dict(zip(('count', 'mean', 'std', 'min', 'max'), got))
    args = [image, bad, c_, h, w, *center, edges, rings, segments, count, mean, std, mn, mx, STREAM]
    return Case('sunerf_enhance_radial_statistics', shape, c.arena, args, expected, empty={3: 0},
                rejections=[({8: 0}, -2), ({8: 4097}, -2), ({9: 0}, -2), ({9: 361}, -2), ({8: 4096, 9: 17}, -2), ({8: 0, 2: 0}, -2), ({2: -1}, -1), ({3: -1}, -1),
                            ({4: -1}, -1), ({5: float('nan')}, -1), ({6: float('inf')}, -1), ({0: None}, -1), ({7: None}, -1), ({10: None}, -1),
                            ({11: None}, -1), ({12: None}, -1), ({13: None}, -1), ({14: None}, -1)])


def nrgf(shape, device):
    from sunerf_hip.enhance import nrgf_launch, statistics_launch
    c_, h, w, rings, outside, compute, with_bad = shape
    c = Ctx(device)
    planes, flagged = _planes(c_, h, w, with_bad)
    image = c.IN('image', torch.from_numpy(planes))
    bad = c.IN('bad', torch.from_numpy(flagged)) if with_bad else c.NULL('bad', IN)
    edges = c.IN('edges', torch.from_numpy(_edges(h, w, rings)))
    center = (0.4 * h + 0.3, 0.5 * w - 0.4)
    bins = c_ * rings
    if compute:
        count = c.OUT('count', I64, bins)
        mean, std, mn, mx = (c.OUT(k, F64, bins) for k in ('mean', 'std', 'min', 'max'))
    else:          # the caller's table: read only, min and max absent
        rng = np.random.default_rng(rings)
        count = c.IN('count', torch.from_numpy(rng.integers(0, 4, bins)))
        mean, std = c.IN('mean', torch.from_numpy(5.0 + rng.standard_normal(bins))), c.IN('std', torch.from_numpy(np.abs(rng.standard_normal(bins)).round(1)))
        mn, mx = c.NULL('min', OUT), c.NULL('max', OUT)
    out, state = c.OUT('out', F32, c_ * h * w), c.OUT('state', I64, 3 * c_)

    def expected():
        given = None if compute else tuple(b.t.view(c_, rings) for b in (count, mean, std))
        image_out, st, table = nrgf_launch(image.t.view(c_, h, w), bad.t.view(c_, h, w) if with_bad else None, *center, edges.t, outside, -3.25, given)
        want = {'out': image_out, 'state': st}
        if compute:
            want.update(zip(('count', 'mean', 'std', 'min', 'max'), table))
        return want
    args = [image, bad, c_, h, w, *center, edges, rings, outside, -3.25, compute, count, mean, std, mn, mx, out, state, STREAM]
    return Case('sunerf_enhance_nrgf', shape, c.arena, args, expected, empty={4: 0},
                rejections=[({8: 0}, -2), ({8: 4097}, -2), ({9: 2}, -2), ({9: -1}, -2), ({9: 2, 3: 0}, -2), ({2: -1}, -1), ({3: -1}, -1), ({4: -1}, -1), ({2: 65536}, -1),
                            ({5: float('nan')}, -1), ({6: -float('inf')}, -1), ({0: None}, -1), ({7: None}, -1), ({12: None}, -1), ({13: None}, -1),
                            ({14: None}, -1), ({17: None}, -1), ({18: None}, -1)] + ([({15: None}, -1), ({16: None}, -1)] if compute else []))


ENHANCE_CASES = {'sunerf_enhance_mgn': (mgn, tuple(MGN_SHAPES)), 'sunerf_enhance_radial_statistics': (statistics, tuple(RING_SHAPES)),
                 'sunerf_enhance_nrgf': (nrgf, tuple(NRGF_SHAPES))}
PAIRS = [(name, shape) for name, (_, shapes) in ENHANCE_CASES.items() for shape in shapes]


def test_argument_checks_come_in_the_documented_order():
    """The checks of tests/test_enhance_host.py on the library the GPU tests run: no call reaches a launch."""
    from sunerf_hip import lib
    from test_enhance_host import check_argument_order
    check_argument_order(lib.load())


@pytest.mark.parametrize('name,shape', PAIRS, ids=[f'{n[7:]}-{ac.shape_id(s)}' for n, s in PAIRS])
def test_enhance_entry_point_stays_inside_its_buffers(name, shape):
    import test_gpu_abi_extents as extents
    extents.check_entry_point(ENHANCE_CASES[name][0], name, shape)
    builder, _ = ENHANCE_CASES[name]
    for empty in ({2: 0}, {3: 0}, {4: 0}):          # no plane, no row, no column: nothing to do, nothing written
        case = builder(shape, torch.device('cuda', torch.cuda.current_device()))
        case.arena.fill_guards('A')
        case.arena.fill_payload('A', (OUT, ac.WORKSPACE))
        before = case.arena.payload_bits()
        assert extents._call(case, case.arena.device, empty) == 0
        extents._check_guards(case, f'empty call {empty}')
        extents._untouched(case, before, f'empty call {empty}')
