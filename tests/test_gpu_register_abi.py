"""The launching entry point of include/sunerf_hip_register.h checks its arguments in the documented order and stays inside its
buffers: the checks of tests/test_gpu_abi_extents.py (runs A and B with sentinel and NaN fills, guards, inputs -- the descriptor
table among them -- untouched, outputs equal to the wrapper's ``launch`` by bits and independent of what they held, the empty call,
the header's rejections) on cases built with ``abi_cases.Ctx`` / ``Case`` and the guarded arena of tests/abi_arena.py, with the extents
the header states: ``out`` at ``n_frames n_planes out_height out_width`` floats, ``status`` at one byte per pixel and frame, ``coords`` at
two doubles or NULL, ``state`` at 4 int64 per frame; per frame ``coefficients`` and ``mask`` at ``n_planes height width``, ``tx`` at
``width`` and ``ty`` at ``height``; there is no workspace.

The cases live in this file's own table ``REGISTER_CASES`` (tests/test_abi_tables_host.py holds it to the table's symbols)."""
import numpy as np
import pytest
import torch

import abi_cases as ac
import register_reference as rr
from abi_arena import OUT
from abi_cases import F32, F64, I64, STREAM, U8, Case, Ctx

pytestmark = pytest.mark.gpu

# (target, sources, planes, order, off_disk, flags, with coords): one pixel, one below and one above a tile on both axes, wider
# than two tiles, several frames of different shapes -- every order, both off-disk modes, with and without the optional buffers
SHAPES = [((1, 1), ((1, 1),), 1, 0, 1, 0, 1), ((15, 17), ((16, 16),), 1, 1, 0, 0, 0), ((17, 15), ((9, 21),), 2, 3, 1, 1, 1),
          ((16, 16), ((5, 7), (12, 3)), 1, 2, 1, 0, 1), ((3, 35), ((3, 3), (20, 18), (1, 6)), 3, 5, 1, 1, 0), ((33, 18), ((16, 40),), 1, 4, 0, 1, 1)]


def frames(shape, device):
    from sunerf_hip.register import FRAME_DESC, launch
    target, sources, c_, order, off_disk, flags, with_coords = shape
    c = Ctx(device)
    h, w = target
    rows = np.zeros(len(sources), dtype=FRAME_DESC)
    rng = np.random.default_rng(h + 10 * w)
    for i, (hk, wk) in enumerate(sources):
        planes = (2.0 + rng.standard_normal((c_, hk, wk)))
        coef = c.IN(f'frame{i}_coefficients', torch.from_numpy(planes))
        flagged = np.zeros(planes.shape, dtype=np.uint8)
        flagged.reshape(-1)[::5] = 1
        mask = c.IN(f'frame{i}_mask', torch.from_numpy(flagged)) if (flags and i != 1) else None          # frame 1: a NULL mask
        tx_k, ty_k = rr.axes_for((hk, wk), 1.25 * rr.DISK, descending_y=bool(i & 1))
        tx, ty = c.IN(f'frame{i}_tx', torch.from_numpy(tx_k.copy())), c.IN(f'frame{i}_ty', torch.from_numpy(ty_k.copy()))
        rows[i]['coefficients'], rows[i]['mask'] = coef.ptr.value, mask.ptr.value if mask is not None else 0
        rows[i]['tx'], rows[i]['ty'], rows[i]['height'], rows[i]['width'] = tx.ptr.value, ty.ptr.value, hk, wk
        rows[i]['c2w'] = rr.look_at_pose(0.05 * i, 0.3 - 0.25 * i, rr.AU * (1.0 - 0.02 * i)).reshape(-1)
        rows[i]['dt'], rows[i]['shift_y'], rows[i]['shift_x'] = 1.5 - i, 0.3 * i, -0.45 * i
    table = c.IN('frames', torch.from_numpy(rows.view(np.uint8).reshape(-1).copy()))
    tx_r, ty_r = rr.axes_for(target, 1.25 * rr.DISK)
    c2w_ref = c.IN('c2w_ref', torch.from_numpy(rr.look_at_pose(0.0, 0.0, rr.AU).reshape(-1).copy()))
    tx_ref, ty_ref = c.IN('tx_ref', torch.from_numpy(tx_r.copy())), c.IN('ty_ref', torch.from_numpy(ty_r.copy()))
    t = len(sources)
    out, status = c.OUT('out', F32, t * c_ * h * w), c.OUT('status', U8, t * h * w)
    coords = c.OUT('coords', F64, t * 2 * h * w) if with_coords else c.NULL('coords', OUT)
    state = c.OUT('state', I64, 4 * t)
    law = (1.0, *rr.FAST)          # radius, A, B, C

    def expected():
        image, st, co, counts = launch(table.t, t, c_, order, c2w_ref.t, tx_ref.t, ty_ref.t, *law, off_disk, -3.25, flags, want_coords=bool(with_coords))
        want = {'out': image, 'status': st, 'state': counts}
        if with_coords:
            want['coords'] = co
        return want
    args = [table, t, c_, order, c2w_ref, tx_ref, ty_ref, h, w, *law, off_disk, -3.25, flags, out, status, coords, state, STREAM]
    return Case('sunerf_register_frames', shape, c.arena, args, expected, empty={1: 0},
                rejections=[({3: -1}, -2), ({3: 6}, -2), ({13: 2}, -2), ({13: -1}, -2), ({15: 2}, -2), ({15: 4}, -2), ({3: 6, 1: 0}, -2),
                            ({1: -1}, -1), ({2: -1}, -1), ({2: 0}, -1), ({7: -1}, -1), ({8: -1}, -1), ({1: 65536}, -1),
                            ({9: 0.0}, -1), ({9: float('nan')}, -1), ({9: float('inf')}, -1), ({10: float('nan')}, -1),
                            ({11: float('inf')}, -1), ({12: -float('inf')}, -1), ({0: None}, -1), ({4: None}, -1), ({5: None}, -1),
                            ({6: None}, -1), ({16: None}, -1), ({17: None}, -1), ({19: None}, -1)])


REGISTER_CASES = {'sunerf_register_frames': (frames, tuple(SHAPES))}
PAIRS = [(name, shape) for name, (_, shapes) in REGISTER_CASES.items() for shape in shapes]


def test_argument_checks_come_in_the_documented_order():
    """The checks of tests/test_register_host.py on the library the GPU tests run: no call reaches a launch."""
    from sunerf_hip import lib
    from test_register_host import check_argument_order
    check_argument_order(lib.load())


@pytest.mark.parametrize('name,shape', PAIRS, ids=[f'{n[7:]}-{ac.shape_id(s)}' for n, s in PAIRS])
def test_register_entry_point_stays_inside_its_buffers(name, shape):
    import test_gpu_abi_extents as extents
    extents.check_entry_point(REGISTER_CASES[name][0], name, shape)
    for empty in ({7: 0}, {8: 0}):          # out_height or out_width 0: nothing to do, nothing written
        case = frames(shape, torch.device('cuda', torch.cuda.current_device()))
        case.arena.fill_guards('A')
        case.arena.fill_payload('A', (OUT,))
        before = case.arena.payload_bits()
        assert extents._call(case, case.arena.device, empty) == 0
        extents._check_guards(case, f'empty call {empty}')
        extents._untouched(case, before, f'empty call {empty}')
