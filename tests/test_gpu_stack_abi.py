"""The launching entry point of include/sunerf_hip_stack.h checks its arguments in the documented order and stays inside its
buffers: the checks of tests/test_gpu_abi_extents.py (runs A and B with sentinel and NaN fills, guards, inputs untouched, outputs
equal to the wrapper by bits and independent of what they held, the empty call, the header's rejections) on cases built with
``abi_cases.Ctx`` / ``Case`` and the guarded arena of tests/abi_arena.py, with the extents the header states: ``image`` and
``count`` at ``n_planes height width``, ``mask`` at ``n_frames`` times that or NULL, ``state`` at 4 int64 per plane; there is no
workspace.

The cases live in this file's own table ``STACK_CASES`` (tests/test_abi_tables_host.py holds it to the table's symbols)."""
import numpy as np
import pytest
import torch

import abi_cases as ac
from abi_arena import IN, OUT
from abi_cases import F32, I64, STREAM, U8, Case, Ctx

pytestmark = pytest.mark.gpu

# (frames, planes, height, width, method, mode, flags, iterations, with bad, with mask): one frame and 64 of them, one pixel, a
# partial wave, one pixel past a workgroup of 256, several planes -- with the mask NULL and given, with and without flags
SHAPES = [(1, 1, 1, 1, 1, 0, 0, 0, 0, 1), (64, 1, 1, 1, 0, 0, 1, 4, 1, 1), (1, 2, 3, 35, 3, 0, 0, 0, 1, 0), (64, 1, 3, 35, 2, 1, 1, 3, 0, 1),
          (9, 3, 1, 257, 0, 0, 0, 2, 1, 1), (9, 3, 1, 257, 1, 1, 0, 2, 0, 0), (33, 2, 5, 67, 2, 0, 1, 16, 1, 1), (5, 2, 5, 67, 0, 0, 0, 1, 1, 0)]


def combine(shape, device):
    from sunerf_hip.stack import launch
    from test_gpu_stack import make_stack, params_of
    t, c_, h, w, method, mode, flags, iterations, with_bad, with_mask = shape
    c = Ctx(device)
    planes, flagged = make_stack(t, (c_, h, w))
    frames = c.IN('frames', torch.from_numpy(planes.copy()))
    bad = c.IN('bad', torch.from_numpy(flagged.copy())) if with_bad else c.NULL('bad', IN)
    params = c.IN('params', torch.from_numpy(np.ascontiguousarray(params_of(c_), dtype=np.float64)))
    image, count, state = c.OUT('image', F32, c_ * h * w), c.OUT('count', U8, c_ * h * w), c.OUT('state', I64, 4 * c_)
    mask = c.OUT('mask', U8, t * c_ * h * w) if with_mask else c.NULL('mask', OUT)
    call = (method, 30.0, -2, mode, flags, 2.0, iterations, 3, 2)

    def expected():
        img, cnt, msk, st = launch(frames.t.view(t, c_, h, w), bad.t.view(t, c_, h, w) if with_bad else None, params.t.view(c_, 4),
                                   *call, with_mask=bool(with_mask))
        out = {'image': img, 'count': cnt, 'state': st}
        if with_mask:
            out['mask'] = msk
        return out
    args = [frames, bad, params, t, c_, h, w, *call, image, count, mask, state, STREAM]
    return Case('sunerf_stack_combine', shape, c.arena, args, expected, empty={4: 0},
                rejections=[({3: 65}, -2), ({13: 17}, -2), ({7: 4}, -2), ({10: 2}, -2), ({11: 2}, -2), ({3: 65, 4: 0}, -2), ({3: 0}, -1),
                            ({4: -1}, -1), ({13: -1}, -1), ({14: 1}, -1), ({15: 0}, -1), ({12: 0.0}, -1), ({12: float('nan')}, -1),
                            ({7: 2, 8: 100.5}, -1), ({16: frames}, -1), ({17: frames}, -1), ({18: frames}, -1)]
                + ([({16: bad}, -1), ({17: bad}, -1), ({18: bad}, -1)] if with_bad else []))


STACK_CASES = {'sunerf_stack_combine': (combine, tuple(SHAPES))}
PAIRS = [(name, shape) for name, (_, shapes) in STACK_CASES.items() for shape in shapes]


def test_argument_checks_come_in_the_documented_order():
    """The checks of tests/test_stack_host.py on the library the GPU tests run: no call reaches a launch."""
    from sunerf_hip import lib
    from test_stack_host import check_argument_order
    check_argument_order(lib.load())


@pytest.mark.parametrize('name,shape', PAIRS, ids=[f'{n[7:]}-{ac.shape_id(s)}' for n, s in PAIRS])
def test_stack_entry_point_stays_inside_its_buffers(name, shape):
    import test_gpu_abi_extents as extents
    extents.check_entry_point(STACK_CASES[name][0], name, shape)
