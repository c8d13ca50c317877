"""The launching entry point of include/sunerf_hip_despike.h checks its arguments in the documented order and stays inside its
buffers: the checks of tests/test_gpu_abi_extents.py (runs A and B with sentinel and NaN fills, guards, inputs untouched, outputs
equal to the wrapper by bits and independent of what they and the workspace held, the empty call, the header's rejections) on
cases built with ``abi_cases.Ctx`` / ``Case`` and the guarded arena of tests/abi_arena.py, with the extents the header states:
``clean`` and ``mask`` at the image's shape, ``state`` at 6 doubles per plane, and the workspace at exactly
``sunerf_despike_workspace_bytes``.

The cases live in this file's own table ``DESPIKE_CASES`` (tests/test_abi_tables_host.py holds it to the table's symbols)."""
import numpy as np
import pytest
import torch

import abi_cases as ac
from abi_arena import IN
from abi_cases import F32, F64, STREAM, U8, Case, Ctx

pytestmark = pytest.mark.gpu

TILES = 'despike.hip: tiles of 8 x 32 pixels, one per thread of 256, a halo of `radius` on every side; the start kernel: 1024 pixels per workgroup'
# (planes, height, width, radius, mode, flags, passes, with bad): a frame smaller than the window, a single pixel, a single row,
# one pixel past the tile in each axis, two tiles plus one with an odd number of passes (the buffers swap roles), the fill alone,
# and the planes that stop at different passes (a stopped plane's workgroups return at once) -- with an even and an odd count
SHAPES = [(1, 5, 7, 3, 0, 0, 4, 1), (1, 1, 1, 1, 0, 0, 1, 0), (1, 1, 40, 2, 1, 0, 3, 0), (3, 9, 33, 2, 0, 0, 4, 1),
          (2, 17, 65, 3, 1, 1, 5, 1), (2, 16, 64, 1, 0, 2, 0, 1), (3, 19, 70, 2, 0, 0, 4, 0), (3, 19, 70, 3, 1, 3, 7, 0)]


def despike(shape, device):
    from sunerf_hip.despike import launch
    from test_gpu_despike import make_planes, params_of, stopping_planes
    c_, h, w, radius, mode, flags, passes, with_bad = shape
    c = Ctx(device)
    if (h, w) == (19, 70):
        planes, p = stopping_planes()
    else:
        planes, p = make_planes(c_, h, w, 100 * h + w), params_of(c_)
    mask_in = torch.zeros(c_, h, w, dtype=U8)
    mask_in.view(-1)[::7] = 1
    image = c.IN('image', torch.from_numpy(planes))
    bad = c.IN('bad', mask_in) if with_bad else c.NULL('bad', IN)
    params = c.IN('params', torch.from_numpy(np.ascontiguousarray(p, dtype=np.float64)))
    clean, mask, state = c.OUT('clean', F32, c_ * h * w), c.OUT('mask', U8, c_ * h * w), c.OUT('state', F64, 6 * c_)
    nbytes = int(ac._lib().sunerf_despike_workspace_bytes(c_, h, w, radius))
    assert nbytes == (c_ * h * w + 7) // 8 * 8 + c_ * 66 * 4
    ws = c.WS('workspace', nbytes)
    call = (radius, mode, flags, 5.0, 3.0, 2, passes)

    def expected():
        out, m, st = launch(image.t.view(c_, h, w), bad.t.view(c_, h, w) if with_bad else None, params.t.view(c_, 4), *call)
        return {'clean': out, 'mask': m, 'state': st}
    args = [image, bad, params, c_, h, w, *call, clean, mask, state, ws, STREAM]
    return Case('sunerf_despike', shape, c.arena, args, expected, empty={3: 0},
                rejections=[({6: 4}, -2), ({12: 65}, -2), ({11: 49}, -2), ({7: 2}, -2), ({8: 4}, -2), ({6: 0}, -1), ({11: 0}, -1),
                            ({12: -1}, -1), ({9: 0.0}, -1), ({10: float('nan')}, -1), ({4: -1}, -1), ({13: image}, -1)])


DESPIKE_CASES = {'sunerf_despike': (despike, tuple(SHAPES))}
PAIRS = [(name, shape) for name, (_, shapes) in DESPIKE_CASES.items() for shape in shapes]


def test_argument_checks_come_in_the_documented_order():
    """The checks of tests/test_despike_host.py on the library the GPU tests run: no call reaches a launch."""
    from sunerf_hip import lib
    from test_despike_host import check_argument_order
    check_argument_order(lib.load())


def test_the_planes_of_the_stopping_cases_stop_at_different_passes():
    """The two cases of 3 x 19 x 70 are there to run the returned workgroups of a stopped plane inside guarded buffers: a plane
    must stop before the passes run out and another must use them all."""
    dev = torch.device('cuda', torch.cuda.current_device())
    for shape in SHAPES[-2:]:
        state = despike(shape, dev).expected()['state'].cpu().numpy()
        print(shape, 'passes', state[:, 3].tolist(), 'converged', state[:, 4].tolist())
        assert state[:, 3].min() == 0 and state[:, 3].max() == shape[6] and state[:, 4].tolist() == [1.0, 1.0, 0.0]


@pytest.mark.parametrize('name,shape', PAIRS, ids=[f'{n[7:]}-{ac.shape_id(s)}' for n, s in PAIRS])
def test_despike_entry_point_stays_inside_its_buffers(name, shape):
    import test_gpu_abi_extents as extents
    extents.check_entry_point(DESPIKE_CASES[name][0], name, shape)
