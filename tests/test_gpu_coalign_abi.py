"""The launching entry point of include/sunerf_hip_coalign.h checks its arguments in the documented order and stays inside its
buffers: the checks of tests/test_gpu_abi_extents.py (runs A and B with sentinel and NaN fills, guards, inputs untouched, outputs
equal to the wrapper by bits and independent of what they and the workspace held, the empty call, the header's rejections) on
cases built with ``abi_cases.Ctx`` / ``Case`` and the guarded arena of tests/abi_arena.py, with the extents the header states:
``sums`` at ``n_planes (2 max_dy + 1) (2 max_dx + 1) 6`` doubles and the workspace at exactly ``sunerf_coalign_workspace_bytes``.

The cases live in this file's own table ``COALIGN_CASES`` (tests/test_abi_tables_host.py holds it to the table's symbols)."""
import pytest
import torch

import abi_cases as ac
from abi_arena import IN
from abi_cases import F64, STREAM, U8, Case, Ctx

pytestmark = pytest.mark.gpu

# (planes, height, width, max_dy, max_dx, with masks): a single pixel inside a window, a window larger than the frame, one pixel
# past a tile in each axis with an asymmetric window, two chunks of shifts (LDS reused for the slices' sums), the limit of 4225
# shifts with the window above 64 KiB of LDS, runs of several tiles, more planes than runs -- each with NULL masks or with both
SHAPES = [(1, 1, 1, 2, 3, 0), (1, 5, 7, 8, 8, 1), (2, 33, 65, 2, 5, 0), (2, 33, 65, 2, 5, 1), (2, 65, 97, 16, 16, 1),
          (1, 40, 70, 32, 32, 0), (16, 96, 192, 2, 2, 1), (300, 3, 5, 0, 1, 0)]


def shift_sums(shape, device):
    from sunerf_hip.coalign import launch
    n, h, w, my, mx, with_masks = shape
    c = Ctx(device)
    gen = ac._gen(100 * h + w + my)
    planes, tpl = ac._rand(gen, n, h, w) - 0.5, ac._rand(gen, n, h, w) - 0.5
    planes.view(-1)[::11] = float('nan')
    tpl.view(-1)[::13] = float('inf')
    image, templ = c.IN('image', planes), c.IN('templ', tpl)
    if with_masks:
        mask_i, mask_t = torch.zeros(n, h, w, dtype=U8), torch.zeros(n, h, w, dtype=U8)
        mask_i.view(-1)[::7] = 1
        mask_t.view(-1)[::5] = 200
        bad_i, bad_t = c.IN('bad_image', mask_i), c.IN('bad_template', mask_t)
    else:
        bad_i, bad_t = c.NULL('bad_image', IN), c.NULL('bad_template', IN)
    sy, sx = 2 * my + 1, 2 * mx + 1
    sums = c.OUT('sums', F64, n * sy * sx * 6)
    nbytes = int(ac._lib().sunerf_coalign_workspace_bytes(n, h, w, my, mx))
    tiles = -(-h // 32) * -(-w // 32)
    assert nbytes == n * min(tiles, max(1, 256 // n)) * sy * sx * 48
    ws = c.WS('workspace', nbytes)

    def expected():
        masks = (bad_i.t.view(n, h, w), bad_t.t.view(n, h, w)) if with_masks else (None, None)
        return {'sums': launch(image.t.view(n, h, w), templ.t.view(n, h, w), *masks, my, mx)}
    args = [image, templ, bad_i, bad_t, n, h, w, my, mx, sums, ws, STREAM]
    return Case('sunerf_coalign_shift_sums', shape, c.arena, args, expected, empty={4: 0},
                rejections=[({7: 33}, -2), ({8: 33}, -2), ({7: 33, 4: 0}, -2), ({4: -1}, -1), ({5: -1}, -1), ({7: -1}, -1), ({8: -1}, -1),
                            ({9: image}, -1), ({9: templ}, -1)])


COALIGN_CASES = {'sunerf_coalign_shift_sums': (shift_sums, tuple(SHAPES))}
PAIRS = [(name, shape) for name, (_, shapes) in COALIGN_CASES.items() for shape in shapes]


def test_argument_checks_come_in_the_documented_order():
    """The checks of tests/test_coalign_host.py on the library the GPU tests run: no call reaches a launch."""
    from sunerf_hip import lib
    from test_coalign_host import check_argument_order
    check_argument_order(lib.load())


@pytest.mark.parametrize('name,shape', PAIRS, ids=[f'{n[7:]}-{ac.shape_id(s)}' for n, s in PAIRS])
def test_coalign_entry_point_stays_inside_its_buffers(name, shape):
    import test_gpu_abi_extents as extents
    extents.check_entry_point(COALIGN_CASES[name][0], name, shape)
