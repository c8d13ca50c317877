"""The launching entry point of include/sunerf_hip_ssim_loss.h checks its arguments in the documented order and stays inside its
buffers: the checks of tests/test_gpu_abi_extents.py (runs A and B with sentinel and NaN fills, guards, inputs untouched, outputs
equal to the wrapper by bits and independent of what they held, the workspace bound, the empty call, the header's rejections) on
cases built with ``abi_cases.Ctx`` / ``Case`` and the guarded arena of tests/abi_arena.py, with the extents the header states.

The cases live in this file's own table ``SSIM_LOSS_CASES`` (tests/test_abi_tables_host.py holds it to the table's symbols)."""
import pytest

import abi_cases as ac
import ssim_loss_reference as sr
from abi_cases import F32, F64, STREAM, Case, Ctx

pytestmark = pytest.mark.gpu

TILES = 'ssim_loss.hip: 256 threads, one workgroup per patch and group of channels; 4 fp64 partials per workgroup in the workspace'
# (patches, patch side, channels, window, stretch): the smallest call (one window of 3 x 3, one channel); 65 patches of seven
# channels kept as planes in LDS; and a patch side at which a workgroup takes one channel and stores its gradient directly
SHAPES = [(1, 3, 1, 3, 0), (65, 16, 7, 7, 0), (65, 16, 7, 7, 1), (2, 64, 3, 11, 1)]


def loss(shape, device):
    n, P, C, w, stretched = shape
    c = Ctx(device)
    data = dict(zip(('coarse', 'fine', 'target'), sr.make_case(n, P, C, 9)))
    coarse, fine, target = (c.IN(k, data[k]) for k in ('coarse', 'fine', 'target'))
    g_coarse, g_fine = c.OUT('g_coarse', F32, n * P * P * C), c.OUT('g_fine', F32, n * P * P * C)
    plane_ssim, stats = c.OUT('plane_ssim', F64, 2 * n * C), c.OUT('stats', F64, 4)
    nbytes = int(ac._lib().sunerf_ssim_loss_workspace_bytes(n, C))
    ws = c.WS('workspace', nbytes, init='zero')          # header: ZERO-INITIALISED once by the caller (never given a pattern)
    scaling = (1.0, 0.005) if stretched else None

    def expected():
        from sunerf_hip.ssim_loss import launch
        shape2 = (n * P * P, C)
        out = launch(coarse.t.view(shape2), fine.t.view(shape2), target.t.view(shape2), n, P, 1.0, w, scaling)
        return dict(zip(('g_coarse', 'g_fine', 'plane_ssim', 'stats'), out))
    args = [coarse, fine, target, n, P, C, w, 1.0, 1.0, 0.005, stretched, g_coarse, g_fine, plane_ssim, stats, ws, nbytes, STREAM]
    return Case('sunerf_ssim_loss', shape, c.arena, args, expected, ws_index=16, empty={3: 0},
                rejections=[({6: 4}, -2), ({6: 13}, -2), ({4: 65}, -2), ({4: w - 1}, -2), ({5: 65}, -2), ({7: 0.0}, -2), ({3: -1}, -1)])


SSIM_LOSS_CASES = {'sunerf_ssim_loss': (loss, tuple(SHAPES))}
PAIRS = [(name, shape) for name, (_, shapes) in SSIM_LOSS_CASES.items() for shape in shapes]


def test_argument_checks_come_in_the_documented_order():
    """The checks of tests/test_ssim_loss_host.py on the library the GPU tests run: no call reaches a launch."""
    from sunerf_hip import lib
    from test_ssim_loss_host import check_argument_order
    check_argument_order(lib.load())


@pytest.mark.parametrize('name,shape', PAIRS, ids=[f'{n[7:]}-{ac.shape_id(s)}' for n, s in PAIRS])
def test_ssim_loss_entry_point_stays_inside_its_buffers(name, shape):
    import test_gpu_abi_extents as extents
    extents.check_entry_point(SSIM_LOSS_CASES[name][0], name, shape)
