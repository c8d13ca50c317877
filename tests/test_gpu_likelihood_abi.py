"""The launching entry point of include/sunerf_hip_likelihood.h checks its arguments in the documented order and stays inside its
buffers: the checks of tests/test_gpu_abi_extents.py (runs A and B with sentinel and NaN fills, guards, inputs untouched, outputs
equal to the wrapper by bits and independent of what they held, the workspace bound, the empty call, the header's rejections) on
cases built with ``abi_cases.Ctx`` / ``Case`` and the guarded arena of tests/abi_arena.py, with the extents the header states.

The cases live in this file's own table ``LIKELIHOOD_CASES`` (tests/test_abi_tables_host.py holds it to the table's symbols)."""
import ctypes

import pytest
import torch

import abi_cases as ac
import likelihood_reference as lr
from abi_arena import IN
from abi_cases import F32, F64, STREAM, Case, Ctx, HostPtrs, HostValue

pytestmark = pytest.mark.gpu

TILES = 'likelihood.hip: 256 threads x at most 128 workgroups stride over the slots; block partials of 5 rows + 3 words in the workspace'
# (rays, columns, rows, mode, with codes, with regularization and finite-check tensors): the smallest call, and one wave plus one
# ray of seven columns against the largest table
SHAPES = [(1, 1, 1, 0, 0, 0), (1, 1, 1, 1, 1, 1), (65, 7, 64, 0, 1, 0), (65, 7, 64, 1, 1, 1)]


def loss(shape, device):
    n, w, m, mode, with_codes, with_reg = shape
    c = Ctx(device)
    data = lr.make_case(n, w, m, 5, with_codes=True)
    coarse, fine, target = (c.IN(k, data[k[:-6]]) for k in ('coarse_image', 'fine_image', 'target_image'))
    codes = c.IN('codes', data['codes']) if with_codes else c.NULL('codes', IN)
    row_codes, noise, log_gain = c.IN('row_codes', data['row_codes']), c.IN('noise', data['noise']), c.IN('log_gain', data['log_gain'])
    n_reg = n * 3 if with_reg else 0
    reg = c.IN('regularization', data['reg']) if with_reg else c.NULL('regularization', IN)
    extra = [c.IN('finite_check0', torch.rand(n * 5)), c.IN('finite_check1', torch.rand(3))] if with_reg else []
    sizes = HostValue((ctypes.c_int64 * max(1, len(extra)))(*[b.numel for b in extra]))
    g_coarse, g_fine = c.OUT('g_coarse', F32, n * w), c.OUT('g_fine', F32, n * w)
    g_log_gain, channel_stats, stats = c.OUT('g_log_gain', F64, m), c.OUT('channel_stats', F64, m * 4), c.OUT('stats', F32, 8)
    nbytes = int(ac._lib().sunerf_likelihood_workspace_bytes(m))
    ws = c.WS('workspace', nbytes, init='zero')          # header: ZERO-INITIALISED once by the caller (never given a pattern)

    def expected():
        from sunerf_hip.likelihood import launch
        out = launch(coarse.t.view(n, w), fine.t.view(n, w), target.t.view(n, w), codes.t.view(n, w) if with_codes else None, row_codes.t,
                     noise.t.view(m, 8), log_gain.t, mode, reg.t if with_reg else None, [b.t for b in extra], 1.0, 0.5)
        return dict(zip(('g_coarse', 'g_fine', 'g_log_gain', 'channel_stats', 'stats'), out))
    args = [coarse, fine, target, codes, n, w, row_codes, noise, log_gain, m, mode, reg, n_reg, HostPtrs(extra), sizes, len(extra), 1.0, 0.5,
            g_coarse, g_fine, g_log_gain, channel_stats, stats, ws, nbytes, STREAM]
    return Case('sunerf_likelihood_loss', shape, c.arena, args, expected, ws_index=24, empty={4: 0},
                rejections=[({9: 65}, -2), ({10: 2}, -2), ({15: 9}, -2), ({9: 0}, -1), ({5: -1}, -1)])


LIKELIHOOD_CASES = {'sunerf_likelihood_loss': (loss, tuple(SHAPES))}
PAIRS = [(name, shape) for name, (_, shapes) in LIKELIHOOD_CASES.items() for shape in shapes]


def test_argument_checks_come_in_the_documented_order():
    """The checks of tests/test_likelihood_host.py on the library the GPU tests run: no call reaches a launch."""
    from sunerf_hip import lib
    from test_likelihood_host import check_argument_order
    check_argument_order(lib.load())


@pytest.mark.parametrize('name,shape', PAIRS, ids=[f'{n[7:]}-{ac.shape_id(s)}' for n, s in PAIRS])
def test_likelihood_entry_point_stays_inside_its_buffers(name, shape):
    import test_gpu_abi_extents as extents
    extents.check_entry_point(LIKELIHOOD_CASES[name][0], name, shape)
