"""The launching entry point of include/sunerf_hip_noise_gate.h checks its arguments in the documented order and stays inside its
buffers: the checks of tests/test_gpu_abi_extents.py (runs A and B with sentinel and NaN fills, guards, inputs untouched, outputs
equal to the wrapper by bits and independent of what they held, the empty call, the header's rejections) on cases built with
``abi_cases.Ctx`` / ``Case`` and the guarded arena of tests/abi_arena.py, with the extents the header states: ``out`` at the size
of ``frames``, ``state`` at 4 int64 per plane, ``spectrum`` at ``n_planes bt 256`` floats or NULL; there is no workspace.

The cases live in this file's own table ``NOISE_GATE_CASES`` (tests/test_abi_tables_host.py holds it to the table's symbols)."""
import numpy as np
import pytest
import torch

import abi_cases as ac
from abi_arena import IN
from abi_cases import F32, I64, STREAM, Case, Ctx

pytestmark = pytest.mark.gpu

# (frames, planes, height, width, bt, mode, flags, with bad, with spectrum): one sample, one block, one past a block on every
# axis, axes shorter than a block, several planes -- every block length, both modes, with and without the optional inputs
SHAPES = [(1, 1, 1, 1, 1, 0, 0, 0, 0), (1, 1, 16, 16, 1, 1, 1, 1, 1), (16, 1, 16, 16, 16, 0, 0, 1, 0), (17, 1, 17, 17, 16, 1, 0, 0, 1),
          (5, 3, 3, 33, 4, 0, 1, 1, 1), (9, 2, 17, 5, 8, 1, 1, 1, 0), (2, 2, 4, 35, 1, 0, 0, 0, 1)]


def gate(shape, device):
    from sunerf_hip.noise_gate import launch
    from test_noise_gate_host import case_params, case_spectrum
    t, c_, h, w, bt, mode, flags, with_bad, with_spectrum = shape
    c = Ctx(device)
    rng = np.random.default_rng(t + 10 * w)
    planes = (2.0 + 2.0 * rng.standard_normal((t, c_, h, w))).astype(np.float32)
    flagged = np.zeros(planes.shape, dtype=np.uint8)
    if planes.size > 1:
        planes.reshape(-1)[::7] = np.nan
        planes.reshape(-1)[3::11] = np.inf
        flagged.reshape(-1)[::5] = 1
    frames = c.IN('frames', torch.from_numpy(planes))
    bad = c.IN('bad', torch.from_numpy(flagged)) if with_bad else c.NULL('bad', IN)
    params = c.IN('params', torch.from_numpy(np.ascontiguousarray(case_params(c_), dtype=np.float64)))
    spectrum = c.IN('spectrum', torch.from_numpy(case_spectrum(c_, bt))) if with_spectrum else c.NULL('spectrum', IN)
    out, state = c.OUT('out', F32, t * c_ * h * w), c.OUT('state', I64, 4 * c_)
    call = (bt, mode, flags, 2.5)

    def expected():
        image, st = launch(frames.t.view(t, c_, h, w), bad.t.view(t, c_, h, w) if with_bad else None, params.t.view(c_, 4),
                           spectrum.t.view(c_, bt, 16, 16) if with_spectrum else None, *call)
        return {'out': image, 'state': st}
    args = [frames, bad, params, spectrum, t, c_, h, w, *call, out, state, STREAM]
    return Case('sunerf_noise_gate', shape, c.arena, args, expected, empty={5: 0},
                rejections=[({8: 2}, -2), ({8: 32}, -2), ({9: 2}, -2), ({10: 2}, -2), ({8: 3, 5: 0}, -2), ({4: -1}, -1), ({5: -1}, -1),
                            ({7: -1}, -1), ({11: 0.0}, -1), ({11: float('nan')}, -1), ({11: float('inf')}, -1), ({12: frames}, -1),
                            ({12: params}, -1)]
                + ([({12: bad}, -1)] if with_bad else []) + ([({12: spectrum}, -1)] if with_spectrum else []))


NOISE_GATE_CASES = {'sunerf_noise_gate': (gate, tuple(SHAPES))}
PAIRS = [(name, shape) for name, (_, shapes) in NOISE_GATE_CASES.items() for shape in shapes]


def test_argument_checks_come_in_the_documented_order():
    """The checks of tests/test_noise_gate_host.py on the library the GPU tests run: no call reaches a launch."""
    from sunerf_hip import lib
    from test_noise_gate_host import check_argument_order
    check_argument_order(lib.load())


@pytest.mark.parametrize('name,shape', PAIRS, ids=[f'{n[7:]}-{ac.shape_id(s)}' for n, s in PAIRS])
def test_noise_gate_entry_point_stays_inside_its_buffers(name, shape):
    import test_gpu_abi_extents as extents
    extents.check_entry_point(NOISE_GATE_CASES[name][0], name, shape)
