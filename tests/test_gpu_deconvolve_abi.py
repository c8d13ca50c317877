"""The launching entry point of include/sunerf_hip_deconvolve.h checks its arguments in the documented order and stays inside its
buffers: the checks of tests/test_gpu_abi_extents.py (runs A and B with sentinel and NaN fills, guards, inputs untouched, outputs
equal to the wrapper by bits and independent of what they and the workspace held, the empty call, the header's rejections) on
cases built with ``abi_cases.Ctx`` / ``Case`` and the guarded arena of tests/abi_arena.py, with the extents the header states:
``u`` (in and out), ``ratio``, ``state``, and the workspace at exactly ``sunerf_deconvolve_workspace_bytes``.

The cases live in this file's own table ``DECONVOLVE_CASES`` (tests/test_abi_tables_host.py holds it to the table's symbols)."""
import pytest
import torch

import abi_cases as ac
from abi_arena import IN
from abi_cases import F32, F64, STREAM, U8, Case, Ctx

pytestmark = pytest.mark.gpu

TILES = ('deconvolve.hip: ratio tiles of T x T detector pixels, T = min(32, (127 - max(kh, kw)) / bin + 1), one fp64 pair per tile in '
         'the workspace; update tiles of 32 x 32 input pixels; 256 threads')
# (planes, height, width, psf rows, psf columns, bin, per-plane kernels, boundary, iterations, with bad, stop): a kernel larger than
# the image, a single pixel, one tile plus one / two tiles plus one, a ragged batch with per-plane kernels under the stopping rule,
# exactly one tile and no update, a binned ragged frame, the largest kernel
SHAPES = [(1, 5, 7, 9, 9, 1, 0, 0, 2, 1, 0.0), (1, 1, 1, 3, 3, 1, 0, 1, 1, 0, 0.0), (1, 33, 65, 5, 5, 1, 0, 1, 2, 1, 0.0),
          (3, 34, 67, 5, 5, 1, 1, 0, 4, 1, 27.0), (1, 32, 32, 3, 3, 2, 0, 1, 0, 1, 0.0), (2, 37, 53, 7, 5, 3, 1, 1, 2, 0, 0.0),
          (1, 40, 48, 89, 89, 8, 0, 1, 1, 1, 0.0)]


def richardson_lucy(shape, device):
    from sunerf_hip.deconvolve import launch
    from sunerf_hip.instrument import Instrument, correlate_bin_adjoint
    c_, h, w, kh, kw, b, per_plane, boundary, n_it, with_bad, stop = shape
    c = Ctx(device)
    gen = ac._gen(100 * h + w + kh)
    oh, ow = h // b, w // b
    psf = (ac._rand(gen, c_ if per_plane else 1, kh, kw).double() + 0.01).numpy()
    inst = Instrument(psf=psf if per_plane else psf[0], bin=b, boundary=('zero', 'nearest')[boundary])
    K, (ay, ax) = inst.effective_kernel()
    K = K / K.sum(axis=(1, 2), keepdims=True)
    start = ac._rand(gen, c_, h, w) + 0.1
    data = ac._rand(gen, c_, oh, ow) * 2.0 - 0.05            # a few negatives
    if oh * ow > 2:
        data.view(-1)[1] = float('nan')
    mask = torch.zeros(c_, oh, ow, dtype=U8)
    mask.view(-1)[-1] = 1
    valid = torch.isfinite(data) & ((mask == 0) if with_bad else torch.ones_like(mask, dtype=torch.bool))
    u = c.INOUT('u', start)
    d = c.IN('d', data)
    bad = c.IN('bad', mask) if with_bad else c.NULL('bad', IN)
    taps = c.IN('K', torch.from_numpy(K))
    params = c.IN('params', torch.tensor([[50.0 + 25.0 * p, 1.0] for p in range(c_)], dtype=F64))
    call = (K.shape[0], K.shape[1], K.shape[2], b, ay, ax, inst.scale, boundary)
    norm = c.IN('norm', correlate_bin_adjoint(valid.to(F32).to(device), h, w, taps.t.view(K.shape), *call).cpu())
    ratio, state = c.OUT('ratio', F32, c_ * oh * ow), c.OUT('state', F64, 4 * c_)
    nbytes = int(ac._lib().sunerf_deconvolve_workspace_bytes(c_, h, w, K.shape[1], K.shape[2], b))
    ws = c.WS('workspace', nbytes)

    def expected():
        out = start.to(device).contiguous()                   # u holds the result of the run before: the wrapper starts from the same start
        st, r = launch(out, d.t.view(c_, oh, ow), bad.t.view(c_, oh, ow) if with_bad else None, norm.t.view(c_, h, w), params.t.view(c_, 2),
                       taps.t.view(K.shape), *call, n_it, stop)
        return {'u': out, 'ratio': r, 'state': st}
    args = [u, d, bad, norm, params, c_, h, w, taps, *call[:6], float(call[6]), call[7], n_it, stop, ratio, state, ws, STREAM]
    return Case('sunerf_deconvolve_richardson_lucy', shape, c.arena, args, expected, empty={5: 0},
                rejections=[({10: 97}, -2), ({11: 97}, -2), ({12: 9}, -2), ({16: 2}, -2), ({17: -1}, -1), ({17: 10001}, -1),
                            ({18: -1.0}, -1), ({18: float('nan')}, -1), ({9: c_ + 1}, -1)])


DECONVOLVE_CASES = {'sunerf_deconvolve_richardson_lucy': (richardson_lucy, tuple(SHAPES))}
PAIRS = [(name, shape) for name, (_, shapes) in DECONVOLVE_CASES.items() for shape in shapes]


def test_argument_checks_come_in_the_documented_order():
    """The checks of tests/test_deconvolve_host.py on the library the GPU tests run: no call reaches a launch."""
    from sunerf_hip import lib
    from test_deconvolve_host import check_argument_order
    check_argument_order(lib.load())


def test_the_stopping_rule_of_the_ragged_batch_stops_some_planes_only():
    """The case with a threshold is there to run the skipped workgroups of all three kernels inside guarded buffers: it must
    stop at least one plane before the count runs out and leave at least one running."""
    dev = torch.device('cuda', torch.cuda.current_device())
    case = richardson_lucy(SHAPES[3], dev)
    state = case.expected()['state'].cpu().numpy()
    print('iterations', state[:, 2].tolist(), 'stopped', state[:, 3].tolist(), 'deviance per valid pixel', (state[:, 0] / state[:, 1]).tolist())
    assert 0 < state[:, 3].sum() < state.shape[0] and state[:, 2].min() < SHAPES[3][8]


@pytest.mark.parametrize('name,shape', PAIRS, ids=[f'{n[7:]}-{ac.shape_id(s)}' for n, s in PAIRS])
def test_deconvolve_entry_point_stays_inside_its_buffers(name, shape):
    import test_gpu_abi_extents as extents
    extents.check_entry_point(DECONVOLVE_CASES[name][0], name, shape)
