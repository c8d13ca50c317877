"""The launching entry point of include/sunerf_hip_psf_grad.h checks its arguments in the documented order and stays inside its
buffers: the checks of tests/test_gpu_abi_extents.py (runs A and B with sentinel and NaN fills, guards, inputs untouched, outputs
equal to the wrapper by bits and independent of what they and the workspace held, the empty call, the header's rejections) on
cases built with ``abi_cases.Ctx`` / ``Case`` and the guarded arena of tests/abi_arena.py, with the extents the header states:
``g_K`` at ``n_kernels kh kw`` doubles and the workspace at exactly ``sunerf_psf_grad_workspace_bytes``.

The cases live in this file's own table ``PSF_GRAD_CASES`` (tests/test_abi_tables_host.py holds it to the table's symbols)."""
import pytest

import abi_cases as ac
from abi_cases import F64, STREAM, Case, Ctx

pytestmark = pytest.mark.gpu

# (planes, height, width, n_kernels, kh, kw, bin, anchor_y, anchor_x, boundary): a kernel larger than the frame under both
# boundaries, the largest kernel at the largest bin (the tile shrinks to 4, nine chunks of taps, LDS reused for the slices' sums),
# the patch shape with a kernel per channel over three windows, and a batch whose runs span planes
SHAPES = [(1, 5, 7, 1, 9, 9, 1, 4, 4, 1), (1, 5, 7, 1, 9, 9, 1, 4, 4, 0), (1, 40, 40, 1, 96, 96, 8, 47, 50, 1),
          (21, 48, 48, 7, 18, 18, 2, 0, 0, 0), (1040, 4, 4, 1, 2, 2, 1, 0, 1, 1)]


def tap_gradient(shape, device):
    from sunerf_hip.psf_fit import tap_gradient as wrapper
    n, h, w, nk, kh, kw, b, ay, ax, boundary = shape
    c = Ctx(device)
    gen = ac._gen(100 * h + w + kh)
    oh, ow = h // b, w // b
    planes = ac._rand(gen, n, h, w) - 0.5
    cot = ac._rand(gen, n, oh, ow) - 0.5
    if (kh, b) == (18, 2):                        # the cotangent of a cropped patch
        cot[:, 16:, :] = 0.0
        cot[:, :, 16:] = 0.0
    inp, g_out = c.IN('in', planes), c.IN('g_out', cot)
    g_K = c.OUT('g_K', F64, nk * kh * kw)
    nbytes = int(ac._lib().sunerf_psf_grad_workspace_bytes(n, h, w, nk, kh, kw, b))
    assert nbytes > 0
    ws = c.WS('workspace', nbytes)

    def expected():
        return {'g_K': wrapper(inp.t.view(n, h, w), g_out.t.view(n, oh, ow), nk, kh, kw, b, ay, ax, 0.25, boundary)}
    args = [inp, g_out, n, h, w, nk, kh, kw, b, ay, ax, 0.25, boundary, g_K, ws, STREAM]
    return Case('sunerf_psf_grad_taps', shape, c.arena, args, expected, empty={2: 0},
                rejections=[({6: 97}, -2), ({7: 97}, -2), ({8: 9}, -2), ({12: 2}, -2), ({5: n + 1}, -1), ({5: 0}, -1), ({9: kh}, -1),
                            ({10: -1}, -1)])


PSF_GRAD_CASES = {'sunerf_psf_grad_taps': (tap_gradient, tuple(SHAPES))}
PAIRS = [(name, shape) for name, (_, shapes) in PSF_GRAD_CASES.items() for shape in shapes]


def test_argument_checks_come_in_the_documented_order():
    """The checks of tests/test_psf_fit_host.py on the library the GPU tests run: no call reaches a launch."""
    from sunerf_hip import lib
    from test_psf_fit_host import check_argument_order
    check_argument_order(lib.load())


@pytest.mark.parametrize('name,shape', PAIRS, ids=[f'{n[7:]}-{ac.shape_id(s)}' for n, s in PAIRS])
def test_psf_grad_entry_point_stays_inside_its_buffers(name, shape):
    import test_gpu_abi_extents as extents
    extents.check_entry_point(PSF_GRAD_CASES[name][0], name, shape)
